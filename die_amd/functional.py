"""Differentiable device ops over libdie_hip.so's layer kernels, for callers that hold plain tensors.

    conv2d_wide(input, weight, *, activation=None, padding_mode='circular', dropout=None)
        one wide NeuralAutomataAgent layer, act(conv(input, weight)) (* the counter-based dropout mask): die_conv2d_wide forward,
        die_conv2d_wide_backward (die_nca_wide_grad.hip: both adjoint GEMMs on the fp32 matrix instruction) backward.
    gather_scale(sense, obs, coefs)
        the per-agent read-out of a (3, W, H) sense tensor, NeuralAutomataAgent.differentiable_action's last step.

    gather_scale_batch(sense, population)
        the same read-out for every replica of a BatchedNeuralAutomataAgent's worlds: (R, 3, W, H) -> (3, R, Nmax).

`ConvolutionModel.forward_device` evaluates a whole wide stack through `conv2d_wide`; `BatchedNeuralAutomataAgent.forward_device`
a population of them in one launch per layer (die_nca_wide_backward_batch backward).  There is no eager fallback: a shape the
kernels do not take raises."""
import ctypes as C
from typing import Optional, Sequence, Tuple

import torch as th

from . import _lib
from .device_array import _ptr, stream_ptr

_ADJOINT_PADS = ('circular', 'zeros')


def _planes_of(t: th.Tensor):
    n, cells = t.shape[0], t.shape[1] * t.shape[2]
    return (_lib.ConvPlane * n)(*[_lib.ConvPlane(t.data_ptr() + 4 * c * cells, _lib.DIE_PLANE_F32, 0) for c in range(n)])


def _launch_forward(input, weight, act, pad, drop):
    """One die_conv2d_wide into storage of its own: (cout, W, H)."""
    cout, cin, k, _ = weight.shape
    _, W, H = input.shape
    out = th.empty((cout, W, H), dtype=th.float32, device=input.device)
    _lib.check(_lib.lib.die_conv2d_wide(W, H, cin, _planes_of(input), 0, cout, _ptr(out), W * H, k, _ptr(weight), act, pad,
                                        None if drop is None else C.byref(drop), stream_ptr(input.device)), 'die_conv2d_wide')
    return out


def _launch_backward(input, weight, grad, fwd_out, act, pad, drop, want_grad_in: bool):
    """One die_conv2d_wide_backward: (grad_weight, grad_input or None).  `want_grad_in` False passes a NULL grad_in: the
    input-gradient kernel is not launched."""
    cout, cin, k, _ = weight.shape
    _, W, H = input.shape
    need = _lib.lib.die_conv2d_wide_backward_workspace_bytes(W, H, cin, cout, k)
    if need < 0:
        raise ValueError(f'a layer shape die_conv2d_wide_backward does not take ({cin} -> {cout} channels, kernel size {k}: 1..'
                         f'{_lib.NCA_WIDE_MAX_CHANNELS} channels, kernel size in {_lib.NCA_WIDE_KERNEL_SIZES})')
    dev = input.device
    ws = th.empty((need // 4,), dtype=th.float32, device=dev)
    grad_w = th.empty_like(weight)
    grad_in = th.empty_like(input) if want_grad_in else None
    _lib.check(_lib.lib.die_conv2d_wide_backward(W, H, cin, _planes_of(input), 0, cout, _ptr(grad), W * H, _ptr(fwd_out), W * H, k,
                                                 _ptr(weight), act, pad, None if drop is None else C.byref(drop), _ptr(grad_w),
                                                 _ptr(grad_in), W * H, _ptr(ws), need, stream_ptr(dev)), 'die_conv2d_wide_backward')
    return grad_w, grad_in


class _Conv2dWide(th.autograd.Function):
    """conv2d_wide: the forward is die_conv2d_wide into storage the graph owns — with a mask the layer is launched masked (the
    value returned) and unmasked (act(z), kept for the backward, which recomputes the mask from its key), as
    NeuralAutomataAgent.differentiable_sense does — the backward one die_conv2d_wide_backward."""

    @staticmethod
    def forward(ctx, input, weight, act, pad, dropout, needs_grad):
        drop = None if dropout is None else _lib.nca_dropout(dropout[0], dropout[1], 0, dropout[2])
        out = _launch_forward(input, weight, act, pad, drop)
        if needs_grad:
            # what the backward reads of the forward: act(z) unmasked; nothing where neither an activation nor a mask was applied
            fwd_out = None if act == _lib.NCA_ACTIVATIONS[None] and drop is None else \
                out if drop is None else _launch_forward(input, weight, act, pad, None)
            ctx.act, ctx.pad, ctx.dropout, ctx.has_fwd = act, pad, dropout, fwd_out is not None
            ctx.save_for_backward(input, weight, *(() if fwd_out is None else (fwd_out,)))
        return out

    @staticmethod
    @th.autograd.function.once_differentiable
    def backward(ctx, grad):
        input, weight = ctx.saved_tensors[:2]
        fwd_out = ctx.saved_tensors[2] if ctx.has_fwd else None
        drop = None if ctx.dropout is None else _lib.nca_dropout(ctx.dropout[0], ctx.dropout[1], 0, ctx.dropout[2])
        grad_w, grad_in = _launch_backward(input, weight, grad.to(dtype=th.float32).contiguous(), fwd_out, ctx.act, ctx.pad, drop,
                                           ctx.needs_input_grad[0])
        return grad_in, grad_w, None, None, None, None


def conv2d_wide(input: th.Tensor, weight: th.Tensor, *, activation: Optional[str] = None, padding_mode: str = 'circular',
                dropout: Optional[Tuple[float, int, int]] = None) -> th.Tensor:
    """One wide layer on the device: `input` (cin, W, H) and `weight` (cout, cin, k, k), float32 CUDA tensors with 1..32 channels
    and k in (1, 3, 5) -> act(conv(input, weight)) as a (cout, W, H) tensor with a `grad_fn`, bit for bit die_conv2d_wide's values.
    `activation`: None, 'tanh' or 'relu'; `padding_mode`: torch.nn.Conv2d's; `dropout`: None or (p, seed, step), the counter-based
    inverted-dropout mask over cells of include/die_hip.h (die_nca_dropout), applied after the activation.

    Gradients flow to `weight` and, where `input` needs one, to `input` (otherwise the input-gradient kernel is not launched).
    The adjoint exists for 'circular' and 'zeros': 'reflect' / 'replicate' raise NotImplementedError before any launch when a
    gradient is needed, and still compute the forward otherwise (e.g. under `torch.no_grad()`)."""
    if activation not in _lib.NCA_ACTIVATIONS:
        raise ValueError(f"activation={activation!r}: None, 'tanh' or 'relu'")
    if padding_mode not in _lib.PAD_MODES:
        raise ValueError(f'padding_mode={padding_mode!r}: one of {sorted(_lib.PAD_MODES)}')
    for name, t, nd in (('input', input, 3), ('weight', weight, 4)):
        if not isinstance(t, th.Tensor) or t.dim() != nd or t.dtype != th.float32 or not t.is_cuda:
            raise ValueError(f'{name}: a float32 CUDA tensor of {nd} dimensions')
    if weight.device != input.device or weight.shape[1] != input.shape[0] or weight.shape[2] != weight.shape[3]:
        raise ValueError(f'weight {tuple(weight.shape)} does not fit input {tuple(input.shape)} (or lives on another device)')
    if dropout is not None:
        p, seed, step = dropout
        dropout = None if float(p) == 0.0 else (float(p), int(seed), int(step))
    needs_grad = th.is_grad_enabled() and (input.requires_grad or weight.requires_grad)
    if needs_grad and padding_mode not in _ADJOINT_PADS:
        raise NotImplementedError(f"padding_mode={padding_mode!r} with a gradient: the adjoint kernels take 'circular' and 'zeros' "
                                  '(the forward alone, e.g. under torch.no_grad(), takes every mode)')
    return _Conv2dWide.apply(input.contiguous(), weight.contiguous(), _lib.NCA_ACTIVATIONS[activation], _lib.PAD_MODES[padding_mode],
                             dropout, needs_grad)


def gather_scale(sense: th.Tensor, obs, coefs: Sequence[float]) -> th.Tensor:
    """The read-out of a (3, W, H) float32 `sense` tensor at every agent slot of `obs` = (agents, medium): (3, N) rows dx, dy,
    deposit, action[c, n] = sense[c, cell of slot n] * coefs[c] (die_gather_scale), with a `grad_fn` whose backward scatters the
    slots' gradients onto their cells (die_gather_scale_backward)."""
    from .agent.evo import _DifferentiableReadOut
    agents, medium = obs
    return _DifferentiableReadOut.apply(sense, agents, medium, tuple(float(c) for c in coefs))


def gather_scale_batch(sense: th.Tensor, population) -> th.Tensor:
    """The read-out of an (R, 3, W, H) float32 `sense` tensor (`BatchedNeuralAutomataAgent.forward_device` or
    `differentiable_sense`) at every agent slot of the population's worlds as they stand now: (3, R, Nmax) float32 in the batch's
    action layout (what `env.step(..., action=...)` and `env.differentiable_step` take), action[c, r, n] = sense[r, c, cell of
    replica r's slot n] * action_coefs[c] (die_gather_scale_batch); the padding slots from n[r] on are 0 and receive no gradient.
    The backward scatters the slots' gradients onto their cells (die_gather_scale_backward_batch: fp32 atomics in arrival order
    where several slots of a replica with a non-zero gradient share a cell — alive agents never do).  The slots' coordinates are
    copied, so `backward` may run after the worlds have been stepped.  The node does not care what produced `sense`: narrow and
    wide stacks alike."""
    from .batch import BatchedNeuralAutomataAgent, _BatchedReadOut
    if not isinstance(population, BatchedNeuralAutomataAgent):
        raise TypeError('population: a BatchedNeuralAutomataAgent')
    env = population.env
    if env.per_replica:
        raise NotImplementedError('gather_scale_batch: large worlds (per_replica) are not batched')
    if not isinstance(sense, th.Tensor) or sense.dtype != th.float32 or not sense.is_cuda or tuple(sense.shape) != (env.R, 3, env.W, env.H):
        raise ValueError(f'sense: a float32 CUDA tensor of shape {(env.R, 3, env.W, env.H)}')
    return _BatchedReadOut.apply(sense, population)
