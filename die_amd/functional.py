"""Differentiable device ops over libdie_hip.so's layer kernels, for callers that hold plain tensors.

    conv2d_wide(input, weight, *, activation=None, padding_mode='circular', dropout=None)
        one wide NeuralAutomataAgent layer, act(conv(input, weight)) (* the counter-based dropout mask): die_conv2d_wide forward,
        die_conv2d_wide_backward (die_nca_wide_grad.hip: both adjoint GEMMs on the fp32 matrix instruction) backward.
    gather_scale(sense, obs, coefs)
        the per-agent read-out of a (3, W, H) sense tensor, NeuralAutomataAgent.differentiable_action's last step.

    gather_scale_batch(sense, population)
        the same read-out for every replica of a BatchedNeuralAutomataAgent's worlds: (R, 3, W, H) -> (3, R, Nmax).
    memory_record(obs, standing=None), memory_planes(memory, record), gather_memory(sense_tail, record)
        the memory channels of a stand-alone NeuralAutomataAgent (die_memory_grad.hip): where every slot stands (die_memory_cells),
        the expand (M, N) -> (M, W, H) and the read-out (M, W, H) -> (M, N), each with a `grad_fn` that keeps the record
        (die_memory_planes_backward, die_gather_memory_backward).  NeuralAutomataAgent.recurrent_action composes them.
    signal_record(obs, standing=None), signal_step(field, emission, record, *, deposit, sigma, decay)
        the signal channels of a stand-alone NeuralAutomataAgent (die_signal_grad.hip): which cells are stood on (die_signal_cells,
        a byte plane) and the field's update (K, W, H) -> (K, W, H) with a `grad_fn` that keeps the record (die_signal_step forward,
        one die_signal_step_backward launch backward).  NeuralAutomataAgent.signalling_action composes them.
    memory_record_batch(population), memory_planes_batch(memory, record), gather_memory_batch(sense_tail, record)
        the same three for every replica of a BatchedNeuralAutomataAgent's worlds, one launch each (die_memory_cells_batch,
        die_memory_planes_backward_batch, die_gather_memory_backward_batch): (R, Nmax) records, (R, M, Nmax) memories, the expand
        as (M, R, W, H) planes.  BatchedNeuralAutomataAgent.recurrent_action composes them.
    signal_record_batch(population, standing=None), signal_step_batch(field, emission, record, *, deposit, sigma, decay)
        the signal channels of every replica, one launch each (die_signal_cells_batch; die_signal_step_batch forward, ONE
        die_signal_step_backward_batch backward): (R, W, H) byte planes, (R, K, W, H) fields of any strides.
        BatchedNeuralAutomataAgent.signalling_action composes them with the three above.

    inherit_memory(memory, record, mode, mutation=0.0), inherit_memory_batch(memory, record, mode, mutation=0.0)
        heredity (die_heredity.hip): what the newborns of one birth pass — `record`, a BirthsRecord from `Env.births_record()` /
        `BatchedEnv.births_record()` — hold in their memory channels, (M, N) -> (M, N) or (R, M, Nmax) -> (R, M, Nmax), with a
        `grad_fn` that keeps the record (die_memory_inherit on a clone forward, die_memory_inherit_backward backward).
        `NeuralAutomataAgent.inherit_memory` / `BatchedNeuralAutomataAgent.inherit_memory` call them.

`ConvolutionModel.forward_device` evaluates a whole wide stack through `conv2d_wide`; `BatchedNeuralAutomataAgent.forward_device`
a population of them in one launch per layer (die_nca_wide_backward_batch backward).  There is no eager fallback: a shape the
kernels do not take raises."""
import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
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


class MemoryRecord:
    """Where every slot stood at one forward (die_memory_cells), by SLOT ID: `cell` (N,) int32, the slot's cell `ix * H + iy` or
    -1 for a dead slot, and `win` (N,) int32, that cell where the slot is the one the standing plane names there (the highest
    alive slot id of the cell), else -1; and the sizes `W`, `H`, `N`.  Both adjoints are driven by these two arrays alone, so a
    graph that keeps the record survives every step, re-sort and reset of the world.  The record also remembers the standing
    plane and epoch it was taken from, for `memory_planes`' forward only: expand before that plane is built again."""
    __slots__ = ('cell', 'win', 'W', 'H', 'N', '_standing', '_epoch')

    def __init__(self, cell, win, W, H, N, standing, epoch):
        self.cell, self.win, self.W, self.H, self.N, self._standing, self._epoch = cell, win, int(W), int(H), int(N), standing, int(epoch)


def _bare_medium(W, H, epoch):
    return _lib.Medium(W, H, _lib.DIE_F32, epoch, None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, None)     # (W, H, gW are read)


def _check_standing(standing, shape: tuple, device) -> None:
    """A `standing` argument of the four record functions: the planes as die_stock_plane(_batch) leaves them."""
    if not isinstance(standing, th.Tensor) or standing.dtype != th.int64 or tuple(standing.shape) != shape or \
            standing.device != device or not standing.is_contiguous():
        raise ValueError(f'standing: a contiguous {shape} int64 tensor on {device}')


def memory_record(obs, standing: Optional[th.Tensor] = None) -> MemoryRecord:
    """The record of `obs` = (agents, medium) as they stand now: one die_memory_cells launch.  `standing`: the (W, H) int64
    standing plane built for these agents at `medium.epoch` (die_stock_plane; NeuralAutomataAgent builds one per forward), or
    None to build one here (a plane of its own, one launch more)."""
    agents, medium = obs
    dev, W, H, N = medium.device, medium.W, medium.H, agents.N
    if N < 1:
        raise ValueError('memory_record: the agents have no slot')
    m, a = medium.c_struct(need_owner=False), agents.c_struct()
    sp = stream_ptr(dev)
    if standing is None:
        standing = th.zeros((W, H), dtype=th.int64, device=dev)
        _lib.check(_lib.lib.die_stock_plane(C.byref(m), C.byref(a), medium.epoch, _ptr(standing), sp), 'die_stock_plane')
    else:
        _check_standing(standing, (W, H), dev)
    cell = th.full((N,), -1, dtype=th.int32, device=dev)
    win = th.full((N,), -1, dtype=th.int32, device=dev)
    _lib.check(_lib.lib.die_memory_cells(C.byref(m), C.byref(a), _ptr(standing), medium.epoch, _ptr(cell), _ptr(win), sp), 'die_memory_cells')
    return MemoryRecord(cell, win, W, H, N, standing, medium.epoch)


def _index_gather(W, H, index, planes, N):
    """die_memory_planes_backward as the index-only gather it is: (M, W, H) planes -> (M, N) rows, row[j][id] = planes[j][index[id]],
    +0 where the index is negative, the values moved as 32-bit words."""
    M = planes.shape[0]
    out = th.empty((M, N), dtype=th.float32, device=planes.device)
    _lib.check(_lib.lib.die_memory_planes_backward(W, H, M, N, _ptr(index), _ptr(planes), W * H, _ptr(out), N, stream_ptr(planes.device)),
               'die_memory_planes_backward')
    return out


def _check_memory_op(name, t, record, tail):
    """`t` must be a float32 (M, *tail(record)) tensor on the record's device, 1 <= M <= 8."""
    if not isinstance(record, MemoryRecord):
        raise TypeError('record: a MemoryRecord (die_amd.functional.memory_record)')
    shape = tail(record)
    if not isinstance(t, th.Tensor) or t.dtype != th.float32 or t.dim() != 1 + len(shape) or tuple(t.shape[1:]) != shape or \
            not 1 <= t.shape[0] <= _lib.MEMORY_MAX_CHANNELS or t.device != record.cell.device:
        raise ValueError(f'{name}: a float32 tensor of shape (M, {", ".join(str(s) for s in shape)}) with M in 1..'
                         f'{_lib.MEMORY_MAX_CHANNELS} on {record.cell.device}')


class _MemoryPlanes(th.autograd.Function):
    """memory_planes: die_memory_planes forward into storage the graph owns, die_memory_planes_backward backward."""

    @staticmethod
    def forward(ctx, memory, record):
        W, H, N, M = record.W, record.H, record.N, memory.shape[0]
        planes = th.empty((M, W, H), dtype=th.float32, device=memory.device)
        m = _bare_medium(W, H, record._epoch)
        _lib.check(_lib.lib.die_memory_planes(C.byref(m), _ptr(record._standing), record._epoch, M, _ptr(memory), N, N, _ptr(planes), W * H,
                                              stream_ptr(memory.device)), 'die_memory_planes')
        ctx.record = record
        return planes

    @staticmethod
    @th.autograd.function.once_differentiable
    def backward(ctx, grad):
        r = ctx.record
        return _index_gather(r.W, r.H, r.win, grad.to(dtype=th.float32).contiguous(), r.N), None


class _GatherMemory(th.autograd.Function):
    """gather_memory: the read-out driven by the record's cells (die_gather_memory's values, bit for bit) forward,
    die_gather_memory_backward backward."""

    @staticmethod
    def forward(ctx, sense_tail, record):
        ctx.record, ctx.M = record, sense_tail.shape[0]
        return _index_gather(record.W, record.H, record.cell, sense_tail, record.N)

    @staticmethod
    @th.autograd.function.once_differentiable
    def backward(ctx, grad):
        r, M = ctx.record, ctx.M
        g = grad.to(dtype=th.float32).contiguous()
        planes = th.empty((M, r.W, r.H), dtype=th.float32, device=g.device)      # (cleared by the call)
        _lib.check(_lib.lib.die_gather_memory_backward(r.W, r.H, M, r.N, _ptr(r.cell), _ptr(g), r.N, _ptr(planes), r.W * r.H,
                                                       stream_ptr(g.device)), 'die_gather_memory_backward')
        return planes, None


def memory_planes(memory: th.Tensor, record: MemoryRecord) -> th.Tensor:
    """The expand with a `grad_fn`: an (M, N) float32 memory by slot id -> the (M, W, H) planes a forward senses, P_j[c] =
    memory[j][winner of c], +0 on empty cells (die_memory_planes on the record's standing plane, into storage the graph owns).
    The backward is die_memory_planes_backward: grad_memory[j][id] = grad_planes[j][record.win[id]], +0 for dead slots and the
    losers of a shared cell — a gather, bit-reproducible."""
    _check_memory_op('memory', memory, record, lambda r: (r.N,))
    return _MemoryPlanes.apply(memory.contiguous(), record)


def gather_memory(sense_tail: th.Tensor, record: MemoryRecord) -> th.Tensor:
    """The memory read-out with a `grad_fn`: the stack's planes 3.. as an (M, W, H) float32 tensor -> (M, N) by slot id,
    memory[j][id] = sense_tail[j][record.cell[id]] for an alive slot, +0 for a dead one: die_gather_memory's values bit for bit,
    read through the record (die_memory_planes_backward's gather with `cell` for an index) so that nothing looks at the world
    again.  The backward is die_gather_memory_backward: the slots' gradients added onto their cells by fp32 atomic adds —
    bit-reproducible run to run whenever no cell holds more than two alive slots with a non-zero gradient."""
    _check_memory_op('sense_tail', sense_tail, record, lambda r: (r.W, r.H))
    return _GatherMemory.apply(sense_tail.contiguous(), record)


class SignalRecord:
    """Which cells were stood on at one forward (die_signal_cells): `occupied`, a (W, H) uint8 plane — 1 where the standing plane
    named an alive slot at its epoch, else 0 — and the sizes `W`, `H`.  The adjoint of the field's update is driven by this plane
    alone, so a graph that keeps the record survives the next standing build, every step, re-sort and `reset_signals()`; it holds
    1 byte per cell where a copy of the standing plane would hold 8.  The record also remembers the standing plane and epoch it
    was taken from, for `signal_step`'s forward only: step before that plane is built again."""
    __slots__ = ('occupied', 'W', 'H', '_standing', '_epoch')

    def __init__(self, occupied, W, H, standing, epoch):
        self.occupied, self.W, self.H, self._standing, self._epoch = occupied, int(W), int(H), standing, int(epoch)


def signal_record(obs, standing: Optional[th.Tensor] = None) -> SignalRecord:
    """The record of `obs` = (agents, medium) as they stand now: one die_signal_cells launch.  `standing`: the (W, H) int64
    standing plane built for these agents at `medium.epoch` (die_stock_plane; NeuralAutomataAgent builds one per forward), or
    None to build one here (a plane of its own, one launch more)."""
    agents, medium = obs
    dev, W, H = medium.device, medium.W, medium.H
    m = medium.c_struct(need_owner=False)
    sp = stream_ptr(dev)
    if standing is None:
        standing = th.zeros((W, H), dtype=th.int64, device=dev)
        a = agents.c_struct()
        _lib.check(_lib.lib.die_stock_plane(C.byref(m), C.byref(a), medium.epoch, _ptr(standing), sp), 'die_stock_plane')
    else:
        _check_standing(standing, (W, H), dev)
    occupied = th.empty((W, H), dtype=th.uint8, device=dev)                   # (every byte is written by the call)
    _lib.check(_lib.lib.die_signal_cells(C.byref(m), _ptr(standing), medium.epoch, _ptr(occupied), sp), 'die_signal_cells')
    return SignalRecord(occupied, W, H, standing, medium.epoch)


class _SignalStep(th.autograd.Function):
    """signal_step: die_signal_step forward into storage the graph owns, one die_signal_step_backward launch backward — the
    forward's own sweep on the gradient planes (on the torus Gᵀ = G) with the masked multiply at its store."""

    @staticmethod
    def forward(ctx, field, emission, record, deposit, sigma, decay):
        K, W, H = field.shape
        out = th.empty((K, W, H), dtype=th.float32, device=field.device)
        m = _bare_medium(W, H, record._epoch)
        _lib.check(_lib.lib.die_signal_step(C.byref(m), _ptr(record._standing), record._epoch, K, _ptr(emission), W * H, _ptr(field),
                                            _ptr(out), W * H, deposit, sigma, decay, stream_ptr(field.device)), 'die_signal_step')
        ctx.record, ctx.constants = record, (deposit, sigma, decay)
        return out

    @staticmethod
    @th.autograd.function.once_differentiable
    def backward(ctx, grad):
        r, (deposit, sigma, decay) = ctx.record, ctx.constants
        want_field, want_emission = ctx.needs_input_grad[:2]
        if not (want_field or want_emission):
            return None, None, None, None, None, None
        g = grad.to(dtype=th.float32).contiguous()
        K = g.shape[0]
        grad_field = th.empty_like(g) if want_field else None                  # (every cell is written by the call)
        grad_emission = th.empty_like(g) if want_emission else None
        _lib.check(_lib.lib.die_signal_step_backward(r.W, r.H, _ptr(r.occupied), K, _ptr(g), r.W * r.H, _ptr(grad_field), _ptr(grad_emission),
                                                     r.W * r.H, deposit, sigma, decay, stream_ptr(g.device)), 'die_signal_step_backward')
        return grad_field, grad_emission, None, None, None, None


def signal_step(field: th.Tensor, emission: th.Tensor, record: SignalRecord, *, deposit: float, sigma: float, decay: float) -> th.Tensor:
    """The signal field's update with a `grad_fn`: `field` and `emission` (K, W, H) float32 on the record's device, 1 <= K <= 8 ->
    `(1 - decay) * gaussian(field + occupied * deposit * emission, sigma, mode='wrap', truncate=4)`, die_signal_step's launch and
    bits on the record's standing plane, into storage the graph owns.  The backward is ONE die_signal_step_backward launch, which
    produces only the gradients asked for: grad_field = (1 - decay) * gaussian(grad) — the same sweep — and grad_emission =
    occupied ? deposit * grad_field : +0.  A sweep and a mask: no atomics, bit-reproducible."""
    if not isinstance(record, SignalRecord):
        raise TypeError('record: a SignalRecord (die_amd.functional.signal_record)')
    dev = record.occupied.device
    for name, t in (('field', field), ('emission', emission)):
        if not isinstance(t, th.Tensor) or t.dtype != th.float32 or t.dim() != 3 or tuple(t.shape[1:]) != (record.W, record.H) or \
                not 1 <= t.shape[0] <= _lib.SIGNAL_MAX_CHANNELS or t.device != dev:
            raise ValueError(f'{name}: a float32 tensor of shape (K, {record.W}, {record.H}) with K in 1..{_lib.SIGNAL_MAX_CHANNELS} on {dev}')
    if field.shape[0] != emission.shape[0]:
        raise ValueError(f'field has {field.shape[0]} planes, emission {emission.shape[0]}')
    return _SignalStep.apply(field.contiguous(), emission.contiguous(), record, float(deposit), float(sigma), float(decay))


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


# ---------------------------------------------------------------------------------------------------- memory channels, batched
class BatchedMemoryRecord:
    """Where every slot of every replica stood at one forward (die_memory_cells_batch): `cell` and `win`, (R, Nmax) int32 by slot
    id — `MemoryRecord`'s two arrays with an R in front, the padding slots from n[r] on -1 in both — and the sizes `W`, `H`, `R`,
    `Nmax`, `n`.  Both batched adjoints are driven by these two arrays alone, so a graph that keeps the record survives every
    step and reset of the worlds.  The record also remembers the standing planes (the population's own buffer) and the epoch it
    was taken at, for `memory_planes_batch`'s forward only: expand before the next record is taken."""
    __slots__ = ('cell', 'win', 'W', 'H', 'R', 'Nmax', 'n', '_batch', '_standing', '_epoch')

    def __init__(self, cell, win, W, H, n, batch, standing, epoch):
        self.cell, self.win, self.W, self.H, self.R, self.Nmax = cell, win, int(W), int(H), int(cell.shape[0]), int(cell.shape[1])
        self.n, self._batch, self._standing, self._epoch = tuple(n), batch, standing, int(epoch)


def _record_population(population, what: str, kind: str, alone: str):
    """The population of a batched record, checked: it has channels of `kind` ('memory' / 'signal') and small worlds; its env."""
    from .batch import BatchedNeuralAutomataAgent
    if not isinstance(population, BatchedNeuralAutomataAgent):
        raise TypeError('population: a BatchedNeuralAutomataAgent')
    if not getattr(population, f'_{kind}_channels'):
        raise ValueError(f'{what}: a population without {kind} channels ({kind}_channels=0) has no record')
    if population.env.per_replica:
        raise NotImplementedError(f'{what}: large worlds (per_replica) are not batched — every replica is a stand-alone agent: use '
                                  f'replica_agent(r).{alone}')
    return population.env


def memory_record_batch(population, standing: Optional[th.Tensor] = None) -> BatchedMemoryRecord:
    """The record of a BatchedNeuralAutomataAgent's worlds as they stand now: the R standing planes built at the env's epoch
    (die_stock_plane_batch) in a buffer the POPULATION owns and zeroes on every call — not the env's stock planes, so a later
    `env.step(population)` finds those as it left them, and two calls at one epoch are safe — then one die_memory_cells_batch
    launch.  `standing`: such planes already built for these worlds at this epoch (a `signal_record_batch`'s), taken as they
    are.  Small worlds; a population with memory channels."""
    env = _record_population(population, 'memory_record_batch', 'memory', 'recurrent_action / functional.memory_record')
    dev, R, W, H, Nmax = env.device, env.R, env.W, env.H, env.Nmax
    if standing is None:
        standing = _standing_planes_batch(population)
    else:
        _check_standing(standing, (R, W, H), dev)
    m, a, _, b = env._structs()
    sp = stream_ptr(dev)
    cell = th.empty((R, Nmax), dtype=th.int32, device=dev)           # (every word is written: the padding slots -1)
    win = th.empty((R, Nmax), dtype=th.int32, device=dev)
    _lib.check(_lib.lib.die_memory_cells_batch(C.byref(m), C.byref(a), C.byref(b), _ptr(standing), env.epoch, _ptr(cell), _ptr(win), sp),
               'die_memory_cells_batch')
    return BatchedMemoryRecord(cell, win, W, H, env.n, b, standing, env.epoch)


def _index_gather_batch(record, index, planes, plane_stride, replica_stride, M):
    """die_memory_planes_backward_batch as the index-only gather it is: planes of R replicas -> (R, M, Nmax) rows, +0 where the
    index is negative (the padding included), the values moved as 32-bit words."""
    out = th.empty((record.R, M, record.Nmax), dtype=th.float32, device=planes.device)
    _lib.check(_lib.lib.die_memory_planes_backward_batch(record.W, record.H, M, C.byref(record._batch), _ptr(index), _ptr(planes), plane_stride,
                                                         replica_stride, _ptr(out), record.Nmax, stream_ptr(planes.device)),
               'die_memory_planes_backward_batch')
    return out


def _plane_strides(t: th.Tensor, replica_dim: int, plane_dim: int, W: int, H: int):
    """(tensor, plane_stride, replica_stride) of a 4-d tensor of planes whose planes are dense: as it is where its strides say
    so (a slice of a larger buffer, a permuted view), else a contiguous copy."""
    if t.stride()[2:] != (H, 1) or t.stride(plane_dim) < W * H or t.stride(replica_dim) < W * H:
        t = t.contiguous()
    return t, t.stride(plane_dim), t.stride(replica_dim)


def _check_batched_memory_op(name, t, record, tail):
    """`t` must be a float32 (R, M, *tail(record)) tensor on the record's device, 1 <= M <= 8."""
    if not isinstance(record, BatchedMemoryRecord):
        raise TypeError('record: a BatchedMemoryRecord (die_amd.functional.memory_record_batch)')
    shape = tail(record)
    if not isinstance(t, th.Tensor) or t.dtype != th.float32 or t.dim() != 2 + len(shape) or t.shape[0] != record.R or \
            tuple(t.shape[2:]) != shape or not 1 <= t.shape[1] <= _lib.MEMORY_MAX_CHANNELS or t.device != record.cell.device:
        raise ValueError(f'{name}: a float32 tensor of shape ({record.R}, M, {", ".join(str(s) for s in shape)}) with M in 1..'
                         f'{_lib.MEMORY_MAX_CHANNELS} on {record.cell.device}')


class _BatchedMemoryPlanes(th.autograd.Function):
    """memory_planes_batch: die_memory_planes_batch forward into storage the graph owns, die_memory_planes_backward_batch backward."""

    @staticmethod
    def forward(ctx, memory, record):
        R, W, H, M = record.R, record.W, record.H, memory.shape[1]
        # plane j of replica r at (j * R + r) * W * H: a batched layer launch reads plane j of every replica one plane apart
        planes = th.empty((M, R, W, H), dtype=th.float32, device=memory.device)
        m = _bare_medium(W, H, record._epoch)
        _lib.check(_lib.lib.die_memory_planes_batch(C.byref(m), C.byref(record._batch), _ptr(record._standing), record._epoch, M, _ptr(memory),
                                                    record.Nmax, _ptr(planes), stream_ptr(memory.device)), 'die_memory_planes_batch')
        ctx.record, ctx.M = record, M
        return planes

    @staticmethod
    @th.autograd.function.once_differentiable
    def backward(ctx, grad):
        r = ctx.record
        g, plane_stride, replica_stride = _plane_strides(grad.to(dtype=th.float32), 1, 0, r.W, r.H)
        return _index_gather_batch(r, r.win, g, plane_stride, replica_stride, ctx.M), None


class _BatchedGatherMemory(th.autograd.Function):
    """gather_memory_batch: the read-out driven by the record's cells forward, die_gather_memory_backward_batch backward."""

    @staticmethod
    def forward(ctx, sense_tail, record):
        ctx.record, ctx.M = record, sense_tail.shape[1]
        t, plane_stride, replica_stride = _plane_strides(sense_tail, 0, 1, record.W, record.H)
        return _index_gather_batch(record, record.cell, t, plane_stride, replica_stride, ctx.M)

    @staticmethod
    @th.autograd.function.once_differentiable
    def backward(ctx, grad):
        r, M = ctx.record, ctx.M
        g = grad.to(dtype=th.float32).contiguous()
        planes = th.empty((r.R, M, r.W, r.H), dtype=th.float32, device=g.device)      # (cleared by the call)
        _lib.check(_lib.lib.die_gather_memory_backward_batch(r.W, r.H, M, C.byref(r._batch), _ptr(r.cell), _ptr(g), r.Nmax, _ptr(planes),
                                                             r.W * r.H, M * r.W * r.H, stream_ptr(g.device)),
                   'die_gather_memory_backward_batch')
        return planes, None


def memory_planes_batch(memory: th.Tensor, record: BatchedMemoryRecord) -> th.Tensor:
    """The expand of every replica with a `grad_fn`: an (R, M, Nmax) float32 memory by slot id -> (M, R, W, H) planes — plane j of
    replica r one plane after replica r - 1's, the layout in which a batched layer launch reads them — in storage the graph owns
    (die_memory_planes_batch on the record's standing planes).  `out[j, r]` is bit for bit the stand-alone `memory_planes` of
    replica r.  The backward is die_memory_planes_backward_batch: a gather, bit-reproducible; the padding slots get +0."""
    _check_batched_memory_op('memory', memory, record, lambda r: (r.Nmax,))
    return _BatchedMemoryPlanes.apply(memory.contiguous(), record)


def gather_memory_batch(sense_tail: th.Tensor, record: BatchedMemoryRecord) -> th.Tensor:
    """The memory read-out of every replica with a `grad_fn`: the stacks' planes 3.. as an (R, M, W, H) float32 tensor (a slice
    `sense[:, 3:]` is read where it lies) -> (R, M, Nmax) by slot id, bit for bit die_gather_memory_batch's values, read through
    the record; dead and padding slots +0.  The backward is die_gather_memory_backward_batch: fp32 atomic adds, replica r the
    stand-alone bits wherever no cell holds more than two alive slots with a non-zero gradient."""
    _check_batched_memory_op('sense_tail', sense_tail, record, lambda r: (r.W, r.H))
    return _BatchedGatherMemory.apply(sense_tail, record)


# ---------------------------------------------------------------------------------------------------- signal channels, batched
class SignalRecordBatch:
    """Which cells of every replica were stood on at one forward (die_signal_cells_batch): `occupied`, an (R, W, H) uint8 view —
    `SignalRecord`'s plane with an R in front, replica r's plane a multiple of 16 bytes after replica r - 1's — and the sizes `W`,
    `H`, `R`.  The batched adjoint of the fields' update is driven by these planes alone, so a graph that keeps the record survives
    every step, reset and reseeding of the worlds and `reset_signals()`.  The record also remembers the standing planes and the
    epoch it was taken at, for `signal_step_batch`'s forward only: step before those planes are built again."""
    __slots__ = ('occupied', 'W', 'H', 'R', '_batch', '_standing', '_epoch')

    def __init__(self, occupied, W, H, batch, standing, epoch):
        self.occupied, self.W, self.H, self.R = occupied, int(W), int(H), int(occupied.shape[0])
        self._batch, self._standing, self._epoch = batch, standing, int(epoch)


def _standing_planes_batch(population) -> th.Tensor:
    """The R standing planes of a population's worlds as they stand now, built at the env's epoch (die_stock_plane_batch) in a
    buffer the POPULATION owns and zeroes on every call — not the env's stock planes."""
    env = population.env
    standing = getattr(population, '_standing', None)
    if standing is None:
        standing = population._standing = th.zeros((env.R, env.W, env.H), dtype=th.int64, device=env.device)
    else:
        standing.zero_()
    m, a, _, b = env._structs()
    _lib.check(_lib.lib.die_stock_plane_batch(C.byref(m), C.byref(a), C.byref(b), env.epoch, _ptr(standing), stream_ptr(env.device)),
               'die_stock_plane_batch')
    return standing


def signal_record_batch(population, standing: Optional[th.Tensor] = None) -> SignalRecordBatch:
    """The record of a BatchedNeuralAutomataAgent's worlds as they stand now: ONE die_signal_cells_batch launch for all R
    replicas.  `standing`: the contiguous (R, W, H) int64 standing planes built for these worlds at the env's epoch
    (die_stock_plane_batch), or None to build them here, in the buffer the population owns (`memory_record_batch`'s: one launch
    more).  Small worlds; a population with signal channels."""
    env = _record_population(population, 'signal_record_batch', 'signal', 'signalling_action / functional.signal_record')
    dev, R, W, H = env.device, env.R, env.W, env.H
    if standing is None:
        standing = _standing_planes_batch(population)
    else:
        _check_standing(standing, (R, W, H), dev)
    m, _, _, b = env._structs()
    stride = (W * H + 15) // 16 * 16                                          # every replica's bytes on a 16-byte boundary
    store = th.empty((R, stride), dtype=th.uint8, device=dev)                  # (every byte of every plane is written by the call)
    _lib.check(_lib.lib.die_signal_cells_batch(C.byref(m), C.byref(b), _ptr(standing), env.epoch, _ptr(store), stride, stream_ptr(dev)),
               'die_signal_cells_batch')
    return SignalRecordBatch(store[:, :W * H].view(R, W, H), W, H, b, standing, env.epoch)


class _SignalStepBatch(th.autograd.Function):
    """signal_step_batch: die_signal_step_batch forward into storage the graph owns, ONE die_signal_step_backward_batch launch
    backward.  Inside, the field and its gradient lie (K, R, W, H) — plane k of every replica one plane apart, as a batched layer
    launch reads them; outside they are (R, K, W, H) views of that."""

    @staticmethod
    def forward(ctx, field, emission, record, deposit, sigma, decay):
        R, K, W, H = field.shape
        field = field.permute(1, 0, 2, 3).contiguous()                         # (free for a view of this op's own output)
        emission, plane_stride, replica_stride = _plane_strides(emission, 0, 1, W, H)
        if replica_stride < (K - 1) * plane_stride + W * H:                    # (the launch reads a replica's K planes together)
            emission = emission.contiguous()
            plane_stride, replica_stride = W * H, K * W * H
        out = th.empty((K, R, W, H), dtype=th.float32, device=field.device)
        m = _bare_medium(W, H, record._epoch)
        _lib.check(_lib.lib.die_signal_step_batch(C.byref(m), C.byref(record._batch), _ptr(record._standing), record._epoch, K, _ptr(emission),
                                                  plane_stride, replica_stride, _ptr(field), _ptr(out), deposit, sigma, decay,
                                                  stream_ptr(field.device)), 'die_signal_step_batch')
        ctx.record, ctx.constants = record, (deposit, sigma, decay)
        return out.permute(1, 0, 2, 3)

    @staticmethod
    @th.autograd.function.once_differentiable
    def backward(ctx, grad):
        r, (deposit, sigma, decay) = ctx.record, ctx.constants
        want_field, want_emission = ctx.needs_input_grad[:2]
        if not (want_field or want_emission):
            return None, None, None, None, None, None
        g = grad.to(dtype=th.float32).permute(1, 0, 2, 3).contiguous()         # (K, R, W, H)
        K, cells = g.shape[0], r.W * r.H
        grad_field = th.empty_like(g) if want_field else None                  # (every cell is written by the call)
        grad_emission = th.empty((r.R, K, r.W, r.H), dtype=th.float32, device=g.device) if want_emission else None
        _lib.check(_lib.lib.die_signal_step_backward_batch(r.W, r.H, C.byref(r._batch), _ptr(r.occupied), r.occupied.stride(0), K, _ptr(g),
                                                           _ptr(grad_field), _ptr(grad_emission), cells, K * cells, deposit, sigma, decay,
                                                           stream_ptr(g.device)), 'die_signal_step_backward_batch')
        return None if grad_field is None else grad_field.permute(1, 0, 2, 3), grad_emission, None, None, None, None


def signal_step_batch(field: th.Tensor, emission: th.Tensor, record: SignalRecordBatch, *, deposit: float, sigma: float,
                      decay: float) -> th.Tensor:
    """The update of every replica's signal field with a `grad_fn`: `field` and `emission` (R, K, W, H) float32 on the record's
    device, of any strides (a slice `sense[:, 3:3 + K]` is read where it lies), 1 <= K <= 8 -> the (R, K, W, H) next fields,
    `out[r]` bit for bit the stand-alone `signal_step` of replica r: ONE die_signal_step_batch launch on the record's standing
    planes, into storage the graph owns.  The backward is ONE die_signal_step_backward_batch launch for all K·R planes, which
    produces only the gradients asked for.  A sweep and a mask: no atomics, bit-reproducible."""
    if not isinstance(record, SignalRecordBatch):
        raise TypeError('record: a SignalRecordBatch (die_amd.functional.signal_record_batch)')
    dev = record.occupied.device
    for name, t in (('field', field), ('emission', emission)):
        if not isinstance(t, th.Tensor) or t.dtype != th.float32 or t.dim() != 4 or t.shape[0] != record.R or \
                tuple(t.shape[2:]) != (record.W, record.H) or not 1 <= t.shape[1] <= _lib.SIGNAL_MAX_CHANNELS or t.device != dev:
            raise ValueError(f'{name}: a float32 tensor of shape ({record.R}, K, {record.W}, {record.H}) with K in 1..'
                             f'{_lib.SIGNAL_MAX_CHANNELS} on {dev}')
    if field.shape[1] != emission.shape[1]:
        raise ValueError(f'field has {field.shape[1]} planes a replica, emission {emission.shape[1]}')
    return _SignalStepBatch.apply(field, emission, record, float(deposit), float(sigma), float(decay))


# ---- heredity: the memory a newborn receives (die_heredity.hip) ---------------------------------------------------------------
class BirthsRecord:
    """Who was born to whom in one birth pass (die_births_record), by SLOT ID: `parent_of` and `child_of`, int32 device tensors of
    shape (N,) — or (R, Nmax) for a BatchedEnv, the slots from n[r] on -1 — with parent_of[s] the parent of a slot born in the
    pass and child_of[s] the child of a slot that bred in it, -1 otherwise; `seeds`, the world seed of every replica (`seed`: the
    first, a stand-alone world's own), `step`, the world step the pass drew at, and `n`, the slots of every replica.  Freshly
    allocated by every `births_record()` call, so a graph may keep it through later steps and resets."""
    __slots__ = ('parent_of', 'child_of', 'seeds', 'step', 'n')

    def __init__(self, parent_of, child_of, seeds, step, n):
        self.parent_of, self.child_of = parent_of, child_of
        self.seeds, self.step, self.n = tuple(int(q) for q in seeds), int(step), tuple(int(k) for k in n)

    @property
    def seed(self) -> int:
        return self.seeds[0]

    @property
    def batched(self) -> bool:
        return self.parent_of.dim() == 2

    def _batch(self) -> _lib.Batch:
        return _lib.Batch(len(self.n), 0, 0, self.parent_of.shape[1], 1, (C.c_int64 * 64)(*self.n))

    def _seed_words(self):
        return (C.c_uint64 * len(self.seeds))(*[q & 0xFFFFFFFFFFFFFFFF for q in self.seeds])


def inherit_arguments(mode, mutation, what: str = 'inherit_memory'):
    """(mode, mutation) checked — 'blank' or 'copy', and a real number a >= 0 that float32 holds, 0 unless the mode is 'copy' — or
    the ValueError that says which is wrong."""
    if not isinstance(mode, str) or mode not in _lib.INHERIT_MODES:
        raise ValueError(f"{what}: memory_inherit={mode!r}: 'blank' or 'copy'")
    if isinstance(mutation, (bool, np.bool_)) or not isinstance(mutation, (int, float, np.integer, np.floating)):
        raise ValueError(f'{what}: memory_mutation={mutation!r}: a float >= 0')
    a = float(mutation)
    if not 0.0 <= a <= float(np.finfo(np.float32).max):
        raise ValueError(f'{what}: memory_mutation={mutation!r}: a finite float >= 0 (float32)')
    if a > 0.0 and mode != 'copy':
        raise ValueError(f"{what}: memory_mutation={mutation!r} needs memory_inherit='copy' (a blank newborn has nothing to mutate)")
    return mode, a


def check_inherit_operands(what: str, memory, record, batched: bool, M: Optional[int] = None, contiguous: bool = False) -> None:
    """A BirthsRecord of the right kind and a float32 memory of its shape on its device ((M, N), or (R, M, Nmax)), or the ValueError."""
    if not isinstance(record, BirthsRecord) or record.batched != batched:
        kind = 'BatchedEnv.births_record()' if batched else 'Env.births_record()'
        raise ValueError(f'{what}: record must be the BirthsRecord of {kind}, got {type(record).__name__}' +
                         (' of the other kind' if isinstance(record, BirthsRecord) else ''))
    dev, lead = record.parent_of.device, tuple(record.parent_of.shape)
    ok = isinstance(memory, th.Tensor) and memory.dtype == th.float32 and memory.device == dev and memory.dim() == len(lead) + 1 and \
        (not contiguous or memory.is_contiguous())
    if ok:
        Mc = memory.shape[-2]
        ok = 1 <= Mc <= _lib.MEMORY_MAX_CHANNELS and (M is None or Mc == M) and tuple(memory.shape) == lead[:-1] + (Mc, lead[-1])
    if not ok:
        want = lead[:-1] + ('M' if M is None else M, lead[-1])
        got = (tuple(memory.shape), memory.dtype, str(memory.device)) if isinstance(memory, th.Tensor) else type(memory).__name__
        raise ValueError(f"{what}: memory must be a {'contiguous ' if contiguous else ''}float32 tensor of shape "
                         f"({', '.join(str(v) for v in want)}) on {dev}, got {got}")


def inherit_memory_(memory: th.Tensor, record: BirthsRecord, mode: str, mutation: float) -> th.Tensor:
    """die_memory_inherit / _batch IN PLACE on a contiguous memory; every argument has been checked by the caller."""
    code, sp = _lib.INHERIT_MODES[mode], stream_ptr(memory.device)
    M, N = memory.shape[-2], memory.shape[-1]
    if record.batched:
        b = record._batch()
        _lib.check(_lib.lib.die_memory_inherit_batch(code, mutation, M, C.byref(b), _ptr(record.parent_of), _ptr(memory), record._seed_words(),
                                                     record.step & 0xFFFFFFFF, sp), 'die_memory_inherit_batch')
    else:
        _lib.check(_lib.lib.die_memory_inherit(code, mutation, M, N, _ptr(record.parent_of), _ptr(memory), N, record.seed & 0xFFFFFFFFFFFFFFFF,
                                               record.step & 0xFFFFFFFF, sp), 'die_memory_inherit')
    return memory


class _InheritMemory(th.autograd.Function):
    """inherit_memory / inherit_memory_batch: a clone and the in-place kernel forward, the gather of die_memory_inherit_backward backward."""

    @staticmethod
    def forward(ctx, memory, record, mode, mutation):
        ctx.record, ctx.mode = record, mode
        return inherit_memory_(memory.detach().clone(memory_format=th.contiguous_format), record, mode, mutation)

    @staticmethod
    @th.autograd.function.once_differentiable
    def backward(ctx, grad):
        r, code = ctx.record, _lib.INHERIT_MODES[ctx.mode]
        g = grad.to(dtype=th.float32).contiguous()
        out = th.empty_like(g)
        M, N, sp = g.shape[-2], g.shape[-1], stream_ptr(g.device)
        if r.batched:
            b = r._batch()
            _lib.check(_lib.lib.die_memory_inherit_backward_batch(code, M, C.byref(b), _ptr(r.parent_of), _ptr(r.child_of), _ptr(g), _ptr(out), sp),
                       'die_memory_inherit_backward_batch')
        else:
            _lib.check(_lib.lib.die_memory_inherit_backward(code, M, N, _ptr(r.parent_of), _ptr(r.child_of), _ptr(g), _ptr(out), N, sp),
                       'die_memory_inherit_backward')
        return out, None, None, None


def inherit_memory(memory: th.Tensor, record: BirthsRecord, mode: str, mutation: float = 0.0) -> th.Tensor:
    """Heredity with a `grad_fn`: the (M, N) float32 memory by slot id as a step's read-out left it -> the memory after the
    newborns of `record` (`Env.births_record()`) have received theirs.  For every child f of parent p: +0 ('blank'), the parent's
    word ('copy'), or the parent's value plus `mutation` times a uniform draw in [-1, 1] from the births' own key and step
    ('copy', mutation > 0); every other slot keeps its bits.  The input is left alone (the kernel runs on a clone).
    Backward, one gather launch: a parent's gradient is its own plus its child's ('copy'; 'blank': its own), a child's +0, every
    other slot's passes through — bit-reproducible."""
    mode, mutation = inherit_arguments(mode, mutation)
    check_inherit_operands('inherit_memory', memory, record, False)
    return _InheritMemory.apply(memory, record, mode, mutation)


def inherit_memory_batch(memory: th.Tensor, record: BirthsRecord, mode: str, mutation: float = 0.0) -> th.Tensor:
    """`inherit_memory` for every replica of a BatchedEnv in one launch: (R, M, Nmax) -> (R, M, Nmax), `record` the
    `BatchedEnv.births_record()` of the pass; replica r is `inherit_memory` on its own record and world seed, bit for bit, and the
    padding slots from n[r] on pass through, values and gradients alike."""
    mode, mutation = inherit_arguments(mode, mutation, 'inherit_memory_batch')
    check_inherit_operands('inherit_memory_batch', memory, record, True)
    return _InheritMemory.apply(memory, record, mode, mutation)
