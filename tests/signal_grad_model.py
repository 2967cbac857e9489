"""The model of the signal channels' adjoint (include/die_hip.h die_signal_cells / die_signal_step_backward;
die_amd.functional.signal_step; NeuralAutomataAgent.signalling_action), used by tests/test_signal_grad_cpu.py and
tests/test_gpu_signal_grad.py.  It extends tests/signal_model.py (the update) and tests/memory_grad_model.py (the recurrent loop).

The update is F' = (1 - decay) G(F + occ * deposit * S) with G the periodic gaussian of symmetric taps, so G^T = G and, for a
gradient g of F',

    adjoint           gF = (1 - decay) G(g),   gS = occ ? deposit * gF : 0                       (float64)
    emulate_backward  the same in fp32 in the kernels' order: the forward's sweep on g (tests/signal_model.py `emulate` where nobody
                      stands), then ONE fp32 multiply by deposit on the occupied cells, +0 elsewhere

and `unroll`, the T-step loop of `signalling_action` chained through `signals_next` (and `memory_next`) in torch: the loop of
tests/memory_grad_model.py with the field among the observation planes and the update after the stack; occupancies, records, the
slots' cells, the world's planes and the masks are given CONSTANTS."""
from typing import Optional, Sequence

import numpy as np
import torch

from tests import memory_grad_model as MG
from tests import signal_model as SM

f32 = np.float32


def adjoint(g, occ, deposit, sigma, decay):
    """(gF, gS) in float64 for the gradient g (K, W, H) of the updated field."""
    gF = (1.0 - float(f32(decay))) * SM.gaussian(np.asarray(g, dtype=np.float64), sigma)
    return gF, np.where(occ[None], float(f32(deposit)) * gF, 0.0)


def emission_grad32(gF, occ, deposit) -> np.ndarray:
    """gS from an fp32 gF as the kernel makes it: one fp32 multiply where somebody stands, +0.0 elsewhere."""
    gF = np.asarray(gF, dtype=f32)
    return np.where(occ[None], (f32(deposit) * gF).astype(f32), f32(0.0)).astype(f32)


def emulate_backward(g, occ, deposit, sigma, decay):
    """(gF, gS) in fp32 in the kernels' order: the forward's own sweep on g — `emulate` where nobody stands adds +0.0 to every cell,
    which changes nothing unless the cell holds -0.0 — then the masked multiply."""
    g = np.asarray(g, dtype=f32)
    gF = SM.emulate(g, np.zeros_like(occ), np.zeros_like(g), deposit, sigma, decay)
    return gF, emission_grad32(gF, occ, deposit)


def bound(g, sigma, decay) -> np.ndarray:
    """What |device gF - adjoint gF| may be: tests/signal_model.py `bound` with F := g and nobody standing."""
    g = np.asarray(g, dtype=f32)
    return SM.bound(g, np.zeros(g.shape[1:], dtype=bool), np.zeros_like(g), 0.0, sigma, decay)


def grad_case(W: int, H: int, K: int, seed: int = 0) -> np.ndarray:
    """A gradient (K, W, H): mixed signs on about 60 % of the cells, +0.0 (never -0.0) on the rest."""
    rs = np.random.RandomState(77 + 1000 * W + H + 7 * K + seed)
    return np.where(rs.rand(K, W, H) < 0.6, rs.uniform(-2, 2, (K, W, H)), 0.0).astype(f32)


# ---- the loop ---------------------------------------------------------------------------------------------------------------------
def t_gaussian(a: torch.Tensor, sigma) -> torch.Tensor:
    """tests/signal_model.py `gaussian` in torch: axis -2 first, then axis -1, wrapping."""
    w, R = SM.taps(sigma), SM.radius(sigma)
    out = a
    for axis in (-2, -1):
        out = sum(float(w[k + R]) * torch.roll(out, -k, dims=axis) for k in range(-R, R + 1))
    return out


def t_update(field: torch.Tensor, occ: torch.Tensor, emission: torch.Tensor, deposit, sigma, decay) -> torch.Tensor:
    return (1.0 - float(f32(decay))) * t_gaussian(field + occ[None] * (float(f32(deposit)) * emission), sigma)


def unroll(weights: Sequence[torch.Tensor], boundary: str, hidden_activation: Optional[str], frames, occs, sig0: torch.Tensor, constants, coefs,
           records=None, mem0: Optional[torch.Tensor] = None, with_agent_channel: bool = True, chem0: Optional[torch.Tensor] = None, world=None,
           detach_at: Sequence[int] = ()):
    """T = len(frames) rounds of `signalling_action`.  frames[t]: as in tests/memory_grad_model.py `unroll`; occs[t]: the (W, H)
    occupancy the update masks with; `sig0` (K, W, H) and `mem0` (M, N) or None: torch tensors whose dtype the loop runs in;
    `constants` = (deposit, sigma, decay); records[t] = (cell, win) with memory; `world` threads the chem plane as there.
    `detach_at`: rounds whose incoming field (and memory) are detached.  Returns dict(actions [T x (3, N)], signals [T + 1 x (K, W, H)],
    memories [T + 1 x (M, N)] or None, sense [T x (3 + K + M, W, H)], chem)."""
    dtype = sig0.dtype
    as_t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    W, H = np.asarray(frames[0]['food']).shape
    K = sig0.shape[0]
    deposit, sigma, decay = constants
    sig, mem, chem = sig0, mem0, chem0
    out = dict(actions=[], signals=[sig0], memories=None if mem0 is None else [mem0], sense=[])
    for t, f in enumerate(frames):
        cut = t in detach_at
        sig_in = sig.detach() if cut else sig
        parts = ([as_t(f['occ'])] if with_agent_channel else []) + [as_t(f['food']), chem if world is not None else as_t(f['chem'])]
        planes = [torch.stack(parts), sig_in]
        if mem is not None:
            cell, win = records[t]
            planes.append(MG.t_expand(W, H, win, mem.detach() if cut else mem))
        s = MG.conv_stack(weights, boundary, hidden_activation, torch.cat(planes), as_t(f['mask']) if f.get('mask') is not None else None)
        action = s[:3][:, MG._idx(f['cx']), MG._idx(f['cy'])] * torch.as_tensor(coefs, dtype=dtype)[:, None]
        sig = t_update(sig_in, as_t(np.asarray(occs[t], dtype=np.float64)), s[3:3 + K], deposit, sigma, decay)
        out['actions'].append(action)
        out['signals'].append(sig)
        out['sense'].append(s)
        if mem is not None:
            mem = MG.t_gather(cell, s[3 + K:])
            out['memories'].append(mem)
        if world is not None:
            from tests import field_step_adjoint_model as FS
            chem = FS.step_chem(chem, action[2], world['cells'][t], world['sigma'], world['decay'])
    out['chem'] = chem
    return out
