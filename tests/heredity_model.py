"""TEST INFRASTRUCTURE ONLY: the numpy twin of heredity (die_amd/csrc/die_heredity.hip, die_births.hip's record; include/die_hip.h
die_births_record / die_memory_inherit / die_memory_inherit_backward), written from the rule of DESIGN.md §6 with
tests/births_model.py's matching and oracle/rng.py's Philox.

The record of one birth pass, by slot id (int32, -1 = none):
    parent_of[free[j]] = parents[j],  child_of[parents[j]] = free[j]      for the pairs (parents[j], free[j]) of births_model.match

`inherit`, on an (M, N) float32 memory, for every pair (p, f) and channel m:
    'blank'          mem[m][f] = +0
    'copy', a == 0   mem[m][f] = mem[m][p]                    (moved as 32-bit words)
    'copy', a > 0    mem[m][f] = fl32(mem[m][p] + fl32(fl32(a) * u)),   u = float32(int32(word)) * 2^-31,
                     word = word (m & 3) of Philox(counter = (p, m >> 2, world_step, 12), key = world_seed)
every other word left alone.  `inherit_adjoint` is its transpose (the noise is an additive constant), and `unroll` the recurrent
T-step loop of tests/memory_grad_model.py with an inheritance link after every round that saw a birth pass."""
from typing import Optional, Sequence

import numpy as np
import torch

from oracle.rng import _draw
from tests import births_model as B
from tests import memory_grad_model as MG

STREAM_HEREDITY = 12
MODES = ('blank', 'copy')
MASK64 = 0xFFFFFFFFFFFFFFFF


def record(alive, agent_food, born_threshold: float, stride: Optional[int] = None):
    """(parent_of, child_of) of the birth pass on these n slots (their state BEFORE the pass), int32; `stride` > n pads both with -1
    as the batched record does."""
    n = len(alive)
    parents, free = B.match(alive, agent_food, born_threshold)
    parent_of = np.full(n if stride is None else stride, -1, dtype=np.int32)
    child_of = parent_of.copy()
    parent_of[free] = parents
    child_of[parents] = free
    return parent_of, child_of


def pairs(parent_of):
    """(parents, children) int64 arrays of a record, by ascending child."""
    children = np.flatnonzero(np.asarray(parent_of) >= 0)
    return np.asarray(parent_of)[children].astype(np.int64), children.astype(np.int64)


def unit_noise(world_seed: int, world_step: int, parents, M: int) -> np.ndarray:
    """u of every (channel, parent): (M, len(parents)) float32 in [-1, 1]."""
    p = np.asarray(parents, dtype=np.uint64)
    out = np.zeros((M, len(p)), dtype=np.float32)
    for m in range(M):
        w = _draw(int(world_seed) & MASK64, int(world_step) & 0xFFFFFFFF, p | (np.uint64(m >> 2) << np.uint64(32)), STREAM_HEREDITY)
        word = np.asarray(w[m & 3], dtype=np.uint32)
        out[m] = word.view(np.int32).astype(np.float32) * np.float32(2.0 ** -31)      # the conversion rounds to nearest even, the scaling is exact
    return out


def noise(world_seed: int, world_step: int, parents, M: int, a: float) -> np.ndarray:
    """fl32(fl32(a) * u): what is added to the parent's value, (M, len(parents)) float32."""
    return (np.float32(a) * unit_noise(world_seed, world_step, parents, M)).astype(np.float32)


def inherit(mem, parent_of, mode: str, a: float = 0.0, world_seed: int = 0, world_step: int = 0) -> np.ndarray:
    """The memory after heredity: a new (M, N) float32 array."""
    assert mode in MODES and a >= 0 and (mode == 'copy' or a == 0)
    out = np.array(mem, dtype=np.float32)
    parents, children = pairs(np.asarray(parent_of)[:out.shape[1]])
    if not len(children):
        return out
    words = out.view(np.uint32)
    if mode == 'blank':
        words[:, children] = 0
    elif a == 0:
        words[:, children] = words[:, parents]
    else:
        out[:, children] = (out[:, parents] + noise(world_seed, world_step, parents, out.shape[0], a)).astype(np.float32)
    return out


def inherit_adjoint(grad, parent_of, child_of, mode: str, dtype=np.float32) -> np.ndarray:
    """The gradient with respect to the memory before heredity, from the one after it: (M, N)."""
    assert mode in MODES
    g = np.asarray(grad, dtype=dtype)
    out = g.copy()
    n = g.shape[1]
    parent_of, child_of = np.asarray(parent_of)[:n], np.asarray(child_of)[:n]
    children, parents = np.flatnonzero(parent_of >= 0), np.flatnonzero(child_of >= 0)
    if mode == 'copy':
        out[:, parents] = (g[:, parents] + g[:, child_of[parents]]).astype(dtype)
    out[:, children] = 0
    return out


def jacobian_apply(x, parent_of, mode: str, dtype=np.float64) -> np.ndarray:
    """J x: heredity's linear part (the noise dropped) applied to a tangent (M, N)."""
    out = np.array(x, dtype=dtype)
    parents, children = pairs(np.asarray(parent_of)[:out.shape[1]])
    out[:, children] = out[:, parents] if mode == 'copy' else 0
    return out


# ---- the recurrent loop with births ---------------------------------------------------------------------------------------------
def t_inherit(mem: torch.Tensor, parent_of, mode: str, added=None) -> torch.Tensor:
    """`inherit` in torch, differentiable: `added` (M, number of pairs) is the noise as a constant, None for none."""
    parents, children = pairs(np.asarray(parent_of)[:mem.shape[1]])
    if not len(children):
        return mem
    if mode == 'blank':
        new = torch.zeros((mem.shape[0], len(children)), dtype=mem.dtype)
    else:
        new = mem[:, MG._idx(parents)]
        if added is not None:
            new = new + torch.as_tensor(np.asarray(added), dtype=mem.dtype)
    return mem.index_copy(1, MG._idx(children), new)


def unroll(weights: Sequence[torch.Tensor], boundary: str, hidden_activation: Optional[str], frames, records, links, mem0: torch.Tensor,
           coefs, with_agent_channel: bool = True, detach_inherited: bool = False):
    """tests/memory_grad_model.unroll's rounds (the world's planes taken as data) with heredity between them: links[t] = None or
    (parent_of, mode, added) applied to the memory round t leaves, before round t + 1 reads it.  `detach_inherited`: the inherited
    memory is detached (what a `.detach()` of `inherit_memory`'s result does).  Returns dict(actions, memories [the memory every
    round's forward read, then the last one], sense)."""
    dtype = mem0.dtype
    as_t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    W, H = np.asarray(frames[0]['food']).shape
    mem = mem0
    out = dict(actions=[], memories=[mem0], sense=[])
    for t, (cell, win) in enumerate(records):
        f = frames[t]
        P = MG.t_expand(W, H, win, mem)
        field = ([as_t(f['occ'])] if with_agent_channel else []) + [as_t(f['food']), as_t(f['chem'])]
        s = MG.conv_stack(weights, boundary, hidden_activation, torch.cat([torch.stack(field), P]),
                          as_t(f['mask']) if f.get('mask') is not None else None)
        action = s[:3][:, MG._idx(f['cx']), MG._idx(f['cy'])] * torch.as_tensor(coefs, dtype=dtype)[:, None]
        mem = MG.t_gather(cell, s[3:])
        if links[t] is not None:
            mem = t_inherit(mem, *links[t])
            if detach_inherited:
                mem = mem.detach()
        out['actions'].append(action)
        out['memories'].append(mem)
        out['sense'].append(s)
    return out
