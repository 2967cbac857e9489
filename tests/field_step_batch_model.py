"""The oracle of the differentiable BatchedEnv.step (tests/test_batch_field_step_cpu.py, tests/test_gpu_batch_field_step_grad.py):
tests/field_step_adjoint_model.py with an R in front.  Replica r = c * E + e is candidate c's e-th world; its rollout is the stand-alone
model's — the same `step_chem`, the same read-out (tests/nca_grad_model.py) — with candidate c's conv layers, and all R rollouts hang
on ONE torch graph whose loss is the sum of the replicas' losses, so that `weight.grad` of candidate c is the sum over its E worlds,
which is what a (C, P) `parameters.grad` holds.  sigma and decay may differ per replica (per-replica Dynamics).

Positions, the 'agents' plane, food and the winners' cells are data, as in the stand-alone model: recorded from the device, or made up
with `synthetic_batch`."""
from typing import Sequence

import numpy as np
import torch

from tests import field_step_adjoint_model as F
from tests import nca_grad_model as G


def _per_replica(v, R: int):
    return [float(v)] * R if np.ndim(v) == 0 else [float(x) for x in v]


def rollout(weights: Sequence[Sequence[np.ndarray]], boundary: str, chem0: Sequence[np.ndarray], frames, cells, c: Sequence[np.ndarray],
            u: Sequence[np.ndarray], sigma, decay=F.DECAY, coefs=F.COEFS, with_agent_channel: bool = True, episodes: int = 1,
            dtype=torch.float64):
    """weights[cand][layer]; chem0[r], frames[r] (T + 1 dicts), cells[r] (T arrays), c[r] (W, H), u[r] (3, n_r) per replica, as the
    stand-alone `rollout` takes them for one world; sigma, decay: one number or one per replica.
    Returns dict(loss (R,), grads[cand][layer], chem[r] = chem_T, action[r] = action_T) as numpy float64."""
    R, E = len(frames), int(episodes)
    assert R % E == 0 and len(weights) == R // E and len(cells) == len(chem0) == len(c) == len(u) == R
    sig, dec = _per_replica(sigma, R), _per_replica(decay, R)
    as_t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    convs = [G.layers(w, boundary, dtype) for w in weights]
    losses, chems, actions = [], [], []
    for r in range(R):
        T = len(cells[r])
        assert len(frames[r]) == T + 1
        net, chem = convs[r // E], as_t(chem0[r])

        def act(t):
            f = frames[r][t]
            planes = torch.stack(([as_t(f['occ'])] if with_agent_channel else []) + [as_t(f['food']), chem])
            m = as_t(f['mask']) if f.get('mask') is not None else None
            return G.action(net, planes, f['cx'], f['cy'], coefs, m)

        for t in range(T):
            chem = F.step_chem(chem, act(t)[2], cells[r][t], sig[r], dec[r])
        action = act(T)
        losses.append((as_t(c[r]) * chem).sum() + (as_t(u[r]) * action).sum())
        chems.append(chem)
        actions.append(action)
    torch.stack(losses).sum().backward()
    f64 = lambda x: x.detach().to(torch.float64).numpy()
    return dict(loss=np.array([float(v.detach()) for v in losses]), grads=[[f64(k.weight.grad) for k in net] for net in convs],
                chem=[f64(x) for x in chems], action=[f64(x) for x in actions])


def synthetic_batch(name: str, W: int, H: int, T: int, R: int, episodes: int = 1):
    """A made-up batch for the CPU checks: replica r is the case's `synthetic_frames` trajectory without its first r slots (replicas
    of different sizes, as the 'alive' layout holds them) on a chem plane scaled by 1 + r / 8, with its own loss vectors; candidate c
    holds the case's weights shifted by c / 100.  Returns (weights[cand][layer], chem0[r], frames[r], cells[r], c[r], u[r])."""
    weights = [[w + 0.01 * cand for w in F.weights_of(name, W, H)] for cand in range(R // episodes)]
    chem0, frames, cells, cs, us = [], [], [], [], []
    for r in range(R):
        ch, fr, ce = replica_frames(name, W, H, T, r)
        cv, uv = F.loss_vectors(name, W, H, fr[0]['cx'].size)
        rs = np.random.RandomState(1000 + r)
        chem0.append(ch)
        frames.append(fr)
        cells.append(ce)
        cs.append(cv * rs.uniform(0.5, 1.5))
        us.append(uv * rs.uniform(0.5, 1.5))
    return weights, chem0, frames, cells, cs, us


def replica_frames(name: str, W: int, H: int, T: int, r: int):
    """`synthetic_frames` of the case for replica r: the trajectory itself for r = 0; for r > 0 its slots from r on, the winners
    decided again among them by the host rule (a dropped slot may have been one)."""
    chem0, frames, cells = F.synthetic_frames(name, W, H, T)
    if r == 0:
        return chem0, frames, cells
    assert not F.CASES[name].get('sort_every')          # (a batch never re-sorts: array entry n is slot n throughout)
    alive = F.world_of(name, W, H)[1][2][r:] > 0
    kept = [dict(f, cx=f['cx'][r:], cy=f['cy'][r:]) for f in frames]
    won = [F.deposit_cells(kept[t + 1]['cx'], kept[t + 1]['cy'], alive, None, H) for t in range(T)]
    return chem0 * (1.0 + r / 8.0), kept, won
