"""The model of the batched signal adjoint (include/die_hip.h die_signal_cells_batch / die_signal_step_backward_batch;
die_amd.functional.signal_step_batch; BatchedNeuralAutomataAgent.signalling_action), used by tests/test_signal_grad_batch_cpu.py and
tests/test_gpu_signal_grad_batch.py: loops over tests/signal_grad_model.py, one replica at a time — the replicas of a batch share
nothing but, with episodes, their candidate's weights.

    update_batch / adjoint_batch / emulate_backward_batch / bound_batch
                    tests/signal_model.py `update` and the three maps of signal_grad_model per replica, on (R, K, W, H) fields and
                    (R, W, H) occupancies
    case_batch      R different cases of tests/signal_model.py `case` / signal_grad_model `grad_case` (the seed is the replica)
    unroll_batch    signal_grad_model.unroll per replica with candidate r // E's weights: the E replicas of a candidate share their
                    weight tensors, so a loss summed over the replicas gives each candidate the sum of its E worlds' gradients,
                    accumulated in the loop's dtype (float64 for the reference)"""
from typing import Sequence

import numpy as np

from tests import signal_grad_model as SG
from tests import signal_model as SM


def update_batch(F, occ, planes, deposit, sigma, decay) -> np.ndarray:
    """(R, K, W, H) in float64."""
    return np.stack([SM.update(F[r], occ[r], planes[r], deposit, sigma, decay) for r in range(len(F))])


def adjoint_batch(g, occ, deposit, sigma, decay):
    """(gF, gS), (R, K, W, H) float64 each, for the gradient g (R, K, W, H) of the updated fields and the occupancies (R, W, H)."""
    pairs = [SG.adjoint(g[r], occ[r], deposit, sigma, decay) for r in range(len(g))]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def emulate_backward_batch(g, occ, deposit, sigma, decay):
    """The same in fp32 in the kernels' order."""
    pairs = [SG.emulate_backward(g[r], occ[r], deposit, sigma, decay) for r in range(len(g))]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def bound_batch(g, sigma, decay) -> np.ndarray:
    return np.stack([SG.bound(g[r], sigma, decay) for r in range(len(g))])


def case_batch(W: int, H: int, K: int, R: int):
    """(F (R, K, W, H), occ (R, W, H), planes (R, K, W, H), g (R, K, W, H)): another case in every replica."""
    cases = []
    for r in range(R):
        seed = 10 * r
        while not SM.case(W, H, K, seed=seed)[1].any():              # (a 3 x 8 world at 15 % can come out empty: somebody stands in every replica)
            seed += 1
        cases.append(SM.case(W, H, K, seed=seed))
    g = np.stack([SG.grad_case(W, H, K, seed=r) for r in range(R)])
    return np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases]), g


def unroll_batch(weights, boundary, hidden_activation, frames, occs, sig0, constants, coefs, records=None, mem0=None, episodes: int = 1,
                 with_agent_channel: bool = True, chem0=None, worlds=None, detach_at: Sequence[int] = ()):
    """weights[c]: candidate c's layer tensors (leaves where a gradient is wanted); frames[r], occs[r], records[r]: replica r's T
    rounds as signal_grad_model.unroll takes them; sig0[r] (K, W, H), mem0[r] (M, n[r]) or None, chem0[r] and worlds[r] or None.
    Returns the list of the R replicas' `unroll` outputs: replica r runs candidate r // episodes."""
    pick = lambda seq, r: None if seq is None else seq[r]     # noqa: E731
    return [SG.unroll(weights[r // episodes], boundary, hidden_activation, frames[r], occs[r], sig0[r], constants, coefs, pick(records, r),
                      pick(mem0, r), with_agent_channel, pick(chem0, r), pick(worlds, r), detach_at) for r in range(len(frames))]
