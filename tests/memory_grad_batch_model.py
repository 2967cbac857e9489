"""The model of the batched memory adjoints (include/die_hip.h die_memory_cells_batch / die_memory_planes_backward_batch /
die_gather_memory_backward_batch; BatchedNeuralAutomataAgent.recurrent_action), used by tests/test_memory_grad_batch_cpu.py and
tests/test_gpu_memory_grad_batch.py: loops over tests/memory_grad_model.py, one replica at a time.

    record_batch           replica r's first n[r] slots: memory_grad_model.record; the padding slots n[r] .. Nmax - 1: -1 twice
    expand_batch / expand_adjoint_batch / gather_batch / gather_adjoint_batch
                           the four maps of memory_grad_model per replica, on (R, M, Nmax) memories and (R, M, W, H) planes; the
                           padding gathers 0 and scatters nothing, because its index is -1
    unroll_batch           memory_grad_model.unroll per replica with candidate r // E's weights: the E replicas of a candidate
                           share their weight tensors, so a loss summed over the replicas gives each candidate the sum of its E
                           worlds' gradients, accumulated in the loop's dtype (float64 for the reference)."""
from typing import Sequence

import numpy as np
import torch

from tests import memory_grad_model as MG


def record_batch(W: int, H: int, x, y, alive, n: Sequence[int]):
    """(cell, win), int32 (R, Nmax) each.  x, y: (R, Nmax) uint32 coordinate words, alive (R, Nmax); replica r holds n[r] slots."""
    x, y, alive = np.asarray(x), np.asarray(y), np.asarray(alive)
    R, Nmax = x.shape
    cell, win = np.full((R, Nmax), -1, dtype=np.int32), np.full((R, Nmax), -1, dtype=np.int32)
    for r in range(R):
        k = int(n[r])
        if k:
            cell[r, :k], win[r, :k] = MG.record(W, H, x[r, :k], y[r, :k], alive[r, :k])
    return cell, win


def _per_replica(fn, W, H, index, values, dtype):
    return np.stack([fn(W, H, index[r], values[r], dtype) for r in range(len(index))])


def expand_batch(W, H, win, mem, dtype=np.float64):
    """(R, M, Nmax) -> (R, M, W, H)."""
    return _per_replica(MG.expand, W, H, win, mem, dtype)


def expand_adjoint_batch(W, H, win, grad_planes, dtype=np.float64):
    """(R, M, W, H) -> (R, M, Nmax): every word written, the padding 0."""
    return _per_replica(MG.expand_adjoint, W, H, win, grad_planes, dtype)


def gather_batch(W, H, cell, planes, dtype=np.float64):
    return _per_replica(MG.gather, W, H, cell, planes, dtype)


def gather_adjoint_batch(W, H, cell, grad_memory, dtype=np.float64):
    """(R, M, Nmax) -> (R, M, W, H), ascending slot id within a replica."""
    return _per_replica(MG.gather_adjoint, W, H, cell, grad_memory, dtype)


def unroll_batch(weights, boundary, hidden_activation, frames, records, mem0, coefs, episodes: int = 1, with_agent_channel: bool = True,
                 detach_at: Sequence[int] = ()):
    """weights[c]: candidate c's layer tensors (leaves where a gradient is wanted); frames[r], records[r]: replica r's T rounds as
    memory_grad_model.unroll takes them; mem0[r]: replica r's (M, n[r]) incoming memory.  Returns the list of the R replicas'
    `unroll` outputs: replica r runs candidate r // episodes."""
    return [MG.unroll(weights[r // episodes], boundary, hidden_activation, frames[r], records[r], mem0[r], coefs, with_agent_channel,
                      detach_at=detach_at) for r in range(len(frames))]


def pad_rows(rows, Nmax: int, dtype=np.float64) -> np.ndarray:
    """R arrays (M, n[r]) -> (R, M, Nmax), zeros in the padding."""
    out = np.zeros((len(rows), rows[0].shape[0], Nmax), dtype=dtype)
    for r, v in enumerate(rows):
        out[r, :, :v.shape[1]] = v
    return out


# ---- host-made records for the index kernels -----------------------------------------------------------------------------------
def crowded_record(kind: str = 'crowded'):
    """tests/test_gpu_memory_grad.py's made-up 24 x 68 record of 300 slots: forty pairs, every seventh slot dead, and with
    'crowded' a cell that four slots share (three or more of them alive); 'pairs' leaves the pairs alone."""
    W, H, N = 24, 68, 300
    rs = np.random.RandomState(17)
    cells = rs.choice(W * H, N, replace=False)
    cells[1:80:2] = cells[0:80:2]
    alive = np.arange(N) % 7 != 3
    if kind == 'crowded':
        cells[[100, 200]] = cells[0]
    cell = np.where(alive, cells, -1).astype(np.int32)
    win = np.full(N, -1, dtype=np.int32)
    for i in np.flatnonzero(alive):                                  # ascending slot id: the last writer wins its cell
        win[cell == cell[i]] = -1
        win[i] = cell[i]
    return W, H, N, cell, win


def replicated_record(kind: str, n: Sequence[int]):
    """`crowded_record` in every replica, cut to n[r] slots (0 allowed) and padded with -1 to max(n, 1): (W, H, Nmax, cell, win).
    A loser whose winner was cut off wins its cell."""
    W, H, N, cell, _ = crowded_record(kind)
    Nmax = max(max(n), 1)
    cells, wins = np.full((len(n), Nmax), -1, dtype=np.int32), np.full((len(n), Nmax), -1, dtype=np.int32)
    for r, k in enumerate(n):
        assert k <= N
        cells[r, :k] = cell[:k]
        for i in np.flatnonzero(cell[:k] >= 0):
            wins[r, :k][cell[:k] == cell[i]] = -1
            wins[r, i] = cell[i]
    return W, H, Nmax, cells, wins
