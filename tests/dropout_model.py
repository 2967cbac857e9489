"""TEST INFRASTRUCTURE ONLY: the numpy twin of the counter-based agent-dropout mask (die_amd/csrc/die_rng.h, include/die_hip.h
die_nca_dropout), written from its definition with oracle/rng.py's Philox.

For key s, forward-call counter t and cell c = ix·H + iy of a (W, H) plane: word(c) is word c & 3 of
Philox(counter = (lo32(c >> 2), hi32(c >> 2), t, 10), key = s); the cell is dropped iff word(c) < thr = ceil(p · 2^32) (float64,
compared as 64-bit integers); a kept cell is multiplied by keep = float32(1 / (1 − p))."""
import math

import numpy as np

from oracle.rng import _draw

STREAM_DROPOUT = 10
MASK64 = 0xFFFFFFFFFFFFFFFF


def words(seed: int, step: int, cells) -> np.ndarray:
    """word(c) of every cell index in `cells` (uint32)."""
    c = np.asarray(cells, dtype=np.uint64)
    r = _draw(int(seed) & MASK64, int(step) & 0xFFFFFFFF, c >> np.uint64(2), STREAM_DROPOUT)
    return np.choose((c & np.uint64(3)).astype(np.int64), [r[0], r[1], r[2], r[3]]).astype(np.uint32)


def threshold(p: float) -> int:
    if not 0.0 < p <= 1.0:
        raise ValueError(f'p = {p}: 0 < p <= 1')
    return int(math.ceil(float(p) * 4294967296.0))


def keep_factor(p: float) -> np.float32:
    return np.float32(np.inf) if p >= 1.0 else np.float32(1.0 / (1.0 - float(p)))


def dropped(seed: int, step: int, W: int, H: int, p: float) -> np.ndarray:
    """(W, H) bool: the cells the mask zeroes."""
    w = words(seed, step, np.arange(W * H, dtype=np.uint64)).astype(np.uint64)
    return (w < np.uint64(threshold(p))).reshape(W, H)                   # (p = 1: thr = 2^32, above every word)


def mask(seed: int, step: int, W: int, H: int, p: float) -> np.ndarray:
    """(W, H) float32: 0 where dropped, keep elsewhere."""
    return np.where(dropped(seed, step, W, H, p), np.float32(0), keep_factor(p)).astype(np.float32)


def replica_masks(seed: int, stride: int, step: int, R: int, W: int, H: int, p: float) -> np.ndarray:
    """(R, W, H): replica r is masked with key seed + r·stride (mod 2^64)."""
    return np.stack([mask((int(seed) + r * int(stride)) & MASK64, step, W, H, p) for r in range(R)])
