"""TEST INFRASTRUCTURE ONLY: the numpy twin of the birth pass of `Dynamics(agents_born=True)` (die_amd/csrc/die_births.hip,
include/die_hip.h die_agent_births), written from the rules of DESIGN.md §6 with oracle/rng.py's Philox.  Integer-exact for the
ranks, the draw and the displacement; float32 operations for the share.

State: x, y uint32 (Q0.32), alive uint8, agent_food float32, all of n slots in slot order.
  parents   slots alive with agent_food > float32(born_threshold), ascending
  free      slots not alive, ascending
  parent j breeds into free slot j for j < min(#parents, #free):
      child = float32(0.5) * food,  parent keeps food - child;  child alive = 1
      w = Philox(counter = (lo32(parent), hi32(parent), world_step, 11), key = world_seed)
      ox = (int64(int32(w[0])) * q) >> 31,  oy likewise from w[1],  q = round(born_spread * 2^32)
      wrap: x' = (x + ox) mod 2^32;  limit: x' = clip(x + ox, 0, 2^32 - 1)"""
import numpy as np

from oracle.rng import _draw

STREAM_BIRTH = 11
MASK64 = 0xFFFFFFFFFFFFFFFF
WRAP, LIMIT = 0, 1


def spread_q(born_spread: float) -> int:
    if not 0.0 <= float(born_spread) <= 0.5:
        raise ValueError(f'born_spread = {born_spread}: 0 .. 0.5')
    return int(round(float(born_spread) * 4294967296.0))      # (round half to even, as the library's llrint)


def match(alive, agent_food, born_threshold: float):
    """(parents, free) that breed: equal-length int64 arrays, pair j = (parents[j], free[j])."""
    alive = np.asarray(alive) != 0
    food = np.asarray(agent_food, dtype=np.float32)
    parents = np.nonzero(alive & (food > np.float32(born_threshold)))[0]
    free = np.nonzero(~alive)[0]
    k = min(len(parents), len(free))
    return parents[:k].astype(np.int64), free[:k].astype(np.int64)


def displacement(world_seed: int, world_step: int, parents, born_spread: float):
    """(ox, oy) int64 Q0.32 increments of the children of `parents`."""
    p = np.asarray(parents, dtype=np.uint64)
    w = _draw(int(world_seed) & MASK64, int(world_step) & 0xFFFFFFFF, p, STREAM_BIRTH)
    q = np.int64(spread_q(born_spread))
    signed = lambda u: np.asarray(u, dtype=np.uint32).view(np.int32).astype(np.int64)
    return (signed(w[0]) * q) >> np.int64(31), (signed(w[1]) * q) >> np.int64(31)


def place(X, off, boundary: int) -> np.ndarray:
    s = np.asarray(X, dtype=np.uint32).astype(np.int64) + np.asarray(off, dtype=np.int64)
    if boundary == WRAP:
        return (s & np.int64(0xFFFFFFFF)).astype(np.uint32)
    return np.clip(s, 0, 0xFFFFFFFF).astype(np.uint32)


def births(x, y, alive, agent_food, *, world_seed: int, world_step: int, born_threshold: float = 0.5, born_spread: float = 0.02,
           boundary: int = WRAP):
    """One birth pass: (x, y, alive, agent_food, born) — new arrays, the inputs are left alone."""
    x, y = np.array(x, dtype=np.uint32), np.array(y, dtype=np.uint32)
    alive, food = np.array(alive, dtype=np.uint8), np.array(agent_food, dtype=np.float32)
    parents, free = match(alive, food, born_threshold)
    if len(parents):
        ox, oy = displacement(world_seed, world_step, parents, born_spread)
        child = np.float32(0.5) * food[parents]
        keep = food[parents] - child
        cx, cy = place(x[parents], ox, boundary), place(y[parents], oy, boundary)
        food[parents] = keep
        x[free], y[free], alive[free], food[free] = cx, cy, 1, child
    return x, y, alive, food, len(parents)
