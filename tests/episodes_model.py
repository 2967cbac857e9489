"""Host model of episodes (a candidate evaluated on E worlds per generation; die_*_update_episodes, BatchedEnv.reset(seeds=...)):
the fold of per-replica terms into per-candidate fitness, in numpy float64 and in the device's order, and the seed formulas.
Replica r = c·E + e is candidate c on its e-th world (candidate-major)."""
import numpy as np


def replica_sums(terms) -> np.ndarray:
    """F_r: the serial float64 sum over t ascending of terms[t, r] ((T, R) or (T, R, 2) with the reward in word 0)."""
    t = np.asarray(terms, dtype=np.float64)
    if t.ndim == 3:
        t = t[..., 0]
    F = np.zeros(t.shape[1], dtype=np.float64)
    for row in t:                                       # one add per step, in step order
        F = F + row
    return F


def fold(terms, candidates: int, episodes: int):
    """(f, F): F the (C, E) per-episode sums, f_c = (((0 + F_c0) + F_c1) + …) / E."""
    F = replica_sums(terms)
    assert F.shape == (candidates * episodes,)
    F = F.reshape(candidates, episodes)
    f = np.zeros(candidates, dtype=np.float64)
    for c in range(candidates):
        s = np.float64(0.0)
        for e in range(episodes):
            s = s + F[c, e]
        f[c] = s / np.float64(episodes)
    return f, F


def episode_seeds(seed: int, candidates: int, episodes: int, candidate_stride: int = 0):
    """seed + e + candidate_stride·c·E for c … for e …"""
    return [seed + e + candidate_stride * c * episodes for c in range(candidates) for e in range(episodes)]


def generation_seeds(reseed: int, g: int, candidates: int, episodes: int, reseed_stride: int = 0):
    """for_population(reseed=S, reseed_stride=k): generation g, replica (c, e) gets S + g·C·E + e + k·c·E."""
    return [reseed + g * candidates * episodes + e + reseed_stride * c * episodes for c in range(candidates) for e in range(episodes)]


def generation_seeds_today(reseed: int, g: int, replicas: int, reseed_stride: int = 0):
    """The formula without episodes: reset(seed=S + g·R, seed_stride=k), replica r gets S + g·R + r·k."""
    return [reseed + g * replicas + r * reseed_stride for r in range(replicas)]
