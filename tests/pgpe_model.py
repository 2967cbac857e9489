"""Host model of the PGPE search (die_amd/csrc/die_search.hip, include/die_hip.h `die_pgpe`), written from its specification,
not from the kernels: float64 numpy, one rounding per operation in the order the specification states, the Philox draws
from oracle/rng.py.

- sample: z(i, p) from normals2(seed, generation, n·P, stream=8, scale=1)[0] (counter i·P + p); ε = σ_p·z;
  row 2i = fl32(c_p + ε), row 2i + 1 = fl32(c_p − ε)
- update: f_r = Σ_t terms[t, r] (t ascending); centred ranks u_r = k/(R − 1) − 0.5 (ascending, ties by index);
  ε̃ = row_2i − c; g_μ = (1/n) Σ_i ε̃·(u_2i − u_2i+1)/2, g_σ = (1/n) Σ_i ((u_2i + u_2i+1)/2)·(ε̃² − σ²)/σ (i ascending);
  ClipUp (ĝ = g_μ/‖g_μ‖, v ← m·v + α·ĝ, clipped to max_speed, c ← c + v) or Adam on −g_μ; σ' = σ + η·g_σ clamped to
  [σ(1 − δ), σ(1 + δ)] then [σ_min, σ_max]; pop_best / best; a history row (mean, max, min, median, ‖g_μ‖, mean σ')."""
import dataclasses
from typing import Optional

import numpy as np

from oracle.rng import normals2

STREAM_SEARCH = 8
f32 = np.float32


@dataclasses.dataclass
class Config:
    center_lr: float = 0.05
    stdev_lr: float = 0.1
    optimizer: str = 'clipup'
    max_speed: float = 0.1
    momentum: float = 0.9
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    stdev_max_change: Optional[float] = 0.2
    stdev_min: Optional[float] = None
    stdev_max: Optional[float] = None


class State:
    """The device buffers of die_pgpe, as float32 arrays (state) and float64 (fitness, evals, history)."""

    def __init__(self, center, stdev, R, seed=0, cfg: Optional[Config] = None):
        self.center = np.asarray(center, dtype=f32).copy()
        self.stdev = np.asarray(stdev, dtype=f32).copy()
        self.P = self.center.size
        self.R, self.seed, self.cfg = int(R), int(seed), cfg or Config()
        self.opt_a = np.zeros(self.P, f32)
        self.opt_b = np.zeros(self.P, f32)
        self.pop_best = np.zeros(self.P, f32)
        self.best = np.zeros(self.P, f32)
        self.fitness = np.zeros(self.R)
        self.evals = np.array([-np.inf, -np.inf])
        self.history = []

    def copy(self):
        s = State(self.center, self.stdev, self.R, self.seed, dataclasses.replace(self.cfg))
        for k in ('opt_a', 'opt_b', 'pop_best', 'best', 'fitness', 'evals'):
            setattr(s, k, getattr(self, k).copy())
        s.history = [h.copy() for h in self.history]
        return s


def noise(seed, generation, n, P):
    """z of (n, P): Box–Muller on the first two Philox words of counter i·P + p."""
    return normals2(seed, generation, n * P, stream=STREAM_SEARCH, scale=1.0)[0].reshape(n, P)


def sample(st: State, generation: int) -> np.ndarray:
    n, P = st.R // 2, st.P
    e = st.stdev.astype(np.float64) * noise(st.seed, generation, n, P)
    c = st.center.astype(np.float64)
    rows = np.empty((st.R, P), dtype=f32)
    rows[0::2] = (c + e).astype(f32)
    rows[1::2] = (c - e).astype(f32)
    return rows


def fitness(terms) -> np.ndarray:
    """Σ_t terms[t, r], t ascending (a serial sum, not numpy's pairwise one)."""
    terms = np.asarray(terms, dtype=np.float64)
    f = np.zeros(terms.shape[1])
    for t in range(terms.shape[0]):
        f = f + terms[t]
    return f


def centred_ranks(f) -> np.ndarray:
    R = len(f)
    order = np.argsort(f, kind='stable')
    k = np.empty(R, dtype=np.int64)
    k[order] = np.arange(R)
    return k / (R - 1) - 0.5


def gradients(st: State, rows: np.ndarray, u: np.ndarray):
    n = st.R // 2
    c, s = st.center.astype(np.float64), st.stdev.astype(np.float64)
    ss = s * s
    gm, gs = np.zeros(st.P), np.zeros(st.P)
    for i in range(n):
        e = rows[2 * i].astype(np.float64) - c
        du, av = (u[2 * i] - u[2 * i + 1]) / 2.0, (u[2 * i] + u[2 * i + 1]) / 2.0
        gm = gm + e * du
        gs = gs + av * ((e * e - ss) / s)
    return gm / n, gs / n


def update(st: State, rows: np.ndarray, terms, generation: int) -> State:
    """One die_pgpe_update on a copy of `st` (terms: (T, R))."""
    st, cfg = st.copy(), st.cfg
    R = st.R
    f = fitness(terms)
    u = centred_ranks(f)
    b = int(np.argmax(f))                   # (the first of the maxima)
    srt = np.sort(f)
    hist = [_serial_sum(f) / R, srt[-1], srt[0], (srt[R // 2 - 1] + srt[R // 2]) / 2.0]
    st.fitness = f
    st.pop_best = rows[b].copy()
    st.evals[0] = f[b]
    if f[b] > st.evals[1]:
        st.evals[1] = f[b]
        st.best = rows[b].copy()
    gm, gs = gradients(st, rows, u)
    s = st.stdev.astype(np.float64)
    ns = s + cfg.stdev_lr * gs
    if cfg.stdev_max_change is not None:
        ns = np.minimum(np.maximum(ns, s * (1.0 - cfg.stdev_max_change)), s * (1.0 + cfg.stdev_max_change))
    if cfg.stdev_min is not None:
        ns = np.maximum(ns, cfg.stdev_min)
    if cfg.stdev_max is not None:
        ns = np.minimum(ns, cfg.stdev_max)
    st.stdev = ns.astype(f32)
    norm = float(np.sqrt(np.sum(gm * gm)))
    c = st.center.astype(np.float64)
    if cfg.optimizer == 'clipup':
        gh = gm / norm if norm > 0 else np.zeros_like(gm)
        v = cfg.momentum * st.opt_a.astype(np.float64) + cfg.center_lr * gh
        vn = float(np.sqrt(np.sum(v * v)))
        if vn > cfg.max_speed:
            v = v * cfg.max_speed / vn
        st.center = (c + v).astype(f32)
        st.opt_a = v.astype(f32)
    else:
        t = generation + 1
        g = -gm
        m = cfg.beta1 * st.opt_a.astype(np.float64) + (1.0 - cfg.beta1) * g
        v = cfg.beta2 * st.opt_b.astype(np.float64) + (1.0 - cfg.beta2) * (g * g)
        bc1, bc2s = 1.0 - cfg.beta1 ** t, np.sqrt(1.0 - cfg.beta2 ** t)
        st.center = (c - (cfg.center_lr / bc1) * (m / (np.sqrt(v) / bc2s + cfg.eps))).astype(f32)
        st.opt_a, st.opt_b = m.astype(f32), v.astype(f32)
    st.history = st.history + [np.array(hist + [norm, float(np.sum(st.stdev.astype(np.float64))) / st.P])]
    return st


def _serial_sum(x) -> float:
    s = 0.0
    for v in np.asarray(x, dtype=np.float64).tolist():
        s += v
    return s


# The sphere objective both suites use: f = −‖x‖² over SPHERE_P parameters, the reference's hyperparameters (popsize 10,
# radius_init 1.5, ClipUp max_speed 0.1 / momentum 0.9, center_lr 0.05, stdev_lr 0.1), the centre drawn in (−0.5, 0.5) from
# torch.Generator().manual_seed(seed).  After SPHERE_GENERATIONS the model leaves 0.31..0.36 of the starting distance over
# seeds 0..5 (tests/test_pgpe_cpu.py); the device run must leave less than SPHERE_RATIO of it.
SPHERE_P, SPHERE_R, SPHERE_GENERATIONS, SPHERE_RATIO = 162, 10, 100, 0.5
REFERENCE = dict(radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1, optimizer='clipup',
                 optimizer_config=dict(max_speed=0.1, momentum=0.9))
