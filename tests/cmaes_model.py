"""Host model of separable CMA-ES (die_amd/csrc/die_cmaes.hip, include/die_hip.h `die_cmaes`), written from its
specification, not from the kernels: float64 numpy, one rounding per operation in the order the specification states, the
Philox draws from oracle/rng.py.

- constants: w'_k = ln((λ+1)/2) − ln k; μ = ⌊λ/2⌋; positive weights normalised to 1, μ_eff = 1/Σ w_k²; c_σ, d_σ, c_c, c_1,
  c_μ, χ_d times their ratios; active negative weights w'_k·min(α_μ⁻, α_μeff⁻, α_posdef⁻)/Σ|w'⁻|, or 0
- sample: z(i, p) = normals2(seed, g, λ·d, stream=9, scale=1)[0][i·d + p]; row i = fl32(m_p + (σ·sqrt(C_p))·z(i, p))
- update: f_r = Σ_t terms[t, r] (t ascending); ranks by descending f, ties to the lower index; y = sqrt(C)·z; y_w, z_w over
  the μ best (best first); m, p_σ, h_σ, p_c, C, σ in that order; pop_best / best; a history row
  (mean, max, min, median, σ', mean of σ'·sqrt(C'))."""
import dataclasses
import math

import numpy as np

from oracle.rng import normals2

STREAM_CMAES = 9
f32 = np.float32


@dataclasses.dataclass
class Config:
    c_m: float = 1.0
    c_sigma_ratio: float = 1.0
    damp_sigma_ratio: float = 1.0
    c_c_ratio: float = 1.0
    c_1_ratio: float = 1.0
    c_mu_ratio: float = 1.0
    active: bool = True
    csa_squared: bool = False


def constants(lam: int, d: int, cfg: Config = None) -> dict:
    """Weights (λ, best rank first) and the learning rates, the way the header states them."""
    cfg = cfg or Config()
    d = float(d)
    mu = lam // 2
    wp = np.log((lam + 1) / 2.0) - np.log(np.arange(1, lam + 1, dtype=np.float64))
    w_pos = wp[:mu] / np.sum(wp[:mu])
    mu_eff = 1.0 / np.sum(w_pos ** 2)
    neg = wp[mu:]
    mu_eff_minus = np.sum(neg) ** 2 / np.sum(neg ** 2) if np.any(neg != 0) else 0.0
    c_sigma = cfg.c_sigma_ratio * (mu_eff + 2.0) / (d + mu_eff + 5.0)
    d_sigma = cfg.damp_sigma_ratio * (1.0 + 2.0 * max(0.0, math.sqrt((mu_eff - 1.0) / (d + 1.0)) - 1.0) + c_sigma)
    c_c = cfg.c_c_ratio * (1.0 + 1.0 / d + mu_eff / d) / (math.sqrt(d) + 1.0 / d + 2.0 * mu_eff / d)
    c_1 = cfg.c_1_ratio * 1.0 / (d + 2.0 * math.sqrt(d) + mu_eff / d)
    c_mu = cfg.c_mu_ratio * min(1.0 - c_1, (0.25 + mu_eff + 1.0 / mu_eff - 2.0) / (d + 4.0 * math.sqrt(d) + mu_eff / 2.0))
    chi_d = math.sqrt(d) * (1.0 - 1.0 / (4.0 * d) + 1.0 / (21.0 * d * d))
    if cfg.active and np.any(neg != 0):
        alpha = min(1.0 + c_1 / c_mu, 1.0 + 2.0 * mu_eff_minus / (mu_eff + 2.0), (1.0 - c_1 - c_mu) / (d * c_mu))
        w_neg = neg * alpha / np.sum(np.abs(neg))
    else:
        w_neg = np.zeros_like(neg)
    return dict(weights=np.concatenate([w_pos, w_neg]), mu=mu, mu_eff=float(mu_eff), mu_eff_minus=float(mu_eff_minus),
                c_sigma=c_sigma, d_sigma=d_sigma, c_c=c_c, c_1=c_1, c_mu=c_mu, chi_d=chi_d)


class State:
    """The device buffers of die_cmaes: m, C, p_σ, p_c, σ (float64), pop_best / best (float32), fitness, evals, history."""

    def __init__(self, center, sigma, R, seed=0, cfg: Config = None):
        self.m = np.asarray(center, dtype=np.float64).copy()
        self.P = self.m.size
        self.R, self.seed, self.cfg = int(R), int(seed), cfg or Config()
        self.k = constants(self.R, self.P, self.cfg)
        self.C = np.ones(self.P)
        self.ps = np.zeros(self.P)
        self.pc = np.zeros(self.P)
        self.sigma = float(sigma)
        self.pop_best = np.zeros(self.P, f32)
        self.best = np.zeros(self.P, f32)
        self.fitness = np.zeros(self.R)
        self.evals = np.array([-np.inf, -np.inf])
        self.order = np.arange(self.R)
        self.history = []
        self.h_sigma = []                # h_σ of every update
        self.h_margin = []               # ‖p_σ‖/sqrt(1 − (1 − c_σ)^(2(g+1))) over the threshold

    def copy(self):
        s = State(self.m, self.sigma, self.R, self.seed, dataclasses.replace(self.cfg))
        for k in ('C', 'ps', 'pc', 'pop_best', 'best', 'fitness', 'evals', 'order'):
            setattr(s, k, getattr(self, k).copy())
        s.history = [h.copy() for h in self.history]
        s.h_sigma, s.h_margin = list(self.h_sigma), list(self.h_margin)
        return s


def noise(seed, generation, R, P):
    """z of (R, P): Box–Muller on the first two Philox words of counter i·P + p."""
    return normals2(seed, generation, R * P, stream=STREAM_CMAES, scale=1.0)[0].reshape(R, P)


def sample(st: State, generation: int) -> np.ndarray:
    z = noise(st.seed, generation, st.R, st.P)
    t = st.sigma * np.sqrt(st.C)
    return (st.m + t * z).astype(f32)


def fitness(terms) -> np.ndarray:
    """Σ_t terms[t, r], t ascending (a serial sum, not numpy's pairwise one)."""
    terms = np.asarray(terms, dtype=np.float64)
    f = np.zeros(terms.shape[1])
    for t in range(terms.shape[0]):
        f = f + terms[t]
    return f


def ranking(f) -> np.ndarray:
    """Replica of rank k (best first): descending f, ties to the lower replica index."""
    return np.argsort(-np.asarray(f, dtype=np.float64), kind='stable')


def update(st: State, rows: np.ndarray, terms, generation: int) -> State:
    """One die_cmaes_update on a copy of `st` (terms: (T, R)); `rows` are the generation's samples."""
    st, cfg, k = st.copy(), st.cfg, st.k
    R, d, mu, w = st.R, float(st.P), k['mu'], k['weights']
    f = fitness(terms)
    order = ranking(f)
    b = int(order[0])
    srt = np.sort(f)
    median = srt[R // 2] if R % 2 else (srt[R // 2 - 1] + srt[R // 2]) / 2.0
    hist = [_serial_sum(f) / R, srt[-1], srt[0], median]
    st.fitness, st.order = f, order
    st.pop_best = rows[b].copy()
    st.evals[0] = f[b]
    if f[b] > st.evals[1]:
        st.evals[1] = f[b]
        st.best = rows[b].copy()
    z = noise(st.seed, generation, R, st.P)[order]          # z_{k:λ}, best first
    sd = np.sqrt(st.C)
    y = sd * z
    yw, zw = np.zeros(st.P), np.zeros(st.P)
    for j in range(mu):
        yw = yw + w[j] * y[j]
        zw = zw + w[j] * z[j]
    st.m = st.m + (cfg.c_m * st.sigma) * yw
    cs, cc = k['c_sigma'], k['c_c']
    st.ps = (1.0 - cs) * st.ps + math.sqrt(cs * (2.0 - cs) * k['mu_eff']) * zw
    psq = float(np.sum(st.ps * st.ps))
    psn = math.sqrt(psq)
    lhs = psn / math.sqrt(1.0 - (1.0 - cs) ** (2.0 * (generation + 1)))
    thr = (1.4 + 2.0 / (d + 1.0)) * k['chi_d']
    h = 1.0 if lhs < thr else 0.0
    st.h_sigma.append(h)
    st.h_margin.append(lhs / thr)
    st.pc = (1.0 - cc) * st.pc + (h * math.sqrt(cc * (2.0 - cc) * k['mu_eff'])) * yw
    wo = w.copy()
    for j in range(R):
        if w[j] < 0:
            wo[j] = w[j] * d / float(np.sum(z[j] * z[j]))
    rank_mu = np.zeros(st.P)
    for j in range(R):
        rank_mu = rank_mu + wo[j] * (y[j] * y[j])
    c1, cmu = k['c_1'], k['c_mu']
    coef = 1.0 + (1.0 - h) * (c1 * cc * (2.0 - cc)) - c1 - cmu * _serial_sum(w)
    st.C = coef * st.C + c1 * (st.pc * st.pc) + cmu * rank_mu
    if cfg.csa_squared:
        st.sigma = st.sigma * math.exp((cs / (2.0 * k['d_sigma'])) * (psq / d - 1.0))
    else:
        st.sigma = st.sigma * math.exp((cs / k['d_sigma']) * (psn / k['chi_d'] - 1.0))
    st.history = st.history + [np.array(hist + [st.sigma, float(np.sum(st.sigma * np.sqrt(st.C))) / st.P])]
    return st


def _serial_sum(x) -> float:
    s = 0.0
    for v in np.asarray(x, dtype=np.float64).tolist():
        s += v
    return s


def run(st: State, objective, generations: int) -> State:
    """`generations` of sample, objective(rows) -> (R,) fitness, update."""
    g0 = len(st.history)
    for g in range(g0, g0 + generations):
        rows = sample(st, g)
        st = update(st, rows, np.asarray(objective(rows), dtype=np.float64)[None, :], g)
    return st


def sphere(rows):
    return -np.sum(rows.astype(np.float64) ** 2, axis=1)


def ellipsoid_scales(d):
    return 10.0 ** (3.0 * np.arange(d) / (d - 1))


def ellipsoid(rows):
    """The separable ellipsoid f = −Σ 10^(3p/(d−1))·x_p² (coefficients 1..1000)."""
    r = rows.astype(np.float64)
    return -np.sum(ellipsoid_scales(r.shape[1]) * r * r, axis=1)


# The sphere: SPHERE_P = 20 parameters with the default popsize 4 + ⌊3 ln 20⌋ = 12, stdev_init 0.3, the centre drawn in
# (−0.5, 0.5) from torch.Generator().manual_seed(seed).  After SPHERE_GENERATIONS the model's centre is 0.0016..0.0054 of its
# starting distance over seeds 0..5 (tests/test_cmaes_cpu.py); a run must leave less than SPHERE_RATIO of it.
SPHERE_P, SPHERE_SIGMA, SPHERE_GENERATIONS, SPHERE_RATIO = 20, 0.3, 100, 0.05

# The separable ellipsoid (d = ELLIPSOID_D, popsize 10, stdev_init 0.3, the centre drawn as for the sphere): after
# ELLIPSOID_GENERATIONS the model's C_0/C_{d−1} is 639..1963 over seeds 0..5 (the optimum is 1000, the ratio of the
# coefficients) and f(centre_0)/f(centre_G) is 2.8e7 and more; a run must pass ELLIPSOID_COND and ELLIPSOID_GAIN.
ELLIPSOID_D, ELLIPSOID_R, ELLIPSOID_SIGMA, ELLIPSOID_GENERATIONS, ELLIPSOID_COND, ELLIPSOID_GAIN = 10, 10, 0.3, 120, 100.0, 1e5
