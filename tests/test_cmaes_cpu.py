"""Separable CMA-ES (die_cmaes_sample / die_cmaes_update, die_amd.search.CMAES), CPU side: the library exports both entry
points and the state struct matches its header field list, every bad argument is refused on the host before any launch, the
weights and constants follow the header's formulas on hand-computed cases, and the float64 model of tests/cmaes_model.py is
pinned on one generation by hand, minimises the sphere and adapts its covariance on the separable ellipsoid.  No kernel is
launched here."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import cmaes_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


def test_entry_points_exported_and_struct_follows_header(lib):
    so = C.CDLL(lib.LIB_PATH)
    for name in ('die_cmaes_sample', 'die_cmaes_update'):
        assert hasattr(so, name) and name in lib.EXPORTS
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    # die_cmaes: replicas, csa_squared (2 x i32), num_params i64, seed u64, eight doubles, weights[64], ten pointers,
    # history_rows i64, work
    assert C.sizeof(lib.Cmaes) == 2 * 4 + 8 + 8 + 8 * 8 + 64 * 8 + 10 * 8 + 8 + 8
    assert lib.cmaes_work_doubles(10, 162) == (4 + 10) * 256 + 162
    import die_amd
    assert die_amd.CMAES is die_amd.search.CMAES


FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host


def _state(lib, **kw):
    k = M.constants(10, 162)
    f = dict(replicas=10, csa_squared=0, num_params=162, seed=0, c_m=1.0, c_sigma=k['c_sigma'], d_sigma=k['d_sigma'], c_c=k['c_c'],
             c_1=k['c_1'], c_mu=k['c_mu'], mu_eff=k['mu_eff'], chi_d=k['chi_d'],
             weights=(C.c_double * 64)(*k['weights'].tolist()), center=FAKE, C=FAKE, p_sigma=FAKE, p_c=FAKE, sigma=FAKE,
             pop_best=FAKE, best=FAKE, fitness=FAKE, evals=FAKE, history=FAKE, history_rows=64, work=FAKE)
    f.update(kw)
    return lib.Cmaes(**f)


def _refused(lib, fn, *args, match):
    rc = getattr(lib.lib, fn)(*args)
    assert rc == -1, (fn, rc)
    msg = lib.lib.die_last_error().decode()
    assert match in msg, msg


@pytest.mark.parametrize('kw, match', [
    (dict(replicas=1), 'replicas 1: in 2..64'),
    (dict(replicas=65), 'replicas 65'),
    (dict(num_params=0), 'num_params 0'),
    (dict(c_m=0.0), 'c_m 0: must be positive'),
    (dict(c_sigma=0.0), 'c_sigma 0: in (0, 1]'),
    (dict(c_sigma=1.5), 'c_sigma 1.5'),
    (dict(d_sigma=0.0), 'd_sigma 0: must be positive'),
    (dict(c_c=0.0), 'c_c 0: in (0, 1]'),
    (dict(c_1=-0.1), 'c_1 -0.1'),
    (dict(c_1=0.6, c_mu=0.5), 'sum at most 1'),
    (dict(mu_eff=0.5), 'mu_eff 0.5: at least 1'),
    (dict(chi_d=0.0), 'chi_d 0: must be positive'),
    (dict(weights=(C.c_double * 64)()), 'weights[0] 0: must be positive'),
    (dict(center=None), 'null state buffer'),
    (dict(C=None), 'null state buffer'),
    (dict(sigma=None), 'null state buffer'),
    (dict(work=None), 'null state buffer'),
    (dict(history=None), 'null state buffer'),
])
def test_bad_state_refused_by_both_entry_points(lib, kw, match):
    s = _state(lib, **kw)
    _refused(lib, 'die_cmaes_sample', C.byref(s), FAKE, 0, None, match=match)
    _refused(lib, 'die_cmaes_update', C.byref(s), FAKE, FAKE, 30, 20, 2, 0, None, match=match)


def test_bad_call_arguments_refused(lib):
    s = _state(lib)
    _refused(lib, 'die_cmaes_sample', None, FAKE, 0, None, match='null state')
    _refused(lib, 'die_cmaes_sample', C.byref(s), None, 0, None, match='null parameter matrix')
    _refused(lib, 'die_cmaes_sample', C.byref(s), FAKE, -1, None, match='generation -1')
    _refused(lib, 'die_cmaes_sample', C.byref(s), FAKE, 1 << 32, None, match='generation 4294967296')
    up = lambda *a: _refused(lib, 'die_cmaes_update', *a[:-1], match=a[-1])
    up(None, FAKE, FAKE, 30, 20, 2, 0, None, 'null state')
    up(C.byref(s), None, FAKE, 30, 20, 2, 0, None, 'null parameter matrix or terms')
    up(C.byref(s), FAKE, None, 30, 20, 2, 0, None, 'null parameter matrix or terms')
    up(C.byref(s), FAKE, FAKE, 0, 20, 2, 0, None, 'T 0')
    up(C.byref(s), FAKE, FAKE, 30, 0, 2, 0, None, 'strides (0, 2) must be positive')
    up(C.byref(s), FAKE, FAKE, 30, 20, -2, 0, None, 'strides (20, -2) must be positive')
    up(C.byref(s), FAKE, FAKE, 30, 20, 2, 64, None, 'generation 64 beyond the 64 history rows')


def test_searcher_refusals_and_initial_state_without_gpu(lib):
    from die_amd.search import CMAES
    with pytest.raises(NotImplementedError, match='eigendecomposition'):
        CMAES(10, 162, stdev_init=0.1, separable=False, device='cpu')
    with pytest.raises(ValueError, match='popsize 1'):
        CMAES(1, 162, stdev_init=0.1, device='cpu')
    with pytest.raises(ValueError, match='popsize 65'):
        CMAES(65, 162, stdev_init=0.1, device='cpu')
    with pytest.raises(ValueError, match='popsize 66'):             # the default 4 + floor(3 ln P) beyond 64
        CMAES(None, 10 ** 9, stdev_init=0.1, device='cpu')
    for bad in (0.0, -0.1, math.inf, math.nan):
        with pytest.raises(ValueError, match='stdev_init'):
            CMAES(10, 162, stdev_init=bad, device='cpu')
    with pytest.raises(ValueError, match='c_m 0'):
        CMAES(10, 162, stdev_init=0.1, c_m=0.0, device='cpu')
    with pytest.raises(ValueError, match='c_sigma'):
        CMAES(10, 162, stdev_init=0.1, c_sigma_ratio=100.0, device='cpu')
    with pytest.raises(ValueError, match='c_1 \\+ c_mu'):
        CMAES(10, 162, stdev_init=0.1, c_1_ratio=200.0, device='cpu')
    with pytest.raises(ValueError, match='num_params, or a center_init'):
        CMAES(10, stdev_init=0.1, device='cpu')
    s = CMAES(None, 162, stdev_init=0.1, seed=5, device='cpu')      # NEProblem(initial_bounds=(-0.5, 0.5))
    want = -0.5 + torch.rand(162, generator=torch.Generator().manual_seed(5), dtype=torch.float32)
    assert torch.equal(s.center, want.double())
    assert s.R == 19 and s.P == 162 and s.iter == 0 and s.sigma == 0.1
    assert torch.equal(s.C, torch.ones(162, dtype=torch.float64)) and torch.equal(s.stdev, torch.full((162,), 0.1, dtype=torch.float64))
    assert not s.p_sigma.any() and not s.p_c.any()
    with pytest.raises(RuntimeError, match='before ask'):
        s.tell(torch.zeros((3, 19), dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------- weights and constants
def test_constants_two_replicas_one_parameter_by_hand():
    """λ = 2, d = 1: w' = (ln 1.5, ln 0.75), μ = 1, w_1 = 1, μ_eff = μ_eff⁻ = 1; c_σ = 3/7, d_σ = 10/7, c_c = 3/4, c_1 = 1/4,
    c_μ = min(3/4, 0.25/5.5) = 1/22, χ_1 = 67/84; α_μ⁻ = 6.5, α_μeff⁻ = 5/3, α_posdef⁻ = 15.5 -> w_2 = −5/3."""
    k = M.constants(2, 1)
    assert k['mu'] == 1 and k['mu_eff'] == 1.0 and k['mu_eff_minus'] == 1.0
    for name, want in (('c_sigma', 3 / 7), ('d_sigma', 10 / 7), ('c_c', 3 / 4), ('c_1', 1 / 4), ('c_mu', 1 / 22), ('chi_d', 67 / 84)):
        assert k[name] == pytest.approx(want, rel=1e-15, abs=0), name
    assert k['weights'][0] == 1.0 and k['weights'][1] == pytest.approx(-5 / 3, rel=1e-15)
    assert M.constants(2, 1, M.Config(active=False))['weights'].tolist() == [1.0, 0.0]


@pytest.mark.parametrize('lam, pinned', [
    (10, dict(mu=5, mu_eff=3.1672992814107017, mu_eff_minus=3.989115019106924, c_sigma=0.030365994543201782,
              d_sigma=1.0303659945432018, c_c=0.08030284357461202, c_1=0.0053340332907040825, c_mu=0.008079549413705334,
              chi_d=12.708303300804651, w0=0.45627264690340597, w_last=-0.2512995962545942)),
    (19, dict(mu=9, mu_eff=5.647567327551322, mu_eff_minus=7.481941489259823, c_sigma=0.04429583020444281,
              d_sigma=1.0442958302044427, c_c=0.08130655792951193, c_1=0.005333597719077364, c_mu=0.0188871801207932,
              chi_d=12.708303300804651, w0=0.2906776508585161, w_last=-0.058280819745540474)),
])
def test_constants_at_162_parameters(lam, pinned):
    """The reference agent's 162 parameters at the reference's popsize 10 and at the default 4 + ⌊3 ln 162⌋ = 19 (odd: rank
    10's w' = ln 10 − ln 10 is exactly 0, and stays 0).  Each value is restated from its formula, then pinned."""
    d, k = 162.0, M.constants(lam, 162)
    mu = lam // 2
    wp = [math.log((lam + 1) / 2) - math.log(j) for j in range(1, lam + 1)]
    wpos = [v / math.fsum(wp[:mu]) for v in wp[:mu]]
    mu_eff = 1 / math.fsum(v * v for v in wpos)
    neg = wp[mu:]
    mu_eff_minus = math.fsum(neg) ** 2 / math.fsum(v * v for v in neg)
    c_1 = 1 / (d + 2 * math.sqrt(d) + mu_eff / d)
    c_mu = min(1 - c_1, (0.25 + mu_eff + 1 / mu_eff - 2) / (d + 4 * math.sqrt(d) + mu_eff / 2))
    alpha = min(1 + c_1 / c_mu, 1 + 2 * mu_eff_minus / (mu_eff + 2), (1 - c_1 - c_mu) / (d * c_mu))
    assert alpha == pytest.approx((1 - c_1 - c_mu) / (d * c_mu), rel=1e-15)      # positive definiteness binds at d = 162
    want_w = wpos + [v * alpha / math.fsum(abs(u) for u in neg) for v in neg]
    assert np.allclose(k['weights'], want_w, rtol=1e-14, atol=0)
    assert math.fsum(k['weights'][:mu]) == pytest.approx(1.0, rel=1e-15)
    assert math.fsum(k['weights'][mu:]) == pytest.approx(-alpha, rel=1e-14)
    assert k['mu'] == pinned['mu']
    for name in ('mu_eff', 'mu_eff_minus', 'c_sigma', 'd_sigma', 'c_c', 'c_1', 'c_mu', 'chi_d'):
        assert k[name] == pytest.approx(pinned[name], rel=1e-13, abs=0), name
    assert k['weights'][0] == pytest.approx(pinned['w0'], rel=1e-13) and k['weights'][-1] == pytest.approx(pinned['w_last'], rel=1e-13)
    if lam % 2:
        assert k['weights'][mu] == 0.0
    assert not M.constants(lam, 162, M.Config(active=False))['weights'][mu:].any()
    # the searcher's constants (die_amd.search.cmaes_constants, what the device gets) are the model's
    from die_amd.search import cmaes_constants
    got = cmaes_constants(lam, 162)
    assert np.allclose(got['weights'], k['weights'], rtol=1e-14, atol=1e-17)
    for name in ('mu_eff', 'mu_eff_minus', 'c_sigma', 'd_sigma', 'c_c', 'c_1', 'c_mu', 'chi_d'):
        assert got[name] == pytest.approx(k[name], rel=1e-14), name


def test_ratios_scale_their_constant():
    base = M.constants(10, 162)
    k = M.constants(10, 162, M.Config(c_sigma_ratio=0.5, damp_sigma_ratio=2.0, c_c_ratio=0.25, c_1_ratio=0.5, c_mu_ratio=0.5))
    assert k['c_sigma'] == pytest.approx(0.5 * base['c_sigma'], rel=1e-15)
    assert k['d_sigma'] == pytest.approx(2.0 * (base['d_sigma'] - base['c_sigma'] + k['c_sigma']), rel=1e-15)
    assert k['c_c'] == pytest.approx(0.25 * base['c_c'], rel=1e-15)
    assert k['c_1'] == pytest.approx(0.5 * base['c_1'], rel=1e-15)
    assert k['c_mu'] == pytest.approx(0.5 * base['c_mu'], rel=1e-15)


# ---------------------------------------------------------------------------------------------------- the model, by hand
def test_model_one_generation_two_replicas_by_hand():
    """λ = 2, d = 1, m = 0.5, σ = 0.25, C = 1, f = (1, 3): rank 1 is replica 1, so y_w = z_w = z_1 and m' = 0.5 + 0.25·z_1;
    p_σ = sqrt(c_σ(2 − c_σ))·z_1 = (√33/7)·z_1, whose normalised length is |z_1| (below 2.4·χ_1: h_σ = 1);
    p_c = sqrt(c_c(2 − c_c))·z_1 = (√15/4)·z_1; the active weight −5/3 gives w°_2 = −(5/3)/z_0², so
    C' = (1 − c_1 − c_μ(1 − 5/3)) + c_1·p_c² + c_μ(z_1² − 5/3) = 3/4 − 1/22 + (15/64 + 1/22)·z_1²;
    σ' = 0.25·exp(0.3·((√33/7)·|z_1|·84/67 − 1)) (c_σ/d_σ = 0.3, the raw ‖p_σ‖ over χ_1)."""
    seed = 3
    st = M.State([0.5], 0.25, 2, seed=seed)
    rows = M.sample(st, 0)
    z = M.noise(seed, 0, 2, 1)[:, 0]
    assert rows.tolist() == [[f32(0.5 + 0.25 * z[0])], [f32(0.5 + 0.25 * z[1])]]
    out = M.update(st, rows, np.array([[1.0, 3.0]]), 0)
    z1 = z[1]
    assert abs(z1) < 2.4 * 67 / 84 and out.h_sigma == [1.0]
    assert out.order.tolist() == [1, 0] and out.fitness.tolist() == [1.0, 3.0]
    assert out.pop_best.tolist() == rows[1].tolist() and out.best.tolist() == rows[1].tolist() and out.evals.tolist() == [3.0, 3.0]
    assert out.m[0] == pytest.approx(0.5 + 0.25 * z1, rel=1e-15)
    assert out.ps[0] == pytest.approx(math.sqrt(33) / 7 * z1, rel=1e-14)
    assert out.pc[0] == pytest.approx(math.sqrt(15) / 4 * z1, rel=1e-14)
    assert out.C[0] == pytest.approx(3 / 4 - 1 / 22 + (15 / 64 + 1 / 22) * z1 * z1, rel=1e-14)
    assert out.sigma == pytest.approx(0.25 * math.exp(0.3 * (math.sqrt(33) / 7 * abs(z1) * 84 / 67 - 1)), rel=1e-14)
    h = out.history[0]
    assert h[:4].tolist() == [2.0, 3.0, 1.0, 2.0] and h[4] == out.sigma
    assert h[5] == pytest.approx(out.sigma * math.sqrt(out.C[0]), rel=1e-15)
    # not active: the second rank has weight 0, C' = 3/4 + (15/64)·z_1² (the rank-μ term is c_μ·z_1²  minus c_μ·1)
    na = M.update(M.State([0.5], 0.25, 2, seed=seed, cfg=M.Config(active=False)), rows, np.array([[1.0, 3.0]]), 0)
    assert na.C[0] == pytest.approx(1 - 1 / 4 - 1 / 22 + (15 / 64 + 1 / 22) * z1 * z1, rel=1e-14)
    # csa_squared: σ' = 0.25·exp((c_σ/(2 d_σ))(p_σ² − 1)) = 0.25·exp(0.15·(33 z_1²/49 − 1))
    sq = M.update(M.State([0.5], 0.25, 2, seed=seed, cfg=M.Config(csa_squared=True)), rows, np.array([[1.0, 3.0]]), 0)
    assert sq.sigma == pytest.approx(0.25 * math.exp(0.15 * (33 * z1 * z1 / 49 - 1)), rel=1e-14)
    # a worse generation: pop_best follows it, best stays
    rows2 = M.sample(out, 1)
    out2 = M.update(out, rows2, np.array([[0.5, -1.0]]), 1)
    assert out2.order.tolist() == [0, 1] and out2.pop_best.tolist() == rows2[0].tolist()
    assert out2.best.tolist() == rows[1].tolist() and out2.evals.tolist() == [0.5, 3.0]


def test_model_ranks_descending_ties_to_lower_index_and_median():
    f = np.array([2.0, 2.0, 1.0, 3.0, 2.0])
    assert M.ranking(f).tolist() == [3, 0, 1, 4, 2]
    st = M.State(np.zeros(3), 0.5, 5)
    out = M.update(st, M.sample(st, 0), f[None, :], 0)
    assert out.history[0][:4].tolist() == [2.0, 3.0, 1.0, 2.0]                # odd λ: the middle value
    assert np.array_equal(out.pop_best, M.sample(st, 0)[3])


def test_model_sample_is_philox_stream_9():
    st = M.State(np.linspace(-1, 1, 7), 0.3, 5, seed=123)
    st.C = np.linspace(0.5, 2.0, 7)
    rows = M.sample(st, 4)
    from oracle.rng import normals2
    z = normals2(123, 4, 35, stream=9, scale=1.0)[0].reshape(5, 7)
    assert np.array_equal(rows, (st.m + (0.3 * np.sqrt(st.C)) * z).astype(f32))
    assert not np.array_equal(rows, M.sample(st, 5))


def _c0(P, seed):
    return (-0.5 + torch.rand(P, generator=torch.Generator().manual_seed(seed))).double().numpy()


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_model_minimises_the_sphere(seed):
    P = M.SPHERE_P
    R = 4 + int(math.floor(3 * math.log(P)))
    c0 = _c0(P, seed)
    st = M.run(M.State(c0, M.SPHERE_SIGMA, R, seed=seed), M.sphere, M.SPHERE_GENERATIONS)
    ratio = np.linalg.norm(st.m) / np.linalg.norm(c0)
    assert ratio < 0.01 < M.SPHERE_RATIO, ratio
    h = np.array(st.history)
    assert h.shape == (M.SPHERE_GENERATIONS, 6) and h[-1, 0] > h[0, 0] and h[-1, 4] < M.SPHERE_SIGMA


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_model_adapts_the_covariance_on_the_ellipsoid(seed):
    """f = −Σ 10^(3p/(d−1))·x_p², d = 10: C learns the inverse scales (C_0/C_9 -> about 1000) and f drops by orders of
    magnitude; the thresholds the GPU run must meet are pinned in tests/cmaes_model.py."""
    d = M.ELLIPSOID_D
    c0 = _c0(d, seed)
    st = M.run(M.State(c0, M.ELLIPSOID_SIGMA, M.ELLIPSOID_R, seed=seed), M.ellipsoid, M.ELLIPSOID_GENERATIONS)
    cond = st.C[0] / st.C[-1]
    gain = M.ellipsoid(c0[None])[0] / M.ellipsoid(st.m[None])[0]
    assert cond > 5 * M.ELLIPSOID_COND and gain > 100 * M.ELLIPSOID_GAIN, (cond, gain)
    assert np.all(np.diff(np.log(st.C)) < 0.5)                              # roughly decreasing along p
    no_active = M.run(M.State(c0, M.ELLIPSOID_SIGMA, M.ELLIPSOID_R, seed=seed, cfg=M.Config(active=False)), M.ellipsoid,
                      M.ELLIPSOID_GENERATIONS)
    assert no_active.C[0] / no_active.C[-1] > M.ELLIPSOID_COND
