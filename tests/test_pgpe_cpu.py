"""PGPE search (die_pgpe_sample / die_pgpe_update, die_amd.search.PGPE), CPU side: the library exports both entry points and
the state struct matches its header field list, every bad argument is refused on the host before any launch, and the float64
model of tests/pgpe_model.py is pinned on hand-computed cases and minimises the sphere the GPU suite uses.  No kernel is
launched here."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import pgpe_model as M

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
    for name in ('die_pgpe_sample', 'die_pgpe_update'):
        assert hasattr(so, name) and name in lib.EXPORTS
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    # die_pgpe: replicas, optimizer (2 x i32), num_params i64, seed u64, ten doubles, nine pointers, history_rows i64, work
    assert C.sizeof(lib.Pgpe) == 2 * 4 + 8 + 8 + 10 * 8 + 9 * 8 + 8 + 8
    assert lib.pgpe_work_doubles(162) == 4 * 256 + 162
    import die_amd
    assert die_amd.PGPE is die_amd.search.PGPE


FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host


def _state(lib, **kw):
    f = dict(replicas=10, optimizer=lib.DIE_PGPE_CLIPUP, num_params=162, seed=0, center_lr=0.05, stdev_lr=0.1, max_speed=0.1,
             momentum=0.9, beta1=0.9, beta2=0.999, eps=1e-8, stdev_max_change=0.2, stdev_min=-math.inf, stdev_max=math.inf,
             center=FAKE, stdev=FAKE, opt_a=FAKE, opt_b=FAKE, pop_best=FAKE, best=FAKE, fitness=FAKE, evals=FAKE, history=FAKE,
             history_rows=64, work=FAKE)
    f.update(kw)
    return lib.Pgpe(**f)


def _refused(lib, fn, *args, match):
    rc = getattr(lib.lib, fn)(*args)
    assert rc == -1, (fn, rc)
    msg = lib.lib.die_last_error().decode()
    assert match in msg, msg


@pytest.mark.parametrize('kw, match', [
    (dict(replicas=9), 'replicas 9: an even number'),
    (dict(replicas=0), 'replicas 0'),
    (dict(replicas=66), 'replicas 66'),
    (dict(num_params=0), 'num_params 0'),
    (dict(optimizer=7), 'unknown optimizer 7'),
    (dict(center_lr=0.0), 'center_lr 0: must be positive'),
    (dict(stdev_lr=-0.1), 'stdev_lr -0.1: must be positive'),
    (dict(max_speed=0.0), 'max_speed 0: must be positive'),
    (dict(momentum=1.0), 'momentum 1'),
    (dict(optimizer=1, eps=0.0), 'Adam eps 0'),
    (dict(optimizer=1, beta2=1.0), 'Adam betas'),
    (dict(stdev_min=2.0, stdev_max=1.0), 'stdev_min 2 above stdev_max 1'),
    (dict(center=None), 'null state buffer'),
    (dict(work=None), 'null state buffer'),
    (dict(optimizer=1, opt_b=None), 'null state buffer'),
])
def test_bad_state_refused_by_both_entry_points(lib, kw, match):
    s = _state(lib, **kw)
    _refused(lib, 'die_pgpe_sample', C.byref(s), FAKE, 0, None, match=match)
    _refused(lib, 'die_pgpe_update', C.byref(s), FAKE, FAKE, 30, 20, 2, 0, None, match=match)


def test_bad_call_arguments_refused(lib):
    s = _state(lib)
    _refused(lib, 'die_pgpe_sample', None, FAKE, 0, None, match='null state')
    _refused(lib, 'die_pgpe_sample', C.byref(s), None, 0, None, match='null parameter matrix')
    _refused(lib, 'die_pgpe_sample', C.byref(s), FAKE, -1, None, match='generation -1')
    _refused(lib, 'die_pgpe_sample', C.byref(s), FAKE, 1 << 32, None, match='generation 4294967296')
    up = lambda *a: _refused(lib, 'die_pgpe_update', *a[:-1], match=a[-1])
    up(None, FAKE, FAKE, 30, 20, 2, 0, None, 'null state')
    up(C.byref(s), None, FAKE, 30, 20, 2, 0, None, 'null parameter matrix or terms')
    up(C.byref(s), FAKE, None, 30, 20, 2, 0, None, 'null parameter matrix or terms')
    up(C.byref(s), FAKE, FAKE, 0, 20, 2, 0, None, 'T 0')
    up(C.byref(s), FAKE, FAKE, 30, 0, 2, 0, None, 'strides (0, 2) must be positive')
    up(C.byref(s), FAKE, FAKE, 30, 20, -2, 0, None, 'strides (20, -2) must be positive')
    up(C.byref(s), FAKE, FAKE, 30, 20, 2, 64, None, 'generation 64 beyond the 64 history rows')


def test_searcher_refusals_and_initial_state_without_gpu(lib):
    from die_amd.search import PGPE
    kw = dict(center_learning_rate=0.05, stdev_learning_rate=0.1, device='cpu')
    with pytest.raises(ValueError, match='popsize 9'):
        PGPE(9, 162, radius_init=1.5, **kw)
    with pytest.raises(ValueError, match='popsize 66'):
        PGPE(66, 162, radius_init=1.5, **kw)
    with pytest.raises(ValueError, match='radius_init 0'):
        PGPE(10, 162, radius_init=0.0, **kw)
    with pytest.raises(ValueError, match='exactly one of radius_init and stdev_init'):
        PGPE(10, 162, **kw)
    with pytest.raises(ValueError, match='optimizer'):
        PGPE(10, 162, radius_init=1.5, optimizer='cmaes', **kw)
    with pytest.raises(ValueError, match='unknown keys'):
        PGPE(10, 162, radius_init=1.5, optimizer_config=dict(speed=1.0), **kw)
    s = PGPE(10, 162, radius_init=1.5, seed=5, **kw)           # NEProblem(initial_bounds=(-0.5, 0.5)), radius_init -> stdev
    want = -0.5 + torch.rand(162, generator=torch.Generator().manual_seed(5), dtype=torch.float32)
    assert torch.equal(s.center, want)
    assert torch.equal(s.stdev, torch.full((162,), math.sqrt(1.5 ** 2 / 162), dtype=torch.float32))
    assert s.R == 10 and s.P == 162 and s.iter == 0


# ---------------------------------------------------------------------------------------------------- the model, by hand
def _state_model(center, stdev, R, **cfg):
    return M.State(np.array(center, f32), np.array(stdev, f32), R, cfg=M.Config(**cfg))


def test_model_two_replicas_by_hand():
    """R = 2, P = 1: rows c ± 0.125 with c = 0.5, σ = 0.25; f = (1, 3) -> u = (−0.5, 0.5), g_μ = 0.125·(−1)/2 = −0.0625,
    g_σ = 0 (the pair's mean rank is 0); ClipUp: ĝ = −1, v = 0.05·ĝ (below max_speed), c = 0.45; pop_best = best = row 1."""
    st = _state_model([0.5], [0.25], 2)
    rows = np.array([[0.625], [0.375]], f32)
    out = M.update(st, rows, np.array([[1.0, 3.0]]), 0)
    assert out.fitness.tolist() == [1.0, 3.0]
    assert out.center[0] == f32(0.5 - 0.05) and out.opt_a[0] == f32(-0.05) and out.stdev[0] == f32(0.25)
    assert out.pop_best.tolist() == [f32(0.375)] and out.best.tolist() == [f32(0.375)] and out.evals.tolist() == [3.0, 3.0]
    assert out.history[0].tolist() == [2.0, 3.0, 1.0, 2.0, 0.0625, 0.25]
    # the next generation is worse: pop_best follows it, best stays
    out2 = M.update(out, np.array([[0.25], [0.5]], f32), np.array([[0.5], [-1.0]]).T, 1)
    assert out2.pop_best.tolist() == [f32(0.25)] and out2.best.tolist() == [f32(0.375)] and out2.evals.tolist() == [0.5, 3.0]


def test_model_ties_rank_by_replica_index():
    f = np.array([2.0, 2.0, 1.0, 2.0])
    assert M.centred_ranks(f).tolist() == [1 / 3 - 0.5, 2 / 3 - 0.5, -0.5, 0.5]
    rows = np.arange(8, dtype=f32).reshape(4, 2)
    out = M.update(_state_model([0, 0], [1, 1], 4), rows, f[None, :], 0)
    assert np.array_equal(out.pop_best, rows[0]) and out.evals[0] == 2.0          # the first of the tied maxima
    assert out.history[0][:4].tolist() == [7 / 4, 2.0, 1.0, 2.0]


def test_model_clipup_at_and_above_max_speed():
    """P = 1, c = 0, σ = 1, rows ±0.5 with the + row fitter: ĝ = +1.  At: α = 0.1, no momentum -> |v| = max_speed exactly, no
    clip.  Above: α = 0.25 -> clipped to 0.1; and momentum 0.9 on a stored 0.1 plus α = 0.1 -> 0.19…, clipped to 0.1."""
    rows, terms = np.array([[0.5], [-0.5]], f32), np.array([[3.0, 1.0]])
    at = M.update(_state_model([0], [1], 2, center_lr=0.1, momentum=0.0), rows, terms, 0)
    assert at.opt_a[0] == f32(0.1) and at.center[0] == f32(0.1)
    above = M.update(_state_model([0], [1], 2, center_lr=0.25, momentum=0.0), rows, terms, 0)
    assert above.opt_a[0] == f32(0.1) and above.center[0] == f32(0.1)
    st = _state_model([0], [1], 2, center_lr=0.1, momentum=0.9)
    st.opt_a[0] = f32(0.1)
    mom = M.update(st, rows, terms, 0)
    v = 0.9 * float(f32(0.1)) + 0.1
    assert v > 0.1 and mom.opt_a[0] == f32(v * 0.1 / v) and mom.center[0] == f32(v * 0.1 / v)
    half = M.update(_state_model([0], [1], 2, center_lr=0.05, momentum=0.0), rows, terms, 0)
    assert half.opt_a[0] == f32(0.05)                                               # below: untouched


def test_model_stdev_clamp_on_both_sides():
    """R = 4, P = 2, c = 0, σ = 1: f = (3, 4, 1, 2) -> u = (1/6, 1/2, −1/2, −1/6), mean ranks of the pairs ±1/3.  Pair 0 moves
    only p0 (ε̃ = 3), pair 1 only p1: g_σ = ((1/3)·8 + (−1/3)·(−1))/2 = 1.5 for p0 and −1.5 for p1.  With stdev_lr = 1:
    σ' = 2.5 and −0.5, clamped to 1.2 and 0.8 (δ = 0.2), then to [0.9, 1.1] by stdev_min / stdev_max; no δ: 2.5 and −0.5
    (the absolute clamp alone: 2.0 and 0.5)."""
    rows = np.array([[3, 0], [-3, 0], [0, 3], [0, -3]], f32)
    terms = np.array([[3.0, 4.0, 1.0, 2.0]])
    u = M.centred_ranks(terms[0])
    assert np.allclose(u, [1 / 6, 1 / 2, -1 / 2, -1 / 6], rtol=0, atol=1e-15)
    st = _state_model([0, 0], [1, 1], 4, stdev_lr=1.0)
    _, gs = M.gradients(st, rows, u)
    assert np.allclose(gs, [1.5, -1.5], rtol=1e-15)
    assert M.update(st, rows, terms, 0).stdev.tolist() == [f32(1.2), f32(0.8)]
    st.cfg.stdev_min, st.cfg.stdev_max = 0.9, 1.1
    assert M.update(st, rows, terms, 0).stdev.tolist() == [f32(1.1), f32(0.9)]
    st.cfg.stdev_max_change, st.cfg.stdev_min, st.cfg.stdev_max = None, None, None
    assert np.allclose(M.update(st, rows, terms, 0).stdev, [2.5, -0.5], rtol=1e-6)
    st.cfg.stdev_min, st.cfg.stdev_max = 0.5, 2.0
    assert M.update(st, rows, terms, 0).stdev.tolist() == [f32(2.0), f32(0.5)]


def test_model_adam_first_step():
    """Adam's first step: m = (1 − β1)·g, v = (1 − β2)·g², bias-corrected to g and g², so the centre moves by
    lr·g_μ/(|g_μ| + eps) — lr in the ascent direction (torch.optim.Adam on the loss −f)."""
    st = _state_model([0.5], [0.25], 2, optimizer='adam')
    out = M.update(st, np.array([[0.625], [0.375]], f32), np.array([[1.0, 3.0]]), 0)
    g = 0.0625                                                                      # the loss gradient −g_μ
    assert out.opt_a[0] == f32(0.1 * g) and out.opt_b[0] == f32(0.001 * g * g)
    m_hat, v_hat = (0.1 * g) / 0.1, (0.001 * g * g) / 0.001
    assert abs(float(out.center[0]) - (0.5 - 0.05 * m_hat / (math.sqrt(v_hat) + 1e-8))) <= 3e-8
    assert out.center[0] == f32(0.5 - (0.05 / (1 - 0.9)) * ((0.1 * g) / (math.sqrt(0.001 * g * g) / math.sqrt(1 - 0.999) + 1e-8)))


def test_model_sample_is_symmetric_philox():
    st = _state_model(np.linspace(-1, 1, 7), np.linspace(0.1, 0.7, 7), 6)
    st.seed = 123
    rows = M.sample(st, 4)
    z = M.noise(123, 4, 3, 7)
    from oracle.rng import normals2
    assert np.array_equal(z[1], normals2(123, 4, 21, stream=8, scale=1.0)[0][7:14])
    e = st.stdev.astype(np.float64) * z
    assert np.array_equal(rows[0::2], (st.center + e).astype(f32)) and np.array_equal(rows[1::2], (st.center - e).astype(f32))
    assert not np.array_equal(rows, M.sample(st, 5))


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_model_minimises_the_sphere(seed):
    """The reference's hyperparameters on the 162-parameter sphere: the calibration of tests/test_gpu_pgpe.py's threshold."""
    P = M.SPHERE_P
    c0 = (-0.5 + torch.rand(P, generator=torch.Generator().manual_seed(seed))).numpy()
    st = M.State(c0, np.full(P, math.sqrt(1.5 ** 2 / P), f32), M.SPHERE_R, seed=seed)
    for g in range(M.SPHERE_GENERATIONS):
        rows = M.sample(st, g)
        st = M.update(st, rows, -np.sum(rows.astype(np.float64) ** 2, axis=1)[None, :], g)
    ratio = np.linalg.norm(st.center.astype(np.float64)) / np.linalg.norm(c0.astype(np.float64))
    assert ratio < 0.4 < M.SPHERE_RATIO, ratio
    h = np.array(st.history)
    assert h.shape == (M.SPHERE_GENERATIONS, 6) and h[-1, 0] > h[0, 0]
