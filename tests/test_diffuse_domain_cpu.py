"""The diffusion domain cases (tests/diffuse_domain_cases.py), CPU side: an fp32 emulation of the kernels' arithmetic stays inside
every case's bound against the float64 oracle — so a GPU failure accuses the kernel, not the bound or the inputs —, the oracle is the
explicit periodic sum where the field is narrower than the radius, and die_diffuse_decay / die_diffuse_decay_mode refuse bad
arguments on the host (fake pointers: a launch would have failed).  No kernel is launched."""
import math
import os

import numpy as np
import pytest

from oracle import cpu_ref as R
from tests import diffuse_domain_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host
ARG, UNSUPPORTED = -1, -3


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


# ---- the cases themselves
def test_the_cases_span_the_template_grid():
    cases = D.direct_cases()
    rows = {(c['dtype'], D.radius(c['sigma'])) for c in cases if D.takes_row_sweep(*c['shape'], c['sigma'], c['mode'])}
    lds = {(c['dtype'], D.radius(c['sigma']), c['mode']) for c in cases if not D.takes_row_sweep(*c['shape'], c['sigma'], c['mode'])}
    assert rows == {(t, r) for t in ('f32', 'f16') for r in (1, 2, 3, 4)}
    assert lds == {(t, r, m) for t in ('f32', 'f16') for r in range(1, 9) for m in D.MODES}
    assert [D.radius(s) for s in D.ROWS_SIGMAS] == [1, 2, 3, 4, 4] and [D.radius(s) for s in D.LDS_SIGMAS] == list(range(1, 9))
    assert [D.radius(s) for s in D.STEP_SIGMAS] == [1, 4] and [D.radius(s) for s in D.BATCH_SIGMAS] == [1, 2, 3, 4]
    # the sigmas on the rounding edge are exact in fp32 and land on it: 4 sigma + .5 is the integer itself
    assert 4.0 * float(np.float32(0.375)) + 0.5 == 2.0 and 4.0 * float(np.float32(0.875)) + 0.5 == 4.0
    # every group 1 shape takes the row sweep, every group 3 shape the LDS kernel except (16, 256) under wrap below sigma 1.2
    assert all(D.takes_row_sweep(W, H, s) for W, H in D.ROWS_SHAPES for s in D.ROWS_SIGMAS)
    for W, H in D.LDS_SHAPES:
        for s in D.LDS_SIGMAS:
            assert D.takes_row_sweep(W, H, s) == ((W, H) == (16, 256) and s < 1.2)
    for W, H, rpw in D.RAGGED_SHAPES:
        assert D.rows_per_wave(W, H) == rpw and W % rpw == 3 and D.rows_per_wave(W - 4, H) == rpw // 2
    assert all(D.rows_per_wave(W, H) == 2 and W % 2 == 1 for W, H in D.ROWS_SHAPES)
    # the strip and workgroup edges of the row sweep: 248 columns a strip, two strips a workgroup
    strips = [-(-H // 248) for _, H in D.ROWS_SHAPES]
    assert strips == [1, 1, 1, 2, 3] and (252 - 248) // 4 == 1


def test_inputs_are_what_the_module_says():
    for dtype in ('f32', 'f16'):
        for scale in (1.0,) if dtype == 'f32' else D.F16_SCALES:
            chem, want = D.inputs(17, 257, dtype, scale, 0.8, 'wrap')
            assert chem.dtype == D.np_dtype(dtype) and want.dtype == np.float64
            dense = float((chem > 0).mean())
            assert 0.5 < dense < 0.7 and chem.min() >= 0 and np.isfinite(want).all()
            if scale < 1e-4:                                     # subnormal halves, in and out, and not all flushed by numpy
                tiny = float(np.finfo(np.float16).tiny)
                assert 0 < chem.max() < tiny and want.max() < tiny and (chem > 0).sum() > 1000
                assert len(np.unique(chem)) > 50
    b16 = D.bound(np.array([0.0, 3e-6, 1.0, 1.5, 300.0]), 'f16')
    ulp = [2.0 ** -24, 2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -2]
    assert np.allclose(b16, [0.5 * u + 1e-5 * w + 1e-7 for u, w in zip(ulp, [0.0, 3e-6, 1.0, 1.5, 300.0])], rtol=1e-12, atol=0)
    assert D.ratio(np.array([np.nan]), np.array([1.0]), 'f32') == math.inf


# ---- the emulation is inside every bound
GROUPS = [('rows', dt) for dt in ('f32', 'f16')] + [('lds', dt) for dt in ('f32', 'f16')]


@pytest.mark.parametrize('group,dtype', GROUPS)
def test_emulation_is_inside_the_bound(group, dtype):
    worst = {}
    for c in D.direct_cases():
        if c['group'] != group or c['dtype'] != dtype:
            continue
        W, H = c['shape']
        chem, want = D.inputs(W, H, dtype, c['scale'], c['sigma'], c['mode'])
        for fma in (False, True):
            got = D.emulate(chem, c['sigma'], D.DECAY, c['mode'], dtype, fma=fma)
            assert got.dtype == chem.dtype and got.shape == chem.shape
            r = D.ratio(got, want, dtype)
            key = (c['mode'], c['scale'])
            worst[key] = max(worst.get(key, 0.0), r)
            assert r <= 1.0, (c, fma, r)
    for (mode, scale), r in sorted(worst.items()):
        print(f'diffuse domain {group} {dtype} {mode} scale {scale:g}: emulation worst error / bound {r:.3f}')
    assert worst


@pytest.mark.parametrize('W,H,rpw', D.RAGGED_SHAPES)
def test_emulation_is_inside_the_bound_on_the_ragged_fields(W, H, rpw):
    chem, want = D.inputs.__wrapped__(W, H, 'f32', 1.0, D.RAGGED_SIGMA, 'wrap')
    r = D.ratio(D.emulate(chem, D.RAGGED_SIGMA, D.DECAY, 'wrap', 'f32'), want, 'f32')
    print(f'diffuse domain ragged f32 {W}x{H} rpw {rpw}: emulation worst error / bound {r:.3f}')
    assert r <= 1.0


def test_the_bound_is_not_slack():
    """One fp16 ulp off breaks the fp16 bound, at both scales; 3e-5 relative, or the outermost tap pair of R = 3 left out of one
    axis (2 * 4.4e-4 of a neighbour), breaks the fp32 one: the bounds would see a kernel that is subtly wrong."""
    chem, want = D.inputs(17, 257, 'f16', 1.0, 0.8, 'reflect')
    got = D.emulate(chem, 0.8, D.DECAY, 'reflect', 'f16').astype(np.float64)
    assert D.ratio(got + np.spacing(got.astype(np.float16)).astype(np.float64), want, 'f16') > 1.0
    # (among subnormal halves the 1e-7 of the fp32 bound is two of their ulps; what that scale is for is a flush to zero)
    chem, want = D.inputs(17, 257, 'f16', 6e-6, 0.8, 'reflect')
    assert D.ratio(np.zeros_like(want), want, 'f16') > 10.0
    chem, want = D.inputs(17, 257, 'f32', 1.0, 0.8, 'wrap')
    got = D.emulate(chem, 0.8, D.DECAY, 'wrap', 'f32').astype(np.float64)
    assert D.ratio(got * (1 + 3e-5), want, 'f32') > 1.0
    w = D.taps_f32(0.8)
    short = w.copy()
    short[0] = short[-1] = 0
    x = chem.astype(np.float32)
    got = D._pass(D._pass(x, w, 0, 'wrap', False), short, 1, 'wrap', False) * np.float32(0.9)
    assert D.ratio(got, want, 'f32') > 10.0


# ---- the oracle below the radius
@pytest.mark.parametrize('W,H', [(1, 4), (3, 4), (2, 8), (3, 8)])
@pytest.mark.parametrize('sigma', [0.875, 1.0])
def test_oracle_is_the_explicit_sum_below_the_radius(W, H, sigma):
    chem = np.random.RandomState(W * 10 + H).rand(W, H)
    s, d = float(np.float32(sigma)), float(np.float32(D.DECAY))
    assert W < D.radius(sigma)
    assert np.abs(R.diffuse_decay(chem, s, d) - R.diffuse_decay_explicit(chem, s, d)).max() <= 1e-15


# ---- the host refusals
def _call(lib, *, entry='die_diffuse_decay', src=FAKE, dst=FAKE + 65536, W=24, H=40, dtype=0, sigma=0.8, decay=0.1, mode=0):
    if entry == 'die_diffuse_decay':
        return lib.lib.die_diffuse_decay(src, dst, W, H, dtype, sigma, decay, None)
    return lib.lib.die_diffuse_decay_mode(src, dst, W, H, dtype, sigma, decay, mode, None)


REFUSALS = [
    ('null src', dict(src=None), ARG, b'distinct non-null planes'),
    ('null dst', dict(dst=None), ARG, b'distinct non-null planes'),
    ('in place', dict(dst=FAKE), ARG, b'distinct non-null planes'),
    ('W 0', dict(W=0), ARG, b'bad size 0x40'),
    ('H 0', dict(H=0), ARG, b'bad size 24x0'),
    ('W negative', dict(W=-3), ARG, b'bad size -3x40'),
    ('dtype 2', dict(dtype=2), ARG, b'bad dtype 2'),
    ('dtype -1', dict(dtype=-1), ARG, b'bad dtype -1'),
    ('sigma 0', dict(sigma=0.0), ARG, b'sigma must be positive'),
    ('sigma negative', dict(sigma=-0.8), ARG, b'sigma must be positive'),
    ('sigma nan', dict(sigma=math.nan), ARG, b'sigma must be positive'),
    ('radius 0', dict(sigma=0.124), ARG, b'gives an empty kernel'),
    ('radius 9', dict(sigma=2.125), UNSUPPORTED, b'needs radius 9 > 8'),
    ('sigma inf', dict(sigma=math.inf), UNSUPPORTED, b'sigma inf needs radius'),
    ('sigma 1e30', dict(sigma=1e30), UNSUPPORTED, b'sigma 1e+30 needs radius'),
]


@pytest.mark.parametrize('entry', ['die_diffuse_decay', 'die_diffuse_decay_mode'])
@pytest.mark.parametrize('case,kw,status,needle', REFUSALS)
def test_bad_arguments_refused_before_launch(lib, entry, case, kw, status, needle):
    assert _call(lib, entry=entry, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error(), (case, lib.lib.die_last_error())
    assert lib.lib.die_last_error().startswith(b'die_diffuse_decay: ')


@pytest.mark.parametrize('mode', [-1, 5])
def test_a_mode_outside_the_enum_is_refused(lib, mode):
    assert _call(lib, entry='die_diffuse_decay_mode', mode=mode) == ARG
    assert b'bad boundary mode %d' % mode in lib.lib.die_last_error()


def test_the_radius_of_a_huge_sigma_saturates(lib):
    """(int)(4 sigma + .5) is undefined beyond int's range; the library compares in double before the cast, so that inf and 1e30
    are refused as too LARGE — by rule, not by what the conversion happens to give — and name a radius above the limit."""
    for sigma in (math.inf, 1e30, 1e10):
        assert _call(lib, sigma=sigma) == UNSUPPORTED
        assert lib.lib.die_last_error().endswith(b'needs radius 2147483647 > 8'), lib.lib.die_last_error()
