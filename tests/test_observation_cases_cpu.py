"""The observation cases (tests/observation_cases.py), CPU side: the float64 models against scipy, matplotlib, numpy and the
oracle, the conditions on the inputs that make exact comparisons on the device legitimate, and — part 6 — every model run with one
planted error at a time: the case list tells each of them from the true model.  No kernel is launched."""
import numpy as np
import pytest

from oracle import cpu_ref as R
from tests import observation_cases as O


# ---------------------------------------------------------------------------------------------------------------- sense mask
def test_the_sense_cases_span_the_domain():
    cases = O.sense_cases()
    assert [O.sense_radius(s) for s in O.SM_SIGMAS] == list(O.SM_RADII)
    # the rounding edges of int(4 sigma + .5), on the fp32 values the entry gets
    assert 4.0 * float(np.float32(0.125)) + 0.5 == 1.0 and O.sense_radius(O.below32(0.125)) == 0
    assert O.sense_radius(0.375) == 2 and O.sense_radius(O.below32(0.375)) == 1
    assert O.sense_radius(O.below32(4.125)) == 16 and O.sense_radius(4.125) == 17
    small = [c for c in cases if c['shape'] != O.BIG_SHAPE]
    for shape in O.SM_SHAPES:
        mine = [c for c in small if c['shape'] == shape]
        assert {(c['sigma'], c['decimals']) for c in mine} == {(s, d) for s in O.SM_SIGMAS for d in O.SM_DECIMALS}
        assert {(c['decimals'], c['density'], c['epoch']) for c in mine} == \
            {(d, r, e) for d in O.SM_DECIMALS for r in O.SM_DENSITIES for e in (1, O.OWNER_EPOCH_MAX)}
    # narrow fields: the taps clamp on BOTH sides at once at the large radii
    assert all(min(W, H) < 2 * 16 for W, H in O.SM_SHAPES[:5])
    big = [c for c in cases if c['shape'] == O.BIG_SHAPE]
    W, H = O.BIG_SHAPE
    assert len(big) == 1 and O.sense_radius(big[0]['sigma']) == 1
    assert W * H > O.GRID_BLOCKS * O.BLOCK and (W - 1) * H <= O.GRID_BLOCKS * O.BLOCK and W * (H - 1) <= O.GRID_BLOCKS * O.BLOCK


def test_the_claim_planes_carry_stale_words():
    for c in O.sense_cases():
        words = O.sense_inputs(c).view(np.uint64)
        occ = O.occupied(words, c['epoch'])
        assert occ.any()
        stale = words[~occ]
        if stale.size == 0:
            assert c['shape'] in ((1, 1), (2, 2), (5, 3), (1, 40), (40, 1))
            continue
        assert (stale != 0).all()
        tags = set((stale >> np.uint64(59)).tolist())
        assert tags <= {c['epoch'] - 1, c['epoch'] % O.OWNER_EPOCH_MAX + 1, 0} and c['epoch'] not in tags
        assert ((stale >> np.uint64(32)) & np.uint64(O.OWNER_SLOT_MASK) != 0).all() and (stale & np.uint64(0xFFFFFFFF) != 0).all()
    c = next(c for c in O.sense_cases() if c['shape'] == (96, 80))
    tags = set((O.sense_inputs(c).view(np.uint64) >> np.uint64(59)).reshape(-1).tolist())
    assert tags == {c['epoch'] - 1, c['epoch'], c['epoch'] % O.OWNER_EPOCH_MAX + 1, 0}


def test_sense_model_is_the_reference_with_a_margin():
    """The model gives scipy's mask on every case, and no reference value lies within 2^-40 of its threshold: the device mask is
    compared bit for bit.  Prints the worst margin."""
    worst = (np.inf, None)
    for c in O.sense_cases():
        words = O.sense_inputs(c)
        want, g = O.sense_reference(words, c['epoch'], c['sigma'], c['decimals'])
        got, tmp = O.sense_model(words, c['epoch'], c['sigma'], c['decimals'])
        assert np.array_equal(got, want), O.sense_id(c)
        m = O.sense_margin(g, c['decimals'])
        worst = min(worst, (m, O.sense_id(c)))
        assert m >= O.SM_MARGIN, (O.sense_id(c), m)
        assert tmp.shape == words.shape and 0 <= tmp.min() and tmp.max() <= 1 + 1e-15
    print(f'sense mask cases: worst threshold margin {worst[0]:.3e} ({worst[1]}), {worst[0] / O.SM_MARGIN:.0f} x the bound')


def test_sense_weights_are_scipys():
    for s, r in zip(O.SM_SIGMAS, O.SM_RADII):
        w = O.sense_weights(s, r)
        assert np.allclose(w, R.gaussian_weights(float(np.float32(s))), rtol=1e-14, atol=0) and abs(w.sum() - 1) < 1e-15


def test_an_occupied_cell_is_always_visible():
    """What lets NeuralAutomataAgent leave the agents channel unmasked: at the Env's sigma 2.0 / 3 decimals an agent's own weight
    w0^2 is far above the 0.0005 the rounding keeps, whatever the edges do."""
    w0 = O.sense_weights(O.ENV_SENSE_SIGMA, 8)[8]
    assert w0 * w0 > 0.039 and w0 * w0 > 70 * 0.0005
    rs = np.random.RandomState(2)
    for W, H in ((48, 40), (37, 23), (1, 1), (5, 3), (96, 80)):
        for density in O.SM_DENSITIES:
            occ = O.occupancy(W, H, density, rs)
            assert O.env_mask(occ)[occ].all()
    # env_mask is RefEnv.sense_mask
    medium = np.stack([O.occupancy(48, 40, 0.05, rs).astype(np.float64)] * 3)
    ref = R.RefEnv(medium, np.zeros((4, 3)), R.RefDynamics(apply_sense_mask=True))
    assert np.array_equal(ref.sense_mask().astype(bool), O.env_mask(medium[0]))


# ---------------------------------------------------------------------------------------------------------------- colormap
def _listed(N):
    from matplotlib.colors import ListedColormap
    lut = O.make_lut(N).astype(np.float64)
    cm = ListedColormap(lut[:N])
    cm.set_extremes(under=lut[N], over=lut[N + 1], bad=lut[N + 2])
    cm._init()
    return cm, lut


@pytest.mark.parametrize('N', O.LUT_SIZES)
def test_the_lookup_table_is_a_listed_colormap(N):
    pytest.importorskip('matplotlib')
    cm, lut = _listed(N)
    assert cm.N == N and np.array_equal(np.asarray(cm._lut), lut)
    assert (cm._i_under, cm._i_over, cm._i_bad) == (N, N + 1, N + 2)


@pytest.mark.parametrize('N', O.LUT_SIZES)
def test_index_model_is_matplotlibs(N):
    """Colormap.__call__ on the float64 values of every probe picks the row the model names (the rows are distinct)."""
    pytest.importorskip('matplotlib')
    cm, lut = _listed(N)
    t = O.trace_probes(N)
    assert t.dtype == np.float32 and t.shape == O.RENDER_SHAPE
    with np.errstate(invalid='ignore'):
        got = cm(t.astype(np.float64).reshape(-1))
    idx = O.cmap_index(t, N).reshape(-1)
    assert np.array_equal(got, lut[idx])
    assert set(range(N + 3)) <= set(idx.tolist())                              # every row of the table is asked for
    k = (np.arange(N + 1) / N).astype(np.float32)
    if N in (7, 10, 255):                                                      # k / N rounded to fp32 does not give k back
        x = k.astype(np.float64) * N
        assert (x != np.arange(N + 1)).any()                                   # (the fp32 neighbours put probes on either side)


def test_trace_step_has_two_answers_only_where_the_product_rounds():
    t = O.trace_probes(256)
    occ = np.random.RandomState(3).rand(*t.shape) < 0.3
    two, one = O.trace_step(t, O.TRACE_DECAY, occ)
    assert two.dtype == one.dtype == np.float32
    differ = (two.view(np.uint32) != one.view(np.uint32)) & ~np.isnan(two)
    assert 0 < differ.mean() < 0.5 and not differ[~occ].any()
    same, _ = O.trace_step(t, 1.0, np.zeros_like(occ))
    keep = ~np.isnan(t) & ~((t == 0) & np.signbit(t))
    assert np.array_equal(same.view(np.uint32)[keep], t.view(np.uint32)[keep])           # decay 1, nobody there: the same bits …
    assert (same[(t == 0) & np.signbit(t)].view(np.uint32) == 0).all()                   # … but -0.0 + 0.0 is +0.0


# ---------------------------------------------------------------------------------------------------------------- uint8
def test_u8_inputs():
    finite, rest = O.all_f16()
    assert finite.dtype == np.float16 and len(set(finite.view(np.uint16).reshape(-1).tolist())) == 248 * 256
    assert np.isfinite(finite).all() and np.isinf(rest).sum() == 2 and not np.isnan(rest).any()
    x = O.u8_exact(finite)
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)          # 11-bit x 8-bit + .5 fits fp32: exact on any path
    plane, either = O.u8_f32_inputs()                                          # (asserts that `either` is exactly the planted cells)
    assert plane.dtype == np.float32 and either.sum() == 254 and not np.isnan(plane).any()
    want = O.to_u8_model(plane)
    assert want[plane.reshape(-1).tolist().index(0.5) // plane.shape[1], plane.reshape(-1).tolist().index(0.5) % plane.shape[1]] == 128
    # numpy's own fp32 evaluation is inside what the test accepts
    got = (np.clip(plane, 0, 1) * np.float32(255) + np.float32(0.5)).astype(np.uint8)
    ok = (got == want) | (either & (np.abs(got.astype(int) - want.astype(int)) <= 1))
    assert ok.all() and (got == want)[~either].all()


# ---------------------------------------------------------------------------------------------------------------- gradient image
@pytest.mark.parametrize('W,H', O.GR_SHAPES)
def test_gradient_model_is_np_gradient(W, H):
    chem, planted = O.gradient_chem(W, H)
    assert np.array_equal(chem * 1024, np.rint(chem * 1024)) and chem.min() >= 0 and chem.max() <= 1
    assert np.array_equal(chem.astype(np.float16).astype(np.float64), chem)    # representable in fp16, hence in fp32
    gx, gy, norm = O.gradient_parts(chem)
    g = np.gradient(chem)
    assert np.array_equal(gx, g[0]) and np.array_equal(gy, g[1])
    s = gx * gx + gy * gy
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)          # differences, halving, squares and their sum: exact in fp32
    for normalized in (True, False):
        for clip in O.GR_CLIPS:
            want = R.gradient_field(chem, normalized, None if clip is None else float(np.float32(clip)))
            img = O.gradient_image(chem, normalized, clip)
            assert np.array_equal(img, 0.5 * (np.stack([want[0], want[1], np.zeros_like(gx)], axis=-1) + 1.0))
            # the condition: the planted exact ties apart, no cell sits on the clip
            ties = O.gradient_ties(chem, clip)
            if clip == 2.0 ** -11:
                assert np.array_equal(ties, planted) and (norm[planted] == clip).all()
            else:
                assert not ties.any()
    if planted.any():
        assert planted.sum() == 4 and ((np.abs(gx[planted]) == 2.0 ** -11) ^ (np.abs(gy[planted]) == 2.0 ** -11)).all()
        assert (norm[5:12, 5:12] == 0).sum() > 20                              # the flat patch: 0 / 0 -> 0
        assert ((gx == 2.0 ** -11) & (gy == 0)).any()


# ---------------------------------------------------------------------------------------------------------------- 6. sharpness
@pytest.mark.parametrize('bug', O.SENSE_BUGS)
def test_sense_cases_see_a_planted_error(bug):
    seen = []
    for c in O.sense_cases():
        if c['shape'] == O.BIG_SHAPE:
            continue
        words = O.sense_inputs(c)
        d = c['decimals']
        if (bug == 'decimals_minus' and d == 0) or (bug == 'decimals_plus' and d == 9):
            continue
        true, _ = O.sense_model(words, c['epoch'], c['sigma'], d)
        wrong, _ = O.sense_model(words, c['epoch'], c['sigma'], d, bug=bug)
        if not np.array_equal(true, wrong):
            seen.append(O.sense_id(c))
    print(f'sense mask, planted {bug}: told apart by {len(seen)} cases')
    assert seen
    if bug == 'radius_truncated':                                              # only 0.375 has 4 sigma + .5 rounding up
        assert all('-s0.375-' in s for s in seen)


@pytest.mark.parametrize('bug', O.CMAP_BUGS)
def test_colormap_probes_see_a_planted_error(bug):
    for N in O.LUT_SIZES:
        t = O.trace_probes(N)
        differ = O.cmap_index(t, N) != O.cmap_index(t, N, bug=bug)
        if bug == 'round' and N == 1:
            continue                                                           # one colour: floor and round both give 0 inside
        assert differ.any(), (bug, N)


@pytest.mark.parametrize('bug', O.U8_BUGS)
def test_u8_inputs_see_a_planted_error(bug):
    finite, rest = O.all_f16()
    plane, either = O.u8_f32_inputs()
    for v, skip in ((finite, None), (rest, None), (plane, either)):
        a, b = O.to_u8_model(v), O.to_u8_model(v, bug=bug)
        far = np.abs(a.astype(int) - b.astype(int)) >= 1
        if skip is not None:
            far &= ~skip
        assert far.any(), bug


@pytest.mark.parametrize('bug', O.GRADIENT_BUGS)
def test_gradient_cases_see_a_planted_error(bug):
    seen = 0
    for W, H in O.GR_SHAPES:
        chem, _ = O.gradient_chem(W, H)
        for normalized in (True, False):
            for clip in O.GR_CLIPS:
                d = np.abs(O.gradient_image(chem, normalized, clip) - O.gradient_image(chem, normalized, clip, bug=bug)).max()
                assert d == 0 or d > 100 * O.GR_TOL                            # nothing in between: the tolerance cannot hide it
                seen += d > 0
                if bug == 'one_sided_halved' and not normalized:
                    assert d > 0, (W, H, clip)                                 # every shape has edges
    assert seen
    if bug == 'clip_strict':                                                   # exactly the planted ties, at clip 2^-11
        assert seen == 2
