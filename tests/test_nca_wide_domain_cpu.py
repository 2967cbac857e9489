"""The wide layer's domain sweep without a GPU: that the lattice of tests/nca_wide_domain_cases.py does what
tests/test_gpu_nca_wide_domain.py relies on.

1. Exactness: an fp32 accumulation in k_conv_wide's order and in the reverse order equals the float64 model bit for bit.
2. The model: tests/nca_wide_model.conv equals torch's float64 conv2d after F.pad wherever torch takes the shape, and the header's
   formula written as loops (cases.conv_loops) everywhere — fields below the radius included.
3. The precondition (asserted inside the generator) holds for every case of both tables, the plane-kind cases and the stacks."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dropout_model as D
from tests import nca_wide_grad_model as G
from tests import nca_wide_domain_cases as K
from tests import nca_wide_model as M
from tests import stock_plane_model as S

GROUPS = [name for name, _ in K.FIELD_GROUPS]
# the sample of the pair cross: the five pairs of the field table and the ends of both channel lists
CROSS_SAMPLE = K.PAIRS + ((1, 32), (32, 1), (2, 15), (13, 31), (31, 17), (17, 16), (4, 3), (8, 32))
TORCH_PAD = {'circular': 'circular', 'zeros': 'constant', 'reflect': 'reflect', 'replicate': 'replicate'}


def test_the_case_tables():
    assert K.CIN == (1, 2, 3, 4, 5, 8, 13, 16, 17, 31, 32) and K.COUT == (1, 3, 15, 16, 17, 31, 32)
    assert K.PAIRS == ((1, 1), (3, 16), (16, 3), (5, 17), (32, 32)) and K.CROSS_FIELD == (17, 66) and K.KS == (1, 3, 5)
    assert set(K.FIELDS) == {(1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (5, 4), (16, 64), (15, 63), (17, 65), (20, 68), (33, 130)}
    assert {H % 4 for _, H in K.FIELDS} == {0, 1, 2, 3}
    for k in K.KS:
        for mode in K.MODES:
            assert len(K.cross_cases(k, mode)) == 77
    assert set(CROSS_SAMPLE) <= {(a, b) for a in K.CIN for b in K.COUT}
    # 'reflect' only where the header allows it: k / 2 below W and H
    assert [c[2:] for c in K.field_cases('below_radius', 'reflect')[::5]] == [(1, 1, 1), (1, 1, 7), (1, 7, 1), (1, 2, 3), (3, 2, 3), (1, 3, 2), (3, 3, 2)]
    assert len(K.field_cases('below_radius', 'circular')) == 5 * 3 * 5 and len(K.field_cases('three_tiles', 'reflect')) == 15


def test_the_largest_layer_of_the_cross():
    """32 -> 32, k = 5, 17 x 66: 800 terms an output, weights over 256 or 512, max |z| between 2 and 4."""
    c = K.case(32, 32, 5, 17, 66)
    assert c['s'] in (8, 9) and all(2.0 <= np.abs(z).max() < 4.0 for z in c['z'].values())
    assert np.abs(c['x']).max() == 3 and np.abs(c['w']).max() * 2 ** c['s'] == 7 and (c['w'] != 0).all()
    assert np.array_equal(c['x'], np.round(c['x'])) and np.array_equal(c['g'], np.round(c['g'])) and np.abs(c['g']).max() == 3


def test_pad_index_is_the_four_rules():
    v = np.arange(-7, 12)
    assert K.pad_index(v, 5, 'circular').tolist() == [3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1]
    assert K.pad_index(v, 5, 'zeros').tolist() == [-1] * 7 + [0, 1, 2, 3, 4] + [-1] * 7
    assert K.pad_index(v, 5, 'replicate').tolist() == [0] * 7 + [0, 1, 2, 3, 4] + [4] * 7
    assert K.pad_index(np.arange(-4, 9), 5, 'reflect').tolist() == [4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0]
    assert K.pad_index(np.arange(-2, 3), 1, 'circular').tolist() == [0] * 5


# ------------------------------------------------------------------------------------------------ 1. exactness
def _exact(cases, mode):
    for cin, cout, k, W, H in cases:
        c = K.case(cin, cout, k, W, H)
        want = c['z'][mode]
        for reverse in (False, True):
            got = K.conv_fp32(c['x'], c['w'], mode, reverse)
            assert got.dtype == np.float32 and np.array_equal(got, want), (cin, cout, k, W, H, mode, reverse)


@pytest.mark.parametrize('mode', K.MODES)
@pytest.mark.parametrize('group', GROUPS)
def test_fp32_in_the_kernels_order_and_in_reverse_is_the_float64_model_on_every_field(group, mode):
    _exact(K.field_cases(group, mode), mode)


@pytest.mark.parametrize('mode', K.MODES)
@pytest.mark.parametrize('k', K.KS)
def test_fp32_in_the_kernels_order_and_in_reverse_is_the_float64_model_on_a_sample_of_the_cross(k, mode):
    _exact([c for c in K.cross_cases(k, mode) if c[:2] in CROSS_SAMPLE], mode)


def test_an_off_lattice_weight_does_round():
    """What the lattice buys: the same 32 -> 32 layer with weights over 10 (no power of two) is NOT order-independent in fp32."""
    c = K.case(32, 32, 5, 17, 66)
    w = (c['w'] * 2.0 ** c['s'] / 10).astype(np.float32)
    assert not np.array_equal(K.conv_fp32(c['x'], w, 'circular'), K.conv_fp32(c['x'], w, 'circular', reverse=True))


def test_the_epilogues_and_the_adjoint_are_exact_in_fp32_too():
    """relu and the p = 0.5 mask in fp32 equal their float64 values; both adjoint sums in fp32 equal tests/nca_wide_grad_model."""
    cin, cout, k, W, H = 5, 17, 3, 17, 66
    c = K.case(cin, cout, k, W, H)
    mask = D.mask(c['seed'], K.DROP_STEP, W, H, K.DROP_P)
    assert set(np.unique(mask)) == {0.0, 2.0}
    for mode in G.MODES:
        z = c['z'][mode]
        t = np.maximum(z, np.float32(0))
        assert np.array_equal((t * mask[None]).astype(np.float64), np.maximum(z.astype(np.float64), 0) * mask)
        want_w, want_in = G.layer_backward(c['x'], c['w'], c['g'], t, 'relu', mask, mode)
        gz = (c['g'] * mask[None] * (t > 0)).astype(np.float32)
        got_w, got_in = G.conv_backward(c['x'], c['w'], gz, mode, dtype=np.float32)
        assert got_w.dtype == np.float32 and np.array_equal(got_w, want_w) and np.array_equal(got_in, want_in), mode
        assert np.array_equal(want_w.astype(np.float32), want_w) and np.array_equal(want_in.astype(np.float32), want_in)


# ------------------------------------------------------------------------------------------------ 2. the model
def _torch_conv(x, w, mode):
    """torch float64 conv2d after F.pad, or None where torch refuses the shape."""
    r = w.shape[-1] // 2
    xt, wt = torch.from_numpy(np.asarray(x, dtype=np.float64))[None], torch.from_numpy(np.asarray(w, dtype=np.float64))
    try:
        xp = F.pad(xt, (r, r, r, r), mode=TORCH_PAD[mode]) if r else xt
    except (RuntimeError, AssertionError, NotImplementedError):
        return None
    return F.conv2d(xp, wt)[0].numpy()


@pytest.mark.parametrize('mode', K.MODES)
@pytest.mark.parametrize('group', GROUPS)
def test_the_model_is_torch_float64_where_torch_takes_the_shape_and_the_headers_formula_everywhere(group, mode):
    by_torch = by_loops = 0
    for cin, cout, k, W, H in K.field_cases(group, mode):
        c = K.case(cin, cout, k, W, H)
        want = c['z'][mode].astype(np.float64)
        assert np.array_equal(M.conv(c['x'], c['w'], mode), want)
        ref = _torch_conv(c['x'], c['w'], mode)
        if ref is not None:
            assert np.array_equal(ref, want), (cin, cout, k, W, H, mode, 'torch')
            by_torch += 1
        if ref is None or W * H <= 64 * 16 or (cin, cout) == (5, 17):
            assert np.array_equal(K.conv_loops(c['x'], c['w'], mode), want), (cin, cout, k, W, H, mode, 'loops')
            by_loops += 1
    print(f'{group} {mode}: {by_torch} cases against torch, {by_loops} against the loops')
    assert by_loops > 0 and (by_torch > 0 or group == 'below_radius')
    if group == 'below_radius' and mode == 'circular':
        # torch refuses a circular pad wider than the field: those cases are held by the loops alone
        assert by_torch < len(K.field_cases(group, mode))


@pytest.mark.parametrize('k', K.KS)
def test_the_model_is_torch_float64_on_a_sample_of_the_cross(k):
    for mode in K.MODES:
        for cin, cout, k_, W, H in K.cross_cases(k, mode):
            if (cin, cout) in CROSS_SAMPLE:
                c = K.case(cin, cout, k, W, H)
                assert np.array_equal(_torch_conv(c['x'], c['w'], mode), c['z'][mode].astype(np.float64)), (cin, cout, k, mode)


# ------------------------------------------------------------------------------------------------ 3. the precondition
@pytest.mark.parametrize('k', K.KS)
def test_the_precondition_holds_on_the_whole_cross(k):
    """K.case asserts it while it draws; here every case of the cross is drawn, and the figures the method rests on are restated."""
    worst = 0.0
    for cin, cout, k_, W, H in K.cross_cases(k, 'circular'):
        c = K.case(cin, cout, k, W, H)
        assert c['modes'] == K.modes_for(W, H, k) and set(c['z']) == set(c['modes'])
        wi = np.abs(c['w'].astype(np.float64)) * 2.0 ** c['s']
        assert np.array_equal(wi, np.round(wi)) and wi.min() >= 1 and wi.max() <= 7
        mag = max(K.conv_model(np.abs(c['x']), wi, m).max() for m in c['modes'])
        worst = max(worst, mag)
        assert mag < K.EXACT and mag <= 21 * cin * k * k
        for m in c['modes']:                                      # what the device is held to IS tests/nca_wide_model.conv
            assert np.array_equal(M.conv(c['x'], c['w'], m), c['z'][m].astype(np.float64)), (cin, cout, k, m)
        top = max(np.abs(z).max() for z in c['z'].values())
        assert top < K.Z_LIMIT and (c['s'] == 0 or top >= K.Z_LIMIT / 2), (cin, cout, k, top)     # s is the smallest
    print(f'k = {k}: the largest sum of magnitudes is {worst:.0f} units, 2^24 = {K.EXACT:.0f}')


@pytest.mark.parametrize('group', GROUPS)
def test_the_precondition_holds_on_every_field(group):
    for mode in K.MODES:
        for cin, cout, k, W, H in K.field_cases(group, mode):
            c = K.case(cin, cout, k, W, H)
            assert mode in c['modes'] and np.abs(c['z'][mode]).max() < K.Z_LIMIT


def test_the_plane_kind_cases_read_as_their_values():
    for cin, kinds in K.KIND_CASES.items():
        assert len(kinds) == cin and kinds[-1] == K.STOCK and K.STOCK not in kinds[:-1]
        assert any(kind != K.F32 for kind in kinds[4:]), 'a plane that is not fp32 past the first chunk of 4'
        for W, H in K.KIND_FIELDS:
            for k in K.KIND_KS:
                c = K.kind_case(cin, k, W, H)
                for i, kind in enumerate(kinds):
                    if kind == K.F16:
                        assert np.array_equal(c['x'][i].astype(np.float16).astype(np.float32), c['x'][i])
                    if kind in (K.AGENTS, K.STOCK):
                        occ, _, bits, tag = S.decode(c['words'][i], K.EPOCH)
                        assert np.array_equal(occ, c['x'][i] != 0) and set(np.unique(tag)) <= {0, K.EPOCH - 1, K.EPOCH}
                        if W * H > 12:
                            assert (tag == K.EPOCH - 1).sum() > 0 and (tag == 0).sum() > 0
                for mode in c['modes']:
                    assert np.array_equal(K.conv_fp32(c['x'], c['w'], mode), c['z'][mode])
    assert K.KIND_CASES[9][7] == K.AGENTS


@pytest.mark.parametrize('W,H', K.STACK_FIELDS)
@pytest.mark.parametrize('agents', [True, False])
def test_the_stack_is_exact_up_to_the_last_tanh(W, H, agents):
    for mode in K.MODES:
        c = K.stack_case(W, H, agents, mode)
        assert c['planes'].shape == (K.STACK_R, 2 + agents, W, H) and len(c['pairs']) == 14
        assert np.array_equal(c['planes'].astype(np.float16).astype(np.float32), c['planes'])
        r, row = c['pairs'][-1]
        t = c['planes'][r]
        for (k, cout, act), w, want in zip(K.STACK_LAYERS, c['weights'], K.stack_model(c, r, row, mode)):
            z = K.conv_fp32(t, w[row], mode)
            assert np.array_equal(z, K.conv_fp32(t, w[row], mode, reverse=True))
            t = np.maximum(z, np.float32(0)) if act == 'relu' else z
            assert np.array_equal(t.astype(np.float64), want) and np.abs(want).max() < K.Z_LIMIT
