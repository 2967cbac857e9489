"""The numpy model of the conv layer and its adjoint (tests/conv_adjoint_model.py), on its own: against torch's float64 autograd
wherever torch takes the shape, by the adjoint identities <conv(x), g> = <x, grad_in> = <w, grad_w> and a tap-by-tap restatement
of the header's formula on the fields torch refuses (a radius beyond the field: 'circular' wraps several times), and the fp32
yardstick of EVERY case tests/test_gpu_conv_abi.py runs: the same evaluation in float32 (torch's where it takes the shape, the
model's own taps in float32 everywhere) stays within 1e-5 of the model, relative to max|.| of each array — an order or more under
the ceilings the device is held to, which keeps those ceilings meaningful.  No kernel is launched here.

Bounds.  float64 against float64: a sum of n products evaluated in two orders differs by at most about n * 2^-53 times the sum of
the terms' magnitudes; the longest sums here are the weight gradient's W * H = 4 290 terms and the layer's 4 * 49 = 196, so 1e-12
of max|.| (terms of order 1, results of order 1 to 60) leaves a factor of a few.  Identities: 1e-13 of the sum of |terms|."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import conv_adjoint_model as A

YARDSTICK = 1e-5
F64_TOL = 1e-12
TORCH_PAIRS = ((1, 4), (4, 1), (4, 4), (2, 3))
TORCH_FIELDS = ((17, 66), (24, 40), (7, 9), (33, 130))
WRAP_FIELDS = ((1, 1), (2, 3), (3, 2), (2, 2))


def _torch_accepts(W, H, k, mode):
    r = k // 2
    if mode == 'circular':
        return r <= W and r <= H
    if mode == 'reflect':
        return r < W and r < H
    return True


def _torch_eval(x, w, g, mode, dtype):
    """(out, grad_w, grad_in) of nn.Conv2d(padding='same', padding_mode=mode) in `dtype`, as float64 arrays."""
    cout, cin, k, _ = w.shape
    layer = nn.Conv2d(cin, cout, k, padding='same', padding_mode=mode, bias=False, dtype=dtype)
    with torch.no_grad():
        layer.weight.copy_(torch.as_tensor(w, dtype=dtype))
    xt = torch.as_tensor(x, dtype=dtype).clone().requires_grad_(True)
    out = layer(xt[None])[0]
    (out * torch.as_tensor(g, dtype=dtype)).sum().backward()
    return tuple(t.detach().to(torch.float64).numpy() for t in (out, layer.weight.grad, xt.grad))


def _rel(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


# ------------------------------------------------------------------------------------------------ 1. against torch float64
@pytest.mark.parametrize('mode', A.BWD_MODES)
@pytest.mark.parametrize('k', A.KS)
def test_model_matches_torch_float64_autograd(k, mode):
    worst = 0.0
    for W, H in TORCH_FIELDS:
        for cin, cout in TORCH_PAIRS:
            c = A.case_inputs(k, mode, cin, cout, W, H)
            out, gw, gi = _torch_eval(c['x'], c['w'], c['g'], mode, torch.float64)
            mw, mi = A.conv_backward(c['x'], c['w'], c['g'], mode)
            errs = (_rel(A.conv(c['x'], c['w'], mode), out), _rel(A.conv_taps(c['x'], c['w'], mode), out), _rel(mw, gw), _rel(mi, gi))
            worst = max(worst, *errs)
            assert max(errs) <= F64_TOL, (W, H, cin, cout, errs)
    print(f'conv model vs torch float64, k = {k} {mode}: worst {worst:.2e} of max|.| (ceiling {F64_TOL:.0e})')


@pytest.mark.parametrize('mode', ('reflect', 'replicate'))
def test_forward_model_matches_torch_float64_in_the_forward_only_modes(mode):
    for k in A.KS:
        for W, H in ((17, 66), (7, 9), (5, 4)):
            c = A.case_inputs(k, mode, 3, 2, W, H)
            with torch.no_grad():
                want = torch.nn.functional.conv2d(
                    torch.nn.functional.pad(torch.as_tensor(c['x'], dtype=torch.float64)[None], (k // 2,) * 4, mode=mode if k > 1 else 'replicate'),
                    torch.as_tensor(c['w'], dtype=torch.float64))[0].numpy()
            assert _rel(A.conv(c['x'], c['w'], mode), want) <= F64_TOL
            assert _rel(A.conv_taps(c['x'], c['w'], mode), want) <= F64_TOL


def test_tanh_mask_adjoint_and_gather_backward_match_torch_autograd():
    rs = np.random.RandomState(5)
    W, H, N = 6, 7, 40
    z, g = rs.standard_normal((3, W, H)), rs.standard_normal((3, W, H))
    mask = (rs.rand(W, H) > 0.25) * (4.0 / 3.0)
    zt = torch.as_tensor(z).requires_grad_(True)
    (torch.tanh(zt) * torch.as_tensor(mask) * torch.as_tensor(g)).sum().backward()
    assert _rel(A.tanh_mask_adjoint(g, np.tanh(z), mask), zt.grad.numpy()) <= F64_TOL
    assert _rel(A.tanh_mask_adjoint(g, np.tanh(z)), (g * (1 - np.tanh(z) ** 2))) <= F64_TOL
    cx, cy = rs.randint(0, W, N), rs.randint(0, H, N)
    cx[:5], cy[:5] = cx[0], cy[0]                                 # five slots on one cell
    coefs, ga = (0.1, 0.1, 2.0), rs.standard_normal((3, N))
    pt = torch.as_tensor(z).requires_grad_(True)
    act = pt[:, torch.as_tensor(cx), torch.as_tensor(cy)] * torch.as_tensor(coefs, dtype=torch.float64)[:, None]
    assert np.array_equal(act.detach().numpy(), A.gather(z, cx, cy, coefs))
    (act * torch.as_tensor(ga)).sum().backward()
    got = A.gather_backward(cx, cy, ga, coefs, W, H)
    assert _rel(got, pt.grad.numpy()) <= F64_TOL
    untouched = np.ones((W, H), dtype=bool)
    untouched[cx, cy] = False
    assert untouched.any() and np.all(got[:, untouched] == 0)


# ------------------------------------------------------------------------------------------------ 2. where torch refuses
def _by_the_formula(x, w, mode):
    """die_hip.h's formula with Python loops: 'circular' reads (x + a - r) mod W, 'zeros' drops what falls outside."""
    cout, cin, k, _ = w.shape
    r, (W, H) = k // 2, x.shape[1:]
    out = np.zeros((cout, W, H))
    for px in range(W):
        for py in range(H):
            for a in range(k):
                for b in range(k):
                    qx, qy = px + a - r, py + b - r
                    if mode == 'zeros' and not (0 <= qx < W and 0 <= qy < H):
                        continue
                    out[:, px, py] += w[:, :, a, b] @ x[:, qx % W, qy % H]
    return out


@pytest.mark.parametrize('mode', A.BWD_MODES)
@pytest.mark.parametrize('W,H', WRAP_FIELDS)
def test_adjoint_identities_where_the_radius_exceeds_the_field(W, H, mode):
    worst = 0.0
    for k in A.KS:
        for cin, cout in TORCH_PAIRS:
            c = A.case_inputs(k, mode, cin, cout, W, H)
            x, w, g = (c[n].astype(np.float64) for n in 'xwg')
            out = A.conv(x, w, mode)
            assert np.abs(out - _by_the_formula(x, w, mode)).max() <= F64_TOL * max(np.abs(out).max(), 1.0)
            assert np.abs(A.conv_taps(x, w, mode) - out).max() <= F64_TOL * max(np.abs(out).max(), 1.0)
            gw, gi = A.conv_backward(x, w, g, mode)
            lhs, scale = float((out * g).sum()), float(np.abs(out * g).sum()) + float(np.abs(w * gw).sum()) + float(np.abs(x * gi).sum())
            for rhs in (float((x * gi).sum()), float((w * gw).sum())):
                worst = max(worst, abs(lhs - rhs) / scale)
                assert abs(lhs - rhs) <= 1e-13 * scale, (k, cin, cout, lhs, rhs)
    print(f'adjoint identities on {W} x {H} {mode}: worst {worst:.2e} of the sum of |terms| (ceiling 1e-13)')


# ------------------------------------------------------------------------------------------------ 3. the fp32 yardstick
def _mixed(x):
    """What the mixed-kinds forward case reads: plane 0 from a claim plane (0 / 1), plane 1 rounded to fp16."""
    v = x.astype(np.float64)
    v[0] = A.occupancy(*x.shape[1:])
    v[1] = x[1].astype(np.float16)
    return v


@pytest.mark.parametrize('mode', A.FWD_MODES)
@pytest.mark.parametrize('k', A.KS)
def test_fp32_evaluation_of_every_gpu_case_stays_within_the_yardstick(k, mode):
    worst = dict(fwd_torch=0.0, fwd_numpy=0.0, grad_w_torch=0.0, grad_w_numpy=0.0, grad_in_torch=0.0, grad_in_numpy=0.0)

    def note(key, err, where):
        worst[key] = max(worst[key], err)
        assert err <= YARDSTICK, (key, where, err)

    for W, H in A.shapes_for(mode, k):
        for cin, cout in A.PAIRS:
            c = A.case_inputs(k, mode, cin, cout, W, H)
            variants = [c['x'].astype(np.float64)] + ([_mixed(c['x'])] if cin == 4 else [])
            for x in variants:
                out = A.conv(x, c['w'], mode)
                note('fwd_numpy', _rel(A.conv_taps(x, c['w'], mode, np.float32), out), (W, H, cin, cout))
                if mode not in A.BWD_MODES:
                    if _torch_accepts(W, H, k, mode):
                        with torch.no_grad():
                            xt = torch.nn.functional.pad(torch.as_tensor(x, dtype=torch.float32)[None], (k // 2,) * 4, mode=mode if k > 1 else 'replicate')
                            t32 = torch.nn.functional.conv2d(xt, torch.as_tensor(c['w']))[0].to(torch.float64).numpy()
                        note('fwd_torch', _rel(t32, out), (W, H, cin, cout))
                    continue
                gw, gi = A.conv_backward(x, c['w'], c['g'], mode)
                nw, ni = A.conv_backward(x, c['w'], c['g'], mode, np.float32)
                note('grad_w_numpy', _rel(nw, gw), (W, H, cin, cout))
                note('grad_in_numpy', _rel(ni, gi), (W, H, cin, cout))
                if _torch_accepts(W, H, k, mode):
                    t32, tw, ti = _torch_eval(x, c['w'], c['g'], mode, torch.float32)
                    note('fwd_torch', _rel(t32, out), (W, H, cin, cout))
                    note('grad_w_torch', _rel(tw, gw), (W, H, cin, cout))
                    note('grad_in_torch', _rel(ti, gi), (W, H, cin, cout))
    print(f'fp32 yardstick k = {k} {mode}: ' + '  '.join(f'{n} {v:.2e}' for n, v in worst.items() if v > 0) + f'  (of max|.|; ceiling {YARDSTICK:.0e})')


def test_case_list_is_pinned():
    assert A.SHAPES == ((16, 64), (17, 66), (20, 68), (33, 130), (1, 1), (2, 3), (3, 2), (5, 4))
    assert len(A.PAIRS) == 16 and set(A.PAIRS) == {(i, o) for i in range(1, 5) for o in range(1, 5)}
    assert A.shapes_for('reflect', 7) == ((16, 64), (17, 66), (20, 68), (33, 130), (5, 4))
    assert A.shapes_for('reflect', 3) == ((16, 64), (17, 66), (20, 68), (33, 130), (2, 3), (3, 2), (5, 4))
    assert A.shapes_for('circular', 7) == A.SHAPES and A.shapes_for('reflect', 1) == A.SHAPES
    a, b = A.case_inputs(3, 'zeros', 2, 3, 5, 4), A.case_inputs(3, 'zeros', 2, 3, 5, 4)
    assert all(np.array_equal(a[n], b[n]) and a[n].dtype == np.float32 for n in 'xwg')
    assert set(np.unique(A.occupancy(5, 4))) <= {0.0, 1.0} and 0.2 < A.WORLD_OCC.mean() < 0.4
    assert 0 <= a['x'].min() and a['x'].max() < 1 and np.abs(a['w']).max() <= 0.5


def test_fp32_read_out_keeps_the_adjoint_identity_of_the_gpu_case_within_1e_6():
    """<gather(planes), g> against <planes, scatter(g)> with every product and every cell's sum rounded to fp32, as the device
    rounds them, and the two inner products in float64: what the device test asks of the kernels, asked of plain fp32 first."""
    from oracle import cpu_ref as R
    W, H, x, y, planes, g, coefs = A.gather_case()
    cx, cy = R.cell(x, W), R.cell(y, H)
    assert np.array_equal(cx[:W * H] * H + cy[:W * H], np.arange(W * H))
    assert list(zip(cx[-4:], cy[-4:])) == [(0, 0), (0, H - 1), (W - 1, 0), (W - 1, H - 1)]
    cf = np.asarray(coefs, dtype=np.float32)
    act = A.gather(planes, cx, cy, cf)
    assert act.dtype == np.float32
    scat = np.zeros((3, W, H), dtype=np.float32)
    for c in range(3):
        np.add.at(scat[c], (cx, cy), g[c] * cf[c])
    lhs, rhs = float((act.astype(np.float64) * g).sum()), float((planes.astype(np.float64) * scat).sum())
    print(f'fp32 read-out adjoint identity: {lhs:.9e} against {rhs:.9e}, apart by {abs(lhs - rhs) / abs(rhs):.2e} (ceiling 1e-6)')
    assert abs(lhs - rhs) <= 1e-6 * abs(rhs)
    assert np.abs(scat - A.gather_backward(cx, cy, g, cf.astype(np.float64), W, H)).max() <= 1e-6 * np.abs(scat).max()
