"""The NeuralAutomataAgent layer kernels through their C entry points (include/die_hip.h: die_conv2d, die_conv2d_dropout,
die_conv2d_backward, die_gather_scale, die_gather_scale_backward), called by ctypes as die_amd/agent/evo.py calls them, over the
argument domain the header documents and the Python class never reaches: every pair of 1..4 input and 1..4 output channels,
k = 1, 3, 5, 7, every padding mode, planes of mixed kinds, grad_in on a first layer, fields smaller than the tile and than the
radius, fwd_out / drop in every combination, p = 1 — against the float64 numpy model of tests/conv_adjoint_model.py.

Cases (shapes, channel pairs, inputs) are that module's: tests/test_conv_adjoint_model_cpu.py shows that a plain fp32 evaluation
of every one of them stays within 1e-5 of the model.  Ceilings: forward max|dev - f64| <= 1e-5 * max(1, max|f64|) (the project's
forward tolerance); backward 1e-4 * max|ref| per array (tests/test_gpu_nca_grad.py's).  Every test prints its worst device error
beside the fp32 numpy error of the same cases.

Every output is allocated with one plane more than the call is given and a tail behind it, the workspace with exactly the bytes
die_conv2d_backward_workspace_bytes names and a tail, all pre-filled with a sentinel that must come back untouched.  A test
enqueues all its launches on one stream and synchronises once before it reads anything back."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib as L
from die_amd.device_array import _ptr, from_q32, stream_ptr, to_q32
from oracle import cpu_ref as R
from tests import conv_adjoint_model as A
from tests import dropout_model as M
from tests import nca_grad_model as G

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FWD_TOL, BWD_TOL = 1e-5, 1e-4
SENT = np.float32(-7.25e7)                                        # no result comes near it
TAIL = 64                                                         # sentinel floats behind every buffer
F32, F16, AGENTS = L.DIE_PLANE_F32, L.DIE_PLANE_F16, L.DIE_PLANE_AGENTS
MIXED = (AGENTS, F16, F32, F32)
KINDS_A, KINDS_B = (AGENTS, F16, F32, F32), (F16, AGENTS, F16, AGENTS)
DROP_SHAPES = ((20, 68), (5, 4), (17, 66), (2, 3))                # H % 4 == 0 (one Philox block per thread) and not (cell by cell)
DROP_STEP = 3


@functools.lru_cache(maxsize=None)
def _world():
    """The one small world whose claim plane every 'agents' input reads (A.WORLD_OCC: a (W, H) case takes its first W * H words)."""
    occ = A.WORLD_OCC
    rs = np.random.RandomState(1)
    medium = np.stack([occ, rs.rand(*occ.shape), rs.rand(*occ.shape)])
    env = die.Env.from_numpy(medium, np.array([[0.5], [0.5], [1.0], [1.0]]), device=DEV)
    env.medium._ensure_owner()
    assert np.array_equal(env.medium.to_numpy()[0], occ)
    return env


def _sentinel(n):
    return torch.full((n,), float(SENT), dtype=torch.float32, device=DEV)


def _planes(x, kinds):
    """The device planes of a (cin, W, H) float32 array read as `kinds`: (tensors, die_conv_plane array, the float64 values the
    device reads: an fp16 plane's rounded values, a claim plane's 0 / 1)."""
    med = _world().medium
    cin, W, H = x.shape
    keep, seen = [], np.empty(x.shape)
    for c, kind in enumerate(kinds[:cin]):
        if kind == AGENTS:
            keep.append(med.owner.view(-1)[:W * H])
            seen[c] = A.occupancy(W, H)
        elif kind == F16:
            half = x[c].astype(np.float16)
            keep.append(torch.from_numpy(half).to(DEV))
            seen[c] = half
        else:
            keep.append(torch.from_numpy(x[c]).to(DEV))
            seen[c] = x[c]
    arr = (L.ConvPlane * cin)(*[L.ConvPlane(t.data_ptr(), kind, 0) for t, kind in zip(keep, kinds)])
    return keep, arr, seen


def _plane_ptrs(buf, n, cells):
    return (C.c_void_p * n)(*[buf.data_ptr() + 4 * o * cells for o in range(n)])


def _forward(W, H, arr, cin, cout, k, w_dev, tanh, pad, drop=None, through_dropout=False):
    """One forward launch into (cout + 1) sentinel planes and a tail; the buffer stays on the device."""
    buf = _sentinel((cout + 1) * W * H + TAIL)
    outs, epoch, sp = _plane_ptrs(buf, cout, W * H), _world().medium.epoch, stream_ptr(DEV)
    if drop is not None or through_dropout:
        L.check(L.lib.die_conv2d_dropout(W, H, cin, arr, epoch, cout, outs, k, _ptr(w_dev), tanh, pad,
                                         None if drop is None else C.byref(drop), sp), 'die_conv2d_dropout')
    else:
        L.check(L.lib.die_conv2d(W, H, cin, arr, epoch, cout, outs, k, _ptr(w_dev), tanh, pad, sp), 'die_conv2d')
    return buf


def _backward(W, H, arr, cin, cout, k, w_dev, g_dev, pad, want_gin, t_buf=None, drop=None):
    """One die_conv2d_backward: (grad_weights + tail, (cin + 1) grad_in planes + tail or None, workspace + tail)."""
    nw = cout * cin * k * k
    need = L.lib.die_conv2d_backward_workspace_bytes(W, H, cin, cout, k)
    assert need == -(-W // 16) * -(-H // 64) * nw * 4
    gw, ws = _sentinel(nw + TAIL), _sentinel(need // 4 + TAIL)
    gin = _sentinel((cin + 1) * W * H + TAIL) if want_gin else None
    L.check(L.lib.die_conv2d_backward(W, H, cin, arr, _world().medium.epoch, cout, _plane_ptrs(g_dev, cout, W * H), k, _ptr(w_dev), _ptr(gw),
                                      _plane_ptrs(gin, cin, W * H) if want_gin else None,
                                      None if t_buf is None else _plane_ptrs(t_buf, cout, W * H),
                                      None if drop is None else C.byref(drop), pad, _ptr(ws), need, stream_ptr(DEV)),
            'die_conv2d_backward')
    return gw, gin, ws


def _host(buf, n, shape, what):
    """The first n floats of a buffer as `shape`; everything behind them must still be the sentinel."""
    h = buf.cpu().numpy()
    assert np.all(h[n:] == SENT), f'{what}: written behind what the call was given ({int((h[n:] != SENT).sum())} floats)'
    return h[:n].reshape(shape)


class _Worst:
    """The largest error per label, for the one line a test prints."""

    def __init__(self):
        self.v = {}

    def note(self, label, err):
        self.v[label] = max(self.v.get(label, 0.0), float(err))

    def line(self):
        return '  '.join(f'{n} {v:.2e}' for n, v in self.v.items())


# ------------------------------------------------------------------------------------------------ 1. the forward
@pytest.mark.parametrize('mode', A.FWD_MODES)
@pytest.mark.parametrize('k', A.KS)
def test_forward_every_channel_pair_and_shape(k, mode):
    pad = L.PAD_MODES[mode]
    jobs, masked = [], []
    for W, H in A.shapes_for(mode, k):
        for cin, cout in A.PAIRS:
            c = A.case_inputs(k, mode, cin, cout, W, H)
            w_dev = torch.from_numpy(c['w']).to(DEV)
            for name, kinds in [('fp32 planes', (F32,) * 4)] + ([('mixed kinds', MIXED)] if cin == 4 else []):
                keep, arr, seen = _planes(c['x'], kinds)
                bufs = [_forward(W, H, arr, cin, cout, k, w_dev, tanh, pad) for tanh in (0, 1)]
                job = dict(where=f'{W}x{H} {cin}->{cout} {name}', W=W, H=H, cout=cout, w=c['w'], seen=seen, bufs=bufs, keep=(keep, w_dev))
                jobs.append(job)
                if name == 'fp32 planes' and (W, H) in DROP_SHAPES:
                    for tanh in (0, 1):
                        same = _forward(W, H, arr, cin, cout, k, w_dev, tanh, pad, through_dropout=True)      # drop NULL: die_conv2d itself
                        masked.append((job, tanh, None, None, same))
                        for p in (0.25, 1.0):
                            drop = L.nca_dropout(p, c['seed'], 0, DROP_STEP)
                            masked.append((job, tanh, p, c['seed'], _forward(W, H, arr, cin, cout, k, w_dev, tanh, pad, drop)))
    torch.cuda.synchronize()
    worst = _Worst()
    for j in jobs:
        W, H, cout = j['W'], j['H'], j['cout']
        ref, ref32 = A.conv(j['seen'], j['w'], mode), A.conv_taps(j['seen'], j['w'], mode, np.float32)
        j['got'] = []
        for tanh, buf in enumerate(j['bufs']):
            got = _host(buf, cout * W * H, (cout, W, H), f'{j["where"]} tanh={tanh}')
            j['got'].append(got)
            want, want32 = (np.tanh(ref), np.tanh(ref32)) if tanh else (ref, ref32)
            scale = max(1.0, np.abs(want).max())
            err = np.abs(got - want).max() / scale
            worst.note(f'die_conv2d tanh={tanh}: device', err)
            worst.note(f'tanh={tanh}: fp32 numpy', np.abs(want32 - want).max() / scale)
            assert err <= FWD_TOL, (j['where'], tanh, err)
    for j, tanh, p, seed, buf in masked:
        W, H, cout = j['W'], j['H'], j['cout']
        got = _host(buf, cout * W * H, (cout, W, H), f'{j["where"]} tanh={tanh} p={p}')
        plain = j['got'][tanh]
        if p is None:
            assert np.array_equal(got, plain), (j['where'], tanh, 'die_conv2d_dropout(drop = NULL) is not die_conv2d')
            continue
        mask = M.mask(seed, DROP_STEP, W, H, p)
        assert mask.dtype == np.float32 and (p < 1 or not mask.any())
        assert np.array_equal(got, plain * mask[None]), (j['where'], tanh, p)          # one fp32 multiply per cell, nothing else
    print(f'conv abi forward k = {k} {mode}: {worst.line()}  (of max(1, max|f64|); ceiling {FWD_TOL:.0e}; {len(jobs)} cases, '
          f'{len(masked)} masked launches)')


# ------------------------------------------------------------------------------------------------ 2. the backward
def _check_grads(where, W, H, cin, cout, k, run, want_w, want_in, worst, label, yard=None):
    gw_buf, gin_buf, ws_buf = run
    nw = cout * cin * k * k
    need = L.lib.die_conv2d_backward_workspace_bytes(W, H, cin, cout, k) // 4
    _host(ws_buf, need, (need,), f'{where}: workspace')
    gw = _host(gw_buf, nw, (cout, cin, k, k), f'{where}: grad_weights')
    out = [gw]
    pairs = [('grad_w', gw, want_w)]
    if gin_buf is not None:
        gin = _host(gin_buf, cin * W * H, (cin, W, H), f'{where}: grad_in')
        out.append(gin)
        pairs.append(('grad_in', gin, want_in))
    for n, (name, got, want) in enumerate(pairs):
        top = np.abs(want).max()
        err = np.abs(got - want).max()
        worst.note(f'{label} {name}: device', err / top if top > 0 else err)
        if yard is not None:
            worst.note(f'{name}: fp32 numpy', np.abs(yard[n] - want).max() / top if top > 0 else 0.0)
        assert err <= BWD_TOL * top, (where, label, name, err / top if top > 0 else err)
    return out


@pytest.mark.parametrize('mode', A.BWD_MODES)
@pytest.mark.parametrize('k', A.KS)
def test_backward_every_channel_pair_and_shape(k, mode):
    pad = L.PAD_MODES[mode]
    jobs = []
    for W, H in A.SHAPES:
        for cin, cout in A.PAIRS:
            c = A.case_inputs(k, mode, cin, cout, W, H)
            w_dev, g_dev = torch.from_numpy(c['w']).to(DEV), torch.from_numpy(c['g']).to(DEV)
            j = dict(where=f'{W}x{H} {cin}->{cout}', W=W, H=H, cin=cin, cout=cout, c=c, keep=[w_dev, g_dev])
            args = (W, H, cin, cout, k, w_dev, g_dev, pad)
            # plain: fp32 planes, no tanh; grad_in wanted, not wanted, and wanted again
            keep, arr, j['seen'] = _planes(c['x'], (F32,) * 4)
            j['plain'] = [_backward(W, H, arr, *args[2:], want) for want in (True, False, True)]
            j['keep'].append(keep)
            # a first layer of claim-plane / fp16 inputs that carried the tanh, its grad_in wanted: fwd_out without drop, and p = 1
            keep, arr, j['seen_a'] = _planes(c['x'], KINDS_A)
            j['t_a'] = _forward(W, H, arr, cin, cout, k, w_dev, 1, pad)
            j['tanh'] = _backward(W, H, arr, *args[2:], True, t_buf=j['t_a'])
            j['p1'] = _backward(W, H, arr, *args[2:], True, t_buf=j['t_a'], drop=L.nca_dropout(1.0, c['seed'], 0, DROP_STEP))
            j['keep'].append(keep)
            # the other kinds, fwd_out with the p = 0.25 mask
            keep, arr, j['seen_b'] = _planes(c['x'], KINDS_B)
            j['t_b'] = _forward(W, H, arr, cin, cout, k, w_dev, 1, pad)
            j['masked'] = _backward(W, H, arr, *args[2:], True, t_buf=j['t_b'], drop=L.nca_dropout(0.25, c['seed'], 0, DROP_STEP))
            j['keep'].append(keep)
            jobs.append(j)
    torch.cuda.synchronize()
    worst = _Worst()
    for j in jobs:
        W, H, cin, cout, c, where = j['W'], j['H'], j['cin'], j['cout'], j['c'], j['where']
        shape = (W, H, cin, cout, k)
        want = A.conv_backward(j['seen'], c['w'], c['g'], mode)
        yard = A.conv_backward(j['seen'], c['w'], c['g'], mode, np.float32)
        first = _check_grads(where, *shape, j['plain'][0], *want, worst, 'plain', yard)
        without = _check_grads(where, *shape, j['plain'][1], *want, worst, 'plain')
        again = _check_grads(where, *shape, j['plain'][2], *want, worst, 'plain')
        assert np.array_equal(first[0], without[0]), (where, 'grad_weights depend on whether grad_in was asked for')
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]), (where, 'two calls, two results')
        t = _host(j['t_a'], cout * W * H, (cout, W, H), f'{where}: forward, kinds A')
        ref = np.tanh(A.conv(j['seen_a'], c['w'], mode))
        assert np.abs(t - ref).max() <= FWD_TOL, (where, 'forward of kinds A')
        _check_grads(where, *shape, j['tanh'], *A.conv_backward(j['seen_a'], c['w'], A.tanh_mask_adjoint(c['g'], t), mode), worst,
                     'fwd_out, claim / fp16 inputs')
        for name, got in zip(('grad_weights', 'grad_in'), _check_grads(where, *shape, j['p1'], np.zeros_like(c['w']), np.zeros_like(c['x']),
                                                                        worst, 'p=1')):
            assert not got.any(), (where, f'p = 1: {name} is not zero')
        t = _host(j['t_b'], cout * W * H, (cout, W, H), f'{where}: forward, kinds B')
        ref = np.tanh(A.conv(j['seen_b'], c['w'], mode))
        assert np.abs(t - ref).max() <= FWD_TOL, (where, 'forward of kinds B')
        mask = M.mask(c['seed'], DROP_STEP, W, H, 0.25)
        _check_grads(where, *shape, j['masked'], *A.conv_backward(j['seen_b'], c['w'], A.tanh_mask_adjoint(c['g'], t, mask), mode), worst,
                     'fwd_out + drop p=0.25, fp16 / claim inputs')
    print(f'conv abi backward k = {k} {mode}: {worst.line()}  (of max|ref| per array; ceiling {BWD_TOL:.0e}; {len(jobs)} cases of 7 calls)')


# ------------------------------------------------------------------------------------------------ 3. two calls composed
@pytest.mark.parametrize('mode', A.BWD_MODES)
def test_two_layer_chain_matches_torch_float64_autograd(mode):
    """4 -> 2, k = 5, then 2 -> 3, k = 3 with the tanh, on 17 x 66: the second call's grad_in is the first call's grad_out."""
    W, H, pad = 17, 66, L.PAD_MODES[mode]
    c1, c2 = A.case_inputs(5, mode, 4, 2, W, H), A.case_inputs(3, mode, 2, 3, W, H)
    w1, w2, g = (torch.from_numpy(v).to(DEV) for v in (c1['w'], c2['w'], c2['g']))
    keep, arr1, seen = _planes(c1['x'], (F32,) * 4)
    hid = _forward(W, H, arr1, 4, 2, 5, w1, 0, pad)
    arr2 = (L.ConvPlane * 2)(*[L.ConvPlane(hid.data_ptr() + 4 * o * W * H, F32, 0) for o in range(2)])
    t = _forward(W, H, arr2, 2, 3, 3, w2, 1, pad)
    run2 = _backward(W, H, arr2, 2, 3, 3, w2, g, pad, True, t_buf=t)
    run1 = _backward(W, H, arr1, 4, 2, 5, w1, run2[1], pad, False)
    torch.cuda.synchronize()
    convs = G.layers([c1['w'].astype(np.float64), c2['w'].astype(np.float64)], mode)
    s = G.sense(convs, torch.as_tensor(seen))
    (s * torch.as_tensor(c2['g'].astype(np.float64))).sum().backward()
    assert np.abs(_host(t, 3 * W * H, (3, W, H), 'chain: forward') - s.detach().numpy()).max() <= FWD_TOL
    worst = _Worst()
    for li, (run, conv, shape) in enumerate(((run1, convs[0], (4, 2, 5)), (run2, convs[1], (2, 3, 3)))):
        cin, cout, kk = shape
        got = _host(run[0], cout * cin * kk * kk, (cout, cin, kk, kk), f'chain: layer {li} grad_weights')
        want = conv.weight.grad.numpy()
        err = np.abs(got - want).max() / np.abs(want).max()
        worst.note(f'layer {li} grad_w: device', err)
        assert err <= BWD_TOL, (li, err)
    print(f'conv abi chain {mode}: {worst.line()}  (of max|grad_f64|; ceiling {BWD_TOL:.0e})')


# ------------------------------------------------------------------------------------------------ 4. the read-out
def _medium(W, H):
    return L.Medium(W, H, L.DIE_F32, 1, None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, None)      # the read-out reads the geometry only


def _slots(x, y, W, H):
    """(device x, device y, cells) of slots at float coordinates: Q0.32 words and the cells the host twin of die_cell gives them."""
    qx, qy = to_q32(x), to_q32(y)
    dev = [torch.from_numpy(q.view(np.int32).copy()).to(DEV) for q in (qx, qy)]
    return dev[0], dev[1], R.cell(from_q32(qx), W), R.cell(from_q32(qy), H)


def _scatter(W, H, xd, yd, grads, coefs):
    N = grads.shape[1]
    g_dev = torch.from_numpy(np.ascontiguousarray(grads, dtype=np.float32)).to(DEV)
    planes = _sentinel(3 * W * H + TAIL)
    m, a = _medium(W, H), L.Agents(N, _ptr(xd), _ptr(yd), None, None, None)
    u = L.Action(N, g_dev[0].data_ptr(), g_dev[1].data_ptr(), g_dev[2].data_ptr())
    L.check(L.lib.die_gather_scale_backward(C.byref(m), C.byref(a), C.byref(u), (C.c_float * 3)(*coefs), _plane_ptrs(planes, 3, W * H),
                                            stream_ptr(DEV)), 'die_gather_scale_backward')
    return planes, g_dev


def test_scatter_of_4096_slots_on_four_cells_is_exact():
    W, H, N = 5, 4, 4096
    rs = np.random.RandomState(54)
    stands = np.array([(0, 0), (4, 3), (2, 1), (3, 2)])[rs.randint(0, 4, N)]
    xd, yd, cx, cy = _slots(stands[:, 0] / (W - 1), stands[:, 1] / (H - 1), W, H)
    assert np.array_equal(cx, stands[:, 0]) and np.array_equal(cy, stands[:, 1])
    grads, coefs = rs.randint(-8, 9, (3, N)).astype(np.float32), (0.5, 0.25, 2.0)
    planes, keep = _scatter(W, H, xd, yd, grads, coefs)
    torch.cuda.synchronize()
    got = _host(planes, 3 * W * H, (3, W, H), 'scatter')
    # integers up to 8 times a power of two: every partial sum (|.| <= 4096 * 16, a multiple of 1 / 4) is an fp32 number, in any order
    want = A.gather_backward(cx, cy, grads, coefs, W, H)
    assert np.array_equal(got, want)
    free = np.ones((W, H), dtype=bool)
    free[stands[:, 0], stands[:, 1]] = False
    assert free.sum() == W * H - 4 and not got[:, free].any() and np.abs(want[:, ~free]).max() >= 100


def test_gather_is_the_adjoint_of_the_scatter():
    W, H, x, y, planes, grads, coefs = A.gather_case()
    N = x.size
    xd, yd, cx, cy = _slots(x, y, W, H)
    assert np.array_equal(cx[:W * H] * H + cy[:W * H], np.arange(W * H))
    assert list(zip(cx[-4:], cy[-4:])) == [(0, 0), (0, H - 1), (W - 1, 0), (W - 1, H - 1)]
    p_dev = torch.from_numpy(planes).to(DEV)
    act = _sentinel(4 * N + TAIL)
    m, a = _medium(W, H), L.Agents(N, _ptr(xd), _ptr(yd), None, None, None)
    u = L.Action(N, *[act.data_ptr() + 4 * c * N for c in range(3)])
    L.check(L.lib.die_gather_scale(C.byref(m), C.byref(a), _plane_ptrs(p_dev, 3, W * H), (C.c_float * 3)(*coefs), C.byref(u), stream_ptr(DEV)),
            'die_gather_scale')
    scat, keep = _scatter(W, H, xd, yd, grads, coefs)
    torch.cuda.synchronize()
    action = _host(act, 3 * N, (3, N), 'gather')
    gp = _host(scat, 3 * W * H, (3, W, H), 'scatter')
    assert np.array_equal(action, A.gather(planes, cx, cy, np.asarray(coefs, dtype=np.float32)))      # one fp32 multiply per value
    want = A.gather_backward(cx, cy, grads, np.asarray(coefs, dtype=np.float32).astype(np.float64), W, H)
    assert np.abs(gp - want).max() <= 1e-6 * np.abs(want).max()
    lhs, rhs = float((action.astype(np.float64) * grads).sum()), float((planes.astype(np.float64) * gp).sum())
    print(f'conv abi read-out: <gather(planes), g> = {lhs:.9e}, <planes, scatter(g)> = {rhs:.9e}, apart by {abs(lhs - rhs) / abs(rhs):.2e} (ceiling 1e-6)')
    assert abs(lhs - rhs) <= 1e-6 * abs(rhs)
