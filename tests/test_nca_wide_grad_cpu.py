"""The wide layer's adjoint, CPU side.  No kernel is launched here.

1. The float64 numpy model (tests/nca_wide_grad_model.py) against torch's own float64 autograd of the convolution, the activation
   and the mask, on EVERY layer case (the padding is written out by indexing, so torch also takes the fields smaller than the
   radius, which nn.Conv2d's 'circular' refuses): 1e-12 of max|.| per array (sums of at most 4 290 * 1 or 32 * 25 terms of order 1
   in two orders: n * 2^-53 leaves a factor of a few hundred).
2. The fp32 yardstick: torch's fp32 autograd of every case against the model (which is handed that evaluation's own fp32 forward
   output as t), max|fp32 - f64| / max|f64| per array.  Worst measured: grad_w 2.1e-6 (5 -> 4, k = 5 on 33 x 130), grad_in 9.9e-7
   (17 -> 16, k = 5 on 17 x 66); the long sums of 32 -> 32 over 33 x 130 stay under 1.9e-6.  Every case stays at or below 1e-5, so the device ceiling of
   tests/test_gpu_nca_wide_grad.py is the project's backward tolerance, 1e-4 * max|ref| per array, with the tenfold margin
   tests/test_gpu_nca_grad.py and tests/test_gpu_conv_abi.py have; no case had to be drawn again beyond
   tests/conv_adjoint_model.REDRAWN.
3. Every refusal of die_conv2d_wide_backward and its workspace query comes back on the host, with its code and message, before any
   launch (ctypes on the built library, fake pointers that are never dereferenced).
4. include/die_hip.h declares the two symbols, die_amd._lib binds them, the ABI version stays.
5. The relu stack of the forward_device test keeps every hidden pre-activation away from the kink, in the float64 model alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import nca_wide_grad_model as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('die_conv2d_wide_backward_workspace_bytes', 'die_conv2d_wide_backward')
F64_TOL = 1e-12
YARDSTICK = 1e-5


def torch_eval(x, w, g, mode, activation, mask, dtype):
    """(t = act(z) unmasked, grad_w, grad_in) of <act(conv(x, w)) * mask, g> by torch autograd in `dtype`; t in `dtype`, the
    gradients as float64 arrays."""
    k = w.shape[-1]
    r = k // 2
    xt = torch.as_tensor(x, dtype=dtype).clone().requires_grad_(True)
    wt = torch.as_tensor(w, dtype=dtype).clone().requires_grad_(True)
    _, W, H = xt.shape
    if mode == 'circular':
        ix, iy = (torch.arange(W + 2 * r) - r) % W, (torch.arange(H + 2 * r) - r) % H
        xp = xt[:, ix[:, None], iy[None, :]]
    else:
        xp = torch.nn.functional.pad(xt, (r, r, r, r))
    z = torch.nn.functional.conv2d(xp[None], wt)[0]
    t = z if activation is None else torch.tanh(z) if activation == 'tanh' else torch.relu(z)
    y = t if mask is None else t * torch.as_tensor(mask, dtype=dtype)
    (y * torch.as_tensor(g, dtype=dtype)).sum().backward()
    return t.detach().numpy(), wt.grad.to(torch.float64).numpy(), xt.grad.to(torch.float64).numpy()


def _rel(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


@pytest.mark.parametrize('mode', G.MODES)
@pytest.mark.parametrize('k', G.KS)
def test_model_matches_torch_float64_autograd_on_every_case(k, mode):
    worst = 0.0
    for cin, cout, W, H, act, masked in G.layer_cases(k, mode):
        c = G.case_inputs(k, mode, cin, cout, W, H)
        mask = G.case_mask(c, W, H, masked)
        t, gw, gi = torch_eval(c['x'], c['w'], c['g'], mode, act, mask, torch.float64)
        assert _rel(G.act_forward(G.conv(c['x'], c['w'], mode), act), t) <= F64_TOL
        mw, mi = G.layer_backward(c['x'], c['w'], c['g'], t, act, mask, mode)
        errs = (_rel(mw, gw), _rel(mi, gi))
        worst = max(worst, *errs)
        assert max(errs) <= F64_TOL, (cin, cout, W, H, act, masked, errs)
    print(f'wide adjoint model vs torch float64, k = {k} {mode}: worst {worst:.2e} of max|.| (ceiling {F64_TOL:.0e})')


@pytest.mark.parametrize('mode', G.MODES)
@pytest.mark.parametrize('k', G.KS)
def test_fp32_evaluation_of_every_case_stays_within_the_yardstick(k, mode):
    worst = dict(grad_w=(0.0, None), grad_in=(0.0, None))
    for case in G.layer_cases(k, mode):
        cin, cout, W, H, act, masked = case
        c = G.case_inputs(k, mode, cin, cout, W, H)
        mask = G.case_mask(c, W, H, masked)
        t32, gw32, gi32 = torch_eval(c['x'], c['w'], c['g'], mode, act, mask, torch.float32)
        assert t32.dtype == np.float32
        mw, mi = G.layer_backward(c['x'], c['w'], c['g'], t32, act, mask, mode)
        for name, err in (('grad_w', _rel(gw32, mw)), ('grad_in', _rel(gi32, mi))):
            if err > worst[name][0]:
                worst[name] = (err, case)
    print(f'wide adjoint fp32 yardstick k = {k} {mode}: ' + '  '.join(f'{n} {v:.2e} at {where}' for n, (v, where) in worst.items()) +
          f'  (of max|f64| per array; ceiling {YARDSTICK:.0e})')
    for name, (err, where) in worst.items():
        assert err <= YARDSTICK, (name, where, err)


def test_case_list_is_pinned():
    assert G.SHAPES == ((16, 64), (17, 66), (20, 68), (33, 130), (1, 1), (2, 3), (3, 2), (5, 4))
    assert G.PAIRS == ((1, 1), (3, 16), (16, 3), (4, 5), (5, 4), (17, 16), (16, 17), (32, 32)) and G.KS == (1, 3, 5)
    assert len(G.layer_cases(1, 'circular')) == 64 and len(G.layer_cases(3, 'zeros')) == 64 + 3 * 3 * 5 == len(G.layer_cases(5, 'circular'))
    crossed = {(a, m) for *_, a, m in G.layer_cases(5, 'zeros')[64:]}
    assert crossed == {(a, m) for a in G.ACTIVATIONS for m in (False, True)} - {(None, False)}
    from tests import conv_adjoint_model as A
    a, b = G.case_inputs(3, 'zeros', 17, 16, 5, 4), A.case_inputs(3, 'zeros', 17, 16, 5, 4)
    assert all(np.array_equal(a[n], b[n]) for n in 'xwg')                   # drawn as case_inputs draws them


# ------------------------------------------------------------------------------------------------ 3. the refusals
@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


def test_new_symbols_declared_bound_and_abi_unchanged(lib):
    so = C.CDLL(lib.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'die_hip.h')).read()
    for name in NEW:
        assert hasattr(so, name) and name in lib.EXPORTS, name
        assert re.search(r'\b' + name + r'\(', header), name
        assert getattr(lib.lib, name).argtypes is not None
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24 and re.search(r'#define\s+DIE_ABI_VERSION\s+24\b', header)
    assert len(lib.lib.die_conv2d_wide_backward.argtypes) == 21
    import die_amd
    assert die_amd.functional.conv2d_wide and die_amd.functional.gather_scale and hasattr(die_amd.ConvolutionModel, 'forward_device')


@pytest.mark.parametrize('W,H,cin,cout,k', [(16, 64, 1, 1, 1), (17, 66, 3, 16, 3), (33, 130, 32, 32, 5), (1024, 1024, 32, 32, 5), (5, 4, 17, 16, 3)])
def test_workspace_formula(lib, W, H, cin, cout, k):
    assert lib.lib.die_conv2d_wide_backward_workspace_bytes(W, H, cin, cout, k) == -(-W // 16) * -(-H // 64) * cout * cin * k * k * 4


def test_workspace_query_returns_minus_one_for_refused_shapes(lib):
    for bad in ((0, 8, 3, 3, 3), (8, 0, 3, 3, 3), (8, 8, 0, 3, 3), (8, 8, 3, 0, 3), (8, 8, 33, 3, 3), (8, 8, 3, 33, 3), (8, 8, 3, 3, 7),
                (8, 8, 3, 3, 2), (8, 8, 3, 3, 0), (16 * 65536, 4, 3, 3, 3)):
        assert lib.lib.die_conv2d_wide_backward_workspace_bytes(*bad) == -1, bad


FAKE = 1 << 24                       # never dereferenced: every call below is refused on the host
W0, H0, CIN, COUT, K0 = 24, 40, 5, 17, 3
CELLS, NW = W0 * H0, 17 * 5 * 9


def _call(L, *, W=W0, H=H0, cin=CIN, cout=COUT, k=K0, act=1, pad=0, null=(), kinds=None, g_stride=CELLS, t_stride=CELLS, gin_stride=CELLS,
          ws_bytes=None, drop=None, gin='far', gw=None, in_data=None):
    """One die_conv2d_wide_backward on disjoint fake buffers, with the named deviations."""
    span = 64 * CELLS * 4                                         # more than any buffer of the call
    a = dict(in_=FAKE, g=FAKE + span, t=FAKE + 2 * span, w=FAKE + 3 * span, gw=FAKE + 4 * span, gin=FAKE + 5 * span, ws=FAKE + 6 * span)
    if gin != 'far':
        a['gin'] = gin if not isinstance(gin, str) else a[gin]
    if gw is not None:
        a['gw'] = a[gw]
    for n in null:
        a[n] = None
    planes = None
    if a['in_'] is not None:
        n = max(1, min(cin, 32))
        planes = (L.ConvPlane * n)(*[L.ConvPlane((in_data[c] if in_data else a['in_'] + 8 * c * CELLS), (kinds or [0] * 32)[c], 0)
                                     for c in range(n)])
    need = L.lib.die_conv2d_wide_backward_workspace_bytes(W, H, cin, cout, k)
    return L.lib.die_conv2d_wide_backward(W, H, cin, planes, 1, cout, a['g'], g_stride, a['t'], t_stride, k, a['w'], act, pad,
                                          None if drop is None else C.byref(drop), a['gw'], a['gin'], gin_stride, a['ws'],
                                          max(need, 0) if ws_bytes is None else ws_bytes, None)


def _bad_drop(L):
    return L.NcaDropout(0.0, 1, 0, 0, 0)


@pytest.mark.parametrize('case, kw, rc, needle', [
    ('bad padding mode', dict(pad=4), -1, b'bad padding mode'),
    ('negative padding mode', dict(pad=-1), -1, b'bad padding mode'),
    ('reflect', dict(pad=2), -3, b"the adjoint of 'reflect' / 'replicate' padding is not implemented ('circular' and 'zeros' are)"),
    ('replicate', dict(pad=3), -3, b"the adjoint of 'reflect' / 'replicate' padding is not implemented ('circular' and 'zeros' are)"),
    ('no rows', dict(W=0), -1, b'bad size'),
    ('no columns', dict(H=0), -1, b'bad size'),
    ('too tall', dict(W=16 * 65536), -1, b'too tall'),
    ('no input channel', dict(cin=0), -1, b'channels'),
    ('33 input channels', dict(cin=33), -1, b'channels'),
    ('33 output channels', dict(cout=33), -1, b'channels'),
    ('kernel size 7', dict(k=7), -1, b'kernel size 7'),
    ('even kernel', dict(k=2), -1, b'kernel size 2'),
    ('bad activation', dict(act=3), -1, b'bad activation'),
    ('null inputs', dict(null=('in_',)), -1, b'null argument'),
    ('null grad_out', dict(null=('g',)), -1, b'null argument'),
    ('null weights', dict(null=('w',)), -1, b'null argument'),
    ('null grad_weights', dict(null=('gw',)), -1, b'null argument'),
    ('null workspace', dict(null=('ws',)), -1, b'null argument'),
    ('tanh without fwd_out', dict(null=('t',), act=1), -1, b'without the forward outputs'),
    ('relu without fwd_out', dict(null=('t',), act=2), -1, b'without the forward outputs'),
    ('mask without fwd_out', dict(null=('t',), act=0, drop='ok'), -1, b'without the forward outputs'),
    ('grad_weights is the weights', dict(gw='w'), -1, b'grad_weights is the weights'),
    ('grad_out planes overlap', dict(g_stride=CELLS - 1), -1, b'grad_out_stride'),
    ('fwd_out planes overlap', dict(t_stride=CELLS - 1), -1, b'fwd_out_stride'),
    ('grad_in planes overlap', dict(gin_stride=CELLS - 1), -1, b'grad_in_stride'),
    ('workspace too small', dict(ws_bytes=NW * 4 - 4), -1, b'workspace too small'),
    ('bad input plane kind', dict(kinds=[0, 0, 3, 0, 0] + [0] * 27), -1, b'bad input plane 2'),
    ('null input plane', dict(in_data=[FAKE, 0, FAKE, FAKE, FAKE]), -1, b'bad input plane 1'),
    ('grad_in is an input plane', dict(gin='in_'), -1, b'grad_in aliases'),
    ('grad_in ends inside the inputs', dict(gin=FAKE - 4 * CIN * CELLS + 16), -1, b'grad_in aliases'),
    ('grad_in is grad_out', dict(gin='g'), -1, b'grad_in aliases'),
    ('grad_in is fwd_out', dict(gin='t'), -1, b'grad_in aliases'),
    ('grad_in is the weights', dict(gin='w'), -1, b'grad_in aliases'),
    ('grad_in is grad_weights', dict(gin='gw'), -1, b'grad_in aliases'),
    ('grad_in is the workspace', dict(gin='ws'), -1, b'grad_in aliases'),
    ('grad_in misaligned where H % 4 == 0', dict(gin=FAKE + 5 * 64 * CELLS * 4 + 4), -1, b'16-byte aligned'),
    ('grad_in_stride odd where H % 4 == 0', dict(gin_stride=CELLS + 1), -1, b'multiple of 4'),
    ('p = 0', dict(drop='bad'), -1, b'die_conv2d_wide_backward'),
])
def test_backward_refused_before_launch(lib, case, kw, rc, needle):
    kw = dict(kw)
    if kw.get('drop') == 'ok':
        kw['drop'] = lib.nca_dropout(0.25, 1, 0, 0)
    elif kw.get('drop') == 'bad':
        kw['drop'] = _bad_drop(lib)
    assert _call(lib, **kw) == rc, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


def test_null_fwd_out_is_fine_without_activation_and_mask_until_the_next_check(lib):
    """act none, no drop, fwd_out NULL: that check passes and the NEXT refusal (a workspace one byte short) is what comes back."""
    assert _call(lib, null=('t',), act=0, ws_bytes=NW * 4 - 1) == -1
    assert b'workspace too small' in lib.lib.die_last_error()


# ------------------------------------------------------------------------------------------------ 5. the relu stack and its kink
def test_relu_stack_seeds_keep_hidden_pre_activations_off_the_kink():
    checked = 0
    for width, ks, act, seed in G.STACKS:
        if act != 'relu':
            continue
        for W, H in G.STACK_FIELDS:
            planes, weights, _ = G.stack_case(width, ks, act, seed, W, H)
            zs = G.stack_pre_activations(planes, weights, act)[:-1]
            for li, z in enumerate(zs):
                live = np.abs(z[z != 0])                            # a cell at exactly 0 has relu' = 0 in either convention
                assert live.size > z.size // 2, (W, H, li, 'the layer is mostly dead')
                assert live.min() >= 1e-4 * np.abs(z).max(), (W, H, li, live.min(), np.abs(z).max())
                assert (z > 0).mean() > 0.1 and (z < 0).mean() > 0.1, (W, H, li, 'one-sided')
                # exact in fp32 too: the values are small multiples of 2^-10
                assert np.array_equal(z, np.round(z * 1024) / 1024) and np.abs(z).max() < 2 ** 13
                checked += 1
    assert checked == 4
