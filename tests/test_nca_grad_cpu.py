"""The adjoint of the NeuralAutomataAgent sensing, CPU side: the three entry points are exported under the unchanged ABI version,
the workspace size is what include/die_hip.h says, every bad argument is refused on the host before any launch (fake pointers:
a launch would have failed), and the float64 oracle of the GPU tests (tests/nca_grad_model.py) agrees with finite differences.
No kernel is launched here."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import nca_grad_model as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('die_gather_scale_backward', 'die_conv2d_backward_workspace_bytes', 'die_conv2d_backward')
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


def test_new_symbols_exported_under_abi_24(lib):
    so = C.CDLL(lib.LIB_PATH)
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    for name in NEW:
        assert hasattr(so, name) and name in lib.EXPORTS, name


@pytest.mark.parametrize('W,H,cin,cout,k,tiles', [
    (16, 64, 3, 3, 3, 1), (17, 66, 3, 3, 5, 4), (24, 40, 2, 3, 3, 2), (33, 130, 3, 3, 7, 9), (1, 1, 1, 1, 1, 1),
    (96, 96, 3, 3, 3, 12), (1024, 1024, 4, 4, 7, 1024),
])
def test_workspace_bytes_is_one_partial_row_per_tile(lib, W, H, cin, cout, k, tiles):
    assert -(-W // 16) * -(-H // 64) == tiles
    assert lib.lib.die_conv2d_backward_workspace_bytes(W, H, cin, cout, k) == tiles * cout * cin * k * k * 4


@pytest.mark.parametrize('args', [(0, 8, 3, 3, 3), (8, 0, 3, 3, 3), (-1, 8, 3, 3, 3), (8, 8, 0, 3, 3), (8, 8, 5, 3, 3), (8, 8, 3, 0, 3),
                                  (8, 8, 3, 5, 3), (8, 8, 3, 3, 0), (8, 8, 3, 3, 2), (8, 8, 3, 3, 4), (8, 8, 3, 3, 9), (8, 8, 3, 3, -3)])
def test_workspace_bytes_refuses_bad_shapes(lib, args):
    assert lib.lib.die_conv2d_backward_workspace_bytes(*args) == -1


def _conv(lib, *, W=24, H=40, cin=3, cout=3, k=3, pad=0, null=None, ws_bytes=None, grad_in=True, fwd=True, drop=None, kind=0,
          null_plane=None, alias=None, p=0.25, reserved=0):
    L = lib
    planes = (L.ConvPlane * 4)(*[L.ConvPlane(FAKE + 65536 * i, kind, 0) for i in range(4)])
    ptrs = lambda base: (C.c_void_p * 4)(*[FAKE + 65536 * (base + i) for i in range(4)])
    a = dict(planes=planes, g=ptrs(8), w=FAKE + 65536 * 40, gw=FAKE + 65536 * 41, gin=ptrs(16) if grad_in else None,
             fwd=ptrs(24) if fwd else None, ws=FAKE + 65536 * 48)
    if null:
        a[null] = None
    if null_plane == 'planes':
        planes[1].data = None
    elif null_plane:
        a[null_plane][1] = None
    if alias == 'input':
        a['gin'][0] = planes[2].data
    elif alias == 'grad_out':
        a['gin'][1] = a['g'][0]
    elif alias == 'fwd_out':
        a['gin'][2] = a['fwd'][2]
    elif alias == 'itself':
        a['gin'][2] = a['gin'][0]
    elif alias == 'weights':
        a['gw'] = a['w']
    need = L.lib.die_conv2d_backward_workspace_bytes(W, H, cin, cout, k)
    d = L.NcaDropout(p, 1, 0, 0, reserved)
    return L.lib.die_conv2d_backward(W, H, cin, a['planes'], 1, cout, a['g'], k, a['w'], a['gw'], a['gin'], a['fwd'],
                                     C.byref(d) if drop else None, pad, a['ws'], max(need, 0) if ws_bytes is None else ws_bytes, None)


def _gather(lib, *, null=None, N=10, grad_N=None, null_plane=None, same_planes=False, W=24, null_array=None):
    L = lib
    m = L.Medium(W, 40, L.DIE_F32, 2, FAKE, FAKE, FAKE, FAKE + 8, 0, 0, 0, 0, 0, 0, 0, 0, None)
    ag = L.Agents(N, FAKE, None if null_array == 'x' else FAKE + 4096, None, None, None)
    u = L.Action(N if grad_N is None else grad_N, FAKE + 8192, None if null_array == 'dy' else FAKE + 12288, FAKE + 16384)
    planes = (C.c_void_p * 3)(*[FAKE + 65536 * (1 + i) for i in range(3)])
    if null_plane is not None:
        planes[null_plane] = None
    if same_planes:
        planes[2] = planes[0]
    a = dict(m=C.byref(m), ag=C.byref(ag), u=C.byref(u), coefs=(C.c_float * 3)(0.1, 0.1, 1.0), planes=planes)
    if null:
        a[null] = None
    return L.lib.die_gather_scale_backward(a['m'], a['ag'], a['u'], a['coefs'], a['planes'], None)


@pytest.mark.parametrize('case, call, kw, status, needle', [
    ('conv: null input planes', _conv, dict(null='planes'), ARG, b'null argument'),
    ('conv: null gradient planes', _conv, dict(null='g'), ARG, b'null argument'),
    ('conv: null weights', _conv, dict(null='w'), ARG, b'null argument'),
    ('conv: null grad_weights', _conv, dict(null='gw'), ARG, b'null argument'),
    ('conv: null workspace', _conv, dict(null='ws'), ARG, b'null argument'),
    ('conv: an input plane is null', _conv, dict(null_plane='planes'), ARG, b'bad input plane'),
    ('conv: an input plane of no kind', _conv, dict(kind=3), ARG, b'bad input plane'),
    ('conv: a gradient plane is null', _conv, dict(null_plane='g'), ARG, b'null gradient plane'),
    ('conv: a grad_in plane is null', _conv, dict(null_plane='gin'), ARG, b'null grad_in plane'),
    ('conv: a forward plane is null', _conv, dict(null_plane='fwd'), ARG, b'null forward output plane'),
    ('conv: empty field', _conv, dict(W=0), ARG, b'bad size'),
    ('conv: negative field', _conv, dict(H=-4), ARG, b'bad size'),
    ('conv: no input channel', _conv, dict(cin=0), ARG, b'channels'),
    ('conv: five input channels', _conv, dict(cin=5), ARG, b'channels'),
    ('conv: five output channels', _conv, dict(cout=5), ARG, b'channels'),
    ('conv: even kernel', _conv, dict(k=4), UNSUPPORTED, b'kernel size'),
    ('conv: kernel of 9', _conv, dict(k=9), UNSUPPORTED, b'kernel size'),
    ('conv: no such padding', _conv, dict(pad=4), ARG, b'bad padding mode'),
    ('conv: negative padding mode', _conv, dict(pad=-1), ARG, b'bad padding mode'),
    ('conv: reflect', _conv, dict(pad=2), UNSUPPORTED, b'not implemented'),
    ('conv: replicate', _conv, dict(pad=3), UNSUPPORTED, b'not implemented'),
    ('conv: workspace one byte short', _conv, dict(ws_bytes=2 * 81 * 4 - 1), ARG, b'workspace too small'),
    ('conv: no workspace bytes', _conv, dict(ws_bytes=0), ARG, b'workspace too small'),
    ('conv: grad_in is an input plane', _conv, dict(alias='input'), ARG, b'in-place grad_in'),
    ('conv: grad_in is a gradient plane', _conv, dict(alias='grad_out'), ARG, b'in-place grad_in'),
    ('conv: grad_in is a forward plane', _conv, dict(alias='fwd_out'), ARG, b'in-place grad_in'),
    ('conv: two grad_in planes are one', _conv, dict(alias='itself'), ARG, b'in-place grad_in'),
    ('conv: grad_weights is the weights', _conv, dict(alias='weights'), ARG, b'grad_weights is the weights'),
    ('conv: a mask without forward planes', _conv, dict(fwd=False, drop=True), ARG, b'without the forward outputs'),
    ('conv: p = 0', _conv, dict(drop=True, p=0.0), ARG, b'0 < p <= 1'),
    ('conv: p = nan', _conv, dict(drop=True, p=float('nan')), ARG, b'0 < p <= 1'),
    ('conv: reserved word set', _conv, dict(drop=True, reserved=3), ARG, b'reserved'),
    ('gather: null medium', _gather, dict(null='m'), ARG, b'null argument'),
    ('gather: null agents', _gather, dict(null='ag'), ARG, b'null argument'),
    ('gather: null gradient', _gather, dict(null='u'), ARG, b'null argument'),
    ('gather: null coefficients', _gather, dict(null='coefs'), ARG, b'null argument'),
    ('gather: null planes', _gather, dict(null='planes'), ARG, b'null argument'),
    ('gather: no slot', _gather, dict(N=0), ARG, b'bad arrays'),
    ('gather: another number of gradients', _gather, dict(grad_N=9), ARG, b'bad arrays'),
    ('gather: null coordinates', _gather, dict(null_array='x'), ARG, b'bad arrays'),
    ('gather: null gradient row', _gather, dict(null_array='dy'), ARG, b'bad arrays'),
    ('gather: a plane is null', _gather, dict(null_plane=1), ARG, b'null plane'),
    ('gather: two planes are one', _gather, dict(same_planes=True), ARG, b'are one'),
    ('gather: empty field', _gather, dict(W=0), ARG, b'bad size'),
])
def test_bad_arguments_refused_before_launch(lib, case, call, kw, status, needle):
    assert call(lib, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


def test_differentiable_mode_refuses_reflect_and_replicate_before_touching_the_medium(lib):
    from die_amd import NeuralAutomataAgent

    class NoMedium:
        def __getattr__(self, name):
            raise AssertionError(f'the medium was touched ({name}) before the refusal')

    for boundary in ('reflect', 'replicate'):
        ag = NeuralAutomataAgent(kernel_sizes=(3, 3), boundary=boundary)
        with pytest.raises(NotImplementedError, match='differentiable'):
            ag.differentiable_sense(NoMedium())
        with pytest.raises(NotImplementedError, match='differentiable'):
            ag.differentiable_action((None, NoMedium()))
        assert ag.dropout_step == 0


# ---- the oracle against finite differences (float64, a 5 x 6 field)
@pytest.mark.parametrize('padding_mode', ['circular', 'zeros'])
@pytest.mark.parametrize('sizes,masked', [((3,), False), ((3, 3), True), ((5, 1), False)])
def test_oracle_gradients_agree_with_finite_differences(padding_mode, sizes, masked):
    import torch
    W, H, N = 5, 6, 7
    rs = np.random.RandomState(len(sizes) * 10 + sizes[0] + masked)
    planes = np.stack([(rs.rand(W, H) < 0.3).astype(np.float64), rs.rand(W, H), rs.rand(W, H)])
    weights = [rs.uniform(-0.5, 0.5, (3, 3, k, k)) for k in sizes]
    cx, cy = rs.randint(0, W, N), rs.randint(0, H, N)
    cx[1], cy[1] = cx[0], cy[0]                                   # two slots on one cell
    coefs, grad_action = (0.1, 0.1, 2.0), rs.standard_normal((3, N))
    mask = (rs.rand(W, H) > 0.25) * (4.0 / 3.0) if masked else None
    act, grads = G.gradients(weights, padding_mode, planes, cx, cy, coefs, grad_action, mask)
    assert act.shape == (3, N) and [g.shape for g in grads] == [w.shape for w in weights]

    def loss(ws):
        with torch.no_grad():
            m = None if mask is None else torch.as_tensor(mask)
            a = G.action(G.layers(ws, padding_mode), torch.as_tensor(planes), cx, cy, coefs, m)
        return float((a.numpy() * grad_action).sum())

    eps = 1e-6
    for li, w in enumerate(weights):
        fd = np.zeros_like(w)
        for idx in np.ndindex(*w.shape):
            hi, lo = [x.copy() for x in weights], [x.copy() for x in weights]
            hi[li][idx] += eps
            lo[li][idx] -= eps
            fd[idx] = (loss(hi) - loss(lo)) / (2 * eps)
        # central differences: eps^2 * f''' / 6 truncation (~1e-12) plus 2^-53 * |loss| / eps rounding (~1e-10)
        assert np.abs(fd - grads[li]).max() <= 1e-7 * max(np.abs(grads[li]).max(), 1e-3), (li, np.abs(fd - grads[li]).max())
    # the action itself: indexing, coefficients and mask as stated
    with torch.no_grad():
        s = G.sense(G.layers(weights, padding_mode), torch.as_tensor(planes)).numpy()
    want = s[:, cx, cy] * np.array(coefs)[:, None] * (1.0 if mask is None else mask[cx, cy][None])
    assert np.allclose(act, want, rtol=1e-14, atol=0)
    assert np.array_equal(act[:, 0], act[:, 1])
