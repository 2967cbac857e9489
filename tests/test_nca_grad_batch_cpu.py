"""The batched adjoint of the NeuralAutomataAgent sensing, CPU side: the library exports the new entry points, their workspace and
storage formulas are the documented ones, every refusal is returned on the host before any launch (fake pointers, never
dereferenced), and the numpy model of the fold order reduces, for E = 1, to the stand-alone tile-order sum.  No kernel is launched."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import nca_grad_batch_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('die_nca_sense_batch_store_bytes', 'die_nca_sense_batch_store', 'die_gather_scale_batch', 'die_gather_scale_backward_batch',
       'die_nca_backward_batch_workspace_bytes', 'die_nca_backward_batch')


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


def test_new_symbols_exported_and_abi_unchanged(lib):
    so = C.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert hasattr(so, name) and name in lib.EXPORTS, name
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    header = open(os.path.join(ROOT, 'include', 'die_hip.h')).read()
    for name in NEW:
        assert name + '(' in header, name
    assert '#define DIE_ABI_VERSION 24' in header


@pytest.mark.parametrize('W,H,R,L', [(96, 96, 16, 2), (24, 40, 3, 2), (20, 68, 2, 3), (33, 132, 2, 2), (17, 66, 1, 1), (64, 64, 64, 8)])
def test_workspace_and_store_formulas(lib, W, H, R, L):
    assert lib.lib.die_nca_backward_batch_workspace_bytes(W, H, R, L) == M.workspace_bytes(W, H, R, L)
    assert lib.lib.die_nca_sense_batch_store_bytes(W, H, R, L) == L * R * 4 * W * H * 4


def test_queries_return_minus_one_for_refused_shapes(lib):
    for bad in ((0, 8, 1, 1), (8, 0, 1, 1), (8, 8, 0, 1), (8, 8, 65, 1), (8, 8, 1, 0), (8, 8, 1, lib.NCA_MAX_LAYERS + 1)):
        assert lib.lib.die_nca_backward_batch_workspace_bytes(*bad) == -1, bad
        assert lib.lib.die_nca_sense_batch_store_bytes(*bad) == -1, bad
        assert M.workspace_bytes(*bad) == -1
    assert lib.lib.die_nca_backward_batch_workspace_bytes(16 * 65536, 4, 1, 1) == -1      # more rows of tiles than a grid takes


FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host
W, H = 24, 40


def _structs(L, *, layers=((3, 3, 3), (3, 3, 3)), replicas=4, episodes=0, pad=0, n=10, plane_stride=None, agent_stride=10):
    m = L.Medium(W, H, L.DIE_F32, 1, FAKE, FAKE, FAKE, None, 0, 0, 0, 0, 0, 0, 0, 0, None)
    arr = (L.NcaLayer * len(layers))(*[L.NcaLayer(k, cin, cout, 0, FAKE, cout * cin * k * k) for k, cin, cout in layers])
    nca = L.NcaBatch(len(layers), pad, 1, 1, arr, (C.c_float * 3)(0.01, 0.01, 2.0), episodes, None, 0)
    b = L.Batch(replicas, 0, W * H if plane_stride is None else plane_stride, agent_stride, 1, (C.c_int64 * 64)(*([n] * 64)))
    return m, arr, nca, b


def _backward(L, *, null=None, workspace_bytes=None, sense_stride=3 * W * H, grad_stride=162, **kw):
    m, arr, nca, b = _structs(L, **kw)
    need = L.lib.die_nca_backward_batch_workspace_bytes(W, H, max(1, min(64, kw.get('replicas', 4))), len(kw.get('layers', (0, 0))))
    a = dict(m=C.byref(m), b=C.byref(b), nca=C.byref(nca), store=FAKE, g=FAKE + 64, grad=FAKE + 128, ws=FAKE + 256)
    if null:
        a[null] = None
    return L.lib.die_nca_backward_batch(a['m'], a['b'], a['nca'], a['store'], a['g'], sense_stride, a['grad'], grad_stride, None, a['ws'],
                                        need if workspace_bytes is None else workspace_bytes, None)


@pytest.mark.parametrize('case, kw, rc, needle', [
    ('null medium', dict(null='m'), -1, b'null argument'),
    ('null batch', dict(null='b'), -1, b'null argument'),
    ('null stack', dict(null='nca'), -1, b'null argument'),
    ('null store', dict(null='store'), -1, b'null argument'),
    ('null gradient planes', dict(null='g'), -1, b'null argument'),
    ('null grad', dict(null='grad'), -1, b'null argument'),
    ('null workspace', dict(null='ws'), -1, b'null argument'),
    ('no replica', dict(replicas=0), -1, b'replicas'),
    ('65 replicas', dict(replicas=65), -1, b'replicas'),
    ('episodes do not divide the replicas', dict(replicas=4, episodes=3), -1, b'episodes'),
    ('even kernel', dict(layers=((4, 3, 3),)), -1, b'kernel size 4'),
    ('kernel above 7', dict(layers=((9, 3, 3),)), -1, b'kernel size 9'),
    ('five channels', dict(layers=((3, 3, 5), (3, 5, 3))), -1, b'channels'),
    ('last layer not 3 planes', dict(layers=((3, 3, 2),)), -1, b'last layer'),
    ('reflect', dict(pad=2), -3, b'reflect'),
    ('replicate', dict(pad=3), -3, b'reflect'),
    ('workspace too small', dict(workspace_bytes=1024), -1, b'workspace too small'),
    ('planes overlap', dict(plane_stride=W * H - 1), -1, b'plane_stride'),
    ('more agents than the stride', dict(n=11), -1, b'agents'),
    ('gradient planes overlap', dict(sense_stride=3 * W * H - 1), -1, b'sense_stride'),
    ('gradient rows overlap', dict(grad_stride=161), -1, b'grad_stride'),
])
def test_backward_refused_before_launch(lib, case, kw, rc, needle):
    assert _backward(lib, **kw) == rc, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


def _sense(L, *, null=None, store_bytes=None, drop=None, masked=None, **kw):
    m, arr, nca, b = _structs(L, **kw)
    need = L.lib.die_nca_sense_batch_store_bytes(W, H, max(1, min(64, kw.get('replicas', 4))), len(kw.get('layers', (0, 0))))
    a = dict(m=C.byref(m), b=C.byref(b), nca=C.byref(nca), store=FAKE)
    if null:
        a[null] = None
    return L.lib.die_nca_sense_batch_store(a['m'], a['b'], a['nca'], a['store'], need if store_bytes is None else store_bytes, masked,
                                           None if drop is None else C.byref(drop), None)


@pytest.mark.parametrize('case, kw, needle', [
    ('null medium', dict(null='m'), b'null argument'),
    ('null batch', dict(null='b'), b'null argument'),
    ('null stack', dict(null='nca'), b'null argument'),
    ('null store', dict(null='store'), b'null argument'),
    ('no replica', dict(replicas=0), b'replicas'),
    ('65 replicas', dict(replicas=65), b'replicas'),
    ('episodes do not divide the replicas', dict(replicas=4, episodes=3), b'episodes'),
    ('even kernel', dict(layers=((4, 3, 3),)), b'kernel size 4'),
    ('five channels', dict(layers=((3, 3, 5), (3, 5, 3))), b'channels'),
    ('store too small', dict(store_bytes=1024), b'store too small'),
    ('mask without planes for the masked values', dict(drop=(0.25, 7, 1, 0, 0)), b'masked'),
    ('p out of range', dict(drop=(1.5, 7, 1, 0, 0), masked=FAKE + 512), b'dropout p'),
])
def test_sense_store_refused_before_launch(lib, case, kw, needle):
    if 'drop' in kw:
        kw = dict(kw, drop=lib.NcaDropout(*kw['drop']))
    assert _sense(lib, **kw) == -1, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


@pytest.mark.parametrize('backward', [False, True])
@pytest.mark.parametrize('case, kw, needle', [
    ('null medium', dict(null='m'), b'null argument'),
    ('null agents', dict(null='a'), b'null argument'),
    ('null batch', dict(null='b'), b'null argument'),
    ('null planes', dict(null='planes'), b'null argument'),
    ('null coefficients', dict(null='coefs'), b'null argument'),
    ('null action', dict(null='act'), b'null argument'),
    ('no replica', dict(replicas=0), b'replicas'),
    ('65 replicas', dict(replicas=65), b'replicas'),
    ('planes overlap', dict(sense_stride=3 * W * H - 1), b'sense_stride'),
    ('more agents than the stride', dict(n=11), b'agents'),
    ('null x', dict(x=None), b'bad arrays'),
])
def test_read_out_and_its_adjoint_refused_before_launch(lib, backward, case, kw, needle):
    L = lib
    kw = dict(kw)
    null, x, stride = kw.pop('null', None), kw.pop('x', FAKE), kw.pop('sense_stride', 4 * W * H)
    m, arr, nca, b = _structs(L, **kw)
    ag = L.Agents(10, x, FAKE, None, None, None)
    act = L.Action(10, FAKE, FAKE, FAKE)
    a = dict(m=C.byref(m), a=C.byref(ag), b=C.byref(b), planes=FAKE, coefs=(C.c_float * 3)(0.1, 0.1, 2.0), act=C.byref(act))
    if null:
        a[null] = None
    if backward:
        rc = L.lib.die_gather_scale_backward_batch(a['m'], a['a'], a['b'], a['act'], a['coefs'], a['planes'], stride, None)
    else:
        rc = L.lib.die_gather_scale_batch(a['m'], a['a'], a['b'], a['planes'], stride, a['coefs'], a['act'], None)
    assert rc == -1, (case, L.lib.die_last_error())
    assert needle in L.lib.die_last_error(), (case, L.lib.die_last_error())


def test_fold_order_reduces_to_the_stand_alone_sum_for_one_episode():
    rs = np.random.RandomState(0)
    R, T, nw = 6, M.tiles(33, 132), 81
    assert T == 9
    # terms of very different size: rounding each replica's sum to fp32 first and adding those (E > 1 below) is visibly another result
    part = (rs.standard_normal((R, T, nw)) * 10.0 ** rs.randint(-6, 7, (R, T, nw))).astype(np.float32)
    one = M.fold_batch(part, 1)
    for r in range(R):
        assert np.array_equal(one[r], M.fold_stand_alone(part[r])), r
    # E > 1: candidate c's rows one behind the other, one walk, one rounding — not the fp32 sum of its replicas' gradients
    for E in (2, 3):
        got = M.fold_batch(part, E)
        assert got.shape == (R // E, nw)
        for c in range(R // E):
            assert np.array_equal(got[c], M.fold_stand_alone(part[c * E:(c + 1) * E].reshape(E * T, nw))), (E, c)
            exact = part[c * E:(c + 1) * E].astype(np.float64).sum(axis=(0, 1))
            assert np.abs(got[c] - exact).max() <= 2.0 ** -23 * np.abs(exact).max() + 1e-30
        assert not np.array_equal(got, sum(one[e::E] for e in range(E)))


def test_python_refusals_need_no_device(lib):
    """What the Python layer refuses on its own arguments (the device-side refusals: tests/test_gpu_nca_grad_batch.py)."""
    from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent
    for name in ('differentiable_action', 'differentiable_sense', '_check_differentiable'):
        assert hasattr(BatchedNeuralAutomataAgent, name), name
    import inspect
    assert 'action' in inspect.signature(BatchedEnv.step).parameters
    assert inspect.signature(BatchedEnv.step).parameters['action'].default is None
