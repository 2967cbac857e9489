"""The batched adjoint of a wide NeuralAutomataAgent population, CPU side: the float64 model of
tests/nca_wide_grad_batch_model.py against torch's float64 autograd of the same population written as one nn.Sequential per
candidate, the fp32 yardstick of every case (torch fp32 on the CPU against the float64 model: the device ceiling of 1e-4 * max|ref|
per layer block stands only while this stays at or below 1e-5), the four new symbols and their argument counts, the byte formulas,
and every refusal of the two calls, returned on the host before any launch (fake pointers, never dereferenced).  No kernel is
launched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from torch import nn

from tests import nca_wide_grad_batch_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'die_nca_wide_sense_batch_store_bytes': 5, 'die_nca_wide_sense_batch_store': 8,
       'die_nca_wide_backward_batch_workspace_bytes': 4, 'die_nca_wide_backward_batch': 14}


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ the model and the yardstick
def _torch_population(name, dtype):
    """torch autograd of a case's population: ((C, P) gradient, [grad at replica r's planes], [hidden and last outputs of replica r])."""
    case = M.CASES[name]
    planes, weights, g, masks = M.cpu_inputs(name)
    E, mode = case.get('E', 1), case.get('boundary', 'circular')
    rows, gins, outs = [], [], []
    for c, ws in enumerate(weights):
        stack = nn.Sequential()
        for li, w in enumerate(ws):
            conv = nn.Conv2d(w.shape[1], w.shape[0], w.shape[2], padding='same', padding_mode=mode, bias=False).to(dtype)
            with torch.no_grad():
                conv.weight.copy_(torch.as_tensor(w, dtype=dtype))
            stack.append(conv)
            last = li == len(ws) - 1
            if last or case['act'] is not None:
                stack.append(nn.Tanh() if last or case['act'] == 'tanh' else nn.ReLU())
        loss = 0
        xs = []
        for e in range(E):
            r = c * E + e
            x = torch.as_tensor(planes[r], dtype=dtype).requires_grad_()
            xs.append(x)
            t, kept = x[None], []
            for module in stack:
                t = module(t)
                if not isinstance(module, nn.Conv2d):
                    kept.append(t[0].detach().numpy())
                elif case['act'] is None and module is not stack[-2]:
                    kept.append(t[0].detach().numpy())
            outs.append(kept)
            out = t[0] if masks is None else t[0] * torch.as_tensor(masks[r], dtype=dtype)
            loss = loss + (out * torch.as_tensor(g[r], dtype=dtype)).sum()
        loss.backward()
        rows.append(np.concatenate([m.weight.grad.numpy().astype(np.float64).ravel() for m in stack if isinstance(m, nn.Conv2d)]))
        gins += [x.grad.numpy().astype(np.float64) for x in xs]
    return np.stack(rows), gins, outs


def _model(name, ts=None):
    case = M.CASES[name]
    planes, weights, g, masks = M.cpu_inputs(name)
    return M.population_backward(planes, weights, g, case['act'], case.get('boundary', 'circular'), masks, case.get('E', 1), ts)


@pytest.mark.parametrize('name', sorted(M.CASES))
def test_model_matches_torch_float64_autograd(name):
    case = M.CASES[name]
    want, want_in, outs = _torch_population(name, torch.float64)
    got, got_in = _model(name)
    assert got.shape == (case['R'] // case.get('E', 1), M.row_length(case))
    for c in range(got.shape[0]):
        for li, (a, b) in enumerate(zip(M.blocks(case, got[c]), M.blocks(case, want[c]))):
            assert np.abs(b).max() > 0 and np.abs(a - b).max() <= 1e-11 * np.abs(b).max(), (c, li)
    for r, (a, b) in enumerate(zip(got_in, want_in)):
        assert np.abs(a - b).max() <= 1e-11 * np.abs(b).max(), r
    # the forward the adjoint was taken of is the forward model's
    planes, weights, g, masks = M.cpu_inputs(name)
    assert len(outs[0]) == len(case['sizes'])
    ref = M.sense(planes[0], weights[0], case['act'], case.get('boundary', 'circular'))
    assert np.abs(outs[0][-1] - ref).max() <= 1e-12


@pytest.mark.parametrize('name', sorted(M.CASES))
def test_fp32_yardstick_stays_below_1e_5(name):
    """A plain fp32 evaluation against the float64 model, per layer block; the model takes act' from the fp32 evaluation's own
    outputs, so relu's kink cannot split the two."""
    case = M.CASES[name]
    f32, _, outs = _torch_population(name, torch.float32)
    got, _ = _model(name, ts=outs)
    worst = 0.0
    for c in range(got.shape[0]):
        for li, (a, b) in enumerate(zip(M.blocks(case, f32[c]), M.blocks(case, got[c]))):
            worst = max(worst, float(np.abs(a - b).max() / np.abs(b).max()))
    print(f'wide batch yardstick {name}: fp32 torch {worst:.2e} of max|grad_f64| per layer block (must stay <= {M.YARDSTICK:.0e}; '
          f'device ceiling {M.TOL:.0e})')
    assert worst <= M.YARDSTICK


def test_episode_rows_are_sums_and_one_episode_rows_are_the_replicas():
    planes, weights, g, masks = M.cpu_inputs('two episodes')
    rows, _ = M.population_backward(planes, weights, g, 'tanh', episodes=2)
    for c in range(2):
        parts = [M.flat(M.stack_backward(planes[2 * c + e], weights[c], g[2 * c + e], 'tanh')[0]) for e in range(2)]
        assert np.array_equal(rows[c], parts[0] + parts[1])
        assert not np.array_equal(rows[c], parts[0])


# ------------------------------------------------------------------------------------------------ the ABI
def test_new_symbols_are_bound_with_their_argument_counts(lib):
    so = C.CDLL(lib.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'die_hip.h')).read()
    for name, count in NEW.items():
        assert hasattr(so, name) and name in lib.EXPORTS, name
        assert len(getattr(lib.lib, name).argtypes) == count, name
        assert name + '(' in header, name
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    assert '#define DIE_ABI_VERSION 24' in header


FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host
W, H = 24, 72
TANH = 1
STACK = ((3, 3, 8, TANH), (3, 8, 3, TANH))       # (k, cin, cout, activation)


def _structs(L, *, layers=STACK, replicas=4, episodes=0, pad=0, n=10, plane_stride=None, agent_stride=10, epoch=1, weights=FAKE, dtype=None):
    m = L.Medium(W, H, L.DIE_F32 if dtype is None else dtype, 1, FAKE, FAKE + (1 << 16), FAKE + (2 << 16), None, 0, 0, 0, 0, 0, 0, 0, 0, None)
    arr = (L.NcaLayer * len(layers))(*[L.NcaLayer(k, cin, cout, act, weights, cout * cin * k * k) for k, cin, cout, act in layers])
    nca = L.NcaBatch(len(layers), pad, 1, epoch, arr, (C.c_float * 3)(0.01, 0.01, 2.0), episodes, None, 0)
    b = L.Batch(replicas, 0, W * H if plane_stride is None else plane_stride, agent_stride, 1, (C.c_int64 * 64)(*([n] * 64)))
    return m, arr, nca, b


@pytest.mark.parametrize('Wq,Hq,R,layers', [
    (96, 96, 16, ((3, 3, 16), (3, 16, 16), (3, 16, 3))), (24, 72, 3, ((3, 3, 8), (3, 8, 3))), (20, 136, 2, ((3, 3, 16), (5, 16, 16), (3, 16, 3))),
    (24, 72, 2, ((1, 3, 32), (3, 32, 3))), (17, 66, 2, ((3, 2, 17), (3, 17, 3))), (17, 66, 1, ((5, 3, 3),)), (64, 64, 64, ((3, 3, 32),) + ((3, 32, 32),) * 6 + ((3, 32, 3),))])
def test_byte_queries_equal_the_formulas(lib, Wq, Hq, R, layers):
    arr = (lib.NcaLayer * len(layers))(*[lib.NcaLayer(k, cin, cout, TANH, FAKE, cout * cin * k * k) for k, cin, cout in layers])
    nca = lib.NcaBatch(len(layers), 0, int(layers[0][1] == 3), 1, arr, (C.c_float * 3)(0.01, 0.01, 2.0), 0, None, 0)
    want = M.workspace_bytes(Wq, Hq, R, layers)
    assert want > 0 and lib.lib.die_nca_wide_backward_batch_workspace_bytes(Wq, Hq, R, C.byref(nca)) == want
    cmax = max(c for _, _, c in layers)
    tiles = -(-Wq // 16) * -(-Hq // 64)
    assert want == 4 * (R * tiles * max(co * ci * k * k for k, ci, co in layers) + min(len(layers) - 1, 2) * R * cmax * Wq * Hq)
    assert lib.lib.die_nca_wide_sense_batch_store_bytes(Wq, Hq, R, len(layers), cmax) == M.store_bytes(Wq, Hq, R, len(layers), cmax) \
        == len(layers) * R * cmax * Wq * Hq * 4


def test_byte_queries_return_minus_one_for_refused_shapes(lib):
    for bad in ((0, 8, 1, 1, 8), (8, 0, 1, 1, 8), (8, 8, 0, 1, 8), (8, 8, 65, 1, 8), (8, 8, 1, 0, 8), (8, 8, 1, lib.NCA_MAX_LAYERS + 1, 8),
                (8, 8, 1, 1, 0), (8, 8, 1, 1, 33), (16 * 65536, 4, 1, 1, 8)):
        assert lib.lib.die_nca_wide_sense_batch_store_bytes(*bad) == -1, bad
        assert M.store_bytes(*bad) == -1, bad
    good = dict(Wq=W, Hq=H, replicas=4)
    for case, kw in (('no stack', dict(null=True)), ('W', dict(Wq=0)), ('H', dict(Hq=0)), ('no replica', dict(replicas=0)),
                     ('65 replicas', dict(replicas=65)), ('too tall', dict(Wq=16 * 65536)), ('episodes', dict(episodes=3)),
                     ('k 7', dict(layers=((7, 3, 8, TANH), (3, 8, 3, TANH)))), ('33 channels', dict(layers=((3, 3, 33, TANH), (3, 33, 3, TANH)))),
                     ('2 planes out', dict(layers=((3, 3, 8, TANH), (3, 8, 2, TANH)))), ('last relu', dict(layers=((3, 3, 8, TANH), (3, 8, 3, 2)))),
                     ('activation 3', dict(layers=((3, 3, 8, 3), (3, 8, 3, TANH)))), ('chain', dict(layers=((3, 3, 8, TANH), (3, 9, 3, TANH)))),
                     ('reflect', dict(pad=2)), ('replicate', dict(pad=3)), ('no layer', dict(layers=()))):
        kw = dict(good, **kw)
        Wq, Hq, R, null = kw.pop('Wq'), kw.pop('Hq'), kw.pop('replicas'), kw.pop('null', False)
        m, arr, nca, b = _structs(lib, **kw)
        assert lib.lib.die_nca_wide_backward_batch_workspace_bytes(Wq, Hq, R, None if null else C.byref(nca)) == -1, case
    m, arr, nca, b = _structs(lib)
    assert lib.lib.die_nca_wide_backward_batch_workspace_bytes(W, H, 4, C.byref(nca)) > 0


P_ROW = 3 * 8 * 9 + 8 * 3 * 9


def _backward(L, *, null=None, workspace_bytes=None, sense_stride=3 * W * H, grad_stride=P_ROW, drop=None, grad=None, ws=None,
              grad_in=None, grad_in_stride=3 * W * H, **kw):
    m, arr, nca, b = _structs(L, **kw)
    good = _structs(L)[2]
    need = L.lib.die_nca_wide_backward_batch_workspace_bytes(W, H, 4, C.byref(good))
    assert need > 0
    a = dict(m=C.byref(m), b=C.byref(b), nca=C.byref(nca), store=FAKE + (3 << 16), g=FAKE + (40 << 16), grad=FAKE + (50 << 16) if grad is None else grad,
             ws=FAKE + (60 << 16) if ws is None else ws)
    if null:
        a[null] = None
    return L.lib.die_nca_wide_backward_batch(a['m'], a['b'], a['nca'], a['store'], a['g'], sense_stride, a['grad'], grad_stride,
                                             None if drop is None else C.byref(L.NcaDropout(*drop)), a['ws'],
                                             need if workspace_bytes is None else workspace_bytes, grad_in, grad_in_stride, None)


GIN = FAKE + (200 << 16)             # a grad_in clear of everything else
BACKWARD_REFUSALS = [
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
    ('kernel size 7', dict(layers=((7, 3, 8, TANH), (3, 8, 3, TANH))), -1, b'kernel size 7'),
    ('even kernel', dict(layers=((4, 3, 8, TANH), (3, 8, 3, TANH))), -1, b'kernel size 4'),
    ('33 channels', dict(layers=((3, 3, 33, TANH), (3, 33, 3, TANH))), -1, b'channels'),
    ('no channel', dict(layers=((3, 3, 0, TANH), (3, 0, 3, TANH))), -1, b'channels'),
    ('last layer not 3 planes', dict(layers=((3, 3, 8, TANH), (3, 8, 2, TANH))), -1, b'last layer'),
    ('last layer not tanh', dict(layers=((3, 3, 8, TANH), (3, 8, 3, 2))), -1, b'activation'),
    ('unknown activation', dict(layers=((3, 3, 8, 3), (3, 8, 3, TANH))), -1, b'activation'),
    ('reflect', dict(pad=2), -3, b'reflect'),
    ('replicate', dict(pad=3), -3, b'reflect'),
    ('sense_epoch 0', dict(epoch=0), -1, b'sense_epoch'),
    ('sense_epoch past the last', dict(epoch=32), -1, b'sense_epoch'),
    ('planes overlap', dict(plane_stride=W * H - 1), -1, b'plane_stride'),
    ('gradient planes overlap', dict(sense_stride=3 * W * H - 1), -1, b'sense_stride'),
    ('gradient rows overlap', dict(grad_stride=P_ROW - 1), -1, b'grad_stride'),
    ('grad is the weights', dict(grad=FAKE), -1, b"weights"),
    ('workspace too small', dict(workspace_bytes=1024), -1, b'workspace too small'),
    ('workspace one byte short', dict(workspace_bytes=-1), -1, b'workspace too small'),
    ('dropout p out of range', dict(drop=(1.5, 7, 1, 0, 0)), -1, b'dropout p'),
    ('dropout reserved word', dict(drop=(0.25, 7, 1, 0, 1)), -1, b'reserved'),
    ('grad_in stride below the planes', dict(grad_in=GIN, grad_in_stride=3 * W * H - 4), -1, b'grad_in_stride'),
    ('grad_in not aligned', dict(grad_in=GIN + 4), -1, b'16-byte aligned'),
    ('grad_in stride not a multiple of 4', dict(grad_in=GIN, grad_in_stride=3 * W * H + 2), -1, b'multiple of 4'),
    ('grad_in is the store', dict(grad_in=FAKE + (3 << 16)), -1, b'aliases'),
    ('grad_in ends in the gradient planes', dict(grad_in=FAKE + (40 << 16) - 16), -1, b'aliases'),
    ('grad_in is grad', dict(grad_in=FAKE + (50 << 16)), -1, b'aliases'),
    ('grad_in in the workspace', dict(grad_in=FAKE + (60 << 16) + 64), -1, b'aliases'),
    ('grad_in is the chem plane', dict(grad_in=FAKE + (2 << 16)), -1, b'aliases'),
    ('grad_in is the food plane of the last replica', dict(grad_in=FAKE + (1 << 16) + 3 * 4 * W * H), -1, b'aliases'),
    ('grad_in is the claim plane', dict(grad_in=FAKE), -1, b'aliases'),
    ('grad_in holds the weights', dict(grad_in=GIN, weights=GIN + 64), -1, b"weights"),
    ('bad field dtype', dict(dtype=7), -1, b'dtype'),
]


@pytest.mark.parametrize('case, kw, rc, needle', BACKWARD_REFUSALS, ids=[c[0] for c in BACKWARD_REFUSALS])
def test_backward_refused_before_launch(lib, case, kw, rc, needle):
    if kw.get('workspace_bytes') == -1:
        kw = dict(kw, workspace_bytes=lib.lib.die_nca_wide_backward_batch_workspace_bytes(W, H, 4, C.byref(_structs(lib)[2])) - 1)
    assert _backward(lib, **kw) == rc, (case, lib.lib.die_last_error())
    err = lib.lib.die_last_error()
    assert needle in err and b'die_nca_wide_backward_batch' in err, (case, err)


def _sense(L, *, null=None, store_bytes=None, drop=None, masked=None, **kw):
    m, arr, nca, b = _structs(L, **kw)
    need = L.lib.die_nca_wide_sense_batch_store_bytes(W, H, 4, 2, 8)
    a = dict(m=C.byref(m), b=C.byref(b), nca=C.byref(nca), store=FAKE + (3 << 16))
    if null:
        a[null] = None
    return L.lib.die_nca_wide_sense_batch_store(a['m'], a['b'], a['nca'], a['store'], need if store_bytes is None else store_bytes, masked,
                                                None if drop is None else C.byref(L.NcaDropout(*drop)), None)


SENSE_REFUSALS = [
    ('null medium', dict(null='m'), b'null argument'),
    ('null batch', dict(null='b'), b'null argument'),
    ('null stack', dict(null='nca'), b'null argument'),
    ('null store', dict(null='store'), b'null argument'),
    ('no replica', dict(replicas=0), b'replicas'),
    ('65 replicas', dict(replicas=65), b'replicas'),
    ('episodes do not divide the replicas', dict(replicas=4, episodes=3), b'episodes'),
    ('kernel size 7', dict(layers=((7, 3, 8, TANH), (3, 8, 3, TANH))), b'kernel size 7'),
    ('33 channels', dict(layers=((3, 3, 33, TANH), (3, 33, 3, TANH))), b'channels'),
    ('last layer not tanh', dict(layers=((3, 3, 8, TANH), (3, 8, 3, 0))), b'activation'),
    ('unknown activation', dict(layers=((3, 3, 8, 9), (3, 8, 3, TANH))), b'activation'),
    ('sense_epoch 0', dict(epoch=0), b'sense_epoch'),
    ('planes overlap', dict(plane_stride=W * H - 1), b'plane_stride'),
    ('store too small', dict(store_bytes=1024), b'store too small'),
    ('mask without planes for the masked values', dict(drop=(0.25, 7, 1, 0, 0)), b'masked'),
    ('masked values in the store', dict(drop=(0.25, 7, 1, 0, 0), masked=FAKE + (3 << 16)), b'masked'),
    ('p out of range', dict(drop=(1.5, 7, 1, 0, 0), masked=FAKE + (90 << 16)), b'dropout p'),
]


@pytest.mark.parametrize('case, kw, needle', SENSE_REFUSALS, ids=[c[0] for c in SENSE_REFUSALS])
def test_sense_store_refused_before_launch(lib, case, kw, needle):
    assert _sense(lib, **kw) == -1, (case, lib.lib.die_last_error())
    err = lib.lib.die_last_error()
    assert needle in err and b'die_nca_wide_sense_batch_store' in err, (case, err)


def test_python_surface_needs_no_device(lib):
    import inspect
    from die_amd import functional
    from die_amd.batch import BatchedNeuralAutomataAgent
    assert list(inspect.signature(BatchedNeuralAutomataAgent.forward_device).parameters) == ['self', 'parameters']
    assert inspect.signature(BatchedNeuralAutomataAgent.forward_device).parameters['parameters'].default is None
    assert list(inspect.signature(functional.gather_scale_batch).parameters) == ['sense', 'population']
    with pytest.raises(TypeError):
        functional.gather_scale_batch(torch.zeros((1, 3, 4, 4)), object())
