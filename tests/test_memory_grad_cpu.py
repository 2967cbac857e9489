"""Gradients through memory channels (NeuralAutomataAgent.recurrent_action, die_memory_grad.hip), CPU side: the model's two
adjoints (tests/memory_grad_model.py) against their defining identities and against torch's float64 autograd of the recurrent
loop, the fp32 error figure the GPU ceiling rests on, `recurrent_action`'s refusals on stub objects, and the three new symbols
with their host-side argument checks (fake pointers: a launch would have failed).  No kernel is launched here."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import memory_grad_model as MG
from tests import memory_model as M
from tests import stock_plane_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'die_memory_cells': 7, 'die_memory_planes_backward': 10, 'die_gather_memory_backward': 10}
FAKE = 1 << 20
ARG, UNSUPPORTED = -1, -3
FP32_FIGURE = 1e-5                   # the fp32 loop's worst max|err| / max|ref| per gradient array: the GPU ceiling (1e-4) rests on it


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------- the record and the adjoints
def _crafted_record(permuted: bool):
    W, H = MG.CRAFTED
    _, agents = MG.crafted_world()
    alive = agents[2] > 0
    x, y = MG.label_words(np.rint(agents[0] * (W - 1)), W), MG.label_words(np.rint(agents[1] * (H - 1)), H)
    if permuted:                                                     # storage entry j holds slot perm[j]: the record is by slot id all the same
        perm = np.random.RandomState(5).permutation(len(x))
        x, y, alive = (M.to_slot_order(v[perm], perm) for v in (x, y, alive))
    return W, H, MG.record(W, H, x, y, alive)


def test_the_record_of_the_crafted_world():
    W, H, (cell, win) = _crafted_record(False)
    assert cell.dtype == win.dtype == np.int32
    assert cell.tolist() == [21, 13, -1, 6, 13, -1, 29, 21, 17, 13, 4, 25]
    assert win.tolist() == [-1, -1, -1, 6, -1, -1, 29, 21, 17, 13, 4, 25]          # 9 wins (2, 3), 7 wins (4, 1); dead slots -1
    assert _crafted_record(True)[2][0].tolist() == cell.tolist() and _crafted_record(True)[2][1].tolist() == win.tolist()


@pytest.mark.parametrize('permuted', [False, True])
def test_adjoint_identities(permuted):
    W, H, (cell, win) = _crafted_record(permuted)
    rs = np.random.RandomState(11)
    N = len(cell)
    for Mc in (1, 3):
        m, p = rs.standard_normal((Mc, N)), rs.standard_normal((Mc, W, H))
        lhs, rhs = (MG.expand(W, H, win, m) * p).sum(), (m * MG.expand_adjoint(W, H, win, p)).sum()
        assert abs(lhs - rhs) <= 1e-13 * max(1.0, abs(lhs)), (lhs, rhs)
        s, g = rs.standard_normal((Mc, W, H)), rs.standard_normal((Mc, N))
        lhs, rhs = (MG.gather(W, H, cell, s) * g).sum(), (s * MG.gather_adjoint(W, H, cell, g)).sum()
        assert abs(lhs - rhs) <= 1e-13 * max(1.0, abs(lhs)), (lhs, rhs)
        # the losers and the dead get no gradient from the expand; three slots' gradients meet on the crowded cell
        assert not MG.expand_adjoint(W, H, win, p)[:, win < 0].any()
        assert np.allclose(MG.gather_adjoint(W, H, cell, g)[:, 2, 3], g[:, [1, 4, 9]].sum(axis=1), rtol=0, atol=1e-15)


def test_the_maps_agree_with_the_memory_model():
    W, H = MG.CRAFTED
    _, agents = MG.crafted_world()
    x, y = MG.label_words(np.rint(agents[0] * (W - 1)), W), MG.label_words(np.rint(agents[1] * (H - 1)), H)
    cell, win = MG.record(W, H, x, y, agents[2] > 0)
    rs = np.random.RandomState(3)
    mem, planes = rs.standard_normal((2, 12)).astype(np.float32), rs.standard_normal((2, W, H)).astype(np.float32)
    assert np.array_equal(MG.expand(W, H, win, mem, np.float32), M.expand(W, H, x, y, agents[2] > 0, mem))
    assert np.array_equal(MG.gather(W, H, cell, planes, np.float32), M.gather(W, H, x, y, agents[2] > 0, planes))


# ---------------------------------------------------------------------------------------------------- the loop
W_, H_, N_, T_ = 9, 7, 14, 3
COEFS = (0.1, 0.1, 2.0)


def _loop_inputs(Mc, p=0.0):
    rs = np.random.RandomState(100 + Mc)
    frames, records = MG.synthetic_rounds(W_, H_, N_, T_, rs, crowd=True, p=p, seed=9)
    cin, hidden = 3 + Mc, 8
    weights = [rs.uniform(-0.5, 0.5, (hidden, cin, 3, 3)), rs.uniform(-0.5, 0.5, (3 + Mc, hidden, 3, 3))]
    mem0 = rs.standard_normal((Mc, N_))
    proj = [rs.standard_normal((3, N_)) for _ in range(T_)], rs.standard_normal((Mc, N_))
    return frames, records, weights, mem0, proj


def _run(Mc, dtype, boundary='circular', p=0.0, keep=False):
    frames, records, weights, mem0, (pa, pm) = _loop_inputs(Mc, p)
    ws = [torch.tensor(w, dtype=dtype, requires_grad=True) for w in weights]
    m0 = torch.tensor(mem0, dtype=dtype, requires_grad=True)
    out = MG.unroll(ws, boundary, 'tanh', frames, records, m0, COEFS)
    if keep:
        for v in out['expanded'] + out['sense'] + out['memories'][1:]:
            v.retain_grad()
    loss = sum((torch.as_tensor(a, dtype=dtype) * act).sum() for a, act in zip(pa, out['actions'])) + \
        (torch.as_tensor(pm, dtype=dtype) * out['memories'][-1]).sum()
    loss.backward()
    grads = [w.grad.double().numpy() for w in ws] + [m0.grad.double().numpy()]
    return out, records, m0, grads


@pytest.mark.parametrize('Mc', [1, 2])
def test_model_adjoints_equal_autograd_of_the_loop(Mc):
    out, records, m0, _ = _run(Mc, torch.float64, keep=True)
    mems = [m0] + out['memories'][1:]
    for t, (cell, win) in enumerate(records):
        want = MG.expand_adjoint(W_, H_, win, out['expanded'][t].grad.numpy())
        assert np.allclose(mems[t].grad.numpy(), want, rtol=0, atol=1e-14 * max(1.0, np.abs(want).max())), t
        want = MG.gather_adjoint(W_, H_, cell, mems[t + 1].grad.numpy())          # (the last memory's gradient is the loss's own term)
        got = out['sense'][t].grad.numpy()[3:]
        assert np.allclose(got, want, rtol=0, atol=1e-14 * max(1.0, np.abs(want).max())), t
        assert np.abs(want).max() > 0


@pytest.mark.parametrize('boundary, p', [('circular', 0.0), ('zeros', 0.0), ('circular', 0.25)])
def test_fp32_error_figure(boundary, p):
    worst = 0.0
    for Mc in (1, 2):
        ref = _run(Mc, torch.float64, boundary, p)[3]
        got = _run(Mc, torch.float32, boundary, p)[3]
        for r, g in zip(ref, got):
            assert np.abs(r).max() > 0
            worst = max(worst, MG.rel_err(g, r))
    print(f'fp32 loop against float64, {boundary}, p={p}: worst max|err| / max|ref| per gradient array = {worst:.3e}')
    assert worst <= FP32_FIGURE, worst


# ---------------------------------------------------------------------------------------------------- the refusals
class NoMedium:
    world = None

    def __getattr__(self, name):
        raise AssertionError(f'the medium was touched ({name}) before the refusal')


class Decomposed(NoMedium):
    world = (128, 128, 0, 0)


class Fp16Medium(NoMedium):
    dtype = torch.float16


class Fp32Medium(NoMedium):
    dtype = torch.float32
    device = torch.device('cpu')


class Agents:
    N = 10
    global_slots = False


def test_recurrent_action_refusals_touch_nothing(lib):
    from die_amd import NeuralAutomataAgent
    kw = dict(kernel_sizes=(3, 3), p_agent_dropout=0.25, dropout_seed=3)
    with pytest.raises(ValueError, match='differentiable_action'):
        NeuralAutomataAgent(**kw).recurrent_action((object(), NoMedium()))
    cases = [
        (dict(memory_channels=2, with_stock_channel=True), NoMedium(), None, NotImplementedError, 'stock'),
        (dict(memory_channels=2), Decomposed(), None, NotImplementedError, 'decomposed'),
        (dict(memory_channels=2), Fp16Medium(), None, NotImplementedError, 'fp32'),
        (dict(memory_channels=2, boundary='reflect'), NoMedium(), None, NotImplementedError, 'reflect'),
        (dict(memory_channels=2, boundary='replicate'), NoMedium(), None, NotImplementedError, 'replicate'),
        (dict(memory_channels=2), Fp32Medium(), torch.zeros((2, 9)), ValueError, 'memory'),                          # another N
        (dict(memory_channels=2), Fp32Medium(), torch.zeros((3, 10)), ValueError, 'memory'),                         # another M
        (dict(memory_channels=2), Fp32Medium(), torch.zeros((2, 10), dtype=torch.float64), ValueError, 'memory'),    # another dtype
        (dict(memory_channels=2), Fp32Medium(), torch.zeros((2, 10), device='meta'), ValueError, 'memory'),          # another device
        (dict(memory_channels=2), Fp32Medium(), np.zeros((2, 10), dtype=np.float32), ValueError, 'memory'),          # no tensor
    ]
    for extra, medium, memory, exc, needle in cases:
        ag = NeuralAutomataAgent(**kw, **extra)
        with pytest.raises(exc, match=needle):
            ag.recurrent_action((Agents(), medium), memory)
        assert ag.dropout_step == 0 and ag.memory is None and ag._sense_output is None, extra
    ag = NeuralAutomataAgent(**kw, memory_channels=2)                # the agent's own memory, bound to another N
    ag.memory, ag._memory_rebind = torch.ones((2, 7)), False
    with pytest.raises(ValueError, match='reset_memory'):
        ag.recurrent_action((Agents(), Fp32Medium()))
    assert ag.dropout_step == 0 and torch.equal(ag.memory, torch.ones((2, 7)))
    # what the issue keeps refused stays refused
    with pytest.raises(NotImplementedError, match='forward_device'):
        ag.model.forward_device(None)
    with pytest.raises(NotImplementedError, match='differentiable_action'):
        ag.differentiable_action((None, NoMedium()))


# ---------------------------------------------------------------------------------------------------- the symbols
def test_new_symbols_declared_and_exported(lib):
    so = C.CDLL(lib.LIB_PATH)
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    header = open(os.path.join(ROOT, 'include', 'die_hip.h')).read()
    assert '#define DIE_ABI_VERSION 24' in header
    for name, n_args in NEW.items():
        assert hasattr(so, name) and name in lib.EXPORTS, name
        assert len(lib._SIGNATURES[name][1]) == n_args and len(getattr(lib.lib, name).argtypes) == n_args, name
        proto = header[header.index(f'int {name}('):]
        proto = proto[:proto.index(';')]
        assert proto.count(',') + 1 == n_args, (name, proto)
    assert 'more than two alive slots' in header                     # the reproducibility sentence, as the issue words it
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build_list', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert 'die_memory_grad.hip' in mod.SOURCES


W, H, N = 20, 68, 300
A, B, D = FAKE, FAKE + (1 << 20), FAKE + (2 << 20)                     # a megabyte apart: nothing overlaps


def _cells(L, *, null=None, null_array=None, W=W, H=H, gW=0, epoch=3, N_=N, standing=A, cell=B, win=D):
    m = L.Medium(W, H, L.DIE_F32, 5, FAKE, FAKE, FAKE, FAKE + 8, gW, gW, 0, 0, 0, 0, 0, 0, None)
    arrays = {k: FAKE + (3 << 20) + 4096 * i for i, k in enumerate(('x', 'y', 'alive'), 1)}
    if null_array:
        arrays[null_array] = None
    a = L.Agents(N_, arrays['x'], arrays['y'], arrays['alive'], None, None)
    args = dict(m=C.byref(m), a=C.byref(a), standing=standing, cell=cell, win=win)
    if null:
        args[null] = None
    return L.lib.die_memory_cells(args['m'], args['a'], args['standing'], epoch, args['cell'], args['win'], None)


def _index(L, name, *, null=None, W=W, H=H, M_=3, n_slots=N, index=A, planes=B, plane_stride=W * H, memory=D, row_stride=N):
    args = dict(index=index, planes=planes, memory=memory)
    if null:
        args[null] = None
    if name == 'die_memory_planes_backward':
        return L.lib.die_memory_planes_backward(W, H, M_, n_slots, args['index'], args['planes'], plane_stride, args['memory'], row_stride, None)
    return L.lib.die_gather_memory_backward(W, H, M_, n_slots, args['index'], args['memory'], row_stride, args['planes'], plane_stride, None)


CELLS_CASES = [
    ('null medium', dict(null='m'), ARG, b'null argument'),
    ('null agents', dict(null='a'), ARG, b'null argument'),
    ('null standing plane', dict(null='standing'), ARG, b'null argument'),
    ('null cell record', dict(null='cell'), ARG, b'null argument'),
    ('null win record', dict(null='win'), ARG, b'null argument'),
    ('null x', dict(null_array='x'), ARG, b'null agent array'),
    ('null alive', dict(null_array='alive'), ARG, b'null agent array'),
    ('empty field', dict(W=0), ARG, b'bad size'),
    ('decomposed medium', dict(gW=128), UNSUPPORTED, b'decomposed'),
    ('2^31 cells', dict(W=1 << 16, H=1 << 15), ARG, b'int32 cell index'),
    ('epoch 0', dict(epoch=0), ARG, b'epoch 0 outside 1..31'),
    ('epoch 32', dict(epoch=32), ARG, b'epoch 32 outside 1..31'),
    ('too many slots', dict(N_=1 << 27), ARG, b'slots'),
    ('negative slots', dict(N_=-1), ARG, b'slots'),
    ('the records are one', dict(win=B), ARG, b'two records overlap'),
    ('win starts in cell', dict(win=B + 4 * (N - 1)), ARG, b'two records overlap'),
    ('cell is the standing plane', dict(cell=A), ARG, b'overlaps the standing plane'),
    ('win starts in the standing plane', dict(win=A + 8 * W * H - 4), ARG, b'overlaps the standing plane'),
    ('cell is the x array', dict(cell=FAKE + (3 << 20) + 4096), ARG, b'overlaps the agent arrays'),
    ('win ends in the alive array', dict(win=FAKE + (3 << 20) + 3 * 4096 - 4 * N + 1), ARG, b'overlaps the agent arrays'),
]
INDEX_CASES = [
    ('null record', dict(null='index'), ARG, b'null argument'),
    ('null planes', dict(null='planes'), ARG, b'null argument'),
    ('null memory', dict(null='memory'), ARG, b'null argument'),
    ('empty field', dict(H=0), ARG, b'bad size'),
    ('no memory channel', dict(M_=0), ARG, b'0 memory channels outside 1..8'),
    ('nine memory channels', dict(M_=9), ARG, b'9 memory channels outside 1..8'),
    ('2^31 cells', dict(W=1 << 16, H=1 << 15, plane_stride=1 << 31), ARG, b'int32 cell index'),
    ('too many slots', dict(n_slots=1 << 27, row_stride=1 << 27), ARG, b'slots'),
    ('negative slots', dict(n_slots=-1), ARG, b'slots'),
    ('row_stride below a row', dict(row_stride=N - 1), ARG, b'row_stride'),
    ('plane_stride below a plane', dict(plane_stride=W * H - 1), ARG, b'plane_stride'),
]
PLANES_BACKWARD = INDEX_CASES + [
    ('the output is the record', dict(memory=A), ARG, b'overlaps the record'),
    ('the output ends in the record', dict(memory=A - 4 * (2 * N + 1)), ARG, b'overlaps the record'),
    ('the output is the planes', dict(memory=B), ARG, b"overlaps the planes' gradient"),
    ('the output starts in the last plane', dict(memory=B + 4 * (3 * W * H - 1)), ARG, b"overlaps the planes' gradient"),
]
GATHER_BACKWARD = INDEX_CASES + [
    ('the output is the record', dict(planes=A), ARG, b'overlaps the record'),
    ('the output starts in the record', dict(planes=A + 4 * (N - 1)), ARG, b'overlaps the record'),
    ('the output is the memory gradient', dict(planes=D), ARG, b'overlaps the memory gradient'),
    ('the output ends in the memory gradient', dict(planes=D - 4 * (2 * W * H + 1)), ARG, b'overlaps the memory gradient'),
]


def _ids(v):
    return v if isinstance(v, str) else None


@pytest.mark.parametrize('case, kw, status, needle', CELLS_CASES, ids=_ids)
def test_memory_cells_refusals(lib, case, kw, status, needle):
    assert _cells(lib, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and b'die_memory_cells:' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


@pytest.mark.parametrize('case, kw, status, needle', PLANES_BACKWARD, ids=_ids)
def test_memory_planes_backward_refusals(lib, case, kw, status, needle):
    assert _index(lib, 'die_memory_planes_backward', **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and b'die_memory_planes_backward:' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


@pytest.mark.parametrize('case, kw, status, needle', GATHER_BACKWARD, ids=_ids)
def test_gather_memory_backward_refusals(lib, case, kw, status, needle):
    assert _index(lib, 'die_gather_memory_backward', **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and b'die_gather_memory_backward:' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())
