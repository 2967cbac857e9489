"""Batched BPTT (BatchedNeuralAutomataAgent.recurrent_action, the batched twins in die_memory_grad.hip and the memory-aware
store / backward pair), CPU side: the batched model (tests/memory_grad_batch_model.py) against its defining identities and against
torch's float64 autograd of the batched loop, the fp32 error figure the GPU ceiling rests on (E = 2 included), the new symbols with
their argument counts under ABI 24, a refusal table per entry point — status and message, returned on the host before any launch
(fake pointers, never dereferenced) — and `recurrent_action`'s refusals on stub objects.  No kernel is launched here."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from tests import memory_grad_batch_model as MB
from tests import memory_grad_model as MG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'die_memory_cells_batch': 8, 'die_memory_planes_backward_batch': 11, 'die_gather_memory_backward_batch': 11,
       'die_nca_wide_sense_batch_store_memory': 10, 'die_nca_wide_backward_batch_memory_workspace_bytes': 5,
       'die_nca_wide_backward_batch_memory': 16}
FAKE = 1 << 20
ARG, UNSUPPORTED = -1, -3
GPU_CEILING = 1e-4                   # tests/test_gpu_memory_grad_batch.py CEILING
FP32_FIGURE = GPU_CEILING / 10       # the fp32 loop's worst max|err| / max|ref| per gradient array must stay below a tenth of it


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
def _words(W, H, N, rs, n):
    """R replicas' coordinate words and alive flags, (R, Nmax): slots on cells of their own but for a triple and a pair."""
    x, y, alive = (np.zeros((len(n), N), dtype=t) for t in (np.uint32, np.uint32, bool))
    for r, k in enumerate(n):
        cells = rs.choice(W * H, N, replace=False)
        cells[1] = cells[2] = cells[0]
        cells[4] = cells[3]
        x[r], y[r] = MG.label_words(cells // H, W), MG.label_words(cells % H, H)
        alive[r] = np.arange(N) % 5 != 2
    return x, y, alive


def test_the_batched_record_is_the_record_per_replica_with_a_padding_of_minus_one():
    W, H, N, n = 9, 7, 14, (14, 9, 0, 5)
    x, y, alive = _words(W, H, N, np.random.RandomState(2), n)
    cell, win = MB.record_batch(W, H, x, y, alive, n)
    assert cell.dtype == win.dtype == np.int32 and cell.shape == win.shape == (4, N)
    for r, k in enumerate(n):
        assert (cell[r, k:] == -1).all() and (win[r, k:] == -1).all()
        if k:
            c, w = MG.record(W, H, x[r, :k], y[r, :k], alive[r, :k])
            assert np.array_equal(cell[r, :k], c) and np.array_equal(win[r, :k], w)
            assert (cell[r, :k][~alive[r, :k]] == -1).all()
    assert (np.bincount(cell[0][cell[0] >= 0]) > 1).sum() == 2 and (win[0] >= 0).sum() == len(np.unique(cell[0][cell[0] >= 0]))


@pytest.mark.parametrize('Mc', [1, 3])
def test_batched_adjoint_identities(Mc):
    W, H, N, n = 9, 7, 14, (14, 9, 0, 5)
    rs = np.random.RandomState(11)
    cell, win = MB.record_batch(W, H, *_words(W, H, N, rs, n), n)
    R = len(n)
    m, p = rs.standard_normal((R, Mc, N)), rs.standard_normal((R, Mc, W, H))
    lhs, rhs = (MB.expand_batch(W, H, win, m) * p).sum(), (m * MB.expand_adjoint_batch(W, H, win, p)).sum()
    assert abs(lhs - rhs) <= 1e-13 * max(1.0, abs(lhs)), (lhs, rhs)
    s, g = rs.standard_normal((R, Mc, W, H)), rs.standard_normal((R, Mc, N))
    lhs, rhs = (MB.gather_batch(W, H, cell, s) * g).sum(), (s * MB.gather_adjoint_batch(W, H, cell, g)).sum()
    assert abs(lhs - rhs) <= 1e-13 * max(1.0, abs(lhs)), (lhs, rhs)
    for r, k in enumerate(n):                                        # the padding gathers 0 and scatters nothing; a replica of no slot: zeros
        assert not MB.expand_adjoint_batch(W, H, win, p)[r, :, k:].any() and not MB.gather_batch(W, H, cell, s)[r, :, k:].any()
    assert not MB.gather_adjoint_batch(W, H, cell, g)[2].any() and not MB.expand_batch(W, H, win, m)[2].any()
    wide = g.copy()
    wide[:, :, :] = g
    for r, k in enumerate(n):
        wide[r, :, k:] = 7.0                                         # whatever stands in the padding changes nothing
    assert np.array_equal(MB.gather_adjoint_batch(W, H, cell, wide), MB.gather_adjoint_batch(W, H, cell, g))


# ---------------------------------------------------------------------------------------------------- the batched loop
W_, H_, T_ = 9, 7, 3
COEFS = (0.1, 0.1, 2.0)


def _loop_inputs(Mc, R, E, n, p=0.0):
    rs = np.random.RandomState(200 + Mc + R)
    frames, records = [], []
    for r in range(R):
        f, rec = MG.synthetic_rounds(W_, H_, n[r], T_, rs, crowd=True, p=p, seed=9 + r)
        frames.append(f)
        records.append(rec)
    cin, hidden = 3 + Mc, 8
    weights = [[rs.uniform(-0.5, 0.5, (hidden, cin, 3, 3)), rs.uniform(-0.5, 0.5, (3 + Mc, hidden, 3, 3))] for _ in range(R // E)]
    mem0 = [rs.standard_normal((Mc, n[r])) for r in range(R)]
    proj = [[rs.standard_normal((3, n[r])) for _ in range(T_)] for r in range(R)], [rs.standard_normal((Mc, n[r])) for r in range(R)]
    return frames, records, weights, mem0, proj


def _run(Mc, dtype, R=3, E=1, n=(14, 9, 11, 14), boundary='circular', p=0.0, keep=False):
    frames, records, weights, mem0, (pa, pm) = _loop_inputs(Mc, R, E, n, p)
    ws = [[torch.tensor(w, dtype=dtype, requires_grad=True) for w in row] for row in weights]
    m0 = [torch.tensor(m, dtype=dtype, requires_grad=True) for m in mem0]
    outs = MB.unroll_batch(ws, boundary, 'tanh', frames, records, m0, COEFS, E)
    if keep:
        for out in outs:
            for v in out['expanded'] + out['sense'] + out['memories'][1:]:
                v.retain_grad()
    loss = 0.
    for r, out in enumerate(outs):
        loss = loss + sum((torch.as_tensor(a, dtype=dtype) * act).sum() for a, act in zip(pa[r], out['actions'])) + \
            (torch.as_tensor(pm[r], dtype=dtype) * out['memories'][-1]).sum()
    loss.backward()
    rows = [np.concatenate([w.grad.double().numpy().ravel() for w in row]) for row in ws]
    return outs, records, m0, rows, [m.grad.double().numpy() for m in m0], (frames, weights, mem0, pa, pm)


@pytest.mark.parametrize('Mc', [1, 2])
def test_batched_model_adjoints_equal_autograd_of_the_loop(Mc):
    R, n = 3, (14, 9, 11)
    outs, records, m0, _, _, _ = _run(Mc, torch.float64, R, 1, n, keep=True)
    Nmax = max(n)
    for t in range(T_):
        cell = np.stack([np.pad(records[r][t][0], (0, Nmax - n[r]), constant_values=-1) for r in range(R)])
        win = np.stack([np.pad(records[r][t][1], (0, Nmax - n[r]), constant_values=-1) for r in range(R)])
        mems = [([m0[r]] + outs[r]['memories'][1:]) for r in range(R)]
        gp = np.stack([outs[r]['expanded'][t].grad.numpy() for r in range(R)])
        want = MB.expand_adjoint_batch(W_, H_, win, gp)
        gm_next = MB.pad_rows([mems[r][t + 1].grad.numpy() for r in range(R)], Nmax)
        want_planes = MB.gather_adjoint_batch(W_, H_, cell, gm_next)
        for r in range(R):
            got = mems[r][t].grad.numpy()
            assert np.allclose(got, want[r, :, :n[r]], rtol=0, atol=1e-14 * max(1.0, np.abs(got).max())), (t, r)
            assert not want[r, :, n[r]:].any()
            got = outs[r]['sense'][t].grad.numpy()[3:]
            assert np.abs(got).max() > 0 and np.allclose(got, want_planes[r], rtol=0, atol=1e-14 * max(1.0, np.abs(got).max())), (t, r)


def test_episode_rows_are_the_float64_sums_over_a_candidates_worlds():
    """E = 2: row c of the batched loop is the sum of the gradients of candidate c's two worlds run alone."""
    Mc, R, E, n = 2, 4, 2, (14, 9, 11, 14)
    _, records, _, rows, gm, (frames, weights, mem0, pa, pm) = _run(Mc, torch.float64, R, E, n)
    assert len(rows) == 2
    for c in range(2):
        total = 0.
        for r in (2 * c, 2 * c + 1):
            ws = [torch.tensor(w, requires_grad=True) for w in weights[c]]
            m = torch.tensor(mem0[r], requires_grad=True)
            out = MG.unroll(ws, 'circular', 'tanh', frames[r], records[r], m, COEFS)
            (sum((torch.as_tensor(a) * act).sum() for a, act in zip(pa[r], out['actions'])) + (torch.as_tensor(pm[r]) * out['memories'][-1]).sum()).backward()
            total = total + np.concatenate([w.grad.numpy().ravel() for w in ws])
            assert np.allclose(m.grad.numpy(), gm[r], rtol=0, atol=1e-13 * np.abs(gm[r]).max())
        assert np.abs(total).max() > 0 and np.abs(rows[c] - total).max() <= 1e-13 * np.abs(total).max()


@pytest.mark.parametrize('R, E, boundary, p', [(3, 1, 'circular', 0.0), (3, 1, 'zeros', 0.0), (4, 2, 'circular', 0.0), (4, 2, 'circular', 0.25)])
def test_fp32_error_figure_of_the_batched_loop(R, E, boundary, p):
    worst = 0.0
    for Mc in (1, 2):
        _, _, _, ref_rows, ref_m, _ = _run(Mc, torch.float64, R, E, boundary=boundary, p=p)
        _, _, _, got_rows, got_m, _ = _run(Mc, torch.float32, R, E, boundary=boundary, p=p)
        for r, g in zip(ref_rows + ref_m, got_rows + got_m):
            assert np.abs(r).max() > 0
            worst = max(worst, MG.rel_err(g, r))
    print(f'fp32 batched loop against float64, R={R} E={E} {boundary} p={p}: worst max|err| / max|ref| per gradient array = {worst:.3e} '
          f'(must stay <= {FP32_FIGURE:.0e}, a tenth of the GPU ceiling {GPU_CEILING:.0e})')
    assert worst <= FP32_FIGURE, worst


# ---------------------------------------------------------------------------------------------------- the symbols
def test_new_symbols_declared_exported_and_bound(lib):
    so = C.CDLL(lib.LIB_PATH)
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    header = open(os.path.join(ROOT, 'include', 'die_hip.h')).read()
    assert '#define DIE_ABI_VERSION 24' in header
    for name, n_args in NEW.items():
        assert hasattr(so, name) and name in lib.EXPORTS, name
        assert len(lib._SIGNATURES[name][1]) == n_args and len(getattr(lib.lib, name).argtypes) == n_args, name
        kind = 'int64_t' if name.endswith('_bytes') else 'int'
        proto = header[header.index(f'{kind} {name}('):]
        proto = proto[:proto.index(';')]
        assert proto.count(',') + 1 == n_args, (name, proto)


def test_python_surface_needs_no_device(lib):
    import inspect
    from die_amd import functional
    from die_amd.batch import BatchedNeuralAutomataAgent
    sig = inspect.signature(BatchedNeuralAutomataAgent.recurrent_action).parameters
    assert list(sig) == ['self', 'memory', 'parameters'] and sig['memory'].default is None and sig['parameters'].default is None
    for name in ('memory_record_batch', 'memory_planes_batch', 'gather_memory_batch', 'BatchedMemoryRecord'):
        assert hasattr(functional, name), name
    with pytest.raises(TypeError):
        functional.memory_record_batch(object())
    with pytest.raises(TypeError):
        functional.memory_planes_batch(torch.zeros((2, 1, 4)), object())
    with pytest.raises(TypeError):
        functional.gather_memory_batch(torch.zeros((2, 1, 4, 4)), object())


# ---------------------------------------------------------------------------------------------------- the refusal tables
W, H, N, R = 20, 68, 300, 3
A, B, D = FAKE, FAKE + (4 << 20), FAKE + (8 << 20)                     # four megabytes apart: nothing overlaps


def _batch(L, *, replicas=R, plane_stride=W * H, agent_stride=N, n=None):
    n = [N, N - 7, 0] + [0] * 61 if n is None else n
    return L.Batch(replicas, 0, plane_stride, agent_stride, 1, (C.c_int64 * 64)(*n))


def _cells(L, *, null=None, null_array=None, slot=None, W=W, H=H, gW=0, epoch=3, standing=A, cell=B, win=D, **bkw):
    m = L.Medium(W, H, L.DIE_F32, 5, FAKE, FAKE, FAKE, FAKE + 8, gW, gW, 0, 0, 0, 0, 0, 0, None)
    arrays = {k: FAKE + (12 << 20) + (1 << 16) * i for i, k in enumerate(('x', 'y', 'alive'), 1)}
    if null_array:
        arrays[null_array] = None
    a = L.Agents(N, arrays['x'], arrays['y'], arrays['alive'], None, slot)
    args = dict(m=C.byref(m), a=C.byref(a), b=C.byref(_batch(L, **bkw)), standing=standing, cell=cell, win=win)
    if null:
        args[null] = None
    return L.lib.die_memory_cells_batch(args['m'], args['a'], args['b'], args['standing'], epoch, args['cell'], args['win'], None)


def _index(L, name, *, null=None, W=W, H=H, M_=3, index=A, planes=B, plane_stride=W * H, replica_stride=3 * W * H, memory=D, row_stride=N, **bkw):
    args = dict(b=C.byref(_batch(L, **bkw)), index=index, planes=planes, memory=memory)
    if null:
        args[null] = None
    if name == 'die_memory_planes_backward_batch':
        return L.lib.die_memory_planes_backward_batch(W, H, M_, args['b'], args['index'], args['planes'], plane_stride, replica_stride,
                                                      args['memory'], row_stride, None)
    return L.lib.die_gather_memory_backward_batch(W, H, M_, args['b'], args['index'], args['memory'], row_stride, args['planes'], plane_stride,
                                                  replica_stride, None)


BATCH_CASES = [
    ('no replica', dict(replicas=0), ARG, b'replicas'),
    ('65 replicas', dict(replicas=65), ARG, b'replicas'),
    ('no slot a replica', dict(agent_stride=0), ARG, b'agent_stride'),
    ('too many slots', dict(agent_stride=1 << 27), ARG, b'agent_stride'),
    ('a replica with more agents than slots', dict(n=[N, N + 1, 0] + [0] * 61), ARG, b'replica 1 has'),
    ('a replica with fewer than no agent', dict(n=[N, N, -1] + [0] * 61), ARG, b'replica 2 has'),
]
CELLS_CASES = [
    ('null medium', dict(null='m'), ARG, b'null argument'),
    ('null agents', dict(null='a'), ARG, b'null argument'),
    ('null batch', dict(null='b'), ARG, b'null argument'),
    ('null standing planes', dict(null='standing'), ARG, b'null argument'),
    ('null cell record', dict(null='cell'), ARG, b'null argument'),
    ('null win record', dict(null='win'), ARG, b'null argument'),
    ('empty field', dict(W=0), ARG, b'bad size'),
    ('decomposed medium', dict(gW=128), UNSUPPORTED, b'decomposed'),
    ('2^31 cells', dict(W=1 << 16, H=1 << 15, plane_stride=1 << 31), ARG, b'int32 cell index'),
    ('epoch 0', dict(epoch=0), ARG, b'epoch 0 outside 1..31'),
    ('epoch 32', dict(epoch=32), ARG, b'epoch 32 outside 1..31'),
] + BATCH_CASES + [
    ('planes overlap', dict(plane_stride=W * H - 1), ARG, b'plane_stride'),
    ('null y', dict(null_array='y'), ARG, b'null agent array'),
    ('a slot array', dict(slot=FAKE), ARG, b'slot order'),
    ('the records are one', dict(win=B), ARG, b'two records overlap'),
    ('win starts in the last row of cell', dict(win=B + 4 * (R * N - 1)), ARG, b'two records overlap'),
    ('cell is the standing planes', dict(cell=A), ARG, b'overlaps the standing planes'),
    ('win starts in the last standing plane', dict(win=A + 8 * (R * W * H) - 4), ARG, b'overlaps the standing planes'),
    ('cell is the x array', dict(cell=FAKE + (12 << 20) + (1 << 16)), ARG, b'overlaps the agent arrays'),
]
INDEX_CASES = [
    ('null batch', dict(null='b'), ARG, b'null argument'),
    ('null record', dict(null='index'), ARG, b'null argument'),
    ('null planes', dict(null='planes'), ARG, b'null argument'),
    ('null memory', dict(null='memory'), ARG, b'null argument'),
    ('empty field', dict(H=0), ARG, b'bad size'),
    ('no memory channel', dict(M_=0), ARG, b'0 memory channels outside 1..8'),
    ('nine memory channels', dict(M_=9), ARG, b'9 memory channels outside 1..8'),
    ('2^31 cells', dict(W=1 << 16, H=1 << 15, plane_stride=1 << 31, replica_stride=1 << 33), ARG, b'int32 cell index'),
] + BATCH_CASES + [
    ('row_stride below a row', dict(row_stride=N - 1), ARG, b'row_stride'),
    ('plane_stride below a plane', dict(plane_stride=W * H - 1), ARG, b'plane_stride'),
    ('replica_stride below a plane', dict(replica_stride=W * H - 1), ARG, b'would share words'),
    ('replica_stride below a replica\'s planes', dict(replica_stride=3 * W * H - 1), ARG, b'would share words'),
    ('plane-major planes that interleave', dict(replica_stride=W * H, plane_stride=R * W * H - 1), ARG, b'would share words'),
]
PLANES_BACKWARD = INDEX_CASES + [
    ('the output is the record', dict(memory=A), ARG, b'overlaps the record'),
    ('the output ends in the record', dict(memory=A - 4 * ((R * 3 - 1) * N + 1)), ARG, b'overlaps the record'),
    ('the output is the planes', dict(memory=B), ARG, b"overlaps the planes' gradient"),
    ('the output starts in the last plane', dict(memory=B + 4 * (R * 3 * W * H - 1)), ARG, b"overlaps the planes' gradient"),
]
GATHER_BACKWARD = INDEX_CASES + [
    ('the output is the record', dict(planes=A), ARG, b'overlaps the record'),
    ('the output starts in the last row of the record', dict(planes=A + 4 * (R * N - 1)), ARG, b'overlaps the record'),
    ('the output is the memory gradient', dict(planes=D), ARG, b'overlaps the memory gradient'),
    ('the output ends in the memory gradient', dict(planes=D - 4 * (R * 3 * W * H - 1)), ARG, b'overlaps the memory gradient'),
]


def _refused(lib, rc, status, needle, who, case):
    err = lib.lib.die_last_error()
    assert rc == status, (case, err)
    assert needle in err and who in err, (case, err)


@pytest.mark.parametrize('case, kw, status, needle', CELLS_CASES, ids=[c[0] for c in CELLS_CASES])
def test_memory_cells_batch_refusals(lib, case, kw, status, needle):
    _refused(lib, _cells(lib, **kw), status, needle, b'die_memory_cells_batch:', case)


@pytest.mark.parametrize('case, kw, status, needle', PLANES_BACKWARD, ids=[c[0] for c in PLANES_BACKWARD])
def test_memory_planes_backward_batch_refusals(lib, case, kw, status, needle):
    _refused(lib, _index(lib, 'die_memory_planes_backward_batch', **kw), status, needle, b'die_memory_planes_backward_batch:', case)


@pytest.mark.parametrize('case, kw, status, needle', GATHER_BACKWARD, ids=[c[0] for c in GATHER_BACKWARD])
def test_gather_memory_backward_batch_refusals(lib, case, kw, status, needle):
    _refused(lib, _index(lib, 'die_gather_memory_backward_batch', **kw), status, needle, b'die_gather_memory_backward_batch:', case)


def test_plane_major_strides_pass_the_checks_up_to_the_overlap_check(lib):
    """die_memory_planes_batch's layout, plane j of replica r at (j * R + r) * W * H, is taken: the call gets as far as the overlap
    check it is given to fail."""
    rc = _index(lib, 'die_memory_planes_backward_batch', replica_stride=W * H, plane_stride=R * W * H, memory=B)
    _refused(lib, rc, ARG, b"overlaps the planes' gradient", b'die_memory_planes_backward_batch:', 'plane-major')


# ---- the memory-aware store / backward pair ----
WS, HS, RS, MS = 24, 72, 4, 2
TANH = 1
STACK = ((3, 3 + MS, 8, TANH), (3, 8, 3 + MS, TANH))                 # (k, cin, cout, activation): ([agents,] food, chem, 2 memory planes)
P_ROW = (3 + MS) * 8 * 9 * 2
MEM = FAKE + (300 << 16)             # memory planes clear of everything else
GIN = FAKE + (400 << 16)


def _structs(L, *, layers=STACK, replicas=RS, episodes=0, pad=0, plane_stride=None, epoch=1, weights=FAKE, dtype=None, agents_channel=1):
    m = L.Medium(WS, HS, L.DIE_F32 if dtype is None else dtype, 1, FAKE, FAKE + (1 << 16), FAKE + (2 << 16), None, 0, 0, 0, 0, 0, 0, 0, 0, None)
    arr = (L.NcaLayer * len(layers))(*[L.NcaLayer(k, cin, cout, act, weights, cout * cin * k * k) for k, cin, cout, act in layers])
    nca = L.NcaBatch(len(layers), pad, agents_channel, epoch, arr, (C.c_float * 3)(0.01, 0.01, 2.0), episodes, None, 0)
    b = L.Batch(replicas, 0, WS * HS if plane_stride is None else plane_stride, 10, 1, (C.c_int64 * 64)(*([10] * 64)))
    return m, arr, nca, b


def _sense(L, *, null=None, store_bytes=None, drop=None, masked=None, mem=MEM, M_=MS, **kw):
    m, arr, nca, b = _structs(L, **kw)
    need = L.lib.die_nca_wide_sense_batch_store_bytes(WS, HS, RS, 2, 8)
    a = dict(m=C.byref(m), b=C.byref(b), nca=C.byref(nca), store=FAKE + (3 << 16), mem=mem)
    if null:
        a[null] = None
    return L.lib.die_nca_wide_sense_batch_store_memory(a['m'], a['b'], a['nca'], a['store'], need if store_bytes is None else store_bytes, masked,
                                                       None if drop is None else C.byref(L.NcaDropout(*drop)), a['mem'], M_, None)


def _need(L):
    return L.lib.die_nca_wide_backward_batch_memory_workspace_bytes(WS, HS, RS, C.byref(_structs(L)[2]), MS)


def _backward(L, *, null=None, workspace_bytes=None, sense_stride=(3 + MS) * WS * HS, grad_stride=P_ROW, drop=None, grad=None, grad_in=None,
              grad_in_stride=(3 + MS) * WS * HS, mem=MEM, M_=MS, **kw):
    m, arr, nca, b = _structs(L, **kw)
    need = _need(L)
    assert need > 0
    a = dict(m=C.byref(m), b=C.byref(b), nca=C.byref(nca), store=FAKE + (3 << 16), g=FAKE + (40 << 16), grad=FAKE + (50 << 16) if grad is None else grad,
             ws=FAKE + (60 << 16), mem=mem)
    if null:
        a[null] = None
    return L.lib.die_nca_wide_backward_batch_memory(a['m'], a['b'], a['nca'], a['store'], a['g'], sense_stride, a['grad'], grad_stride,
                                                    None if drop is None else C.byref(L.NcaDropout(*drop)), a['ws'],
                                                    need if workspace_bytes is None else workspace_bytes, grad_in, grad_in_stride, a['mem'], M_, None)


PLAIN = ((3, 3, 8, TANH), (3, 8, 3, TANH))                           # a stack without memory
STACK_REFUSALS = [
    ('null medium', dict(null='m'), ARG, b'null argument'),
    ('null batch', dict(null='b'), ARG, b'null argument'),
    ('null stack', dict(null='nca'), ARG, b'null argument'),
    ('null store', dict(null='store'), ARG, b'null argument'),
    ('null memory planes', dict(null='mem'), ARG, b'null argument'),
    ('no memory channel', dict(M_=0), ARG, b'0 memory channels outside 1..8'),
    ('nine memory channels', dict(M_=9), ARG, b'9 memory channels outside 1..8'),
    ('no replica', dict(replicas=0), ARG, b'replicas'),
    ('65 replicas', dict(replicas=65), ARG, b'replicas'),
    ('planes overlap', dict(plane_stride=WS * HS - 1), ARG, b'plane_stride'),
    ('episodes do not divide the replicas', dict(episodes=3), ARG, b'episodes'),
    ('kernel size 7', dict(layers=((7, 5, 8, TANH), (3, 8, 5, TANH))), ARG, b'kernel size 7'),
    ('33 channels', dict(layers=((3, 5, 33, TANH), (3, 33, 5, TANH))), ARG, b'channels'),
    ('a stack without memory', dict(layers=PLAIN), ARG, b'input has 5'),
    ('another M than the stack\'s', dict(M_=3), ARG, b'input has 6'),
    ('the last layer gives 3 planes', dict(layers=((3, 5, 8, TANH), (3, 8, 3, TANH))), ARG, b'last layer gives 3 planes'),
    ('no agents channel, the same stack', dict(agents_channel=0), ARG, b'input has 4'),
    ('last layer not tanh', dict(layers=((3, 5, 8, TANH), (3, 8, 5, 2))), ARG, b'activation'),
    ('sense_epoch 0', dict(epoch=0), ARG, b'sense_epoch'),
    ('bad field dtype', dict(dtype=7), ARG, b'dtype'),
]
SENSE_REFUSALS = STACK_REFUSALS + [
    ('store too small', dict(store_bytes=1024), ARG, b'store too small'),
    ('mask without planes for the masked values', dict(drop=(0.25, 7, 1, 0, 0)), ARG, b'masked'),
    ('p out of range', dict(drop=(1.5, 7, 1, 0, 0), masked=FAKE + (90 << 16)), ARG, b'dropout p'),
    ('the memory planes are the store', dict(mem=FAKE + (3 << 16)), ARG, b'memory planes overlap'),
    ('the memory planes end in the store', dict(mem=FAKE + (3 << 16) - 4 * (MS * RS * WS * HS - 1)), ARG, b'memory planes overlap'),
]
BACKWARD_REFUSALS = STACK_REFUSALS + [
    ('null gradient planes', dict(null='g'), ARG, b'null argument'),
    ('null grad', dict(null='grad'), ARG, b'null argument'),
    ('null workspace', dict(null='ws'), ARG, b'null argument'),
    ('reflect', dict(pad=2), UNSUPPORTED, b'reflect'),
    ('gradient planes of three planes a replica', dict(sense_stride=3 * WS * HS), ARG, b'sense_stride'),
    ('gradient planes overlap', dict(sense_stride=(3 + MS) * WS * HS - 1), ARG, b'below 5 planes'),
    ('gradient rows overlap', dict(grad_stride=P_ROW - 1), ARG, b'grad_stride'),
    ('grad is the weights', dict(grad=FAKE), ARG, b'weights'),
    ('workspace one byte short', dict(workspace_bytes=-1), ARG, b'workspace too small'),
    ('dropout reserved word', dict(drop=(0.25, 7, 1, 0, 1)), ARG, b'reserved'),
    ('grad_in of three planes a replica', dict(grad_in=GIN, grad_in_stride=3 * WS * HS), ARG, b'grad_in_stride'),
    ('grad_in not aligned', dict(grad_in=GIN + 4), ARG, b'16-byte aligned'),
    ('grad_in stride not a multiple of 4', dict(grad_in=GIN, grad_in_stride=(3 + MS) * WS * HS + 2), ARG, b'multiple of 4'),
    ('grad_in is the store', dict(grad_in=FAKE + (3 << 16)), ARG, b'aliases'),
    ('grad_in is the chem plane', dict(grad_in=FAKE + (2 << 16)), ARG, b'aliases'),
    ('grad_in is the memory planes', dict(grad_in=MEM), ARG, b'aliases'),
    ('grad_in starts in the last memory plane', dict(grad_in=MEM + 4 * (MS * RS * WS * HS - 4)), ARG, b'aliases'),
]

@pytest.mark.parametrize('case, kw, status, needle', SENSE_REFUSALS, ids=[c[0] for c in SENSE_REFUSALS])
def test_sense_store_memory_refused_before_launch(lib, case, kw, status, needle):
    _refused(lib, _sense(lib, **kw), status, needle, b'die_nca_wide_sense_batch_store_memory:', case)


@pytest.mark.parametrize('case, kw, status, needle', BACKWARD_REFUSALS, ids=[c[0] for c in BACKWARD_REFUSALS])
def test_backward_memory_refused_before_launch(lib, case, kw, status, needle):
    if kw.get('workspace_bytes') == -1:
        kw = dict(kw, workspace_bytes=_need(lib) - 1)
    _refused(lib, _backward(lib, **kw), status, needle, b'die_nca_wide_backward_batch_memory:', case)


def test_byte_queries(lib):
    """The memory query is the parent's formula with the stack's own channel counts; each query gives -1 for the other's stack,
    and the parent call keeps refusing a 3 + M stack."""
    good = _structs(lib)[2]
    tiles = -(-WS // 16) * -(-HS // 64)
    want = 4 * (RS * tiles * max(co * ci * k * k for k, ci, co, _ in STACK) + 1 * RS * 8 * WS * HS)
    assert _need(lib) == want
    q = lib.lib.die_nca_wide_backward_batch_memory_workspace_bytes
    assert lib.lib.die_nca_wide_backward_batch_workspace_bytes(WS, HS, RS, C.byref(good)) == -1
    plain = _structs(lib, layers=PLAIN)[2]
    assert q(WS, HS, RS, C.byref(plain), MS) == -1 and lib.lib.die_nca_wide_backward_batch_workspace_bytes(WS, HS, RS, C.byref(plain)) > 0
    for bad in (dict(M=0), dict(M=9), dict(M=3), dict(Wq=0), dict(R_=0), dict(R_=65), dict(null=True)):
        assert q(bad.get('Wq', WS), HS, bad.get('R_', RS), None if bad.get('null') else C.byref(good), bad.get('M', MS)) == -1, bad
    for pad in (2, 3):
        assert q(WS, HS, RS, C.byref(_structs(lib, pad=pad)[2]), MS) == -1
    m, arr, nca, b = _structs(lib)
    rc = lib.lib.die_nca_wide_backward_batch(C.byref(m), C.byref(b), C.byref(nca), FAKE + (3 << 16), FAKE + (40 << 16), 5 * WS * HS, FAKE + (50 << 16),
                                             P_ROW, None, FAKE + (60 << 16), want, None, 0, None)
    _refused(lib, rc, ARG, b'input has 3', b'die_nca_wide_backward_batch:', 'the parent on a memory stack')


# ---------------------------------------------------------------------------------------------------- recurrent_action's refusals
def _stub(memory_channels=2, stock=False, per_replica=False, dtype=torch.float32, boundary='circular', p=0.0, training=True, dropout_seed=3):
    """A BatchedNeuralAutomataAgent that never saw a device: what `recurrent_action` reads before its first launch."""
    from die_amd.batch import BatchedNeuralAutomataAgent

    class Env:
        R, Nmax, W, H = 3, 10, 16, 12
        device = torch.device('cpu')

        def __getattr__(self, name):
            raise AssertionError(f'the worlds were touched ({name}) before the refusal')

    env = Env()
    env.per_replica, env.dtype = per_replica, dtype
    pop = BatchedNeuralAutomataAgent.__new__(BatchedNeuralAutomataAgent)
    pop.env, pop.R, pop.candidates, pop.episodes, pop.P = env, 3, 3, 1, 5
    pop._memory_channels, pop._stock_channel, pop._arch = memory_channels, stock, dict(boundary=(boundary,))
    pop.template = types.SimpleNamespace(model=types.SimpleNamespace(agent_dropout=types.SimpleNamespace(p=p), training=training))
    pop.dropout_seed, pop.dropout_seed_stride, pop.dropout_step = dropout_seed, 1, 4
    pop.parameters = torch.zeros((3, 5))
    pop.memory = torch.full((3, 2, 10), 0.5) if memory_channels else None
    return pop


def test_recurrent_action_refusals_touch_nothing(lib):
    cases = [
        (dict(memory_channels=0), None, ValueError, 'without memory'),
        (dict(stock=True), None, NotImplementedError, 'stock'),
        (dict(per_replica=True), None, NotImplementedError, 'per_replica'),
        (dict(dtype=torch.float16), None, NotImplementedError, 'fp32'),
        (dict(boundary='reflect'), None, NotImplementedError, 'reflect'),
        (dict(boundary='replicate'), None, NotImplementedError, 'replicate'),
        (dict(p=0.25, dropout_seed=None), None, NotImplementedError, 'dropout_seed'),
        ({}, torch.zeros((3, 2, 9)), ValueError, 'memory must be'),                            # another Nmax
        ({}, torch.zeros((3, 3, 10)), ValueError, 'memory must be'),                           # another M
        ({}, torch.zeros((2, 2, 10)), ValueError, 'memory must be'),                           # another R
        ({}, torch.zeros((3, 2, 10), dtype=torch.float64), ValueError, 'memory must be'),      # another dtype
        ({}, torch.zeros((3, 2, 10), device='meta'), ValueError, 'memory must be'),            # another device
        ({}, np.zeros((3, 2, 10), dtype=np.float32), ValueError, 'memory must be'),            # no tensor
    ]
    for kw, memory, exc, needle in cases:
        pop = _stub(**kw)
        held = pop.memory
        with pytest.raises(exc, match=needle) as info:
            pop.recurrent_action(memory)
        assert 'recurrent_action' in str(info.value) or needle == 'dropout_seed', kw
        assert pop.dropout_step == 4 and pop.memory is held and (held is None or bool((held == 0.5).all())), kw
    pop = _stub()                                                    # a parameter matrix of the wrong shape
    with pytest.raises(ValueError, match='parameters'):
        pop.recurrent_action(None, torch.zeros((3, 4)))
    assert pop.dropout_step == 4 and bool((pop.memory == 0.5).all())
    # what the issue keeps refused stays refused (the template's own refusal, reached before anything else)
    from die_amd import NeuralAutomataAgent
    pop = _stub()
    pop.template = NeuralAutomataAgent(kernel_sizes=(3, 3), hidden_channels=4, hidden_activation='tanh', memory_channels=2)
    for call in (pop.differentiable_sense, pop.differentiable_action, pop.forward_device):
        with pytest.raises(NotImplementedError, match='no gradients through memory channels'):
            call()
    assert pop.dropout_step == 4 and bool((pop.memory == 0.5).all())
