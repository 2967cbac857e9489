"""Gradients through signal channels (NeuralAutomataAgent.signalling_action, die_signal_grad.hip), CPU side: the float64 adjoint of
tests/signal_model.py `update` against its defining identity, the float64 loop's autograd against central differences, the fp32
emulation of the backward kernel inside the bound the GPU test allows — over that test's whole grid —, and the two new symbols with
their host-side argument checks (fake pointers: a launch would have failed).  No kernel is launched here."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import memory_grad_model as MG
from tests import signal_grad_model as SG
from tests import signal_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'die_signal_cells': 5, 'die_signal_step_backward': 13}
FAKE = 1 << 20
ARG, UNSUPPORTED = -1, -3
GRID = [(W, H, sigma, K) for W, H in SM.SHAPES for sigma in SM.SIGMAS for K in SM.CHANNELS]


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------- the adjoint
@pytest.mark.parametrize('W,H,sigma,K', GRID)
def test_adjoint_identity(W, H, sigma, K):
    """<update(F, S), g> = <F, gF> + <S, gS> in float64, to 1e-12 of the sum of the terms' magnitudes."""
    F, occ, planes = SM.case(W, H, K)
    g = SG.grad_case(W, H, K).astype(np.float64)
    gF, gS = SG.adjoint(g, occ, SM.DEPOSIT, sigma, SM.DECAY)
    terms = [SM.update(F, occ, planes, SM.DEPOSIT, sigma, SM.DECAY) * g, F.astype(np.float64) * gF, planes.astype(np.float64) * gS]
    lhs, rhs = terms[0].sum(), terms[1].sum() + terms[2].sum()
    assert abs(lhs - rhs) <= 1e-12 * sum(np.abs(t).sum() for t in terms), (lhs, rhs)
    assert occ.any() and np.abs(terms[2]).sum() > 0 and not gS[:, ~occ].any()       # the emission term is there, and only where somebody stands


@pytest.mark.parametrize('W,H,sigma,K', GRID)
def test_fp32_emulation_stays_inside_the_gpu_bound(W, H, sigma, K):
    """The reference alone — the backward in fp32 in the kernels' order — lies within tests/signal_model.py `bound` (F := g, nobody
    standing) of the float64 adjoint; the emission gradient adds one fp32 rounding of a product of magnitude |deposit| * |gF|."""
    _, occ, _ = SM.case(W, H, K)
    g = SG.grad_case(W, H, K)
    gF, gS = SG.adjoint(g, occ, SM.DEPOSIT, sigma, SM.DECAY)
    eF, eS = SG.emulate_backward(g, occ, SM.DEPOSIT, sigma, SM.DECAY)
    assert eF.dtype == eS.dtype == np.float32
    bound = SG.bound(g, sigma, SM.DECAY)
    assert (np.abs(eF.astype(np.float64) - gF) <= bound).all(), (np.abs(eF - gF) / bound).max()
    assert (np.abs(eS.astype(np.float64) - gS) <= SM.DEPOSIT * bound + 2.0 ** -24 * np.abs(gS)).all()
    assert not eS[:, ~occ].view(np.uint32).any()                                   # +0.0 where nobody stands, as bits


# ---------------------------------------------------------------------------------------------------- the loop
W_, H_, N_, T_ = 9, 7, 14, 3
COEFS = (0.1, 0.1, 2.0)
CONSTANTS = (0.75, 0.8, 0.05)


def _loop(K, Mc, dtype=torch.float64, shift=None, detach_at=()):
    rs = np.random.RandomState(300 + 10 * K + Mc)
    frames, records = MG.synthetic_rounds(W_, H_, N_, T_, rs, crowd=True)
    occs = [f['occ'] > 0 for f in frames]
    cin, hidden, cout = 3 + K + Mc, 8, 3 + K + Mc
    params = [rs.uniform(-0.5, 0.5, (hidden, cin, 3, 3)), rs.uniform(-0.5, 0.5, (cout, hidden, 3, 3)), rs.standard_normal((K, W_, H_))]
    if Mc:
        params.append(rs.standard_normal((Mc, N_)))
    proj_a, proj_s = [rs.standard_normal((3, N_)) for _ in range(T_)], rs.standard_normal((K, W_, H_))
    if shift is not None:
        params = [p + e for p, e in zip(params, shift)]
    ts = [torch.tensor(p, dtype=dtype, requires_grad=True) for p in params]
    out = SG.unroll(ts[:2], 'circular', 'tanh', frames, occs, ts[2], CONSTANTS, COEFS, records if Mc else None, ts[3] if Mc else None,
                    detach_at=detach_at)
    loss = sum((torch.as_tensor(a, dtype=dtype) * act).sum() for a, act in zip(proj_a, out['actions'])) + \
        (torch.as_tensor(proj_s, dtype=dtype) * out['signals'][-1]).sum()
    return loss, ts, [p.shape for p in params], out


@pytest.mark.parametrize('K,Mc', [(1, 0), (2, 0), (2, 1)])
def test_central_differences_of_the_float64_loop_against_its_autograd(K, Mc):
    """Along three random directions of all the parameters (both layers, the incoming field, the incoming memory):
    (L(p + e d) - L(p - e d)) / 2e against <grad, d>.  With e = 1e-5 the truncation term e^2 L''' / 6 and the rounding term
    2^-53 |L| / e are both below 1e-9 of a loss of order 1..10; the assertion allows 1e-7 of sum |grad_i d_i|."""
    loss, ts, shapes, _ = _loop(K, Mc)
    loss.backward()
    grads = [t.grad.numpy() for t in ts]
    assert all(np.abs(g).max() > 0 for g in grads)
    rs = np.random.RandomState(K + Mc)
    eps = 1e-5
    for _ in range(3):
        d = [rs.standard_normal(s) for s in shapes]
        up = float(_loop(K, Mc, shift=[eps * v for v in d])[0].detach())
        down = float(_loop(K, Mc, shift=[-eps * v for v in d])[0].detach())
        want = sum((g * v).sum() for g, v in zip(grads, d))
        scale = sum(np.abs(g * v).sum() for g, v in zip(grads, d))
        assert abs((up - down) / (2 * eps) - want) <= 1e-7 * scale, ((up - down) / (2 * eps), want)


def test_a_detached_field_cuts_the_emission_rows_off_a_loss_on_the_last_action():
    K = 2
    rs = np.random.RandomState(5)
    for detach_at, reached in (((), True), (range(1, T_), False)):
        _, ts, _, out = _loop(K, 0, detach_at=detach_at)
        (torch.as_tensor(rs.standard_normal((3, N_))) * out['actions'][-1]).sum().backward()
        rows = ts[1].grad.numpy()[3:3 + K]
        assert bool(np.abs(rows).max() > 0) == reached and np.abs(ts[1].grad.numpy()[:3]).max() > 0


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
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build_list', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert 'die_signal_grad.hip' in mod.SOURCES
    from die_amd import NeuralAutomataAgent, functional
    assert all(hasattr(functional, n) for n in ('SignalRecord', 'signal_record', 'signal_step')) and hasattr(NeuralAutomataAgent, 'signalling_action')


W, H, K = 20, 68, 3
CELLS = W * H
A, B, D, E = FAKE, FAKE + (1 << 20), FAKE + (2 << 20), FAKE + (3 << 20)       # a megabyte apart: nothing overlaps


def _cells(L, *, null=None, W=W, H=H, gW=0, epoch=3, standing=A, out=B):
    m = L.Medium(W, H, L.DIE_F32, 5, FAKE, FAKE, FAKE, FAKE + 8, gW, gW, 0, 0, 0, 0, 0, 0, None)
    args = dict(m=C.byref(m), standing=standing, out=out)
    if null:
        args[null] = None
    return L.lib.die_signal_cells(args['m'], args['standing'], epoch, args['out'], None)


def _backward(L, *, null=(), W=W, H=H, K=K, occupied=A, grad_next=B, field_stride=CELLS, grad_field=D, grad_emission=E, plane_stride=CELLS,
              deposit=0.75, sigma=0.5, decay=0.1):
    args = dict(occupied=occupied, grad_next=grad_next, grad_field=grad_field, grad_emission=grad_emission)
    for name in ([null] if isinstance(null, str) else null):
        args[name] = None
    return L.lib.die_signal_step_backward(W, H, args['occupied'], K, args['grad_next'], field_stride, args['grad_field'], args['grad_emission'],
                                          plane_stride, deposit, sigma, decay, None)


CELLS_CASES = [
    ('null medium', dict(null='m'), ARG, b'null argument'),
    ('null standing plane', dict(null='standing'), ARG, b'null argument'),
    ('null output', dict(null='out'), ARG, b'null argument'),
    ('empty field', dict(W=0), ARG, b'bad size'),
    ('decomposed medium', dict(gW=128), UNSUPPORTED, b'decomposed'),
    ('epoch 0', dict(epoch=0), ARG, b'epoch 0 outside 1..31'),
    ('epoch 32', dict(epoch=32), ARG, b'epoch 32 outside 1..31'),
    ('the output is the standing plane', dict(out=A), ARG, b'overlaps the standing plane'),
    ('the output starts in the standing plane', dict(out=A + 8 * CELLS - 1), ARG, b'overlaps the standing plane'),
    ('the output ends in the standing plane', dict(out=A - CELLS + 1), ARG, b'overlaps the standing plane'),
]
SPAN = ((K - 1) * CELLS + CELLS) * 4
BACKWARD_CASES = [
    ('null mask', dict(null='occupied'), ARG, b'null argument'),
    ('null incoming gradient', dict(null='grad_next'), ARG, b'null argument'),
    ('both outputs null', dict(null=('grad_field', 'grad_emission')), ARG, b'both absent'),
    ('empty field', dict(H=0), ARG, b'bad size'),
    ('no channel', dict(K=0), ARG, b'0 signal channels outside 1..8'),
    ('nine channels', dict(K=9), ARG, b'9 signal channels outside 1..8'),
    ('sigma 0', dict(sigma=0.0), ARG, b'sigma'),
    ('sigma nan', dict(sigma=float('nan')), ARG, b'sigma'),
    ('radius 0', dict(sigma=0.1), ARG, b'radius 0 outside 1..8'),
    ('radius 9', dict(sigma=2.2), ARG, b'radius 9 outside 1..8'),
    ('decay below 0', dict(decay=-0.1), ARG, b'decay'),
    ('decay above 1', dict(decay=1.5), ARG, b'decay'),
    ('decay nan', dict(decay=float('nan')), ARG, b'decay'),
    ('deposit inf', dict(deposit=float('inf')), ARG, b'deposit'),
    ('deposit nan', dict(deposit=float('nan')), ARG, b'deposit'),
    ('field_stride below a plane', dict(field_stride=CELLS - 1), ARG, b'field_stride'),
    ('plane_stride below a plane', dict(plane_stride=CELLS - 1), ARG, b'plane_stride'),
    ('grad_field is the incoming gradient', dict(grad_field=B), ARG, b'grad_field overlaps grad_field_next'),
    ('grad_field starts in the incoming gradient', dict(grad_field=B + SPAN - 4), ARG, b'grad_field overlaps grad_field_next'),
    ('grad_field ends in the mask', dict(grad_field=A - SPAN + 4), ARG, b'grad_field overlaps the occupancy plane'),
    ('grad_emission is the incoming gradient', dict(grad_emission=B), ARG, b'grad_emission overlaps grad_field_next'),
    ('grad_emission starts in the mask', dict(grad_emission=A + CELLS - 1), ARG, b'grad_emission overlaps the occupancy plane'),
    ('the outputs are one', dict(grad_emission=D), ARG, b'grad_emission overlaps grad_field'),
    ('grad_emission ends in grad_field', dict(grad_emission=D - SPAN + 4), ARG, b'grad_emission overlaps grad_field'),
]


def _ids(v):
    return v if isinstance(v, str) else None


@pytest.mark.parametrize('case, kw, status, needle', CELLS_CASES, ids=_ids)
def test_signal_cells_refusals(lib, case, kw, status, needle):
    assert _cells(lib, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and b'die_signal_cells:' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


@pytest.mark.parametrize('case, kw, status, needle', BACKWARD_CASES, ids=_ids)
def test_signal_step_backward_refusals(lib, case, kw, status, needle):
    assert _backward(lib, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and b'die_signal_step_backward:' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())



# ---------------------------------------------------------------------------------------------------- the example
def test_the_example_refuses_signal_channels_on_populations(lib, monkeypatch):
    import sys
    monkeypatch.syspath_prepend(os.path.join(ROOT, 'examples'))
    import recurrent_agent
    monkeypatch.setattr(sys, 'argv', ['recurrent_agent.py', '--replicas', '2', '--signal-channels', '2'])
    with pytest.raises(SystemExit, match='populations'):
        recurrent_agent.main()
    student = recurrent_agent.make_student(2, signal_channels=2)
    assert student.signal_channels == 2 and student.memory_channels == 2
    assert recurrent_agent.make_student(2).signal_channels == 0                   # the defaults are the run they were
