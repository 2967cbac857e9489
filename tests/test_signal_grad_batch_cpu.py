"""Batched BPTT through the signal channels (BatchedNeuralAutomataAgent.signalling_action), CPU side: the five new symbols with
their host-side argument checks (fake pointers: a launch would have failed), the float64 batched model of
tests/signal_grad_batch_model.py against its defining identity per replica and against the stand-alone model, the refusals of
`signalling_action` on a population that never saw a device, and the arguments of examples/signalling_population.py.  No kernel
is launched here."""
import ctypes as C
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import memory_grad_model as MG
from tests import signal_grad_batch_model as SB
from tests import signal_grad_model as SG
from tests import signal_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'die_signal_cells_batch': 7, 'die_signal_step_backward_batch': 15, 'die_nca_wide_sense_batch_store_signal': 12,
       'die_nca_wide_backward_batch_signal_workspace_bytes': 6, 'die_nca_wide_backward_batch_signal': 18}
FAKE = 1 << 20
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


# ---------------------------------------------------------------------------------------------------- the symbols
def test_new_symbols_declared_and_exported(lib):
    so = C.CDLL(lib.LIB_PATH)
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    header = open(os.path.join(ROOT, 'include', 'die_hip.h')).read()
    assert '#define DIE_ABI_VERSION 24' in header
    for name, n_args in NEW.items():
        assert hasattr(so, name) and name in lib.EXPORTS, name
        assert len(lib._SIGNATURES[name][1]) == n_args and len(getattr(lib.lib, name).argtypes) == n_args, name
        kind = 'int64_t' if name.endswith('_bytes') else 'int'
        proto = header[header.index(f'\n{kind} {name}('):]
        proto = proto[:proto.index(';')]
        assert proto.count(',') + 1 == n_args, (name, proto)
    from die_amd import functional
    from die_amd.batch import BatchedNeuralAutomataAgent
    assert all(hasattr(functional, n) for n in ('SignalRecordBatch', 'signal_record_batch', 'signal_step_batch'))
    sig = inspect.signature(BatchedNeuralAutomataAgent.signalling_action).parameters
    assert list(sig) == ['self', 'signals', 'memory', 'parameters'] and all(sig[k].default is None for k in list(sig)[1:])
    with pytest.raises(TypeError):
        functional.signal_record_batch(object())
    with pytest.raises(TypeError):
        functional.signal_step_batch(torch.zeros((2, 1, 4, 4)), torch.zeros((2, 1, 4, 4)), object(), deposit=1., sigma=.5, decay=0.)


# ---------------------------------------------------------------------------------------------------- the float64 model
@pytest.mark.parametrize('W,H,sigma,K', [(3, 8, 0.25, 1), (7, 252, 1.0, 3), (17, 257, 1.5, 2)])
def test_batched_model_is_R_stand_alone_runs_and_its_adjoint_identity_holds_per_replica(W, H, sigma, K):
    """<update(F, S)_r, g_r> = <F_r, gF_r> + <S_r, gS_r> in float64 for every replica, to 1e-12 of the sum of the terms' magnitudes;
    every replica's arrays are those of the stand-alone model on its own case, and the replicas differ."""
    R = 3
    F, occ, planes, g = SB.case_batch(W, H, K, R)
    g64 = g.astype(np.float64)
    gF, gS = SB.adjoint_batch(g64, occ, SM.DEPOSIT, sigma, SM.DECAY)
    nxt = SB.update_batch(F, occ, planes, SM.DEPOSIT, sigma, SM.DECAY)
    eF, eS = SB.emulate_backward_batch(g, occ, SM.DEPOSIT, sigma, SM.DECAY)
    bound = SB.bound_batch(g, sigma, SM.DECAY)
    for r in range(R):
        terms = [nxt[r] * g64[r], F[r].astype(np.float64) * gF[r], planes[r].astype(np.float64) * gS[r]]
        lhs, rhs = terms[0].sum(), terms[1].sum() + terms[2].sum()
        assert abs(lhs - rhs) <= 1e-12 * sum(np.abs(t).sum() for t in terms), (r, lhs, rhs)
        alone_F, alone_S = SG.adjoint(g64[r], occ[r], SM.DEPOSIT, sigma, SM.DECAY)
        assert np.array_equal(gF[r], alone_F) and np.array_equal(gS[r], alone_S)
        assert occ[r].any() and np.abs(terms[2]).sum() > 0 and not gS[r][:, ~occ[r]].any()
        assert (np.abs(eF[r].astype(np.float64) - gF[r]) <= bound[r]).all()          # the fp32 reference inside the GPU test's bound
        assert np.array_equal(eS[r].view(np.uint32), SG.emission_grad32(eF[r], occ[r], SM.DEPOSIT).view(np.uint32))
    assert not np.array_equal(occ[0], occ[1]) and not np.array_equal(g[0], g[1])


def test_with_episodes_a_candidate_row_is_the_sum_of_its_worlds():
    """unroll_batch with E = 2: the two replicas of a candidate share its weight tensors, so its gradient is the sum of the two
    stand-alone gradients — the float64 statement of the (C, P) gradient's row c."""
    W, H, N, T, K, E, R = 9, 7, 14, 2, 2, 2, 4
    rs = np.random.RandomState(11)
    worlds = [MG.synthetic_rounds(W, H, N, T, np.random.RandomState(20 + r), crowd=True) for r in range(R)]
    frames = [w[0] for w in worlds]
    occs = [[f['occ'] > 0 for f in fr] for fr in frames]
    raw = [[rs.uniform(-0.5, 0.5, (8, 3 + K, 3, 3)), rs.uniform(-0.5, 0.5, (3 + K, 8, 3, 3))] for _ in range(R // E)]
    sig0 = [torch.tensor(rs.standard_normal((K, W, H))) for _ in range(R)]
    proj = rs.standard_normal((R, 3, N))
    constants, coefs = (0.75, 0.8, 0.05), (0.1, 0.1, 2.0)

    def grads(replicas, episodes):
        ws = [[torch.tensor(w, requires_grad=True) for w in raw[c]] for c in sorted({r // E for r in replicas})]
        outs = SB.unroll_batch(ws, 'circular', 'tanh', [frames[r] for r in replicas], [occs[r] for r in replicas], [sig0[r] for r in replicas],
                               constants, coefs, episodes=episodes)
        sum((torch.as_tensor(proj[r]) * out['actions'][-1]).sum() for r, out in zip(replicas, outs)).backward()
        return [[w.grad.numpy() for w in row] for row in ws]

    both = grads([0, 1, 2, 3], E)
    for c in range(R // E):
        alone = [grads([c * E + e], 1)[0] for e in range(E)]
        for layer in range(2):
            want = alone[0][layer] + alone[1][layer]
            assert np.abs(want).max() > 0 and np.allclose(both[c][layer], want, rtol=1e-12, atol=1e-14 * np.abs(want).max())


# ---------------------------------------------------------------------------------------------------- the refusal tables
W, H, K, R, N = 20, 68, 3, 3, 300
CELLS = W * H
OCC = (CELLS + 15) // 16 * 16
A, B, D, E_ = FAKE, FAKE + (4 << 20), FAKE + (8 << 20), FAKE + (12 << 20)      # four megabytes apart: nothing overlaps


def _batch(L, *, replicas=R, plane_stride=CELLS, agent_stride=N, n=None):
    n = [N, N - 7, 0] + [0] * 61 if n is None else n
    return L.Batch(replicas, 0, plane_stride, agent_stride, 1, (C.c_int64 * 64)(*n))


def _cells(L, *, null=None, W=W, H=H, gW=0, epoch=3, standing=A, out=B, occupied_stride=OCC, **bkw):
    m = L.Medium(W, H, L.DIE_F32, 5, FAKE, FAKE, FAKE, FAKE + 8, gW, gW, 0, 0, 0, 0, 0, 0, None)
    args = dict(m=C.byref(m), b=C.byref(_batch(L, **bkw)), standing=standing, out=out)
    if null:
        args[null] = None
    return L.lib.die_signal_cells_batch(args['m'], args['b'], args['standing'], epoch, args['out'], occupied_stride, None)


def _backward(L, *, null=(), W=W, H=H, K=K, occupied=A, occupied_stride=OCC, grad_next=B, grad_field=D, grad_emission=E_, plane_stride=CELLS,
              replica_stride=K * CELLS, deposit=0.75, sigma=0.5, decay=0.1, field_stride=CELLS, **bkw):
    args = dict(b=C.byref(_batch(L, plane_stride=field_stride, **bkw)), occupied=occupied, grad_next=grad_next, grad_field=grad_field, grad_emission=grad_emission)
    for name in ([null] if isinstance(null, str) else null):
        args[name] = None
    return L.lib.die_signal_step_backward_batch(W, H, args['b'], args['occupied'], occupied_stride, K, args['grad_next'], args['grad_field'],
                                                args['grad_emission'], plane_stride, replica_stride, deposit, sigma, decay, None)


BATCH_CASES = [
    ('no replica', dict(replicas=0), ARG, b'replicas'),
    ('65 replicas', dict(replicas=65), ARG, b'replicas'),
    ('planes overlap', dict(plane_stride=CELLS - 1), ARG, b'plane_stride'),
    ('no slot a replica', dict(agent_stride=0), ARG, b'agent_stride'),
    ('a replica with more agents than slots', dict(n=[N, N + 1, 0] + [0] * 61), ARG, b'replica 1 has'),
    ('a replica with fewer than no agent', dict(n=[N, N, -1] + [0] * 61), ARG, b'replica 2 has'),
]
CELLS_CASES = [
    ('null medium', dict(null='m'), ARG, b'null argument'),
    ('null batch', dict(null='b'), ARG, b'null argument'),
    ('null standing planes', dict(null='standing'), ARG, b'null argument'),
    ('null output', dict(null='out'), ARG, b'null argument'),
    ('empty field', dict(W=0), ARG, b'bad size'),
    ('decomposed medium', dict(gW=128), UNSUPPORTED, b'decomposed'),
    ('epoch 0', dict(epoch=0), ARG, b'epoch 0 outside 1..31'),
    ('epoch 32', dict(epoch=32), ARG, b'epoch 32 outside 1..31'),
] + BATCH_CASES + [
    ('occupied_stride below a plane', dict(occupied_stride=CELLS - 1), ARG, b'occupied_stride'),
    ('the output is the standing planes', dict(out=A), ARG, b'overlaps the standing planes'),
    ('the output starts in the last standing plane', dict(out=A + 8 * ((R - 1) * CELLS + CELLS) - 1), ARG, b'overlaps the standing planes'),
    ('the last byte plane ends in the standing planes', dict(out=A - ((R - 1) * OCC + CELLS) + 1), ARG, b'overlaps the standing planes'),
]
FIELD_SPAN = ((K * R - 1) * CELLS + CELLS) * 4                         # K * R planes, plane-major
EM_SPAN = ((R - 1) * K * CELLS + (K - 1) * CELLS + CELLS) * 4          # R replicas of K planes, replica-major
OCC_SPAN = (R - 1) * OCC + CELLS
BACKWARD_CASES = [
    ('null batch', dict(null='b'), ARG, b'null argument'),
    ('null masks', dict(null='occupied'), ARG, b'null argument'),
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
] + [c for c in BATCH_CASES if 'plane_stride' not in c[1]] + [
    ('gradient planes overlap', dict(field_stride=CELLS - 1), ARG, b'plane_stride %d smaller than a plane' % (CELLS - 1)),
    ('occupied_stride below a plane', dict(occupied_stride=CELLS - 1), ARG, b'occupied_stride'),
    ('plane_stride below a plane', dict(plane_stride=CELLS - 1), ARG, b'plane_stride'),
    ('replica_stride below a plane', dict(replica_stride=CELLS - 1), ARG, b'would share words'),
    ('replica_stride below a replica\'s planes', dict(replica_stride=K * CELLS - 1), ARG, b'would share words'),
    ('plane-major planes that interleave', dict(replica_stride=CELLS, plane_stride=R * CELLS - 1), ARG, b'would share words'),
    ('grad_field is the incoming gradient', dict(grad_field=B), ARG, b'grad_field overlaps grad_field_next'),
    ('grad_field starts in the last incoming plane', dict(grad_field=B + FIELD_SPAN - 4), ARG, b'grad_field overlaps grad_field_next'),
    ('grad_field ends in the first mask', dict(grad_field=A - FIELD_SPAN + 4), ARG, b'grad_field overlaps the occupancy planes'),
    ('grad_field starts in the last mask', dict(grad_field=A + OCC_SPAN - 1), ARG, b'grad_field overlaps the occupancy planes'),
    ('grad_emission is the incoming gradient', dict(grad_emission=B), ARG, b'grad_emission overlaps grad_field_next'),
    ('grad_emission ends in the incoming gradient', dict(grad_emission=B - EM_SPAN + 4), ARG, b'grad_emission overlaps grad_field_next'),
    ('grad_emission starts in the last mask', dict(grad_emission=A + OCC_SPAN - 1), ARG, b'grad_emission overlaps the occupancy planes'),
    ('the outputs are one', dict(grad_emission=D), ARG, b'grad_emission overlaps grad_field'),
    ('grad_emission starts in the last plane of grad_field', dict(grad_emission=D + FIELD_SPAN - 4), ARG, b'grad_emission overlaps grad_field'),
    ('the last replica\'s emission planes end in grad_field', dict(grad_emission=D - EM_SPAN + 4), ARG, b'grad_emission overlaps grad_field'),
]


def _refused(lib, rc, status, needle, who, case):
    err = lib.lib.die_last_error()
    assert rc == status, (case, err)
    assert needle in err and who in err, (case, err)


@pytest.mark.parametrize('case, kw, status, needle', CELLS_CASES, ids=[c[0] for c in CELLS_CASES])
def test_signal_cells_batch_refusals(lib, case, kw, status, needle):
    _refused(lib, _cells(lib, **kw), status, needle, b'die_signal_cells_batch:', case)


@pytest.mark.parametrize('case, kw, status, needle', BACKWARD_CASES, ids=[c[0] for c in BACKWARD_CASES])
def test_signal_step_backward_batch_refusals(lib, case, kw, status, needle):
    _refused(lib, _backward(lib, **kw), status, needle, b'die_signal_step_backward_batch:', case)


@pytest.mark.parametrize('layout, strides', [('replica-major', dict(plane_stride=CELLS, replica_stride=K * CELLS)),
                                             ('replica-major, planes 3.. of 3 + K + 2', dict(plane_stride=CELLS, replica_stride=(5 + K) * CELLS)),
                                             ('plane-major', dict(plane_stride=R * CELLS, replica_stride=CELLS))])
def test_both_emission_layouts_pass_the_checks_up_to_the_overlap_check(lib, layout, strides):
    """Either layout is taken: the call gets as far as the LAST overlap check, which it is given to fail; and without a
    grad_emission its strides are not looked at."""
    _refused(lib, _backward(lib, grad_emission=D, **strides), ARG, b'grad_emission overlaps grad_field', b'die_signal_step_backward_batch:', layout)
    rc = _backward(lib, null='grad_emission', grad_field=B, plane_stride=0, replica_stride=0)
    _refused(lib, rc, ARG, b'grad_field overlaps grad_field_next', b'die_signal_step_backward_batch:', 'no emission gradient')


# ---- the signal-aware store / backward pair ----
WS, HS, RS, MS, KS = 24, 72, 4, 2, 2
TANH = 1
STACK = ((3, 3 + KS + MS, 8, TANH), (3, 8, 3 + KS + MS, TANH))      # (k, cin, cout, activation): ([agents,] food, chem, 2 signal, 2 memory planes)
NO_MEMORY = ((3, 3 + KS, 8, TANH), (3, 8, 3 + KS, TANH))
PLAIN = ((3, 3, 8, TANH), (3, 8, 3, TANH))
P_ROW = (3 + KS + MS) * 8 * 9 * 2
MEM = FAKE + (300 << 16)             # memory and signal planes clear of everything else
SIG = FAKE + (350 << 16)
GIN = FAKE + (400 << 16)
N_SENSE = 3 + KS + MS


def _structs(L, *, layers=STACK, replicas=RS, episodes=0, pad=0, plane_stride=None, epoch=1, weights=FAKE, dtype=None, agents_channel=1):
    m = L.Medium(WS, HS, L.DIE_F32 if dtype is None else dtype, 1, FAKE, FAKE + (1 << 16), FAKE + (2 << 16), None, 0, 0, 0, 0, 0, 0, 0, 0, None)
    arr = (L.NcaLayer * len(layers))(*[L.NcaLayer(k, cin, cout, act, weights, cout * cin * k * k) for k, cin, cout, act in layers])
    nca = L.NcaBatch(len(layers), pad, agents_channel, epoch, arr, (C.c_float * 3)(0.01, 0.01, 2.0), episodes, None, 0)
    b = L.Batch(replicas, 0, WS * HS if plane_stride is None else plane_stride, 10, 1, (C.c_int64 * 64)(*([10] * 64)))
    return m, arr, nca, b


def _sense(L, *, null=None, store_bytes=None, drop=None, masked=None, mem=MEM, M_=MS, sig=SIG, K_=KS, **kw):
    m, arr, nca, b = _structs(L, **kw)
    need = L.lib.die_nca_wide_sense_batch_store_bytes(WS, HS, RS, 2, 8)
    a = dict(m=C.byref(m), b=C.byref(b), nca=C.byref(nca), store=FAKE + (3 << 16), mem=mem, sig=sig)
    if null:
        a[null] = None
    return L.lib.die_nca_wide_sense_batch_store_signal(a['m'], a['b'], a['nca'], a['store'], need if store_bytes is None else store_bytes, masked,
                                                       None if drop is None else C.byref(L.NcaDropout(*drop)), a['mem'], M_, a['sig'], K_, None)


def _need(L, layers=STACK, M_=MS, K_=KS):
    return L.lib.die_nca_wide_backward_batch_signal_workspace_bytes(WS, HS, RS, C.byref(_structs(L, layers=layers)[2]), M_, K_)


def _stack_backward(L, *, null=None, workspace_bytes=None, sense_stride=N_SENSE * WS * HS, grad_stride=P_ROW, drop=None, grad=None, grad_in=None,
                    grad_in_stride=N_SENSE * WS * HS, mem=MEM, M_=MS, sig=SIG, K_=KS, **kw):
    m, arr, nca, b = _structs(L, **kw)
    need = _need(L)
    assert need > 0
    a = dict(m=C.byref(m), b=C.byref(b), nca=C.byref(nca), store=FAKE + (3 << 16), g=FAKE + (40 << 16), grad=FAKE + (50 << 16) if grad is None else grad,
             ws=FAKE + (60 << 16), mem=mem, sig=sig)
    if null:
        a[null] = None
    return L.lib.die_nca_wide_backward_batch_signal(a['m'], a['b'], a['nca'], a['store'], a['g'], sense_stride, a['grad'], grad_stride,
                                                    None if drop is None else C.byref(L.NcaDropout(*drop)), a['ws'],
                                                    need if workspace_bytes is None else workspace_bytes, grad_in, grad_in_stride, a['mem'], M_,
                                                    a['sig'], K_, None)


STACK_REFUSALS = [
    ('null medium', dict(null='m'), ARG, b'null argument'),
    ('null batch', dict(null='b'), ARG, b'null argument'),
    ('null stack', dict(null='nca'), ARG, b'null argument'),
    ('null store', dict(null='store'), ARG, b'null argument'),
    ('null signal planes', dict(null='sig'), ARG, b'null argument'),
    ('memory channels without memory planes', dict(null='mem'), ARG, b'memory channels'),
    ('memory planes without a memory channel', dict(M_=0), ARG, b'memory channels'),
    ('nine memory channels', dict(M_=9), ARG, b'9 memory channels outside 0..8'),
    ('no signal channel', dict(K_=0), ARG, b'0 signal channels outside 1..8'),
    ('nine signal channels', dict(K_=9), ARG, b'9 signal channels outside 1..8'),
    ('no replica', dict(replicas=0), ARG, b'replicas'),
    ('65 replicas', dict(replicas=65), ARG, b'replicas'),
    ('planes overlap', dict(plane_stride=WS * HS - 1), ARG, b'plane_stride'),
    ('episodes do not divide the replicas', dict(episodes=3), ARG, b'episodes'),
    ('kernel size 7', dict(layers=((7, 7, 8, TANH), (3, 8, 7, TANH))), ARG, b'kernel size 7'),
    ('33 channels', dict(layers=((3, 7, 33, TANH), (3, 33, 7, TANH))), ARG, b'channels'),
    ('a stack without signal or memory planes', dict(layers=PLAIN), ARG, b'input has 7'),
    ('a stack without memory, memory given', dict(layers=NO_MEMORY), ARG, b'input has 7'),
    ('another K than the stack\'s', dict(K_=3), ARG, b'input has 8'),
    ('the last layer gives 3 planes', dict(layers=((3, 7, 8, TANH), (3, 8, 3, TANH))), ARG, b'last layer gives 3 planes'),
    ('no agents channel, the same stack', dict(agents_channel=0), ARG, b'input has 6'),
    ('last layer not tanh', dict(layers=((3, 7, 8, TANH), (3, 8, 7, 2))), ARG, b'activation'),
    ('sense_epoch 0', dict(epoch=0), ARG, b'sense_epoch'),
    ('bad field dtype', dict(dtype=7), ARG, b'dtype'),
]
SENSE_REFUSALS = STACK_REFUSALS + [
    ('store too small', dict(store_bytes=1024), ARG, b'store too small'),
    ('mask without planes for the masked values', dict(drop=(0.25, 7, 1, 0, 0)), ARG, b'masked'),
    ('p out of range', dict(drop=(1.5, 7, 1, 0, 0), masked=FAKE + (90 << 16)), ARG, b'dropout p'),
    ('the memory planes are the store', dict(mem=FAKE + (3 << 16)), ARG, b'memory planes overlap'),
    ('the signal planes are the store', dict(sig=FAKE + (3 << 16)), ARG, b'signal planes overlap'),
    ('the signal planes end in the store', dict(sig=FAKE + (3 << 16) - 4 * (KS * RS * WS * HS - 1)), ARG, b'signal planes overlap'),
    ('the signal planes are the masked planes', dict(drop=(0.25, 7, 1, 0, 0), masked=SIG), ARG, b'signal planes overlap'),
]
BACKWARD_REFUSALS = STACK_REFUSALS + [
    ('null gradient planes', dict(null='g'), ARG, b'null argument'),
    ('null grad', dict(null='grad'), ARG, b'null argument'),
    ('null workspace', dict(null='ws'), ARG, b'null argument'),
    ('reflect', dict(pad=2), UNSUPPORTED, b'reflect'),
    ('gradient planes of three planes a replica', dict(sense_stride=3 * WS * HS), ARG, b'sense_stride'),
    ('gradient planes overlap', dict(sense_stride=N_SENSE * WS * HS - 1), ARG, b'below 7 planes'),
    ('gradient rows overlap', dict(grad_stride=P_ROW - 1), ARG, b'grad_stride'),
    ('grad is the weights', dict(grad=FAKE), ARG, b'weights'),
    ('workspace one byte short', dict(workspace_bytes=-1), ARG, b'workspace too small'),
    ('dropout reserved word', dict(drop=(0.25, 7, 1, 0, 1)), ARG, b'reserved'),
    ('grad_in of three planes a replica', dict(grad_in=GIN, grad_in_stride=3 * WS * HS), ARG, b'grad_in_stride'),
    ('grad_in not aligned', dict(grad_in=GIN + 4), ARG, b'16-byte aligned'),
    ('grad_in stride not a multiple of 4', dict(grad_in=GIN, grad_in_stride=N_SENSE * WS * HS + 2), ARG, b'multiple of 4'),
    ('grad_in is the store', dict(grad_in=FAKE + (3 << 16)), ARG, b'aliases'),
    ('grad_in is the memory planes', dict(grad_in=MEM), ARG, b'aliases'),
    ('grad_in is the signal planes', dict(grad_in=SIG), ARG, b'aliases'),
    ('grad_in starts in the last signal plane', dict(grad_in=SIG + 4 * (KS * RS * WS * HS - 4)), ARG, b'aliases'),
]


@pytest.mark.parametrize('case, kw, status, needle', SENSE_REFUSALS, ids=[c[0] for c in SENSE_REFUSALS])
def test_sense_store_signal_refused_before_launch(lib, case, kw, status, needle):
    _refused(lib, _sense(lib, **kw), status, needle, b'die_nca_wide_sense_batch_store_signal:', case)


@pytest.mark.parametrize('case, kw, status, needle', BACKWARD_REFUSALS, ids=[c[0] for c in BACKWARD_REFUSALS])
def test_backward_signal_refused_before_launch(lib, case, kw, status, needle):
    if kw.get('workspace_bytes') == -1:
        kw = dict(kw, workspace_bytes=_need(lib) - 1)
    _refused(lib, _stack_backward(lib, **kw), status, needle, b'die_nca_wide_backward_batch_signal:', case)


def test_no_memory_is_null_planes_and_zero_channels(lib):
    """M = 0 with null memory planes passes every stack check on a 3 + K stack: the calls get as far as a check they are given to fail."""
    _refused(lib, _sense(lib, layers=NO_MEMORY, mem=None, M_=0, store_bytes=1024), ARG, b'store too small', b'die_nca_wide_sense_batch_store_signal:', 'M = 0')
    rc = _stack_backward(lib, layers=NO_MEMORY, mem=None, M_=0, sense_stride=(3 + KS) * WS * HS, grad_stride=1)
    _refused(lib, rc, ARG, b'grad_stride', b'die_nca_wide_backward_batch_signal:', 'M = 0')


def test_byte_queries_and_the_older_entry_points(lib):
    """The signal query is the parent's formula with the stack's own channel counts and -1 for a refused shape; the two older
    queries and calls keep refusing a stack with signal planes, in their own words."""
    tiles = -(-WS // 16) * -(-HS // 64)
    want = 4 * (RS * tiles * max(co * ci * k * k for k, ci, co, _ in STACK) + 1 * RS * 8 * WS * HS)
    assert _need(lib) == want
    assert _need(lib, NO_MEMORY, 0, KS) == 4 * (RS * tiles * max(co * ci * k * k for k, ci, co, _ in NO_MEMORY) + RS * 8 * WS * HS)
    good = _structs(lib)[2]
    q = lib.lib.die_nca_wide_backward_batch_signal_workspace_bytes
    for bad in (dict(M=-1), dict(M=9), dict(M=3), dict(K_=0), dict(K_=9), dict(K_=3), dict(Wq=0), dict(R_=0), dict(R_=65), dict(null=True)):
        assert q(bad.get('Wq', WS), HS, bad.get('R_', RS), None if bad.get('null') else C.byref(good), bad.get('M', MS), bad.get('K_', KS)) == -1, bad
    for pad in (2, 3):
        assert q(WS, HS, RS, C.byref(_structs(lib, pad=pad)[2]), MS, KS) == -1
    assert q(WS, HS, RS, C.byref(_structs(lib, layers=PLAIN)[2]), MS, KS) == -1
    assert lib.lib.die_nca_wide_backward_batch_workspace_bytes(WS, HS, RS, C.byref(good)) == -1
    assert lib.lib.die_nca_wide_backward_batch_memory_workspace_bytes(WS, HS, RS, C.byref(good), MS) == -1
    m, arr, nca, b = _structs(lib)
    rc = lib.lib.die_nca_wide_backward_batch(C.byref(m), C.byref(b), C.byref(nca), FAKE + (3 << 16), FAKE + (40 << 16), N_SENSE * WS * HS,
                                             FAKE + (50 << 16), P_ROW, None, FAKE + (60 << 16), want, None, 0, None)
    _refused(lib, rc, ARG, b'input has 3', b'die_nca_wide_backward_batch:', 'the parent on a signal stack')
    rc = lib.lib.die_nca_wide_backward_batch_memory(C.byref(m), C.byref(b), C.byref(nca), FAKE + (3 << 16), FAKE + (40 << 16), N_SENSE * WS * HS,
                                                    FAKE + (50 << 16), P_ROW, None, FAKE + (60 << 16), want, None, 0, MEM, MS, None)
    _refused(lib, rc, ARG, b'input has 5', b'die_nca_wide_backward_batch_memory:', 'the memory call on a signal stack')
    need = lib.lib.die_nca_wide_sense_batch_store_bytes(WS, HS, RS, 2, 8)
    rc = lib.lib.die_nca_wide_sense_batch_store_memory(C.byref(m), C.byref(b), C.byref(nca), FAKE + (3 << 16), need, None, None, MEM, MS, None)
    _refused(lib, rc, ARG, b'input has 5', b'die_nca_wide_sense_batch_store_memory:', 'the memory store on a signal stack')


# ---------------------------------------------------------------------------------------------------- signalling_action's refusals
def _stub(signal_channels=2, memory_channels=2, stock=False, per_replica=False, dtype=torch.float32, boundary='circular', p=0.0, training=True,
          dropout_seed=3):
    """A BatchedNeuralAutomataAgent that never saw a device: what `signalling_action` reads before its first launch."""
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
    pop._signal_channels, pop._memory_channels, pop._stock_channel, pop._arch = signal_channels, memory_channels, stock, dict(boundary=(boundary,))
    pop.template = types.SimpleNamespace(model=types.SimpleNamespace(agent_dropout=types.SimpleNamespace(p=p), training=training))
    pop.dropout_seed, pop.dropout_seed_stride, pop.dropout_step = dropout_seed, 1, 4
    pop.parameters = torch.zeros((3, 5))
    pop.memory = torch.full((3, 2, 10), 0.5) if memory_channels else None
    pop._signals = torch.full((2, 3, 16, 12), 0.25) if signal_channels else None
    return pop


def test_signalling_action_refusals_touch_nothing(lib):
    sig, mem = (3, 2, 16, 12), (3, 2, 10)
    cases = [
        (dict(signal_channels=0), None, None, ValueError, 'recurrent_action'),
        (dict(signal_channels=0, memory_channels=0), None, None, ValueError, 'forward_device'),
        (dict(stock=True), None, None, NotImplementedError, 'stock'),
        (dict(per_replica=True), None, None, NotImplementedError, 'per_replica'),
        (dict(dtype=torch.float16), None, None, NotImplementedError, 'fp32'),
        (dict(boundary='reflect'), None, None, NotImplementedError, 'reflect'),
        (dict(boundary='replicate'), None, None, NotImplementedError, 'replicate'),
        (dict(p=0.25, dropout_seed=None), None, None, NotImplementedError, 'dropout_seed'),
        ({}, torch.zeros((3, 2, 16, 13)), None, ValueError, 'signals must be'),                     # another H
        ({}, torch.zeros((3, 3, 16, 12)), None, ValueError, 'signals must be'),                     # another K
        ({}, torch.zeros((2, 3, 16, 12)), None, ValueError, 'signals must be'),                     # the inner layout is not the public one
        ({}, torch.zeros(sig, dtype=torch.float64), None, ValueError, 'signals must be'),           # another dtype
        ({}, torch.zeros(sig, device='meta'), None, ValueError, 'signals must be'),                 # another device
        ({}, np.zeros(sig, dtype=np.float32), None, ValueError, 'signals must be'),                 # no tensor
        ({}, None, torch.zeros((3, 2, 9)), ValueError, 'memory must be'),                           # another Nmax
        ({}, None, torch.zeros((3, 3, 10)), ValueError, 'memory must be'),                          # another M
        ({}, None, torch.zeros(mem, dtype=torch.float64), ValueError, 'memory must be'),            # another dtype
        ({}, None, torch.zeros(mem, device='meta'), ValueError, 'memory must be'),                  # another device
        ({}, None, np.zeros(mem, dtype=np.float32), ValueError, 'memory must be'),                  # no tensor
        (dict(memory_channels=0), None, torch.zeros(mem), ValueError, 'without memory channels'),   # memory given with M = 0
    ]
    for kw, signals, memory, exc, needle in cases:
        pop = _stub(**kw)
        held, field = pop.memory, pop._signals
        with pytest.raises(exc, match=needle) as info:
            pop.signalling_action(signals, memory)
        assert 'signalling_action' in str(info.value) or needle == 'dropout_seed', kw
        assert pop.dropout_step == 4 and pop.memory is held and pop._signals is field, kw
        assert (held is None or bool((held == 0.5).all())) and (field is None or bool((field == 0.25).all())), kw
    pop = _stub()                                                    # a parameter matrix of the wrong shape
    with pytest.raises(ValueError, match='parameters'):
        pop.signalling_action(None, None, torch.zeros((3, 4)))
    assert pop.dropout_step == 4 and bool((pop.memory == 0.5).all()) and bool((pop._signals == 0.25).all())
    # what the issue keeps refused stays refused (the template's own refusal, reached before anything else)
    from die_amd import NeuralAutomataAgent
    pop = _stub()
    pop.template = NeuralAutomataAgent(kernel_sizes=(3, 3), hidden_channels=4, hidden_activation='tanh', memory_channels=2, signal_channels=2)
    for call in (pop.differentiable_sense, pop.differentiable_action, pop.forward_device, pop.recurrent_action):
        with pytest.raises(NotImplementedError, match='signal'):
            call()
    assert pop.dropout_step == 4 and bool((pop.memory == 0.5).all()) and bool((pop._signals == 0.25).all())


# ---------------------------------------------------------------------------------------------------- the examples
@pytest.fixture
def examples(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, 'examples'))
    import recurrent_agent
    import signalling_population
    return recurrent_agent, signalling_population


def test_the_new_example_reads_its_arguments(lib, examples):
    _, sp = examples
    a = sp.parse(['--replicas', '4', '--students', '2', '--signal-channels', '3', '--memory-channels', '0', '--unroll', '5', '--size', '32'])
    assert (a.replicas, a.students, a.signal_channels, a.memory_channels, a.unroll, a.size) == (4, 2, 3, 0, 5, 32)
    d = sp.parse([])
    assert (d.replicas, d.students, d.signal_channels, d.memory_channels, d.unroll, d.detach_every, d.steps) == (4, 4, 2, 2, 8, 0, 200)
    assert sp.check_arguments(6, 3, 1, 8) == (3, 2) and sp.check_arguments(5, None, 8, 0) == (5, 1)
    for argv, needle in ((['--replicas', '4', '--students', '3'], 'must divide'), (['--replicas', '0'], '--replicas'),
                         (['--students', '0'], 'must divide'), (['--signal-channels', '0'], 'recurrent_agent.py'),
                         (['--signal-channels', '9'], '--signal-channels'), (['--memory-channels', '9'], '--memory-channels'),
                         (['--memory-channels', '-1'], '--memory-channels'), (['--unroll', '0'], '--unroll'), (['--detach-every', '-1'], '--detach-every')):
        with pytest.raises(SystemExit, match=needle):
            sp.parse(argv)
    # the rest of its options are recurrent_agent.py's, and its students are that example's
    for option in ('--size', '--unroll', '--detach-every', '--steps', '--warm', '--hidden-channels', '--lr', '--seed', '--time'):
        assert option in inspect.getsource(sp.parse) and option in inspect.getsource(examples[0].main), option
    assert sp.make_student is examples[0].make_student and sp.SCALE == examples[0].SCALE


def test_recurrent_agent_still_refuses_signal_channels_on_populations_and_points_to_the_new_example(lib, examples, monkeypatch):
    ra, _ = examples
    monkeypatch.setattr(sys, 'argv', ['recurrent_agent.py', '--replicas', '2', '--signal-channels', '2'])
    with pytest.raises(SystemExit, match='populations with signal channels: examples/signalling_population.py'):
        ra.main()
    assert os.path.exists(os.path.join(ROOT, 'examples', 'signalling_population.py'))
