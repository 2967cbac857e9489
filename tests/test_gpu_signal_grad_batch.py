"""Batched BPTT through the signal channels on the device (BatchedNeuralAutomataAgent.signalling_action; die_signal_cells_batch /
die_signal_step_backward_batch; die_nca_wide_sense_batch_store_signal / die_nca_wide_backward_batch_signal;
die_amd.functional.signal_record_batch / signal_step_batch):

  1. the batched record byte for byte against R stand-alone calls and the numpy occupancy, guard bytes included;
  2. the batched backward kernel bit for bit against R stand-alone calls, against the batched forward's own sweep, in both emission
     layouts and with either output absent, inside tests/signal_grad_model.py `bound` of the float64 adjoint;
  3. the adjoint identity on device outputs;
  4. `signalling_action` bit for bit against `env.step(pop, action=buf)` on twin batches and against
     `replica_agent(r).signalling_action` on `Env.from_numpy(*benv.replica_numpy(r))`;
  5. one link: gradients bit for bit the stand-alone ones, the same bits twice;
  6. BPTT against the float64 loop of tests/signal_grad_batch_model.py fed the device's own records, on crowded worlds; the way
     through the field and its absence behind a detach; E = 2;
  7. field, memory and world together (BatchedEnv.differentiable_step between the links);
  8. a backward after the worlds were stepped, reset and the fields blanked;
  9. the refusals, which leave everything alone;
 10. ten Adam steps of examples/signalling_population.py.

The ceiling of every gradient comparison that is not bit for bit is 1e-4 of max|reference| per array and 1e-5 for the forward
trajectory (tests/test_gpu_signal_grad.py); the kernel's own bound is tests/signal_model.py `bound`.

No batched step takes a world with H % 4 != 0, so the 13 x 10 worlds stand still between their rounds (the field, which is what
the chain runs through, does not); the rounds of the 16 x 12 worlds are stepped by the detached actions."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from torch.nn.utils import parameters_to_vector

import die_amd as die
from die_amd import _lib, functional
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent
from die_amd.device_array import stream_ptr
from tests import field_step_adjoint_model as F
from tests import memory_grad_model as MG
from tests import memory_model as MM
from tests import signal_grad_batch_model as SB
from tests import signal_grad_model as SG
from tests import signal_model as SM
from tests import stock_plane_model as S

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CEILING = 1e-4                       # of max|grad_f64| per array: tests/test_gpu_signal_grad.py's, tests/test_gpu_memory_grad.py CEILING
FORWARD = 1e-5                       # the forward trajectory against the float64 loop (tests/test_gpu_signal_grad.py)
ID_TOL = 1e-6                        # tests/test_gpu_field_step_grad.py ID_TOL: the identity, of the sum of the terms' magnitudes
GUARD = 8                            # fp32 words of NaN around and between float planes (a multiple of 4: 16-byte planes stay so)
BYTE_GUARD = 16                      # bytes of 0xFF around the byte planes
NAN_BITS = MM.bits(np.float32('nan'))
SENTINEL = 7.5                       # what the planes of a sense-gradient buffer that are not the emission's hold
CONSTANTS = (0.75, 0.8, 0.05)        # signal_deposit, signal_sigma, signal_decay of the agents below (tests/test_gpu_signal.py's)
EPOCH = 9
N_REPLICA = (5, 0, 3)                # n[r] of the hand-made batches: different, one of them 0


def _sp():
    return stream_ptr(torch.device(DEV))


def _bits(t):
    return MM.bits(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)


def _medium(W, H):
    return _lib.Medium(W, H, _lib.DIE_F32, 1, None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, None)


def _batch(R, plane_stride, n=None):
    n = list(N_REPLICA[:R] if n is None else n)
    return _lib.Batch(R, 0, plane_stride, max(max(n), 1), 1, (C.c_int64 * 64)(*(n + [0] * (64 - len(n)))))


def _planes(values, pad, fill=None):
    """(buffer, view (n, cells + pad)): `values` (n, W, H) as n float planes cells + pad words apart, NaN in front and in every gap."""
    n, W, H = values.shape
    stride = W * H + pad
    buf = torch.full((pad + n * stride,), float('nan'), dtype=torch.float32, device=DEV)
    view = buf[pad:].view(n, stride)
    src = np.full((n, W * H), fill, dtype=np.float32) if fill is not None else np.ascontiguousarray(values, dtype=np.float32).reshape(n, W * H)
    view[:, :W * H] = torch.from_numpy(src).to(DEV)
    return buf, view


def _gaps_untouched(buf, n, cells, pad):
    host = _bits(buf)
    gaps = np.concatenate([host[:pad]] + [host[pad + k * (cells + pad) + cells:pad + (k + 1) * (cells + pad)] for k in range(n)])
    return gaps.size == (n + 1) * pad and (gaps == NAN_BITS).all()


def _byte_planes(R, cells, stride, fill=None):
    """(buffer, view (R, stride)): R byte planes `stride` bytes apart between BYTE_GUARD bytes of 0xFF; everything 0xFF but `fill`."""
    buf = torch.full((BYTE_GUARD + R * stride + BYTE_GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    view = buf[BYTE_GUARD:BYTE_GUARD + R * stride].view(R, stride)
    if fill is not None:
        view[:, :cells] = torch.from_numpy(np.ascontiguousarray(fill, dtype=np.uint8).reshape(R, cells)).to(DEV)
    return buf, view


def _byte_gaps_untouched(buf, R, cells, stride):
    host = buf.cpu().numpy()
    body = host[BYTE_GUARD:BYTE_GUARD + R * stride].reshape(R, stride)
    return (host[:BYTE_GUARD] == 0xFF).all() and (host[BYTE_GUARD + R * stride:] == 0xFF).all() and (body[:, cells:] == 0xFF).all()


def _standing(occ, stride):
    """(R, stride) int64 standing planes with exactly `occ` (R, W, H) occupied at EPOCH, stale words of the epoch before among the rest."""
    R, W, H = occ.shape
    words = np.zeros((R, stride), dtype=np.uint64)
    for r in range(R):
        words[r, :W * H] = SM.standing_words(occ[r], EPOCH, np.random.RandomState(W + H + r)).reshape(-1)
    return torch.from_numpy(words.view(np.int64)).to(DEV), words


# ---------------------------------------------------------------------------------------------------- 1. the record
@pytest.mark.parametrize('stores', ['16-byte stores', 'byte stores'])
@pytest.mark.parametrize('W,H', SM.SHAPES)
def test_signal_cells_batch_is_R_stand_alone_records_byte_for_byte(W, H, stores):
    R, cells = 3, W * H
    stride = (cells + 15) // 16 * 16 if stores == '16-byte stores' else cells + 3
    assert (stride % 16 == 0) == (stores == '16-byte stores')
    _, occ, _, _ = SB.case_batch(W, H, 1, R)
    pstride = (cells + 3) // 2 * 2                                                 # even: every replica's words on a 16-byte boundary
    standing, words = _standing(occ, pstride)
    assert all((words[r, :cells][~occ[r].reshape(-1)] != 0).any() and occ[r].any() for r in range(R))     # stale words among the empty cells
    buf, out = _byte_planes(R, cells, stride)
    b = _batch(R, pstride)
    _lib.check(_lib.lib.die_signal_cells_batch(C.byref(_medium(W, H)), C.byref(b), standing.data_ptr(), EPOCH, out.data_ptr(), stride, _sp()),
               'die_signal_cells_batch')
    got = out[:, :cells].cpu().numpy().reshape(R, W, H)
    assert np.array_equal(got, occ.astype(np.uint8))                               # every byte of every plane written: nothing left of the 0xFF
    assert _byte_gaps_untouched(buf, R, cells, stride)                             # between and around the planes: intact
    assert np.array_equal(standing.cpu().numpy().view(np.uint64), words)
    for r in range(R):                                                             # R stand-alone calls: the same bytes
        alone = torch.full((cells,), 0xFF, dtype=torch.uint8, device=DEV)
        _lib.check(_lib.lib.die_signal_cells(C.byref(_medium(W, H)), standing[r].data_ptr(), EPOCH, alone.data_ptr(), _sp()), 'die_signal_cells')
        assert np.array_equal(alone.cpu().numpy(), got[r].reshape(-1)), r
    out.fill_(0xFF)                                                                # … and at another epoch nobody stands anywhere
    _lib.check(_lib.lib.die_signal_cells_batch(C.byref(_medium(W, H)), C.byref(b), standing.data_ptr(), EPOCH + 1, out.data_ptr(), stride, _sp()),
               'die_signal_cells_batch')
    assert not out[:, :cells].cpu().numpy().any() and _byte_gaps_untouched(buf, R, cells, stride)


# ---------------------------------------------------------------------------------------------------- 2. the backward kernel
def _backward_batch(W, H, b, mask, mstride, K, g, gf, ge, plane_stride, replica_stride, sigma):
    _lib.check(_lib.lib.die_signal_step_backward_batch(W, H, C.byref(b), mask.data_ptr(), mstride, K, g.data_ptr(),
                                                       None if gf is None else gf.data_ptr(), None if ge is None else ge.data_ptr(),
                                                       plane_stride, replica_stride, SM.DEPOSIT, sigma, SM.DECAY, _sp()),
               'die_signal_step_backward_batch')


def _kernel_case(W, H, sigma, K, R=3, pad=GUARD, tail=2):
    """The batched backward on gradient planes cells + pad words apart: everything around the outputs checked, every replica and
    channel compared bit for bit with the stand-alone call on that replica's planes.  Returns (g, occ, grad_field) as (R, K, W, H)."""
    cells, stride = W * H, W * H + pad
    _, occ, planes, g = SB.case_batch(W, H, K, R)
    assert not (MM.bits(g) == 0x80000000).any() and (g > 0).any() and (g < 0).any()          # mixed signs, no negative zero
    mstride = (cells + 15) // 16 * 16
    mask_buf, mask = _byte_planes(R, cells, mstride, fill=occ)
    km = lambda a: np.ascontiguousarray(np.swapaxes(a, 0, 1)).reshape(K * R, W, H)           # (R, K, ..) -> plane k * R + r
    g_buf, gin = _planes(km(g), pad)
    f_buf, gf = _planes(km(g), pad, fill=np.nan)
    b = _batch(R, stride)
    # the emission gradient replica-major, at plane 3 of an (R, 3 + K + tail, W, H) sense-gradient buffer full of a sentinel
    n_sense = 3 + K + tail
    sense = torch.full((R, n_sense, W, H), SENTINEL, dtype=torch.float32, device=DEV)
    ge = sense[:, 3:3 + K]
    _backward_batch(W, H, b, mask, mstride, K, gin, gf, ge, cells, n_sense * cells, sigma)
    got_f = np.swapaxes(gf[:, :cells].reshape(K, R, W, H).cpu().numpy(), 0, 1)
    host = sense.cpu().numpy()
    got_e = host[:, 3:3 + K]
    assert not np.isnan(got_f).any()                                               # every cell of every output plane is written
    assert (host[:, :3] == SENTINEL).all() and (host[:, 3 + K:] == SENTINEL).all() # … and the other planes of the buffer survive
    assert _gaps_untouched(g_buf, K * R, cells, pad) and _gaps_untouched(f_buf, K * R, cells, pad)
    assert np.array_equal(_bits(gin[:, :cells]), MM.bits(km(g)).reshape(K * R, cells))         # the inputs are read, not written
    assert np.array_equal(mask[:, :cells].cpu().numpy().reshape(R, W, H), occ.astype(np.uint8)) and _byte_gaps_untouched(mask_buf, R, cells, mstride)
    # plane-major, as the field lies: the same bits
    e_buf, pm = _planes(km(g), pad, fill=np.nan)
    _backward_batch(W, H, b, mask, mstride, K, gin, None, pm, R * stride, stride, sigma)
    assert _gaps_untouched(e_buf, K * R, cells, pad)
    assert np.array_equal(MM.bits(np.swapaxes(pm[:, :cells].reshape(K, R, W, H).cpu().numpy(), 0, 1)), MM.bits(got_e))
    # each output alone (the other null): the same bits
    _, only_f = _planes(km(g), pad, fill=np.nan)
    _backward_batch(W, H, b, mask, mstride, K, gin, only_f, None, 0, 0, sigma)
    assert np.array_equal(_bits(only_f), _bits(gf))
    # the adjoint IS the forward's sweep: die_signal_step_batch on the gradient planes at an epoch where nobody stands
    standing, _ = _standing(occ, stride)
    em = torch.from_numpy(planes).to(DEV)
    _, fwd = _planes(km(g), pad, fill=np.nan)
    _lib.check(_lib.lib.die_signal_step_batch(C.byref(_medium(W, H)), C.byref(b), standing.data_ptr(), EPOCH + 1, K, em.data_ptr(), cells, K * cells,
                                              gin.data_ptr(), fwd.data_ptr(), SM.DEPOSIT, sigma, SM.DECAY, _sp()), 'die_signal_step_batch')
    assert np.array_equal(_bits(gf[:, :cells]), _bits(fwd[:, :cells]))
    # every replica alone: die_signal_step_backward on its K planes where they lie (R strides apart), outputs laid out alike
    for r in range(R):
        _, af = _planes(km(g), pad, fill=np.nan)
        _, ae = _planes(km(g), pad, fill=np.nan)
        _lib.check(_lib.lib.die_signal_step_backward(W, H, mask[r].data_ptr(), K, gin[r].data_ptr(), R * stride, af[r].data_ptr(), ae[r].data_ptr(),
                                                     R * stride, SM.DEPOSIT, sigma, SM.DECAY, _sp()), 'die_signal_step_backward')
        alone_f = af[:, :cells].reshape(K, R, W, H)[:, r].cpu().numpy()
        alone_e = ae[:, :cells].reshape(K, R, W, H)[:, r].cpu().numpy()
        assert np.array_equal(MM.bits(alone_f), MM.bits(got_f[r])) and np.array_equal(MM.bits(alone_e), MM.bits(got_e[r])), r
        # the emission gradient: one fp32 multiply of the device's own grad_field where somebody stands, +0.0 elsewhere
        assert np.array_equal(MM.bits(got_e[r]), MM.bits(SG.emission_grad32(got_f[r], occ[r], SM.DEPOSIT))), r
        assert got_e[r].any() and not MM.bits(got_e[r][:, ~occ[r]]).any(), r
    return g, occ, got_f


@pytest.mark.parametrize('K', SM.CHANNELS)
@pytest.mark.parametrize('sigma', SM.SIGMAS)
@pytest.mark.parametrize('W,H', SM.SHAPES)
def test_backward_batch_kernel_against_the_stand_alone_call_the_forward_sweep_and_the_model(W, H, sigma, K):
    g, occ, got_f = _kernel_case(W, H, sigma, K)
    want, _ = SB.adjoint_batch(g, occ, SM.DEPOSIT, sigma, SM.DECAY)
    err, bound = np.abs(got_f.astype(np.float64) - want), SB.bound_batch(g, sigma, SM.DECAY)
    print(f'{W}x{H} sigma {sigma} K {K} R 3: worst share of the bound {(err / bound).max():.4f}')
    assert (err <= bound).all(), (err / bound).max()


def test_backward_batch_kernel_eight_channels():
    W, H, sigma, K = 7, 252, 0.5, 8
    g, occ, got_f = _kernel_case(W, H, sigma, K, tail=0)
    want, _ = SB.adjoint_batch(g, occ, SM.DEPOSIT, sigma, SM.DECAY)
    assert (np.abs(got_f.astype(np.float64) - want) <= SB.bound_batch(g, sigma, SM.DECAY)).all()


# ---------------------------------------------------------------------------------------------------- 3. the identity
@pytest.mark.parametrize('W,H', [(7, 252), (17, 257)], ids=['row kernel, two strips', 'tile kernel'])
def test_adjoint_identity_on_device_outputs(W, H):
    """<die_signal_step_batch(F, S), g> = <F, gF> + <S, gS> over all replicas with every array the device's own, summed in float64:
    within ID_TOL of the sum of the terms' magnitudes (tests/test_gpu_signal_grad.py test 3), and so for every replica alone."""
    R, K, sigma, cells = 2, 2, 0.5, W * H
    F_, occ, planes, g = SB.case_batch(W, H, K, R)
    standing, _ = _standing(occ, cells)
    b = _batch(R, cells, n=(4, 2))
    kr = lambda a: torch.from_numpy(np.ascontiguousarray(np.swapaxes(a, 0, 1))).to(DEV)      # (K, R, W, H): the field's layout
    tF, tg, tS = kr(F_), kr(g), torch.from_numpy(planes).to(DEV)
    mask = torch.empty((R, W, H), dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib.die_signal_cells_batch(C.byref(_medium(W, H)), C.byref(b), standing.data_ptr(), EPOCH, mask.data_ptr(), cells, _sp()),
               'die_signal_cells_batch')
    nxt, gF = torch.full_like(tF, float('nan')), torch.full_like(tF, float('nan'))
    gS = torch.full_like(tS, float('nan'))
    _lib.check(_lib.lib.die_signal_step_batch(C.byref(_medium(W, H)), C.byref(b), standing.data_ptr(), EPOCH, K, tS.data_ptr(), cells, K * cells,
                                              tF.data_ptr(), nxt.data_ptr(), SM.DEPOSIT, sigma, SM.DECAY, _sp()), 'die_signal_step_batch')
    _backward_batch(W, H, b, mask, cells, K, tg, gF, gS, cells, K * cells, sigma)
    d = lambda t: t.cpu().numpy().astype(np.float64)
    rk = lambda t: np.swapaxes(d(t), 0, 1)
    terms = [rk(nxt) * rk(tg), rk(tF) * rk(gF), d(tS) * d(gS)]                     # (R, K, W, H) each
    for r in [slice(None)] + list(range(R)):
        lhs, rhs, scale = terms[0][r].sum(), terms[1][r].sum() + terms[2][r].sum(), sum(np.abs(t[r]).sum() for t in terms)
        print(f'signal step batch {W}x{H} replica {r}: apart by {abs(lhs - rhs) / scale:.2e} of the terms\' magnitudes (ceiling {ID_TOL:.0e})')
        assert abs(lhs - rhs) <= ID_TOL * scale
        assert np.abs(terms[2][r]).sum() > 0.01 * scale                            # the emission term is a real share of it


# ---------------------------------------------------------------------------------------------------- populations and worlds
WIDE = dict(kernel_sizes=(3, 3), hidden_channels=8, hidden_activation='tanh')


def _cands(n, seed, K=2, M=0, p=0.0, **kw):
    torch.manual_seed(seed)
    deposit, sigma, decay = CONSTANTS
    sig = dict(signal_channels=K, signal_deposit=deposit, signal_sigma=sigma, signal_decay=decay) if K else {}
    out = []
    for _ in range(n):
        ag = die.NeuralAutomataAgent(scale=F.COEFS[0], deposit=F.COEFS[2], memory_channels=M, p_agent_dropout=p, **sig, **dict(WIDE, **kw))
        with torch.no_grad():
            for q in ag.model.parameters():
                q.uniform_(-0.5, 0.5)
        out.append(ag)
    return out


def _make(W, H, R=3, E=1, K=2, M=0, p=0.0, seed=11, slots='alive', dyn=None, pop_kw=None, model_kw=None):
    benv = BatchedEnv((W, H), die.Dynamics(**(dyn or dict(init_agent_ratio=0.3))), replicas=R, seed=seed, max_agents=slots, device=DEV)
    pop = BatchedNeuralAutomataAgent.from_agents(benv, _cands(R // E, W + R, K, M, p, **(model_kw or {})), E, **(pop_kw or {}))
    assert pop._signal_channels == K and pop._memory_channels == M and not benv.per_replica
    return benv, pop


def _crowd(benv, seed):
    """Replace every replica's world by one of random coordinates with a fifth of the slots dead and more agents than a third of the
    cells (tests/test_gpu_stock.py `_world`): dead slots, and cells that several alive agents share.  The batch must hold the fixed
    layout; the state goes in as the constructor puts a replica's in."""
    from tests.test_gpu_stock import _world
    assert benv._fixed is not None and benv.epoch == 1
    for r in range(benv.R):
        medium, agents = _world(benv.W, benv.H, benv.Nmax, np.random.RandomState(seed + r))
        e = die.Env.from_numpy(medium, agents, device=DEV, sort_every=0)
        assert e.agents.N == benv.Nmax == benv.n[r] and e.medium.epoch == 1
        benv.owner[r].copy_(e.medium.owner); benv.food[r].copy_(e.medium.food); benv.chem[r].copy_(e.medium.chem)
        benv.x[r].copy_(e.agents.x); benv.y[r].copy_(e.agents.y); benv.alive[r].copy_(e.agents.alive); benv.agent_food[r].copy_(e.agents.agent_food)
    torch.cuda.synchronize()


def _alone(benv, pop, r):
    """Replica r as a stand-alone world and agent, as they stand now (the population's dropout counter)."""
    env = die.Env.from_numpy(*benv.replica_numpy(r), device=DEV, sort_every=0)
    ag = pop.replica_agent(r)
    ag.dropout_step = pop.dropout_step
    return env, ag


def _world_bits(benv):
    return benv._state.cpu().numpy().copy(), benv.epoch


def _same_world(a, b):
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def _row_of(ag):
    return parameters_to_vector([q.grad for q in ag.model.parameters()]).detach().cpu().numpy()


def _layer_grads(pop, row):
    """A (P,) row as the list of its layers' (cout, cin, k, k) arrays."""
    return [np.asarray(row[off:off + cout * cin * k * k]).reshape(cout, cin, k, k) for k, cin, cout, off in pop._layers]


# ---------------------------------------------------------------------------------------------------- 4. the same as the step
VALUES = {
    # (W, H), R, E, M, seeded mask
    '24x68': ((24, 68), 3, 1, 0, False), '24x68 memory': ((24, 68), 3, 1, 2, False),
    '24x68 mask': ((24, 68), 3, 1, 0, True), '24x68 memory mask': ((24, 68), 3, 1, 2, True),
    '24x68 memory mask E=2': ((24, 68), 4, 2, 2, True),
    '13x10': ((13, 10), 3, 1, 0, False), '13x10 memory': ((13, 10), 3, 1, 2, False),
    '13x10 mask': ((13, 10), 3, 1, 0, True), '13x10 memory mask': ((13, 10), 3, 1, 2, True),
}


@pytest.mark.parametrize('case', list(VALUES))
def test_signalling_action_is_the_step_and_the_stand_alone_call_bit_for_bit(case, links=3, before=None):
    """24 x 68: past the wide layer's 16 x 64 tile in both axes, the row kernel.  13 x 10: H % 4 != 0, the tile kernel; no batched
    step takes such a world, so it stands still and is compared with the stand-alone call only.  (`links`, `before` — a callable of
    the two fresh batches: tests/test_gpu_epoch_wrap.py runs the same checks across the epoch wrap.)"""
    (W, H), R, E, M, seeded = VALUES[case]
    K = 2
    kw = dict(R=R, E=E, K=K, M=M, p=0.25 if seeded else 0.0, pop_kw=dict(dropout_seed=40, dropout_seed_stride=1) if seeded else {})
    (benv_s, pop_s), (benv_d, pop_d) = _make(W, H, **kw), _make(W, H, **kw)
    if before is not None:
        before(benv_s, benv_d)
    Nmax = benv_s.Nmax
    _same_world(_world_bits(benv_s), _world_bits(benv_d))
    assert len(set(benv_d.n)) > 1                                                 # differing n[r]: padding slots
    steps = H % 4 == 0
    buf = torch.zeros((3, R, Nmax), dtype=torch.float32, device=DEV)
    pop_d.parameters.requires_grad_()                                              # (a graph hangs on what asks for a gradient: here the weights)
    signals = memory = None
    for t in range(links):
        sig_in = pop_d.signals.clone()
        mem_in = pop_d.memory.clone() if M else None
        alone = [_alone(benv_d, pop_d, r) for r in range(R)]
        action, signals, memory = pop_d.signalling_action(signals, memory)
        assert action.shape == (3, R, Nmax) and signals.shape == (R, K, W, H) and action.dtype == signals.dtype == torch.float32
        assert action.grad_fn is not None and signals.grad_fn is not None
        assert (memory is None) == (M == 0) and (M == 0 or (memory.shape == (R, M, Nmax) and memory.grad_fn is not None))
        if steps:
            benv_s.step(pop_s, action=buf)
        for r in range(R):
            n = benv_d.n[r]
            assert not steps or np.array_equal(_bits(action[:, r, :n]), _bits(buf[:, r, :n])), (t, r)
            assert not _bits(action[:, r, n:]).any() and (M == 0 or not _bits(memory[r, :, n:]).any()), (t, r)        # the padding: 0
            env, ag = alone[r]
            a, s, m = ag.signalling_action(env._get_current_obs, sig_in[r].contiguous(), mem_in[r, :, :n].contiguous() if M else None)
            assert np.array_equal(_bits(a), _bits(action[:, r, :n])) and np.array_equal(_bits(s), _bits(signals[r])), (t, r)
            assert M == 0 or np.array_equal(_bits(m), _bits(memory[r, :, :n])), (t, r)
        # the population's own copies, in its own storage
        assert np.array_equal(_bits(pop_d.signals), _bits(signals)) and pop_d._signals.data_ptr() != signals.data_ptr(), t
        assert M == 0 or (np.array_equal(_bits(pop_d.memory), _bits(memory)) and pop_d.memory.data_ptr() != memory.data_ptr()), t
        assert pop_d.dropout_step == (t + 1 if seeded else 0)
        if steps:
            assert np.array_equal(_bits(pop_s.signals), _bits(signals)) and pop_s.dropout_step == pop_d.dropout_step, t
            assert M == 0 or np.array_equal(_bits(pop_s.memory), _bits(memory)), t
            benv_d.step_action(action)
            _same_world(_world_bits(benv_s), _world_bits(benv_d))
    assert float(signals.detach().abs().max()) > 0 and (M == 0 or float(memory.detach().abs().max()) > 0)


# ---------------------------------------------------------------------------------------------------- 5. one link
@pytest.mark.parametrize('W,H,M', [(13, 10, 0), (16, 12, 2), (24, 68, 0)])
def test_one_link_gradients_are_the_stand_alone_ones_bit_for_bit(W, H, M):
    K, R = 2, 3
    benv, pop = _make(W, H, R=R, K=K, M=M)
    Nmax = benv.Nmax
    rs = np.random.RandomState(3)
    u = torch.from_numpy(rs.standard_normal((3, R, Nmax)).astype(np.float32)).to(DEV) * (benv.alive > 0)      # the alive slots' actions
    v = torch.from_numpy(rs.standard_normal((R, K, W, H)).astype(np.float32)).to(DEV)
    sig0 = (rs.uniform(-1, 1, (R, K, W, H)) * (rs.rand(R, K, W, H) < 0.6)).astype(np.float32)
    leaf = torch.from_numpy(sig0).to(DEV).requires_grad_()
    alone = [_alone(benv, pop, r) for r in range(R)]
    pop.parameters.requires_grad_()
    action, signals, _ = pop.signalling_action(leaf)
    loss = (u * action).sum() + (v * signals).sum()
    loss.backward(retain_graph=True)
    got_p, got_s = pop.parameters.grad.clone(), leaf.grad.clone()
    pop.parameters.grad = leaf.grad = None
    loss.backward()
    assert np.array_equal(_bits(got_p), _bits(pop.parameters.grad)) and np.array_equal(_bits(got_s), _bits(leaf.grad))        # the same bits twice
    assert got_s.shape == (R, K, W, H)                                             # the gradient comes back in the public shape
    for r in range(R):
        n = benv.n[r]
        env, ag = alone[r]
        sig = torch.from_numpy(sig0[r]).to(DEV).requires_grad_()
        a, s, _ = ag.signalling_action(env._get_current_obs, sig)
        ((u[:, r, :n] * a).sum() + (v[r] * s).sum()).backward()
        assert np.array_equal(_bits(got_p[r]), MM.bits(_row_of(ag))), r
        assert np.array_equal(_bits(got_s[r]), _bits(sig.grad)), r
    assert float(got_s.abs().max()) > 0 and float(got_p.abs().max()) > 0
    # a leaf of other strides: the inner (K, R, W, H) layout permuted back
    inner = torch.from_numpy(np.ascontiguousarray(np.swapaxes(sig0, 0, 1))).to(DEV).requires_grad_()
    benv2, pop2 = _make(W, H, R=R, K=K, M=M)
    pop2.parameters.requires_grad_()
    a2, s2, _ = pop2.signalling_action(inner.permute(1, 0, 2, 3))
    ((u * a2).sum() + (v * s2).sum()).backward()
    assert np.array_equal(_bits(inner.grad.permute(1, 0, 2, 3)), _bits(got_s)) and np.array_equal(_bits(pop2.parameters.grad), _bits(got_p))


# ---------------------------------------------------------------------------------------------------- 6. BPTT
def _frame(benv, pop, r):
    W, H, n = benv.W, benv.H, benv.n[r]
    m, _ = benv.replica_numpy(r)
    cx = S.cell(benv.x[r, :n].cpu().numpy().view(np.uint32), W)
    cy = S.cell(benv.y[r, :n].cpu().numpy().view(np.uint32), H)
    return dict(occ=m[0], food=m[1], chem=m[2], cx=cx, cy=cy, mask=None)


def _occupancies(benv, pop):
    """The device's own record of who stands where now, (R, W, H) bool — and the model's, which it must equal."""
    rec = functional.signal_record_batch(pop)
    assert rec.occupied.dtype == torch.uint8 and tuple(rec.occupied.shape) == (benv.R, benv.W, benv.H)
    occ = rec.occupied.cpu().numpy() > 0
    for r in range(benv.R):
        assert np.array_equal(occ[r], SM.occupancy_of(benv.W, benv.H, benv.replica_numpy(r)[1])), r
    return occ


def _bptt(W, H, R=3, E=1, T=3, loss_on_signals=True, detach=False, before=None):
    """T rounds chained through signals_next from a leaf on crowded worlds (60 slots on 13 x 10, 90 on 16 x 12); the worlds are
    stepped by the detached actions where a batched step takes them (H % 4 == 0).  `before`: a callable of (benv, pop) run on the
    crowded worlds first (tests/test_gpu_epoch_wrap.py: real steps up to the epoch wrap)."""
    K, N = 2, 60 if (W, H) == (13, 10) else 90
    benv, pop = _make(W, H, R=R, E=E, K=K, slots=N, dyn=dict(init_agent_ratio=0.1))
    _crowd(benv, seed=21)
    if before is not None:
        before(benv, pop)
    rs = np.random.RandomState(4)
    u, v = rs.standard_normal((3, R, N)), rs.standard_normal((R, K, W, H))
    sig0 = (rs.uniform(-1, 1, (R, K, W, H)) * (rs.rand(R, K, W, H) < 0.6)).astype(np.float32)
    leaf = torch.from_numpy(sig0).to(DEV).requires_grad_(True)
    pop.parameters.requires_grad_()
    signals, frames, occs = leaf, [[] for _ in range(R)], [[] for _ in range(R)]
    for t in range(T):
        occ = _occupancies(benv, pop)
        alive = benv.alive.cpu().numpy() > 0
        for r in range(R):
            frames[r].append(_frame(benv, pop, r))
            occs[r].append(occ[r])
            assert alive[r].sum() < N and 0 < occ[r].sum() < alive[r].sum(), (t, r)    # dead slots, and cells that several alive agents share
        action, signals, _ = pop.signalling_action(signals.detach() if detach and t > 0 else signals)
        if t < T - 1 and H % 4 == 0:
            benv.step_action(action)
    ud, vd = (torch.as_tensor(a, dtype=torch.float32, device=DEV) for a in (u, v))
    loss = (ud * action).sum() + ((vd * signals).sum() if loss_on_signals else 0.)
    loss.backward()
    torch.cuda.synchronize()
    # the float64 loop on the device's data
    host = pop.parameters.detach().cpu().double().numpy()
    ws = [[torch.tensor(w, requires_grad=True) for w in _layer_grads(pop, host[c])] for c in range(pop.candidates)]
    s0 = [torch.tensor(sig0[r].astype(np.float64), requires_grad=True) for r in range(R)]
    outs = SB.unroll_batch(ws, 'circular', 'tanh', frames, occs, s0, CONSTANTS, pop.template.action_coefs, episodes=E,
                           with_agent_channel=pop._arch['with_agent_channel'], detach_at=range(1, T) if detach else ())
    ref_loss = sum((torch.as_tensor(u[:, r]) * out['actions'][-1]).sum() + ((torch.as_tensor(v[r]) * out['signals'][-1]).sum() if loss_on_signals else 0.)
                   for r, out in enumerate(outs))
    ref_loss.backward()
    zero = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()     # noqa: E731
    got = [_layer_grads(pop, row) for row in pop.parameters.grad.cpu().numpy()]
    fwd = max(max(MG.rel_err(action[:, r].detach().cpu().numpy(), out['actions'][-1].detach().numpy()),
                  MG.rel_err(signals[r].detach().cpu().numpy(), out['signals'][-1].detach().numpy())) for r, out in enumerate(outs))
    return dict(pop=pop, got=got, ref=[[zero(w) for w in row] for row in ws], got_s=np.zeros(sig0.shape) if leaf.grad is None else leaf.grad.cpu().numpy(), ref_s=np.stack([zero(s) for s in s0]),
                fwd=fwd)


@pytest.mark.parametrize('W,H,R,E', [(13, 10, 3, 1), (16, 12, 3, 1), (13, 10, 4, 2)], ids=['13x10', '16x12 stepped', '13x10 E=2'])
def test_bptt_gradients_match_the_float64_loop(W, H, R, E):
    """With E = 2 row c of the (C, P) gradient is the sum of its two worlds' model gradients: the loop's two replicas of a candidate
    share its weight tensors."""
    run = _bptt(W, H, R, E)
    errs = [MG.rel_err(g, ref) for gc, rc in zip(run['got'], run['ref']) for g, ref in zip(gc, rc)]
    assert len(run['got']) == R // E and all(np.abs(ref).max() > 0 for rc in run['ref'] for ref in rc)
    errs_s = [MG.rel_err(run['got_s'][r], run['ref_s'][r]) for r in range(R)]
    print(f'bptt {W}x{H} T=3 R={R} E={E}: device', ' '.join(f'{e:.3e}' for e in errs), '(of max|grad_f64| per candidate and layer);',
          ' '.join(f'{e:.3e}' for e in errs_s), f'(d loss / d signals0 per replica; ceiling {CEILING:.0e}); forward apart by {run["fwd"]:.2e}')
    assert run['fwd'] <= FORWARD                                                   # the model followed the same trajectory
    assert np.abs(run['ref_s']).max() > 0 and max(errs + errs_s) <= CEILING, (errs, errs_s)


def test_the_gradient_goes_through_the_field():
    # the loss is on the last action alone: the last layer's rows 3 .. 3 + K - 1, which produce emissions, are reached through the field only
    K = 2
    run = _bptt(13, 10, loss_on_signals=False)
    for got, ref in zip(run['got'], run['ref']):
        assert np.abs(got[-1][3:3 + K]).max() > 0 and np.abs(ref[-1][3:3 + K]).max() > 0
        assert MG.rel_err(got[-1][3:3 + K], ref[-1][3:3 + K]) <= CEILING and all(MG.rel_err(g, r) <= CEILING for g, r in zip(got, ref))
    assert max(MG.rel_err(a, b) for a, b in zip(run['got_s'], run['ref_s'])) <= CEILING
    # signals_next.detach() handed on instead: nothing reaches those rows, on the device and in the model
    run = _bptt(13, 10, loss_on_signals=False, detach=True)
    for got, ref in zip(run['got'], run['ref']):
        assert not got[-1][3:3 + K].any() and not ref[-1][3:3 + K].any() and np.abs(got[-1][:3]).max() > 0
        assert all(MG.rel_err(g, r) <= CEILING for g, r in zip(got, ref))
    assert not run['got_s'].any() and not run['ref_s'].any()                        # … nor the leaf, which the first link alone read


# ---------------------------------------------------------------------------------------------------- 7. memory and the worlds
def _through_the_worlds(T=2, before=None):
    """T links of signalling_action + differentiable_step on three 16 x 12 worlds from blank fields and blank memory, a loss on the
    last chem planes and the last fields, against the float64 loop: (forward distance, errors per replica and layer; the emission
    and memory rows of every replica's last layer are held to the ceiling here).  `before`: a callable of (benv, pop) run on the
    fresh worlds first (tests/test_gpu_epoch_wrap.py)."""
    W, H, sigma, K, M, R = 16, 12, 0.8, 2, 2, 3
    benv, pop = _make(W, H, R=R, K=K, M=M, seed=5, dyn=dict(init_agent_ratio=0.3, diffuse_sigma=sigma, rate_decay_chem=F.DECAY, diffuse_mode='wrap'))
    if before is not None:
        before(benv, pop)
    pop.parameters.requires_grad_()
    rs = np.random.RandomState(6)
    cvec, svec = rs.standard_normal((R, W, H)), rs.standard_normal((R, K, W, H))
    chem0 = benv.differentiable_chem().cpu().numpy().copy()
    frames, occs, records, cells = ([[] for _ in range(R)] for _ in range(4))
    signals = memory = None
    for t in range(T):
        occ = _occupancies(benv, pop)
        rec = functional.memory_record_batch(pop)
        cell, win = rec.cell.cpu().numpy(), rec.win.cpu().numpy()
        for r in range(R):
            frames[r].append(_frame(benv, pop, r))
            occs[r].append(occ[r])
            records[r].append((cell[r, :benv.n[r]].copy(), win[r, :benv.n[r]].copy()))
        action, signals, memory = pop.signalling_action(signals, memory)
        benv.differentiable_step(action)
        won = benv.differentiable_chem().grad_fn.saved_tensors[0].cpu().numpy()
        for r in range(R):
            cells[r].append(won[r, :benv.n[r]].copy())
    node = benv.differentiable_chem()
    loss = (torch.as_tensor(cvec, dtype=torch.float32, device=DEV) * node).sum() + (torch.as_tensor(svec, dtype=torch.float32, device=DEV) * signals).sum()
    chem_T, sig_T = node.detach().cpu().numpy().copy(), signals.detach().cpu().numpy().copy()
    loss.backward()
    torch.cuda.synchronize()
    host = pop.parameters.detach().cpu().double().numpy()
    ws = [[torch.tensor(w, requires_grad=True) for w in _layer_grads(pop, host[c])] for c in range(R)]
    outs = SB.unroll_batch(ws, 'circular', 'tanh', frames, occs, [torch.zeros((K, W, H), dtype=torch.float64) for _ in range(R)], CONSTANTS,
                           pop.template.action_coefs, records, [torch.zeros((M, benv.n[r]), dtype=torch.float64) for r in range(R)],
                           with_agent_channel=pop._arch['with_agent_channel'], chem0=[torch.tensor(chem0[r].astype(np.float64)) for r in range(R)],
                           worlds=[dict(cells=cells[r], sigma=sigma, decay=F.DECAY) for r in range(R)])
    sum((torch.as_tensor(cvec[r]) * out['chem']).sum() + (torch.as_tensor(svec[r]) * out['signals'][-1]).sum() for r, out in enumerate(outs)).backward()
    fwd = max(max(MG.rel_err(chem_T[r], out['chem'].detach().numpy()), MG.rel_err(sig_T[r], out['signals'][-1].detach().numpy()))
              for r, out in enumerate(outs))
    got = [_layer_grads(pop, row) for row in pop.parameters.grad.cpu().numpy()]
    errs = []
    for r in range(R):
        ref = [w.grad.numpy() for w in ws[r]]
        errs += [MG.rel_err(g, w) for g, w in zip(got[r], ref)]
        # the emission rows and the memory rows of the last layer reach this loss through the field, the memory and the world
        assert np.abs(ref[-1][3:3 + K]).max() > 0 and MG.rel_err(got[r][-1][3:3 + K], ref[-1][3:3 + K]) <= CEILING, r
        assert np.abs(ref[-1][3 + K:]).max() > 0 and MG.rel_err(got[r][-1][3 + K:], ref[-1][3 + K:]) <= CEILING, r
    return fwd, errs


def test_gradients_through_the_field_the_memory_and_the_worlds():
    fwd, errs = _through_the_worlds()
    print('field, memory and worlds 16x12 T=2 R=3: device', ' '.join(f'{e:.3e}' for e in errs), f'(ceiling {CEILING:.0e}); forward apart by {fwd:.2e}')
    assert fwd <= 1e-4 and max(errs) <= CEILING, (fwd, errs)                        # (the chem plane's forward bound: tests/test_gpu_signal_grad.py test 7)


# ---------------------------------------------------------------------------------------------------- 8. the record carries the graph
def _two_links(move_on):
    W, H, R, K, M = 16, 12, 3, 2, 2
    benv, pop = _make(W, H, R=R, K=K, M=M, seed=5)
    pop.parameters.requires_grad_()
    rs = np.random.RandomState(8)
    v = torch.from_numpy(rs.standard_normal((R, K, W, H)).astype(np.float32)).to(DEV)
    u = torch.from_numpy(rs.standard_normal((3, R, benv.Nmax)).astype(np.float32)).to(DEV)
    signals = memory = None
    loss = 0.
    for _ in range(2):
        action, signals, memory = pop.signalling_action(signals, memory)
        loss = loss + (u * (benv.alive > 0) * action).sum()
        benv.step_action(action)
    loss = loss + (v * signals).sum()
    if move_on:                                                                   # the worlds go on and start over, the fields are blanked
        with torch.no_grad():
            benv.run(pop, 2)
        benv.reset()
        pop.reset_signals()
        assert not pop.signals.any()
    loss.backward()
    torch.cuda.synchronize()
    return _bits(pop.parameters.grad)


def test_backward_after_the_worlds_moved_on_gives_the_same_bits():
    at_once, again, later = _two_links(False), _two_links(False), _two_links(True)
    assert at_once.any()
    assert np.array_equal(at_once, again)                                          # two runs: the same bits
    assert np.array_equal(at_once, later)                                          # the records, not the worlds, drive the backward


# ---------------------------------------------------------------------------------------------------- 9. the refusals
REFUSALS = {
    # what: (how the population differs, the error, a word of its message)
    'no signal channels': (dict(K=0), ValueError, 'recurrent_action'),
    'stock': (dict(model_kw=dict(with_stock_channel=True)), NotImplementedError, 'stock'),
    'per_replica': ({}, NotImplementedError, 'per_replica'),
    'fp16': ({}, NotImplementedError, 'fp32'),
    'reflect': (dict(model_kw=dict(boundary='reflect')), NotImplementedError, 'reflect'),
    'replicate': (dict(model_kw=dict(boundary='replicate')), NotImplementedError, 'replicate'),
    'unseeded dropout': (dict(seeded=False), NotImplementedError, 'dropout_seed'),
    'signals of another shape': ({}, ValueError, 'signals'),
    'signals in the inner layout': ({}, ValueError, 'signals'),
    'signals of another dtype': ({}, ValueError, 'signals'),
    'signals on another device': ({}, ValueError, 'signals'),
    'signals no tensor': ({}, ValueError, 'signals'),
    'memory of another shape': ({}, ValueError, 'memory'),
    'memory of another dtype': ({}, ValueError, 'memory'),
    'memory on another device': ({}, ValueError, 'memory'),
    'memory no tensor': ({}, ValueError, 'memory'),
    'memory without memory channels': (dict(M=0), ValueError, 'memory'),
}


@pytest.mark.parametrize('what', list(REFUSALS))
def test_refusals_on_the_device_leave_everything_alone(what):
    W, H, R = 13, 10, 2
    extra, error, needle = REFUSALS[what]
    K, M = extra.get('K', 2), extra.get('M', 2)
    benv = BatchedEnv((W, H), die.Dynamics(init_agent_ratio=0.3), replicas=R, seed=2, device=DEV,
                      field_dtype=torch.float16 if what == 'fp16' else torch.float32, per_replica=True if what == 'per_replica' else None)
    pop = BatchedNeuralAutomataAgent.from_agents(benv, _cands(R, 1, K, M, 0.25, **extra.get('model_kw', {})),
                                                 dropout_seed=3 if extra.get('seeded', True) else None)
    pop.dropout_step = 4
    Nmax = benv.Nmax
    held, field = pop.memory, pop._signals
    if held is not None:
        held.fill_(0.5)
    if field is not None:
        field.fill_(0.25)
    before = None if benv.per_replica else _world_bits(benv)
    sig, mem = (R, 2, W, H), (R, 2, Nmax)
    signals = {'signals of another shape': torch.zeros((R, 2, W, H + 1), device=DEV), 'signals in the inner layout': torch.zeros((2, R + 1, W, H), device=DEV),
               'signals of another dtype': torch.zeros(sig, dtype=torch.float64, device=DEV), 'signals on another device': torch.zeros(sig),
               'signals no tensor': np.zeros(sig, dtype=np.float32)}.get(what)
    memory = {'memory of another shape': torch.zeros((R, 2, Nmax + 1), device=DEV), 'memory of another dtype': torch.zeros(mem, dtype=torch.float64, device=DEV),
              'memory on another device': torch.zeros(mem), 'memory no tensor': np.zeros(mem, dtype=np.float32),
              'memory without memory channels': torch.zeros(mem, device=DEV)}.get(what)
    with pytest.raises(error, match=needle):
        pop.signalling_action(signals, memory)
    assert pop.dropout_step == 4 and pop.memory is held and pop._signals is field
    assert (held is None or bool((held == 0.5).all())) and (field is None or bool((field == 0.25).all()))
    if before is not None:
        _same_world(before, _world_bits(benv))


def test_the_other_differentiable_calls_keep_refusing_a_signalling_population():
    benv, pop = _make(13, 10, R=2, K=2, M=2, p=0.25, pop_kw=dict(dropout_seed=3))
    pop.dropout_step = 4
    pop.memory.fill_(0.5)
    pop._signals.fill_(0.25)
    before = _world_bits(benv)
    for call in (pop.differentiable_sense, pop.differentiable_action, pop.forward_device, pop.recurrent_action):
        with pytest.raises(NotImplementedError, match='signal'):
            call()
    assert pop.dropout_step == 4 and bool((pop.memory == 0.5).all()) and bool((pop._signals == 0.25).all())
    _same_world(before, _world_bits(benv))


# ---------------------------------------------------------------------------------------------------- 10. training
def test_ten_adam_steps_of_the_example_decrease_the_loss():
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    try:
        import signalling_population
    finally:
        sys.path.pop(0)
    pop, losses = signalling_population.train(16, 2, 2, 3, 0, 10, replicas=4, students=2, log=lambda *_: None)
    print('signalling_population --size 16 --unroll 3 --replicas 4 --students 2, K=2 M=2, ten Adam steps:', ' '.join(f'{v:.4f}' for v in losses))
    assert len(losses) == 10 and np.isfinite(losses).all() and losses[-1] < losses[0]
    assert pop.candidates == 2 and pop.parameters.grad.shape == (2, pop.P)
    for row in pop.parameters.grad.cpu().numpy():                                  # the emission rows, after the last backward
        rows = _layer_grads(pop, row)[-1][3:5]
        assert np.isfinite(rows).all() and np.abs(rows).max() > 0
    assert float(pop.signals.abs().max()) > 0 and float(pop.memory.abs().max()) > 0
