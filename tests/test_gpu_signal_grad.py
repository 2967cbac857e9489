"""Gradients through signal channels on the device (die_signal_grad.hip; die_amd.functional.signal_record / signal_step;
NeuralAutomataAgent.signalling_action): the occupancy record byte for byte, the backward kernel against the float64 adjoint inside
the forward's bound and against the forward's own sweep bit for bit, the adjoint identity on device outputs, `signalling_action`
against `forward` bit for bit on twin worlds, backpropagation through time against the float64 loop of tests/signal_grad_model.py
fed the device's own records, the gradient's way through the field (and its absence behind a detach), through the memory and the
world as well, a backward after the world has moved on, the refusals, and ten Adam steps of examples/recurrent_agent.py.

The ceiling of every gradient comparison is 1e-4 of max|reference| per array (tests/test_gpu_memory_grad.py CEILING); the kernel's
own bound is tests/signal_model.py `bound`, which tests/test_signal_grad_cpu.py shows the fp32 reference alone to stay inside."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib, functional
from die_amd.device_array import stream_ptr
from tests import field_step_adjoint_model as F
from tests import memory_grad_model as MG
from tests import memory_model as MM
from tests import signal_grad_model as SG
from tests import signal_model as SM
from tests.test_gpu_field_step_grad import ID_TOL
from tests.test_gpu_memory_grad import CEILING, _device_grads, _errors, _frame, _same_state, _state, _step_with
from tests.test_gpu_signal import GUARD, _bits, _gaps_untouched, _guarded, _signal_step
from tests.test_gpu_stock import _world

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTE_GUARD = 16                      # bytes of 0xFF before and after a byte plane (16: the plane stays 16-byte aligned)
CONSTANTS = (0.75, 0.8, 0.05)        # signal_deposit, signal_sigma, signal_decay of the agents below (tests/test_gpu_signal.py's)


def _sp():
    return stream_ptr(torch.device(DEV))


def _medium(W, H):
    return _lib.Medium(W, H, _lib.DIE_F32, 1, None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, None)


def _guarded_bytes(cells, shift=0, fill=None):
    """(buffer, view): `cells` bytes with BYTE_GUARD + shift bytes of 0xFF in front and BYTE_GUARD behind."""
    buf = torch.full((BYTE_GUARD + shift + cells + BYTE_GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    view = buf[BYTE_GUARD + shift:BYTE_GUARD + shift + cells]
    if fill is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(fill, dtype=np.uint8).reshape(-1)).to(DEV))
    return buf, view


def _byte_guards_untouched(buf, cells, shift=0):
    host = buf.cpu().numpy()
    return (host[:BYTE_GUARD + shift] == 0xFF).all() and (host[BYTE_GUARD + shift + cells:] == 0xFF).all()


# ---------------------------------------------------------------------------------------------------- 1. the record
@pytest.mark.parametrize('shift', [0, 3], ids=['16-byte stores', 'byte stores'])
@pytest.mark.parametrize('W,H', SM.SHAPES)
def test_signal_cells_is_the_occupancy_byte_for_byte(W, H, shift):
    epoch, cells = 9, W * H
    _, occ, _ = SM.case(W, H, 1)
    rs = np.random.RandomState(W + H)
    words = SM.standing_words(occ, epoch, rs)
    assert (words[~occ] != 0).any() and occ.any()                                 # stale words of the epoch before among the empty cells
    standing = torch.from_numpy(words.view(np.int64)).to(DEV)
    buf, out = _guarded_bytes(cells, shift)
    _lib.check(_lib.lib.die_signal_cells(C.byref(_medium(W, H)), standing.data_ptr(), epoch, out.data_ptr(), _sp()), 'die_signal_cells')
    assert np.array_equal(out.cpu().numpy().reshape(W, H), occ.astype(np.uint8))  # every byte written: nothing left of the 0xFF
    assert _byte_guards_untouched(buf, cells, shift)
    assert np.array_equal(standing.cpu().numpy().view(np.uint64), words)
    out.fill_(0xFF)                                                               # … and at another epoch nobody stands anywhere
    _lib.check(_lib.lib.die_signal_cells(C.byref(_medium(W, H)), standing.data_ptr(), epoch + 1, out.data_ptr(), _sp()), 'die_signal_cells')
    assert not out.cpu().numpy().any()


# ---------------------------------------------------------------------------------------------------- 2. the backward kernel
def _backward(W, H, K, mask, g, stride, gf, ge, em_stride, deposit, sigma, decay):
    _lib.check(_lib.lib.die_signal_step_backward(W, H, mask.data_ptr(), K, g.data_ptr(), stride, None if gf is None else gf.data_ptr(),
                                                 None if ge is None else ge.data_ptr(), em_stride, deposit, sigma, decay, _sp()),
               'die_signal_step_backward')


def _kernel_case(W, H, sigma, K, pad):
    """One run of the backward kernel on planes `pad` words apart: (grad_field, grad_emission) host arrays (K, W, H), everything
    around them checked."""
    epoch, cells, stride = 9, W * H, W * H + pad
    _, occ, planes = SM.case(W, H, K)
    g = SG.grad_case(W, H, K)
    assert not (MM.bits(g) == 0x80000000).any() and (g > 0).any() and (g < 0).any()      # mixed signs, no negative zero
    mask_buf, mask = _guarded_bytes(cells, fill=occ)
    g_buf, gin = _guarded(g, pad)
    f_buf, gf = _guarded(np.full((K, W, H), np.nan, dtype=np.float32), pad)
    e_buf, ge = _guarded(np.full((K, W, H), np.nan, dtype=np.float32), pad)
    _backward(W, H, K, mask, gin, stride, gf, ge, stride, SM.DEPOSIT, sigma, SM.DECAY)
    got_f, got_e = (t[:, :cells].reshape(K, W, H).cpu().numpy() for t in (gf, ge))
    assert not np.isnan(got_f).any() and not np.isnan(got_e).any()                # every cell of every output plane is written
    for buf in (g_buf, f_buf, e_buf):
        assert _gaps_untouched(buf, K, cells, pad)
    assert np.array_equal(_bits(gin[:, :cells]), MM.bits(g).reshape(K, cells))     # the inputs are read, not written
    assert np.array_equal(mask.cpu().numpy().reshape(W, H), occ.astype(np.uint8)) and _byte_guards_untouched(mask_buf, cells)
    # the adjoint IS the forward's sweep: die_signal_step on the field g, at an epoch where nobody stands, same strides and alignment
    rs = np.random.RandomState(W + H)
    standing = torch.from_numpy(SM.standing_words(occ, epoch, rs).view(np.int64)).to(DEV)
    _, em = _guarded(planes, pad)
    _, fwd = _guarded(np.full((K, W, H), np.nan, dtype=np.float32), pad)
    _signal_step(W, H, K, standing, epoch + 1, em, stride, gin, fwd, stride, SM.DEPOSIT, sigma, SM.DECAY)
    assert np.array_equal(_bits(gf[:, :cells]), _bits(fwd[:, :cells]))
    # the emission gradient: one fp32 multiply of the device's own grad_field where somebody stands, +0.0 elsewhere
    assert np.array_equal(MM.bits(got_e), MM.bits(SG.emission_grad32(got_f, occ, SM.DEPOSIT)))
    assert got_e.any() and not MM.bits(got_e[:, ~occ]).any()
    # each output absent in turn: the other gets the same bits
    _, only_f = _guarded(np.full((K, W, H), np.nan, dtype=np.float32), pad)
    _, only_e = _guarded(np.full((K, W, H), np.nan, dtype=np.float32), pad)
    _backward(W, H, K, mask, gin, stride, only_f, None, 0, SM.DEPOSIT, sigma, SM.DECAY)
    _backward(W, H, K, mask, gin, stride, None, only_e, stride, SM.DEPOSIT, sigma, SM.DECAY)
    assert np.array_equal(_bits(only_f), _bits(gf)) and np.array_equal(_bits(only_e), _bits(ge))
    return g, occ, got_f, got_e


@pytest.mark.parametrize('K', SM.CHANNELS)
@pytest.mark.parametrize('sigma', SM.SIGMAS)
@pytest.mark.parametrize('W,H', SM.SHAPES)
def test_backward_kernel_against_the_model_and_the_forward_sweep(W, H, sigma, K):
    """|grad_field - (1 - decay) G(g)| <= tests/signal_model.py `bound` with F := g and nobody standing — the forward's bound, since the
    adjoint is the forward's sweep — and grad_field bit for bit that sweep.  Planes GUARD words apart (the row kernel where it
    applies), then 6 words apart (no plane 16-byte aligned: the tile kernel), where the forward's bits at that padding are the measure."""
    g, occ, got_f, _ = _kernel_case(W, H, sigma, K, GUARD)
    want, _ = SG.adjoint(g, occ, SM.DEPOSIT, sigma, SM.DECAY)
    err, bound = np.abs(got_f.astype(np.float64) - want), SG.bound(g, sigma, SM.DECAY)
    print(f'{W}x{H} sigma {sigma} K {K}: worst share of the bound {(err / bound).max():.4f}')
    assert (err <= bound).all(), (err / bound).max()
    _, _, tile_f, _ = _kernel_case(W, H, sigma, K, 6)
    assert (np.abs(tile_f.astype(np.float64) - want) <= bound).all()


def test_backward_kernel_eight_channels():
    W, H, sigma, K = 7, 252, 0.5, 8
    g, occ, got_f, _ = _kernel_case(W, H, sigma, K, GUARD)
    want, _ = SG.adjoint(g, occ, SM.DEPOSIT, sigma, SM.DECAY)
    assert (np.abs(got_f.astype(np.float64) - want) <= SG.bound(g, sigma, SM.DECAY)).all()


def test_backward_kernel_on_the_record_of_a_world_with_shared_cells():
    """The mask as the library makes it — die_stock_plane, then functional.signal_record — for agents of which several share a cell
    and some are dead: the record is the model's occupancy, and the emission gradient follows it."""
    W, H, N, K, sigma = 12, 20, 150, 2, 0.5
    medium, agents = _world(W, H, N, np.random.RandomState(12))
    env = die.Env.from_numpy(medium, agents, device=DEV, sort_every=0)
    a = env.agents.to_numpy()
    occ = SM.occupancy_of(W, H, a)
    alive = int((a[2] > 0).sum())
    assert 0 < occ.sum() < alive < N                                              # shared cells, dead slots
    record = functional.signal_record(env._get_current_obs)
    assert record.occupied.dtype == torch.uint8 and tuple(record.occupied.shape) == (W, H) and (record.W, record.H) == (W, H)
    assert np.array_equal(record.occupied.cpu().numpy(), occ.astype(np.uint8))
    g = SG.grad_case(W, H, K)
    gin = torch.from_numpy(g).to(DEV)
    gf, ge = torch.full_like(gin, float('nan')), torch.full_like(gin, float('nan'))
    _backward(W, H, K, record.occupied, gin, W * H, gf, ge, W * H, SM.DEPOSIT, sigma, SM.DECAY)
    got_f, got_e = gf.cpu().numpy(), ge.cpu().numpy()
    want, _ = SG.adjoint(g, occ, SM.DEPOSIT, sigma, SM.DECAY)
    assert (np.abs(got_f.astype(np.float64) - want) <= SG.bound(g, sigma, SM.DECAY)).all()
    assert np.array_equal(MM.bits(got_e), MM.bits(SG.emission_grad32(got_f, occ, SM.DEPOSIT))) and got_e.any()


# ---------------------------------------------------------------------------------------------------- 3. the identity
@pytest.mark.parametrize('W,H', [(7, 252), (17, 257)], ids=['row kernel, two strips', 'tile kernel'])
def test_adjoint_identity_on_device_outputs(W, H):
    """<die_signal_step(F, S), g> = <F, gF> + <S, gS> with every array the device's own, summed in float64: within ID_TOL of the sum of
    the terms' magnitudes (tests/test_gpu_field_step_grad.py test 4: fp32 outputs, 2^-24 a term, far below 1e-6 of that sum)."""
    K, sigma, epoch, cells = 2, 0.5, 9, W * H
    F_, occ, planes = SM.case(W, H, K)
    g = SG.grad_case(W, H, K)
    rs = np.random.RandomState(W + H)
    standing = torch.from_numpy(SM.standing_words(occ, epoch, rs).view(np.int64)).to(DEV)
    tF, tS, tg = (torch.from_numpy(a).to(DEV) for a in (F_, planes, g))
    mask = torch.empty((W, H), dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib.die_signal_cells(C.byref(_medium(W, H)), standing.data_ptr(), epoch, mask.data_ptr(), _sp()), 'die_signal_cells')
    nxt, gF, gS = (torch.full_like(tF, float('nan')) for _ in range(3))
    _signal_step(W, H, K, standing, epoch, tS, cells, tF, nxt, cells, SM.DEPOSIT, sigma, SM.DECAY)
    _backward(W, H, K, mask, tg, cells, gF, gS, cells, SM.DEPOSIT, sigma, SM.DECAY)
    d = lambda t: t.cpu().numpy().astype(np.float64)
    terms = [d(nxt) * d(tg), d(tF) * d(gF), d(tS) * d(gS)]
    lhs, rhs, scale = terms[0].sum(), terms[1].sum() + terms[2].sum(), sum(np.abs(t).sum() for t in terms)
    print(f'signal step {W}x{H}: <step(F, S), g> = {lhs:.9e}, <F, gF> + <S, gS> = {rhs:.9e}, apart by {abs(lhs - rhs) / scale:.2e} of the '
          f"terms' magnitudes (ceiling {ID_TOL:.0e})")
    assert abs(lhs - rhs) <= ID_TOL * scale
    assert np.abs(terms[2]).sum() > 0.01 * scale                                  # the emission term is a real share of it


# ---------------------------------------------------------------------------------------------------- the agents and worlds
def _agent(K=2, M=0, seed=0, p=0.0, dropout_seed=None, scale=F.COEFS[0], **kw):
    torch.manual_seed(seed)
    deposit, sigma, decay = CONSTANTS
    ag = die.NeuralAutomataAgent(kernel_sizes=(3, 3), hidden_channels=8, hidden_activation='tanh', scale=scale, deposit=F.COEFS[2],
                                 p_agent_dropout=p, dropout_seed=dropout_seed, signal_channels=K, memory_channels=M, signal_deposit=deposit,
                                 signal_sigma=sigma, signal_decay=decay, **kw)
    with torch.no_grad():
        for q in ag.model.parameters():
            q.uniform_(-0.5, 0.5)
    assert ag.model.training
    return ag


def _twin(ag, **kw):
    other = _agent(**kw)
    other.model.load_state_dict(ag.model.state_dict())
    return other


def _env(W, H, seed=3, **dyn):
    return die.Env((W, H), die.Dynamics(init_agent_ratio=0.3, **dyn), seed=seed, device=DEV, sort_every=0)


def _crowded_env(W, H, N, seed):
    """Random coordinates, a fifth of the slots dead, more agents than a third of the cells: dead slots and shared cells."""
    medium, agents = _world(W, H, N, np.random.RandomState(seed))
    return die.Env.from_numpy(medium, agents, device=DEV, sort_every=0)


def _occupancy(env):
    """The device's own record of who stands where now, as a host (W, H) bool array — and the model's, which it must equal."""
    occ = functional.signal_record(env._get_current_obs).occupied.cpu().numpy() > 0
    assert np.array_equal(occ, SM.occupancy_of(env.medium.W, env.medium.H, env.agents.to_numpy()))
    return occ


def _host_record(env):
    rec = functional.memory_record(env._get_current_obs)
    return rec.cell.cpu().numpy().copy(), rec.win.cpu().numpy().copy()


def _model(ag, frames, occs, sig0, loss_of, records=None, mem0=None, world=None, chem0=None, detach_at=()):
    """The float64 loop on the device's data: ([d loss / d weight per layer], d loss / d sig0, the loop's tensors)."""
    ws = [torch.tensor(k.weight.detach().cpu().double().numpy(), requires_grad=True) for k in ag.model.conv_layers()]
    s0 = torch.tensor(np.asarray(sig0, dtype=np.float64), requires_grad=True)
    m0 = None if mem0 is None else torch.tensor(np.asarray(mem0, dtype=np.float64))
    c0 = None if chem0 is None else torch.tensor(np.asarray(chem0, dtype=np.float64))
    out = SG.unroll(ws, 'circular', 'tanh', frames, occs, s0, ag.signal_constants, ag.action_coefs, records, m0, 'agents' in ag.obs_channels,
                    c0, world, detach_at)
    loss_of(out, lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)).backward()
    zero = lambda t: np.zeros(tuple(t.shape))
    return [zero(w) if w.grad is None else w.grad.numpy() for w in ws], zero(s0) if s0.grad is None else s0.grad.numpy(), out


# ---------------------------------------------------------------------------------------------------- 4. the same as forward
@pytest.mark.parametrize('seeded', [False, True], ids=['no mask', 'seeded mask'])
@pytest.mark.parametrize('M', [0, 2], ids=['no memory', 'memory'])
@pytest.mark.parametrize('W,H', [(13, 10), (24, 68)])
def test_signalling_action_is_forward_bit_for_bit(W, H, M, seeded, links=3, before=None):
    """13 x 10: H % 4 != 0, the tile kernel; 24 x 68: the row kernel, past the wide layer's 16 x 64 tile in both axes.
    (`links`, `before` — a callable of the two fresh worlds: tests/test_gpu_epoch_wrap.py runs the same checks across the epoch wrap.)"""
    K = 2
    kw = dict(p=0.25, dropout_seed=5) if seeded else {}
    plain_env, diff_env = _env(W, H), _env(W, H)
    plain = _agent(K, M, **kw)
    diff = _twin(plain, K=K, M=M, **kw)
    _same_state(_state(plain_env), _state(diff_env))
    if before is not None:
        before(plain_env, diff_env)
    signals = memory = None
    for t in range(links):
        obs_p, obs_d = plain_env._get_current_obs, diff_env._get_current_obs
        act = plain.forward(obs_p)
        action, signals, memory = diff.signalling_action(obs_d, signals, memory)
        N = obs_p[0].N
        assert action.shape == (3, N) and signals.shape == (K, W, H) and action.dtype == signals.dtype == torch.float32
        assert action.grad_fn is not None and signals.grad_fn is not None
        assert np.array_equal(_bits(act.data[:, :N]), _bits(action.detach())), t
        assert np.array_equal(_bits(plain.signals), _bits(signals.detach())), t
        assert np.array_equal(_bits(diff.signals), _bits(signals.detach())) and diff.signals.data_ptr() != signals.data_ptr(), t
        if M:
            assert memory.shape == (M, N) and memory.grad_fn is not None
            assert np.array_equal(_bits(plain.memory), _bits(memory.detach())), t
            assert np.array_equal(_bits(diff.memory), _bits(memory.detach())) and diff.memory.data_ptr() != memory.data_ptr(), t
        else:
            assert memory is None and diff.memory is None
        assert plain.dropout_step == diff.dropout_step == (t + 1 if seeded else 0)
        assert np.array_equal(_bits(plain._sense_output), _bits(diff._sense_output))
        plain_env.step(act)
        _step_with(diff_env, action)
        _same_state(_state(plain_env), _state(diff_env))
    assert float(signals.detach().abs().max()) > 0 and float(plain_env.medium.chem.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 5., 6. BPTT
def _bptt(loss_on_signals=True, detach=False, T=3, M=0, shape=(13, 10), before=None):
    """Three rounds on 13 x 10 chained through signals_next from a leaf, the world stepped by the detached actions between them.
    `M`: memory channels besides, chained from blank memory through memory_next.  `before`: a callable of (env, agent) run on the
    fresh world first (tests/test_gpu_epoch_wrap.py: real steps up to the epoch wrap)."""
    (W, H), K = shape, 2
    env, ag = _crowded_env(W, H, 60 * W * H // 130, seed=21), _agent(K, M)
    if before is not None:
        before(env, ag)
    N = env.agents.N
    rs = np.random.RandomState(4)
    u, v = rs.standard_normal((3, N)), rs.standard_normal((K, W, H))
    sig0 = (rs.uniform(-1, 1, (K, W, H)) * (rs.rand(K, W, H) < 0.6)).astype(np.float32)
    leaf = torch.from_numpy(sig0).to(DEV).requires_grad_(True)
    signals, frames, occs, alive, records = leaf, [], [], [], []
    memory = torch.zeros((M, N), dtype=torch.float32, device=DEV) if M else None
    for t in range(T):
        frames.append(_frame(env, ag))
        occs.append(_occupancy(env))
        if M:
            records.append(_host_record(env))
        alive.append(int((env.agents.to_numpy()[2] > 0).sum()))
        action, signals, memory = ag.signalling_action(env._get_current_obs, signals.detach() if detach and t > 0 else signals, memory)
        if t < T - 1:
            _step_with(env, action)
    assert all(n < N for n in alive)                                              # dead slots in every round …
    assert all(0 < int(o.sum()) < n for o, n in zip(occs, alive))                 # … and cells that several alive agents share
    ud, vd = (torch.as_tensor(a, dtype=torch.float32, device=DEV) for a in (u, v))
    loss = (ud * action).sum() + ((vd * signals).sum() if loss_on_signals else 0.)
    loss.backward()

    def loss_of(out, as_t):
        return (as_t(u) * out['actions'][-1]).sum() + ((as_t(v) * out['signals'][-1]).sum() if loss_on_signals else 0.)

    kw = dict(records=records, mem0=np.zeros((M, N))) if M else {}
    ref_w, ref_s, out = _model(ag, frames, occs, sig0, loss_of, detach_at=range(1, T) if detach else (), **kw)
    return ag, _device_grads(ag), ref_w, leaf, ref_s, (action, signals, out)


def test_bptt_gradients_match_the_float64_loop():
    ag, got, ref, leaf, ref_s, (action, signals, out) = _bptt()
    fwd = max(MG.rel_err(action.detach().cpu().numpy(), out['actions'][-1].detach().numpy()),
              MG.rel_err(signals.detach().cpu().numpy(), out['signals'][-1].detach().numpy()))
    err = _errors(got + [leaf.grad.cpu().numpy()], ref + [ref_s])
    print('bptt 13x10 T=3: device', ' '.join(f'{e:.3e}' for e in err), f'(of max|grad_f64| per layer, then d loss / d signals0; ceiling '
          f'{CEILING:.0e}); forward apart by {fwd:.2e}')
    assert fwd <= 1e-5                                                            # the model followed the same trajectory
    assert np.abs(ref_s).max() > 0 and all(e <= CEILING for e in err), err


def test_the_gradient_goes_through_the_field():
    # the loss is on the last action alone: the last layer's rows 3 .. 3 + K - 1, which produce emissions, are reached through the field only
    K = 2
    ag, got, ref, leaf, ref_s, _ = _bptt(loss_on_signals=False)
    rows = got[-1][3:3 + K]
    assert np.abs(rows).max() > 0 and np.abs(ref[-1][3:3 + K]).max() > 0
    err = _errors(got + [rows, leaf.grad.cpu().numpy()], ref + [ref[-1][3:3 + K], ref_s])
    print('through the field: device', ' '.join(f'{e:.3e}' for e in err), f'(layers, the emission rows, d loss / d signals0; ceiling {CEILING:.0e})')
    assert all(e <= CEILING for e in err), err
    # signals_next.detach() handed on instead: nothing reaches those rows, on the device and in the model
    ag, got, ref, _, _, _ = _bptt(loss_on_signals=False, detach=True)
    assert not got[-1][3:3 + K].any() and not ref[-1][3:3 + K].any() and np.abs(got[-1][:3]).max() > 0
    assert all(e <= CEILING for e in _errors(got, ref))


# ---------------------------------------------------------------------------------------------------- 7. memory and the world
def _through_the_world(T=2, before=None):
    """T links of signalling_action + differentiable_step on 16 x 12 from a blank field and blank memory, a loss on the last chem
    plane and the last field: (forward distance from the float64 loop, per-layer errors, the device's gradients, the loop's).
    `before`: a callable of (env, agent) run on the fresh world first (tests/test_gpu_epoch_wrap.py)."""
    W, H, sigma, K, M = 16, 12, 0.8, 2, 2
    env = _env(W, H, diffuse_sigma=sigma, rate_decay_chem=F.DECAY, diffuse_mode='wrap')
    ag = _agent(K, M)
    if before is not None:
        before(env, ag)
    N = env.agents.N
    rs = np.random.RandomState(6)
    cvec, svec = rs.standard_normal((W, H)), rs.standard_normal((K, W, H))
    chem0 = env.differentiable_chem().cpu().numpy().copy()
    frames, occs, records, cells, signals, memory = [], [], [], [], None, None
    for t in range(T):
        frames.append(_frame(env, ag))
        occs.append(_occupancy(env))
        records.append(_host_record(env))
        action, signals, memory = ag.signalling_action(env._get_current_obs, signals, memory)
        env.differentiable_step(action)
        cells.append(env.differentiable_chem().grad_fn.saved_tensors[0].cpu().numpy().copy())
    node = env.differentiable_chem()
    loss = (torch.as_tensor(cvec, dtype=torch.float32, device=DEV) * node).sum() + (torch.as_tensor(svec, dtype=torch.float32, device=DEV) * signals).sum()
    chem_T, sig_T = node.detach().cpu().numpy().copy(), signals.detach().cpu().numpy().copy()
    loss.backward()
    got = _device_grads(ag)

    def loss_of(out, as_t):
        return (as_t(cvec) * out['chem']).sum() + (as_t(svec) * out['signals'][-1]).sum()

    kw = dict(records=records, mem0=np.zeros((M, N)), world=dict(cells=cells, sigma=sigma, decay=F.DECAY), chem0=chem0)
    ref, _, out = _model(ag, frames, occs, np.zeros((K, W, H)), loss_of, **kw)
    fwd = max(MG.rel_err(chem_T, out['chem'].detach().numpy()), MG.rel_err(sig_T, out['signals'][-1].detach().numpy()))
    return fwd, _errors(got, ref), got, ref


def test_gradients_through_the_field_the_memory_and_the_world():
    K = 2
    fwd, err, got, ref = _through_the_world()
    print(f'field, memory and world 16x12 T=2: device', ' '.join(f'{e:.3e}' for e in err), f'(ceiling {CEILING:.0e}); forward apart by {fwd:.2e}')
    assert fwd <= 1e-4 and all(e <= CEILING for e in err), (fwd, err)
    assert np.abs(ref[-1][3:3 + K]).max() > 0 and MG.rel_err(got[-1][3:3 + K], ref[-1][3:3 + K]) <= CEILING
    assert np.abs(ref[-1][3 + K:]).max() > 0 and MG.rel_err(got[-1][3 + K:], ref[-1][3 + K:]) <= CEILING


# ---------------------------------------------------------------------------------------------------- 8. the record carries the graph
def _two_links(move_on):
    """Two links on a world whose alive agents stand on cells of their own and do not move (scale 0): no cell ever receives two
    terms, so the read-out's atomics are out of the picture and the gradients are a function of the graph alone."""
    W, H, K = 13, 10, 2
    medium, agents = F.plain_world(W, H, np.random.RandomState(2))
    env = die.Env.from_numpy(medium, agents, device=DEV)
    ag = _agent(K, scale=0.0)
    rs = np.random.RandomState(8)
    N = env.agents.N
    u, v = (torch.as_tensor(a, dtype=torch.float32, device=DEV) for a in (rs.standard_normal((3, N)), rs.standard_normal((K, W, H))))
    signals, loss = None, 0.
    for t in range(2):
        assert int(_occupancy(env).sum()) == int((env.agents.to_numpy()[2] > 0).sum())      # nobody shares a cell
        action, signals, _ = ag.signalling_action(env._get_current_obs, signals)
        loss = loss + (u * action).sum()
        _step_with(env, action)
    loss = loss + (v * signals).sum()
    if move_on:                                                                   # the world goes on, the storage is re-sorted, the field blanked
        for _ in range(2):
            env.step(ag.forward(env._get_current_obs))
        env.sort_agents()
        ag.reset_signals()
        assert not ag.signals.any()
    loss.backward()
    return [MM.bits(g) for g in _device_grads(ag)]


def test_backward_after_the_world_moved_on_gives_the_same_bits():
    at_once, again, later = _two_links(False), _two_links(False), _two_links(True)
    assert all(g.any() for g in at_once)
    assert all(np.array_equal(a, b) for a, b in zip(at_once, again))              # two runs: the same bits
    assert all(np.array_equal(a, b) for a, b in zip(at_once, later))              # the record, not the world, drives the backward


# ---------------------------------------------------------------------------------------------------- 9. the refusals
REFUSALS = {
    # what: (agent arguments, the error, a word of its message)
    'no signal channels': (dict(K=0, M=2), ValueError, 'recurrent_action'),
    'stock': (dict(with_stock_channel=True), NotImplementedError, 'stock'),
    'decomposed': ({}, NotImplementedError, 'decomposed'),
    'fp16': ({}, NotImplementedError, 'fp32'),
    'reflect': (dict(boundary='reflect'), NotImplementedError, 'reflect'),
    'replicate': (dict(boundary='replicate'), NotImplementedError, 'replicate'),
    'signals of another shape': ({}, ValueError, 'signals'),
    'signals of another dtype': ({}, ValueError, 'signals'),
    'signals on another device': ({}, ValueError, 'signals'),
    'signals no tensor': ({}, ValueError, 'signals'),
    'memory of another N': ({}, ValueError, 'memory'),
    'memory of another dtype': ({}, ValueError, 'memory'),
    'memory on another device': ({}, ValueError, 'memory'),
    'memory without memory channels': (dict(M=0), ValueError, 'memory'),
    'a field bound to another shape': ({}, ValueError, 'reset_signals'),
}


@pytest.mark.parametrize('what', list(REFUSALS))
def test_refusals_on_the_device_leave_everything_alone(what):
    W, H, K = 13, 10, 2
    extra, error, needle = REFUSALS[what]
    medium, agents = F.plain_world(W, H, np.random.RandomState(2))
    env = die.Env.from_numpy(medium, agents, device=DEV, field_dtype=torch.float16 if what == 'fp16' else torch.float32)
    ag = _agent(**dict(dict(K=K, M=2, p=0.25, dropout_seed=3), **extra))
    K, M, N = ag.signal_channels, ag.memory_channels, env.agents.N
    bound_shape = (K, W, H + 4) if what == 'a field bound to another shape' else (K, W, H)
    field = torch.full(bound_shape, 0.25, dtype=torch.float32, device=DEV) if K else None
    held = torch.full((M, N), 0.5, dtype=torch.float32, device=DEV) if M else None
    ag.signals, ag._signals_rebind, ag.memory, ag._memory_rebind, ag.dropout_step = field, False, held, False, 4
    if what == 'decomposed':
        env.medium.world = (2 * W, 2 * H, 0, 0)
    signals = {'signals of another shape': torch.zeros((K, W, H + 1), device=DEV), 'signals of another dtype': torch.zeros((K, W, H), dtype=torch.float64, device=DEV),
               'signals on another device': torch.zeros((K, W, H)), 'signals no tensor': np.zeros((K, W, H), dtype=np.float32)}.get(what)
    memory = {'memory of another N': torch.zeros((2, N + 1), device=DEV), 'memory of another dtype': torch.zeros((2, N), dtype=torch.float64, device=DEV),
              'memory on another device': torch.zeros((2, N)), 'memory without memory channels': torch.zeros((2, N), device=DEV)}.get(what)
    before = _state(env)
    with pytest.raises(error, match=needle):
        ag.signalling_action(env._get_current_obs, signals, memory)
    env.medium.world = None
    _same_state(before, _state(env))
    assert ag.dropout_step == 4 and ag.signals is field and ag.memory is held and ag._sense_output is None
    assert (field is None or bool((field == 0.25).all())) and (held is None or bool((held == 0.5).all()))


def test_the_other_differentiable_calls_keep_refusing_a_signalling_agent():
    W, H = 13, 10
    medium, agents = F.plain_world(W, H, np.random.RandomState(2))
    env = die.Env.from_numpy(medium, agents, device=DEV)
    ag = _agent(2, 2)
    for call in (lambda: ag.differentiable_sense(env.medium), lambda: ag.differentiable_action(env._get_current_obs),
                 lambda: ag.model.forward_device(torch.zeros((7, W, H), device=DEV)), lambda: ag.recurrent_action(env._get_current_obs)):
        with pytest.raises(NotImplementedError, match='signal'):
            call()
    assert ag.signals is None and ag.memory is None and ag.dropout_step == 0


# ---------------------------------------------------------------------------------------------------- 10. training
def test_ten_adam_steps_of_the_example_with_signal_channels():
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    try:
        import recurrent_agent
    finally:
        sys.path.pop(0)
    student, losses = recurrent_agent.train(16, 2, 3, 0, 10, log=lambda *_: None, signal_channels=2)
    print('recurrent_agent 16x16 T=3 K=2 M=2, ten Adam steps:', ' '.join(f'{v:.4f}' for v in losses))
    assert len(losses) == 10 and np.isfinite(losses).all() and losses[-1] < losses[0]     # (0.139 -> 0.049 at these defaults, untuned)
    rows = student.model.conv_layers()[-1].weight.grad[3:5]                       # the emission rows, after the last backward
    assert bool(torch.isfinite(rows).all()) and float(rows.abs().max()) > 0
    assert student.signals is not None and float(student.signals.abs().max()) > 0
