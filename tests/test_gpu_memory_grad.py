"""Gradients through memory channels on the device (die_memory_grad.hip; die_amd.functional.memory_record / memory_planes /
gather_memory; NeuralAutomataAgent.recurrent_action): the record and the two adjoints against tests/memory_grad_model.py word for
word, `recurrent_action` against `forward` bit for bit on twin worlds, backpropagation through time against the model's float64
loop fed the device's own records, the gradient's way through the memory (and its absence behind a detach), through the world
(Env.differentiable_step), the refusals, and ten Adam steps of examples/recurrent_agent.py.

The ceiling of every gradient comparison is 1e-4 of max|reference| per array, the project's backward tolerance
(tests/test_gpu_field_step_grad.py GRAD_TOL): tests/test_memory_grad_cpu.py holds a plain fp32 evaluation of the same loop below
1e-5."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib, functional
from die_amd.device_array import DeviceAction, stream_ptr, unpermute
from tests import field_step_adjoint_model as F
from tests import memory_grad_model as MG
from tests import memory_model as MM
from tests import stock_plane_model as S

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CEILING = 1e-4
TAIL = 64
NAN_BITS = MM.bits(np.float32('nan'))
SENT_I = 0x5A5A5A5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sp():
    return stream_ptr(torch.device(DEV))


def _medium(W, H):
    return _lib.Medium(W, H, _lib.DIE_F32, 1, None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, None)


def _nan(n):
    return torch.full((n + TAIL,), float('nan'), dtype=torch.float32, device=DEV)


def _bits(t):
    return MM.bits(t.cpu().numpy())


# ---------------------------------------------------------------------------------------------------- 1. the record
def _record_on_device(env):
    """die_memory_cells on a standing plane built here: (cell, win) host arrays, the 64-word guard bands checked."""
    A, Md = env.agents, env.medium
    N = A.N
    standing = torch.zeros((Md.W, Md.H), dtype=torch.int64, device=DEV)
    out = torch.full((2, N + TAIL), SENT_I, dtype=torch.int32, device=DEV)
    m, a = Md.c_struct(need_owner=False), A.c_struct()
    _lib.check(_lib.lib.die_stock_plane(C.byref(m), C.byref(a), Md.epoch, standing.data_ptr(), _sp()), 'die_stock_plane')
    _lib.check(_lib.lib.die_memory_cells(C.byref(m), C.byref(a), standing.data_ptr(), Md.epoch, out[0].data_ptr(), out[1].data_ptr(), _sp()),
               'die_memory_cells')
    host = out.cpu().numpy()
    assert (host[:, N:] == SENT_I).all()
    return host[0, :N], host[1, :N]


def _crafted_env(**kw):
    medium, agents = MG.crafted_world()
    return die.Env.from_numpy(medium, agents, device=DEV, sort_every=0, **kw)


@pytest.mark.parametrize('world', ['crafted', (13, 10), (16, 12)], ids=str)
def test_memory_cells_against_the_model(world):
    if world == 'crafted':
        env = _crafted_env()
    else:
        env = die.Env(world, die.Dynamics(init_agent_ratio=0.3), seed=7, device=DEV, sort_every=0)
    W, H = env.medium.W, env.medium.H
    want_cell, want_win = MG.record_of(W, H, env.agents.to_numpy())
    assert env.agents.slot is None
    cell, win = _record_on_device(env)
    assert np.array_equal(cell, want_cell) and np.array_equal(win, want_win)
    assert (win >= 0).sum() > 0 and np.unique(win[win >= 0]).size == (win >= 0).sum()        # one winner a cell
    if world == 'crafted':
        assert cell.tolist() == [21, 13, -1, 6, 13, -1, 29, 21, 17, 13, 4, 25] and win.tolist() == [-1, -1, -1, 6, -1, -1, 29, 21, 17, 13, 4, 25]
    env.sort_agents()                                                # a slot array: the record is by slot id all the same
    A = env.agents
    assert np.array_equal(np.sort(A.slot.cpu().numpy()), np.arange(A.N))
    # (a world this small is one sort bucket and keeps its order: shuffle the storage by hand, so that storage order != slot order)
    perm = torch.from_numpy(np.random.RandomState(1).permutation(A.N)).to(DEV)
    A.x, A.y, A.alive, A.agent_food, A.slot = (t[perm].contiguous() for t in (A.x, A.y, A.alive, A.agent_food, A.slot))
    assert not np.array_equal(A.slot.cpu().numpy(), np.arange(A.N))
    cell, win = _record_on_device(env)
    assert np.array_equal(cell, want_cell) and np.array_equal(win, want_win)
    # the functional call gives the same record, from a standing plane of its own
    rec = functional.memory_record(env._get_current_obs)
    assert (rec.W, rec.H, rec.N) == (W, H, env.agents.N) and rec.cell.dtype == rec.win.dtype == torch.int32
    assert np.array_equal(rec.cell.cpu().numpy(), want_cell) and np.array_equal(rec.win.cpu().numpy(), want_win)


def test_memory_cells_of_no_slot_writes_nothing():
    W, H = 13, 10
    out = torch.full((2, TAIL), SENT_I, dtype=torch.int32, device=DEV)
    standing = torch.zeros((W, H), dtype=torch.int64, device=DEV)
    a = _lib.Agents(0, None, None, None, None, None)
    assert _lib.lib.die_memory_cells(C.byref(_medium(W, H)), C.byref(a), standing.data_ptr(), 3, out[0].data_ptr(), out[1].data_ptr(), _sp()) == 0
    assert (out.cpu().numpy() == SENT_I).all()


# ---------------------------------------------------------------------------------------------------- 2., 3. the adjoints
def _index_world(kind):
    """(W, H, N, cell, win): records made up on the host (the two kernels are index-only).  'crafted': the 6 x 5 world, three alive
    slots on one cell.  'crowded': 24 x 68, 300 slots (two blocks), every seventh dead, three slots on one cell and pairs on forty.
    'pairs': the same without the triple — no cell holds more than two alive slots."""
    if kind == 'crafted':
        W, H = MG.CRAFTED
        _, agents = MG.crafted_world()
        cell, win = MG.record(W, H, MG.label_words(np.rint(agents[0] * (W - 1)), W), MG.label_words(np.rint(agents[1] * (H - 1)), H), agents[2] > 0)
        return W, H, 12, cell, win
    W, H, N = 24, 68, 300
    rs = np.random.RandomState(17)
    cells = rs.choice(W * H, N, replace=False)
    cells[1:80:2] = cells[0:80:2]                                    # forty pairs
    alive = np.arange(N) % 7 != 3
    if kind == 'crowded':
        cells[[100, 200]] = cells[0]                                 # (slot 1 shares it too: four, three or more of them alive)
    cell = np.where(alive, cells, -1).astype(np.int32)
    win = np.full(N, -1, dtype=np.int32)
    for i in np.flatnonzero(alive):                                  # ascending slot id: the last writer wins its cell
        win[cell == cell[i]] = -1
        win[i] = cell[i]
    return W, H, N, cell, win


@pytest.mark.parametrize('Mc', [1, 8])
@pytest.mark.parametrize('kind', ['crafted', 'crowded'])
def test_memory_planes_backward_is_the_model_bit_for_bit(kind, Mc):
    W, H, N, cell, win = _index_world(kind)
    win = win.copy()
    dead = np.flatnonzero(win < 0)
    win[dead[0]], win[dead[1]] = W * H, 2 ** 31 - 1                  # at or beyond W * H counts as negative
    rs = np.random.RandomState(Mc)
    ps, row = W * H + 6, N + 5
    gp = rs.standard_normal((Mc, ps)).astype(np.float32)
    won = win[(win >= 0) & (win < W * H)]
    gp[0, won[0]], gp[0, won[1]] = np.float32(-0.0), np.float32(1e-41)
    gp_bits = gp.view(np.uint32)
    gp_bits[Mc - 1, won[2]] = 0x7FC12345                             # a NaN payload
    planes = torch.from_numpy(gp).to(DEV)
    out = _nan(Mc * row)
    twin = torch.from_numpy(win).to(DEV)
    _lib.check(_lib.lib.die_memory_planes_backward(W, H, Mc, N, twin.data_ptr(), planes.data_ptr(), ps, out.data_ptr(), row, _sp()),
               'die_memory_planes_backward')
    got = _bits(out)
    want = MM.bits(MG.expand_adjoint(W, H, win, gp[:, :W * H].reshape(Mc, W, H), np.float32))
    rows = got[:Mc * row].reshape(Mc, row)
    assert np.array_equal(rows[:, :N], want)                         # a gather: bit for bit
    assert (rows[:, N:] == NAN_BITS).all() and (got[Mc * row:] == NAN_BITS).all()        # the gaps and the guard band: untouched
    assert not rows[:, :N][:, ~((win >= 0) & (win < W * H))].any()                       # losers, dead slots, out-of-plane: +0
    ids = np.flatnonzero((win >= 0) & (win < W * H))
    assert rows[0, ids[0]] == 0x80000000 and rows[0, ids[1]] == MM.bits(np.float32(1e-41)) and rows[Mc - 1, ids[2]] == 0x7FC12345


@pytest.mark.parametrize('Mc', [1, 8])
@pytest.mark.parametrize('kind', ['crafted', 'crowded', 'pairs'])
def test_gather_memory_backward_against_the_model(kind, Mc):
    W, H, N, cell, _ = _index_world(kind)
    rs = np.random.RandomState(10 + Mc)
    ps, row = W * H + 6, N + 5
    gm = rs.standard_normal((Mc, row)).astype(np.float32)
    gm[0, np.flatnonzero(cell >= 0)[5]] = 0.0                        # a zero term is skipped
    tgm, tcell = torch.from_numpy(gm).to(DEV), torch.from_numpy(cell).to(DEV)
    runs = []
    for _ in range(2):
        out = _nan(Mc * ps)
        _lib.check(_lib.lib.die_gather_memory_backward(W, H, Mc, N, tcell.data_ptr(), tgm.data_ptr(), row, out.data_ptr(), ps, _sp()),
                   'die_gather_memory_backward')
        runs.append(out)
    torch.cuda.synchronize()
    got = [r.cpu().numpy() for r in runs]
    for g in got:
        planes = g[:Mc * ps].reshape(Mc, ps)
        assert not np.isnan(planes[:, :W * H]).any()                 # fully written: nothing left of the pre-fill
        assert (MM.bits(planes[:, W * H:]) == NAN_BITS).all() and (MM.bits(g[Mc * ps:]) == NAN_BITS).all()
    planes = got[0][:Mc * ps].reshape(Mc, ps)[:, :W * H].reshape(Mc, W, H)
    ref = MG.gather_adjoint(W, H, cell, gm[:, :N].astype(np.float64))
    err = MG.rel_err(planes, ref)
    print(f'gather_memory_backward {kind} M={Mc}: {err:.3e} of max|ref| (ceiling {CEILING:.0e})')
    assert err <= CEILING
    crowd = np.bincount(cell[cell >= 0]).max()
    if kind == 'pairs':
        assert crowd == 2
        assert np.array_equal(MM.bits(planes), MM.bits(MG.gather_adjoint(W, H, cell, gm[:, :N], np.float32)))
        assert np.array_equal(MM.bits(got[0]), MM.bits(got[1]))      # two addends commute: the same bits on every run
    else:
        assert crowd >= 3


# ---------------------------------------------------------------------------------------------------- the agents and worlds
def _agent(seed=0, p=0.0, dropout_seed=None, with_agent_channel=True, scale=F.COEFS[0], **kw):
    torch.manual_seed(seed)
    kw.setdefault('memory_channels', 2)
    ag = die.NeuralAutomataAgent(kernel_sizes=(3, 3), hidden_channels=8, hidden_activation='tanh', scale=scale, deposit=F.COEFS[2],
                                 p_agent_dropout=p, dropout_seed=dropout_seed, with_agent_channel=with_agent_channel, **kw)
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


def _state(env):
    """Everything a step leaves, as host arrays of raw words, the agent arrays in slot order."""
    Md, A = env.medium, env.agents
    out = dict(chem=Md.chem, food=Md.food, owner=Md.owner)
    out.update({k: unpermute(getattr(A, k), A.slot) for k in ('x', 'y', 'alive', 'agent_food')})
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    out['epoch'] = Md.epoch
    return out


def _same_state(a, b):
    for k in a:
        assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)) if isinstance(a[k], np.ndarray) else a[k] == b[k], k


def _step_with(env, action):
    act = DeviceAction(env.agents.N, env.device, env.agents.slot)
    act.data = action.detach().contiguous()
    return env.step(act)


def _frame(env, ag, p=0.0, seed=None):
    """What the model takes as data of the coming round: the planes the world supplies, the slots' cells in array order, the mask."""
    W, H = env.medium.W, env.medium.H
    m = env.medium.to_numpy()
    cx, cy = S.cell(env.agents.x.cpu().numpy().view(np.uint32), W), S.cell(env.agents.y.cpu().numpy().view(np.uint32), H)
    mask = MG.mask_of(seed, ag.dropout_step, W, H, p).astype(np.float64) if seed is not None and p > 0 else None
    return dict(occ=m[0], food=m[1], chem=m[2], cx=cx, cy=cy, mask=mask)


def _host_record(env):
    rec = functional.memory_record(env._get_current_obs)
    return rec.cell.cpu().numpy().copy(), rec.win.cpu().numpy().copy()


def _model(ag, frames, records, mem0, loss_of, world=None, chem0=None, detach_at=()):
    """The float64 loop on the device's data: ([d loss / d weight per layer], d loss / d mem0, the loop's tensors)."""
    ws = [torch.tensor(k.weight.detach().cpu().double().numpy(), requires_grad=True) for k in ag.model.conv_layers()]
    m0 = torch.tensor(np.asarray(mem0, dtype=np.float64), requires_grad=True)
    c0 = None if chem0 is None else torch.tensor(np.asarray(chem0, dtype=np.float64))
    out = MG.unroll(ws, 'circular', 'tanh', frames, records, m0, ag.action_coefs, 'agents' in ag.obs_channels, c0, world, detach_at)
    loss_of(out, lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)).backward()
    zero = lambda t: np.zeros(tuple(t.shape))
    return [zero(w) if w.grad is None else w.grad.numpy() for w in ws], zero(m0) if m0.grad is None else m0.grad.numpy(), out


def _device_grads(ag):
    torch.cuda.synchronize()
    return [q.grad.detach().cpu().numpy().copy() for q in ag.model.parameters()]


def _errors(got, ref):
    assert [g.shape for g in got] == [r.shape for r in ref]
    return [MG.rel_err(g, r) for g, r in zip(got, ref)]


# ---------------------------------------------------------------------------------------------------- 4. the same as forward
@pytest.mark.parametrize('with_agents', [True, False], ids=['agents channel', 'no agents channel'])
@pytest.mark.parametrize('seeded', [False, True], ids=['no mask', 'seeded mask'])
@pytest.mark.parametrize('W,H', [(13, 10), (24, 68)])
def test_recurrent_action_is_forward_bit_for_bit(W, H, seeded, with_agents, links=3, before=None):
    """13 x 10: H % 4 != 0, the expand's scalar path; 24 x 68: H % 4 == 0, past the wide layer's 16 x 64 tile in both axes.
    (`links`, `before` — a callable of the two fresh worlds: tests/test_gpu_epoch_wrap.py runs the same checks across the epoch wrap.)"""
    kw = dict(p=0.25, dropout_seed=5) if seeded else {}
    plain_env, diff_env = _env(W, H), _env(W, H)
    plain = _agent(with_agent_channel=with_agents, **kw)
    diff = _twin(plain, with_agent_channel=with_agents, **kw)
    _same_state(_state(plain_env), _state(diff_env))
    if before is not None:
        before(plain_env, diff_env)
    memory = None
    for t in range(links):
        obs_p, obs_d = plain_env._get_current_obs, diff_env._get_current_obs
        act = plain.forward(obs_p)
        action, memory = diff.recurrent_action(obs_d, memory)
        N = obs_p[0].N
        assert action.shape == (3, N) and memory.shape == (2, N) and action.dtype == memory.dtype == torch.float32
        assert action.grad_fn is not None and memory.grad_fn is not None
        assert np.array_equal(_bits(act.data[:, :N]), _bits(action.detach())), t
        assert np.array_equal(_bits(plain.memory), _bits(memory.detach())), t
        assert np.array_equal(_bits(diff.memory), _bits(memory.detach())) and diff.memory.data_ptr() != memory.data_ptr(), t
        assert plain.dropout_step == diff.dropout_step == (t + 1 if seeded else 0)
        assert np.array_equal(_bits(plain._sense_output), _bits(diff._sense_output))
        plain_env.step(act)
        _step_with(diff_env, action)
        _same_state(_state(plain_env), _state(diff_env))
    assert float(memory.detach().abs().max()) > 0 and float(plain_env.medium.chem.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 5. – 7. BPTT
def _bptt(seeded, loss_on_memory=True, detach=False, leaf=False, T=3, shape=(13, 10), before=None):
    """Three rounds on 13 x 10 chained through memory_next, the world stepped by the detached actions between them.  `before`: a
    callable of (env, agent) run on the fresh world first (tests/test_gpu_epoch_wrap.py: real steps up to the epoch wrap)."""
    W, H = shape
    p, seed = (0.25, 5) if seeded else (0.0, None)
    env, ag = _env(W, H), _agent(p=p, dropout_seed=seed)
    if before is not None:
        before(env, ag)
    N = env.agents.N
    rs = np.random.RandomState(4)
    u, v = rs.standard_normal((3, N)), rs.standard_normal((2, N))
    mem0 = rs.standard_normal((2, N)).astype(np.float32)
    memory = torch.from_numpy(mem0).to(DEV).requires_grad_(leaf)
    leaf_memory, frames, records = memory, [], []
    for t in range(T):
        frames.append(_frame(env, ag, p, seed))
        records.append(_host_record(env))
        action, memory = ag.recurrent_action(env._get_current_obs, memory.detach() if detach and t > 0 else memory)
        if t < T - 1:
            _step_with(env, action)
    ud, vd = (torch.as_tensor(a, dtype=torch.float32, device=DEV) for a in (u, v))
    loss = (ud * action).sum() + ((vd * memory).sum() if loss_on_memory else 0.)
    loss.backward()

    def loss_of(out, as_t):
        return (as_t(u) * out['actions'][-1]).sum() + ((as_t(v) * out['memories'][-1]).sum() if loss_on_memory else 0.)

    ref_w, ref_m, out = _model(ag, frames, records, mem0, loss_of, detach_at=range(1, T) if detach else ())
    assert max(int((np.bincount(c[c >= 0]) > 1).sum()) for c, _ in records) > 0          # cells are shared on the way
    return ag, _device_grads(ag), ref_w, leaf_memory, ref_m, (action, memory, out)


@pytest.mark.parametrize('seeded', [False, True], ids=['no mask', 'seeded mask'])
def test_bptt_gradients_match_the_float64_loop(seeded):
    ag, got, ref, _, _, (action, memory, out) = _bptt(seeded)
    fwd = max(MG.rel_err(action.detach().cpu().numpy(), out['actions'][-1].detach().numpy()),
              MG.rel_err(memory.detach().cpu().numpy(), out['memories'][-1].detach().numpy()))
    err = _errors(got, ref)
    print(f'bptt 13x10 T=3 seeded={seeded}: device', ' '.join(f'{e:.3e}' for e in err), f'(of max|grad_f64| per layer; ceiling {CEILING:.0e}); '
          f'forward apart by {fwd:.2e}')
    assert fwd <= 1e-5                                               # the model followed the same trajectory
    assert all(e <= CEILING for e in err), err


def test_the_gradient_goes_through_the_memory():
    # the loss is on the last action alone: the last layer's rows 3.., which produce memory, are reached through the memory only
    ag, got, ref, leaf, ref_m, _ = _bptt(False, loss_on_memory=False, leaf=True)
    rows = got[-1][3:]
    assert np.abs(rows).max() > 0 and np.abs(ref[-1][3:]).max() > 0
    err = _errors([g for g in got] + [rows, leaf.grad.cpu().numpy()], [r for r in ref] + [ref[-1][3:], ref_m])
    print('through memory: device', ' '.join(f'{e:.3e}' for e in err), f'(layers, the memory rows, d loss / d memory; ceiling {CEILING:.0e})')
    assert all(e <= CEILING for e in err), err
    assert np.abs(ref_m).max() > 0
    # memory_next.detach() handed on instead: nothing reaches those rows
    ag, got, ref, _, _, _ = _bptt(False, loss_on_memory=False, detach=True)
    assert not got[-1][3:].any() and not ref[-1][3:].any() and np.abs(got[-1][:3]).max() > 0
    assert all(e <= CEILING for e in _errors(got, ref))


# ---------------------------------------------------------------------------------------------------- 8. through the world
def test_gradients_through_the_memory_and_the_world():
    W, H, T, sigma = 16, 12, 2, 0.8
    env = _env(W, H, diffuse_sigma=sigma, rate_decay_chem=F.DECAY, diffuse_mode='wrap')
    ag = _agent()
    N = env.agents.N
    rs = np.random.RandomState(6)
    cvec = rs.standard_normal((W, H))
    chem0 = env.differentiable_chem().cpu().numpy().copy()
    frames, records, cells, memory = [], [], [], None
    for t in range(T):
        frames.append(_frame(env, ag))
        records.append(_host_record(env))
        action, memory = ag.recurrent_action(env._get_current_obs, memory)
        env.differentiable_step(action)
        cells.append(env.differentiable_chem().grad_fn.saved_tensors[0].cpu().numpy().copy())
    node = env.differentiable_chem()
    loss = (torch.as_tensor(cvec, dtype=torch.float32, device=DEV) * node).sum()
    chem_T = node.detach().cpu().numpy().copy()
    for _ in range(2):                                               # the records are the graph's: the world may go on
        env.step(ag.forward(env._get_current_obs))
    env.sort_agents()
    loss.backward()
    got = _device_grads(ag)

    def loss_of(out, as_t):
        return (as_t(cvec) * out['chem']).sum()

    ref, _, out = _model(ag, frames, records, np.zeros((2, N)), loss_of, world=dict(cells=cells, sigma=sigma, decay=F.DECAY), chem0=chem0)
    chem_err = MG.rel_err(chem_T, out['chem'].detach().numpy())
    err = _errors(got, ref)
    print(f'through the world 16x12 T=2: device', ' '.join(f'{e:.3e}' for e in err), f'(ceiling {CEILING:.0e}); chem_T apart by {chem_err:.2e}')
    assert chem_err <= 1e-4 and all(e <= CEILING for e in err), (chem_err, err)
    # the rows that produce memory reach this loss through the memory AND the world only: a real share, gone behind a detach
    assert np.abs(ref[-1][3:]).max() > 0 and MG.rel_err(got[-1][3:], ref[-1][3:]) <= CEILING
    cut_m, _, _ = _model(ag, frames, records, np.zeros((2, N)), loss_of, world=dict(cells=cells, sigma=sigma, decay=F.DECAY), chem0=chem0,
                         detach_at=range(1, T))
    assert not cut_m[-1][3:].any()


# ---------------------------------------------------------------------------------------------------- 9. the refusals
@pytest.mark.parametrize('what', ['stock', 'fp16', 'reflect', 'wrong N'])
def test_refusals_on_the_device_leave_everything_alone(what):
    W, H = 13, 10
    medium, agents = F.plain_world(W, H, np.random.RandomState(2))
    env = die.Env.from_numpy(medium, agents, device=DEV, field_dtype=torch.float16 if what == 'fp16' else torch.float32)
    kw = dict(with_stock_channel=True) if what == 'stock' else dict(boundary='reflect') if what == 'reflect' else {}
    ag = _agent(p=0.25, dropout_seed=3, **kw)
    N = env.agents.N
    held = torch.full((2, N), 0.5, dtype=torch.float32, device=DEV)
    ag.memory, ag._memory_rebind, ag.dropout_step = held, False, 4
    before = _state(env)
    memory = torch.zeros((2, N + 1), device=DEV) if what == 'wrong N' else None
    with pytest.raises(ValueError if what == 'wrong N' else NotImplementedError):
        ag.recurrent_action(env._get_current_obs, memory)
    _same_state(before, _state(env))
    assert ag.dropout_step == 4 and ag.memory is held and bool((held == 0.5).all()) and ag._sense_output is None


# ---------------------------------------------------------------------------------------------------- 10. training
def test_ten_adam_steps_of_the_example_decrease_the_loss():
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    try:
        import recurrent_agent
    finally:
        sys.path.pop(0)
    student, losses = recurrent_agent.train(16, 2, 3, 0, 10, log=lambda *_: None)
    print('recurrent_agent 16x16 T=3, ten Adam steps:', ' '.join(f'{v:.4f}' for v in losses))
    assert len(losses) == 10 and np.isfinite(losses).all() and losses[-1] < losses[0]
    assert student.memory is not None and float(student.memory.abs().max()) > 0
