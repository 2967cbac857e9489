"""Heredity on the device (die_births.hip's record, die_heredity.hip; Env.births_record, NeuralAutomataAgent.inherit_memory, their
batched twins): the record, the in-place rule and its adjoint through the C ABI against tests/heredity_model.py word for word; a
slot that dies and is refilled within one step; batched replicas against their stand-alone Envs after every step; the explicit
call against the step's own; backpropagation through time across births against the model's float64 loop fed the device's own
records (ceiling: the project's backward tolerance, 1e-4 of max|reference| per array, tests/test_gpu_memory_grad.py CEILING — the
link adds copies and at most one add); the refusals; one PGPE generation."""
import ctypes as C

import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib, functional
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent
from die_amd.device_array import DeviceAction
from die_amd.search import PGPE
from tests import field_step_adjoint_model as F
from tests import heredity_model as HM
from tests import memory_grad_model as MG
from tests import memory_model as MM
from tests import stock_plane_model as S

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CEILING = 1e-4                      # tests/test_gpu_memory_grad.py CEILING
TAIL = 64
SENT_I = 0x5A5A5A5A
NAN_BITS = MM.bits(np.float32('nan'))
GRID_SLOTS = 256 * 256              # HEREDITY_MAX_GROUPS / BIRTH_RECORD_MAX_GROUPS workgroups of 256 threads: one trip of a grid
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
MODES = (('blank', 0.0), ('copy', 0.0), ('copy', 0.25))
SEED, STEP = 0xFEDCBA9876543210, 0x80000007


def _bits(t):
    return MM.bits(t.cpu().numpy())


def _patterns(n, rs):
    """name -> (alive, food): parents are alive with food above 0.5, free slots dead, the rest alive and poor."""
    k = np.arange(n)
    P, Fr, O = 1, 2, 0
    roles = {
        'no parent': np.where(k % 3 == 0, Fr, O),
        'no free slot': np.where(k % 3 == 0, O, P),
        'more parents than free slots': np.where(k % 4 == 3, Fr, P),
        'more free slots than parents': np.where(k % 4 == 3, P, Fr),
        'at random': rs.choice([P, Fr, O], n, p=[0.4, 0.4, 0.2]),
    }
    out = {}
    for name, role in roles.items():
        alive = (role != Fr).astype(np.uint8)
        food = np.where(role == P, rs.uniform(0.51, 30.0, n), np.where(role == O, rs.uniform(0.0, 0.5, n), 0.0)).astype(np.float32)
        out[name] = (alive, food)
    return out


def _batch(n, stride):
    return _lib.Batch(len(n), 0, 0, stride, 1, (C.c_int64 * 64)(*n))


def _pass_and_record(alive, food, n, stride=None):
    """The birth pass on device copies of R replicas' (alive, food) — rows of `stride` slots — then the record into guard-banded
    arrays: (parent_of, child_of) host arrays of shape (R, stride)."""
    R = len(n)
    stride = stride or max(n)
    pad = lambda rows, dt: torch.from_numpy(np.stack([np.r_[np.asarray(v, dtype=dt), np.zeros(stride - len(v), dtype=dt)] for v in rows])).to(DEV)
    al, fo = pad(alive, np.uint8), pad(food, np.float32)
    x, y = (torch.zeros((R, stride), dtype=torch.int32, device=DEV) for _ in range(2))
    need = _lib.lib.die_births_workspace_bytes(R, stride)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    a = _lib.Agents(stride, x.data_ptr(), y.data_ptr(), al.data_ptr(), fo.data_ptr(), None)
    p = _lib.Births(0.5, 0, 0.02, STEP, 0)
    b = _batch(n, stride)
    seeds = (C.c_uint64 * R)(*[SEED + r for r in range(R)])
    out = torch.full((2, R * stride + TAIL), SENT_I, dtype=torch.int32, device=DEV)
    if R == 1 and stride == n[0]:
        _lib.check(_lib.lib.die_agent_births(C.byref(a), C.byref(p), SEED, None, ws.data_ptr(), need, None), 'die_agent_births')
        _lib.check(_lib.lib.die_births_record(n[0], ws.data_ptr(), need, out[0].data_ptr(), out[1].data_ptr(), None), 'die_births_record')
    else:
        _lib.check(_lib.lib.die_agent_births_batch(C.byref(a), C.byref(b), C.byref(p), seeds, None, ws.data_ptr(), need, None), 'births_batch')
        _lib.check(_lib.lib.die_births_record_batch(C.byref(b), ws.data_ptr(), need, out[0].data_ptr(), out[1].data_ptr(), None), 'record_batch')
    host = out.cpu().numpy()
    assert (host[:, R * stride:] == SENT_I).all()
    return host[0, :R * stride].reshape(R, stride), host[1, :R * stride].reshape(R, stride)


def _inherit_on_device(mem, parent_of, mode, a, n, row):
    """die_memory_inherit on a guard-banded copy of the (M, row) array `mem`: the (M, row) words afterwards."""
    M = mem.shape[0]
    buf = torch.full((M * row + TAIL,), float('nan'), dtype=torch.float32, device=DEV)
    buf[:M * row] = torch.from_numpy(mem.reshape(-1)).to(DEV)
    par = torch.from_numpy(np.ascontiguousarray(parent_of[:n])).to(DEV)
    _lib.check(_lib.lib.die_memory_inherit(_lib.INHERIT_MODES[mode], a, M, n, par.data_ptr(), buf.data_ptr(), row, SEED, STEP, None),
               'die_memory_inherit')
    got = _bits(buf)
    assert (got[M * row:] == NAN_BITS).all()
    return got[:M * row].reshape(M, row)


def _backward_on_device(g, parent_of, child_of, mode, n, row):
    M = g.shape[0]
    out = torch.full((M * row + TAIL,), float('nan'), dtype=torch.float32, device=DEV)
    tg = torch.from_numpy(g).to(DEV)
    par, chi = (torch.from_numpy(np.ascontiguousarray(v[:n])).to(DEV) for v in (parent_of, child_of))
    _lib.check(_lib.lib.die_memory_inherit_backward(_lib.INHERIT_MODES[mode], M, n, par.data_ptr(), chi.data_ptr(), tg.data_ptr(), out.data_ptr(),
                                                    row, None), 'die_memory_inherit_backward')
    got = _bits(out)
    assert (got[M * row:] == NAN_BITS).all()
    return got[:M * row].reshape(M, row)


def _check_rule(n, alive, food, rs, Ms=(1, 4, 5, 8), tag=''):
    parent_of, child_of = _pass_and_record([alive], [food], [n])
    want_p, want_c = HM.record(alive, food, 0.5)
    assert np.array_equal(parent_of[0], want_p) and np.array_equal(child_of[0], want_c), (n, tag)
    row = n + 5                                                      # a row stride larger than N
    born = int((want_p >= 0).sum())
    for M in Ms:
        mem = rs.standard_normal((M, row)).astype(np.float32)
        g = rs.standard_normal((M, row)).astype(np.float32)
        for mode, a in MODES:
            got = _inherit_on_device(mem, want_p, mode, a, n, row)
            want = mem.copy()
            want[:, :n] = HM.inherit(mem[:, :n], want_p, mode, a, SEED, STEP)
            assert np.array_equal(got, MM.bits(want)), (n, tag, M, mode, a)          # the gaps between the rows untouched too
            if a > 0 and born:
                par, chi = HM.pairs(want_p)
                d = np.abs(want[:, chi].astype(np.float64) - mem[:, par].astype(np.float64))      # |child - parent| <= a, up to the sum's rounding
                assert d.max() > 0 and (d <= a + np.spacing(np.maximum(np.abs(want[:, chi]), np.abs(mem[:, par])))).all()
        for mode in ('blank', 'copy'):
            got = _backward_on_device(g, want_p, want_c, mode, n, row)
            rows = got[:, :n]
            assert np.array_equal(rows, MM.bits(HM.inherit_adjoint(g[:, :n], want_p, want_c, mode, np.float32))), (n, tag, M, mode)
            assert (got[:, n:] == NAN_BITS).all()                    # out of place: the gaps are nobody's
    return born


# ---------------------------------------------------------------------------------------------------- 1. the C ABI against the model
@pytest.mark.parametrize('n', SIZES)
def test_record_inherit_and_adjoint_equal_the_model(n):
    rs = np.random.RandomState(n)
    born = {name: _check_rule(n, alive, food, rs, tag=name) for name, (alive, food) in _patterns(n, rs).items()}
    assert born['no parent'] == 0 and born['no free slot'] == 0
    if n >= 8:
        assert born['more parents than free slots'] == n // 4 and born['more free slots than parents'] == n // 4 and born['at random'] > 0


def test_a_second_trip_of_every_grid_stride_loop():
    """65 537 slots: one more than 256 workgroups of 256 threads cover, the smallest N at which a thread of the record, of the
    rule and of the adjoint walks to a second slot (all three cap their grids at 256 workgroups a replica)."""
    n = GRID_SLOTS + 1
    rs = np.random.RandomState(5)
    k = np.arange(n)
    role = np.where(k % 2 == 0, 2, 1)                                # free, parent, free, ...: the LAST slot is a child
    role[:4] = 1                                                     # (the pairs are then (0, 4), (1, 6), ...: far apart in the end)
    alive = (role != 2).astype(np.uint8)
    food = np.where(role == 1, 0.9, 0.0).astype(np.float32)
    want_p, _ = HM.record(alive, food, 0.5)
    assert want_p[n - 1] >= 0 and (want_p >= 0).sum() > 30000        # the slot of the second trip is written
    assert _check_rule(n, alive, food, rs, Ms=(5,), tag='second trip') == (want_p >= 0).sum()


def test_special_values_keep_their_bits_at_no_mutation():
    n, M = 65, 5
    rs = np.random.RandomState(9)
    alive, food = _patterns(n, rs)['at random']
    want_p, want_c = HM.record(alive, food, 0.5)
    par, chi = HM.pairs(want_p)
    assert len(par) >= 4
    mem = rs.standard_normal((M, n)).astype(np.float32)
    words = mem.view(np.uint32)
    specials = (0x80000000, 0x00000123, 0x7F800000, 0x7FC12345)      # -0.0, a denormal, inf, a NaN payload
    for j, w in enumerate(specials):
        words[j % M, par[j]] = w
    got = _inherit_on_device(mem, want_p, 'copy', 0.0, n, n)
    assert np.array_equal(got, MM.bits(HM.inherit(mem, want_p, 'copy')))
    for j, w in enumerate(specials):
        assert got[j % M, chi[j]] == w and got[j % M, par[j]] == w
    g = rs.standard_normal((M, n)).astype(np.float32)
    g.view(np.uint32)[0, np.flatnonzero((want_p < 0) & (want_c < 0))[0]] = 0x7FC12345
    for mode in ('blank', 'copy'):                                   # a slot that is neither passes its gradient word through
        assert np.array_equal(_backward_on_device(g, want_p, want_c, mode, n, n), MM.bits(HM.inherit_adjoint(g, want_p, want_c, mode)))


@pytest.mark.parametrize('M', [1, 5])
def test_batched_entry_points_equal_the_model_per_replica(M):
    n, stride = [1000, 257, 64], 1000                                # ragged n[r]
    R = len(n)
    rs = np.random.RandomState(21 + M)
    worlds = [_patterns(k, rs)[name] for k, name in zip(n, ('at random', 'more parents than free slots', 'more free slots than parents'))]
    parent_of, child_of = _pass_and_record([w[0] for w in worlds], [w[1] for w in worlds], n, stride)
    for r in range(R):
        wp, wc = HM.record(*worlds[r], 0.5, stride)
        assert np.array_equal(parent_of[r], wp) and np.array_equal(child_of[r], wc), r      # the padding slots: -1 in both
        assert (wp >= 0).sum() > 0
    mem = rs.standard_normal((R, M, stride)).astype(np.float32)
    g = rs.standard_normal((R, M, stride)).astype(np.float32)
    par, chi = (torch.from_numpy(v.copy()).to(DEV) for v in (parent_of, child_of))
    b = _batch(n, stride)
    seeds = (C.c_uint64 * R)(*[SEED + 3 * r for r in range(R)])
    for mode, a in MODES:
        buf = torch.full((mem.size + TAIL,), float('nan'), dtype=torch.float32, device=DEV)
        buf[:mem.size] = torch.from_numpy(mem.reshape(-1)).to(DEV)
        _lib.check(_lib.lib.die_memory_inherit_batch(_lib.INHERIT_MODES[mode], a, M, C.byref(b), par.data_ptr(), buf.data_ptr(), seeds, STEP, None),
                   'die_memory_inherit_batch')
        got = _bits(buf)
        assert (got[mem.size:] == NAN_BITS).all()
        got = got[:mem.size].reshape(R, M, stride)
        for r in range(R):
            want = mem[r].copy()
            want[:, :n[r]] = HM.inherit(mem[r][:, :n[r]], parent_of[r], mode, a, SEED + 3 * r, STEP)
            assert np.array_equal(got[r], MM.bits(want)), (r, mode, a)               # the padding slots untouched
    for mode in ('blank', 'copy'):
        out = torch.full((g.size + TAIL,), float('nan'), dtype=torch.float32, device=DEV)
        tg = torch.from_numpy(g).to(DEV)
        _lib.check(_lib.lib.die_memory_inherit_backward_batch(_lib.INHERIT_MODES[mode], M, C.byref(b), par.data_ptr(), chi.data_ptr(), tg.data_ptr(),
                                                              out.data_ptr(), None), 'die_memory_inherit_backward_batch')
        got = _bits(out)
        assert (got[g.size:] == NAN_BITS).all()
        got = got[:g.size].reshape(R, M, stride)
        for r in range(R):
            want = g[r].copy()                                       # the padding slots pass through
            want[:, :n[r]] = HM.inherit_adjoint(g[r][:, :n[r]], parent_of[r], child_of[r], mode)
            assert np.array_equal(got[r], MM.bits(want)), (r, mode)


def test_abi_refusals_come_before_any_launch():
    n, M = 64, 2
    need = _lib.lib.die_births_workspace_bytes(1, n)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    out = torch.full((2, n), SENT_I, dtype=torch.int32, device=DEV)
    mem = torch.full((M, n), 0.5, dtype=torch.float32, device=DEV)
    g = torch.ones((M, n), dtype=torch.float32, device=DEV)
    L = _lib.lib
    bad = [
        L.die_births_record(n, None, need, out[0].data_ptr(), out[1].data_ptr(), None),
        L.die_births_record(n, ws.data_ptr(), need - 1, out[0].data_ptr(), out[1].data_ptr(), None),      # a workspace too small
        L.die_births_record(0, ws.data_ptr(), need, out[0].data_ptr(), out[1].data_ptr(), None),
        L.die_births_record(n, ws.data_ptr(), need, out[0].data_ptr(), out[0].data_ptr(), None),          # overlapping outputs
        L.die_memory_inherit(1, 0.0, 0, n, out[0].data_ptr(), mem.data_ptr(), n, 1, 0, None),
        L.die_memory_inherit(1, 0.0, 9, n, out[0].data_ptr(), mem.data_ptr(), n, 1, 0, None),
        L.die_memory_inherit(2, 0.0, M, n, out[0].data_ptr(), mem.data_ptr(), n, 1, 0, None),             # no such mode
        L.die_memory_inherit(1, -1.0, M, n, out[0].data_ptr(), mem.data_ptr(), n, 1, 0, None),
        L.die_memory_inherit(1, float('nan'), M, n, out[0].data_ptr(), mem.data_ptr(), n, 1, 0, None),
        L.die_memory_inherit(0, 0.5, M, n, out[0].data_ptr(), mem.data_ptr(), n, 1, 0, None),             # a mutation with 'blank'
        L.die_memory_inherit(1, 0.0, M, n, out[0].data_ptr(), mem.data_ptr(), n - 1, 1, 0, None),         # a stride below a row
        L.die_memory_inherit(1, 0.0, M, n, None, mem.data_ptr(), n, 1, 0, None),
        L.die_memory_inherit(1, 0.0, M, 0, out[0].data_ptr(), mem.data_ptr(), n, 1, 0, None),
        L.die_memory_inherit_backward(1, M, n, out[0].data_ptr(), out[1].data_ptr(), g.data_ptr(), g.data_ptr(), n, None),      # in place
        L.die_memory_inherit_backward(1, M, n, out[0].data_ptr(), None, g.data_ptr(), mem.data_ptr(), n, None),
    ]
    assert all(rc != 0 for rc in bad), bad
    torch.cuda.synchronize()
    assert bool((out == SENT_I).all()) and bool((mem == 0.5).all()) and bool((g == 1).all())


# ---------------------------------------------------------------------------------------------------- the agents and worlds
WIDE = dict(kernel_sizes=(3, 3), hidden_channels=8, hidden_activation='tanh')


def _agent(mode, a=0.0, seed=0, M=2, **kw):
    torch.manual_seed(seed)
    extra = dict(memory_inherit=mode, memory_mutation=a) if mode is not None else {}
    ag = die.NeuralAutomataAgent(scale=F.COEFS[0], deposit=F.COEFS[2], memory_channels=M, **WIDE, **extra, **kw)
    with torch.no_grad():
        for q in ag.model.parameters():
            q.uniform_(-0.5, 0.5)
    return ag


def _plain_step(env, data):
    """env.step with an action that carries no agent."""
    act = DeviceAction(env.agents.N, env.device, env.agents.slot)
    act.data = data.detach().contiguous()
    return env.step(act)


def _born_dyn(**kw):
    return die.Dynamics(agents_die=True, agents_born=True, **kw)


# ---------------------------------------------------------------------------------------------------- 2. die and refill within one step
@pytest.mark.parametrize('mode,a', MODES)
def test_a_slot_that_dies_and_is_refilled_holds_its_parents_memory(mode, a):
    W, H = 8, 8
    medium = np.zeros((3, W, H))
    medium[1] = 0.5
    medium[1, 5, 5] = 0.0                                            # the foodless cell
    medium[2] = np.random.RandomState(2).rand(W, H)
    cells = [(2, 2), (5, 5), (6, 1)]                                 # slot 0 well fed, slot 1 starving on the foodless cell, slot 2 poor but alive
    food = [0.9, 5e-5, 0.3]
    agents = np.array([[cx / (W - 1) for cx, _ in cells], [cy / (H - 1) for _, cy in cells], [1.0] * 3, food])
    for cx, cy in cells:
        medium[0, cx, cy] = 1.0

    def world():
        return die.Env.from_numpy(medium, agents, _born_dyn(), device=DEV, sort_every=0, seed=77)

    def zero_action_rows(ag):
        with torch.no_grad():
            ag.model.conv_layers()[-1].weight[:3].zero_()            # no action: no cost, nobody moves; the memory rows stay
        return ag

    env, ag = world(), zero_action_rows(_agent(mode, a))
    twin_env, twin = world(), zero_action_rows(_agent(None))         # the same forward without heredity: what the read-out wrote
    twin.model.load_state_dict(ag.model.state_dict())
    _, _, _, _, info = env.step(ag.forward(env._get_current_obs))
    twin.forward(twin_env._get_current_obs)
    rec = env.births_record()
    parent_of, child_of = rec.parent_of.cpu().numpy(), rec.child_of.cpu().numpy()
    assert parent_of.tolist() == [-1, 0, -1] and child_of.tolist() == [1, -1, -1]      # the starved slot is the parent's child
    assert info['num_agents'] == 3 and (rec.seed, rec.step) == (77, 0)
    written = twin.memory.cpu().numpy()
    got = ag.memory.cpu().numpy()
    assert written[:, 1].all() and not np.array_equal(MM.bits(written[:, 1]), MM.bits(written[:, 0]))
    assert np.array_equal(MM.bits(got[:, [0, 2]]), MM.bits(written[:, [0, 2]]))        # the parent and the bystander keep theirs
    assert np.array_equal(MM.bits(got), MM.bits(HM.inherit(written, parent_of, mode, a, 77, 0)))
    assert not np.array_equal(MM.bits(got[:, 1]), MM.bits(written[:, 1]))              # not the dead agent's
    if mode == 'blank':
        assert not MM.bits(got[:, 1]).any()
    elif a == 0:
        assert np.array_equal(MM.bits(got[:, 1]), MM.bits(written[:, 0]))


# ---------------------------------------------------------------------------------------------------- 3. replicas equal stand-alone runs
REFERENCE_DYNAMICS = dict(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8)     # examples/learning_agents.py
STEPS = 40


def _population(R, mode, a, seed=5, **kw):
    """tests/test_gpu_births.py _nca_population with memory: zero rows (the colony grows), saturated rows (it dies out), init_weights()."""
    torch.manual_seed(seed)
    template = die.NeuralAutomataAgent(scale=0.01, deposit=60.0, kernel_sizes=(3, 3), hidden_channels=8, hidden_activation='tanh',
                                       memory_channels=2, memory_inherit=mode, memory_mutation=a, **kw)
    rows = []
    for r in range(R):
        template.model.init_weights()
        v = torch.nn.utils.parameters_to_vector(template.model.parameters()).detach().clone()
        rows.append(torch.zeros_like(v) if r % 3 == 0 else v * 50.0 if r % 3 == 1 else v)
    return template, torch.stack(rows)


@pytest.mark.parametrize('mode,a,E,kw', [('blank', 0.0, 1, {}), ('copy', 0.0, 1, {}), ('copy', 0.1, 1, {}), ('copy', 0.1, 2, {}),
                                         ('copy', 0.1, 1, dict(signal_channels=2))],
                         ids=['blank', 'copy', 'copy mutated', 'episodes', 'signals'])
def test_replicas_inherit_like_their_stand_alone_envs(mode, a, E, kw):
    W, H, R, N = 32, 32, 3 * E, 400
    dyn_kw = dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15)
    template, rows = _population(R // E, mode, a, **kw)
    seeds = [11 + r for r in range(R)]
    benv = BatchedEnv((W, H), _born_dyn(**dyn_kw), replicas=R, seeds=seeds, max_agents=N)
    pop = BatchedNeuralAutomataAgent(benv, template, rows, episodes=E)
    k0 = [int(benv.alive[r, :benv.n[r]].sum().item()) for r in range(R)]
    envs = [die.Env((W, H), _born_dyn(**dyn_kw), seed=seeds[r], max_agents=N) for r in range(R)]
    alone = [pop.replica_agent(r).to(DEV) for r in range(R)]
    assert all(ag.memory_inherit == mode and ag.memory_mutation == a for ag in alone)
    first, mems, inherited = torch.empty((STEPS, R, 2), dtype=torch.float64, device=DEV), [], 0
    for t in range(STEPS):
        benv.step(pop, first[t])
        rec = benv.births_record()
        for r, (env, ag) in enumerate(zip(envs, alone)):
            env.step(ag.forward(env._get_current_obs))
            assert torch.equal(pop.memory[r, :, :benv.n[r]].view(torch.int32), ag.memory.view(torch.int32)), (t, r)
            one = env.births_record()
            assert torch.equal(rec.parent_of[r, :benv.n[r]], one.parent_of) and torch.equal(rec.child_of[r, :benv.n[r]], one.child_of), (t, r)
            m, ags = benv.replica_numpy(r)
            assert np.array_equal(m, env.medium.to_numpy()) and np.array_equal(ags, env.agents.to_numpy()), (t, r)
            if kw:
                assert torch.equal(pop.signals[r], ag.signals), (t, r)
        children = rec.parent_of >= 0
        inherited += int((pop.memory.transpose(1, 2)[children] != 0).any(dim=1).sum().item())
        mems.append(pop.memory.clone())
    _, alive = BatchedEnv.read_results(first)
    born = int(np.clip(np.diff(np.vstack([np.asarray(k0)[None], alive]), axis=0), 0, None).sum())
    print(f'heredity {mode} a={a} E={E} {kw}: at least {born} children in {STEPS} steps, {inherited} of them with a non-zero memory')
    assert alive[-1, 0] > k0[0] and born >= 8                        # the zero-weight colony grew; at least 8 children in total
    benv.reset()                                                     # across reset(): the world step starts over, so the run repeats
    pop.reset()
    for t in range(STEPS):
        assert torch.equal(benv.step(pop).view(torch.int64), first[t].view(torch.int64)), t
        assert torch.equal(pop.memory.view(torch.int32), mems[t].view(torch.int32)), t


def test_per_replica_worlds_inherit_through_their_own_envs():
    W, H, R, N = 32, 32, 3, 400
    dyn_kw = dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15)
    template, rows = _population(R, 'copy', 0.1)
    big = BatchedEnv((W, H), _born_dyn(**dyn_kw), replicas=R, seed=11, max_agents=N, per_replica=True)
    small = BatchedEnv((W, H), _born_dyn(**dyn_kw), replicas=R, seed=11, max_agents=N, per_replica=False)
    pb, ps = BatchedNeuralAutomataAgent(big, template, rows), BatchedNeuralAutomataAgent(small, template, rows)
    assert torch.equal(big.run(pb, 12), small.run(ps, 12))
    for r in range(R):
        assert torch.equal(pb.agents[r].memory.view(torch.int32), ps.memory[r, :, :small.n[r]].view(torch.int32)), r
    with pytest.raises(NotImplementedError, match=r'envs\[r\]\.births_record'):
        big.births_record()
    with pytest.raises(NotImplementedError, match='per_replica'):
        pb.inherit_memory(small.births_record())


# ---------------------------------------------------------------------------------------------------- 4. explicit equals automatic
@pytest.mark.parametrize('mode,a', MODES)
def test_the_explicit_call_equals_the_steps_own(mode, a):
    W, H, N = 24, 24, 200
    make = lambda: die.Env((W, H), _born_dyn(init_agent_ratio=0.2), seed=3, max_agents=N, sort_every=0)
    auto_env, hand_env, bare_env = make(), make(), make()
    auto, hand, bare = _agent(mode, a), _agent(mode, a), _agent(None)
    born = 0
    for t in range(6):
        auto_env.step(auto.forward(auto_env._get_current_obs))       # the step inherits by itself
        act = hand.forward(hand_env._get_current_obs)
        _plain_step(hand_env, act.data)                              # an action that carries no agent: the caller's call
        rec = hand_env.births_record()
        assert hand.inherit_memory(rec) is hand.memory
        twin_act = bare.forward(bare_env._get_current_obs)           # a mode-less twin: the functional call on its memory
        bare_env.step(twin_act)
        bare.memory = functional.inherit_memory(bare.memory, bare_env.births_record(), mode, a)
        born += int((rec.parent_of >= 0).sum().item())
        for other in (hand, bare):
            assert torch.equal(auto.memory.view(torch.int32), other.memory.view(torch.int32)), t
        assert torch.equal(auto_env.agents.agent_food, hand_env.agents.agent_food) and torch.equal(auto_env.agents.x, bare_env.agents.x), t
    assert born > 0


# ---------------------------------------------------------------------------------------------------- 5. BPTT across births
def _frame(env):
    W, H = env.medium.W, env.medium.H
    m = env.medium.to_numpy()
    cx, cy = S.cell(env.agents.x.cpu().numpy().view(np.uint32), W), S.cell(env.agents.y.cpu().numpy().view(np.uint32), H)
    return dict(occ=m[0], food=m[1], chem=m[2], cx=cx, cy=cy, mask=None)


def _link(rec, r, n, mode, a, M):
    """A model link from the device's own record of replica r (None: a stand-alone record)."""
    parent_of = (rec.parent_of if r is None else rec.parent_of[r, :n]).cpu().numpy().copy()
    par, _ = HM.pairs(parent_of)
    added = HM.noise(rec.seeds[r or 0], rec.step, par, M, a).astype(np.float64) if a > 0 else None
    return parent_of, mode, added


def _layer_arrays(ag):
    return [k.weight.detach().cpu().double().numpy() for k in ag.model.conv_layers()]


def _window(mode, a, loss='all', detach=False, T=4, before=None, dyn=None, slots=400):
    """T links of recurrent_action, a plain env.step, inherit_memory(record, memory_next) on 24 x 24 (`detach`: the inherited
    memory is handed on detached), the loss backpropagated: the device's tensors and gradients, and what the float64 loop needs
    to repeat them — the device's own records.  `before`: a callable of (env, agent) run on the fresh world first
    (tests/test_gpu_epoch_wrap.py: real steps up to the epoch wrap, under a Dynamics `dyn` and with `slots` that keep the colony breeding
    that long)."""
    W, H, N, M = 24, 24, slots, 2                                    # (more free slots than the first pass fills: later passes breed too)
    env = die.Env((W, H), _born_dyn(**(dyn or dict(init_agent_ratio=0.2))), seed=3, max_agents=N, sort_every=0, device=DEV)
    ag = _agent(mode, a)
    if before is not None:
        before(env, ag)
    rs = np.random.RandomState(4)
    us, vs = rs.standard_normal((T, 3, N)), rs.standard_normal((T, M, N))
    mem0 = rs.standard_normal((M, N)).astype(np.float32)
    leaf = torch.from_numpy(mem0).to(DEV).requires_grad_()
    memory, frames, records, links, acts, mems = leaf, [], [], [], [], []
    for t in range(T):
        frames.append(_frame(env))
        rec0 = functional.memory_record(env._get_current_obs)
        records.append((rec0.cell.cpu().numpy().copy(), rec0.win.cpu().numpy().copy()))
        action, memory_next = ag.recurrent_action(env._get_current_obs, memory)
        _plain_step(env, action)
        rec = env.births_record()
        memory = ag.inherit_memory(rec, memory_next)
        assert memory.grad_fn is not None and torch.equal(ag.memory.view(torch.int32), memory.detach().view(torch.int32))
        assert ag.memory.data_ptr() != memory.data_ptr()
        links.append(_link(rec, None, N, mode, a, M))
        acts.append(action)
        mems.append(memory)
        if detach:
            memory = memory.detach()
    births = [int((l[0] >= 0).sum()) for l in links]
    assert sum(births[:-1]) > 0, births                              # a birth inside the window, with a forward after it
    at = max(t for t in range(T - 1) if births[t])                   # the last pass with children that a forward followed
    kids = (links[at][0] >= 0).astype(np.float64)

    def loss_of(acts, mems, as_t):
        if loss == 'all':
            return sum((as_t(us[t]) * acts[t]).sum() + (as_t(vs[t]) * mems[t]).sum() for t in range(T))
        if loss == 'children memory':                                # the memory that pass's children received, nothing else
            return (as_t(vs[at] * kids) * mems[at]).sum()
        return (as_t(us[at + 1] * kids) * acts[at + 1]).sum()        # 'children action': what those children did at the next forward

    total = loss_of(acts, mems, lambda v: torch.as_tensor(v, dtype=torch.float32, device=DEV))
    if total.requires_grad:
        total.backward()
    torch.cuda.synchronize()
    grads = [np.zeros(tuple(q.shape)) if q.grad is None else q.grad.detach().cpu().numpy().copy() for q in ag.model.parameters()]
    run = dict(ag=ag, leaf=leaf, frames=frames, records=records, links=links, mem0=mem0, dev_acts=acts, dev_mems=mems, loss_of=loss_of,
               births=births, kids=int(kids.sum()))
    return run, grads


def _float64(run, detach=False):
    ag = run['ag']
    ws = [torch.tensor(w, requires_grad=True) for w in _layer_arrays(ag)]
    m0 = torch.tensor(run['mem0'].astype(np.float64), requires_grad=True)
    out = HM.unroll(ws, 'circular', 'tanh', run['frames'], run['records'], run['links'], m0, ag.action_coefs, True, detach_inherited=detach)
    loss = run['loss_of'](out['actions'], out['memories'][1:], lambda v: torch.as_tensor(np.asarray(v), dtype=torch.float64))
    if loss.requires_grad:
        loss.backward()
    zero = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()
    return [zero(w) for w in ws], zero(m0), out


@pytest.mark.parametrize('mode,a', MODES)
def test_bptt_across_births_matches_the_float64_loop(mode, a):
    run, got = _window(mode, a)
    ref_w, ref_m, out = _float64(run)
    fwd = max(MG.rel_err(run['dev_mems'][-1].detach().cpu().numpy(), out['memories'][-1].detach().numpy()),
              MG.rel_err(run['dev_acts'][-1].detach().cpu().numpy(), out['actions'][-1].detach().numpy()))
    errs = [MG.rel_err(g, r) for g, r in zip(got, ref_w)] + [MG.rel_err(run['leaf'].grad.cpu().numpy(), ref_m)]
    print(f'bptt across births 24x24 T=4 {mode} a={a}: births per link {run["births"]}; device', ' '.join(f'{e:.3e}' for e in errs),
          f'(layers, d loss / d memory; ceiling {CEILING:.0e}); forward apart by {fwd:.2e}')
    assert all(np.abs(r).max() > 0 for r in ref_w) and np.abs(ref_m).max() > 0
    assert fwd <= 1e-5                                               # the model followed the same trajectory
    assert all(e <= CEILING for e in errs), errs


def test_a_childs_gradient_reaches_its_parent():
    # the loss on the memory a pass's children received: under 'copy' it is their parents' read-out, under 'blank' a constant
    run, got = _window('copy', 0.1, 'children memory')
    ref_w, _, _ = _float64(run)
    assert run['kids'] > 0 and all(np.abs(g).max() > 0 for g in got)
    assert all(MG.rel_err(g, r) <= CEILING for g, r in zip(got, ref_w))
    _, blank = _window('blank', 0.0, 'children memory')
    assert not any(g.any() for g in blank)
    # the loss on what the children of a pass did at the next forward: the last layer's memory rows are reached through the memory only
    run, got = _window('copy', 0.1, 'children action')
    ref_w, _, _ = _float64(run)
    assert run['kids'] > 0 and np.abs(got[-1][3:]).max() > 0 and np.abs(ref_w[-1][3:]).max() > 0
    assert all(MG.rel_err(g, r) <= CEILING for g, r in zip(got, ref_w))
    # ... and behind a .detach() of the inherited memory nothing reaches them
    run, cut = _window('copy', 0.1, 'children action', detach=True)
    ref_cut, _, _ = _float64(run, detach=True)
    assert not cut[-1][3:].any() and not ref_cut[-1][3:].any() and np.abs(cut[-1][:3]).max() > 0
    assert all(MG.rel_err(g, r) <= CEILING for g, r in zip(cut, ref_cut))


def _cands(n, seed, mode, a, M=2):
    torch.manual_seed(seed)
    out = []
    for _ in range(n):
        ag = die.NeuralAutomataAgent(scale=F.COEFS[0], deposit=F.COEFS[2], memory_channels=M, memory_inherit=mode, memory_mutation=a, **WIDE)
        with torch.no_grad():
            for q in ag.model.parameters():
                q.uniform_(-0.5, 0.5)
        out.append(ag)
    return out


def _batched_window(mode, a, T=4, before=None, dyn=None, slots=400):
    """T links of the batched recurrent_action, step_action, inherit_memory(record, memory_next) on three 24 x 24 worlds against the
    float64 loop fed the device's own records: (births per replica and link, errors per array, forward distance).  `before`: a
    callable of (benv, pop) run on the fresh worlds first (tests/test_gpu_epoch_wrap.py: real steps up to the epoch wrap, under a
    Dynamics `dyn` and with `slots` that keep the colonies breeding that long)."""
    W, H, R, N, M = 24, 24, 3, slots, 2
    benv = BatchedEnv((W, H), _born_dyn(**(dyn or dict(init_agent_ratio=0.2))), replicas=R, seed=11, max_agents=N, device=DEV)
    pop = BatchedNeuralAutomataAgent.from_agents(benv, _cands(R, 27, mode, a))
    if before is not None:
        before(benv, pop)
    Nmax = benv.Nmax
    rs = np.random.RandomState(4)
    us, vs = rs.standard_normal((T, 3, R, Nmax)), rs.standard_normal((T, R, M, Nmax))
    mem0 = rs.standard_normal((R, M, Nmax)).astype(np.float32)
    leaf = torch.from_numpy(mem0).to(DEV).requires_grad_()
    pop.parameters.requires_grad_()
    memory, loss = leaf, 0.
    frames, records, links = ([[] for _ in range(R)] for _ in range(3))
    for t in range(T):
        rec0 = functional.memory_record_batch(pop)
        cell, win = rec0.cell.cpu().numpy(), rec0.win.cpu().numpy()
        for r in range(R):
            n = benv.n[r]
            m, _ = benv.replica_numpy(r)
            frames[r].append(dict(occ=m[0], food=m[1], chem=m[2], mask=None, cx=S.cell(benv.x[r, :n].cpu().numpy().view(np.uint32), W),
                                  cy=S.cell(benv.y[r, :n].cpu().numpy().view(np.uint32), H)))
            records[r].append((cell[r, :n].copy(), win[r, :n].copy()))
        action, memory_next = pop.recurrent_action(memory)
        benv.step_action(action)
        rec = benv.births_record()
        memory = pop.inherit_memory(rec, memory_next)
        assert memory.grad_fn is not None and torch.equal(pop.memory.view(torch.int32), memory.detach().view(torch.int32))
        for r in range(R):
            links[r].append(_link(rec, r, benv.n[r], mode, a, M))
        loss = loss + (torch.as_tensor(us[t], dtype=torch.float32, device=DEV) * action).sum() + \
            (torch.as_tensor(vs[t], dtype=torch.float32, device=DEV) * memory).sum()
    births = [[int((l[0] >= 0).sum()) for l in links[r]] for r in range(R)]
    assert sum(sum(b[:-1]) for b in births) > 0, births
    loss.backward()
    torch.cuda.synchronize()
    got, gm = pop.parameters.grad.cpu().numpy(), leaf.grad.cpu().numpy()
    host = pop.parameters.detach().cpu().double().numpy()
    split = lambda row: [np.asarray(row[off:off + cout * cin * k * k]).reshape(cout, cin, k, k) for k, cin, cout, off in pop._layers]
    errs, fwd = [], 0.0
    for r in range(R):
        n = benv.n[r]
        ws = [torch.tensor(w, requires_grad=True) for w in split(host[r])]
        m0 = torch.tensor(mem0[r, :, :n].astype(np.float64), requires_grad=True)
        out = HM.unroll(ws, 'circular', 'tanh', frames[r], records[r], links[r], m0, pop.template.action_coefs, True)
        ref = sum((torch.as_tensor(us[t][:, r, :n]) * out['actions'][t]).sum() + (torch.as_tensor(vs[t][r, :, :n]) * out['memories'][t + 1]).sum()
                  for t in range(T))
        ref.backward()
        errs += [MG.rel_err(g, w.grad.numpy()) for g, w in zip(split(got[r]), ws)] + [MG.rel_err(gm[r, :, :n], m0.grad.numpy())]
        fwd = max(fwd, MG.rel_err(pop.memory[r, :, :n].cpu().numpy(), out['memories'][-1].detach().numpy()))
    return births, errs, fwd


@pytest.mark.parametrize('mode,a', [('blank', 0.0), ('copy', 0.1)])
def test_batched_bptt_across_births_matches_the_float64_loop(mode, a):
    births, errs, fwd = _batched_window(mode, a)
    print(f'batched bptt across births 24x24 R=3 T=4 {mode} a={a}: births {births}; device worst {max(errs):.3e} of max|grad_f64| per array '
          f'(ceiling {CEILING:.0e}); forward apart by {fwd:.2e}')
    assert fwd <= 1e-5
    assert max(errs) <= CEILING, errs


# ---------------------------------------------------------------------------------------------------- 6. refusals, search
def test_refusals_leave_memory_counters_and_world_alone():
    W, H, N = 24, 24, 200
    env = die.Env((W, H), _born_dyn(init_agent_ratio=0.2), seed=3, max_agents=N, sort_every=0)
    with pytest.raises(ValueError, match='no birth pass yet'):
        env.births_record()
    ag = _agent('copy', 0.1, p_agent_dropout=0.25, dropout_seed=3)
    env.step(ag.forward(env._get_current_obs))
    rec = env.births_record()
    held = ag.memory.clone()
    state = lambda: [t.clone() for t in (env.agents.x, env.agents.y, env.agents.alive, env.agents.agent_food, env.medium.chem, env.medium.food)]
    before, step = state(), ag.dropout_step
    none, nomem = _agent(None), die.NeuralAutomataAgent(scale=0.1, kernel_sizes=(3, 3))
    none.memory = held.clone()
    batched = functional.BirthsRecord(rec.parent_of[None], rec.child_of[None], rec.seeds, rec.step, rec.n)
    cases = [(nomem, rec, None), (none, rec, None), (ag, None, None), (ag, batched, None), (ag, rec, held[:, :-1]), (ag, rec, held.double()),
             (ag, rec, held.cpu()), (ag, rec, held[:1])]
    for who, record, memory in cases:
        with pytest.raises(ValueError):
            who.inherit_memory(record, memory)
    with pytest.raises(ValueError):
        functional.inherit_memory(held, rec, 'blank', 0.5)
    with pytest.raises(ValueError):
        functional.inherit_memory(held, rec, 'clone')
    assert torch.equal(ag.memory.view(torch.int32), held.view(torch.int32)) and ag.dropout_step == step
    assert all(torch.equal(u, v) for u, v in zip(before, state()))
    # a world without births; a pass consumed by a later step
    plain = die.Env((W, H), die.Dynamics(agents_die=True, init_agent_ratio=0.2), seed=3, max_agents=N, sort_every=0)
    with pytest.raises(ValueError, match='no births'):
        plain.births_record()
    plain.apply_births()
    assert plain.births_record().step == 0
    plain.step(die.PhysarumAgent(max_agents=N, seed=2).forward(plain._get_current_obs))
    with pytest.raises(ValueError, match='consumed'):
        plain.births_record()
    # the batched constructor: the old refusal word for word without a rule, none with one
    benv = BatchedEnv((W, H), _born_dyn(init_agent_ratio=0.2), replicas=2, seed=3, max_agents=N)
    with pytest.raises(NotImplementedError, match='inheritance at birth is not defined yet'):
        BatchedNeuralAutomataAgent(benv, _agent(None))
    pop = BatchedNeuralAutomataAgent(benv, _agent('blank'))
    with pytest.raises(ValueError, match='no birth pass yet'):
        benv.births_record()
    with pytest.raises(ValueError):
        pop.inherit_memory(rec)                                      # a stand-alone record
    with pytest.raises(NotImplementedError, match='agents_born'):
        benv.differentiable_step(torch.zeros((3, 2, benv.Nmax), dtype=torch.float32, device=DEV))


def test_one_pgpe_generation_under_births_with_memory():
    W, H, R, T, N = 32, 32, 6, 16, 400
    dyn = lambda: _born_dyn(**REFERENCE_DYNAMICS)
    template = die.NeuralAutomataAgent(scale=0.01, deposit=20.0, kernel_sizes=(3, 3), hidden_channels=8, hidden_activation='tanh',
                                       memory_channels=2, memory_inherit='copy', memory_mutation=0.1)
    benv = BatchedEnv((W, H), dyn(), replicas=R, seeds=[9] * R, max_agents=N)
    pop = BatchedNeuralAutomataAgent(benv, template)
    s = PGPE(R, center_init=pop.parameters[0].cpu(), radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1,
             optimizer_config=dict(max_speed=0.1, momentum=0.9), seed=11, device='cuda')
    s.ask(pop.parameters)
    rows = pop.parameters.cpu()
    benv.run(pop, 3)                                                 # a used batch: the generation starts from blank memory
    benv.reset()
    pop.reset()
    res = benv.run(pop, T)
    s.tell(res)
    fitness = s.fitness.cpu().tolist()
    rew, _ = BatchedEnv.read_results(res)
    for r in range(R):
        env = die.Env((W, H), dyn(), seed=9, max_agents=N)
        ag = BatchedNeuralAutomataAgent.unpack(template, rows[r]).to(env.device)
        total = 0.0
        obs = env._get_current_obs
        want = []
        for _ in range(T):
            obs, rw, *_ = env.step(ag.forward(obs))
            want.append(rw)
        assert np.array_equal(rew[:, r], np.array(want)), r
        assert fitness[r] == sum(want), r
        assert torch.equal(pop.memory[r].view(torch.int32), ag.memory.view(torch.int32)), r
