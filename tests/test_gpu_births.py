"""Dynamics(agents_born=True) on the device: the entry points against the numpy model (tests/births_model.py) bit for bit (at a
few slots, and past every grid cap of the three kernels: tests/midsize_shapes.py), a
stepped Env against the same world stepped without births plus `apply_births()`, batched replicas against their stand-alone Envs
(NCA narrow and wide, Physarum with headings; across reset(), with episodes, through step_action), one PGPE generation, and the
refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent, BatchedPhysarumAgent
from die_amd.search import PGPE
from tests import births_model as M
from tests.midsize_shapes import BIRTH_BATCH_NS, BIRTH_NS, BIRTH_PATTERNS

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SIZES = (1, 63, 64, 65, 320, 321, 641)          # a lane, a wave's edge, a workgroup's edge (256), several workgroups


# ---------------------------------------------------------------- 1. the entry points against the model
def _patterns(n, rs):
    """name -> (alive, food): who is a parent (alive, 0.9), who is free (dead), who is neither (alive, poor)."""
    k = np.arange(n)
    P, F, O = 1, 2, 0
    def build(role):
        alive = (role != F).astype(np.uint8)
        food = np.where(role == P, rs.uniform(0.51, 30.0, n), np.where(role == O, rs.uniform(0.0, 0.5, n), 0.0)).astype(np.float32)
        return alive, food
    third = max(n // 3, 1)
    cases = {
        'all parents, no free slot': np.full(n, P),
        'all free, no parent': np.full(n, F),
        'more parents than free': np.where(k % 4 == 3, F, P),
        'more free than parents': np.where(k % 4 == 3, P, F),
        'equal counts': np.where(k % 2 == 0, P, F)[:n] if n % 2 == 0 else np.r_[np.where(k[:-1] % 2 == 0, P, F), O],
        'free slots before the parents': np.where(k < third, F, np.where(k >= n - third, P, O)),
        'free slots after the parents': np.where(k < third, P, np.where(k >= n - third, F, O)),
        'interleaved at random': rs.choice([P, F, O], n, p=[0.4, 0.4, 0.2]),
        'the threshold itself is no parent': np.where(k % 2 == 0, P, F),
    }
    out = {name: build(np.asarray(role)) for name, role in cases.items()}
    a, f = out['the threshold itself is no parent']
    f[a != 0] = np.float32(0.5)
    return out


def _dev(x, y, alive, food):
    t = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).view(dt) if dt is not None else np.ascontiguousarray(v)).to(DEV)
    return [t(x, np.int32), t(y, np.int32), t(alive, None), t(food, None)]


def _call(arrs, n, seed, step, boundary, spread, count0, ws=None):
    """die_agent_births on device copies; returns (x, y, alive, food as numpy, count)."""
    x, y, alive, food = arrs
    res = torch.zeros(2, dtype=torch.float64, device=DEV)
    res.view(torch.int64)[1] = count0
    need = _lib.lib.die_births_workspace_bytes(1, n)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV) if ws is None else ws
    a = _lib.Agents(n, x.data_ptr(), y.data_ptr(), alive.data_ptr(), food.data_ptr(), None)
    p = _lib.Births(0.5, boundary, spread, step, 0)
    rc = _lib.lib.die_agent_births(C.byref(a), C.byref(p), seed, res.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == 0, _lib.lib.die_last_error()
    torch.cuda.synchronize()
    return (x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32), alive.cpu().numpy(), food.cpu().numpy(),
            int(res.cpu().view(torch.int64)[1]))


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and \
        np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32)) and got[4] == want[4]


@pytest.mark.parametrize('boundary', [M.WRAP, M.LIMIT], ids=['wrap', 'limit'])
@pytest.mark.parametrize('n', SIZES)
def test_entry_point_equals_the_model(n, boundary):
    rs = np.random.RandomState(100 + n)
    spread, seed, step = 0.3, 0x1234567890ABCDEF + n, 17 + n         # a wide spread: many children cross an edge
    for name, (alive, food) in _patterns(n, rs).items():
        x = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        y = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        x[alive == 0] = 0; y[alive == 0] = 0
        count0 = int(alive.sum())
        wx, wy, wa, wf, born = M.births(x, y, alive, food, world_seed=seed, world_step=step, born_spread=spread, boundary=boundary)
        want = (wx, wy, wa, wf, count0 + born)
        got = _call(_dev(x, y, alive, food), n, seed, step, boundary, spread, count0)
        assert _same(got, want), (n, name)
        again = _call(_dev(x, y, alive, food), n, seed, step, boundary, spread, count0)      # the same bits on every run
        assert _same(again, got), (n, name)
        assert got[4] == int(got[2].sum()), (n, name)


# Past the grid caps (tests/test_batch_midsize_cpu.py recomputes why each n): 65 537 gives 257 workgroups — the rank pass's sum over
# the workgroups before it takes a second trip; 131 073 is one chunk past BIRTH_MAX_GROUPS — every workgroup walks two chunks, carrying
# its running ranks across the barriers, and the last one gets an empty range; 262 145 walks three; 2 097 665 with every second
# slot a parent has more pairs than the spawn grid has threads.
@pytest.mark.parametrize('boundary', [M.WRAP, M.LIMIT], ids=['wrap', 'limit'])
@pytest.mark.parametrize('n', BIRTH_NS)
def test_entry_point_equals_the_model_past_the_grid_caps(n, boundary):
    rs = np.random.RandomState(100 + n)
    spread, seed, step = 0.3, 0x1234567890ABCDEF + n, 17 + n
    pats = _patterns(n, rs)
    for name in BIRTH_PATTERNS:
        alive, food = pats[name]
        x = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        y = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        x[alive == 0] = 0; y[alive == 0] = 0
        count0 = int(alive.sum())
        wx, wy, wa, wf, born = M.births(x, y, alive, food, world_seed=seed, world_step=step, born_spread=spread, boundary=boundary)
        assert born > 0, (n, name)
        if name == 'equal counts' and n == BIRTH_NS[-1]:
            assert born > 4096 * 256                                   # the spawn loop strides
        want = (wx, wy, wa, wf, count0 + born)
        got = _call(_dev(x, y, alive, food), n, seed, step, boundary, spread, count0)
        assert _same(got, want), (n, name)
        again = _call(_dev(x, y, alive, food), n, seed, step, boundary, spread, count0)      # the same bits on every run
        assert _same(again, got), (n, name)
        assert got[4] == int(got[2].sum()), (n, name)


def test_batched_entry_equals_stand_alone_calls_past_the_grid_caps():
    """One call, stride 131 073: replica 0 walks two chunks a workgroup, replica 1 (65 537 slots) has workgroups without a slot
    in the same grid, replica 2 fits one workgroup.  Each ends as its stand-alone call; the padding behind n[r] stays."""
    rs = np.random.RandomState(8)
    ns, spread, step = BIRTH_BATCH_NS, 0.3, 5
    stride, R = max(ns), len(ns)
    seeds = [11, 2 ** 63 + 5, 11]
    worlds = []
    for n in ns:
        alive, food = _patterns(n, rs)['interleaved at random']
        x = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        y = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        worlds.append((x, y, alive, food))
    for boundary in (M.WRAP, M.LIMIT):
        pad = lambda v, fill: np.r_[v, np.full(stride - len(v), fill, v.dtype)]
        # (the padding behind n[r] looks like parents AND must stay untouched: only slots < n count)
        batch = _dev(*[np.stack([pad(w[i], f) for w in worlds]) for i, f in ((0, 77), (1, 77), (2, 1), (3, 9.0))])
        before = [t.clone() for t in batch]
        res = torch.zeros((R, 2), dtype=torch.float64, device=DEV)
        ws = torch.empty(_lib.lib.die_births_workspace_bytes(R, stride), dtype=torch.uint8, device=DEV)
        a = _lib.Agents(stride, *[t.data_ptr() for t in batch], None)
        b = _lib.Batch(R, 0, 0, stride, 0, (C.c_int64 * 64)(*ns))
        p = _lib.Births(0.5, boundary, spread, step, 0)
        rc = _lib.lib.die_agent_births_batch(C.byref(a), C.byref(b), C.byref(p), (C.c_uint64 * R)(*seeds), res.data_ptr(), ws.data_ptr(),
                                             ws.numel(), None)
        assert rc == 0, _lib.lib.die_last_error()
        torch.cuda.synchronize()
        counts = res.cpu().view(torch.int64)[:, 1].tolist()
        for r, n in enumerate(ns):
            alone = _call(_dev(*worlds[r]), n, seeds[r], step, boundary, spread, 0)
            got = (batch[0][r, :n].cpu().numpy().view(np.uint32), batch[1][r, :n].cpu().numpy().view(np.uint32),
                   batch[2][r, :n].cpu().numpy(), batch[3][r, :n].cpu().numpy(), counts[r])
            assert _same(got, alone), (r, boundary)
            assert alone[4] > 0
            for t, t0 in zip(batch, before):
                assert torch.equal(t[r, n:], t0[r, n:]), r


def test_batched_entry_equals_stand_alone_calls():
    """R = 3 replicas of different n in one call: each ends as its stand-alone call (other seed, same step)."""
    rs = np.random.RandomState(7)
    ns, stride, spread, step = (641, 65, 320), 641, 0.05, 3
    seeds = [11, 2 ** 63 + 5, 11]
    worlds = []
    for n in ns:
        alive, food = _patterns(n, rs)['interleaved at random']
        x = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        y = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        worlds.append((x, y, alive, food))
    for boundary in (M.WRAP, M.LIMIT):
        pad = lambda v, fill: np.r_[v, np.full(stride - len(v), fill, v.dtype)]
        # (the padding behind n[r] looks like parents AND must stay untouched: only slots < n count)
        batch = _dev(*[np.stack([pad(w[i], f) for w in worlds]) for i, f in ((0, 77), (1, 77), (2, 1), (3, 9.0))])
        before = [t.clone() for t in batch]
        res = torch.zeros((3, 2), dtype=torch.float64, device=DEV)
        ws = torch.empty(_lib.lib.die_births_workspace_bytes(3, stride), dtype=torch.uint8, device=DEV)
        a = _lib.Agents(stride, *[t.data_ptr() for t in batch], None)
        b = _lib.Batch(3, 0, 0, stride, 0, (C.c_int64 * 64)(*ns))
        p = _lib.Births(0.5, boundary, spread, step, 0)
        rc = _lib.lib.die_agent_births_batch(C.byref(a), C.byref(b), C.byref(p), (C.c_uint64 * 3)(*seeds), res.data_ptr(), ws.data_ptr(),
                                             ws.numel(), None)
        assert rc == 0, _lib.lib.die_last_error()
        torch.cuda.synchronize()
        counts = res.cpu().view(torch.int64)[:, 1].tolist()
        for r, n in enumerate(ns):
            alone = _call(_dev(*worlds[r]), n, seeds[r], step, boundary, spread, 0)
            got = (batch[0][r, :n].cpu().numpy().view(np.uint32), batch[1][r, :n].cpu().numpy().view(np.uint32),
                   batch[2][r, :n].cpu().numpy(), batch[3][r, :n].cpu().numpy(), counts[r])
            assert _same(got, alone), (r, boundary)
            assert alone[4] > 0
            for t, t0 in zip(batch, before):
                assert torch.equal(t[r, n:], t0[r, n:]), r

        # bad arguments: an error, and nothing launched
        state = [t.clone() for t in batch]
        def refused(replicas=3, n=ns, ws_bytes=ws.numel(), stride_=stride):
            bb = _lib.Batch(replicas, 0, 0, stride_, 0, (C.c_int64 * 64)(*n))
            return _lib.lib.die_agent_births_batch(C.byref(a), C.byref(bb), C.byref(p), (C.c_uint64 * 3)(*seeds), res.data_ptr(),
                                                   ws.data_ptr(), ws_bytes, None)
        assert refused(ws_bytes=ws.numel() - 256) == -1
        assert refused(n=(641, 642, 320)) == -1
        assert refused(replicas=0) == -1 and refused(replicas=65) == -1
        torch.cuda.synchronize()
        assert all(torch.equal(t, s) for t, s in zip(batch, state))
        assert res.cpu().view(torch.int64)[:, 1].tolist() == counts


# ---------------------------------------------------------------- 2. Env, stepped
def _seeded_world(W, H, seed=7):
    from die_amd.device_array import from_q32, to_q32
    from oracle import cpu_ref as R
    medium, agents = R.synthetic_init(W, H, 0.15, seed=seed)
    medium[1] = medium[1].astype(np.float32)
    agents[:2] = from_q32(to_q32(agents[:2]))
    alive = np.nonzero(agents[2] > 0)[0]
    agents[3] = agents[3].astype(np.float32)
    agents[3, alive[::3]] = np.float32(0.9)             # a step costs 0.24 + 0.01·|move| at most: 0.9 stays above 0.5
    return medium, agents, alive[::3]


def test_env_steps_with_births_equal_steps_plus_apply_births():
    W, H, steps = 64, 48, 40                            # 40 steps: the claim plane's epoch wraps
    medium, agents, rich = _seeded_world(W, H)
    assert agents.shape[1] == W * H and 0 < len(rich) < (agents[2] == 0).sum()
    kw = dict(scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1), deposit=12.0)
    dyn = lambda born: die.Dynamics(agents_die=True, agents_born=born, init_agent_ratio=0.15)
    A = die.Env.from_numpy(medium, agents, dyn(True), device=DEV, seed=21)
    B = die.Env.from_numpy(medium, agents, dyn(False), device=DEV, seed=21, sync=False)
    ag_a, ag_b = (die.PhysarumAgent(max_agents=A.agents.N, seed=3, **kw) for _ in range(2))
    k0 = int((agents[2] > 0).sum())
    counts = [k0]
    for i in range(steps):
        _, rew_a, _, _, info = A.step(ag_a.forward(A._get_current_obs))
        _, res, *_ = B.step(ag_b.forward(B._get_current_obs))
        B.apply_births(step=i, result=res)
        rew_b, n_b = B.read_result(res)
        a_np = A.agents.to_numpy()
        assert np.array_equal(A.medium.to_numpy(), B.medium.to_numpy()), i
        assert np.array_equal(a_np, B.agents.to_numpy()), i
        assert rew_a == rew_b and info['num_agents'] == n_b, i
        assert info['num_agents'] == int((a_np[2] > 0).sum()), i
        counts.append(info['num_agents'])
    assert counts[1] >= k0 + 1                           # the rich agents bred at step 1 (nobody starves from 0.9 in one step)
    assert A._pic is None and A.agents.slot is None
    assert np.array_equal(ag_a.direction_rads_numpy(), ag_b.direction_rads_numpy())
    assert min(np.diff(counts)) < 0                      # and the death pressure is still there


# ---------------------------------------------------------------- 3. batched replicas
REFERENCE_DYNAMICS = dict(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8)     # examples/learning_agents.py
STEPS = 40


def _run_alone(env, agent, steps):
    obs, rew, alive = env._get_current_obs, [], []
    for _ in range(steps):
        obs, rw, _, _, info = env.step(agent.forward(obs))
        rew.append(rw); alive.append(info['num_agents'])
    return np.array(rew), np.array(alive)


def _assert_replica_is(benv, r, env, rew, alive, want_rew, want_alive):
    m, a = benv.replica_numpy(r)
    assert np.array_equal(m, env.medium.to_numpy()), r
    assert np.array_equal(a, env.agents.to_numpy()), r
    assert np.array_equal(rew[:, r], want_rew), r
    assert np.array_equal(alive[:, r], want_alive), r


def _grows_and_shrinks(benv, alive, k0):
    """At some step a replica gains agents and at some step a replica loses some."""
    steps = np.diff(np.vstack([np.asarray(k0)[None], alive]), axis=0)
    assert (steps > 0).any() and (steps < 0).any(), steps.T


def _initial_alive(benv):
    return [int(benv.alive[r, :benv.n[r]].sum().item()) for r in range(benv.R)]


def _nca_population(R, seed=5, **model_kw):
    """Candidates of three kinds (tests/test_gpu_batch_lifecycle.py): all-zero weights (no action cost: every agent only feeds, grows
    past the threshold and breeds — the colony GROWS by construction), saturated weights (a cost above any agent's food: the
    colony SHRINKS to nothing within a few steps) and init_weights() ones."""
    torch.manual_seed(seed)
    template = die.NeuralAutomataAgent(scale=0.01, deposit=60.0, kernel_sizes=(3, 3), **model_kw)
    rows = []
    for r in range(R):
        template.model.init_weights()
        v = torch.nn.utils.parameters_to_vector(template.model.parameters()).detach().clone()
        rows.append(torch.zeros_like(v) if r % 3 == 0 else v * 50.0 if r % 3 == 1 else v)
    return template, torch.stack(rows)


def _born_dyn(**kw):
    return die.Dynamics(agents_die=True, agents_born=True, **kw)


@pytest.mark.parametrize('W,H,R,N,model_kw', [
    (64, 48, 5, 900, {}),                                                        # narrow; seeds 11..15 seed different numbers of agents
    (32, 32, 3, 400, dict(hidden_channels=8, hidden_activation='tanh')),         # wide: 3 -> 8 -> 3
], ids=['narrow', 'wide'])
def test_nca_replicas_breed_like_their_stand_alone_envs(W, H, R, N, model_kw):
    dyn_kw = dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15)
    template, rows = _nca_population(R, **model_kw)
    benv = BatchedEnv((W, H), _born_dyn(**dyn_kw), replicas=R, seed=11, max_agents=N)
    k0 = _initial_alive(benv)
    assert len(set(k0)) > 1 and max(k0) < N
    bag = BatchedNeuralAutomataAgent(benv, template, rows)
    first = benv.run(bag, STEPS).clone()
    rew, alive = BatchedEnv.read_results(first)
    for r in range(R):
        env = die.Env((W, H), _born_dyn(**dyn_kw), seed=11 + r, max_agents=N)
        ag = BatchedNeuralAutomataAgent.unpack(template, rows[r]).to(env.device)
        want_rew, want_alive = _run_alone(env, ag, STEPS)
        _assert_replica_is(benv, r, env, rew, alive, want_rew, want_alive)
    _grows_and_shrinks(benv, alive, k0)
    assert alive[-1, 0] > k0[0] and alive[-1, 1] == 0       # the zero-weight colony grew, the saturated one died out
    benv.reset()                                            # across reset(): the world step starts over, so the run repeats
    assert torch.equal(benv.run(bag, STEPS), first)


def test_physarum_replicas_breed_like_their_stand_alone_envs():
    W, H, R, N = 64, 48, 4, 1200
    dyn_kw = dict(init_agent_ratio=0.15, boundary=die.BoundaryCondition.limit)
    kw = dict(scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1), deposit=12.0)      # a step costs 0.24: the poorer cells starve their agents
    benv = BatchedEnv((W, H), _born_dyn(**dyn_kw), replicas=R, seed=40, max_agents=N)
    k0 = _initial_alive(benv)
    bag = BatchedPhysarumAgent(benv, seed=7, **kw)
    rew, alive = BatchedEnv.read_results(benv.run(bag, STEPS))
    for r in range(R):
        env = die.Env((W, H), _born_dyn(**dyn_kw), seed=40 + r, max_agents=N)
        ag = die.PhysarumAgent(max_agents=N, seed=7 + r, **kw)
        want_rew, want_alive = _run_alone(env, ag, STEPS)
        _assert_replica_is(benv, r, env, rew, alive, want_rew, want_alive)
        assert np.array_equal(bag.direction_rads_numpy(r), ag.direction_rads_numpy()), r       # headings: a newborn takes its slot's
    _grows_and_shrinks(benv, alive, k0)                     # seeds 40..43: the well-fed half breeds at step 1, starvation follows


def test_episodes_and_recorded_actions():
    """episodes=2: replica c·2 + e is candidate c on world e; and a second batch driven by step_action of the recorded actions
    stays bit-equal, births included (both count world steps)."""
    W, H, R, N, E = 32, 32, 4, 400, 2
    dyn_kw = dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15)
    template, rows = _nca_population(R // E)
    seeds = [3, 4, 3, 4]
    make = lambda: BatchedEnv((W, H), _born_dyn(**dyn_kw), replicas=R, seeds=seeds, max_agents=N)
    one, two = make(), make()
    k0 = _initial_alive(one)
    pop = BatchedNeuralAutomataAgent(one, template, rows, episodes=E)
    buf = torch.zeros((3, R, one.Nmax), dtype=torch.float32, device=one.device)
    out = torch.empty((STEPS, R, 2), dtype=torch.float64, device=one.device)
    for t in range(STEPS):
        one.step(pop, out[t], action=buf)
        second = two.step_action(buf)
        assert torch.equal(out[t].view(torch.int64), second.view(torch.int64)), t
        assert torch.equal(one._state, two._state), t
    rew, alive = BatchedEnv.read_results(out)
    for r in range(R):
        env = die.Env((W, H), _born_dyn(**dyn_kw), seed=seeds[r], max_agents=N)
        ag = BatchedNeuralAutomataAgent.unpack(template, rows[r // E]).to(env.device)
        want_rew, want_alive = _run_alone(env, ag, STEPS)
        _assert_replica_is(one, r, env, rew, alive, want_rew, want_alive)
    _grows_and_shrinks(one, alive, k0)


def test_per_replica_regime_goes_through_env():
    """Large worlds step one Env per replica: forced onto a small world, replica r is still the stand-alone run."""
    W, H, R, N = 64, 48, 3, 900
    dyn_kw = dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15)
    template, rows = _nca_population(R)
    benv = BatchedEnv((W, H), _born_dyn(**dyn_kw), replicas=R, seed=11, max_agents=N, per_replica=True)
    small = BatchedEnv((W, H), _born_dyn(**dyn_kw), replicas=R, seed=11, max_agents=N, per_replica=False)
    k0 = _initial_alive(small)
    a = benv.run(BatchedNeuralAutomataAgent(benv, template, rows), 12)
    b = small.run(BatchedNeuralAutomataAgent(small, template, rows), 12)
    assert torch.equal(a, b)
    for r in range(R):
        for u, v in zip(benv.replica_numpy(r), small.replica_numpy(r)):
            assert np.array_equal(u, v), r
    assert (BatchedEnv.read_results(a)[1][-1] > np.array(k0)).any()


# ---------------------------------------------------------------- 4. search
def test_one_pgpe_generation_under_births():
    """ask -> reset + run -> tell: every candidate's fitness is the summed rewards of its row run stand-alone."""
    W, H, R, T, N = 64, 64, 6, 16, 1500
    dyn = lambda: _born_dyn(**REFERENCE_DYNAMICS)
    template = die.NeuralAutomataAgent(scale=0.01, deposit=20.0, kernel_sizes=(3, 3))
    benv = BatchedEnv((W, H), dyn(), replicas=R, seeds=[9] * R, max_agents=N)
    k0 = _initial_alive(benv)
    pop = BatchedNeuralAutomataAgent(benv, template)
    s = PGPE(R, center_init=pop.parameters[0].cpu(), radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1,
             optimizer_config=dict(max_speed=0.1, momentum=0.9), seed=11, device='cuda')
    s.ask(pop.parameters)
    rows = pop.parameters.cpu()
    benv.run(pop, 3)                                         # a used batch: reset() must put the world step back to 0
    benv.reset()
    res = benv.run(pop, T)
    s.tell(res)
    _, alive = BatchedEnv.read_results(res)
    assert (np.diff(np.vstack([np.asarray(k0)[None], alive]), axis=0) > 0).any()          # births shaped the fitness
    fitness = s.fitness.cpu().tolist()
    for r in range(R):
        env = die.Env((W, H), dyn(), seed=9, max_agents=N)
        ag = BatchedNeuralAutomataAgent.unpack(template, rows[r]).to(env.device)
        want_rew, _ = _run_alone(env, ag, T)
        assert fitness[r] == sum(want_rew.tolist()), r


# ---------------------------------------------------------------- 5. refusals
def _snapshot(env):
    torch.cuda.synchronize()
    return env.medium.to_numpy(), env.agents.to_numpy(), env._steps, env.medium.epoch


def _unchanged(env, snap):
    now = _snapshot(env)
    return np.array_equal(now[0], snap[0]) and np.array_equal(now[1], snap[1]) and now[2:] == snap[2:]


def test_refusals_leave_the_state_untouched():
    W, H = 64, 48
    born = lambda **kw: die.Dynamics(agents_born=True, **kw)
    with pytest.raises(ValueError, match='sort_every'):
        die.Env((W, H), born(), seed=1, sort_every=8)
    with pytest.raises(NotImplementedError, match='compat'):
        die.Env((W, H), born(agents_die=True, compat='reference'), seed=1)
    with pytest.raises(ValueError, match='born_spread'):
        die.Env((W, H), born(born_spread=0.75), seed=1)
    env = die.Env((W, H), born(agents_die=True), seed=1)
    assert env._sort_every == 0 and not env._all_alive
    agent = die.PhysarumAgent(max_agents=env.agents.N, seed=2)
    snap = _snapshot(env)
    with pytest.raises(NotImplementedError, match='agents_born'):
        env.run(agent, 62, graph=True)
    with pytest.raises(NotImplementedError, match='agents_born'):
        env.differentiable_step(torch.zeros((3, env.agents.N), dtype=torch.float32, device=env.device))
    with pytest.raises(ValueError, match='slot order'):
        env.sort_agents()
    assert _unchanged(env, snap)
    # a world whose arrays were re-sorted cannot breed: apply_births refuses, and so does a step once the flag is set
    other = die.Env((W, H), die.Dynamics(agents_die=True), seed=1, sort_every=1)
    other.step(die.PhysarumAgent(max_agents=other.agents.N, seed=2).forward(other._get_current_obs))
    assert other.agents.slot is not None
    snap = _snapshot(other)
    with pytest.raises(ValueError, match='slot order'):
        other.apply_births()
    assert _unchanged(other, snap)
    from die_amd.dist import DistEnv
    with pytest.raises(NotImplementedError, match='agents_born'):
        DistEnv((256, 256), (1, 1), born(), probe_reach=11, device=DEV)
    benv = BatchedEnv((32, 32), born(agents_die=True), replicas=2, seed=1, max_agents=300)
    state = benv._state.clone()
    with pytest.raises(NotImplementedError, match='agents_born'):
        benv.differentiable_step(torch.zeros((3, 2, benv.Nmax), dtype=torch.float32, device=benv.device))
    assert torch.equal(benv._state, state) and benv._steps == 0


def test_a_world_of_tile_binned_size_takes_the_classic_step(monkeypatch):
    """From PIC_MIN_CELLS cells on a world takes the tile-binned step when it applies; with agents_born it does not apply.  (The
    threshold is forced down to a 256 x 256 world: one step of 2^23 cells with W·H slots is too slow for a test.)"""
    monkeypatch.setattr(die.Env, 'PIC_MIN_CELLS', 1 << 16)
    monkeypatch.setattr(die.Env, 'PIC_MIN_CELLS_64', 1 << 16)
    W = H = 256
    kw = dict(scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
    plain = die.Env((W, H), die.Dynamics(), seed=3, max_agents='alive', sort_every=0)
    plain.step(die.PhysarumAgent(max_agents=plain.agents.N, seed=2, **kw).forward(plain._get_current_obs))
    assert plain._pic is not None                           # the same world without births does take the binned step
    env = die.Env((W, H), die.Dynamics(agents_born=True), seed=3, max_agents='alive')
    _, _, _, _, info = env.step(die.PhysarumAgent(max_agents=env.agents.N, seed=2, **kw).forward(env._get_current_obs))
    assert env._pic is None and env._sort_every == 0
    assert info['num_agents'] == env.agents.N               # the 'alive' layout without agents_die: no free slot, nobody is born
