"""Batched replicas in the fixed slot layout (BatchedEnv(max_agents=N)) and reseeded worlds (reset(seed=...), die_init_batch):
replica r must be, bit for bit, the stand-alone `Env(field_size, dynamics, seed=seeds[r], max_agents=N)` driven by the matching
agent — fields, every agent slot, per-step reward and num_agents — in both regimes, with NCA populations, a food flow and the
death pressure; a reseeded batch must be the freshly constructed batch of its seeds; the searchers' reseeding generation must be
the generation driven by hand on fresh batches."""
import numpy as np
import pytest
import torch
import ctypes as C

import die_amd as die
from die_amd import _lib
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent, BatchedPhysarumAgent
from die_amd.data_init import DataInitializer
from die_amd.device_array import DeviceAgents, DeviceMedium, _ptr, stream_ptr
from die_amd.search import CMAES, PGPE

pytestmark = pytest.mark.gpu

REFERENCE_DYNAMICS = dict(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8)     # examples/learning_agents.py


def _run_alone(env, agent, steps):
    obs, rew, alive = env._get_current_obs, [], []
    for _ in range(steps):
        obs, rw, _, _, info = env.step(agent.forward(obs))
        rew.append(rw)
        alive.append(info['num_agents'])
    return np.array(rew), np.array(alive)


def _assert_replica_is(benv, r, env, rew=None, alive=None, want_rew=None, want_alive=None):
    m, a = benv.replica_numpy(r)
    assert np.array_equal(m, env.medium.to_numpy()), r
    assert np.array_equal(a, env.agents.to_numpy()), r
    if rew is not None:
        assert np.array_equal(rew[:, r], want_rew), r
        assert np.array_equal(alive[:, r], want_alive), r


def _seeded_counts(W, H, dyn, seeds):
    return [die.Env((W, H), dyn, seed=q, max_agents='alive').agents.N for q in seeds]


def _slots(kind, W, H, dyn, seeds):
    """max_agents of a case: None (W·H, the reference's default) or the tightest N that holds every seeded world."""
    return None if kind == 'full' else max(_seeded_counts(W, H, dyn, seeds))


def _physarum_kw(W, H, deposit):
    return dict(scale=1.53 / (max(W, H) - 1), sense_offset=10.2 / (max(W, H) - 1), deposit=deposit)


def _wave(W, H):
    return lambda: die.WaveSequence((W, H), dt=0.01).get_flow_operator(scale=0.5, decay=0.5)


# ---------------------------------------------------------------- the fixed layout, no reseeding
@pytest.mark.parametrize('W,H,R,f16,boundary,slots,agents_die,per_replica', [
    (64, 48, 3, False, 'wrap', 'full', False, False),
    (96, 64, 4, True, 'limit', 'tight', False, False),
    (64, 48, 3, False, 'limit', 'tight', True, False),
    (64, 48, 4, True, 'wrap', 'full', True, False),
    (96, 64, 3, False, 'wrap', 'full', False, True),            # the large-world regime (one Env per replica) forced on a small world
])
def test_fixed_layout_physarum_equals_stand_alone(W, H, R, f16, boundary, slots, agents_die, per_replica):
    """40 steps: the claim plane's 5-bit epoch wraps."""
    seed, agent_seed, steps = 40, 7, 40
    dt = torch.float16 if f16 else torch.float32
    dyn = lambda: die.Dynamics(agents_die=agents_die, init_agent_ratio=0.15, boundary=die.BoundaryCondition(boundary))
    N = _slots(slots, W, H, dyn(), [seed + r for r in range(R)])
    kw = _physarum_kw(W, H, 12.0 if agents_die else 4.0)
    benv = BatchedEnv((W, H), dyn(), replicas=R, seed=seed, field_dtype=dt, per_replica=per_replica, max_agents=N)
    assert benv.per_replica == per_replica and benv.n == [N or W * H] * R
    bag = BatchedPhysarumAgent(benv, seed=agent_seed, **kw)
    rew, alive = BatchedEnv.read_results(benv.run(bag, steps))
    benv.check()
    for r in range(R):
        env = die.Env((W, H), dyn(), seed=seed + r, max_agents=N, field_dtype=dt)
        assert env.agents.N == benv.n[r]
        ag = die.PhysarumAgent(max_agents=env.agents.N, seed=agent_seed + r, **kw)
        want_rew, want_alive = _run_alone(env, ag, steps)
        _assert_replica_is(benv, r, env, rew, alive, want_rew, want_alive)
        assert np.array_equal(bag.direction_rads_numpy(r), ag.direction_rads_numpy()), r
        if agents_die:
            assert alive[-1, r] < alive[0, r], r                  # deaths happened: the lifecycle path is covered


def _nca_population(R, deposit=60.0, seed=5):
    torch.manual_seed(seed)
    template = die.NeuralAutomataAgent(scale=0.01, deposit=deposit, kernel_sizes=(3, 3))
    rows = []
    for r in range(R):
        template.model.init_weights()
        rows.append(torch.nn.utils.parameters_to_vector(template.model.parameters()).detach().clone())
    return template, torch.stack(rows)


@pytest.mark.parametrize('slots,agents_die,flow,per_replica', [
    ('full', False, False, False),
    ('tight', True, True, False),                                 # death pressure and a food flow together
    ('full', True, False, True),
])
def test_fixed_layout_nca_population_equals_stand_alone(slots, agents_die, flow, per_replica):
    W, H, R, seed, steps = (96, 96, 4, 11, 40) if not per_replica else (128, 96, 3, 11, 33)
    template, rows = _nca_population(R)
    dyn = lambda: die.Dynamics(agents_die=agents_die, init_agent_ratio=0.15, **dict(REFERENCE_DYNAMICS, food_infinite=not flow),
                               **(dict(op_food_flow=_wave(W, H)()) if flow else {}))
    N = _slots(slots, W, H, dyn(), [seed + r for r in range(R)])
    benv = BatchedEnv((W, H), dyn(), replicas=R, seed=seed, per_replica=per_replica, max_agents=N)
    bag = BatchedNeuralAutomataAgent(benv, template, rows)
    rew, alive = BatchedEnv.read_results(benv.run(bag, steps))
    for r in range(R):
        env = die.Env((W, H), dyn(), seed=seed + r, max_agents=N)
        ag = BatchedNeuralAutomataAgent.unpack(template, rows[r]).to(env.device)
        want_rew, want_alive = _run_alone(env, ag, steps)
        _assert_replica_is(benv, r, env, rew, alive, want_rew, want_alive)
        assert np.array_equal(bag.render(r), ag.render()[0]), r


# ---------------------------------------------------------------- reseeding
@pytest.mark.parametrize('stride', [0, 1])
@pytest.mark.parametrize('f16,agents_die,flow,per_replica', [
    (False, False, False, False),
    (True, True, True, False),
    (False, True, False, True),
])
def test_reset_with_seed_is_a_fresh_batch(stride, f16, agents_die, flow, per_replica):
    W, H, R, N, steps = 64, 48, 4, 700, 12
    dt = torch.float16 if f16 else torch.float32
    dyn = lambda: die.Dynamics(agents_die=agents_die, init_agent_ratio=0.15, food_infinite=not flow,
                               **(dict(op_food_flow=_wave(W, H)()) if flow else {}))
    kw = _physarum_kw(W, H, 12.0 if agents_die else 4.0)
    d = dyn()
    benv = BatchedEnv((W, H), d, replicas=R, seed=3, field_dtype=dt, per_replica=per_replica, max_agents=N)
    start = [benv.replica_numpy(r) for r in range(R)]
    k0 = getattr(d.op_food_flow, '_k', None)
    benv.run(BatchedPhysarumAgent(benv, seed=1, **kw), steps)
    s = 1000
    benv.reset(seed=s, seed_stride=stride)
    seeds = [s + r * stride for r in range(R)]
    assert benv.seeds == seeds and benv._steps == 0 and getattr(d.op_food_flow, '_k', None) == k0
    if not per_replica:
        assert benv.epoch == 1
    d2 = dyn()
    fresh = BatchedEnv((W, H), d2, replicas=R, seeds=seeds, field_dtype=dt, per_replica=per_replica, max_agents=N)
    for r in range(R):
        m, a = benv.replica_numpy(r)
        m2, a2 = fresh.replica_numpy(r)
        assert np.array_equal(m, m2) and np.array_equal(a, a2), r
        if stride == 0:                                           # one world for every candidate
            m0, a0 = benv.replica_numpy(0)
            assert np.array_equal(m, m0) and np.array_equal(a, a0), r
    benv.check()
    # further steps with fresh agents: the fresh batch and the stand-alone Envs of those seeds
    rew, alive = BatchedEnv.read_results(benv.run(BatchedPhysarumAgent(benv, seed=9, **kw), steps))
    rew2, alive2 = BatchedEnv.read_results(fresh.run(BatchedPhysarumAgent(fresh, seed=9, **kw), steps))
    assert np.array_equal(rew, rew2) and np.array_equal(alive, alive2)
    for r in range(R):
        env = die.Env((W, H), dyn(), seed=seeds[r], max_agents=N, field_dtype=dt)
        want_rew, want_alive = _run_alone(env, die.PhysarumAgent(max_agents=N, seed=9 + r, **kw), steps)
        _assert_replica_is(benv, r, env, rew, alive, want_rew, want_alive)
    # a plain reset(): the construction worlds again, bit for bit
    benv.reset()
    for r in range(R):
        m, a = benv.replica_numpy(r)
        assert np.array_equal(m, start[r][0]) and np.array_equal(a, start[r][1]), r


def test_reset_with_seed_refused_on_alive_layout():
    benv = BatchedEnv((64, 48), die.Dynamics(init_agent_ratio=0.15), replicas=2, seed=3)
    before = benv._state.clone()
    with pytest.raises(ValueError, match='max_agents'):
        benv.reset(seed=5)
    assert torch.equal(before, benv._state) and benv.seeds == [3, 4]


def test_overflow_is_reported_and_clipped_like_die_init_agents():
    W, H = 64, 48
    dyn = die.Dynamics(init_agent_ratio=0.15)
    cand = list(range(100, 116))
    k = dict(zip(cand, _seeded_counts(W, H, dyn, cand)))
    low = sorted(cand, key=lambda q: k[q])[:2]
    big = max(cand, key=lambda q: k[q])
    N = max(k[q] for q in low)
    assert k[big] > N
    benv = BatchedEnv((W, H), dyn, replicas=2, seeds=low, max_agents=N)
    benv.check()
    benv.reset(seed=big, seed_stride=0)
    with pytest.raises(ValueError, match=f'replica 0 \\(seed {big}\\).*replica 1 \\(seed {big}\\)'):
        benv.check()
    benv.check()                                                  # the flags were cleared
    # die_init_agents on a stand-alone medium of that seed clips the same way
    dev = benv.device
    medium = DeviceMedium((W, H), dev)
    DataInitializer.init_medium(medium, dyn.init_agent_ratio, big)
    agents = DeviceAgents(N, dev)
    ws = DataInitializer.workspace((W, H), N, dev)
    count = torch.zeros(2, dtype=torch.int64, device=dev)
    _lib.check(_lib.lib.die_init_agents(C.byref(medium.c_struct()), C.byref(agents.c_struct()), big, _ptr(count), _ptr(ws), ws.numel(),
                                        stream_ptr(dev)), 'die_init_agents')
    assert count.tolist() == [N, 1]
    for r in range(2):
        m, a = benv.replica_numpy(r)
        assert np.array_equal(m, medium.to_numpy()) and np.array_equal(a, agents.to_numpy()), r
    assert benv._counts[:, 0].tolist() == [N, N]


class _NoHostRead:
    def __enter__(self):
        self.saved = [(torch.Tensor, n, getattr(torch.Tensor, n)) for n in ('item', 'cpu', 'tolist')]
        self.saved.append((torch.cuda, 'synchronize', torch.cuda.synchronize))

        def boom(*a, **k):
            raise AssertionError('host read')
        for obj, name, _ in self.saved:
            setattr(obj, name, boom)
        return self

    def __exit__(self, *exc):
        for obj, name, fn in self.saved:
            setattr(obj, name, fn)


def test_reseeding_reads_nothing_back():
    W, H, R = 64, 48, 4
    template, rows = _nca_population(R)
    benv = BatchedEnv((W, H), die.Dynamics(init_agent_ratio=0.15, **REFERENCE_DYNAMICS), replicas=R, seed=3, max_agents=None)
    pop = BatchedNeuralAutomataAgent(benv, template, rows)
    searcher = PGPE(R, center_init=rows[0], radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1,
                    device=benv.device).for_population(pop, 5, reseed=77, reseed_stride=1)
    searcher.step()                                               # (first-call set-up outside the guard)
    torch.cuda.synchronize()
    used = torch.cuda.memory_allocated(benv.device)
    with _NoHostRead():
        benv.reset(seed=5, seed_stride=1)
        assert torch.cuda.memory_allocated(benv.device) == used   # no allocation either
        searcher.step()
    benv.check()
    assert searcher.iter == 2 and benv.seeds == [77 + R + r for r in range(R)]


def _searcher(kind, R, rows):
    if kind == 'pgpe':
        return PGPE(R, center_init=rows[0], radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1, optimizer='clipup',
                    optimizer_config=dict(max_speed=0.15, momentum=0.9), seed=4)
    return CMAES(R, center_init=rows[0], stdev_init=0.1, seed=4)


@pytest.mark.parametrize('kind,stride', [('pgpe', 0), ('pgpe', 1), ('cmaes', 0), ('cmaes', 1)])
def test_searcher_reseeding_equals_generations_by_hand(kind, stride):
    W, H, R, T, G, base = 64, 48, 4, 6, 3, 500
    template, rows = _nca_population(R)
    dyn = die.Dynamics(init_agent_ratio=0.15, **REFERENCE_DYNAMICS)
    benv = BatchedEnv((W, H), dyn, replicas=R, seed=3, max_agents=None)
    pop = BatchedNeuralAutomataAgent(benv, template, rows)
    auto = _searcher(kind, R, rows).for_population(pop, T, reseed=base, reseed_stride=stride)
    auto.run(G)
    hand = _searcher(kind, R, rows)
    params = torch.empty((R, pop.P), dtype=torch.float32, device=benv.device)
    for g in range(G):
        hand.ask(params)
        b = BatchedEnv((W, H), dyn, replicas=R, seeds=[base + g * R + r * stride for r in range(R)], max_agents=None)
        hand.tell(b.run(BatchedNeuralAutomataAgent(b, template, params), T))
    assert torch.equal(auto.history(), hand.history())
    assert torch.equal(auto.center.cpu(), hand.center.cpu())
    assert torch.equal(auto._best.cpu(), hand._best.cpu()) and torch.equal(auto._pop_best.cpu(), hand._pop_best.cpu())
    assert benv.seeds == [base + (G - 1) * R + r * stride for r in range(R)]
