"""Episodes on the GPU: a population of C candidates with E episodes each on R = C·E replicas (replica c·E + e is candidate c on
its e-th world) must be, bit for bit, the population without episodes fed the expanded (R, P) rows, and the stand-alone run of
each replica; `reset(seeds=list)` must be the freshly constructed batch of that list; the searchers' generation with episodes
must be the generation driven by hand with the host fold of tests/episodes_model.py; and E = 1 must be today's path."""
import numpy as np
import pytest
import torch

import die_amd as die
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent, BatchedPhysarumPopulation, ParameterSpace, episode_seeds
from die_amd.search import CMAES, PGPE
from tests import episodes_model as M

pytestmark = pytest.mark.gpu

REFERENCE_DYNAMICS = dict(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8)     # examples/learning_agents.py
C_, E = 4, 3
SEEDS = [11, 40, 7, 7, 93, 12, 58, 3, 40, 21, 5, 66]                # no arithmetic pattern; 7 and 40 repeat


def _run_alone(env, agent, steps):
    obs, rew, alive = env._get_current_obs, [], []
    for _ in range(steps):
        obs, rw, _, _, info = env.step(agent.forward(obs))
        rew.append(rw)
        alive.append(info['num_agents'])
    return np.array(rew), np.array(alive)


def _wave(W, H):
    return die.WaveSequence((W, H), dt=0.01).get_flow_operator(scale=0.5, decay=0.5)


def _nca_rows(n, deposit=60.0, seed=5):
    torch.manual_seed(seed)
    template = die.NeuralAutomataAgent(scale=0.01, deposit=deposit, kernel_sizes=(3, 3))
    rows = []
    for _ in range(n):
        template.model.init_weights()
        rows.append(torch.nn.utils.parameters_to_vector(template.model.parameters()).detach().clone())
    return template, torch.stack(rows)


def _assert_same_batch(a: BatchedEnv, b: BatchedEnv):
    assert a.epoch == b.epoch and a.n == b.n
    assert torch.equal(a._state, b._state)                       # every plane and every agent array of every replica
    assert torch.equal(a.chem, b.chem)


def _assert_same_worlds(a: BatchedEnv, b: BatchedEnv):
    """Two batches that were seeded, not stepped alike: everything a step reads (the spare chem plane is not part of a world)."""
    assert a.epoch == b.epoch and a.n == b.n
    for name in ('food', 'chem', 'x', 'y', 'alive', 'agent_food'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for r in range(a.R):
        for x, y in zip(a.replica_numpy(r), b.replica_numpy(r)):  # (the claim plane as occupancy, as Env.medium.to_numpy() shows it)
            assert np.array_equal(x, y), r


# ---------------------------------------------------------------------------------------------------- 1. NCA
@pytest.mark.parametrize('case', ['agents_die_wave_flow', 'fp16'])
def test_nca_episodes_equal_expanded_rows_and_stand_alone_runs(case):
    W, H, T = 64, 48, 36                                          # 36 steps: the claim plane's 5-bit epoch wraps
    die_flow = case == 'agents_die_wave_flow'
    dt = torch.float16 if case == 'fp16' else torch.float32
    slots = 'alive' if die_flow else None
    dyn = lambda: die.Dynamics(agents_die=die_flow, init_agent_ratio=0.15, **dict(REFERENCE_DYNAMICS, food_infinite=not die_flow),
                               **(dict(op_food_flow=_wave(W, H)) if die_flow else {}))
    template, rows = _nca_rows(C_)
    assert len({tuple(r.tolist()) for r in rows}) == C_           # distinct candidates
    env_e = BatchedEnv((W, H), dyn(), replicas=C_ * E, seeds=SEEDS, field_dtype=dt, max_agents=slots)
    env_x = BatchedEnv((W, H), dyn(), replicas=C_ * E, seeds=SEEDS, field_dtype=dt, max_agents=slots)
    assert not env_e.per_replica
    pop_e = BatchedNeuralAutomataAgent(env_e, template, rows, episodes=E)
    pop_x = BatchedNeuralAutomataAgent(env_x, template, rows.repeat_interleave(E, dim=0))
    assert (pop_e.R, pop_e.candidates, pop_e.episodes) == (12, 4, 3) and tuple(pop_e.parameters.shape) == (4, pop_e.P)
    res_e, res_x = env_e.run(pop_e, T), env_x.run(pop_x, T)
    assert torch.equal(res_e, res_x)                              # both result words of every step and replica
    _assert_same_batch(env_e, env_x)
    rew, alive = BatchedEnv.read_results(res_e)
    if die_flow:
        assert (alive[-1] < alive[0]).any()                       # deaths happened
    for c in range(C_):                                           # one replica per candidate against the stand-alone run
        r = c * E + (c + 1) % E
        env = die.Env((W, H), dyn(), seed=SEEDS[r], max_agents=slots, field_dtype=dt)
        ag = BatchedNeuralAutomataAgent.unpack(template, rows[c]).to(env.device)
        want_rew, want_alive = _run_alone(env, ag, T)
        m, a = env_e.replica_numpy(r)
        assert np.array_equal(m, env.medium.to_numpy()) and np.array_equal(a, env.agents.to_numpy()), r
        assert np.array_equal(rew[:, r], want_rew) and np.array_equal(alive[:, r], want_alive), r
        assert np.array_equal(pop_e.render(r), ag.render()[0]), r
    # replicas 2 and 3 share seed 7 but belong to candidates 0 and 1: the row index matters
    assert not np.array_equal(env_e.replica_numpy(2)[0][2], env_e.replica_numpy(3)[0][2])
    # an in-place write to the (C, P) matrix is seen by the next step
    pop_e.parameters[1].mul_(0.5)
    pop_x.parameters[3:6].mul_(0.5)
    assert torch.equal(env_e.step(pop_e), env_x.step(pop_x))
    _assert_same_batch(env_e, env_x)


def test_nca_episodes_in_the_large_world_regime():
    W, H, T, seeds = 64, 48, 5, [9, 2, 2, 30]
    dyn = lambda: die.Dynamics(init_agent_ratio=0.15, **REFERENCE_DYNAMICS)
    template, rows = _nca_rows(2)
    benv = BatchedEnv((W, H), dyn(), replicas=4, seeds=seeds, per_replica=True, max_agents=None)
    pop = BatchedNeuralAutomataAgent(benv, template, rows, episodes=2)
    rew, _ = BatchedEnv.read_results(benv.run(pop, T))
    for r in range(4):
        env = die.Env((W, H), dyn(), seed=seeds[r], max_agents=None)
        want_rew, _ = _run_alone(env, BatchedNeuralAutomataAgent.unpack(template, rows[r // 2]).to(env.device), T)
        m, a = benv.replica_numpy(r)
        assert np.array_equal(m, env.medium.to_numpy()) and np.array_equal(a, env.agents.to_numpy()), r
        assert np.array_equal(rew[:, r], want_rew), r
    benv.reset(seeds=[5, 5, 8, 1])                                # Env.reset(seed=s_r) per replica
    fresh = BatchedEnv((W, H), dyn(), replicas=4, seeds=[5, 5, 8, 1], per_replica=True, max_agents=None)
    assert benv.seeds == [5, 5, 8, 1]
    for r in range(4):
        for x, y in zip(benv.replica_numpy(r), fresh.replica_numpy(r)):
            assert np.array_equal(x, y), r


# ---------------------------------------------------------------------------------------------------- 2. Physarum
def test_physarum_episodes_equal_expanded_rows_and_stand_alone_runs():
    size, T = 64, 20
    rng = np.random.RandomState(3)
    unit = rng.uniform(0.05, 0.95, (C_, 6)).astype(np.float32)
    space = ParameterSpace()
    dyn = lambda: die.Dynamics()
    env_e = BatchedEnv((size, size), dyn(), replicas=C_ * E, seeds=SEEDS)
    env_x = BatchedEnv((size, size), dyn(), replicas=C_ * E, seeds=SEEDS)
    pop_e = BatchedPhysarumPopulation(env_e, parameters=unit, space=space, seed=7, episodes=E)
    pop_x = BatchedPhysarumPopulation(env_x, parameters=np.repeat(unit, E, axis=0), space=space, seed=7)
    assert (pop_e.R, pop_e.candidates, pop_e.episodes) == (12, 4, 3)
    assert tuple(pop_e.parameters.shape) == (4, 6) and pop_e.values().shape == (4, 6)
    assert np.array_equal(pop_e.values(), space.decode(unit))
    te, tx = pop_e.table(), pop_x.table()
    assert te.shape == (12,) and te.tobytes() == tx.tobytes()
    for r in range(12):
        assert te[r].tobytes() == te[(r // E) * E].tobytes(), r   # row r of the table = the decode of row r // E
        assert np.array_equal(pop_e.direction_rads_numpy(r), pop_x.direction_rads_numpy(r)), r    # headings per replica (seed + r)
    res_e, res_x = env_e.run(pop_e, T), env_x.run(pop_x, T)
    assert torch.equal(res_e, res_x)
    _assert_same_batch(env_e, env_x)
    assert torch.equal(pop_e._hd_hi, pop_x._hd_hi) and torch.equal(pop_e._hd_lo, pop_x._hd_lo)
    rew, alive = BatchedEnv.read_results(res_e)
    for c in range(C_):
        r = c * E + (c + 2) % E
        env = die.Env((size, size), dyn(), seed=SEEDS[r], max_agents='alive')
        ag = pop_e.replica_agent(r)
        want_rew, want_alive = _run_alone(env, ag, T)
        m, a = env_e.replica_numpy(r)
        assert np.array_equal(m, env.medium.to_numpy()) and np.array_equal(a, env.agents.to_numpy()), r
        assert np.array_equal(rew[:, r], want_rew) and np.array_equal(alive[:, r], want_alive), r
        assert np.array_equal(pop_e.direction_rads_numpy(r), ag.direction_rads_numpy()), r
    # set_parameters takes (C, 6); reset() decodes and re-draws the headings of all R replicas
    pop_e.set_parameters(unit[::-1].copy())
    pop_x.set_parameters(np.repeat(unit[::-1], E, axis=0))
    pop_e.reset(), pop_x.reset()
    assert pop_e.table().tobytes() == pop_x.table().tobytes()
    assert torch.equal(pop_e._hd_hi, pop_x._hd_hi) and torch.equal(pop_e._hd_lo, pop_x._hd_lo)


# ---------------------------------------------------------------------------------------------------- 3. reset(seeds=list)
@pytest.mark.parametrize('f16', [False, True])
def test_reset_with_a_seed_list_is_a_fresh_batch(f16):
    W, H, R, N = 64, 48, 6, 700
    dt = torch.float16 if f16 else torch.float32
    dyn = lambda: die.Dynamics(init_agent_ratio=0.15, **REFERENCE_DYNAMICS)
    seeds = [90, 13, 13, 2 ** 40 + 5, 0, 77]                     # no pattern, a repeat, a seed beyond 32 bits
    benv = BatchedEnv((W, H), dyn(), replicas=R, seed=3, field_dtype=dt, max_agents=N)
    template, rows = _nca_rows(2)
    benv.run(BatchedNeuralAutomataAgent(benv, template, rows, episodes=3), 4)
    benv.reset(seeds=seeds)
    fresh = BatchedEnv((W, H), dyn(), replicas=R, seeds=seeds, field_dtype=dt, max_agents=N)
    assert benv.seeds == seeds and benv._steps == 0
    _assert_same_worlds(benv, fresh)
    benv.check()
    assert benv._counts[:, 0].tolist() == [int(fresh.alive[r].sum()) for r in range(R)] and benv._counts[:, 1].tolist() == [0] * R
    m1, a1 = benv.replica_numpy(1)
    m2, a2 = benv.replica_numpy(2)
    assert np.array_equal(m1, m2) and np.array_equal(a1, a2)     # the repeated seed: one world twice
    # the stride form is the list of its pattern
    benv.reset(seed=1000, seed_stride=2)
    by_stride = benv._state.clone()
    benv.reset(seeds=[1000 + 2 * r for r in range(R)])
    assert torch.equal(by_stride, benv._state)                   # (the same kernels wrote the same words, claim plane included)
    benv.reset(seeds=episode_seeds(50, 2, 3, 1))
    _assert_same_worlds(benv, BatchedEnv((W, H), dyn(), replicas=R, seed=50, field_dtype=dt, max_agents=N))


def test_seed_list_overflow_flags_only_that_replica():
    W, H = 64, 48
    dyn = die.Dynamics(init_agent_ratio=0.15)
    cand = list(range(100, 116))
    k = {q: die.Env((W, H), dyn, seed=q, max_agents='alive').agents.N for q in cand}
    low = sorted(cand, key=lambda q: k[q])[:2]
    big = max(cand, key=lambda q: k[q])
    N = max(k[q] for q in low)
    assert k[big] > N
    benv = BatchedEnv((W, H), dyn, replicas=3, seeds=[low[0], low[1], low[0]], max_agents=N)
    benv.check()
    benv.reset(seeds=[low[1], big, low[0]])
    torch.cuda.synchronize()
    assert benv._counts[:, 1].tolist() == [0, 1, 0] and benv._counts[:, 0].tolist() == [k[low[1]], N, k[low[0]]]
    with pytest.raises(ValueError) as err:
        benv.check()
    assert f'replica 1 (seed {big})' in str(err.value) and 'replica 0' not in str(err.value) and 'replica 2' not in str(err.value)
    benv.check()                                                  # the flag was cleared


# ---------------------------------------------------------------------------------------------------- 4. the searchers
def _searcher(kind, popsize, center):
    if kind == 'pgpe':
        return PGPE(popsize, center_init=center, radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1, optimizer='clipup',
                    optimizer_config=dict(max_speed=0.15, momentum=0.9), seed=4)
    return CMAES(popsize, center_init=center, stdev_init=0.1, seed=4)


def _assert_same_search(kind, a, b):
    assert torch.equal(a.history(), b.history())
    assert torch.equal(a.center.cpu(), b.center.cpu())
    assert torch.equal(a.fitness.cpu(), b.fitness.cpu())
    assert torch.equal(a._best.cpu(), b._best.cpu()) and torch.equal(a._pop_best.cpu(), b._pop_best.cpu())
    assert torch.equal(a._evals.cpu(), b._evals.cpu())
    if kind == 'pgpe':
        assert torch.equal(a.stdev.cpu(), b.stdev.cpu()) and torch.equal(a._opt_a.cpu(), b._opt_a.cpu())
    else:
        assert torch.equal(a.C, b.C) and a.sigma == b.sigma
        assert torch.equal(a.p_sigma, b.p_sigma) and torch.equal(a.p_c, b.p_c)


@pytest.mark.parametrize('kind,stride', [('pgpe', 0), ('pgpe', 1), ('cmaes', 0), ('cmaes', 1)])
def test_searcher_generations_with_episodes_equal_the_loop_by_hand(kind, stride):
    W, H, T, G, S = 64, 48, 6, 3, 500
    template, rows = _nca_rows(C_)
    dyn = lambda: die.Dynamics(init_agent_ratio=0.15, **REFERENCE_DYNAMICS)
    benv = BatchedEnv((W, H), dyn(), replicas=C_ * E, seed=3, max_agents=None)
    pop = BatchedNeuralAutomataAgent(benv, template, rows, episodes=E)
    auto = _searcher(kind, C_, rows[0]).for_population(pop, T, reseed=S, reseed_stride=stride)
    henv = BatchedEnv((W, H), dyn(), replicas=C_ * E, seed=3, max_agents=None)
    hpop = BatchedNeuralAutomataAgent(henv, template, rows, episodes=E)
    hand = _searcher(kind, C_, rows[0])
    for g in range(G):
        auto.step()
        seeds = M.generation_seeds(S, g, C_, E, stride)
        assert benv.seeds == seeds
        hand.ask(hpop.parameters)
        assert torch.equal(hpop.parameters, pop.parameters)
        henv.reset(seeds=seeds)
        terms = henv.run(hpop, T)
        f, F = M.fold(terms.cpu().numpy(), C_, E)
        assert tuple(auto.episode_fitness.shape) == (C_, E)
        assert np.array_equal(auto.episode_fitness.cpu().numpy(), F)             # the per-replica sums
        assert np.array_equal(auto.fitness.cpu().numpy(), f)
        hand.tell(torch.tensor(f, dtype=torch.float64, device=henv.device).reshape(1, C_))      # the folded (1, C) terms
        _assert_same_search(kind, auto, hand)
    benv.check()
    assert auto.iter == hand.iter == G
    if stride == 0:                                               # every candidate saw the same E worlds
        assert benv.seeds[:E] * C_ == benv.seeds
    else:
        assert len(set(benv.seeds)) == C_ * E
    # the generic interface: tell(terms, episodes=E) on the raw (T, C·E, 2) words is that fold too
    third = _searcher(kind, C_, rows[0])
    params = torch.empty((C_, pop.P), dtype=torch.float32, device=benv.device)
    for g in range(G):
        third.ask(params)
        henv.reset(seeds=M.generation_seeds(S, g, C_, E, stride))
        hpop.set_parameters(params)
        third.tell(henv.run(hpop, T), episodes=E)
    _assert_same_search(kind, auto, third)
    assert torch.equal(auto.episode_fitness, third.episode_fitness)


def test_physarum_search_with_episodes_equals_the_loop_by_hand():
    size, T, G, S = 64, 5, 2, 40
    space = ParameterSpace()
    unit0 = np.full((C_, 6), 0.5, dtype=np.float32)
    envs = [BatchedEnv((size, size), die.Dynamics(), replicas=C_ * E, seed=3, max_agents=None) for _ in range(2)]
    pops = [BatchedPhysarumPopulation(e, parameters=unit0, space=space, seed=7, episodes=E) for e in envs]
    mk = lambda: PGPE(C_, center_init=unit0[0], stdev_init=0.1, center_learning_rate=0.05, stdev_learning_rate=0.1, seed=2)
    auto = mk().for_population(pops[0], T, reseed=S, reseed_stride=1)
    hand = mk()
    for g in range(G):
        auto.step()
        hand.ask(pops[1].parameters)
        envs[1].reset(seeds=M.generation_seeds(S, g, C_, E, 1))
        pops[1].reset()
        f, F = M.fold(envs[1].run(pops[1], T).cpu().numpy(), C_, E)
        hand.tell(torch.tensor(f, dtype=torch.float64, device=envs[1].device).reshape(1, C_))
        assert np.array_equal(auto.episode_fitness.cpu().numpy(), F)
        _assert_same_search('pgpe', auto, hand)


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


def test_a_generation_with_episodes_reads_nothing_back_and_allocates_nothing():
    W, H = 64, 48
    template, rows = _nca_rows(C_)
    benv = BatchedEnv((W, H), die.Dynamics(init_agent_ratio=0.15, **REFERENCE_DYNAMICS), replicas=C_ * E, seed=3, max_agents=None)
    pop = BatchedNeuralAutomataAgent(benv, template, rows, episodes=E)
    searcher = _searcher('pgpe', C_, rows[0]).for_population(pop, 5, reseed=77, reseed_stride=1)
    searcher.step()                                               # (first-call set-up outside the guard)
    torch.cuda.synchronize()
    used = torch.cuda.memory_allocated(benv.device)
    with _NoHostRead():
        benv.reset(seeds=SEEDS)
        searcher.step()
        assert torch.cuda.memory_allocated(benv.device) == used   # no allocation either
        spread = searcher.episode_fitness.std(dim=1)              # the spread across worlds, on the device
    benv.check()
    assert searcher.iter == 2 and benv.seeds == M.generation_seeds(77, 1, C_, E, 1) and tuple(spread.shape) == (C_,)


# ---------------------------------------------------------------------------------------------------- 5. E = 1
@pytest.mark.parametrize('kind', ['pgpe', 'cmaes'])
def test_one_episode_is_todays_path(kind):
    W, H, R, T, G, S = 64, 48, 4, 6, 3, 500
    template, rows = _nca_rows(R)
    dyn = lambda: die.Dynamics(init_agent_ratio=0.15, **REFERENCE_DYNAMICS)
    runs = []
    for kw in (dict(episodes=1), dict()):
        benv = BatchedEnv((W, H), dyn(), replicas=R, seed=3, max_agents=None)
        pop = BatchedNeuralAutomataAgent(benv, template, rows, **kw)
        s = _searcher(kind, R, rows[0]).for_population(pop, T, reseed=S, reseed_stride=1)
        s.run(G)
        assert benv.seeds == M.generation_seeds_today(S, G - 1, R, 1) == M.generation_seeds(S, G - 1, R, 1, 1)
        assert tuple(s.episode_fitness.shape) == (R, 1) and torch.equal(s.episode_fitness[:, 0], s.fitness)
        runs.append((s, benv, pop))
    _assert_same_search(kind, runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1]._state, runs[1][1]._state) and torch.equal(runs[0][2].parameters, runs[1][2].parameters)
    # tell(terms, episodes=1) is tell(terms)
    a, b = _searcher(kind, R, rows[0]), _searcher(kind, R, rows[0])
    pa, pb = (torch.empty((R, runs[0][2].P), dtype=torch.float32, device=runs[0][1].device) for _ in range(2))
    terms = torch.randn((5, R, 2), dtype=torch.float64, device=pa.device)
    a.ask(pa), b.ask(pb)
    a.tell(terms, episodes=1), b.tell(terms)
    _assert_same_search(kind, a, b)
