"""Batched replicas under the death pressure (Dynamics(agents_die=True)): replica r must be, bit for bit, the stand-alone
`Env(field_size, Dynamics(..., agents_die=True), seed=seeds[r], max_agents='alive')` driven by the matching agent — fields,
agents (x, y, alive, agent_food), Physarum headings, per-step reward and num_agents — in both regimes, with NCA populations
(with and without a food flow), across reset(), through one PGPE generation, and over a randomized sweep of shapes."""
import numpy as np
import pytest
import torch

import die_amd as die
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent, BatchedPhysarumAgent
from die_amd.search import PGPE

pytestmark = pytest.mark.gpu

REFERENCE_DYNAMICS = dict(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8)     # examples/learning_agents.py


def _run_alone(env, agent_at, steps):
    obs, want = env._get_current_obs, []
    for i in range(steps):
        obs, rw, _, _, info = env.step(agent_at(i).forward(obs))
        want.append((rw, info['num_agents']))
    return np.array([w[0] for w in want]), np.array([w[1] for w in want])


def _assert_replica_is(benv, r, env, rew, alive, want_rew, want_alive):
    m, a = benv.replica_numpy(r)
    assert np.array_equal(m, env.medium.to_numpy()), r
    assert np.array_equal(a, env.agents.to_numpy()), r
    assert np.array_equal(rew[:, r], want_rew), r
    assert np.array_equal(alive[:, r], want_alive), r


def _physarum_case(W, H, R, dt, dyn_kw, per_replica, steps, seed=40, agent_seed=7, deposit=12.0):
    # (deposit 12: a step costs 0.24 of an agent's food, more than the poorer cells feed — PhysarumAgent's default 4 starves nobody)
    kw = dict(scale=1.53 / (max(W, H) - 1), sense_offset=10.2 / (max(W, H) - 1), deposit=deposit)
    benv = BatchedEnv((W, H), die.Dynamics(agents_die=True, **dyn_kw), replicas=R, seed=seed, field_dtype=dt, per_replica=per_replica)
    assert benv.per_replica == per_replica
    bag = BatchedPhysarumAgent(benv, seed=agent_seed, **kw)
    rew, alive = BatchedEnv.read_results(benv.run(bag, steps))
    for r in range(R):
        env = die.Env((W, H), die.Dynamics(agents_die=True, **dyn_kw), seed=seed + r, max_agents='alive', field_dtype=dt)
        ag = die.PhysarumAgent(max_agents=env.agents.N, seed=agent_seed + r, **kw)
        want_rew, want_alive = _run_alone(env, lambda i: ag, steps)
        _assert_replica_is(benv, r, env, rew, alive, want_rew, want_alive)
        assert np.array_equal(bag.direction_rads_numpy(r), ag.direction_rads_numpy()), r
    return benv, rew, alive


@pytest.mark.parametrize('W,H,R,f16,boundary,per_replica', [
    (64, 48, 5, False, 'wrap', False),
    (256, 128, 3, True, 'limit', False),
    (96, 64, 4, True, 'wrap', False),
    (64, 48, 3, False, 'limit', False),
    (96, 64, 3, False, 'wrap', True),                  # the large-world regime (one Env per replica) forced on a small world
])
def test_physarum_replicas_under_death_pressure(W, H, R, f16, boundary, per_replica):
    """40 steps (the claim plane's 5-bit epoch wraps), finite food: agents starve, and every replica must lose some."""
    dyn_kw = dict(init_agent_ratio=0.15, boundary=die.BoundaryCondition(boundary))
    benv, rew, alive = _physarum_case(W, H, R, torch.float16 if f16 else torch.float32, dyn_kw, per_replica, 40)
    assert len(set(benv.n)) > 1                                  # replicas of different sizes share the launches
    for r in range(R):
        assert alive[-1, r] < benv.n[r], r                       # deaths happened: the lifecycle path is covered
        assert (np.diff(alive[:, r]) <= 0).all(), r              # nobody is born


# ---------------------------------------------------------------- NCA populations
def _nca_population(R, deposit=60.0, seed=5):
    """Candidates of three kinds: all-zero weights (no action cost: nobody dies), saturated weights (|deposit| ≈ the
    coefficient, a cost above any agent's food: extinct within a few steps) and init_weights() ones (some die)."""
    torch.manual_seed(seed)
    template = die.NeuralAutomataAgent(scale=0.01, deposit=deposit, kernel_sizes=(3, 3))
    rows, kinds = [], []
    for r in range(R):
        template.model.init_weights()
        v = torch.nn.utils.parameters_to_vector(template.model.parameters()).detach().clone()
        kind = ('zero', 'saturated', 'init')[r % 3] if r < 3 else 'init'
        rows.append(torch.zeros_like(v) if kind == 'zero' else v * 50.0 if kind == 'saturated' else v)
        kinds.append(kind)
    return template, torch.stack(rows), kinds


def _wave(W, H):
    return lambda: die.WaveSequence((W, H), dt=0.01).get_flow_operator(scale=0.5, decay=0.5)


def _nca_case(W, H, R, dyn_kw, per_replica, steps=33, make_op=None, seed=11):
    template, rows, kinds = _nca_population(R)
    dyn = lambda: die.Dynamics(agents_die=True, **dyn_kw, **({} if make_op is None else dict(op_food_flow=make_op())))
    benv = BatchedEnv((W, H), dyn(), replicas=R, seed=seed, per_replica=per_replica)
    assert benv.per_replica == per_replica
    bag = BatchedNeuralAutomataAgent(benv, template, rows)
    rew, alive = BatchedEnv.read_results(benv.run(bag, steps))
    for r in range(R):
        env = die.Env((W, H), dyn(), seed=seed + r, max_agents='alive')
        ag = BatchedNeuralAutomataAgent.unpack(template, rows[r]).to(env.device)
        want_rew, want_alive = _run_alone(env, lambda i: ag, steps)
        _assert_replica_is(benv, r, env, rew, alive, want_rew, want_alive)
        assert np.array_equal(bag.render(r), ag.render()[0]), r
    for r, kind in enumerate(kinds):
        if kind == 'zero' and make_op is None:                      # (a flowing wave can push a cell's food below 0)
            assert (alive[:, r] == benv.n[r]).all(), r            # actions cost nothing: nobody dies
        elif kind == 'saturated':
            assert (alive[5:, r] == 0).all(), r                     # extinct within a few steps, and stepped on at 0
    init = [r for r, k in enumerate(kinds) if k == 'init']
    assert any(alive[-1, r] < benv.n[r] for r in init)              # some of the ordinary candidates lose agents
    return benv, bag, rew, alive


@pytest.mark.parametrize('per_replica', [False, True])
def test_nca_population_under_death_pressure(per_replica):
    W, H = (96, 96) if not per_replica else (128, 96)
    _nca_case(W, H, 5, dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15), per_replica)


def test_nca_population_dyn_pred_under_death_pressure():
    """The reference's 'dyn-pred' world: waves of food flow over the replicas (one more launch per batched step)."""
    _nca_case(96, 96, 4, dict(food_infinite=False, init_agent_ratio=0.15), False, make_op=_wave(96, 96))


# ---------------------------------------------------------------- reset, search
def _state(benv):
    torch.cuda.synchronize()
    return [tuple(x.copy() for x in benv.replica_numpy(r)) for r in range(benv.R)]


@pytest.mark.parametrize('per_replica', [False, True])
def test_reset_after_deaths(per_replica):
    W, H, R, steps = 64, 64, 4, 20
    template, rows, _ = _nca_population(R)
    make = lambda: BatchedEnv((W, H), die.Dynamics(agents_die=True, **REFERENCE_DYNAMICS), replicas=R, seeds=[3] * R,
                              per_replica=per_replica)
    benv = make()
    bag = BatchedNeuralAutomataAgent(benv, template, rows)
    first = benv.run(bag, steps).clone()
    _, alive = BatchedEnv.read_results(first)
    assert (alive[-1] < np.array(benv.n)).any()                  # there were deaths to undo
    benv.reset()
    fresh = make()
    for (m, a), (fm, fa) in zip(_state(benv), _state(fresh)):
        assert np.array_equal(m, fm) and np.array_equal(a, fa)
    if per_replica:
        assert all(e._all_alive == f._all_alive for e, f in zip(benv.envs, fresh.envs))
    second = benv.run(bag, steps)
    assert torch.equal(first, second)


def test_one_pgpe_generation_under_death_pressure():
    """ask → reset + run → tell: every candidate's fitness is the summed rewards of its row run stand-alone."""
    W, H, R, T = 64, 64, 6, 16
    dyn = lambda: die.Dynamics(agents_die=True, **REFERENCE_DYNAMICS)
    template = die.NeuralAutomataAgent(scale=0.01, deposit=20.0, kernel_sizes=(3, 3))
    benv = BatchedEnv((W, H), dyn(), replicas=R, seeds=[9] * R)
    pop = BatchedNeuralAutomataAgent(benv, template)
    s = PGPE(R, center_init=pop.parameters[0].cpu(), radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1,
             optimizer_config=dict(max_speed=0.1, momentum=0.9), seed=11, device='cuda')
    s.ask(pop.parameters)
    rows = pop.parameters.cpu()
    benv.reset()
    res = benv.run(pop, T)
    s.tell(res)
    _, alive = BatchedEnv.read_results(res)
    assert (alive[-1] < np.array(benv.n)).any()                  # the pressure shaped the fitness
    fitness = s.fitness.cpu().tolist()
    for r in range(R):
        env = die.Env((W, H), dyn(), seed=9, max_agents='alive')
        ag = BatchedNeuralAutomataAgent.unpack(template, rows[r]).to(env.device)
        want_rew, _ = _run_alone(env, lambda i: ag, T)
        assert fitness[r] == sum(want_rew.tolist()), r


# ---------------------------------------------------------------- randomized sweep
def _sweep_case(i):
    rs = np.random.RandomState(1000 + i)
    W = int(rs.choice([32, 48, 64, 96]))
    H = 42 if i % 4 == 3 else int(rs.choice([32, 40, 44, 64, 96]))     # 42: rows not a multiple of 4, refused
    return dict(W=W, H=H, R=int(rs.randint(1, 7)), f16=bool(rs.rand() < 0.3), boundary=str(rs.choice(['wrap', 'limit'])),
                ratio=float(rs.uniform(0.05, 0.3)), rate_feed=float(rs.uniform(0.05, 0.3)), decay=float(rs.uniform(0.02, 0.2)),
                sigma=float(rs.choice([0.5, 0.6, 0.8])), food_infinite=bool(rs.rand() < 0.25), steps=int(rs.randint(6, 15)),
                seed=int(rs.randint(0, 1000)))


@pytest.mark.parametrize('i', range(12))
def test_randomized_sweep(i):
    c = _sweep_case(i)
    dt = torch.float16 if c['f16'] else torch.float32
    dyn_kw = dict(init_agent_ratio=c['ratio'], boundary=die.BoundaryCondition(c['boundary']), rate_feed=c['rate_feed'],
                  rate_decay_chem=c['decay'], diffuse_sigma=c['sigma'], food_infinite=c['food_infinite'])
    if c['H'] % 4:
        benv = BatchedEnv((c['W'], c['H']), die.Dynamics(agents_die=True, **dyn_kw), replicas=c['R'], seed=c['seed'], field_dtype=dt)
        bag = BatchedPhysarumAgent(benv, seed=3)
        before = _state(benv)
        with pytest.raises(NotImplementedError, match='H % 4'):
            benv.step(bag)
        for (m, a), (bm, ba) in zip(_state(benv), before):              # (food, chem and the agents: nothing was launched)
            assert np.array_equal(m[1:], bm[1:]) and np.array_equal(a, ba)
        return
    _physarum_case(c['W'], c['H'], c['R'], dt, dyn_kw, False, c['steps'], seed=c['seed'], agent_seed=c['seed'] + 1)
