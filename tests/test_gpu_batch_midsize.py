"""Batched replicas at mid-size worlds: the sizes at which the batched kernels leave the paths the small-shape tests run.

Three shapes (tests/midsize_shapes.py; tests/test_batch_midsize_cpu.py recomputes every claim made here from the sources):

    S  2 x  514 x  512   the batch sweeps 4 rows a wave, a replica's stand-alone twin 2;  823 partials for the reduction row
    M  2 x 1028 x 1024   8 against 4;  3 290 partials: a second trip of the reduction row's loop
    L  3 x 1676 x 1672   16 against 8;  2 802 272 slots with max_agents=None: the partials are capped at 8192 and every claim,
                         lifecycle, stock, gather and init kernel takes a second grid-stride trip

In each, W is no multiple of the batch's rows per wave (a partial last wave), H > 496 (several strips a row, several workgroups
on the reduction row), and every replica is below Env.PIC_MIN_CELLS, so `BatchedEnv` picks the batched regime itself.  Replica r
must be the stand-alone `Env` of its seed bit for bit — although that Env sweeps with another rows-per-wave value — and, in a
test that shares no device code with what it checks, the float64 oracle within the parity test's tolerances.  Three steps a
case (one against the oracle): the claim plane's epoch wrap is covered at small shapes."""
import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent, BatchedPhysarumAgent
from oracle import cpu_ref as R
from tests.midsize_shapes import SHAPES
from tests.test_gpu_batch_step_action import NAMES, _cell, _moved, batch_state, build, draw_actions, run_twins
from tests.test_gpu_parity import RTOL, quantised_action, ref_dyn

pytestmark = pytest.mark.gpu

STEPS = 3


def _case(name, **kw):
    replicas, W, H = SHAPES[name]
    return dict(shape=(W, H), R=replicas, **kw)


def fast_winners(env, action, W, H):
    """tests/test_gpu_batch_step_action.py host_winners without deposit_cells' Python loop over the alive slots: the same three
    arrays.  (Ascending slot ids written by fancy assignment: the last — highest — write to a cell stays.)"""
    limit = env.dynamics.boundary == die.BoundaryCondition.limit
    x = env.agents.x.cpu().numpy().view(np.uint32)
    y = env.agents.y.cpu().numpy().view(np.uint32)
    alive = env.agents.alive.cpu().numpy() > 0
    where = _cell(_moved(x, action[0], limit), W) * H + _cell(_moved(y, action[1], limit), H)
    idx = np.flatnonzero(alive)
    best = np.full(W * H, -1, dtype=np.int64)
    best[where[idx]] = idx
    winners = best[best >= 0]
    cells = np.full(x.size, -1, dtype=np.int32)
    cells[winners] = where[winners]
    return cells, where, alive


def test_fast_winners_are_host_winners():
    from tests.test_gpu_batch_step_action import host_winners
    case = dict(shape=(24, 68), R=2, agents_die=True, max_agents=None)
    benv, twins = build(case)
    act = draw_actions(case, benv, 1)[0]
    for r, env in enumerate(twins):
        env.agents.alive[::7] = 0                                  # dead slots among the alive ones
        for got, want in zip(fast_winners(env, act[:, r], 24, 68), host_winners(env, act[:, r], 24, 68)):
            assert np.array_equal(got, want), r


# ---------------------------------------------------------------- 1. step_action against stand-alone Envs, bit for bit
ACTION_CASES = {
    'S_f32_full_die': _case('S', max_agents=None, agents_die=True),
    'M_f32_full_die': _case('M', max_agents=None, agents_die=True),
    'L_f32_full_die': _case('L', max_agents=None, agents_die=True),
    'S_f16_alive': _case('S', f16=True),
    'L_f16_alive': _case('L', f16=True),
    'M_f32_rows_flow': _case('M', listed=True, flow=True),         # per-replica Dynamics: radii 2 and 3 in one launch, the wave flow on
}


@pytest.mark.parametrize('name', list(ACTION_CASES))
def test_step_action_equals_stand_alone_steps(name):
    case = ACTION_CASES[name]
    W, H = case['shape']
    benv, twins = build(case, per_replica=None)                    # the regime is BatchedEnv's own choice …
    assert benv.per_replica is False and W * H < die.Env.PIC_MIN_CELLS     # … and it is the batched one
    k0 = [int(benv.alive[r, :k].sum().item()) for r, k in enumerate(benv.n)]
    if case.get('max_agents', 'alive') == 'alive':
        assert len(set(benv.n)) > 1                                # padding exists
    else:
        assert benv.n == [W * H] * benv.R
    if case.get('listed'):
        assert {R.gaussian_weights(d.diffuse_sigma).size // 2 for d in benv._dyn} == {2, 3}
    actions = draw_actions(case, benv, STEPS)
    want, shared = run_twins(case, benv, twins, actions, winners=fast_winners)
    assert all(shared), f'replicas without a shared cell and a loser: {[r for r, s in enumerate(shared) if not s]}'
    dev_actions = torch.from_numpy(actions).to(benv.device)
    for t in range(STEPS):
        res = benv.step_action(dev_actions[t])
        assert benv.epoch == t + 2
        for r in range(benv.R):
            w = want[r][t]
            assert torch.equal(res[r].view(torch.int64), w[0].view(torch.int64)), (t, r, 'result words')
            for what, got, exp in zip(NAMES, batch_state(benv, r), w[1:]):
                assert torch.equal(got, exp), (t, r, what)
    assert benv._steps == STEPS
    if case.get('agents_die'):
        _, alive = BatchedEnv.read_results(res)
        assert (alive < np.array(k0)).all()                       # slots starved in every replica: the lifecycle pass was part of it
    for r, env in enumerate(twins):                                # … and what the public accessors say
        m, a = benv.replica_numpy(r)
        assert np.array_equal(m, env.medium.to_numpy()) and np.array_equal(a, env.agents.to_numpy()), r


# ---------------------------------------------------------------- 2. step_action against the float64 oracle
@pytest.mark.parametrize('name', ['S', 'L'])
def test_step_action_against_the_oracle(name):
    """One step; the comparison of tests/test_gpu_parity.py::test_env_step_parity with its RTOL and atol values: positions, alive,
    the occupancy plane and num_agents exact, agent_food / food / chem / reward within tolerance."""
    replicas, W, H = SHAPES[name]
    dyn = die.Dynamics(init_agent_ratio=0.15)
    benv = BatchedEnv((W, H), dyn, replicas=replicas, seed=3, max_agents=None)
    assert benv.per_replica is False and benv.n == [W * H] * replicas
    N = W * H
    rs = np.random.RandomState(W * 7 + N)
    start = [benv.replica_numpy(r) for r in range(replicas)]
    actions = np.stack([quantised_action(N, rs, 3.0 / W) for _ in range(replicas)], axis=1).astype(np.float32)     # (3, R, N)
    res = benv.step_action(torch.from_numpy(np.ascontiguousarray(actions)).to(benv.device))
    reward, num_agents = BatchedEnv.read_results(res)
    rd = ref_dyn(dyn)
    for f in ('rate_feed', 'rate_decay_chem', 'diffuse_sigma'):    # the C struct carries them as f32
        setattr(rd, f, float(np.float32(getattr(rd, f))))
    for r in range(replicas):
        medium, agents = start[r]
        assert 0 < (agents[2] > 0).sum() < N                       # dead slots ride along
        ref = R.RefEnv(medium, agents, rd)
        _, want_reward, _, _, want_info = ref.step(actions[:, r].astype(np.float64))
        got_medium, got_agents = benv.replica_numpy(r)
        assert np.array_equal(got_agents[:2], ref.agents[:2]), r
        assert np.array_equal(got_agents[2], ref.agents[2]), r
        assert np.array_equal(got_medium[0], ref.medium[0]), r
        assert num_agents[r] == want_info['num_agents'], r
        assert got_medium[0].sum() < num_agents[r]                 # cells were shared: somebody lost a claim
        assert np.allclose(got_agents[3], ref.agents[3], rtol=RTOL, atol=1e-7), r
        assert np.allclose(got_medium[1], ref.medium[1], rtol=RTOL, atol=1e-8), r
        assert np.allclose(got_medium[2], ref.medium[2], rtol=RTOL, atol=1e-7), r
        assert abs(reward[r] - want_reward) <= RTOL * np.abs(ref.last_gained).sum() + 1e-9, r


# ---------------------------------------------------------------- 3. agent-driven steps
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


def test_physarum_replicas_equal_stand_alone_runs():
    """die_forward_env_step_batch on M, the 'alive' layout (replicas of different sizes share the launches)."""
    replicas, W, H = SHAPES['M']
    kw = dict(scale=1.53 / (max(W, H) - 1), sense_offset=10.2 / (max(W, H) - 1))
    benv = BatchedEnv((W, H), die.Dynamics(init_agent_ratio=0.15), replicas=replicas, seed=40)
    assert benv.per_replica is False and len(set(benv.n)) > 1
    bag = BatchedPhysarumAgent(benv, seed=7, **kw)
    rew, alive = BatchedEnv.read_results(benv.run(bag, STEPS))
    for r in range(replicas):
        env = die.Env((W, H), die.Dynamics(init_agent_ratio=0.15), seed=40 + r, max_agents='alive')
        ag = die.PhysarumAgent(max_agents=env.agents.N, seed=7 + r, **kw)
        want_rew, want_alive = _run_alone(env, ag, STEPS)
        assert env._pic is None and env.agents.slot is None          # the classic step, slot order
        _assert_replica_is(benv, r, env, rew, alive, want_rew, want_alive)
        assert np.array_equal(bag.direction_rads_numpy(r), ag.direction_rads_numpy()), r


RICH, POOR, MIDDLE = 0.9, 1e-3, 0.3


def _set_stocks(alive, agent_food):
    """Every alive slot's food, in place: a third RICH (a step costs 0.02 · 12 + 0.01 · |move| < 0.25 at most: still above
    born_threshold 0.5 afterwards, so each of them breeds at the first step, and the halved stock is below 0.5), a third POOR
    (starves unless its cell feeds more than its action costs), a third MIDDLE (0.3 + at most 0.1 · 0.5 fed: no parent).
    Returns the RICH slots."""
    idx = alive.nonzero().flatten()
    agent_food[idx[0::3]] = RICH
    agent_food[idx[1::3]] = POOR
    agent_food[idx[2::3]] = MIDDLE
    return idx[0::3]


def test_nca_stock_population_breeds_and_starves_like_its_stand_alone_envs():
    """L with max_agents=None under deaths and births, a stock-channel population with seeded dropout: one batch runs the batched
    conv, k_stock_plane with blockIdx.y, k_gather_scale_batch, k_nca_move_claim_batch, the lifecycle pass and the three births
    kernels at 2.8 M slots a replica.  Somebody must be born and somebody must die in every replica at the first step."""
    replicas, W, H = SHAPES['L']
    dyn = lambda: die.Dynamics(agents_die=True, agents_born=True, food_infinite=False, init_agent_ratio=0.15)
    torch.manual_seed(W + replicas)
    cands = []
    for _ in range(replicas):
        ag = die.NeuralAutomataAgent(scale=0.01, deposit=12.0, kernel_sizes=(3, 3), with_stock_channel=True, p_agent_dropout=0.25)
        ag.model.init_weights()
        cands.append(ag)
    benv = BatchedEnv((W, H), dyn(), replicas=replicas, seed=11, max_agents=None)
    assert benv.per_replica is False and benv.n == [W * H] * replicas
    rich = [_set_stocks(benv.alive[r], benv.agent_food[r]) for r in range(replicas)]
    k0 = [int(benv.alive[r].sum().item()) for r in range(replicas)]
    pop = BatchedNeuralAutomataAgent.from_agents(benv, cands, dropout_seed=1000)
    assert pop._stock_channel and pop._dropout() is not None
    out = torch.empty((STEPS, replicas, 2), dtype=torch.float64, device=benv.device)
    benv.step(pop, out[0])
    _, after = BatchedEnv.read_results(out[0])
    for r in range(replicas):
        # a RICH slot below 0.5 has bred (no cost takes 0.9 there); only RICH slots can: deaths = k0 + born - alive afterwards
        born = int((benv.agent_food[r][rich[r]] < 0.5).sum().item())
        died = k0[r] + born - int(after[r])
        assert born > 0 and died > 0, (r, born, died)
        assert int(benv.alive[r].sum().item()) == int(after[r]), r
    for t in range(1, STEPS):
        benv.step(pop, out[t])
    rew, alive = BatchedEnv.read_results(out)
    assert benv._stock is not None and pop.dropout_step == STEPS
    for r in range(replicas):
        env = die.Env((W, H), dyn(), seed=11 + r, max_agents=None)
        _set_stocks(env.agents.alive, env.agents.agent_food)
        ag = pop.replica_agent(r)
        assert ag.with_stock_channel and ag.dropout_seed == 1000 + r
        want_rew, want_alive = _run_alone(env, ag, STEPS)
        assert env._pic is None and env.agents.slot is None
        _assert_replica_is(benv, r, env, rew, alive, want_rew, want_alive)
        assert np.array_equal(pop.render(r), ag.render()[0]), r


# ---------------------------------------------------------------- 4. reseeding
def test_reset_with_seed_is_a_fresh_batch():
    """die_init_batch on L with max_agents=None: the reseeded batch is the freshly built batch of those seeds, and replica r the
    stand-alone Env(seed) — fields, every slot, and the (K_r, overflow) words."""
    replicas, W, H = SHAPES['L']
    dyn = lambda: die.Dynamics(init_agent_ratio=0.15)
    kw = dict(scale=1.53 / (max(W, H) - 1), sense_offset=10.2 / (max(W, H) - 1))
    benv = BatchedEnv((W, H), dyn(), replicas=replicas, seed=3, max_agents=None)
    assert benv.per_replica is False
    benv.run(BatchedPhysarumAgent(benv, seed=1, **kw), 2)          # a used batch
    s = 1000
    benv.reset(seed=s)
    seeds = [s + r for r in range(replicas)]
    assert benv.seeds == seeds and benv._steps == 0 and benv.epoch == 1
    fresh = BatchedEnv((W, H), dyn(), replicas=replicas, seeds=seeds, max_agents=None)
    counts = benv._counts.cpu().tolist()
    for r in range(replicas):
        for what, got, exp in zip(NAMES, batch_state(benv, r), batch_state(fresh, r)):
            assert torch.equal(got, exp), (r, what)
        env = die.Env((W, H), dyn(), seed=seeds[r], max_agents=None)
        assert torch.equal(benv.food[r], env.medium.food) and torch.equal(benv.chem[r], env.medium.chem), r
        for what, got, exp in zip(NAMES[3:], batch_state(benv, r)[3:], (env.agents.x, env.agents.y, env.agents.alive, env.agents.agent_food)):
            assert torch.equal(got, exp), (r, what)
        assert counts[r] == [env._num_seeded, 0] and 0 < env._num_seeded < W * H, r
        assert int(benv.alive[r].sum().item()) == env._num_seeded, r
    benv.check()
    m, a = benv.replica_numpy(replicas - 1)                        # the public accessors, on the last replica of the allocation
    assert np.array_equal(m, env.medium.to_numpy()) and np.array_equal(a, env.agents.to_numpy())
    # one further step with fresh agents: the reseeded batch goes where the fresh one goes
    one = benv.step(BatchedPhysarumAgent(benv, seed=9, **kw))
    two = fresh.step(BatchedPhysarumAgent(fresh, seed=9, **kw))
    assert torch.equal(one.view(torch.int64), two.view(torch.int64))
    for r in range(replicas):
        for what, got, exp in zip(NAMES, batch_state(benv, r), batch_state(fresh, r)):
            assert torch.equal(got, exp), (r, what)
