"""Per-replica Dynamics on batched replicas (`BatchedEnv(dynamics=[...])`, die_*_env_step_batch_rows, die_food_flow_batch_masked):
replica r must be, bit for bit, the stand-alone `Env(field_size, dynamics[r], seed=seeds[r], max_agents=...)` driven by
`replica_agent(r)` — the owner-derived agents channel, food, chem, x, y, alive, agent_food and both result words of every step.
A replica whose Dynamics names the batch's flow operator is compared with a fresh operator at the batch's counter, as
tests/test_gpu_flow_batch.py does.  35 steps per case: the claim plane's 5-bit epoch wraps once."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib
from die_amd.batch import (BatchedEnv, BatchedNeuralAutomataAgent, BatchedPhysarumAgent, BatchedPhysarumPopulation, episode_dynamics,
                           episode_seeds)
from die_amd.device_array import _ptr, stream_ptr
from die_amd.env import _identity_food_flow
from die_amd.search import CMAES, PGPE
from tests import episodes_model as M

pytestmark = pytest.mark.gpu

STEPS = 35
SEEDS = [11, 40, 7, 93, 12, 58]                                  # given, no arithmetic pattern
SIZES = [(96, 96, torch.float32), (64, 48, torch.float16)]


def _wave(W, H):
    return die.WaveSequence((W, H), dt=0.01).get_flow_operator(scale=0.5, decay=0.5)


def _three(W, H, **kw):
    """The reference's learning_agents.py `dynamics_choice`: st-perlin, st-perlin-wide, dyn-pred (one operator object)."""
    return [die.Dynamics(food_infinite=True, **kw), die.Dynamics(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8, **kw),
            die.Dynamics(food_infinite=False, op_food_flow=_wave(W, H), **kw)]


def _alone_dynamics(d, W, H, k0=0):
    """`d` for a stand-alone Env: a flow replica gets a fresh operator standing at the batch's counter."""
    if d.op_food_flow is _identity_food_flow:
        return dataclasses.replace(d)
    op = _wave(W, H)
    for _ in range(k0):
        op.next_t()
    return dataclasses.replace(d, op_food_flow=op)


def _run_alone(env, ag, steps):
    obs, rew, alive = env._get_current_obs, [], []
    for _ in range(steps):
        obs, rw, _, _, info = env.step(ag.forward(obs))
        rew.append(rw)
        alive.append(info['num_agents'])
    return np.array(rew), np.array(alive)


def _assert_replicas_alone(benv, agent_of, rew, alive, W, H, dt, max_agents='alive', steps=STEPS, k0=0):
    for r in range(benv.R):
        env = die.Env((W, H), _alone_dynamics(benv.replica_dynamics(r), W, H, k0), seed=benv.seeds[r], max_agents=max_agents, field_dtype=dt)
        want_rew, want_alive = _run_alone(env, agent_of(r, env), steps)
        m, a = benv.replica_numpy(r)
        assert np.array_equal(m, env.medium.to_numpy()), r       # agents channel (from the owner plane), food, chem
        assert np.array_equal(a, env.agents.to_numpy()), r       # x, y, alive, agent_food
        assert np.array_equal(rew[:, r], want_rew), r
        assert np.array_equal(alive[:, r], want_alive), r


def _template(**kw):
    torch.manual_seed(5)
    return die.NeuralAutomataAgent(scale=0.01, deposit=2.0, kernel_sizes=(3, 3), boundary='circular', **kw)


def _nca_rows(template, n):
    rows = []
    for _ in range(n):
        template.model.init_weights()
        rows.append(torch.nn.utils.parameters_to_vector(template.model.parameters()).detach().clone())
    return torch.stack(rows)


PHYS = dict(scale=1.53 / 95, sense_offset=10.2 / 95)


# ---------------------------------------------------------------------------------------------------- mixed replicas
@pytest.mark.parametrize('W,H,dt', SIZES)
def test_nca_mixed_dynamics_equal_stand_alone_runs(W, H, dt):
    dyn = _three(W, H, init_agent_ratio=0.15) * 2
    benv = BatchedEnv((W, H), dyn, replicas=6, seeds=SEEDS, field_dtype=dt)
    assert not benv.per_replica and [benv.replica_dynamics(r) for r in range(6)] == dyn
    template = _template()
    bag = BatchedNeuralAutomataAgent(benv, template, _nca_rows(template, 6))
    rew, alive = BatchedEnv.read_results(benv.run(bag, STEPS))
    assert dyn[2].op_food_flow._k == STEPS                        # the one operator advanced once per batched step
    assert len(set(rew.sum(axis=0).tolist())) == 6
    _assert_replicas_alone(benv, lambda r, env: bag.replica_agent(r), rew, alive, W, H, dt)


@pytest.mark.parametrize('W,H,dt', SIZES)
def test_physarum_population_mixed_dynamics_equal_stand_alone_runs(W, H, dt):
    benv = BatchedEnv((W, H), _three(W, H, init_agent_ratio=0.15) * 2, replicas=6, seeds=SEEDS, field_dtype=dt)
    values = np.tile(np.float32([PHYS['scale'], 4.0, PHYS['sense_offset'], 30, 90, 0.1]), (6, 1))
    values[:, 1] = np.float32([4.0, 3.0, 5.0, 2.5, 4.5, 3.5])
    values[:, 3] = np.float32([30, 45, 20, 30, 60, 25])
    pop = BatchedPhysarumPopulation(benv, values, seed=7)
    rew, alive = BatchedEnv.read_results(benv.run(pop, STEPS))
    _assert_replicas_alone(benv, lambda r, env: pop.replica_agent(r), rew, alive, W, H, dt)


@pytest.mark.parametrize('W,H,dt', SIZES)
def test_physarum_agent_mixed_dynamics_equal_stand_alone_runs(W, H, dt):
    benv = BatchedEnv((W, H), _three(W, H, init_agent_ratio=0.15) * 2, replicas=6, seeds=SEEDS, field_dtype=dt)
    bag = BatchedPhysarumAgent(benv, seed=7, **PHYS)
    rew, alive = BatchedEnv.read_results(benv.run(bag, STEPS))
    _assert_replicas_alone(benv, lambda r, env: die.PhysarumAgent(max_agents=env.agents.N, seed=7 + r, **PHYS), rew, alive, W, H, dt)


# ---------------------------------------------------------------------------------------------------- variants
def test_mixed_dynamics_with_agents_die():
    W, H, dt = 64, 48, torch.float32
    benv = BatchedEnv((W, H), _three(W, H, init_agent_ratio=0.15, agents_die=True) * 2, replicas=6, seeds=SEEDS, field_dtype=dt)
    template = _template()
    bag = BatchedNeuralAutomataAgent(benv, template, _nca_rows(template, 6))
    rew, alive = BatchedEnv.read_results(benv.run(bag, STEPS))
    _assert_replicas_alone(benv, lambda r, env: bag.replica_agent(r), rew, alive, W, H, dt)
    pop = BatchedPhysarumPopulation(benv, seed=7)
    benv.reset()
    rew, alive = BatchedEnv.read_results(benv.run(pop, STEPS))
    _assert_replicas_alone(benv, lambda r, env: pop.replica_agent(r), rew, alive, W, H, dt)


def test_mixed_dynamics_fixed_slots_and_reseeding():
    W, H, dt, N = 64, 48, torch.float32, 700
    benv = BatchedEnv((W, H), _three(W, H, init_agent_ratio=0.15) * 2, replicas=6, seeds=SEEDS, field_dtype=dt, max_agents=N)
    template = _template()
    bag = BatchedNeuralAutomataAgent(benv, template, _nca_rows(template, 6))
    rew, alive = BatchedEnv.read_results(benv.run(bag, STEPS))
    _assert_replicas_alone(benv, lambda r, env: bag.replica_agent(r), rew, alive, W, H, dt, max_agents=N)
    benv.reset(seed=300, seed_stride=2)                           # the rows are not state: new worlds, the same dynamics
    assert benv.seeds == [300 + 2 * r for r in range(6)]
    rew, alive = BatchedEnv.read_results(benv.run(bag, STEPS))
    benv.check()
    _assert_replicas_alone(benv, lambda r, env: bag.replica_agent(r), rew, alive, W, H, dt, max_agents=N)
    benv.reset(seeds=[5, 66, 5, 21, 90, 3])
    rew, alive = BatchedEnv.read_results(benv.run(bag, STEPS))
    benv.check()
    _assert_replicas_alone(benv, lambda r, env: bag.replica_agent(r), rew, alive, W, H, dt, max_agents=N)


def test_mixed_dynamics_with_dropout_seed():
    W, H, dt = 64, 48, torch.float32
    benv = BatchedEnv((W, H), _three(W, H, init_agent_ratio=0.15) * 2, replicas=6, seeds=SEEDS, field_dtype=dt)
    template = _template(p_agent_dropout=0.25)
    assert template.model.training
    bag = BatchedNeuralAutomataAgent(benv, template, _nca_rows(template, 6), dropout_seed=9, dropout_seed_stride=3)
    rew, alive = BatchedEnv.read_results(benv.run(bag, STEPS))
    assert bag.dropout_step == STEPS
    _assert_replicas_alone(benv, lambda r, env: bag.replica_agent(r), rew, alive, W, H, dt)


@pytest.mark.parametrize('W,H,dt', SIZES)
def test_uniform_list_is_the_shared_dynamics(W, H, dt):
    R = 5
    outs = []
    for listed in (False, True):
        d = die.Dynamics(food_infinite=False, rate_decay_chem=0.025, diffuse_sigma=.8, init_agent_ratio=0.15, op_food_flow=_wave(W, H))
        benv = BatchedEnv((W, H), [d] * R if listed else d, replicas=R, seed=3, field_dtype=dt)
        assert (benv._rows is not None) == listed
        template = _template()
        bag = BatchedNeuralAutomataAgent(benv, template, _nca_rows(template, R))
        res = benv.run(bag, STEPS)
        pag = BatchedPhysarumAgent(benv, seed=7, **PHYS)
        res2 = benv.run(pag, 5)
        outs.append((res.clone(), res2.clone(), benv._state.clone(), benv.chem.clone(), benv.epoch))
    a, b = outs
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and a[4] == b[4]


@pytest.mark.parametrize('kind', ['wave', 'perlin'])
@pytest.mark.parametrize('dt', [torch.float32, torch.float16])
def test_full_mask_is_die_food_flow_batch(kind, dt):
    W, H, R = 64, 48, 7
    g = torch.Generator().manual_seed(3)
    food = torch.rand((R, W, H), generator=g).to(device='cuda', dtype=dt)
    planes = [food.clone(), food.clone(), food.clone()]
    fdt = _lib.DIE_F32 if dt == torch.float32 else _lib.DIE_F16
    flow, octaves, seed = (_lib.DIE_FLOW_WAVE, 0, 0) if kind == 'wave' else (_lib.DIE_FLOW_PERLIN, 8, 11)
    b = _lib.Batch(R, 0, W * H, 10, 1, (C.c_int64 * 64)(*([10] * 64)))
    dev = food.device
    for t in (0.0, 0.37):
        m = [_lib.Medium(W, H, fdt, 1, None, _ptr(p), None, None, 0, 0, 0, 0, 0, 0, 0, 0, None) for p in planes]
        _lib.check(_lib.lib.die_food_flow_batch(C.byref(m[0]), C.byref(b), flow, t, 0.5, 0.5, octaves, seed, stream_ptr(dev)))
        _lib.check(_lib.lib.die_food_flow_batch_masked(C.byref(m[1]), C.byref(b), flow, t, 0.5, 0.5, octaves, seed, (1 << R) - 1, stream_ptr(dev)))
        _lib.check(_lib.lib.die_food_flow_batch_masked(C.byref(m[2]), C.byref(b), flow, t, 0.5, 0.5, octaves, seed, 0b0100101, stream_ptr(dev)))
    torch.cuda.synchronize()
    bits = torch.int32 if dt == torch.float32 else torch.int16
    assert torch.equal(planes[0].view(bits), planes[1].view(bits))
    assert not torch.equal(planes[0], food)
    for r in range(R):                                            # a partial mask: set replicas flowed, the others were not touched
        want = planes[0][r] if (0b0100101 >> r) & 1 else food[r]
        assert torch.equal(planes[2][r].view(bits), want.view(bits)), r


@pytest.mark.parametrize('W,H,dt', SIZES)
def test_mixed_radii_equal_stand_alone_runs(W, H, dt):
    """sigma 0.3, 0.5, 0.8, 1.1: gaussian radii 1, 2, 3, 4 in one batch — four sweep launches, each its own instantiation."""
    sig = [0.3, 0.5, 0.8, 1.1, 0.8, 0.3]
    dyn = [die.Dynamics(diffuse_sigma=s, rate_decay_chem=0.05 + 0.01 * i, rate_feed=0.1 + 0.02 * i, food_infinite=bool(i % 2),
                        init_agent_ratio=0.15) for i, s in enumerate(sig)]
    benv = BatchedEnv((W, H), dyn, replicas=6, seeds=SEEDS, field_dtype=dt)
    assert [row.radius for row in benv._rows_host] == [1, 2, 3, 4, 3, 1]
    template = _template()
    bag = BatchedNeuralAutomataAgent(benv, template, _nca_rows(template, 6))
    rew, alive = BatchedEnv.read_results(benv.run(bag, STEPS))
    _assert_replicas_alone(benv, lambda r, env: bag.replica_agent(r), rew, alive, W, H, dt)
    benv.reset()
    pag = BatchedPhysarumAgent(benv, seed=7, **PHYS)
    rew, alive = BatchedEnv.read_results(benv.run(pag, STEPS))
    _assert_replicas_alone(benv, lambda r, env: die.PhysarumAgent(max_agents=env.agents.N, seed=7 + r, **PHYS), rew, alive, W, H, dt)


# ---------------------------------------------------------------------------------------------------- searchers
def _searcher(kind, popsize, center):
    if kind == 'pgpe':
        return PGPE(popsize, center_init=center, radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1, optimizer='clipup',
                    optimizer_config=dict(max_speed=0.15, momentum=0.9), seed=4)
    return CMAES(popsize, center_init=center, stdev_init=0.1, seed=4)


@pytest.mark.parametrize('kind,G', [('pgpe', 3), ('cmaes', 1)])
def test_searcher_generations_over_three_dynamics(kind, G):
    """episode_fitness[c, e] is candidate c's score under dynamics e: the sum of replica c·3 + e's rewards of a hand-stepped
    copy; fitness is their mean, added in episode order."""
    W, H, T, Cn, E = 64, 48, 6, 4, 3
    template = _template()
    rows = _nca_rows(template, Cn)
    mk = lambda: BatchedEnv((W, H), episode_dynamics(_three(W, H, init_agent_ratio=0.15), Cn), replicas=Cn * E,
                            seeds=episode_seeds(3, Cn, E))
    benv, henv = mk(), mk()
    assert [benv.replica_dynamics(r).diffuse_sigma for r in range(6)] == [.5, .8, .5] * 2
    pop = BatchedNeuralAutomataAgent(benv, template, rows, episodes=E)
    hpop = BatchedNeuralAutomataAgent(henv, template, rows, episodes=E)
    auto = _searcher(kind, Cn, rows[0]).for_population(pop, T)
    for g in range(G):
        auto.step()
        hpop.set_parameters(pop.parameters)
        henv.reset()
        terms = henv.run(hpop, T)
        f, F = M.fold(terms.cpu().numpy(), Cn, E)
        assert tuple(auto.episode_fitness.shape) == (Cn, E)
        assert np.array_equal(auto.episode_fitness.cpu().numpy(), F)
        assert np.array_equal(auto.fitness.cpu().numpy(), f)
        assert len({tuple(F[:, e]) for e in range(E)}) == E      # the three dynamics score differently
    assert auto.iter == G


# ---------------------------------------------------------------------------------------------------- per-replica regime
def test_per_replica_regime_mixed_dynamics():
    W, H, dt = 64, 48, torch.float32
    benv = BatchedEnv((W, H), _three(W, H, init_agent_ratio=0.15) * 2, replicas=6, seeds=SEEDS, field_dtype=dt, per_replica=True)
    assert benv.per_replica
    template = _template()
    bag = BatchedNeuralAutomataAgent(benv, template, _nca_rows(template, 6))
    rew, alive = BatchedEnv.read_results(benv.run(bag, STEPS))
    assert benv.dynamics.op_food_flow._k == STEPS
    _assert_replicas_alone(benv, lambda r, env: bag.replica_agent(r), rew, alive, W, H, dt)
    benv.reset()
    pag = BatchedPhysarumAgent(benv, seed=7, **PHYS)
    rew, alive = BatchedEnv.read_results(benv.run(pag, STEPS))
    _assert_replicas_alone(benv, lambda r, env: die.PhysarumAgent(max_agents=env.agents.N, seed=7 + r, **PHYS), rew, alive, W, H, dt)
