"""Seeded agent dropout on the GPU (die_dropout_mask, die_conv2d_dropout, die_nca_env_step_batch_dropout): the device mask is the
numpy twin's (tests/dropout_model.py), a stand-alone agent's masked planes are its eval-mode planes times that mask, and replica r
of a batched population is the stand-alone run of `NeuralAutomataAgent(dropout_seed=S + r·stride)`.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent
from die_amd.device_array import _ptr
from die_amd.search import CMAES, PGPE
from tests import dropout_model as M

pytestmark = pytest.mark.gpu

REFERENCE_DYNAMICS = dict(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8)     # examples/learning_agents.py
DEV = 'cuda:0'


def _device_masks(W, H, p, seed, stride, step, R, pad=0):
    out = torch.full((R, W * H + pad), -7.0, dtype=torch.float32, device=DEV)
    d = _lib.nca_dropout(p, seed, stride, step)
    _lib.check(_lib.lib.die_dropout_mask(W, H, C.byref(d), R, W * H + pad, _ptr(out), None), 'die_dropout_mask')
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[:, W * H:] == -7.0).all()                        # nothing written between the planes
    return host[:, :W * H].reshape(R, W, H)


# ---------------------------------------------------------------------------------------------------- 1. the mask
@pytest.mark.parametrize('W,H', [(96, 96), (64, 128), (30, 50), (17, 23)])
@pytest.mark.parametrize('p', [0.25, 0.5, 1.0])
def test_device_mask_is_the_twin(W, H, p):
    for seed, step in ((0, 0), (1, 7), (2 ** 63 + 12345, 2 ** 32 - 1), (2 ** 64 - 1, 33)):
        for stride, pad in ((0, 0), (1, 5)):
            got = _device_masks(W, H, p, seed, stride, step, 3, pad)
            assert np.array_equal(got, M.replica_masks(seed, stride, step, 3, W, H, p)), (seed, step, stride)
            if p == 1.0:
                assert (got == 0).all()


# ---------------------------------------------------------------------------------------------------- 2. stand-alone sense
def _agent(seed, p, **kw):
    torch.manual_seed(seed)
    ag = die.NeuralAutomataAgent(scale=0.01, deposit=2.0, p_agent_dropout=p, **kw)
    ag.model.init_weights()
    return ag


@pytest.mark.parametrize('W,H,f16,kernel_sizes,boundary', [
    (96, 96, False, (3, 3), 'circular'),
    (64, 48, True, (3,), 'circular'),
    (30, 50, False, (3, 5), 'zeros'),                             # H % 4 != 0: the mask cell by cell
    (17, 23, True, (3,), 'reflect'),
    (64, 130, False, (3, 5), 'replicate'),                        # H % 4 != 0 across three column tiles
])
def test_stand_alone_sense_is_eval_planes_times_the_twin_mask(W, H, f16, kernel_sizes, boundary):
    p, S = 0.25, 2 ** 40 + 9
    dt = torch.float16 if f16 else torch.float32
    rs = np.random.RandomState(W * 31 + H)
    medium = np.stack([(rs.rand(W, H) < 0.15).astype(np.float64), rs.rand(W, H), rs.rand(W, H)])
    agents = np.stack([rs.rand(8), rs.rand(8), np.ones(8), np.ones(8)])               # (only the medium is sensed)
    env = die.Env.from_numpy(medium, agents, field_dtype=dt)
    ag = _agent(W + H, p, kernel_sizes=kernel_sizes, boundary=boundary, dropout_seed=S)
    assert ag.model.training and ag.dropout_step == 0
    ag.model.eval()
    plain = ag.sense(env.medium).cpu().numpy().copy()             # eval mode: no mask (the counter still counts the call)
    assert plain.dtype == np.float32 and plain.shape == (3, W, H) and ag.dropout_step == 1
    ag.model.train()
    for step in (1, 2, 2 ** 32 + 5):
        ag.dropout_step = step
        got = ag.sense(env.medium).cpu().numpy()
        assert ag.dropout_step == step + 1
        want = (plain * M.mask(S, step, W, H, p)[None]).astype(np.float32)
        assert np.array_equal(got, want), step
        assert not np.array_equal(got, plain)
    ag.dropout_step = 1
    again = ag.sense(env.medium).cpu().numpy()
    assert np.array_equal(again, (plain * M.mask(S, 1, W, H, p)[None]).astype(np.float32))     # the same call, the same mask
    one = _agent(W + H, 1.0, kernel_sizes=kernel_sizes, boundary=boundary, dropout_seed=S)     # p = 1: every cell dropped
    assert (one.sense(env.medium).cpu().numpy() == 0).all()


# ---------------------------------------------------------------------------------------------------- 3. batched = stand-alone
def _population(R, seed, p, **kw):
    torch.manual_seed(seed)
    agents = []
    for _ in range(R):
        ag = die.NeuralAutomataAgent(scale=0.01, deposit=2.0, p_agent_dropout=p, **kw)
        ag.model.init_weights()
        agents.append(ag)
    return agents


def _run_alone(env, agent, steps):
    obs, rew, alive = env._get_current_obs, [], []
    for _ in range(steps):
        obs, rw, _, _, info = env.step(agent.forward(obs))
        rew.append(rw)
        alive.append(info['num_agents'])
    return np.array(rew), np.array(alive)


def _wave(W, H):
    return die.WaveSequence((W, H), dt=0.01).get_flow_operator(scale=0.5, decay=0.5)


def _assert_replica_is(benv, pop, r, env, ag, rew, alive, want_rew, want_alive):
    m, a = benv.replica_numpy(r)
    assert np.array_equal(m, env.medium.to_numpy()), r
    assert np.array_equal(a, env.agents.to_numpy()), r
    assert np.array_equal(rew[:, r], want_rew), r
    assert np.array_equal(alive[:, r], want_alive), r
    assert np.array_equal(pop.render(r), ag.render()[0]), r


@pytest.mark.parametrize('case', ['reference', 'fp16_zeros', 'episodes_die_fixed', 'wave_flow', 'per_replica'])
def test_batched_replica_is_the_stand_alone_run_of_its_key(case):
    """36 steps: the claim plane's 5-bit epoch wraps once."""
    S, stride, T, p = 1000, 3, 36, 0.25
    W, H, R, E, dt, slots, per_replica, boundary, sizes = 96, 96, 4, 1, torch.float32, 'alive', False, 'circular', (3, 3)
    dyn = lambda: die.Dynamics(**REFERENCE_DYNAMICS)
    if case == 'fp16_zeros':
        W, H, dt, boundary, sizes = 64, 48, torch.float16, 'zeros', (3,)
        dyn = lambda: die.Dynamics(init_agent_ratio=0.15)
    elif case == 'episodes_die_fixed':
        W, H, E, slots = 64, 48, 2, 700
        dyn = lambda: die.Dynamics(agents_die=True, init_agent_ratio=0.15, **dict(REFERENCE_DYNAMICS, food_infinite=False))
    elif case == 'wave_flow':
        W, H = 64, 64
        dyn = lambda: die.Dynamics(food_infinite=False, op_food_flow=_wave(W, H))
    elif case == 'per_replica':
        W, H, R, T, per_replica = 64, 48, 3, 6, True
    cands = _population(R // E, W + R, p, kernel_sizes=sizes, boundary=boundary)
    seeds = [11 + 5 * r for r in range(R)]
    benv = BatchedEnv((W, H), dyn(), replicas=R, seeds=seeds, field_dtype=dt, max_agents=slots, per_replica=per_replica)
    assert benv.per_replica == per_replica
    pop = BatchedNeuralAutomataAgent.from_agents(benv, cands, E, dropout_seed=S, dropout_seed_stride=stride)
    assert pop.template.model.training and pop.dropout_step == 0 and (pop.dropout_seed, pop.dropout_seed_stride) == (S, stride)
    rew, alive = BatchedEnv.read_results(benv.run(pop, T))
    assert pop.dropout_step == T
    for r in range(R):
        env = die.Env((W, H), dyn(), seed=seeds[r], max_agents=slots, field_dtype=dt)
        ag = pop.replica_agent(r)
        assert ag.dropout_seed == S + r * stride and ag.dropout_step == 0 and ag.model.training
        for q, want in zip(ag.model.parameters(), cands[r // E].model.parameters()):
            assert torch.equal(q, want)
        want_rew, want_alive = _run_alone(env, ag, T)
        _assert_replica_is(benv, pop, r, env, ag, rew, alive, want_rew, want_alive)
        assert (pop.render(r)[..., 0] == 0).mean() > 0.1          # the planes that stay in scratch hold the masked values
    # candidate(c) carries the key of its first replica
    assert pop.candidate(R // E - 1).dropout_seed == S + (R // E - 1) * E * stride
    # the same run without the mask is another run
    benv2 = BatchedEnv((W, H), dyn(), replicas=R, seeds=seeds, field_dtype=dt, max_agents=slots, per_replica=per_replica)
    pop2 = BatchedNeuralAutomataAgent.from_agents(benv2, cands, E, dropout_seed=S, dropout_seed_stride=stride)
    pop2.template.model.eval()
    rew2, _ = BatchedEnv.read_results(benv2.run(pop2, T))
    pop2.template.model.train()
    assert not np.array_equal(rew2, rew)


# ---------------------------------------------------------------------------------------------------- 4. strides
def test_stride_zero_keeps_identical_candidates_identical_and_stride_one_does_not():
    W, H, R, T = 96, 96, 4, 5
    cand = _population(1, 33, 0.25, kernel_sizes=(3, 3))[0]
    runs = {}
    for stride in (0, 1):
        benv = BatchedEnv((W, H), die.Dynamics(**REFERENCE_DYNAMICS), replicas=R, seeds=[77] * R)
        pop = BatchedNeuralAutomataAgent(benv, cand, dropout_seed=5, dropout_seed_stride=stride)       # every row: the template's weights
        rew, _ = BatchedEnv.read_results(benv.run(pop, T))
        runs[stride] = (benv, pop, rew)
    benv, pop, rew = runs[0]
    first = benv.replica_numpy(0)
    for r in range(1, R):
        m, a = benv.replica_numpy(r)
        assert np.array_equal(m, first[0]) and np.array_equal(a, first[1]) and np.array_equal(rew[:, r], rew[:, 0]), r
        assert np.array_equal(pop.render(r), pop.render(0)), r
    benv1, pop1, rew1 = runs[1]
    assert np.array_equal(rew1[:, 0], rew[:, 0])                  # replica 0 has key 5 under either stride
    for x, y in zip(benv1.replica_numpy(0), first):
        assert np.array_equal(x, y)
    for r in range(1, R):
        assert not np.array_equal(benv1.replica_numpy(r)[1], benv1.replica_numpy(0)[1]), r
        assert not np.array_equal(rew1[:, r], rew1[:, 0]), r
        assert not np.array_equal(pop1.render(r), pop1.render(0)), r


# ---------------------------------------------------------------------------------------------------- 5. eval mode
@pytest.mark.parametrize('per_replica', [False, True])
def test_eval_mode_with_a_seed_is_the_template_without_dropout(per_replica):
    W, H, R, T = 64, 48, 3, 6
    dyn = lambda: die.Dynamics(init_agent_ratio=0.15, **REFERENCE_DYNAMICS)
    with_p = _population(R, 8, 0.5, kernel_sizes=(3, 3))
    without = _population(R, 8, 0.0, kernel_sizes=(3, 3))         # the same seed: the same weights
    out = []
    for cands, kw in ((with_p, dict(dropout_seed=4)), (without, dict(dropout_seed=4)), (without, {})):
        benv = BatchedEnv((W, H), dyn(), replicas=R, seed=2, per_replica=per_replica)
        pop = BatchedNeuralAutomataAgent.from_agents(benv, cands, **kw)
        if cands is with_p:
            pop.template.model.eval()
        res = benv.run(pop, T).cpu()
        assert pop.dropout_step == (T if kw else 0)
        out.append((res, [benv.replica_numpy(r) for r in range(R)], [pop.render(r) for r in range(R)]))
    for other in out[1:]:
        assert torch.equal(out[0][0], other[0])
        for r in range(R):
            assert all(np.array_equal(x, y) for x, y in zip(out[0][1][r], other[1][r])), r
            assert np.array_equal(out[0][2][r], other[2][r]), r


# ---------------------------------------------------------------------------------------------------- 6. replay
def test_setting_the_counter_back_replays_the_steps():
    W, H, R = 64, 48, 4
    cands = _population(R, 12, 0.25, kernel_sizes=(3, 3))
    benv = BatchedEnv((W, H), die.Dynamics(init_agent_ratio=0.15, **REFERENCE_DYNAMICS), replicas=R, seed=6)
    pop = BatchedNeuralAutomataAgent.from_agents(benv, cands, dropout_seed=21)
    benv.run(pop, 3)
    torch.cuda.synchronize()
    saved = (benv._state.clone(), benv.chem, benv.chem_next, benv.epoch, benv._steps, pop.dropout_step)
    assert saved[5] == 3
    first = benv.run(pop, 4).clone()
    end = benv._state.clone()
    benv._state.copy_(saved[0])
    benv.chem, benv.chem_next, benv.epoch, benv._steps = saved[1:5]
    stale = benv.run(pop, 4).clone()                              # the state restored, the counter not: other masks, another run
    assert not torch.equal(stale, first)
    benv._state.copy_(saved[0])
    benv.chem, benv.chem_next, benv.epoch, benv._steps = saved[1:5]
    pop.dropout_step = saved[5]
    again = benv.run(pop, 4)
    assert torch.equal(again, first) and torch.equal(benv._state, end) and pop.dropout_step == 7


# ---------------------------------------------------------------------------------------------------- 7. the searchers
def _search(kind, popsize, P, pop, T):
    if kind == 'pgpe':
        s = PGPE(popsize, P, radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1, optimizer='clipup',
                 optimizer_config=dict(max_speed=0.1, momentum=0.9), seed=4)
    else:
        s = CMAES(popsize, P, stdev_init=0.1, seed=4)
    return s.for_population(pop, T)


@pytest.mark.parametrize('kind', ['pgpe', 'cmaes'])
def test_search_with_dropout_is_reproducible_and_its_candidates_replay(kind):
    size, R, T, G, p, S = 96, 10, 30, 3, 0.25, 17
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        template = die.NeuralAutomataAgent(kernel_sizes=[3, 3], scale=0.01, deposit=2.0, p_agent_dropout=p)
        benv = BatchedEnv((size, size), die.Dynamics(**REFERENCE_DYNAMICS), replicas=R, seeds=[0] * R)
        pop = BatchedNeuralAutomataAgent(benv, template, dropout_seed=S)
        s = _search(kind, R, pop.P, pop, T)
        s.run(G)
        assert pop.dropout_step == G * T                          # nothing reset the counter: every generation saw new masks
        runs.append((s, benv, pop))
    (a, benv, pop), (b, _, pop_b) = runs
    assert torch.equal(a.history(), b.history())
    assert torch.equal(torch.as_tensor(a.center).cpu(), torch.as_tensor(b.center).cpu())
    assert torch.equal(a._best.cpu(), b._best.cpu()) and torch.equal(a._pop_best.cpu(), b._pop_best.cpu())
    assert torch.equal(a.fitness.cpu(), b.fitness.cpu()) and torch.equal(pop.parameters, pop_b.parameters)
    assert not torch.isnan(a.history()).any()
    # the last generation's winner and its losing pair (PGPE: rows 2i, 2i + 1; CMAES: the two lowest), replayed alone
    f = a.fitness.cpu().numpy()
    win = int(np.argmax(f))
    lose = int(np.argmin(f))
    check = {win, lose, lose ^ 1} if kind == 'pgpe' else {win, lose, int(np.argsort(f)[1])}
    assert torch.equal(pop.parameters[win], a._pop_best)
    for r in sorted(check):
        ag = pop.candidate(r)
        assert ag.dropout_seed == S + r and ag.model.training
        ag.dropout_step = (G - 1) * T                             # where the population's counter stood when generation G − 1 began
        env = die.Env((size, size), die.Dynamics(**REFERENCE_DYNAMICS), seed=0, max_agents='alive')
        rew, _ = _run_alone(env, ag, T)
        total = 0.0
        for x in rew.tolist():                                    # summed in step order, in float64, as the update sums
            total += x
        assert total == f[r], (r, total, f[r])
        m, ag_arrays = benv.replica_numpy(r)
        assert np.array_equal(m, env.medium.to_numpy()) and np.array_equal(ag_arrays, env.agents.to_numpy()), r


# ---------------------------------------------------------------------------------------------------- 8. refusals
def _snapshot(benv, pop):
    torch.cuda.synchronize()
    return (benv.epoch, benv._steps, pop.dropout_step, pop._calls), [tuple(x.copy() for x in benv.replica_numpy(r)) for r in range(benv.R)]


def _unchanged(before, after):
    return before[0] == after[0] and all(np.array_equal(x, y) for p, q in zip(before[1], after[1]) for x, y in zip(p, q))


def test_refusals_leave_the_batch_unchanged():
    W, H, R = 64, 64, 3
    benv = BatchedEnv((W, H), die.Dynamics(**REFERENCE_DYNAMICS), replicas=R, seed=1)
    drop = die.NeuralAutomataAgent(kernel_sizes=(3,), p_agent_dropout=0.5)
    # no key: the refusal of before, and its message now names the way out
    bare = BatchedNeuralAutomataAgent(benv, drop)
    before = _snapshot(benv, bare)
    with pytest.raises(NotImplementedError, match='dropout_seed'):
        benv.step(bare)
    assert _unchanged(before, _snapshot(benv, bare))
    # bad keywords are refused at construction
    for kw in (dict(dropout_seed=1.5), dict(dropout_seed=True), dict(dropout_seed=1, dropout_seed_stride=-1),
               dict(dropout_seed=1, dropout_seed_stride=0.5)):
        with pytest.raises(ValueError, match='dropout_seed'):
            BatchedNeuralAutomataAgent(benv, drop, **kw)
    pop = BatchedNeuralAutomataAgent(benv, drop, dropout_seed=3)
    before = _snapshot(benv, pop)
    # a population of another batch
    other = BatchedEnv((W, H), die.Dynamics(**REFERENCE_DYNAMICS), replicas=R, seed=1)
    with pytest.raises(ValueError, match='another BatchedEnv'):
        other.step(pop)
    # a parameter matrix of the wrong height
    good = pop.parameters
    pop.parameters = torch.zeros((R + 1, pop.P), device=benv.device)
    with pytest.raises(ValueError):
        benv.step(pop)
    pop.parameters = good
    # a p the library refuses (nn.Dropout's own check was bypassed): refused by die_nca_env_step_batch_dropout before any launch
    drop.model.agent_dropout.p = 1.5
    with pytest.raises(_lib.DieError, match='0 < p <= 1'):
        benv.step(pop)
    drop.model.agent_dropout.p = 0.5
    assert _unchanged(before, _snapshot(benv, pop))
    # a host food-flow operator is not batched, with or without a key
    flow = BatchedEnv((W, H), die.Dynamics(op_food_flow=lambda food: food * 0.5, **REFERENCE_DYNAMICS), replicas=R, seed=1)
    fpop = BatchedNeuralAutomataAgent(flow, drop, dropout_seed=3)
    fb = _snapshot(flow, fpop)
    with pytest.raises(NotImplementedError, match='food-flow'):
        flow.step(fpop)
    assert _unchanged(fb, _snapshot(flow, fpop))
    # the device entry points refuse before they launch: the output keeps its bytes
    out = torch.full((R, W * H), -7.0, dtype=torch.float32, device=DEV)
    for p, replicas, stride in ((0.0, R, W * H), (float('nan'), R, W * H), (0.25, 0, W * H), (0.25, 65, W * H), (0.25, R, W * H - 1)):
        d = _lib.nca_dropout(p, 1, 1, 0)
        assert _lib.lib.die_dropout_mask(W, H, C.byref(d), replicas, stride, _ptr(out), None) == -1
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    # and after all that the population still steps
    benv.step(pop)
    assert pop.dropout_step == 1 and benv._steps == 1
