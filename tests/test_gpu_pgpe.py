"""PGPE search on the device (die_pgpe_sample / die_pgpe_update, die_amd.search.PGPE) and BatchedEnv.reset: the sampling and
the update against the float64 model of tests/pgpe_model.py, a reset batch against a fresh one in both regimes, one generation
of a population against the same rows evaluated on a fresh batch, the sphere the CPU suite calibrates, and a generation loop that
reads nothing back."""

import numpy as np
import pytest
import torch

import die_amd as die
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent
from die_amd.search import PGPE
from tests import pgpe_model as M

pytestmark = pytest.mark.gpu

f32 = np.float32
CFG = dict(center_lr=0.05, stdev_lr=0.1, max_speed=0.1, momentum=0.9)


def _searcher(R, P, optimizer='clipup', seed=7):
    g = torch.Generator().manual_seed(R * 1000 + P)
    center = torch.randn(P, generator=g) * 0.3
    stdev = 0.05 + 0.2 * torch.rand(P, generator=g)
    oc = dict(max_speed=0.1, momentum=0.9) if optimizer == 'clipup' else None
    return PGPE(R, center_init=center, stdev_init=stdev, center_learning_rate=0.05, stdev_learning_rate=0.1, optimizer=optimizer,
                optimizer_config=oc, seed=seed, device='cuda')


def _model_of(s: PGPE, optimizer='clipup') -> M.State:
    st = M.State(s.center.cpu().numpy(), s.stdev.cpu().numpy(), s.R, seed=s.seed, cfg=M.Config(optimizer=optimizer, **CFG))
    st.opt_a = s._opt_a.cpu().numpy().copy()
    if s._opt_b is not None:
        st.opt_b = s._opt_b.cpu().numpy().copy()
    st.evals = s._evals.cpu().numpy().copy()
    st.best = s._best.cpu().numpy().copy()
    return st


def _within_ulps(got, want, k):
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    tol = k * np.spacing(np.maximum(np.abs(got), np.abs(want)))
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= tol


SAMPLE_SHAPES = [(R, P) for R in (2, 10, 64) for P in (1, 162, 4099)] + [(2, 1000003)]


@pytest.mark.parametrize('R, P', SAMPLE_SHAPES)
def test_sample_matches_model(R, P):
    s = _searcher(R, P)
    s.iter = 3                                          # the Philox step word is the generation
    params = torch.empty((R, P), dtype=torch.float32, device='cuda')
    s.ask(params)
    got = params.cpu().numpy()
    want = M.sample(_model_of(s), 3)
    ok = _within_ulps(got, want, 1)
    assert ok.all(), (R, P, np.argwhere(~ok)[:5])
    assert np.mean(got == want) >= 0.999
    c = s.center.cpu().numpy().astype(np.float64)
    up, dn = got[0::2].astype(np.float64) - c, c - got[1::2].astype(np.float64)
    assert np.all(up * dn >= 0)                         # the pair straddles the centre …
    assert np.all(np.abs(up - dn) <= 2 * np.spacing(np.maximum(np.abs(got[0::2]), np.abs(got[1::2])).astype(f32)))   # … symmetrically


def _check_update(s, st, rows, terms, g, optimizer):
    """The device state after the update of generation g against the model's from the same state, rows and terms."""
    want = M.update(st, rows, terms, g)
    assert np.array_equal(s.fitness.cpu().numpy(), want.fitness)
    assert np.array_equal(s._pop_best.cpu().numpy(), want.pop_best)
    assert np.array_equal(s._best.cpu().numpy(), want.best)
    assert np.array_equal(s._evals.cpu().numpy(), want.evals)
    for name, got, ref in (('center', s.center, want.center), ('stdev', s.stdev, want.stdev), ('opt_a', s._opt_a, want.opt_a)) + \
            ((('opt_b', s._opt_b, want.opt_b),) if optimizer == 'adam' else ()):
        ok = _within_ulps(got.cpu().numpy(), ref, 2)
        assert ok.all(), (name, g, np.argwhere(~ok)[:5])
    h = s.history()[g].numpy()
    assert np.array_equal(h[:4], want.history[-1][:4])
    assert np.allclose(h[4:], want.history[-1][4:], rtol=1e-12, atol=0)


@pytest.mark.parametrize('optimizer', ['clipup', 'adam'])
@pytest.mark.parametrize('R, P', [(2, 1), (10, 162), (64, 4099), (2, 1000003)])
def test_update_matches_model_with_ties(R, P, optimizer):
    s = _searcher(R, P, optimizer)
    params = torch.empty((R, P), dtype=torch.float32, device='cuda')
    gen = torch.Generator().manual_seed(R + P)
    for g in range(3):
        st = _model_of(s, optimizer)
        s.ask(params)
        rows = params.cpu().numpy()
        terms = (torch.randint(0, 4, (5, R), generator=gen).double() / 4).numpy()   # quarters: many tied fitnesses
        s.tell(torch.from_numpy(terms).cuda())
        _check_update(s, st, rows, terms, g, optimizer)
    assert s.iter == 3 and s.history().shape == (3, 6)


def _dyn_pred(size):
    return die.Dynamics(food_infinite=False, op_food_flow=die.WaveSequence((size, size), dt=0.01).get_flow_operator(scale=0.5, decay=0.5))


def _st_perlin_wide():
    return die.Dynamics(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8)


def _population(env, R, seed=3):
    torch.manual_seed(seed)
    template = die.NeuralAutomataAgent(kernel_sizes=[3, 3], scale=0.01, deposit=2.0)
    rows = []
    for _ in range(R):
        template.model.init_weights()
        rows.append(torch.nn.utils.parameters_to_vector(template.model.parameters()).detach().clone())
    return BatchedNeuralAutomataAgent(env, template, torch.stack(rows))


@pytest.mark.parametrize('per_replica', [False, True])
def test_reset_equals_fresh_batch(per_replica):
    """An NCA population on the 'dyn-pred' world for 33 steps (the claim epoch wraps), reset, 33 steps again: states and
    rewards are those of a fresh BatchedEnv of the same arguments, bit for bit."""
    size, R, T = 48, 4, 33
    make = lambda: BatchedEnv((size, size), _dyn_pred(size), replicas=R, seeds=[5, 5, 6, 7], per_replica=per_replica)
    benv = make()
    pop = _population(benv, R)
    first = benv.run(pop, T)
    benv.reset()
    assert benv._steps == 0 and (per_replica or benv.epoch == 1) and benv.dynamics.op_food_flow._k == 0
    again = benv.run(pop, T)
    fresh = make()
    pop2 = BatchedNeuralAutomataAgent(fresh, pop.template, pop.parameters)
    want = fresh.run(pop2, T)
    assert torch.equal(first, want) and torch.equal(again, want)
    for r in range(R):
        m, a = benv.replica_numpy(r)
        m2, a2 = fresh.replica_numpy(r)
        assert np.array_equal(m, m2) and np.array_equal(a, a2), r
    benv.reset()                                        # and the state right after a reset is the constructed one
    fresh = make()
    for r in range(R):
        assert all(np.array_equal(x, y) for x, y in zip(benv.replica_numpy(r), fresh.replica_numpy(r))), r


def test_one_generation_equals_evaluation_of_its_rows():
    """One generation on 4 × 48² gives exactly the fitness that evaluating the sampled rows on a fresh BatchedEnv gives
    (population_eval's evaluate_population), and the update then matches the model."""
    size, R, T = 48, 4, 12
    benv = BatchedEnv((size, size), _st_perlin_wide(), replicas=R, seeds=[9] * R)
    pop = _population(benv, R)
    s = PGPE(R, center_init=pop.parameters[0].cpu(), radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1,
             optimizer_config=dict(max_speed=0.1, momentum=0.9), seed=11, device='cuda').for_population(pop, T)
    benv.run(pop, 5)                                    # the worlds have moved on: the generation resets them
    st = _model_of(s)
    s.step()
    rows = pop.parameters.cpu().numpy()
    fresh = BatchedEnv((size, size), _st_perlin_wide(), replicas=R, seeds=[9] * R)
    res = fresh.run(BatchedNeuralAutomataAgent(fresh, pop.template, pop.parameters), T)
    rewards, _ = BatchedEnv.read_results(res)
    want = [sum(rewards[:, r].tolist()) for r in range(R)]
    assert s.fitness.cpu().tolist() == want
    _check_update(s, st, rows, rewards, 0, 'clipup')


def test_sphere_through_ask_and_tell():
    P, R = M.SPHERE_P, M.SPHERE_R
    for seed in (0, 1):
        c0 = -0.5 + torch.rand(P, generator=torch.Generator().manual_seed(seed))
        s = PGPE(R, center_init=c0, seed=seed, device='cuda', **M.REFERENCE)
        params = torch.empty((R, P), dtype=torch.float32, device='cuda')
        for _ in range(M.SPHERE_GENERATIONS):
            s.ask(params)
            s.tell(-(params.double() ** 2).sum(dim=1)[None, :])
        ratio = float(s.center.double().norm() / c0.double().norm())
        assert ratio < M.SPHERE_RATIO, (seed, ratio)
        h = s.history()
        assert h.shape == (M.SPHERE_GENERATIONS, 6) and h[-1, 0] > h[0, 0]


def test_run_reads_nothing_back(monkeypatch):
    size, R = 48, 4
    benv = BatchedEnv((size, size), _dyn_pred(size), replicas=R, seeds=[2] * R)
    pop = _population(benv, R)
    s = PGPE(R, center_init=pop.parameters[0].cpu(), seed=1, device='cuda', **M.REFERENCE).for_population(pop, 3)
    s.run(1)                                            # (first launches outside the patch)

    def no_host_read(*a, **k):
        raise AssertionError('host read inside PGPE.run')
    for name in ('cpu', 'item', 'tolist', 'numpy'):
        monkeypatch.setattr(torch.Tensor, name, no_host_read)
    monkeypatch.setattr(torch.cuda, 'synchronize', no_host_read)
    s.run(70)                                           # (crosses the history's first growth, 64 rows)
    monkeypatch.undo()
    assert s.iter == 71 and s.history().shape == (71, 6)
    st = s.status
    assert st['iter'] == 71 and st['best_eval'] >= st['pop_best_eval'] and st['center'].shape == (pop.P,)
    assert st['mean_eval'] == float(s.history()[-1, 0]) and st['median_eval'] == float(s.history()[-1, 3])
    best = s.best_agent()
    assert torch.equal(torch.nn.utils.parameters_to_vector(best.model.parameters()).detach(), st['best'])
    assert torch.equal(torch.nn.utils.parameters_to_vector(s.center_agent().model.parameters()).detach(), st['center'])


def test_refusals():
    size = 48
    benv = BatchedEnv((size, size), _st_perlin_wide(), replicas=4, seeds=[2] * 4)
    pop = _population(benv, 4)
    kw = dict(center_init=pop.parameters[0].cpu(), seed=1, device='cuda', **M.REFERENCE)
    with pytest.raises(ValueError, match='popsize 5'):
        PGPE(5, **kw)
    with pytest.raises(ValueError, match="popsize 6 != the population's 4"):
        PGPE(6, **kw).for_population(pop, 3)
    other = BatchedEnv((size, size), _st_perlin_wide(), replicas=4, seeds=[2] * 4)
    with pytest.raises(ValueError, match='another BatchedEnv'):
        PGPE(4, **kw).for_population(pop, 3, env=other)
    with pytest.raises(RuntimeError, match='for_population'):
        PGPE(4, **kw).step()
    s = PGPE(4, **kw)
    with pytest.raises(ValueError, match='params'):
        s.ask(torch.empty((4, pop.P + 1), dtype=torch.float32, device='cuda'))
    with pytest.raises(RuntimeError, match='before ask'):
        s.tell(torch.zeros((3, 4), dtype=torch.float64, device='cuda'))
