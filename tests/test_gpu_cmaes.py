"""Separable CMA-ES on the device (die_cmaes_sample / die_cmaes_update, die_amd.search.CMAES): the sampling and the update
against the float64 model of tests/cmaes_model.py (active or not, either step-size rule, many tied fitnesses), a generation
whose model has h_sigma = 0, one generation of a population against the same rows evaluated on a fresh batch, a generation
loop that reads nothing back, and the ellipsoid the CPU suite calibrates."""

import numpy as np
import pytest
import torch

import die_amd as die
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent
from die_amd.search import CMAES
from tests import cmaes_model as M

pytestmark = pytest.mark.gpu

f32 = np.float32


def _searcher(R, P, seed=7, **kw):
    g = torch.Generator().manual_seed(R * 1000 + P)
    center = torch.randn(P, generator=g) * 0.3
    return CMAES(R, center_init=center, stdev_init=0.2, seed=seed, device='cuda', **kw)


def _model_of(s: CMAES, cfg: M.Config) -> M.State:
    """The model at the searcher's current device state."""
    st = M.State(s.center.cpu().numpy(), s.sigma, s.R, seed=s.seed, cfg=cfg)
    st.C, st.ps, st.pc = s.C.numpy().copy(), s.p_sigma.numpy().copy(), s.p_c.numpy().copy()
    st.evals = s._evals.cpu().numpy().copy()
    st.best = s._best.cpu().numpy().copy()
    return st


def _within_ulps(got, want, k):
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    tol = k * np.spacing(np.maximum(np.abs(got), np.abs(want)))
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= tol


SAMPLE_SHAPES = [(2, 1), (10, 162), (19, 162), (64, 4099), (3, 1000003)]


@pytest.mark.parametrize('R, P', SAMPLE_SHAPES)
def test_sample_matches_model(R, P):
    s = _searcher(R, P)
    s._C.copy_(torch.linspace(0.25, 4.0, P, dtype=torch.float64))        # a non-trivial C
    s._sigma[1] = 0.07
    s.iter = 3                                          # the Philox step word is the generation; sigma[3 & 1]
    params = torch.empty((R, P), dtype=torch.float32, device='cuda')
    s.ask(params)
    got = params.cpu().numpy()
    st = _model_of(s, M.Config())
    assert st.sigma == 0.07
    want = M.sample(st, 3)
    ok = _within_ulps(got, want, 1)
    assert ok.all(), (R, P, np.argwhere(~ok)[:5])
    assert np.mean(got == want) >= 0.999


def _check_update(s, st, rows, terms, g):
    """The device state after the update of generation g against the model's from the same state, rows and terms."""
    want = M.update(st, rows, terms, g)
    assert abs(want.h_margin[-1] - 1.0) > 1e-9           # (h_sigma is not at the mercy of the last bits)
    assert np.array_equal(s.fitness.cpu().numpy(), want.fitness)
    assert np.array_equal(s._work[:s.R].cpu().numpy().astype(np.int64), want.order)
    assert np.array_equal(s._pop_best.cpu().numpy(), want.pop_best)
    assert np.array_equal(s._best.cpu().numpy(), want.best)
    assert np.array_equal(s._evals.cpu().numpy(), want.evals)
    for name, got, ref in (('m', s.center.cpu().numpy(), want.m), ('C', s.C.numpy(), want.C), ('p_sigma', s.p_sigma.numpy(), want.ps),
                           ('p_c', s.p_c.numpy(), want.pc)):
        # (rtol 1e-12, with a floor of 1e-12 of the largest entry: an entry near 0 comes out of a cancellation, m + dm)
        floor = 1e-12 * float(np.max(np.abs(ref)))
        assert np.allclose(got, ref, rtol=1e-12, atol=floor), (name, g, np.max(np.abs(got - ref) / (np.abs(ref) + floor)))
    assert s.sigma == pytest.approx(want.sigma, rel=1e-12)
    h = s.history()[g].numpy()
    assert np.array_equal(h[:4], want.history[-1][:4])
    assert np.allclose(h[4:], want.history[-1][4:], rtol=1e-12, atol=0)
    return want


@pytest.mark.parametrize('csa_squared', [False, True])
@pytest.mark.parametrize('active', [True, False])
@pytest.mark.parametrize('R, P', SAMPLE_SHAPES)
def test_update_matches_model_with_ties(R, P, active, csa_squared):
    cfg = M.Config(active=active, csa_squared=csa_squared)
    s = _searcher(R, P, active=active, csa_squared=csa_squared)
    params = torch.empty((R, P), dtype=torch.float32, device='cuda')
    gen = torch.Generator().manual_seed(R + P)
    st = _model_of(s, cfg)
    for g in range(4):
        s.ask(params)
        rows = params.cpu().numpy()
        ok = _within_ulps(rows, M.sample(st, g), 2)
        assert ok.all(), (g, np.argwhere(~ok)[:5])
        terms = (torch.randint(0, 4, (5, R), generator=gen).double() / 4).numpy()   # quarters: many tied fitnesses
        s.tell(torch.from_numpy(terms).cuda())
        st = _check_update(s, st, rows, terms, g)
    s.ask(params)                                       # the next generation's rows, from the updated state
    ok = _within_ulps(params.cpu().numpy(), M.sample(st, 4), 2)
    assert ok.all(), np.argwhere(~ok)[:5]
    assert s.iter == 4 and s.history().shape == (4, 6)


def test_h_sigma_zero_generations_match_model():
    """A linear fitness (f = Σ x) on d = 2, λ = 10: the evolution path outgrows its threshold, and the model has h_sigma = 0
    in generations 3..5, every generation at least 5 % away from the threshold, so the device cannot round to the other side."""
    R, P = 10, 2
    cfg = M.Config()
    s = CMAES(R, center_init=torch.zeros(P), stdev_init=0.1, seed=1, device='cuda')
    params = torch.empty((R, P), dtype=torch.float32, device='cuda')
    st = _model_of(s, cfg)
    for g in range(6):
        s.ask(params)
        rows = params.cpu().numpy()
        terms = rows.astype(np.float64).sum(axis=1).reshape(1, R).copy()     # (a (1, R) view would have stride 0)
        s.tell(torch.from_numpy(terms).cuda())
        st = _check_update(s, st, rows, terms, g)
    assert st.h_sigma[3:] == [0.0, 0.0, 0.0] and 1.0 in st.h_sigma[:3], st.h_sigma
    assert all(abs(m - 1.0) > 0.05 for m in st.h_margin), st.h_margin


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


def test_one_generation_equals_evaluation_of_its_rows():
    """One generation on 5 × 48² gives exactly the fitness that evaluating the sampled rows on a fresh BatchedEnv gives, and
    the update then matches the model."""
    size, R, T = 48, 5, 12
    benv = BatchedEnv((size, size), _st_perlin_wide(), replicas=R, seeds=[9] * R)
    pop = _population(benv, R)
    s = CMAES(R, center_init=pop.parameters[0].cpu(), stdev_init=0.1, seed=11, device='cuda').for_population(pop, T)
    benv.run(pop, 5)                                    # the worlds have moved on: the generation resets them
    st = _model_of(s, M.Config())
    s.step()
    rows = pop.parameters.cpu().numpy()
    fresh = BatchedEnv((size, size), _st_perlin_wide(), replicas=R, seeds=[9] * R)
    res = fresh.run(BatchedNeuralAutomataAgent(fresh, pop.template, pop.parameters), T)
    rewards, _ = BatchedEnv.read_results(res)
    want = [sum(rewards[:, r].tolist()) for r in range(R)]
    assert s.fitness.cpu().tolist() == want
    _check_update(s, st, rows, rewards, 0)


def test_run_reads_nothing_back(monkeypatch):
    size, R = 48, 4
    benv = BatchedEnv((size, size), _st_perlin_wide(), replicas=R, seeds=[2] * R)
    pop = _population(benv, R)
    s = CMAES(R, center_init=pop.parameters[0].cpu(), stdev_init=0.1, seed=1, device='cuda').for_population(pop, 3)
    s.run(1)                                            # (first launches outside the patch)

    def no_host_read(*a, **k):
        raise AssertionError('host read inside CMAES.run')
    for name in ('cpu', 'item', 'tolist', 'numpy'):
        monkeypatch.setattr(torch.Tensor, name, no_host_read)
    monkeypatch.setattr(torch.cuda, 'synchronize', no_host_read)
    s.run(70)                                           # (crosses the history's first growth, 64 rows)
    monkeypatch.undo()
    assert s.iter == 71 and s.history().shape == (71, 6)
    h = s.history()
    assert torch.isfinite(h).all() and (h[:, 4] > 0).all() and (h[:, 5] > 0).all()
    st = s.status
    assert st['iter'] == 71 and st['best_eval'] >= st['pop_best_eval'] and st['center'].shape == (pop.P,)
    assert st['sigma'] == float(h[-1, 4]) and st['mean_eval'] == float(h[-1, 0]) and st['median_eval'] == float(h[-1, 3])
    assert torch.allclose(st['stdev'].mean(), h[-1, 5], rtol=1e-12, atol=0)
    best = s.best_agent()
    assert torch.equal(torch.nn.utils.parameters_to_vector(best.model.parameters()).detach(), st['best'])
    assert torch.equal(torch.nn.utils.parameters_to_vector(s.center_agent().model.parameters()).detach(), st['center'].float())


def test_ellipsoid_through_ask_and_tell():
    d, R = M.ELLIPSOID_D, M.ELLIPSOID_R
    scales = torch.from_numpy(M.ellipsoid_scales(d)).cuda()
    for seed in (0, 1):
        c0 = -0.5 + torch.rand(d, generator=torch.Generator().manual_seed(seed))
        s = CMAES(R, center_init=c0, stdev_init=M.ELLIPSOID_SIGMA, seed=seed, device='cuda')
        params = torch.empty((R, d), dtype=torch.float32, device='cuda')
        for _ in range(M.ELLIPSOID_GENERATIONS):
            s.ask(params)
            x = params.double()
            s.tell(-(scales * x * x).sum(dim=1)[None, :])
        C = s.C
        cond = float(C[0] / C[-1])
        f = lambda x: float((M.ellipsoid_scales(d) * x.double().cpu().numpy() ** 2).sum())
        gain = f(c0) / f(s.center)
        assert cond > M.ELLIPSOID_COND and gain > M.ELLIPSOID_GAIN, (seed, cond, gain)
        assert s.history().shape == (M.ELLIPSOID_GENERATIONS, 6)


def test_refusals():
    size = 48
    benv = BatchedEnv((size, size), _st_perlin_wide(), replicas=4, seeds=[2] * 4)
    pop = _population(benv, 4)
    kw = dict(center_init=pop.parameters[0].cpu(), stdev_init=0.1, seed=1, device='cuda')
    with pytest.raises(ValueError, match='popsize 65'):
        CMAES(65, **kw)
    with pytest.raises(ValueError, match="popsize 5 != the population's 4"):
        CMAES(5, **kw).for_population(pop, 3)
    other = BatchedEnv((size, size), _st_perlin_wide(), replicas=4, seeds=[2] * 4)
    with pytest.raises(ValueError, match='another BatchedEnv'):
        CMAES(4, **kw).for_population(pop, 3, env=other)
    with pytest.raises(RuntimeError, match='for_population'):
        CMAES(4, **kw).step()
    s = CMAES(4, **kw)
    with pytest.raises(ValueError, match='params'):
        s.ask(torch.empty((4, pop.P + 1), dtype=torch.float32, device='cuda'))
    with pytest.raises(RuntimeError, match='before ask'):
        s.tell(torch.zeros((3, 4), dtype=torch.float64, device='cuda'))
    params = torch.empty((4, pop.P), dtype=torch.float32, device='cuda')
    s.ask(params)
    with pytest.raises(ValueError, match='terms'):
        s.tell(torch.zeros((3, 5), dtype=torch.float64, device='cuda'))
    s.tell(torch.zeros((3, 4), dtype=torch.float64, device='cuda'))
    with pytest.raises(RuntimeError, match='before ask\\(\\) of generation 1'):     # z of generation 1 was never drawn
        s.tell(torch.zeros((3, 4), dtype=torch.float64, device='cuda'))
    with pytest.raises(ValueError, match='stdev_init'):
        CMAES(4, center_init=pop.parameters[0].cpu(), stdev_init=-1.0, device='cuda')
