"""Episodes (each candidate evaluated on E worlds per generation), CPU side: the new entry points are exported and declared
with the ABI unchanged, every bad argument is refused on the host before any launch — through the library and through the
classes on device='cpu' — and the seed formulas reduce to today's at E = 1.  No kernel is launched here: the device pointers
below are never dereferenced."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import episodes_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('die_init_batch_seeds', 'die_pgpe_update_episodes', 'die_cmaes_update_episodes', 'die_physarum_decode_episodes')


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


def test_entry_points_exported_declared_and_abi_unchanged(lib):
    so = C.CDLL(lib.LIB_PATH)
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'die_hip.h')).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert hasattr(so, name) and name in lib.EXPORTS, name
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    # die_nca_batch.episodes took the place of `reserved`: same offset, same size
    assert lib.NcaBatch.episodes.offset == lib.NcaBatch.coef.offset + 12 and C.sizeof(lib.NcaBatch) == 56
    assert re.search(r'int32_t\s+episodes\s*;', text)
    import die_amd
    from die_amd import batch
    assert die_amd.episode_seeds is batch.episode_seeds


FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host
R, N, W, H = 4, 100, 96, 96


def _last(lib):
    return lib.lib.die_last_error().decode()


# ---------------------------------------------------------------------------------------------------- die_init_batch_seeds
def _init_args(lib, replicas=R):
    from die_amd.data_init import food_spec_from_seed
    m = lib.Medium(W, H, lib.DIE_F32, 1, FAKE, FAKE, FAKE, FAKE + 8, 0, 0, 0, 0, 0, 0, 0, 0, None)
    a = lib.Agents(N, FAKE, FAKE, FAKE, FAKE, None)
    b = lib.Batch(replicas, 0, W * H, N, 1, (C.c_int64 * 64)(*([N] * 64)))
    spec = food_spec_from_seed(3, scale=0.5, perlin_octaves=8, threshold=1.0)
    return m, a, b, spec


def _init_seeds(lib, seeds, n=None, replicas=R, ws_bytes=None, spec_edit=None, null_seeds=False):
    m, a, b, spec = _init_args(lib, replicas)
    if spec_edit:
        spec_edit(spec)
    arr = (C.c_uint64 * max(1, len(seeds)))(*seeds)
    ws_bytes = lib.lib.die_init_batch_workspace_bytes(W, H, max(1, min(replicas, 64))) if ws_bytes is None else ws_bytes
    return lib.lib.die_init_batch_seeds(C.byref(m), C.byref(a), C.byref(b), 0.1, None if null_seeds else arr,
                                        len(seeds) if n is None else n, C.byref(spec), FAKE, FAKE, ws_bytes, None)


def test_seed_list_refusals_at_the_c_boundary(lib):
    cases = [
        (dict(seeds=list(range(65)), replicas=64), '65 seeds, 1..64 expected'),            # longer than 64
        (dict(seeds=[1], n=0), '0 seeds, 1..64 expected'),
        (dict(seeds=[1, 2, 3, 4], null_seeds=True), 'null seed list'),
        (dict(seeds=[1, 2, 3]), '3 seeds for 4 replicas'),                                 # not one per replica
        (dict(seeds=[1, 2, 3, 4, 5]), '5 seeds for 4 replicas'),
        (dict(seeds=[1, 2, 3, 4], replicas=65), 'replicas'),
        (dict(seeds=[7, 7, 8, 7], spec_edit=lambda s: setattr(s, 'perlin_octaves', 0)), 'wave-mix'),
        (dict(seeds=[5, 9, 5, 2], ws_bytes=8), 'workspace too small'),                     # a list with a repeat passes every other check
        (dict(seeds=[7, 7, 7, 7], ws_bytes=8, spec_edit=lambda s: setattr(s, 'perlin_octaves', 0)), 'workspace too small'),
    ]
    for kw, what in cases:
        assert _init_seeds(lib, **kw) == -1, what
        msg = _last(lib)
        assert msg.startswith('die_init_batch_seeds') and what in msg, (what, msg)


def test_stride_entry_point_keeps_its_refusals(lib):
    m, a, b, spec = _init_args(lib)
    spec.perlin_octaves = 0
    ws = lib.lib.die_init_batch_workspace_bytes(W, H, R)
    assert lib.lib.die_init_batch(C.byref(m), C.byref(a), C.byref(b), 0.1, 3, 1, C.byref(spec), FAKE, FAKE, ws, None) == -1
    assert _last(lib).startswith('die_init_batch:') and 'wave-mix' in _last(lib)


# ---------------------------------------------------------------------------------------------------- the searchers' fold
def _pgpe_state(lib, replicas=4, P=10):
    return lib.Pgpe(replicas, lib.DIE_PGPE_CLIPUP, P, 1, 0.05, 0.1, 0.1, 0.9, 0.9, 0.999, 1e-8, 0.2, -math.inf, math.inf,
                    FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE, FAKE, FAKE, 64, FAKE)


def _cmaes_state(lib, replicas=4, P=10):
    from die_amd.search import cmaes_constants
    k = cmaes_constants(max(replicas, 2), P)                     # (replicas 1 is a refusal case: any valid constants do)
    return lib.Cmaes(replicas, 0, P, 1, 1.0, k['c_sigma'], k['d_sigma'], k['c_c'], k['c_1'], k['c_mu'], k['mu_eff'], k['chi_d'],
                     (C.c_double * 64)(*(k['weights'] + [0.0] * 64)[:64]), FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
                     FAKE, 64, FAKE)


@pytest.mark.parametrize('kind', ['pgpe', 'cmaes'])
def test_update_episodes_refusals_at_the_c_boundary(lib, kind):
    fn = getattr(lib.lib, f'die_{kind}_update_episodes')
    state = _pgpe_state if kind == 'pgpe' else _cmaes_state

    def call(replicas=4, episodes=3, ef=FAKE, folded=FAKE, T=5, terms=FAKE, generation=0):
        s = state(lib, replicas)
        return fn(C.byref(s), FAKE, terms, T, 2 * replicas * max(episodes, 1), 2, episodes, ef, folded, generation, None)

    for kw, what in ((dict(episodes=0), 'episodes 0: at least 1'), (dict(episodes=-2), 'episodes -2: at least 1'),
                     (dict(replicas=10, episodes=7), '10 candidates x 7 episodes: at most 64 replicas'),
                     (dict(replicas=64, episodes=2), 'at most 64 replicas'),
                     (dict(ef=None), 'null episode_fitness or folded buffer'), (dict(folded=None), 'null episode_fitness or folded buffer'),
                     (dict(terms=None), 'null parameter matrix or terms'), (dict(T=0), 'at least one term'),
                     (dict(generation=64), 'beyond the 64 history rows'), (dict(replicas=1), 'replicas 1')):
        assert call(**kw) == -1, what
        msg = _last(lib)
        assert msg.startswith(f'die_{kind}_update_episodes') and what in msg, (what, msg)


def test_decode_episodes_refusals(lib):
    dec = lambda *a: lib.lib.die_physarum_decode_episodes(*a, None)
    for args, what in (((FAKE, 4, 0, 0, None, FAKE, FAKE), 'episodes 0: at least 1'),
                       ((FAKE, 10, 7, 0, None, FAKE, FAKE), '10 candidates x 7 episodes'),
                       ((FAKE, 0, 2, 0, None, FAKE, FAKE), '0 candidates x 2 episodes'),
                       ((None, 4, 2, 0, None, FAKE, FAKE), 'null rows, table or values'),
                       ((FAKE, 4, 2, 2, None, FAKE, FAKE), 'mode 2'),
                       ((FAKE, 4, 2, 1, None, FAKE, FAKE), 'unit mode needs a parameter space')):
        assert dec(*args) == -1, what
        assert what in _last(lib) and _last(lib).startswith('die_physarum_decode_episodes'), _last(lib)


def test_nca_step_refuses_episodes_that_do_not_divide_the_replicas(lib):
    layers = (lib.NcaLayer * 2)(lib.NcaLayer(3, 3, 3, 0, FAKE, 162), lib.NcaLayer(3, 3, 3, 0, FAKE + 4 * 81, 162))
    m = lib.Medium(W, H, lib.DIE_F32, 2, FAKE, FAKE, FAKE, FAKE + 8, 0, 0, 0, 0, 0, 0, 0, 0, None)
    a = lib.Agents(N, FAKE, FAKE, FAKE, FAKE, None)
    d = lib.Dynamics(0.1, 0.025, 0.8, lib.DIE_BOUNDARY_WRAP, lib.DIE_COST_LINEAR, 0.02, 0.01, 1, 0, 0, 0, 0)
    b = lib.Batch(6, 0, W * H, N, 1, (C.c_int64 * 64)(*([N] * 64)))
    scratch = lib.lib.die_nca_batch_scratch_bytes(W, H, 6, 2)
    for episodes, what in ((4, 'episodes 4'), (-1, 'episodes -1')):
        nca = lib.NcaBatch(2, 0, 1, 1, layers, (C.c_float * 3)(0.01, 0.01, 2.0), episodes, FAKE, scratch)
        rc = lib.lib.die_nca_env_step_batch(C.byref(m), C.byref(a), C.byref(nca), None, C.byref(d), C.byref(b), FAKE, FAKE,
                                            lib.lib.die_batch_workspace_bytes(6), None)
        assert rc == -1 and what in _last(lib) and 'divisor of the 6 replicas' in _last(lib), _last(lib)


# ---------------------------------------------------------------------------------------------------- the classes
def _fake_env(R=6, fixed=50):
    return types.SimpleNamespace(R=R, device=torch.device('cpu'), per_replica=False, Nmax=4, n=[4] * R, W=16, H=16, _fixed=fixed)


def _template():
    from die_amd import NeuralAutomataAgent
    return NeuralAutomataAgent(scale=0.01, deposit=2.0, kernel_sizes=(3, 3))


def test_populations_refuse_episodes_that_do_not_divide_the_replicas(lib):
    from die_amd.batch import BatchedNeuralAutomataAgent, BatchedPhysarumPopulation
    for bad, what in ((4, 'holds 6 replicas, not a multiple of 4'), (0, 'an integer >= 1'), (-1, 'an integer >= 1'),
                      (2.0, 'an integer >= 1'), (True, 'an integer >= 1')):
        with pytest.raises(ValueError, match=what):
            BatchedNeuralAutomataAgent(_fake_env(), _template(), episodes=bad)
        with pytest.raises(ValueError, match=what):
            BatchedPhysarumPopulation(_fake_env(), episodes=bad)
    with pytest.raises(ValueError, match='2 agents for 6 replicas of 2 episodes'):
        BatchedNeuralAutomataAgent.from_agents(_fake_env(), [_template(), _template()], episodes=2)


def test_populations_take_one_row_per_candidate(lib):
    from die_amd.batch import BatchedNeuralAutomataAgent, BatchedPhysarumPopulation
    t = _template()
    P = sum(p.numel() for p in t.model.parameters())
    with pytest.raises(ValueError, match=rf'parameters of shape \(6, {P}\): \(2, {P}\) expected \(2 candidates of 3 episodes each'):
        BatchedNeuralAutomataAgent(_fake_env(), t, torch.zeros((6, P)), episodes=3)
    pop = BatchedNeuralAutomataAgent(_fake_env(), t, torch.ones((2, P)), episodes=3)       # (nothing is launched by building)
    assert (pop.R, pop.candidates, pop.episodes) == (6, 2, 3) and tuple(pop.parameters.shape) == (2, P)
    with pytest.raises(ValueError, match=r'\(2, \d+\) expected'):
        pop.set_parameters(torch.zeros((6, P)))
    assert pop._struct(1).episodes == 3
    one = BatchedNeuralAutomataAgent(_fake_env(), t)                                       # E = 1: today's shapes and struct word
    assert (one.R, one.candidates, one.episodes) == (6, 6, 1) and tuple(one.parameters.shape) == (6, P) and one._struct(1).episodes == 0
    rows = np.tile(np.float32([0.005, 4.0, 0.03, 30.0, 90.0, 0.1]), (6, 1))
    with pytest.raises(ValueError, match=r'values of shape \(6, 6\): \(3, 6\) expected \(3 candidates of 2 episodes each'):
        BatchedPhysarumPopulation(_fake_env(), rows, episodes=2)
    with pytest.raises(ValueError, match=r'parameters of shape \(6, 6\): \(3, 6\) expected'):
        BatchedPhysarumPopulation(_fake_env(), parameters=rows, episodes=2)


def _fake_population(candidates, episodes, P=12, fixed=50):
    from die_amd.batch import BatchedNeuralAutomataAgent
    pop = BatchedNeuralAutomataAgent.__new__(BatchedNeuralAutomataAgent)
    pop.R, pop.P, pop.candidates, pop.episodes = candidates * episodes, P, candidates, episodes
    pop.parameters = torch.zeros((candidates, P))
    pop.env = types.SimpleNamespace(_fixed=fixed)
    return pop


def _searcher(kind, popsize, P=12):
    from die_amd.search import CMAES, PGPE
    return (PGPE(popsize, P, radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1, device='cpu') if kind == 'pgpe'
            else CMAES(popsize, P, stdev_init=0.1, device='cpu'))


@pytest.mark.parametrize('kind', ['pgpe', 'cmaes'])
def test_searchers_bind_to_candidates_and_refuse_other_popsizes(lib, kind):
    s = _searcher(kind, 4)
    assert s.for_population(_fake_population(4, 3), 5) is s and s._episodes == 3
    assert tuple(s._results.shape) == (5, 12, 2) and tuple(s.episode_fitness.shape) == (4, 3)
    with pytest.raises(ValueError, match=r"popsize 4 != the population's 2 candidates \(12 replicas of 6 episodes each\)"):
        s.for_population(_fake_population(2, 6), 5)
    with pytest.raises(ValueError, match="popsize 12 != the population's 4 candidates"):
        _searcher(kind, 12).for_population(_fake_population(4, 3), 5)                      # popsize = R is no longer right
    with pytest.raises(ValueError, match="popsize 4 != the population's 12 replicas"):
        s.for_population(_fake_population(12, 1), 5)
    legacy = _fake_population(4, 1)
    del legacy.candidates, legacy.episodes                                                 # a population without the attributes: pop.R
    assert s.for_population(legacy, 5) is s and s._episodes == 1 and tuple(s.episode_fitness.shape) == (4, 1)
    # tell(): the terms must hold candidates x episodes replicas
    params = torch.zeros((4, 12))
    s._asked, s._asked_iter = params, 0
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='episodes='):
            s.tell(torch.zeros((5, 4), dtype=torch.float64), episodes=bad)
    with pytest.raises(ValueError, match='more than 64 replicas'):
        s.tell(torch.zeros((5, 68), dtype=torch.float64), episodes=17)
    with pytest.raises(ValueError, match=r'terms: a \(T, 12\) or \(T, 12, 2\) float64 tensor.*4 candidates x 3 episodes'):
        s.tell(torch.zeros((5, 4), dtype=torch.float64), episodes=3)
    with pytest.raises(ValueError, match=r'terms: a \(T, 4\)'):
        s.tell(torch.zeros((5, 12), dtype=torch.float64))


def test_reset_with_a_seed_list_refusals(lib):
    from die_amd.batch import BatchedEnv
    env = BatchedEnv.__new__(BatchedEnv)
    env.R, env._fixed, env.seeds = 4, 50, [0, 1, 2, 3]
    with pytest.raises(ValueError, match='3 seeds for 4 replicas'):
        env.reset(seeds=[1, 2, 3])
    with pytest.raises(ValueError, match='5 seeds for 4 replicas'):
        env.reset(seeds=[1, 2, 3, 4, 5])
    with pytest.raises(ValueError, match='not both'):
        env.reset(seed=3, seeds=[1, 2, 3, 4])
    with pytest.raises(ValueError, match='not an integer seed'):
        env.reset(seeds=[1, 2.5, 3, 4])
    env._fixed = None                                                                      # the 'alive' layout
    with pytest.raises(ValueError, match='max_agents'):
        env.reset(seeds=[1, 2, 3, 4])
    assert env.seeds == [0, 1, 2, 3]


# ---------------------------------------------------------------------------------------------------- the formulas
def test_seed_formulas_reduce_to_todays_at_one_episode(lib):
    from die_amd.batch import episode_seeds
    assert episode_seeds(100, 2, 3) == [100, 101, 102, 100, 101, 102] == M.episode_seeds(100, 2, 3)
    assert episode_seeds(100, 2, 3, 1) == [100, 101, 102, 103, 104, 105]
    assert episode_seeds(100, 2, 3, 2) == [100, 101, 102, 106, 107, 108] == M.episode_seeds(100, 2, 3, 2)
    for C_, E, k in ((4, 3, 0), (4, 3, 1), (10, 6, 0), (5, 1, 3)):
        assert episode_seeds(7, C_, E, k) == M.episode_seeds(7, C_, E, k)
    for bad in (dict(candidates=0), dict(episodes=0), dict(candidate_stride=-1), dict(episodes=1.5)):
        with pytest.raises(ValueError):
            episode_seeds(**dict(dict(seed=1, candidates=2, episodes=2), **bad))
    for stride in (0, 1, 3):
        for g in range(4):
            # E = 1: reset(seed=S + g·R, seed_stride=k), replica r the world of S + g·R + r·k
            assert M.generation_seeds(500, g, 10, 1, stride) == M.generation_seeds_today(500, g, 10, stride)
            assert episode_seeds(500 + g * 10, 10, 1, stride) == M.generation_seeds_today(500, g, 10, stride)
    s = _searcher('pgpe', 4).for_population(_fake_population(4, 3), 5, reseed=500, reseed_stride=1)
    assert [s._generation_seeds(g) for g in range(3)] == [M.generation_seeds(500, g, 4, 3, 1) for g in range(3)]
    assert s._generation_seeds(2) == list(range(524, 536))
    s.for_population(_fake_population(4, 3), 5, reseed=500)
    assert s._generation_seeds(1) == [512, 513, 514] * 4


def test_fold_model():
    rng = np.random.RandomState(0)
    terms = rng.randn(7, 12, 2) * 10.0 ** rng.randint(-3, 4, (7, 12, 1))
    f, F = M.fold(terms, 4, 3)
    assert F.shape == (4, 3) and f.shape == (4,)
    for c in range(4):
        for e in range(3):
            s = 0.0
            for t in range(7):
                s += terms[t, 3 * c + e, 0]
            assert F[c, e] == s
        assert f[c] == ((0.0 + F[c, 0]) + F[c, 1] + F[c, 2]) / 3.0
    f1, F1 = M.fold(terms[:, :, 0], 12, 1)                       # E = 1: the fitness is the replica's sum
    assert np.array_equal(f1, F1[:, 0]) and np.array_equal(F1[:, 0], M.replica_sums(terms))
