"""The one step path of batched replicas (`BatchedEnv.step`): which library entry points a step calls, in which order, for each
of the three agent kinds — and that a step the library refuses leaves the batch as it was, for the two Physarum kinds as for the
NCA population.  The results of those calls are the business of the bit-for-bit files (tests/test_gpu_parity.py -k batched,
test_gpu_nca_batch.py, test_gpu_physarum_pop.py, test_gpu_flow_batch.py, test_gpu_dropout.py, test_gpu_dynamics_rows.py …)."""
import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent, BatchedPhysarumAgent, BatchedPhysarumPopulation
from die_amd.search import PGPE

pytestmark = pytest.mark.gpu

W, H, R = 32, 32, 4
STEP = {'agent': 'die_forward_env_step_batch', 'pop': 'die_physarum_env_step_batch', 'nca': 'die_nca_env_step_batch'}
RECORDED = tuple(STEP.values()) + tuple(v + '_rows' for v in STEP.values()) + (
    'die_nca_env_step_batch_dropout', 'die_food_flow_batch', 'die_food_flow_batch_masked', 'die_physarum_decode_batch',
    'die_physarum_decode_episodes', 'die_init_batch', 'die_init_batch_seeds')


@pytest.fixture
def calls(monkeypatch):
    """The names of the RECORDED library calls made, in order: each attribute of the CDLL is wrapped to append its name and
    forward the call."""
    log = []
    for name in RECORDED:
        def recorder(*args, _fn=getattr(_lib.lib, name), _name=name):
            log.append(_name)
            return _fn(*args)
        monkeypatch.setattr(_lib.lib, name, recorder)
    return log


def _dynamics(listed: bool, flow: str):
    """One Dynamics, or R of them with two diffuse_sigma; the WaveSequence operator on no replica, on all, or on some."""
    op = None if flow == 'none' else die.WaveSequence((W, H), dt=0.01).get_flow_operator(scale=0.5, decay=0.5)
    kw = lambda r: dict(init_agent_ratio=0.15, **(dict(op_food_flow=op) if flow == 'all' or (flow == 'some' and r in (1, 2)) else {}))
    if not listed:
        return die.Dynamics(diffuse_sigma=0.8, **kw(0))
    return [die.Dynamics(diffuse_sigma=(0.8, 0.5)[r % 2], **kw(r)) for r in range(R)]


def _template(p=0.0):
    torch.manual_seed(5)
    return die.NeuralAutomataAgent(scale=0.01, deposit=2.0, kernel_sizes=(3,), boundary='circular', p_agent_dropout=p)


def _agent(kind: str, benv: BatchedEnv, dropout: bool = False, episodes: int = 1):
    if kind == 'agent':
        return BatchedPhysarumAgent(benv, seed=7)
    if kind == 'pop':
        return BatchedPhysarumPopulation(benv, seed=7, episodes=episodes)
    if dropout:
        return BatchedNeuralAutomataAgent(benv, _template(0.5), episodes=episodes, dropout_seed=3)
    return BatchedNeuralAutomataAgent(benv, _template(), episodes=episodes)


def _expected(kind: str, listed: bool, flow: str, dropout: bool = False, decode=None):
    """The calls of one step by the rules of the batched layer: a decode launch only after a write to `parameters`; the step's
    `_rows` entry point under per-replica Dynamics, else the dropout one when a mask is active, else the plain one; then the
    flow, masked whenever the Dynamics came as a list, and no call for the identity operator."""
    step = STEP[kind] + ('_rows' if listed else '_dropout' if dropout else '')
    flows = [] if flow == 'none' else ['die_food_flow_batch_masked' if listed else 'die_food_flow_batch']
    return ([decode] if decode else []) + [step] + flows


CASES = [(kind, listed, flow, dropout) for kind in STEP for listed in (False, True)
         for flow in (('none', 'all', 'some') if listed else ('none', 'all')) for dropout in ((False, True) if kind == 'nca' else (False,))]


@pytest.mark.parametrize('kind,listed,flow,dropout', CASES)
def test_the_calls_a_step_makes(calls, kind, listed, flow, dropout):
    benv = BatchedEnv((W, H), _dynamics(listed, flow), replicas=R, seed=3)
    assert not benv.per_replica and (benv._rows is not None) == listed
    agent = _agent(kind, benv, dropout)
    decoded = None
    if kind == 'pop':                                            # one step right after an in-place write, one without
        agent.parameters.add_(0.0)
        decoded = 'die_physarum_decode_batch'
    for decode in (decoded, None):
        del calls[:]
        benv.step(agent)
        assert calls == _expected(kind, listed, flow, dropout, decode)
    torch.cuda.synchronize()
    assert (benv._steps, agent._calls, benv.epoch) == (2, 2, 3)
    assert getattr(agent, 'dropout_step', 0) == (2 if dropout else 0)


@pytest.mark.parametrize('kind', ['nca', 'pop'])
def test_the_calls_a_step_makes_with_episodes(calls, kind):
    benv = BatchedEnv((W, H), _dynamics(False, 'none'), replicas=R, seed=3)
    agent = _agent(kind, benv, episodes=2)
    assert (agent.candidates, agent.episodes) == (2, 2)
    agent.parameters.add_(0.0)
    for decode in ('die_physarum_decode_episodes' if kind == 'pop' else None, None):
        del calls[:]
        benv.step(agent)
        assert calls == _expected(kind, False, 'none', decode=decode)
    torch.cuda.synchronize()


@pytest.mark.parametrize('episodes', [1, 2])
def test_a_generation_of_one_episode_reseeds_by_seed_and_stride(calls, episodes):
    """E = 1 must stay on `reset(seed=, seed_stride=)` (die_init_batch); only E > 1 hands the worlds over as a list."""
    benv = BatchedEnv((W, H), _dynamics(False, 'none'), replicas=R, seed=3, max_agents=None)
    pop = _agent('nca', benv, episodes=episodes)
    searcher = PGPE(pop.candidates, center_init=pop.parameters[0], radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1,
                    device=benv.device).for_population(pop, 2, reseed=77, reseed_stride=1)
    del calls[:]
    searcher.step()
    torch.cuda.synchronize()
    assert calls == ['die_init_batch' if episodes == 1 else 'die_init_batch_seeds'] + [STEP['nca']] * 2
    assert searcher.iter == 1 and benv._steps == 2


def _snapshot(benv, agent):
    torch.cuda.synchronize()
    return ((benv.epoch, benv._steps, agent._calls, getattr(agent, 'dropout_step', None)),
            [tuple(x.copy() for x in benv.replica_numpy(r)) for r in range(benv.R)])


@pytest.mark.parametrize('kind', list(STEP))
def test_a_refused_step_changes_nothing(calls, kind):
    """32x30: H is no multiple of 4, which the constructor accepts and every batched step entry point refuses (UNSUPPORTED,
    'only for periodic planes with H % 4 == 0 …') before it launches anything."""
    benv = BatchedEnv((W, 30), _dynamics(False, 'none'), replicas=R, seed=3, per_replica=False)
    agent = _agent(kind, benv, dropout=kind == 'nca')
    before = _snapshot(benv, agent)
    del calls[:]
    with pytest.raises(NotImplementedError, match='H % 4 == 0'):
        benv.step(agent)
    assert calls == [STEP[kind] + ('_dropout' if kind == 'nca' else '')]           # the library was asked, and refused
    after = _snapshot(benv, agent)
    assert after[0] == before[0] == (1, 0, 0, 0 if kind == 'nca' else None)
    assert all(np.array_equal(x, y) for p, q in zip(before[1], after[1]) for x, y in zip(p, q))
