"""Signal channels (die_signal.hip; NeuralAutomataAgent(signal_channels=K)), CPU side: the numpy model of tests/signal_model.py against
the oracle's diffusion, its fp32 emulation inside the GPU test's bound on that test's whole grid, the host rules (channel order,
parameter count, init_params, save / load, the constructor's ValueErrors, the refusals) and every argument check of the three new C
entry points.  No kernel is launched here: the device pointers below are never dereferenced."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from oracle import cpu_ref
from tests import signal_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'die_signal_step': 13, 'die_signal_step_batch': 14, 'die_nca_wide_env_step_batch_signal': 24}
FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host
ARG, UNSUPPORTED = -1, -3
f32 = np.float32


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


GRID = [(W, H, s, K) for (W, H) in SM.SHAPES for s in SM.SIGMAS for K in SM.CHANNELS]


# ---------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize('W,H', SM.SHAPES + [(24, 40)])
@pytest.mark.parametrize('sigma', SM.SIGMAS)
def test_model_without_emission_is_the_oracles_diffusion(W, H, sigma):
    F, occ, planes = SM.case(W, H, 1)
    got = SM.update(F, np.zeros_like(occ), planes, SM.DEPOSIT, sigma, SM.DECAY)[0]
    want = cpu_ref.diffuse_decay(F[0], float(f32(sigma)), float(f32(SM.DECAY)))
    assert np.allclose(got, want, rtol=1e-12, atol=1e-15)
    # … and an emission is an addition in front of it, at the occupied cells only
    E = SM.emission(occ, planes, SM.DEPOSIT)
    assert occ.any() and not E[:, ~occ].any() and np.array_equal(E[:, occ], float(f32(SM.DEPOSIT)) * planes[:, occ].astype(np.float64))
    both = SM.update(F, occ, planes, SM.DEPOSIT, sigma, SM.DECAY)[0]
    assert np.allclose(both, cpu_ref.diffuse_decay(F[0].astype(np.float64) + E[0], float(f32(sigma)), float(f32(SM.DECAY))), rtol=1e-12, atol=1e-15)


def test_radius_and_taps_are_scipys():
    assert [SM.radius(s) for s in SM.SIGMAS] == [1, 2, 4, 6] and SM.radius(2.1) == 8 and SM.radius(0.1) == 0
    for s in SM.SIGMAS:
        assert np.allclose(SM.taps(s), cpu_ref.gaussian_weights(float(f32(s))), rtol=1e-14)


@pytest.mark.parametrize('W,H,sigma,K', GRID)
def test_fp32_emulation_stays_inside_the_bound(W, H, sigma, K):
    """The kernels' arithmetic in numpy uses a small share of the bound the GPU test allows on the same cases."""
    F, occ, planes = SM.case(W, H, K)
    want = SM.update(F, occ, planes, SM.DEPOSIT, sigma, SM.DECAY)
    got = SM.emulate(F, occ, planes, SM.DEPOSIT, sigma, SM.DECAY)
    share = (np.abs(got.astype(np.float64) - want) / SM.bound(F, occ, planes, SM.DEPOSIT, sigma, SM.DECAY)).max()
    assert got.dtype == f32 and share < 0.25, share
    x = F.astype(np.float64) + SM.emission(occ, planes, SM.DEPOSIT)
    assert (x < 0).any() and (x > 0).any() and (x == 0).any()                    # mixed signs: cancellation is among the cases


def test_model_unoccupied_cells_add_exactly_nothing():
    W, H = 5, 12
    zeros, nobody = np.zeros((2, W, H), dtype=f32), np.zeros((W, H), dtype=bool)
    out = SM.emulate(zeros, nobody, np.ones((2, W, H), dtype=f32), 1.0, 0.5, 0.1)
    assert not out.view(np.uint32).any()                                         # all +0.0, not a single negative zero
    one = nobody.copy()
    one[2, 5] = True
    lit = SM.emulate(zeros, one, -np.ones((2, W, H), dtype=f32), 1.0, 0.5, 0.0)
    assert np.isclose(lit.sum(axis=(1, 2)), -1.0, rtol=1e-6).all() and lit[0, 2, 5] == lit.min()      # mass kept at decay 0, negative allowed


# ---------------------------------------------------------------------------------------------------- host rules
def test_channel_order_and_parameter_count(lib):
    from torch.nn.utils import parameters_to_vector
    from die_amd import NeuralAutomataAgent
    ag = NeuralAutomataAgent(signal_channels=2, memory_channels=3, with_stock_channel=True, kernel_sizes=(3, 3), hidden_channels=16)
    assert ag.obs_channels == ['agents', 'env_food', 'chem1', 'signal_0', 'signal_1', 'memory_0', 'memory_1', 'memory_2', 'agent_food']
    assert [tuple(k.weight.shape) for k in ag.model.conv_layers()] == [(16, 9, 3, 3), (3 + 2 + 3, 16, 3, 3)]
    for K, M, C_ in ((1, 0, 16), (2, 0, 16), (4, 2, 8), (8, 8, 32)):             # 3 + K + M -> C -> 3 + K + M, kernel size 3
        a = NeuralAutomataAgent(signal_channels=K, memory_channels=M, kernel_sizes=(3, 3), hidden_channels=C_)
        assert parameters_to_vector(a.model.parameters()).numel() == 9 * C_ * (3 + K + M) * 2, (K, M)
    single = NeuralAutomataAgent(signal_channels=1, kernel_sizes=(5,), with_agent_channel=False)      # a wide stack, a single layer included
    assert single.model.wide and single.obs_channels == ['env_food', 'chem1', 'signal_0']
    assert tuple(single.model.conv_layers()[0].weight.shape) == (4, 3, 5, 5)
    assert not NeuralAutomataAgent().model.wide
    with pytest.raises(NotImplementedError, match='kernel size 7'):
        NeuralAutomataAgent(signal_channels=1, kernel_sizes=(7,))


def test_init_params_omit_the_defaults_and_save_load_round_trips(lib):
    from die_amd import NeuralAutomataAgent
    names = ('signal_channels', 'signal_deposit', 'signal_sigma', 'signal_decay')
    for kw in ({}, dict(signal_channels=0), dict(signal_channels=None), dict(signal_channels=0, signal_sigma=1.0, signal_decay=0.5, signal_deposit=2.0)):
        ag = NeuralAutomataAgent(**kw)
        assert not set(names) & set(ag.init_params) and 'signal_channels' not in ag.model._init_params, kw
        assert ag.signal_channels == 0 and ag.signals is None and ag.obs_channels == ['agents', 'env_food', 'chem1']
    ag = NeuralAutomataAgent(signal_channels=2, signal_sigma=1.0, signal_decay=0.25, signal_deposit=-0.5, kernel_sizes=(3, 3), hidden_channels=8)
    assert {n: ag.init_params[n] for n in names} == dict(signal_channels=2, signal_deposit=-0.5, signal_sigma=1.0, signal_decay=0.25)
    assert ag.signal_constants == (-0.5, 1.0, 0.25)
    buf = io.BytesIO()
    ag.save(buf)
    buf.seek(0)
    back = NeuralAutomataAgent.load(buf)
    assert back.init_params == ag.init_params and back.signal_channels == 2 and back.signal_constants == ag.signal_constants
    assert back.signals is None                                                  # the field is state, not saved
    assert all((u == v).all() for u, v in zip(ag.model.state_dict().values(), back.model.state_dict().values()))
    plain = NeuralAutomataAgent(signal_channels=1, kernel_sizes=(3, 3), hidden_channels=8)      # the constants at their defaults are saved too
    assert {n: plain.init_params[n] for n in names} == dict(signal_channels=1, signal_deposit=1.0, signal_sigma=0.5, signal_decay=0.1)


@pytest.mark.parametrize('kw, needle', [
    (dict(signal_channels=9), 'signal_channels'), (dict(signal_channels=-1), 'signal_channels'), (dict(signal_channels=1.5), 'signal_channels'),
    (dict(signal_channels=True), 'signal_channels'), (dict(signal_channels='2'), 'signal_channels'),
    (dict(signal_channels=1, signal_sigma=0.12), 'signal_sigma'),                # radius 0
    (dict(signal_channels=1, signal_sigma=2.2), 'signal_sigma'),                 # radius 9
    (dict(signal_channels=1, signal_sigma=0.0), 'signal_sigma'), (dict(signal_channels=1, signal_sigma=float('nan')), 'signal_sigma'),
    (dict(signal_channels=1, signal_decay=-0.01), 'signal_decay'), (dict(signal_channels=1, signal_decay=1.01), 'signal_decay'),
    (dict(signal_channels=1, signal_decay=float('nan')), 'signal_decay'),
    (dict(signal_channels=1, signal_deposit=float('inf')), 'signal_deposit'), (dict(signal_channels=1, signal_deposit=float('nan')), 'signal_deposit'),
    (dict(signal_channels=1, signal_deposit='much'), 'signal_deposit'),
])
def test_constructor_value_errors(lib, kw, needle):
    from die_amd import NeuralAutomataAgent
    with pytest.raises(ValueError, match=needle):
        NeuralAutomataAgent(**kw)


def test_constructor_takes_the_ends_of_every_range(lib):
    from die_amd import NeuralAutomataAgent
    for kw in (dict(signal_sigma=0.125), dict(signal_sigma=2.12), dict(signal_decay=0.0), dict(signal_decay=1.0), dict(signal_deposit=0.0),
               dict(signal_deposit=-3.0)):
        NeuralAutomataAgent(signal_channels=8, memory_channels=8, kernel_sizes=(1, 1), **kw)


def test_population_architecture_and_mixed_refusal(lib):
    from die_amd import NeuralAutomataAgent
    from die_amd.batch import BatchedNeuralAutomataAgent, _architecture

    class FakeEnv:
        R = 2

    mk = lambda **kw: NeuralAutomataAgent(kernel_sizes=(3, 3), hidden_channels=8, **kw)       # noqa: E731
    a2, a1, a0, a2s = mk(signal_channels=2), mk(signal_channels=1, memory_channels=1), mk(), mk(signal_channels=2, signal_sigma=1.0)
    assert _architecture(a2)['signal_channels'] == 2 and _architecture(a0)['signal_channels'] == 0 and _architecture(a0)['signal_constants'] is None
    for mixed in ([a2, a1], [a2, a0], [a0, a2], [a2, a2s]):                      # (a2 and a1 observe 5 channels both)
        with pytest.raises(ValueError, match='architecture'):
            BatchedNeuralAutomataAgent.from_agents(FakeEnv(), mixed)
    assert BatchedNeuralAutomataAgent.pack([a2, a2]).shape == (2, 8 * 5 * 9 + 5 * 8 * 9)


def test_refusals_come_before_anything_is_touched(lib):
    from die_amd import NeuralAutomataAgent
    from die_amd.batch import BatchedNeuralAutomataAgent

    class NoMedium:
        world = None

        def __getattr__(self, name):
            raise AssertionError(f'the medium was touched ({name}) before the refusal')

    class Decomposed(NoMedium):
        world = (128, 128, 0, 0)

    for M in (0, 2):
        ag = NeuralAutomataAgent(kernel_sizes=(3, 3), signal_channels=2, memory_channels=M, p_agent_dropout=0.25, dropout_seed=3)
        with pytest.raises(NotImplementedError, match='decomposed'):
            ag.sense(Decomposed(), agents=object())
        with pytest.raises(NotImplementedError, match='decomposed'):
            ag.forward((object(), Decomposed()))
        for name, call in (('differentiable_sense', lambda: ag.differentiable_sense(NoMedium())),
                           ('differentiable_action', lambda: ag.differentiable_action((None, NoMedium()))),
                           ('forward_device', lambda: ag.model.forward_device(None)),
                           ('recurrent_action', lambda: ag.recurrent_action((None, NoMedium())))):
            with pytest.raises(NotImplementedError, match=name + '.*signal'):
                call()
        assert ag.dropout_step == 0 and ag.memory is None and ag.signals is None
        pop = BatchedNeuralAutomataAgent.__new__(BatchedNeuralAutomataAgent)
        pop.template, pop.dropout_seed, pop.dropout_step, pop._wide, pop._stock_channel, pop.env = ag, 5, 0, True, False, None
        pop._memory_channels, pop._signal_channels = M, 2
        for call in (pop.differentiable_sense, pop.differentiable_action, pop.forward_device, pop.recurrent_action):
            with pytest.raises(NotImplementedError, match='signal'):
                call()
        assert pop.dropout_step == 0


def test_examples_signal_channels_flags(lib):
    import argparse
    import importlib
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    try:
        population_eval = importlib.import_module('population_eval')
    finally:
        sys.path.pop(0)
    p = argparse.ArgumentParser()
    population_eval.add_wide_arguments(p)
    assert population_eval.wide_keywords(p.parse_args([])) == {}
    assert population_eval.wide_keywords(p.parse_args(['--signal-sigma', '1.0'])) == {}          # the constants only beside K > 0
    kw = population_eval.wide_keywords(p.parse_args(['--signal-channels', '2', '--hidden-channels', '16']))
    assert kw == dict(signal_channels=2, hidden_channels=16)
    kw = population_eval.wide_keywords(p.parse_args(['--signal-channels', '1', '--signal-sigma', '1.0', '--signal-decay', '0.2', '--signal-deposit', '0.5']))
    assert kw == dict(signal_channels=1, signal_sigma=1.0, signal_decay=0.2, signal_deposit=0.5)
    ag = population_eval.make_template(0., kw)
    assert ag.signal_channels == 1 and ag.obs_channels[-1] == 'signal_0' and ag.signal_constants == (0.5, 1.0, 0.2)
    text = open(os.path.join(ROOT, 'examples', 'learning_agents.py')).read()
    assert '--signal-channels K' in text and 'add_wide_arguments(p)' in text


# ---------------------------------------------------------------------------------------------------- the symbols
def test_new_symbols_exported_with_the_documented_argument_counts(lib):
    so = C.CDLL(lib.LIB_PATH)
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    header = open(os.path.join(ROOT, 'include', 'die_hip.h')).read()
    assert '#define DIE_ABI_VERSION 24' in header and '#define DIE_SIGNAL_MAX_CHANNELS 8' in header and lib.SIGNAL_MAX_CHANNELS == 8
    for name, n_args in NEW.items():
        assert hasattr(so, name) and name in lib.EXPORTS, name
        assert len(lib._SIGNATURES[name][1]) == n_args and len(getattr(lib.lib, name).argtypes) == n_args, name
        proto = header[header.index(f'int {name}('):]
        proto = proto[:proto.index(';')]
        assert proto.count(',') + 1 == n_args, (name, proto)
    # the fused step is the memory step's arguments plus K, both field buffers and the three constants
    assert len(lib._SIGNATURES['die_nca_wide_env_step_batch_memory'][1]) + 6 == NEW['die_nca_wide_env_step_batch_signal']
    spec_text = open(os.path.join(ROOT, 'die_amd', 'build.py')).read()
    assert "'die_signal.hip'" in spec_text


# ---------------------------------------------------------------------------------------------------- the argument checks
W, H, N = 20, 68, 300
MB = 1 << 20
STANDING, EMISSION, FIELD_IN, FIELD_OUT = FAKE, FAKE + 4 * MB, FAKE + 8 * MB, FAKE + 12 * MB      # megabytes apart: nothing overlaps


def _medium(L, W=W, H=H, gW=0):
    return L.Medium(W, H, L.DIE_F32, 5, FAKE, FAKE, FAKE, FAKE + 8, gW, gW, 0, 0, 0, 0, 0, 0, None)


def _batch(L, replicas=3, plane_stride=None, agent_stride=N, n=None):
    counts = [300, 17, 0] + [0] * 61 if n is None else list(n) + [0] * (64 - len(n))
    return L.Batch(replicas, 0, W * H if plane_stride is None else plane_stride, agent_stride, 1, (C.c_int64 * 64)(*counts))


def _signal(L, *, batch=False, null=None, K=3, epoch=3, plane_stride=W * H, field_stride=W * H, replica_stride=8 * W * H, standing=STANDING,
            emission=EMISSION, field_in=FIELD_IN, field_out=FIELD_OUT, deposit=1.0, sigma=0.5, decay=0.1, Wm=W, Hm=H, gW=0, **bkw):
    args = dict(m=C.byref(_medium(L, Wm, Hm, gW)), standing=standing, emission=emission, field_in=field_in, field_out=field_out,
                b=C.byref(_batch(L, **bkw)))
    if null:
        args[null] = None
    if batch:
        return L.lib.die_signal_step_batch(args['m'], args['b'], args['standing'], epoch, K, args['emission'], plane_stride, replica_stride,
                                           args['field_in'], args['field_out'], deposit, sigma, decay, None)
    return L.lib.die_signal_step(args['m'], args['standing'], epoch, K, args['emission'], plane_stride, args['field_in'], args['field_out'],
                                 field_stride, deposit, sigma, decay, None)


CELLS = W * H
BOTH = [
    ('null medium', dict(null='m'), ARG, b'null argument'),
    ('null standing plane', dict(null='standing'), ARG, b'null argument'),
    ('null emission planes', dict(null='emission'), ARG, b'null argument'),
    ('null field_in', dict(null='field_in'), ARG, b'null argument'),
    ('null field_out', dict(null='field_out'), ARG, b'null argument'),
    ('no column', dict(Hm=0), ARG, b'bad size'),
    ('no row', dict(Wm=0), ARG, b'bad size'),
    ('decomposed medium', dict(gW=128), UNSUPPORTED, b'decomposed medium'),
    ('no channel', dict(K=0), ARG, b'0 signal channels outside 1..8'),
    ('nine channels', dict(K=9), ARG, b'9 signal channels outside 1..8'),
    ('epoch 0', dict(epoch=0), ARG, b'epoch 0 outside 1..31'),
    ('epoch 32', dict(epoch=32), ARG, b'epoch 32 outside 1..31'),
    ('sigma 0', dict(sigma=0.0), ARG, b'sigma'),
    ('sigma nan', dict(sigma=float('nan')), ARG, b'sigma'),
    ('sigma of radius 0', dict(sigma=0.12), ARG, b'radius 0 outside 1..8'),
    ('sigma of radius 9', dict(sigma=2.2), ARG, b'radius 9 outside 1..8'),
    ('decay below 0', dict(decay=-0.5), ARG, b'decay'),
    ('decay above 1', dict(decay=1.5), ARG, b'decay'),
    ('decay nan', dict(decay=float('nan')), ARG, b'decay'),
    ('deposit inf', dict(deposit=float('inf')), ARG, b'deposit'),
    ('deposit nan', dict(deposit=float('nan')), ARG, b'deposit'),
    ('plane_stride below a plane', dict(plane_stride=CELLS - 1), ARG, b'plane_stride'),
    ('field_out is field_in', dict(field_out=FIELD_IN), ARG, b'field_out overlaps field_in'),
    ('field_out ends inside field_in', dict(field_out=FIELD_IN - 4 * (2 * CELLS + CELLS) + 4), ARG, b'field_out overlaps field_in'),
    ('field_out starts in the last emission plane', dict(field_out=EMISSION + 4 * (2 * CELLS + CELLS) - 4), ARG, b'overlaps the emission'),
    ('field_out starts in the standing plane', dict(field_out=STANDING + 8 * CELLS - 8), ARG, b'overlaps the standing'),
]
ALONE = BOTH + [
    ('field_stride below a plane', dict(field_stride=CELLS - 1), ARG, b'field_stride'),
    ('field_out one plane into field_in', dict(field_out=FIELD_IN + 4 * CELLS), ARG, b'field_out overlaps field_in'),
]
BATCHED = BOTH + [
    ('null batch', dict(null='b'), ARG, b'null argument'),
    ('no replica', dict(replicas=0), ARG, b'replicas'),
    ('65 replicas', dict(replicas=65), ARG, b'replicas'),
    ('agent_stride 0', dict(agent_stride=0), ARG, b'agent_stride'),
    ('a replica above the stride', dict(n=[301, 1, 1]), ARG, b'replica 0 has 301 agents'),
    ('replica_stride below a replica\'s planes', dict(replica_stride=3 * CELLS - 1), ARG, b'replica_stride'),
    ('field_out in the last replica\'s standing plane', dict(field_out=STANDING + 8 * (2 * CELLS) + 8 * CELLS - 8), ARG, b'overlaps the standing'),
]

def _ids(v):
    return v.replace(' ', '_') if isinstance(v, str) else ''


@pytest.mark.parametrize('case, kw, status, needle', ALONE, ids=_ids)
def test_signal_step_refusals(lib, case, kw, status, needle):
    assert _signal(lib, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and b'die_signal_step:' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


@pytest.mark.parametrize('case, kw, status, needle', BATCHED, ids=_ids)
def test_signal_step_batch_refusals(lib, case, kw, status, needle):
    assert _signal(lib, batch=True, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and b'die_signal_step_batch:' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


def test_signal_step_batch_refuses_a_batch_stride_below_a_plane(lib):
    b = _batch(lib, plane_stride=CELLS - 1)
    rc = lib.lib.die_signal_step_batch(C.byref(_medium(lib)), C.byref(b), STANDING, 3, 3, EMISSION, CELLS, 8 * CELLS, FIELD_IN, FIELD_OUT, 1.0, 0.5,
                                       0.1, None)
    assert rc == ARG and b'plane_stride' in lib.lib.die_last_error()


def _step(lib, *, null=None, replicas=4, K=2, M_=2, with_stock=0, cin0=None, cout=None, with_agents=1, hidden=8, sense_epoch=1, epoch=2, n=10,
          gW=0, H=96, sigma=0.5, decay=0.1, deposit=1.0, memory='given', field_out=None):
    """The fused step: layer 0 reads `cin0` planes (default: what K, M_ and with_stock ask for), the last layer gives `cout`."""
    L, W = lib, 96
    m = L.Medium(W, H, L.DIE_F32, epoch, FAKE, FAKE, FAKE, FAKE + 8, gW, gW, 0, 0, 0, 0, 0, 0, None)
    a = L.Agents(10, FAKE, FAKE, FAKE, FAKE, None)
    good_k, good_m = min(max(K, 1), 8), min(max(M_, 0), 8)
    cin0 = 2 + with_agents + good_k + good_m + (with_stock == 1) if cin0 is None else cin0
    cout = 3 + good_k + good_m if cout is None else cout
    shapes = ((3, cin0, hidden), (3, hidden, cout))
    arr = (L.NcaLayer * 2)(*[L.NcaLayer(k, ci, co, 1, FAKE, co * ci * k * k) for k, ci, co in shapes])
    need = L.lib.die_nca_wide_batch_scratch_bytes(W, H, replicas, 2, min(max(hidden, cout), 32)) if 1 <= replicas <= 64 else 1 << 30
    nca = L.NcaBatch(2, 0, with_agents, sense_epoch, arr, (C.c_float * 3)(0.01, 0.01, 2.0), 0, FAKE, need)
    d = L.Dynamics(0.1, 0.025, 0.8, 0, 0, 0.02, 0.01, 1, 0, 0, 0, 0)
    b = L.Batch(replicas, 0, W * H, 10, 1, (C.c_int64 * 64)(*([n] * 64)))
    G = 1 << 26                                                                  # 64 MiB apart: past the scratch at FAKE, nothing overlaps
    args = dict(m=C.byref(m), a=C.byref(a), nca=C.byref(nca), d=C.byref(d), b=C.byref(b), results=FAKE, ws=FAKE, standing=FAKE + G,
                memory=FAKE + 2 * G, planes=FAKE + 3 * G, field_in=FAKE + 4 * G, field_out=FAKE + 5 * G)
    if field_out is not None:
        args['field_out'] = args[field_out[0]] + field_out[1]
    if memory == 'none':
        args['memory'] = args['planes'] = None
    elif memory == 'half':
        args['planes'] = None
    if null:
        args[null] = None
    return L.lib.die_nca_wide_env_step_batch_signal(args['m'], args['a'], args['nca'], None, args['d'], args['b'], args['results'], args['ws'],
                                                    64 * L.lib.die_batch_workspace_bytes(1), None, None, None, args['standing'], M_,
                                                    args['memory'], args['planes'], with_stock, K, args['field_in'], args['field_out'], deposit,
                                                    sigma, decay, None)


STEP_CASES = [
    ('null medium', dict(null='m'), ARG, b'null argument'),
    ('null agents', dict(null='a'), ARG, b'null argument'),
    ('null stack', dict(null='nca'), ARG, b'null argument'),
    ('null dynamics', dict(null='d'), ARG, b'null argument'),
    ('null batch', dict(null='b'), ARG, b'null argument'),
    ('null results', dict(null='results'), ARG, b'null argument'),
    ('null workspace', dict(null='ws'), ARG, b'null argument'),
    ('null standing planes', dict(null='standing'), ARG, b'null standing planes'),
    ('null field_in', dict(null='field_in'), ARG, b'signal field'),
    ('null field_out', dict(null='field_out'), ARG, b'signal field'),
    ('memory channels without the memory', dict(memory='none'), ARG, b'2 memory channels need both'),
    ('memory channels without the memory planes', dict(memory='half'), ARG, b'2 memory channels need both'),
    ('no memory channel but a memory', dict(M_=0), ARG, b'0 memory channels need both'),
    ('nine memory channels', dict(M_=9), ARG, b'9 memory channels outside 0..8'),
    ('a negative memory count', dict(M_=-1), ARG, b'-1 memory channels outside 0..8'),
    ('with_stock 2', dict(with_stock=2), ARG, b'with_stock is 0 or 1'),
    ('no signal channel', dict(K=0), ARG, b'0 signal channels outside 1..8'),
    ('nine signal channels', dict(K=9), ARG, b'9 signal channels outside 1..8'),
    ('no replica', dict(replicas=0), ARG, b'replicas'),
    ('decomposed medium', dict(gW=128), ARG, b'periodic single-tile'),
    ('H no multiple of 4', dict(H=98), UNSUPPORTED, b'H % 4 == 0'),
    ("layer 0 reads the memory step's 5 planes", dict(cin0=5), ARG, b'input has 7'),
    ('layer 0 without memory reads 5 planes', dict(M_=0, memory='none', cin0=4), ARG, b'input has 5'),
    ('layer 0 misses the stock plane', dict(with_stock=1, cin0=7), ARG, b'input has 8'),
    ('the last layer gives the memory step\'s 5 planes', dict(cout=5), ARG, b'the last layer gives 5 planes (dx, dy, deposit, 2 signal and 2 memory planes: 7)'),
    ('the last layer without memory gives 3 planes', dict(M_=0, memory='none', cout=3), ARG, b'2 signal and 0 memory planes: 5'),
    ('claims do not follow the sensing', dict(sense_epoch=1, epoch=3), ARG, b'cannot follow sensing'),
    ('a replica without agents', dict(n=0), ARG, b'has 0 agents'),
    ('sigma of radius 0', dict(sigma=0.1), ARG, b'radius 0 outside 1..8'),
    ('sigma of radius 9', dict(sigma=2.2), ARG, b'radius 9 outside 1..8'),
    ('decay above 1', dict(decay=1.25), ARG, b'decay'),
    ('deposit nan', dict(deposit=float('nan')), ARG, b'deposit'),
    ('field_out is field_in', dict(field_out=('field_in', 0)), ARG, b'field_out overlaps field_in'),
    ('field_out in the scratch', dict(field_out=('ws', 4096)), ARG, b'field_out overlaps the emission planes'),
    ('field_out in the standing planes', dict(field_out=('standing', 64)), ARG, b'field_out overlaps the standing'),
    ('field_out in the memory planes', dict(field_out=('planes', 64)), ARG, b'field_out overlaps the memory planes'),
]


@pytest.mark.parametrize('case, kw, status, needle', STEP_CASES, ids=_ids)
def test_signal_env_step_refusals(lib, case, kw, status, needle):
    assert _step(lib, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and b'die_nca_wide_env_step_batch_signal:' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


def test_signal_env_step_takes_no_memory_with_null_pointers_up_to_its_own_checks(lib):
    """M = 0 with null memory pointers passes the entry's own checks: what refuses next is a rule of the field (here the radius)."""
    assert _step(lib, M_=0, memory='none', sigma=2.2) == ARG and b'radius 9' in lib.lib.die_last_error()
