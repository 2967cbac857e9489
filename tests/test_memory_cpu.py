"""Memory channels (NeuralAutomataAgent(memory_channels=M), die_memory.hip), CPU side: known answers of the numpy model
(tests/memory_model.py), the constructor and the Python surface, the new symbols under the unchanged ABI version, and every
argument refusal of the four stand-alone entry points and of the fused step on the host (fake pointers: a launch would have
failed).  No kernel is launched here."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from tests import memory_model as M
from tests import stock_plane_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'die_memory_planes': 10, 'die_memory_planes_batch': 9, 'die_gather_memory': 8, 'die_gather_memory_batch': 10,
       'die_nca_wide_env_step_batch_memory': 18}
FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host
ARG, UNSUPPORTED = -1, -3
TOP = 2 ** 32 - 1


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------- the model
def _words(cells, n):
    return np.array([min(TOP, (c << 32) // (n - 1)) for c in cells], dtype=np.uint32)


def test_model_a_shared_cell_reads_the_highest_slot_and_both_get_the_same_memory():
    W, H = 7, 9
    x, y = _words([3, 3, 0], W), _words([4, 4, 0], H)
    mem = np.array([[1.5, 2.5, 3.5], [-1.0, -2.0, -3.0]], dtype=np.float32)
    P = M.expand(W, H, x, y, np.ones(3), mem)
    assert P.shape == (2, W, H) and P.dtype == np.float32
    assert P[0, 3, 4] == 2.5 and P[1, 3, 4] == -2.0 and P[0, 0, 0] == 3.5 and np.count_nonzero(P) == 4
    planes = np.arange(2 * W * H, dtype=np.float32).reshape(2, W, H)
    out = M.gather(W, H, x, y, np.ones(3), planes)
    assert np.array_equal(out[:, 0], out[:, 1]) and out[0, 0] == planes[0, 3, 4] and out[1, 2] == planes[1, 0, 0]


def test_model_a_dead_slot_on_a_crowded_cell_is_skipped_and_zeroed():
    W, H = 7, 9
    x, y = _words([3, 3, 3], W), _words([4, 4, 4], H)
    mem = np.array([[1.5, 2.5, 3.5]], dtype=np.float32)
    assert M.expand(W, H, x, y, [1, 1, 0], mem)[0, 3, 4] == 2.5                # the dead slot above them does not win
    assert M.expand(W, H, x, y, [1, 0, 1], mem)[0, 3, 4] == 3.5
    assert not M.expand(W, H, x, y, [0, 0, 0], mem).any()
    planes = np.full((1, W, H), 7.0, dtype=np.float32)
    out = M.gather(W, H, x, y, [1, 0, 1], planes)
    assert out.tolist() == [[7.0, 0.0, 7.0]] and M.bits(out)[0, 1] == 0          # +0.0, not -0.0


def test_model_shuffled_storage_with_a_slot_array():
    W, H, N = 5, 6, 4
    x, y = _words([0, 1, 2, 3], W), _words([0, 1, 2, 3], H)                       # slot order
    perm = np.array([2, 0, 3, 1])                                                # storage entry j holds slot perm[j]
    assert np.array_equal(M.to_slot_order(x[perm], perm), x)
    assert M.to_slot_order(x, None) is x
    mem = np.array([[10., 11., 12., 13.]], dtype=np.float32)                     # by slot id, whatever the storage order
    P = M.expand(W, H, M.to_slot_order(x[perm], perm), M.to_slot_order(y[perm], perm), np.ones(N), mem)
    assert [P[0, i, i] for i in range(4)] == [10., 11., 12., 13.]


def test_model_negative_zero_and_denormal_payloads_keep_their_bits():
    W, H = 4, 4
    x, y = _words([1, 2, 3], W), _words([1, 2, 3], H)
    mem = np.array([[-0.0, 1e-41, -0.75]], dtype=np.float32)
    P = M.expand(W, H, x, y, np.ones(3), mem)
    assert M.bits(P)[0, 1, 1] == 0x80000000 and M.bits(P)[0, 2, 2] == M.bits(mem)[0, 1] != 0 and P[0, 3, 3] == np.float32(-0.75)
    assert M.bits(P)[0, 0, 0] == 0                                               # an empty cell: +0.0
    back = M.gather(W, H, x, y, np.ones(3), P)
    assert np.array_equal(M.bits(back), M.bits(mem))
    occ, win = S.stock_winners(W, H, x, y, np.ones(3))                           # the winners ARE the stock channel's
    assert occ.sum() == 3 and win[2, 2] == 1


# ---------------------------------------------------------------------------------------------------- the constructor
def test_constructor_validation_and_init_params(lib):
    from die_amd import NeuralAutomataAgent
    for absent in (0, None):
        ag = NeuralAutomataAgent(memory_channels=absent)
        assert ag.memory_channels == 0 and 'memory_channels' not in ag.init_params and ag.memory is None
        assert ag.obs_channels == ['agents', 'env_food', 'chem1'] and not ag.model.wide
        assert 'memory_channels' not in ag.model._init_params
    assert 'memory_channels' not in NeuralAutomataAgent().init_params
    for bad in (9, -1, True, 2.5, 'two'):
        with pytest.raises(ValueError, match='memory_channels'):
            NeuralAutomataAgent(memory_channels=bad)
    assert NeuralAutomataAgent(memory_channels=2.0).memory_channels == 2          # (an integral float, as hidden_channels takes one)
    ag = NeuralAutomataAgent(memory_channels=8, with_stock_channel=True)
    assert ag.init_params['memory_channels'] == 8 and ag.model.wide and ag.memory is None
    with pytest.raises(NotImplementedError, match='kernel size 7'):
        NeuralAutomataAgent(memory_channels=1, kernel_sizes=(7,))
    with pytest.raises(ValueError, match='at least two layers'):
        NeuralAutomataAgent(memory_channels=1, kernel_sizes=(3,), hidden_channels=8)


def test_observation_order_and_weight_shapes(lib):
    from die_amd import NeuralAutomataAgent
    mem = ['memory_0', 'memory_1', 'memory_2']
    for with_agents in (True, False):
        for with_stock in (True, False):
            ag = NeuralAutomataAgent(memory_channels=3, with_agent_channel=with_agents, with_stock_channel=with_stock, kernel_sizes=(3, 1, 5))
            want = (['agents'] if with_agents else []) + ['env_food', 'chem1'] + mem + (['agent_food'] if with_stock else [])
            assert ag.obs_channels == want
            n = len(want)
            shapes = [tuple(k.weight.shape) for k in ag.model.conv_layers()]
            assert shapes == [(n, n, 3, 3), (n, n, 1, 1), (6, n, 5, 5)]           # hidden_channels None: as wide as the observation
    ag = NeuralAutomataAgent(memory_channels=2, kernel_sizes=(3, 3), hidden_channels=16, hidden_activation='relu')
    assert [tuple(k.weight.shape) for k in ag.model.conv_layers()] == [(16, 5, 3, 3), (5, 16, 3, 3)]
    single = NeuralAutomataAgent(memory_channels=4, kernel_sizes=(5,), with_agent_channel=False)       # obs -> 3 + M
    assert [tuple(k.weight.shape) for k in single.model.conv_layers()] == [(7, 6, 5, 5)] and single.model.wide


def test_save_load_restores_the_count_and_not_the_memory(lib):
    import torch
    from die_amd import NeuralAutomataAgent
    ag = NeuralAutomataAgent(scale=0.02, memory_channels=3, with_stock_channel=True, kernel_sizes=(3, 3), hidden_channels=8)
    ag.model.init_weights()
    ag.memory = torch.ones((3, 10))
    buf = io.BytesIO()
    ag.save(buf)
    buf.seek(0)
    saved = torch.load(buf)
    assert saved['params_dict']['memory_channels'] == 3 and not any('memory' in k for k in saved['model_state'])
    buf.seek(0)
    back = NeuralAutomataAgent.load(buf)
    assert back.memory_channels == 3 and back.memory is None and back.obs_channels == ag.obs_channels
    assert back.init_params == ag.init_params
    for p, q in zip(back.model.parameters(), ag.model.parameters()):
        assert torch.equal(p, q)
    plain = NeuralAutomataAgent(kernel_sizes=(3, 3))
    buf = io.BytesIO()
    plain.save(buf)
    buf.seek(0)
    assert 'memory_channels' not in torch.load(buf)['params_dict']
    ag.reset_memory()
    assert not ag.memory.any()


def test_population_architecture_p_and_mixed_refusal(lib):
    from torch.nn.utils import parameters_to_vector
    from die_amd import NeuralAutomataAgent
    from die_amd.batch import BatchedNeuralAutomataAgent, _architecture

    class FakeEnv:
        R = 2

    a2, a3, a0 = (NeuralAutomataAgent(memory_channels=m, kernel_sizes=(3, 3), hidden_channels=8) for m in (2, 3, 0))
    assert _architecture(a2)['memory_channels'] == 2 and _architecture(a0)['memory_channels'] == 0
    for mixed in ([a2, a3], [a2, a0], [a0, a2]):
        with pytest.raises(ValueError, match='architecture'):
            BatchedNeuralAutomataAgent.from_agents(FakeEnv(), mixed)
    # (5 observed channels both: one memory channel traded for the stock channel is still another architecture)
    b = NeuralAutomataAgent(memory_channels=1, with_stock_channel=True, kernel_sizes=(3, 3), hidden_channels=8)
    with pytest.raises(ValueError, match='architecture'):
        BatchedNeuralAutomataAgent.from_agents(FakeEnv(), [a2, b])
    # P of a population is the row length: 8 * 5 * 9 + 5 * 8 * 9
    assert BatchedNeuralAutomataAgent.pack([a2, a2]).shape == (2, 8 * 5 * 9 + 5 * 8 * 9)
    assert parameters_to_vector(a2.model.parameters()).numel() == 720


def test_refusals_come_before_anything_is_touched(lib):
    from die_amd import Dynamics, NeuralAutomataAgent
    from die_amd.batch import BatchedNeuralAutomataAgent

    class NoMedium:
        world = None

        def __getattr__(self, name):
            raise AssertionError(f'the medium was touched ({name}) before the refusal')

    class Decomposed(NoMedium):
        world = (128, 128, 0, 0)

    ag = NeuralAutomataAgent(kernel_sizes=(3, 3), memory_channels=2, p_agent_dropout=0.25, dropout_seed=3)
    with pytest.raises(ValueError, match='agents'):
        ag.sense(NoMedium())
    with pytest.raises(NotImplementedError, match='decomposed'):
        ag.sense(Decomposed(), agents=object())
    with pytest.raises(NotImplementedError, match='decomposed'):
        ag.forward((object(), Decomposed()))
    with pytest.raises(NotImplementedError, match='differentiable_sense'):
        ag.differentiable_sense(NoMedium())
    with pytest.raises(NotImplementedError, match='differentiable_action'):
        ag.differentiable_action((None, NoMedium()))
    with pytest.raises(NotImplementedError, match='forward_device'):
        ag.model.forward_device(None)
    assert ag.dropout_step == 0 and ag.memory is None
    pop = BatchedNeuralAutomataAgent.__new__(BatchedNeuralAutomataAgent)
    pop.template, pop.dropout_seed, pop.dropout_step, pop._wide, pop._stock_channel, pop.env = ag, 5, 0, True, False, None
    for call in (pop.differentiable_sense, pop.differentiable_action, pop.forward_device):
        with pytest.raises(NotImplementedError, match='memory'):
            call()
    assert pop.dropout_step == 0

    class BornEnv:                                                               # the constructor refuses before it reads anything else
        dynamics = Dynamics(agents_born=True, agents_die=True)

        def __getattr__(self, name):
            raise AssertionError(f'the env was touched ({name}) before the refusal')

    with pytest.raises(NotImplementedError, match='agents_born'):
        BatchedNeuralAutomataAgent(BornEnv(), ag)


def test_examples_memory_channels_flag(lib):
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
    kw = population_eval.wide_keywords(p.parse_args(['--memory-channels', '2', '--hidden-channels', '16']))
    assert kw == dict(memory_channels=2, hidden_channels=16)
    ag = population_eval.make_template(0., kw)
    assert ag.memory_channels == 2 and ag.obs_channels[-2:] == ['memory_0', 'memory_1']


# ---------------------------------------------------------------------------------------------------- the symbols
def test_new_symbols_exported_with_the_documented_argument_counts(lib):
    so = C.CDLL(lib.LIB_PATH)
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    header = open(os.path.join(ROOT, 'include', 'die_hip.h')).read()
    assert '#define DIE_ABI_VERSION 24' in header and '#define DIE_MEMORY_MAX_CHANNELS 8' in header and lib.MEMORY_MAX_CHANNELS == 8
    for name, n_args in NEW.items():
        assert hasattr(so, name) and name in lib.EXPORTS, name
        assert len(lib._SIGNATURES[name][1]) == n_args and len(getattr(lib.lib, name).argtypes) == n_args, name
        proto = header[header.index(f'int {name}('):]
        proto = proto[:proto.index(';')]
        assert proto.count(',') + 1 == n_args, (name, proto)
    # the fused step is the stock step's arguments plus M, the memory, its planes and with_stock
    assert len(lib._SIGNATURES['die_nca_wide_env_step_batch_stock'][1]) + 4 == NEW['die_nca_wide_env_step_batch_memory']
    assert 'die_amd/csrc/die_memory.hip' in ' '.join(os.path.join('die_amd/csrc', s) for s in _build_sources())


def _build_sources():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build_list', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.SOURCES


# ---------------------------------------------------------------------------------------------------- the refusals
W, H, N = 20, 68, 300
STANDING, MEMORY, PLANES = FAKE, FAKE + (1 << 20), FAKE + (2 << 20)             # a megabyte apart: nothing overlaps


def _medium(L, W=W, H=H, gW=0):
    return L.Medium(W, H, L.DIE_F32, 5, FAKE, FAKE, FAKE, FAKE + 8, gW, gW, 0, 0, 0, 0, 0, 0, None)


def _batch(L, replicas=3, plane_stride=None, agent_stride=N, n=None, W=W, H=H):
    counts = [300, 17, 0] + [0] * 61 if n is None else list(n) + [0] * (64 - len(n))
    return L.Batch(replicas, 0, W * H if plane_stride is None else plane_stride, agent_stride, 1, (C.c_int64 * 64)(*counts))


def _expand(L, *, batch=False, null=None, M_=3, epoch=3, row_stride=N, n_slots=N, plane_stride=W * H, planes=PLANES, standing=STANDING,
            memory=MEMORY, W=W, H=H, gW=0, batch_plane_stride=None, **bkw):
    m, b = _medium(L, W, H, gW), _batch(L, W=W, H=H, plane_stride=batch_plane_stride, **bkw)
    args = dict(m=C.byref(m), b=C.byref(b), standing=standing, memory=memory, planes=planes)
    if null:
        args[null] = None
    if batch:
        return L.lib.die_memory_planes_batch(args['m'], args['b'], args['standing'], epoch, M_, args['memory'], row_stride, args['planes'], None)
    return L.lib.die_memory_planes(args['m'], args['standing'], epoch, M_, args['memory'], row_stride, n_slots, args['planes'], plane_stride, None)


def _gather(L, *, batch=False, null=None, null_array=None, M_=3, plane_stride=W * H, replica_stride=8 * W * H, row_stride=N, planes=PLANES,
            memory=MEMORY, W=W, H=H, gW=0, N_=N, slot=None, batch_plane_stride=None, **bkw):
    m, b = _medium(L, W, H, gW), _batch(L, W=W, H=H, plane_stride=batch_plane_stride, **bkw)
    arrays = {k: FAKE + (3 << 20) + 4096 * i for i, k in enumerate(('x', 'y', 'alive'), 1)}
    if null_array:
        arrays[null_array] = None
    a = L.Agents(N_, arrays['x'], arrays['y'], arrays['alive'], None, slot)
    args = dict(m=C.byref(m), a=C.byref(a), b=C.byref(b), planes=planes, memory=memory)
    if null:
        args[null] = None
    if batch:
        return L.lib.die_gather_memory_batch(args['m'], args['a'], args['b'], M_, args['planes'], plane_stride, replica_stride, args['memory'],
                                             row_stride, None)
    return L.lib.die_gather_memory(args['m'], args['a'], M_, args['planes'], plane_stride, args['memory'], row_stride, None)


COMMON = [
    ('null medium', dict(null='m'), ARG, b'null argument'),
    ('null memory', dict(null='memory'), ARG, b'null argument'),
    ('null planes', dict(null='planes'), ARG, b'null argument'),
    ('empty field', dict(W=0), ARG, b'bad size'),
    ('decomposed medium', dict(gW=128), UNSUPPORTED, b'decomposed'),
    ('no memory channel', dict(M_=0), ARG, b'0 memory channels outside 1..8'),
    ('nine memory channels', dict(M_=9), ARG, b'9 memory channels outside 1..8'),
]
EXPAND = COMMON + [
    ('null standing plane', dict(null='standing'), ARG, b'null argument'),
    ('epoch 0', dict(epoch=0), ARG, b'epoch 0 outside 1..31'),
    ('epoch 32', dict(epoch=32), ARG, b'epoch 32 outside 1..31'),
]
EXPAND_ALONE = EXPAND + [
    ('too many slots', dict(n_slots=1 << 27, row_stride=1 << 27), ARG, b'slots'),
    ('negative slots', dict(n_slots=-1), ARG, b'slots'),
    ('row_stride below a row', dict(row_stride=N - 1), ARG, b'row_stride'),
    ('plane_stride below a plane', dict(plane_stride=W * H - 1), ARG, b'plane_stride'),
    ('planes are the standing plane', dict(planes=STANDING), ARG, b'overlap the standing plane'),
    ('planes end in the standing plane', dict(planes=STANDING - 4 * (2 * W * H + 1)), ARG, b'overlap the standing plane'),
    ('planes start in the standing plane', dict(planes=STANDING + 8 * W * H - 4), ARG, b'overlap the standing plane'),
    ('planes are the memory', dict(planes=MEMORY), ARG, b'overlap the memory'),
    ('planes start in the last memory row', dict(planes=MEMORY + 4 * (3 * N - 1)), ARG, b'overlap the memory'),
]
BATCHED = [
    ('null batch', dict(null='b'), ARG, b'null argument'),
    ('no replica', dict(replicas=0), ARG, b'replicas'),
    ('65 replicas', dict(replicas=65), ARG, b'replicas'),
    ('plane_stride below a plane', dict(batch_plane_stride=W * H - 1), ARG, b'plane_stride'),
    ('no agent_stride', dict(agent_stride=0), ARG, b'agent_stride'),
    ('a negative count', dict(n=[300, -1, 0]), ARG, b'replica 1 has -1 agents'),
    ('a count above the stride', dict(n=[300, 17, 301]), ARG, b'replica 2 has 301 agents'),
    ('row_stride below a row', dict(row_stride=N - 1), ARG, b'row_stride'),
]
EXPAND_BATCH = EXPAND + BATCHED + [
    ('planes are the standing planes', dict(planes=STANDING), ARG, b'overlap the standing planes'),
    ('planes start in the last standing plane', dict(planes=STANDING + 8 * 3 * W * H - 4), ARG, b'overlap the standing planes'),
    ('planes are the memory', dict(planes=MEMORY), ARG, b'overlap the memory'),
    ('planes start in the last replica\'s memory', dict(planes=MEMORY + 4 * (9 * N - 1)), ARG, b'overlap the memory'),
]
GATHER = COMMON + [
    ('null agents', dict(null='a'), ARG, b'null argument'),
    ('null x', dict(null_array='x'), ARG, b'null agent array'),
    ('null alive', dict(null_array='alive'), ARG, b'null agent array'),
    ('plane_stride below a plane', dict(plane_stride=W * H - 1), ARG, b'plane_stride'),
    ('memory is the planes', dict(memory=PLANES), ARG, b'overlaps the planes'),
]
GATHER_ALONE = GATHER + [
    ('too many slots', dict(N_=1 << 27, row_stride=1 << 27), ARG, b'slots'),
    ('row_stride below a row', dict(row_stride=N - 1), ARG, b'row_stride'),
    ('memory starts in the last plane', dict(memory=PLANES + 4 * (3 * W * H - 1)), ARG, b'overlaps the planes'),
]
GATHER_BATCH = GATHER + [(c[0] + ' (the batch)',) + c[1:] for c in BATCHED] + [
    ('a slot array', dict(slot=FAKE), ARG, b'slot order'),
    ('replica_stride below the planes', dict(replica_stride=3 * W * H - 1), ARG, b'replica_stride'),
    ('memory starts in the last replica\'s planes', dict(memory=PLANES + 4 * (2 * 8 * W * H + 3 * W * H - 1)), ARG, b'overlaps the planes'),
]

def _ids(v):
    return v if isinstance(v, str) else None


@pytest.mark.parametrize('case, kw, status, needle', EXPAND_ALONE, ids=_ids)
def test_memory_planes_refusals(lib, case, kw, status, needle):
    assert _expand(lib, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and b'die_memory_planes:' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


@pytest.mark.parametrize('case, kw, status, needle', EXPAND_BATCH, ids=_ids)
def test_memory_planes_batch_refusals(lib, case, kw, status, needle):
    assert _expand(lib, batch=True, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and b'die_memory_planes_batch:' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


@pytest.mark.parametrize('case, kw, status, needle', GATHER_ALONE, ids=_ids)
def test_gather_memory_refusals(lib, case, kw, status, needle):
    assert _gather(lib, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and b'die_gather_memory:' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


@pytest.mark.parametrize('case, kw, status, needle', GATHER_BATCH, ids=_ids)
def test_gather_memory_batch_refusals(lib, case, kw, status, needle):
    assert _gather(lib, batch=True, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and b'die_gather_memory_batch:' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


def _step(lib, *, null=None, replicas=4, M_=2, with_stock=0, cin0=None, cout=None, with_agents=1, hidden=8, sense_epoch=1, epoch=2, n=10,
          rows=None, gW=0, scratch_short=False, slot=None, H=96):
    """The fused step: layer 0 reads `cin0` planes (default: what M_ and with_stock ask for), the last layer gives `cout`."""
    L, W = lib, 96
    m = L.Medium(W, H, L.DIE_F32, epoch, FAKE, FAKE, FAKE, FAKE + 8, gW, gW, 0, 0, 0, 0, 0, 0, None)
    a = L.Agents(10, FAKE, FAKE, FAKE, FAKE, slot)
    good_m = min(max(M_, 1), 8)
    cin0 = 2 + with_agents + good_m + (with_stock == 1) if cin0 is None else cin0
    cout = 3 + good_m if cout is None else cout
    shapes = ((3, cin0, hidden), (3, hidden, cout))
    arr = (L.NcaLayer * 2)(*[L.NcaLayer(k, ci, co, 1, FAKE, co * ci * k * k) for k, ci, co in shapes])
    need = L.lib.die_nca_wide_batch_scratch_bytes(W, H, replicas, 2, min(max(hidden, cout), 32)) if 1 <= replicas <= 64 else 1 << 30
    nca = L.NcaBatch(2, 0, with_agents, sense_epoch, arr, (C.c_float * 3)(0.01, 0.01, 2.0), 0, FAKE, need - (4 if scratch_short else 0))
    d = L.Dynamics(0.1, 0.025, 0.8, 0, 0, 0.02, 0.01, 1, 0, 0, 0, 0)
    b = L.Batch(replicas, 0, W * H, 10, 1, (C.c_int64 * 64)(*([n] * 64)))
    args = dict(m=C.byref(m), a=C.byref(a), nca=C.byref(nca), d=C.byref(d), b=C.byref(b), results=FAKE, ws=FAKE, standing=FAKE + (1 << 24),
                memory=FAKE + (2 << 24), planes=FAKE + (3 << 24))
    if null:
        args[null] = None
    rows_dev, rows_host = {None: (None, None), 'device only': (FAKE, None), 'host only': (None, (L.DynamicsRow * 64)())}[rows]
    return L.lib.die_nca_wide_env_step_batch_memory(args['m'], args['a'], args['nca'], None, args['d'], args['b'], args['results'], args['ws'],
                                                    64 * L.lib.die_batch_workspace_bytes(1), None, rows_dev, rows_host, args['standing'], M_,
                                                    args['memory'], args['planes'], with_stock, None)


STEP_CASES = [
    ('null medium', dict(null='m'), ARG, b'null argument'),
    ('null agents', dict(null='a'), ARG, b'null argument'),
    ('null stack', dict(null='nca'), ARG, b'null argument'),
    ('null dynamics', dict(null='d'), ARG, b'null argument'),
    ('null batch', dict(null='b'), ARG, b'null argument'),
    ('null results', dict(null='results'), ARG, b'null argument'),
    ('null workspace', dict(null='ws'), ARG, b'null argument'),
    ('null standing planes', dict(null='standing'), ARG, b'null standing planes'),
    ('null memory', dict(null='memory'), ARG, b'null standing planes, memory'),
    ('null memory planes', dict(null='planes'), ARG, b'memory planes'),
    ('no memory channel', dict(M_=0), ARG, b'0 memory channels outside 1..8'),
    ('nine memory channels', dict(M_=9), ARG, b'9 memory channels outside 1..8'),
    ('with_stock 2', dict(with_stock=2), ARG, b'with_stock is 0 or 1'),
    ('no replica', dict(replicas=0), ARG, b'replicas'),
    ('65 replicas', dict(replicas=65), ARG, b'replicas'),
    ('decomposed medium', dict(gW=128), ARG, b'periodic single-tile'),
    ('agents not in slot order', dict(slot=FAKE), ARG, b'slot order'),
    ('H no multiple of 4', dict(H=98), UNSUPPORTED, b'H % 4 == 0'),
    ("layer 0 reads the parent's 3 planes", dict(cin0=3), ARG, b'input has 5'),
    ('layer 0 reads the stock step\'s 4 planes', dict(cin0=4), ARG, b'input has 5'),
    ('layer 0 misses the stock plane', dict(with_stock=1, cin0=5), ARG, b'input has 6'),
    ('layer 0 without the agents channel', dict(with_agents=0, cin0=5), ARG, b'input has 4'),
    ('the last layer gives 3 planes', dict(cout=3), ARG, b'the last layer gives 3 planes'),
    ('the last layer gives one plane too many', dict(cout=6), ARG, b'the last layer gives 6 planes'),
    ('33 hidden channels', dict(hidden=33), ARG, b'at most 32 out'),
    ('scratch four bytes short', dict(scratch_short=True), ARG, b'scratch too small'),
    ('claims do not follow the sensing', dict(sense_epoch=1, epoch=3), ARG, b'cannot follow sensing'),
    ('sense_epoch 0', dict(sense_epoch=0, epoch=1), ARG, b'cannot follow sensing'),
    ('a replica without agents', dict(n=0), ARG, b'has 0 agents'),
    ('a replica above the stride', dict(n=11), ARG, b'has 11 agents'),
    ('device rows without host rows', dict(rows='device only'), ARG, b'rows_host == NULL'),
    ('host rows without device rows', dict(rows='host only'), ARG, b'rows == NULL'),
]


@pytest.mark.parametrize('case, kw, status, needle', STEP_CASES, ids=_ids)
def test_memory_step_refusals(lib, case, kw, status, needle):
    assert _step(lib, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and b'die_nca_wide_env_step_batch_memory:' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())
