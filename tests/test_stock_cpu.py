"""The stock channel (NeuralAutomataAgent(with_stock_channel=True), die_stock.hip), CPU side: known answers of the numpy model
(tests/stock_plane_model.py), the new symbols under the unchanged ABI version, every refusal of the four new entry points on
the host (fake pointers: a launch would have failed), and the Python surface — init_params, save / load, the observation
channels, the population's architecture and every differentiable refusal.  No kernel is launched here."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from tests import stock_plane_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {'die_stock_plane': 5, 'die_stock_plane_batch': 6, 'die_nca_env_step_batch_stock': 14, 'die_nca_wide_env_step_batch_stock': 14}
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
    """A Q0.32 word in the middle of each cell's interval of an axis of n cells."""
    return np.array([min(TOP, (c << 32) // (n - 1)) for c in cells], dtype=np.uint32)


def test_model_the_highest_slot_wins_and_dead_slots_are_skipped():
    W, H = 7, 9
    cx, cy = [3, 3, 3, 3, 0], [4, 4, 4, 4, 0]
    x, y = _words(cx, W), _words(cy, H)
    food = np.array([1.5, 2.5, 3.5, 4.5, 9.0], dtype=np.float32)
    S = M.stock_plane(W, H, x, y, np.array([1, 1, 1, 0, 0]), food)          # three alive on (3, 4), a dead slot above them
    assert S[3, 4] == np.float32(3.5) and S.sum() == np.float32(3.5) and S.dtype == np.float32
    S = M.stock_plane(W, H, x, y, np.array([1, 0, 1, 0, 1]), food)          # a dead slot BETWEEN them is skipped
    assert S[3, 4] == np.float32(3.5) and S[0, 0] == np.float32(9.0) and np.count_nonzero(S) == 2
    S = M.stock_plane(W, H, x, y, np.array([1, 1, 0, 0, 0]), food)
    assert S[3, 4] == np.float32(2.5)
    occ, slot = M.stock_winners(W, H, x, y, np.array([1, 1, 1, 1, 0]))
    assert occ.sum() == 1 and slot[3, 4] == 3 and slot[0, 0] == -1
    assert not M.stock_plane(W, H, x, y, np.zeros(5), food).any()             # nobody alive: an empty plane


def test_model_coordinate_ends_land_on_the_first_and_last_cell():
    for n in (2, 5, 20, 68, 96):
        assert M.cell(np.array([0, TOP], dtype=np.uint32), n).tolist() == [0, n - 1]
    W, H = 20, 68
    x, y = np.array([0, TOP, 0, TOP], dtype=np.uint32), np.array([0, TOP, TOP, 0], dtype=np.uint32)
    S = M.stock_plane(W, H, x, y, np.ones(4), np.array([1, 2, 3, 4], dtype=np.float32))
    assert (S[0, 0], S[W - 1, H - 1], S[0, H - 1], S[W - 1, 0]) == (1, 2, 3, 4) and np.count_nonzero(S) == 4
    # the nearest label: the midpoint between two labels of a 5-cell axis goes up, a word below it down
    half = (1 << 32) // 8
    assert M.cell(np.array([half - 1, half, half + 1], dtype=np.uint32), 5).tolist() == [0, 1, 1]
    # what to_numpy() hands out (X / 2^32) comes back as the same words
    xs = np.array([0, 1, 12345, TOP - 1, TOP], dtype=np.uint32)
    assert np.array_equal(M.q32_words(xs.astype(np.float64) / 4294967296.0), xs)


def test_model_negative_and_denormal_stocks_keep_their_bits():
    W, H = 4, 4
    x, y = _words([1, 2], W), _words([1, 2], H)
    food = np.array([-0.75, 1e-41], dtype=np.float32)
    S = M.stock_plane(W, H, x, y, np.ones(2), food)
    assert S[1, 1] == np.float32(-0.75) and S[2, 2].view(np.uint32) == food[1].view(np.uint32) != 0
    words = M.encode(7, np.array([0, 1]), food)
    occ, slot, bits, tag = M.decode(words, 7)
    assert occ.all() and slot.tolist() == [0, 1] and np.array_equal(bits, food.view(np.uint32)) and tag.tolist() == [7, 7]
    occ, slot, bits, tag = M.decode(words, 8)                                    # read at another epoch: nobody there
    assert not occ.any() and slot.tolist() == [-1, -1] and not bits.any() and tag.tolist() == [7, 7]
    # the word orders by (epoch, slot id) before the payload: a negative stock (sign bit set) never outranks a higher slot
    assert M.encode(7, 1, np.float32(1.0)) > M.encode(7, 0, np.float32(-1.0)) and M.encode(8, 0, 0.0) > M.encode(7, 99, -1.0)


# ---------------------------------------------------------------------------------------------------- the symbols
def test_new_symbols_exported_with_the_documented_argument_counts(lib):
    so = C.CDLL(lib.LIB_PATH)
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    for name, n_args in NEW.items():
        assert hasattr(so, name) and name in lib.EXPORTS, name
        assert len(lib._SIGNATURES[name][1]) == n_args, name
    assert lib.DIE_PLANE_STOCK == 3
    header = open(os.path.join(ROOT, 'include', 'die_hip.h')).read()
    assert 'DIE_PLANE_STOCK = 3' in header and '#define DIE_ABI_VERSION 24' in header
    for name, n_args in NEW.items():                                              # the prototypes say the same
        proto = header[header.index(f'int {name}('):]
        proto = proto[:proto.index(';')]
        assert proto.count(',') + 1 == n_args, (name, proto)
    # the stock entry points are their parents' arguments plus the planes
    assert len(lib._SIGNATURES['die_nca_env_step_batch_rows'][1]) + 1 == NEW['die_nca_env_step_batch_stock']
    assert len(lib._SIGNATURES['die_nca_wide_env_step_batch'][1]) + 1 == NEW['die_nca_wide_env_step_batch_stock']


# ---------------------------------------------------------------------------------------------------- the refusals
def _plane(lib, *, batch=False, null=None, W=20, H=68, gW=0, epoch=3, replicas=3, plane_stride=None, agent_stride=300, n=None,
           null_array=None, N=300):
    L = lib
    m = L.Medium(W, H, L.DIE_F32, 5, FAKE, FAKE, FAKE, FAKE + 8, gW, gW, 0, 0, 0, 0, 0, 0, None)
    arrays = {k: FAKE + 4096 * i for i, k in enumerate(('x', 'y', 'alive', 'agent_food'), 1)}
    if null_array:
        arrays[null_array] = None
    a = L.Agents(N, arrays['x'], arrays['y'], arrays['alive'], arrays['agent_food'], None)
    counts = [300, 17, 0] + [0] * 61 if n is None else list(n) + [0] * (64 - len(n))
    b = L.Batch(replicas, 0, W * H if plane_stride is None else plane_stride, agent_stride, 1, (C.c_int64 * 64)(*counts))
    args = dict(m=C.byref(m), a=C.byref(a), b=C.byref(b), plane=FAKE + (1 << 16))
    if null:
        args[null] = None
    if batch:
        return L.lib.die_stock_plane_batch(args['m'], args['a'], args['b'], epoch, args['plane'], None)
    return L.lib.die_stock_plane(args['m'], args['a'], epoch, args['plane'], None)


def _step(lib, *, wide=False, null=None, replicas=4, cin0=4, with_agents=1, hidden=None, sense_epoch=1, epoch=2, n=10, rows=None,
          gW=0, scratch_short=False, slot=None, H=96, stock=FAKE + (1 << 24)):
    """A batched step whose layer 0 reads `cin0` planes; `stock` non-null takes the new path."""
    L, W = lib, 96
    m = L.Medium(W, H, L.DIE_F32, epoch, FAKE, FAKE, FAKE, FAKE + 8, gW, gW, 0, 0, 0, 0, 0, 0, None)
    a = L.Agents(10, FAKE, FAKE, FAKE, FAKE, slot)
    mid = cin0 if hidden is None else hidden
    shapes = ((3, cin0, mid), (3, mid, 3))
    arr = (L.NcaLayer * 2)(*[L.NcaLayer(k, cin, cout, 1 if wide else 0, FAKE, cout * cin * k * k) for k, cin, cout in shapes])
    if wide:
        need = L.lib.die_nca_wide_batch_scratch_bytes(W, H, replicas, 2, max(mid, 3)) if 1 <= replicas <= 64 else 1 << 30
    else:
        need = L.lib.die_nca_batch_scratch_bytes(W, H, replicas, 2) if 1 <= replicas <= 64 else 1 << 30
    nca = L.NcaBatch(2, 0, with_agents, sense_epoch, arr, (C.c_float * 3)(0.01, 0.01, 2.0), 0, FAKE, need - (4 if scratch_short else 0))
    d = L.Dynamics(0.1, 0.025, 0.8, 0, 0, 0.02, 0.01, 1, 0, 0, 0, 0)
    b = L.Batch(replicas, 0, W * H, 10, 1, (C.c_int64 * 64)(*([n] * 64)))
    args = dict(m=C.byref(m), a=C.byref(a), nca=C.byref(nca), d=C.byref(d), b=C.byref(b), results=FAKE, ws=FAKE)
    if null:
        args[null] = None
    rows_dev, rows_host = {None: (None, None), 'device only': (FAKE, None), 'host only': (None, (L.DynamicsRow * 64)())}[rows]
    fn = L.lib.die_nca_wide_env_step_batch_stock if wide else L.lib.die_nca_env_step_batch_stock
    return fn(args['m'], args['a'], args['nca'], None, args['d'], args['b'], args['results'], args['ws'],
              64 * L.lib.die_batch_workspace_bytes(1), None, rows_dev, rows_host, stock, None)


PLANE_CASES = [
    ('null medium', dict(null='m'), ARG, b'null argument'),
    ('null agents', dict(null='a'), ARG, b'null argument'),
    ('null plane', dict(null='plane'), ARG, b'null argument'),
    ('null x', dict(null_array='x'), ARG, b'null agent array'),
    ('null alive', dict(null_array='alive'), ARG, b'null agent array'),
    ('null agent_food', dict(null_array='agent_food'), ARG, b'null agent array'),
    ('empty field', dict(W=0), ARG, b'bad size'),
    ('decomposed medium', dict(gW=128), UNSUPPORTED, b'decomposed'),
    ('epoch 0', dict(epoch=0), ARG, b'epoch 0 outside 1..31'),
    ('epoch 32', dict(epoch=32), ARG, b'epoch 32 outside 1..31'),
]
BATCH_CASES = [
    ('null batch', dict(null='b'), ARG, b'null argument'),
    ('no replica', dict(replicas=0), ARG, b'replicas'),
    ('65 replicas', dict(replicas=65), ARG, b'replicas'),
    ('plane_stride below a plane', dict(plane_stride=20 * 68 - 1), ARG, b'plane_stride'),
    ('no agent_stride', dict(agent_stride=0), ARG, b'agent_stride'),
    ('a negative count', dict(n=[300, -1, 0]), ARG, b'replica 1 has -1 agents'),
    ('a count above the stride', dict(n=[300, 17, 301]), ARG, b'replica 2 has 301 agents'),
]


@pytest.mark.parametrize('case, kw, status, needle', PLANE_CASES + [('too many slots', dict(N=1 << 27), ARG, b'slots')], ids=lambda v: v if isinstance(v, str) else None)
def test_stock_plane_refusals(lib, case, kw, status, needle):
    assert _plane(lib, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and b'die_stock_plane:' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


@pytest.mark.parametrize('case, kw, status, needle', PLANE_CASES + BATCH_CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_stock_plane_batch_refusals(lib, case, kw, status, needle):
    assert _plane(lib, batch=True, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and b'die_stock_plane_batch:' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


STEP_CASES = [
    ('null medium', dict(null='m'), ARG, b'null argument'),
    ('null agents', dict(null='a'), ARG, b'null argument'),
    ('null stack', dict(null='nca'), ARG, b'null argument'),
    ('null dynamics', dict(null='d'), ARG, b'null argument'),
    ('null batch', dict(null='b'), ARG, b'null argument'),
    ('null results', dict(null='results'), ARG, b'null argument'),
    ('null workspace', dict(null='ws'), ARG, b'null argument'),
    ('no replica', dict(replicas=0), ARG, b'replicas'),
    ('65 replicas', dict(replicas=65), ARG, b'replicas'),
    ('decomposed medium', dict(gW=128), ARG, b'periodic single-tile'),
    ('agents not in slot order', dict(slot=FAKE), ARG, b'slot order'),
    ('H no multiple of 4', dict(H=98), UNSUPPORTED, b'H % 4 == 0'),
    ("layer 0 reads the parent's 3 planes", dict(cin0=3), ARG, b'input has 4'),
    ('layer 0 reads 3 planes without the agents channel, its parent 2', dict(cin0=2, with_agents=0), ARG, b'input has 3'),
    ('layer 0 reads 5 planes', dict(cin0=5), ARG, b'input has 4'),
    ('scratch four bytes short', dict(scratch_short=True), ARG, b'scratch too small'),
    ('claims do not follow the sensing', dict(sense_epoch=1, epoch=3), ARG, b'cannot follow sensing'),
    ('sense_epoch 0', dict(sense_epoch=0, epoch=1), ARG, b'cannot follow sensing'),
    ('a replica without agents', dict(n=0), ARG, b'has 0 agents'),
    ('a replica above the stride', dict(n=11), ARG, b'has 11 agents'),
    ('device rows without host rows', dict(rows='device only'), ARG, b'rows_host == NULL'),
    ('host rows without device rows', dict(rows='host only'), ARG, b'rows == NULL'),
]


@pytest.mark.parametrize('wide', [False, True], ids=['narrow', 'wide'])
@pytest.mark.parametrize('case, kw, status, needle', STEP_CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_stock_step_refusals(lib, wide, case, kw, status, needle):
    name = b'die_nca_wide_env_step_batch_stock' if wide else b'die_nca_env_step_batch_stock'
    assert _step(lib, wide=wide, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error() and name + b':' in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


def test_stock_step_without_planes_is_the_parent_call(lib):
    """stock == NULL: the parent's checks under the parent's name — its layer 0 reads 3 planes, and 4 are refused."""
    assert _step(lib, stock=None, cin0=4) == ARG
    assert b'die_nca_env_step_batch_rows:' in lib.lib.die_last_error() and b'input has 3' in lib.lib.die_last_error()
    assert _step(lib, stock=None, cin0=3, n=0) == ARG                   # (the narrow parent wants both tables: die_nca_env_step_batch_rows)
    assert b'die_nca_env_step_batch_rows:' in lib.lib.die_last_error()
    assert _step(lib, wide=True, stock=None, cin0=4, hidden=8) == ARG
    assert b'die_nca_wide_env_step_batch:' in lib.lib.die_last_error() and b'input has 3' in lib.lib.die_last_error()
    assert _step(lib, wide=True, stock=None, cin0=3, hidden=8, n=0) == ARG
    assert b'die_nca_wide_env_step_batch:' in lib.lib.die_last_error() and b'has 0 agents' in lib.lib.die_last_error()
    # the wide stack's limits hold with the planes too: 33 hidden channels
    assert _step(lib, wide=True, cin0=4, hidden=33) == ARG and b'at most 32 out' in lib.lib.die_last_error()
    assert _step(lib, wide=False, cin0=4, hidden=5) == ARG and b'at most 4 out' in lib.lib.die_last_error()


def test_the_adjoint_still_refuses_the_stock_kind(lib):
    L = lib
    planes = (L.ConvPlane * 4)(*[L.ConvPlane(FAKE + 65536 * i, L.DIE_PLANE_STOCK if i == 3 else 0, 0) for i in range(4)])
    ptrs = lambda base: (C.c_void_p * 4)(*[FAKE + 65536 * (base + i) for i in range(4)])
    need = L.lib.die_conv2d_backward_workspace_bytes(24, 40, 4, 3, 3)
    rc = L.lib.die_conv2d_backward(24, 40, 4, planes, 1, 3, ptrs(8), 3, FAKE + 65536 * 40, FAKE + 65536 * 41, None, ptrs(24), None, 0,
                                   FAKE + 65536 * 48, need, None)
    assert rc == ARG and b'bad input plane 3' in L.lib.die_last_error()
    # … and the forward's other refusals are what they were: a kind past the last one, a null plane of the new kind
    outs = (C.c_void_p * 3)(*[FAKE + 65536 * (8 + i) for i in range(3)])
    planes[3].kind = 4
    assert L.lib.die_conv2d(24, 40, 4, planes, 1, 3, outs, 3, FAKE + 65536 * 40, 1, 0, None) == ARG
    assert b'bad input plane 3' in L.lib.die_last_error()
    # the stock plane is the LAST input plane: kind 3 anywhere else stays a plane of no kind, in both forward calls
    for at in (0, 1, 2):
        planes[3].kind = 0
        planes[at].kind = L.DIE_PLANE_STOCK
        assert L.lib.die_conv2d(24, 40, 4, planes, 1, 3, outs, 3, FAKE + 65536 * 40, 1, 0, None) == ARG
        assert b'bad input plane %d' % at in L.lib.die_last_error()
        assert L.lib.die_conv2d_wide(24, 40, 4, planes, 1, 3, FAKE + 65536 * 8, 24 * 40, 3, FAKE + 65536 * 40, 1, 0, None, None) == ARG
        assert b'bad input plane %d' % at in L.lib.die_last_error()
        planes[at].kind = 0
    planes[3].kind, planes[3].data = L.DIE_PLANE_STOCK, None
    assert L.lib.die_conv2d(24, 40, 4, planes, 1, 3, outs, 3, FAKE + 65536 * 40, 1, 0, None) == ARG
    assert L.lib.die_conv2d_wide(24, 40, 4, planes, 1, 3, FAKE + 65536 * 8, 24 * 40, 3, FAKE + 65536 * 40, 1, 0, None, None) == ARG
    assert b'bad input plane 3' in L.lib.die_last_error()


# ---------------------------------------------------------------------------------------------------- the Python surface
def test_init_params_save_load_and_channels(lib):
    import torch
    from die_amd import NeuralAutomataAgent
    plain = NeuralAutomataAgent(kernel_sizes=(3, 3))
    assert 'with_stock_channel' not in plain.init_params and plain.with_stock_channel is False
    assert 'with_stock_channel' not in NeuralAutomataAgent(with_stock_channel=False).init_params
    assert plain.obs_channels == ['agents', 'env_food', 'chem1'] and plain.model.kernels[0].in_channels == 3
    with pytest.raises(ValueError, match='with_stock_channel'):
        NeuralAutomataAgent(with_stock_channel=1)
    for with_agents, n in ((True, 4), (False, 3)):
        for kw in (dict(kernel_sizes=(3, 3)), dict(kernel_sizes=(3, 1, 3), hidden_channels=8, hidden_activation='relu')):
            ag = NeuralAutomataAgent(scale=0.02, with_agent_channel=with_agents, with_stock_channel=True, **kw)
            assert ag.init_params['with_stock_channel'] is True and ag.with_stock_channel is True
            assert ag.obs_channels[-1] == 'agent_food' and len(ag.obs_channels) == n
            assert ag.obs_channels[:-1] == NeuralAutomataAgent(with_agent_channel=with_agents).obs_channels
            layers = ag.model.conv_layers()
            assert ag.model.kernels[0].in_channels == n and layers[-1].out_channels == 3
            if 'hidden_channels' not in kw:                                       # a narrow stack stays within 4 channels
                assert all(k.out_channels == n for k in layers[:-1]) and n <= 4
            ag.model.init_weights()
            buf = io.BytesIO()
            ag.save(buf)
            buf.seek(0)
            back = NeuralAutomataAgent.load(buf)
            assert back.with_stock_channel is True and back.obs_channels == ag.obs_channels and back.init_params == ag.init_params
            for p, q in zip(back.model.parameters(), ag.model.parameters()):
                assert torch.equal(p, q)
    buf = io.BytesIO()
    plain.save(buf)
    buf.seek(0)
    saved = torch.load(buf)
    assert 'with_stock_channel' not in saved['params_dict'] and 'dropout_seed' not in saved['params_dict']


def test_sense_needs_the_agents_before_anything_is_touched(lib):
    from die_amd import NeuralAutomataAgent

    class NoMedium:
        world = None

        def __getattr__(self, name):
            raise AssertionError(f'the medium was touched ({name}) before the refusal')

    class Decomposed(NoMedium):
        world = (128, 128, 0, 0)

    ag = NeuralAutomataAgent(kernel_sizes=(3, 3), with_stock_channel=True, p_agent_dropout=0.25, dropout_seed=3)
    with pytest.raises(ValueError, match='agents'):
        ag.sense(NoMedium())
    with pytest.raises(NotImplementedError, match='decomposed'):
        ag.sense(Decomposed(), agents=object())
    with pytest.raises(NotImplementedError, match='decomposed'):
        ag.forward((object(), Decomposed()))
    assert ag.dropout_step == 0


def test_every_differentiable_refusal_is_made_before_a_launch(lib):
    from die_amd import NeuralAutomataAgent
    from die_amd.batch import BatchedNeuralAutomataAgent, _architecture

    class NoMedium:
        def __getattr__(self, name):
            raise AssertionError(f'the medium was touched ({name}) before the refusal')

    for kw in (dict(kernel_sizes=(3, 3)), dict(kernel_sizes=(3, 3), hidden_channels=8)):
        ag = NeuralAutomataAgent(with_stock_channel=True, p_agent_dropout=0.25, dropout_seed=5, **kw)
        with pytest.raises(NotImplementedError, match='differentiable_sense'):
            ag.differentiable_sense(NoMedium())
        with pytest.raises(NotImplementedError, match='differentiable_action'):
            ag.differentiable_action((None, NoMedium()))
        assert ag.dropout_step == 0
        # the batched twins: a population object without a BatchedEnv behind it — the refusal comes before anything is read
        pop = BatchedNeuralAutomataAgent.__new__(BatchedNeuralAutomataAgent)
        pop.template, pop.dropout_seed, pop.dropout_step, pop._wide, pop._stock_channel, pop.env = ag, 5, 0, ag.model.wide, True, None
        for call in (pop.differentiable_sense, pop.differentiable_action, pop.forward_device):
            with pytest.raises(NotImplementedError):
                call()
        assert pop.dropout_step == 0
        assert _architecture(ag)['with_stock_channel'] is True
    assert _architecture(NeuralAutomataAgent())['with_stock_channel'] is False
    assert _architecture(NeuralAutomataAgent(with_agent_channel=False, with_stock_channel=True))['with_agent_channel'] is False
    assert _architecture(NeuralAutomataAgent(with_stock_channel=True))['with_agent_channel'] is True


def test_examples_stock_channel_flag_and_init_from_message(lib):
    import argparse
    import importlib
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    try:
        learning_agents, population_eval = importlib.import_module('learning_agents'), importlib.import_module('population_eval')
    finally:
        sys.path.pop(0)
    p = argparse.ArgumentParser()
    population_eval.add_wide_arguments(p)
    assert population_eval.wide_keywords(p.parse_args([])) == {}
    kw = population_eval.wide_keywords(p.parse_args(['--stock-channel', '--hidden-channels', '8']))
    assert kw == dict(with_stock_channel=True, hidden_channels=8)
    stock, plain = population_eval.make_template(0., dict(with_stock_channel=True)), population_eval.make_template()
    assert stock.obs_channels[-1] == 'agent_food' and learning_agents.init_from_mismatch(stock, stock, 'a.pt') is None
    assert learning_agents.init_from_mismatch(plain, plain, 'a.pt') is None
    msg = learning_agents.init_from_mismatch(plain, stock, 'a.pt')
    assert 'a.pt' in msg and 'observes 3 channels' in msg and 'observe 4' in msg and 'without --stock-channel' in msg
    msg = learning_agents.init_from_mismatch(stock, plain, 'b.pt')
    assert 'b.pt' in msg and 'observes 4 channels' in msg and 'observe 3' in msg and 'with --stock-channel' in msg


def test_from_agents_refuses_a_mixed_population(lib):
    from die_amd import NeuralAutomataAgent
    from die_amd.batch import BatchedNeuralAutomataAgent

    class FakeEnv:
        R = 2

    # (3 observed channels both: the agents channel traded for the stock channel is still another architecture)
    mixed = [NeuralAutomataAgent(with_agent_channel=False, with_stock_channel=True), NeuralAutomataAgent()]
    assert mixed[0].model.kernels[0].in_channels == mixed[1].model.kernels[0].in_channels == 3
    with pytest.raises(ValueError, match='architecture'):
        BatchedNeuralAutomataAgent.from_agents(FakeEnv(), mixed)
    with pytest.raises(ValueError, match='architecture'):
        BatchedNeuralAutomataAgent.from_agents(FakeEnv(), [NeuralAutomataAgent(with_stock_channel=True), NeuralAutomataAgent()])
