"""Seeded agent dropout, CPU side: the three entry points are exported under the unchanged ABI version, every bad argument is
refused on the host before any launch, and the numpy twin of the mask (tests/dropout_model.py) is pinned by literals, by its
dropped fraction and by what must and must not change it.  No kernel is launched here."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import dropout_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('die_conv2d_dropout', 'die_nca_env_step_batch_dropout', 'die_dropout_mask')
FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


def test_new_symbols_exported_under_abi_24(lib):
    so = C.CDLL(lib.LIB_PATH)
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    for name in NEW:
        assert hasattr(so, name) and name in lib.EXPORTS, name
    # die_nca_dropout: double p, uint64 seed, uint64 seed_stride, uint32 step, uint32 reserved
    assert C.sizeof(lib.NcaDropout) == 8 + 8 + 8 + 4 + 4
    d = lib.nca_dropout(0.25, -1, 2 ** 64 + 3, 2 ** 32 + 5)
    assert (d.p, d.seed, d.seed_stride, d.step, d.reserved) == (0.25, 2 ** 64 - 1, 3, 5, 0)


BAD_P = [0.0, -0.1, 1.5, float('nan')]


def _mask(lib, *, p=0.25, W=8, H=8, replicas=1, plane_stride=None, drop=True, out=FAKE, reserved=0):
    d = lib.NcaDropout(p, 1, 1, 0, reserved)
    return lib.lib.die_dropout_mask(W, H, C.byref(d) if drop else None, replicas, W * H if plane_stride is None else plane_stride, out, None)


def _conv(lib, *, p=0.25, null=None):
    d = lib.NcaDropout(p, 1, 0, 0, 0)
    planes = (lib.ConvPlane * 3)(*[lib.ConvPlane(FAKE + 4096 * i, lib.DIE_PLANE_F32, 0) for i in range(3)])
    outs = (C.c_void_p * 3)(*[FAKE + 4096 * (8 + i) for i in range(3)])
    args = dict(planes=planes, outs=outs, w=FAKE + 4096 * 16)
    if null:
        args[null] = None
    return lib.lib.die_conv2d_dropout(8, 8, 3, args['planes'], 1, 3, args['outs'], 3, args['w'], 1, 0, C.byref(d), None)


def _step(lib, *, p=0.25, replicas=4, null=None, reserved=0):
    L, W, H = lib, 96, 96
    m = L.Medium(W, H, L.DIE_F32, 2, FAKE, FAKE, FAKE, FAKE + 8, 0, 0, 0, 0, 0, 0, 0, 0, None)
    a = L.Agents(10, FAKE, FAKE, FAKE, FAKE, None)
    layers = ((3, 3, 3), (3, 3, 3))
    arr = (L.NcaLayer * len(layers))(*[L.NcaLayer(k, cin, cout, 0, FAKE, cout * cin * k * k) for k, cin, cout in layers])
    need = L.lib.die_nca_batch_scratch_bytes(W, H, replicas, len(layers)) if 1 <= replicas <= 64 else 1 << 30
    nca = L.NcaBatch(len(layers), 0, 1, 1, arr, (C.c_float * 3)(0.01, 0.01, 2.0), 0, FAKE, need)
    d = L.Dynamics(0.1, 0.025, 0.8, 0, 0, 0.02, 0.01, 1, 0, 0, 0, 0)
    b = L.Batch(replicas, 0, W * H, 10, 1, (C.c_int64 * 64)(*([10] * 64)))
    drop = L.NcaDropout(p, 1, 1, 0, reserved)
    args = dict(m=C.byref(m), nca=C.byref(nca), results=FAKE, ws=FAKE)
    if null:
        args[null] = None
    return L.lib.die_nca_env_step_batch_dropout(args['m'], C.byref(a), args['nca'], None, C.byref(d), C.byref(b), args['results'], args['ws'],
                                                64 * L.lib.die_batch_workspace_bytes(1), C.byref(drop), None)


@pytest.mark.parametrize('call', [_mask, _conv, _step], ids=['mask', 'conv2d', 'step_batch'])
@pytest.mark.parametrize('p', BAD_P, ids=str)
def test_bad_p_refused_before_launch(lib, call, p):
    assert call(lib, p=p) == -1
    assert b'0 < p <= 1' in lib.lib.die_last_error(), lib.lib.die_last_error()


@pytest.mark.parametrize('case, call, kw, needle', [
    ('mask: null dropout', _mask, dict(drop=False), b'null argument'),
    ('mask: null output', _mask, dict(out=None), b'null argument'),
    ('mask: no replica', _mask, dict(replicas=0), b'replicas'),
    ('mask: 65 replicas', _mask, dict(replicas=65), b'replicas'),
    ('mask: stride below a plane', _mask, dict(plane_stride=63), b'plane_stride'),
    ('mask: negative stride', _mask, dict(plane_stride=-64), b'plane_stride'),
    ('mask: empty plane', _mask, dict(W=0), b'bad size'),
    ('mask: reserved word set', _mask, dict(reserved=1), b'reserved'),
    ('conv2d: null input planes', _conv, dict(null='planes'), b'null argument'),
    ('conv2d: null output planes', _conv, dict(null='outs'), b'null argument'),
    ('conv2d: null weights', _conv, dict(null='w'), b'null argument'),
    ('step: null medium', _step, dict(null='m'), b'null argument'),
    ('step: null stack', _step, dict(null='nca'), b'null argument'),
    ('step: null results', _step, dict(null='results'), b'null argument'),
    ('step: null workspace', _step, dict(null='ws'), b'null argument'),
    ('step: no replica', _step, dict(replicas=0), b'replicas'),
    ('step: 65 replicas', _step, dict(replicas=65), b'replicas'),
    ('step: reserved word set', _step, dict(reserved=7), b'reserved'),
])
def test_bad_arguments_refused_before_launch(lib, case, call, kw, needle):
    assert call(lib, **kw) == -1, case
    assert needle in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


# (key, forward call, cell, word): computed with a Philox4x32-10 written on Python integers, apart from oracle/rng.py's
KNOWN_WORDS = [
    (0x0, 0x0, 0x0, 0xE04EF820),
    (0x0, 0x0, 0x1, 0x74728AA9),
    (0x0, 0x0, 0x2, 0xF465079F),
    (0x0, 0x0, 0x3, 0x83EA5F06),
    (0x0, 0x0, 0x4, 0x41CE19DB),                                     # the next block
    (0x1, 0x0, 0x0, 0xB0E48DFC),
    (0x0, 0x1, 0x0, 0x2D0C9C23),
    (0x7, 0x21, 0x23FF, 0xC799897B),                                 # the last cell of 96 x 96
    (0x123456789ABCDEF0, 0xFFFFFFFF, 0x23FF, 0x17761BDB),            # both key words, the largest counter
    (0x5, 0x2, 0x3FFFFFFFF, 0x5989E206),                             # block 2^32 - 1: the last with a zero high word
    (0x5, 0x2, 0x400000000, 0x80225FE1),                             # cell 2^34: block 2^32 = (lo 0, hi 1)
    (0x5, 0x2, 0x400000005, 0x68C81041),
    (0xFFFFFFFFFFFFFFFF, 0x7, 0x10000000002, 0x62D11AFF),
]


def test_twin_words_known_answers():
    for seed, step, cell, want in KNOWN_WORDS:
        assert int(M.words(seed, step, [cell])[0]) == want, (hex(seed), step, hex(cell))
    # the four words of a block are the four cells 4b … 4b + 3, and a plane is the row-major run of its cells
    assert M.words(0, 0, np.arange(5)).tolist() == [w for *_, w in KNOWN_WORDS[:5]]
    assert (M.dropped(0, 0, 1, 5, 0.5).ravel() == (np.array([w for *_, w in KNOWN_WORDS[:5]]) < 2 ** 31)).all()
    assert int(M.words(7, 33, [96 * 96 - 1])[0]) == 0xC799897B


def test_threshold_and_keep_rounding():
    assert M.threshold(1.0) == 2 ** 32 and M.threshold(0.25) == 2 ** 30 and M.threshold(0.5) == 2 ** 31
    assert M.threshold(2.0 ** -32) == 1 and M.threshold(2.0 ** -33) == 1 and M.threshold(2.0 ** -32 * 1.5) == 2
    assert M.threshold(0.1) == math.ceil(0.1 * 4294967296.0) == 429496730
    for bad in (0.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError):
            M.threshold(bad)
    assert M.keep_factor(0.25) == np.float32(4.0 / 3.0) and M.keep_factor(0.5) == np.float32(2.0)
    # p = 1 drops every cell (no word reaches 2^32) and the mask is 0, not NaN
    assert M.dropped(3, 1, 17, 23, 1.0).all() and (M.mask(3, 1, 17, 23, 1.0) == 0).all()
    # p = 2^-32: only a word of exactly 0 is dropped
    w = M.words(9, 4, np.arange(30 * 50))
    assert np.array_equal(M.dropped(9, 4, 30, 50, 2.0 ** -32).ravel(), w == 0)
    # p = 0.25 exactly: dropped iff the word's top two bits are 00
    assert np.array_equal(M.dropped(9, 4, 30, 50, 0.25).ravel(), (w >> 30) == 0)
    m = M.mask(9, 4, 30, 50, 0.25)
    assert m.dtype == np.float32 and set(np.unique(m).tolist()) == {0.0, float(np.float32(4.0 / 3.0))}


@pytest.mark.parametrize('p', [0.25, 0.5])
@pytest.mark.parametrize('seed', [1, 2, 3])
@pytest.mark.parametrize('step', [0, 3])
def test_dropped_fraction(p, seed, step):
    n = 96 * 96
    got = M.dropped(seed, step, 96, 96, p).mean()
    assert abs(got - p) < 5.0 * math.sqrt(p * (1.0 - p) / n), (got, p)


def test_what_changes_the_mask():
    W, H, p = 96, 96, 0.25
    base = M.mask(11, 5, W, H, p)
    assert np.array_equal(base, M.mask(11, 5, W, H, p))
    assert not np.array_equal(base, M.mask(11, 6, W, H, p))              # another forward call
    assert not np.array_equal(base, M.mask(12, 5, W, H, p))              # another key
    assert not np.array_equal(base, M.mask(11 + 2 ** 32, 5, W, H, p))    # the key's high word counts
    assert np.array_equal(base, M.mask(11 + 2 ** 64, 5, W, H, p))        # keys are taken mod 2^64
    assert np.array_equal(base, M.mask(11, 5 + 2 ** 32, W, H, p))        # the counter mod 2^32
    same = M.replica_masks(11, 0, 5, 3, W, H, p)                         # stride 0: one mask for every replica
    assert all(np.array_equal(same[r], base) for r in range(3))
    one = M.replica_masks(11, 1, 5, 3, W, H, p)
    assert np.array_equal(one[0], base) and np.array_equal(one[1], M.mask(12, 5, W, H, p))
    assert not np.array_equal(one[1], one[0]) and not np.array_equal(one[2], one[1])
    two = M.replica_masks(11, 2, 5, 3, W, H, p)
    assert np.array_equal(two[1], one[2]) and not np.array_equal(two[2], one[2])
    # the mask of a plane does not depend on its shape beyond the cell index ix·H + iy
    assert np.array_equal(M.mask(11, 5, 48, 192, p).ravel(), base.ravel())


def test_stand_alone_agent_keeps_the_seed_out_of_saved_arguments_unless_set(lib):
    import io
    import torch
    from die_amd import NeuralAutomataAgent
    from die_amd.batch import BatchedNeuralAutomataAgent as B
    plain = NeuralAutomataAgent(kernel_sizes=(3,), p_agent_dropout=0.25)
    assert plain.dropout_seed is None and plain.dropout_step == 0 and 'dropout_seed' not in plain.init_params
    seeded = NeuralAutomataAgent(kernel_sizes=(3,), p_agent_dropout=0.25, dropout_seed=9)
    assert seeded.dropout_seed == 9 and seeded.init_params['dropout_seed'] == 9
    buf = io.BytesIO()
    seeded.save(buf)
    buf.seek(0)
    back = NeuralAutomataAgent.load(buf)
    assert back.dropout_seed == 9 and back.model.agent_dropout.p == 0.25
    for q, r in zip(back.model.parameters(), seeded.model.parameters()):
        assert torch.equal(q, r)
    seeded.dropout_seed = None                                    # back to the torch-RNG mask: the key leaves the saved arguments
    assert 'dropout_seed' not in seeded.init_params
    with pytest.raises(ValueError):
        NeuralAutomataAgent(dropout_seed=1.5)
    row = torch.nn.utils.parameters_to_vector(plain.model.parameters()).detach()
    assert B.unpack(plain, row).dropout_seed is None              # unpack hands the template's own key on, or the one given
    assert B.unpack(back, row).dropout_seed == 9 and B.unpack(back, row, dropout_seed=12).dropout_seed == 12
    assert B.unpack(plain, row, dropout_seed=12).init_params['dropout_seed'] == 12
