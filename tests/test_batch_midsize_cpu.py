"""The premises of the mid-size batched tests (tests/test_gpu_batch_midsize.py, the large-n tests of tests/test_gpu_births.py and
tests/test_gpu_stock.py), checked without a GPU: every shape there was chosen to reach one size-dependent branch of the kernels,
and the branch points are constants of the sources.  The constants are read from the sources here, the table of shapes is
recomputed from them, and the numpy models are run once at the large n: a changed constant or pattern fails here instead of
leaving a GPU test that quietly no longer reaches its branch."""
import os
import re

import numpy as np
import pytest

from tests import births_model, stock_plane_model
from tests.midsize_shapes import BIRTH_BATCH_NS, BIRTH_NS, BIRTH_PATTERNS, SHAPES, STOCK_BATCH_N, STOCK_N, STOCK_PLANE, stock_plane_fast, \
    stock_winners_fast, stock_world

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'die_amd', 'csrc')


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(text, name):
    m = re.search(rf'^\s*#define\s+{name}\s+(\d+)\b', text, re.M)
    assert m, f'#define {name} not found'
    return int(m.group(1))


@pytest.fixture(scope='module')
def K():
    """The constants the shapes were chosen against, as the sources state them today."""
    env, births, common = _source('die_env.hip'), _source('die_births.hip'), _source('die_common.h')
    k = {name: _define(env, name) for name in ('DIE_STEP_BLOCK', 'DIE_STEP_GRID_CAP', 'DIF_ROWS', 'DIF_WCOLS', 'DIF_BLOCK', 'DIE_MAX_PARTIALS')}
    k.update({name: _define(births, name) for name in ('BIRTH_BLOCK', 'BIRTH_MAX_GROUPS')})
    k.update({name: _define(common, name) for name in ('DIE_BLOCK', 'DIE_WAVE')})
    # rows_per_wave: cells >= (1ll << 23) ? DIF_ROWS : cells >= (1ll << 21) ? 8 : cells >= (1ll << 19) ? 4 : 2
    body = re.search(r'static int rows_per_wave\(int W, int H, int replicas\) \{(.*?)\n\}', env, re.S)
    assert body, 'rows_per_wave not found'
    assert re.search(r'cells = \(int64_t\)W \* H \* replicas;', body.group(1)), 'rows_per_wave no longer counts W·H·replicas cells'
    steps = re.findall(r'cells >= \(1ll << (\d+)\) \? (\w+)', body.group(1))
    last = re.search(r': (\d+);', body.group(1))
    assert len(steps) == 3 and last, body.group(1)
    k['rpw'] = [(1 << int(sh), k[v] if v in k else int(v)) for sh, v in steps] + [(0, int(last.group(1)))]
    # the spawn grid's cap and the 8192-workgroup caps of the slot kernels are literals
    m = re.search(r'half < (\d+) \? half : \1', births)
    assert m, 'k_births_spawn grid cap not found'
    k['SPAWN_GROUPS'] = int(m.group(1))
    m = re.search(r'g < (\d+) \? g : \1', _source('die_stock.hip'))
    assert m, 'k_stock_plane grid cap not found'
    k['STOCK_GROUPS'] = int(m.group(1))
    m = re.search(r'static int init_grid\(int64_t n\) \{.*?g < (\d+) \?', _source('die_init.hip'), re.S)
    assert m, 'init_grid cap not found'
    k['INIT_GROUPS'] = int(m.group(1))
    # the reduction row's walk: eight partials in flight per thread of a DIF_BLOCK workgroup
    m = re.search(r'base < a\.n_part; base \+= DIF_BLOCK \* (\d+)\)', env)
    assert m, 'strided_sum not found'
    k['IN_FLIGHT'] = int(m.group(1))
    return k


def _rpw(k, cells):
    return next(v for lo, v in k['rpw'] if cells >= lo)


def _pic_min_cells():
    """Env.PIC_MIN_CELLS without importing the package's device half: the class attribute as die_amd/env.py writes it."""
    text = open(os.path.join(os.path.dirname(CSRC), 'env.py')).read()
    m = re.search(r'^\s*PIC_MIN_CELLS = 1 << (\d+)', text, re.M)
    assert m
    return 1 << int(m.group(1))


def test_the_thresholds_are_the_ones_the_shapes_were_chosen_for(K):
    assert K['rpw'] == [(1 << 23, 16), (1 << 21, 8), (1 << 19, 4), (0, 2)] and K['DIF_ROWS'] == 16
    assert (K['DIE_STEP_BLOCK'], K['DIE_STEP_GRID_CAP'], K['DIF_WCOLS'], K['DIF_BLOCK']) == (320, 8192, 248, 128)
    assert (K['BIRTH_BLOCK'], K['BIRTH_MAX_GROUPS'], K['SPAWN_GROUPS']) == (256, 512, 4096)
    assert K['DIE_STEP_GRID_CAP'] <= K['DIE_MAX_PARTIALS']
    assert (K['STOCK_GROUPS'], K['INIT_GROUPS'], K['DIE_BLOCK'], K['IN_FLIGHT']) == (8192, 8192, 256, 8)


# name: (batch rpw, twin rpw, n_part) as the issue's table states them
TABLE = {'S': (4, 2, 823), 'M': (8, 4, 3290), 'L': (16, 8, 8192)}


@pytest.mark.parametrize('name', list(SHAPES))
def test_shape_reaches_its_branches(K, name):
    R, W, H = SHAPES[name]
    batch, twin, n_part = TABLE[name]
    assert W * H < _pic_min_cells()                                # the batched regime, unforced
    rpw, rpw_alone = _rpw(K, R * W * H), _rpw(K, W * H)
    assert (rpw, rpw_alone) == (batch, twin) and rpw != rpw_alone  # the batch sweeps with another value than a replica's twin
    assert W % rpw == {'S': 2, 'M': 4, 'L': 12}[name]              # a partial last wave in the batch
    assert H % 4 == 0                                              # rows_kernel_applies
    assert H > K['DIF_WCOLS']                                      # more than one strip per row
    waves = K['DIF_BLOCK'] // K['DIE_WAVE']
    assert H > waves * K['DIF_WCOLS'] and waves * K['DIF_WCOLS'] == 496    # … and more than one workgroup in x
    slots = W * H                                                  # max_agents=None
    got = min(-(-slots // K['DIE_STEP_BLOCK']), K['DIE_STEP_GRID_CAP'])
    assert got == n_part
    assert n_part > K['DIF_BLOCK']                                 # strided_sum: the 2nd … slots of v[q]
    if name in ('M', 'L'):
        assert n_part > K['DIF_BLOCK'] * K['IN_FLIGHT']            # a second trip of the `base` loop
    if name == 'L':
        assert slots > K['DIE_STEP_GRID_CAP'] * K['DIE_STEP_BLOCK'] == 2621440       # claim / lifecycle kernels stride
        assert slots > K['STOCK_GROUPS'] * K['DIE_BLOCK'] == 2097152                 # k_stock_plane, k_gather_scale_batch, init_grid
        assert slots > K['INIT_GROUPS'] * K['DIE_BLOCK']
        assert R * 1672 * 1672 == (1 << 23) - 1856                 # why L is 1676 wide, not 1672
    assert -(-slots // K['BIRTH_BLOCK']) > K['BIRTH_MAX_GROUPS']   # Dynamics.agents_born on any of them: several chunks a workgroup


def test_births_sizes_reach_their_branches(K):
    B, G = K['BIRTH_BLOCK'], K['BIRTH_MAX_GROUPS']
    chunks = [-(-n // B) for n in BIRTH_NS]
    assert BIRTH_NS == (65537, 131073, 262145, 2097665)
    assert chunks[0] > 256 and chunks[0] <= G                      # k_births_rank's sum over the workgroups: a second trip
    assert chunks[1] == G + 1                                      # one chunk past the cap: per = 2, the trailing workgroups get nothing
    per = -(-chunks[1] // G)
    assert per == 2 and (G - 1) * per * B > BIRTH_NS[1]            # (the last workgroup's range is empty)
    assert all(c > G for c in chunks[1:])
    assert BIRTH_NS[3] // 2 > K['SPAWN_GROUPS'] * B == 1048576     # the spawn loop can stride
    assert BIRTH_BATCH_NS == (131073, 65537, 300) and max(BIRTH_BATCH_NS) == BIRTH_BATCH_NS[0]


def test_the_births_model_at_the_large_sizes_gives_what_the_gpu_tests_rely_on(K):
    n = BIRTH_NS[-1]
    rs = np.random.RandomState(100 + n)
    from tests.test_gpu_births import _patterns                    # (the patterns the GPU test draws, from the same generator state)
    pats = _patterns(n, rs)
    assert set(BIRTH_PATTERNS) <= set(pats)
    for name in BIRTH_PATTERNS:
        alive, food = pats[name]
        x = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        y = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        *_, wa, wf, born = births_model.births(x, y, alive, food, world_seed=5, world_step=3, born_spread=0.3, boundary=births_model.LIMIT)
        assert born > 0 and int(wa.sum()) == int(alive.sum()) + born, name
        if name == 'equal counts':
            assert born == 1048832 > K['SPAWN_GROUPS'] * K['BIRTH_BLOCK']          # the spawn loop does stride
        if name == 'more parents than free':
            assert born == int((alive == 0).sum())                                 # every free slot is taken
        if name == 'free slots before the parents':
            parents, free = births_model.match(alive, food, 0.5)
            assert free.max() < parents.min()                                      # the first workgroups hold no parent, the last no free slot


def test_the_stock_world_has_shared_cells(K):
    W, H = STOCK_PLANE
    assert STOCK_N > K['STOCK_GROUPS'] * K['DIE_BLOCK'] and STOCK_BATCH_N == (STOCK_N, 300)
    x, y, alive, food = stock_world(W, H, STOCK_N, np.random.RandomState(1))
    n_alive = int(alive.sum())
    assert 0.4 * STOCK_N < n_alive < 0.6 * STOCK_N                 # about half the slots are alive
    cells = stock_plane_model.cell(x, W)[alive > 0] * H + stock_plane_model.cell(y, H)[alive > 0]
    counts = np.bincount(cells, minlength=W * H)
    assert (counts > 1).sum() > W * H // 2                         # most cells are shared: the highest slot id must win
    # the loop-free winners the GPU test compares with ARE the model's (its Python loop over 2 M slots runs here, once)
    occ, slot = stock_plane_model.stock_winners(W, H, x, y, alive)
    occ2, slot2 = stock_winners_fast(W, H, x, y, alive)
    assert np.array_equal(occ, occ2) and np.array_equal(slot, slot2)
    want = np.zeros((W, H), dtype=np.float32)
    want[occ] = food[slot[occ]]
    assert np.array_equal(stock_plane_fast(W, H, x, y, alive, food).view(np.uint32), want.view(np.uint32))
    assert occ.all()                                               # every cell occupied: the GPU test expects a word on each
