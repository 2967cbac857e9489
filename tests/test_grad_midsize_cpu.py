"""The premises of the mid-size tests of the differentiable paths (the full-block tests of tests/test_gpu_field_step_grad.py and
tests/test_gpu_batch_field_step_grad.py, tests/test_gpu_grad_midsize.py), checked without a GPU.  Every size there was chosen to
reach one size-dependent branch of a kernel, and the branch points are constants of the sources: they are read from the sources
here and every premise is recomputed from them, so a changed constant fails here instead of leaving a GPU test that quietly no
longer reaches its branch.  Also here: the gather's index arithmetic restated in numpy (with the mutations that may not run on a
GPU), the loop-free winners' rule against the oracle-based one, the torch float64 reference against the numpy models at their own
small shapes, and a plain fp32 evaluation of every conv-adjoint case against the reference (the yardstick of the device's
ceiling)."""
import os
import re

import numpy as np
import pytest

from tests import conv_adjoint_model as A
from tests import field_step_adjoint_model as F
from tests import grad_midsize_model as GM
from tests import grad_midsize_shapes as S
from tests import nca_wide_grad_model as G
from tests.test_batch_midsize_cpu import CSRC, _define, _pic_min_cells, _rpw, _source
from tests.test_batch_midsize_cpu import K as K_env                                    # noqa: F401  (the fixture of die_env.hip's constants)

YARDSTICK = 1e-5


@pytest.fixture(scope='module')
def K(K_env):
    """The constants the sizes were chosen against, as the sources state them today."""
    k = dict(K_env)
    env_grad, nca_grad, nca_h = _source('die_env_grad.hip'), _source('die_nca_grad.hip'), _source('die_nca.h')
    k['GATHER_PER_THREAD'] = _define(env_grad, 'GATHER_PER_THREAD')
    k.update({name: _define(nca_h, name) for name in ('NCA_TX', 'NCA_TY')})
    # the capped grids: every launch of the two files caps its workgroups with the literal `g < 8192 ? g : 8192`
    k['ENV_GRAD_CAPS'] = [int(v) for v in re.findall(r'g < (\d+) \? g : \1', env_grad)]
    k['NCA_GRAD_CAPS'] = [int(v) for v in re.findall(r'g < (\d+) \? g : \1', nca_grad)]
    # the gather's runs: n = base + q * DIE_BLOCK, a workgroup's base blockIdx.x * DIE_BLOCK * GATHER_PER_THREAD + threadIdx.x
    assert len(re.findall(r'const int64_t n = base \+ \(int64_t\)q \* DIE_BLOCK;', env_grad)) == 4
    assert len(re.findall(r'base = \(int64_t\)blockIdx\.x \* DIE_BLOCK \* GATHER_PER_THREAD \+ threadIdx\.x', env_grad)) == 2
    assert len(re.findall(r'stride = \(int64_t\)gridDim\.x \* DIE_BLOCK \* GATHER_PER_THREAD;', env_grad)) == 2
    # the fold of the conv adjoints' partial rows
    m = re.search(r'void conv_backward_sum_one\(.*?\{\s*double s = 0\.0;\s*#pragma unroll (\d+)\s*for \(int64_t t = 0; t < rows; \+\+t\)', nca_grad, re.S)
    assert m, 'conv_backward_sum_one not found'
    k['FOLD_UNROLL'] = int(m.group(1))
    assert '((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * nw' in nca_grad                     # the partial row of a tile
    assert '((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * nw' in _source('die_nca_wide_grad.hip')
    # the default re-sort
    text = open(os.path.join(os.path.dirname(CSRC), 'env.py')).read()
    m = re.search(r'^\s*SORT_MIN_CELLS = 1 << (\d+)', text, re.M)
    n = re.search(r'return (\d+) if int\(field_size\[0\]\) \* int\(field_size\[1\]\) >= cls\.SORT_MIN_CELLS else 0', text)
    assert m and n, 'the default re-sort of Env not found'
    k['SORT_MIN_CELLS'], k['SORT_EVERY'] = 1 << int(m.group(1)), int(n.group(1))
    return k


def test_the_constants_are_the_ones_the_sizes_were_chosen_for(K):
    assert (K['GATHER_PER_THREAD'], K['DIE_BLOCK'], K['NCA_TX'], K['NCA_TY'], K['DIF_WCOLS'], K['FOLD_UNROLL']) == (4, 256, 16, 64, 248, 8)
    assert K['ENV_GRAD_CAPS'] == [8192] * 4 and K['NCA_GRAD_CAPS'] == [8192] * 2       # deposit, gather, both batched; the two scatters
    assert K['rpw'] == [(1 << 23, 16), (1 << 21, 8), (1 << 19, 4), (0, 2)]
    assert (K['SORT_MIN_CELLS'], K['SORT_EVERY']) == (1 << 19, 8)


# ------------------------------------------------------------------------------------------------ 1. the gather
def gather_visits(K, N, total=None, grid=None, drop_q=False):
    """k_gather_cells' index arithmetic in numpy: the entries n a launch over `total` entries (N of them valid) stores to, as
    (n, whether it loads cells[n]).  `drop_q`: the mutation n = base (the q * DIE_BLOCK term dropped)."""
    B, Q = K['DIE_BLOCK'], K['GATHER_PER_THREAD']
    total = N if total is None else total
    groups = min(-(-total // (B * Q)), K['ENV_GRAD_CAPS'][1]) if grid is None else grid
    stride = groups * B * Q
    base = (np.arange(groups, dtype=np.int64)[:, None] * B * Q + np.arange(B)[None, :]).reshape(-1)
    out = []
    while base.size and base.min() < total:
        b = base[base < total]
        for q in range(Q):
            n = b + (0 if drop_q else q * B)
            n = n[n < total]
            out.append(n)
        base = base + stride
    n = np.concatenate(out)
    return n, n < N


@pytest.mark.parametrize('N', S.GATHER_NS)
def test_gather_sizes_reach_their_branches(K, N):
    B, Q, cap = K['DIE_BLOCK'], K['GATHER_PER_THREAD'], K['ENV_GRAD_CAPS'][1]
    per = B * Q
    assert per == 1024 and S.GATHER_NS == (255, 256, 257, 1023, 1024, 1025, 3077, 8389637)
    groups, trips = min(-(-N // per), cap), -(-N // (per * cap))
    runs = -(-N // B)                                               # runs of DIE_BLOCK entries that hold an entry
    want = {255: (1, 1, 1), 256: (1, 1, 1), 257: (1, 1, 2), 1023: (1, 1, 4), 1024: (1, 1, 4), 1025: (2, 1, 5), 3077: (4, 1, 13),
            8389637: (8192, 2, 32773)}[N]
    assert (groups, trips, runs) == want
    if N == 8389637:
        assert N - cap * per == per + 5                             # the second trip: workgroup 0 in full, five entries of workgroup 1
    # every entry is stored exactly once
    n, _ = gather_visits(K, N)
    assert n.size == N and np.array_equal(np.sort(n), np.arange(N))
    # the mutation "n = base": by reasoning only on the GPU (every store stays below N, so it changes values only — and the issue
    # allows one run; none was needed).  Restated here: entries from the second run on are never written, so the sentinel stays in
    # grad_deposit — every size but 255 and 256 fails, which no earlier test (N <= about 150) could
    n, _ = gather_visits(K, N, drop_q=True)
    missed = N - np.unique(n).size
    assert (missed > 0) == (N > B) and np.unique(n).max() < N
    # the cells the GPU test draws: about 30 % store +0, both ends of the array carry the special values
    g, cells = S.gather_case(N)
    out = (cells < 0) | (cells >= g.size)
    assert 0.25 * N < out.sum() < 0.4 * N
    assert {S.INT32_MIN, g.size, 2 ** 31 - 1, -1} <= set(cells[:7].tolist()) and {S.INT32_MIN, g.size, -1} <= set(cells[-7:].tolist())
    assert cells[0] == 0 and cells[1] == g.size - 1 and cells[-1] == 0 and cells[-2] == g.size - 1
    want = S.gather_want(g, cells)
    assert np.all(want[out].view(np.uint32) == 0) and np.array_equal(want[~out], g.reshape(-1)[cells[~out]])


def test_batched_gather_rows_end_inside_later_runs(K):
    B, Q = K['DIE_BLOCK'], K['GATHER_PER_THREAD']
    stride, n = S.GATHER_BATCH_STRIDE, S.GATHER_BATCH_N
    assert stride == 3 * B * Q + 5 and n == (stride, B * Q + 1, 0) and S.GATHER_PLANE[1] % 4 == 0
    # the launch is sized by agent_stride: four workgroups a row; row 1 ends one entry into workgroup 1's first run, so that
    # workgroup's runs 1 .. 3 and the whole of workgroups 2 and 3 only store the padding's +0
    at, loads = gather_visits(K, n[1], total=stride)
    assert at.size == stride and np.array_equal(np.sort(at), np.arange(stride)) and loads.sum() == n[1]
    first_padding = n[1]
    assert first_padding // (B * Q) == 1 and (first_padding % (B * Q)) // B == 0 and first_padding % B == 1
    at, loads = gather_visits(K, 0, total=stride)
    assert not loads.any() and at.size == stride
    # the cells: junk behind n[r] is a valid cell everywhere
    g, cells, junk = S.gather_batch_case()
    W, H = S.GATHER_PLANE
    for r in range(3):
        assert junk[r, n[r]:].all() and not junk[r, :n[r]].any()
        assert np.all((cells[r, n[r]:] >= 0) & (cells[r, n[r]:] < W * H))


# ------------------------------------------------------------------------------------------------ 2. the slot kernels
def test_slot_counts_pass_the_grid_caps(K):
    B, cap = K['DIE_BLOCK'], 8192
    assert S.SLOT_N == 2097665 > cap * B == 2097152 and S.SLOT_N - cap * B == 513
    assert S.DEPOSIT_BATCH_N == (S.SLOT_N, 65537, 300) and S.SCATTER_BATCH_N == (S.SLOT_N, 300)
    # the batched launches are sized by the stride (deposit) or the largest n[r] (scatter): the short rows end after 257 and 2 workgroups
    assert [-(-v // B) for v in S.DEPOSIT_BATCH_N] == [8195, 257, 2]
    W, H = S.SCATTER_PLANE
    assert (W, H) == S.ALONE_SHAPE and W * H < _pic_min_cells()


def test_loop_free_winners_are_the_oracle_rule():
    """grad_midsize_shapes.winner_cells against ref_cells_of (RefEnv's cells and alive index, the reference's fancy-index assignment)
    and against field_step_adjoint_model.deposit_cells, in slot order and permuted, on a crowded small world."""
    from tests.test_gpu_field_step_grad import ref_cells_of
    from tests import stock_plane_model as M
    W, H, N = 24, 68, 20000
    rs = np.random.RandomState(3)
    q32 = lambda v: np.floor(v * 2.0 ** 32) / 2.0 ** 32
    agents = np.stack([q32(rs.rand(N)), q32(rs.rand(N)), (rs.rand(N) < 0.5).astype(np.float64), np.ones(N)])
    medium = rs.rand(3, W, H)
    x, y = M.q32_words(agents[0]), M.q32_words(agents[1])
    want = ref_cells_of(medium, agents)
    got = S.winner_cells(W, H, x, y, agents[2])
    assert np.array_equal(got, want) and 0 < (want >= 0).sum() < (agents[2] > 0).sum() // 2      # most alive slots lose their cell
    assert np.array_equal(got, F.deposit_cells(M.cell(x, W), M.cell(y, H), agents[2], None, H))
    perm = rs.permutation(N)
    assert np.array_equal(S.winner_cells(W, H, x[perm], y[perm], agents[2][perm], perm), want[perm])


def test_scatter_world_has_both_kinds_of_cell():
    W, H = S.SCATTER_PLANE
    x, y, grads = S.scatter_world(W, H, S.SLOT_N, np.random.RandomState(31))
    total, mag, count = S.scatter_reference(W, H, x, y, grads, S.SCATTER_COEFS)
    assert (count == 1).sum() > 3 * W * H // 4 and (count > 1).sum() > 3 * W * H * 2 // 5 and count.max() >= 8
    # check_scatter on an fp32 sum in slot order (np.add.at in float32): it passes, and a sum that drops the last 513 slots (a
    # stride loop without its second trip) or takes them twice does not
    got = np.zeros((3, W * H), dtype=np.float32)
    terms = grads * np.asarray(S.SCATTER_COEFS, dtype=np.float32)[:, None]
    from tests import stock_plane_model as M
    where = M.cell(x, W) * H + M.cell(y, H)
    for q in range(3):
        np.add.at(got[q], where, terms[q])
    one, many, worst = S.check_scatter(got, total, mag, count)
    assert worst <= 1.0 and one == (count == 1).sum() and many == (count > 1).sum()
    for sign in (-1.0, 1.0):
        bad = got.copy()
        for q in range(3):
            np.add.at(bad[q], where[-513:], sign * terms[q][-513:])
        with pytest.raises(AssertionError):
            S.check_scatter(bad, total, mag, count)


# ------------------------------------------------------------------------------------------------ 3. the conv adjoints
def test_conv_fields_have_many_tiles(K):
    TX, TY, U = K['NCA_TX'], K['NCA_TY'], K['FOLD_UNROLL']
    tiles = {name: (-(-W // TX), -(-H // TY)) for name, (W, H) in S.CONV_FIELDS.items()}
    assert S.CONV_FIELDS == {'many_tiles': (514, 512), 'ragged': (130, 515)}
    assert tiles == {'many_tiles': (33, 8), 'ragged': (9, 9)}
    W, H = S.CONV_FIELDS['many_tiles']
    assert W % TX == 2 and H % TY == 0 and H % 4 == 0 and 33 * 8 == 264 and 264 % U == 0       # whole unrolled trips, a ragged tile row of 2 rows
    W, H = S.CONV_FIELDS['ragged']
    assert W % TX == 2 and H % TY == 3 and H % 4 != 0 and 81 % U == 1                            # unrolled trips and a remainder; scalar stores
    R, Wb, Hb = S.BATCH_SHAPE
    assert (Wb, Hb) == S.CONV_FIELDS['many_tiles'] and R == 2 and (2 * 264) % U == 0             # E = 2: one walk over 528 rows
    # the mutations that only change values, restated: folding rows & ~7 rows drops the 81st tile of the ragged field (its last
    # tile, the corner) and nothing on 264 tiles; blockIdx.x alone as the tile index writes 8 (9) of the rows, the rest stay NaN
    assert 81 & ~(U - 1) == 80 and 264 & ~(U - 1) == 264
    assert all(ty < tx * ty for tx, ty in tiles.values())


def test_worlds_reach_their_sweeps(K):
    R, W, H = S.BATCH_SHAPE
    assert (_rpw(K, R * W * H), _rpw(K, W * H)) == (4, 2) and H % 4 == 0 and W * H < _pic_min_cells()
    W, H = S.ALONE_SHAPE
    assert W * H >= K['SORT_MIN_CELLS'] and W * H < _pic_min_cells() and _rpw(K, W * H) == 4 and W % 4 == 0 and H % 4 == 0
    assert -(-H // K['DIF_WCOLS']) == 5                              # five strips a row
    # the default re-sort runs after every SORT_EVERY-th step: the whole-path test takes SORT_EVERY - 1 plain steps first, so that
    # its first differentiable step is the one that re-sorts and its second works on permuted arrays
    assert K['SORT_EVERY'] == 8


def test_torch_reference_is_the_numpy_model_at_the_models_own_shapes():
    for k, mode, cin, cout, W, H, act, masked in ((5, 'zeros', 17, 16, 33, 130, 'relu', True), (3, 'circular', 32, 32, 17, 66, 'tanh', True),
                                                  (3, 'circular', 3, 16, 20, 68, None, False)):
        c = G.case_inputs(k, mode, cin, cout, W, H)
        mask = G.case_mask(c, W, H, masked)
        t = None if act is None else G.act_forward(G.conv(c['x'], c['w'], mode), act).astype(np.float32)
        z, gw, gi = GM.reference(c['x'], c['w'], c['g'], t, act, mask, mode)
        mw, mi = G.layer_backward(c['x'], c['w'], c['g'], t, act, mask, mode)
        assert np.abs(z - G.conv(c['x'], c['w'], mode)).max() <= 1e-12 * np.abs(z).max()
        assert np.abs(gw - mw).max() <= 1e-12 * np.abs(mw).max() and np.abs(gi - mi).max() <= 1e-12 * np.abs(mi).max()
    # the narrow model's k = 7 and its tanh-and-mask adjoint
    c = A.case_inputs(7, 'circular', 4, 4, 33, 130)
    t = np.tanh(A.conv(c['x'], c['w'], 'circular')).astype(np.float32)
    mask = GM.D.mask(c['seed'], GM.DROP_STEP, 33, 130, GM.DROP_P)
    _, gw, gi = GM.reference(c['x'], c['w'], c['g'], t, 'tanh', mask, 'circular')
    mw, mi = A.conv_backward(c['x'], c['w'], A.tanh_mask_adjoint(c['g'], t, mask), 'circular')
    assert np.abs(gw - mw).max() <= 1e-12 * np.abs(mw).max() and np.abs(gi - mi).max() <= 1e-12 * np.abs(mi).max()


@pytest.mark.parametrize('name', list(GM.WIDE_CASES) + list(GM.NARROW_CASES))
def test_fp32_evaluation_of_every_midsize_case_stays_within_the_yardstick(name):
    c = GM.WIDE_CASES.get(name) or GM.NARROW_CASES[name]
    inp = GM.case_inputs(c)
    mask = GM.case_mask(c, inp)
    t32, gw32, gi32 = GM.fp32_evaluation(inp['x'], inp['w'], inp['g'], c['act'], mask, c['mode'])
    _, gw, gi = GM.reference(inp['x'], inp['w'], inp['g'], t32, c['act'], mask, c['mode'])
    errs = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in ((gw32, gw), (gi32, gi))]
    print(f'mid-size conv adjoint fp32 yardstick {name}: grad_w {errs[0]:.2e}  grad_in {errs[1]:.2e}  (of max|f64| per array; ceiling {YARDSTICK:.0e})')
    assert max(errs) <= YARDSTICK, errs
    if c['masked']:
        assert 0.15 < (mask == 0).mean() < 0.35
    if c['act'] == 'relu':
        assert 0.1 < (t32 > 0).mean() < 0.9
