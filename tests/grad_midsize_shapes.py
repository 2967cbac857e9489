"""TEST INFRASTRUCTURE ONLY: the shapes and sizes of the mid-size tests of the differentiable paths, in one place for the GPU tests
that run them (the full-block tests of tests/test_gpu_field_step_grad.py and tests/test_gpu_batch_field_step_grad.py,
tests/test_gpu_grad_midsize.py) and for the CPU module that recomputes why each was chosen (tests/test_grad_midsize_cpu.py).
numpy only."""
import numpy as np

from tests import stock_plane_model as M
from tests.midsize_shapes import SHAPES, STOCK_N

INT32_MIN = -2 ** 31

# k_gather_cells / k_gather_cells_batch: a workgroup takes GATHER_PER_THREAD = 4 runs of DIE_BLOCK = 256 entries.  One run short of
# full, full, one entry into the second run; one workgroup short of full, full, one entry into the second workgroup; four workgroups,
# the last with five entries; and one entry count past the 8192-workgroup cap whose second trip fills workgroup 0 and starts workgroup 1.
GATHER_NS = (255, 256, 257, 1023, 1024, 1025, 3 * 1024 + 5, 8192 * 1024 + 1029)
GATHER_PLANE = (24, 68)                                    # (W, H) of the gradient plane the gathers read; H % 4 == 0: the row sweep
GATHER_BATCH_STRIDE = 3 * 1024 + 5
GATHER_BATCH_N = (3 * 1024 + 5, 1025, 0)                   # n[1] ends inside workgroup 1's first run; replica 2 is padding only

# k_deposit_cells(_batch), k_gather_scale_backward(_batch): more slots than the grid's 8192 x 256 threads
SLOT_N = STOCK_N                                           # 2 097 665
DEPOSIT_PLANE = (256, 256)                                 # a million alive slots on 65 536 cells: nearly every cell is shared
DEPOSIT_BATCH_N = (SLOT_N, 65537, 300)
SCATTER_PLANE = (1028, 1024)                               # two slots a cell on average: cells with one contributor and with several
SCATTER_BATCH_N = (SLOT_N, 300)
SCATTER_COEFS = (0.3, 0.25, 1.7)                           # (no powers of two only: the fp32 product rounds)

# the conv adjoints' partial rows: name -> (W, H)
CONV_FIELDS = {'many_tiles': (514, 512), 'ragged': (130, 515)}

# whole paths: the batch shape S of tests/midsize_shapes.py and one stand-alone world large enough for the default re-sort
BATCH_SHAPE = SHAPES['S']                                  # (2, 514, 512)
ALONE_SHAPE = (1028, 1024)


def gather_cells(n_cells, N, rs):
    """int32 (N,): random cells of a plane of n_cells, about 30 % of them -1; at both ends of the array (the first run of the first
    workgroup, the last run of the last): both ends of the plane, a loser, one index at the plane's end, one far beyond it and
    INT32_MIN — the last three must store +0."""
    cells = rs.randint(0, n_cells, N).astype(np.int32)
    cells[rs.rand(N) < 0.3] = -1
    special = np.array([0, n_cells - 1, -1, n_cells, 2 ** 31 - 1, INT32_MIN, 7], dtype=np.int64).astype(np.int32)
    cells[:special.size] = special
    cells[-special.size:] = special[::-1]
    return cells


def gather_case(N):
    """(grad_chem_next (W, H) float32, cells int32 (N,)) of the stand-alone gather test at N entries."""
    W, H = GATHER_PLANE
    rs = np.random.RandomState(N % (2 ** 31))
    return rs.standard_normal((W, H)).astype(np.float32), gather_cells(W * H, N, rs)


def gather_batch_case():
    """(grad_chem_next (R, W, H) float32, cells int32 (R, stride), junk bool (R, stride)) of the batched gather test: row r holds
    gather_cells of n[r] entries, and behind them junk that is a valid cell of the plane — read as an index it would fetch a
    gradient, and the padding must be +0."""
    (W, H), n, stride = GATHER_PLANE, GATHER_BATCH_N, GATHER_BATCH_STRIDE
    rs = np.random.RandomState(stride)
    g = rs.standard_normal((len(n), W, H)).astype(np.float32)
    cells = rs.randint(0, W * H, (len(n), stride)).astype(np.int32)
    junk = np.ones(cells.shape, dtype=bool)
    for r, k in enumerate(n):
        if k:
            cells[r, :k] = gather_cells(W * H, k, rs)
        junk[r, :k] = False
    return g, cells, junk


def gather_want(plane, cells):
    """where(0 <= cells < plane.size, plane[cells], +0): the gather on the host, word for word (float32 in, float32 out)."""
    plane = np.asarray(plane, dtype=np.float32).reshape(-1)
    c = np.asarray(cells).astype(np.int64)
    ok = (c >= 0) & (c < plane.size)
    return np.where(ok, plane[np.where(ok, c, 0)], np.float32(0)).astype(np.float32)


def winner_cells(W, H, x, y, alive, slot=None):
    """die_deposit_cells on the host without a loop: entry n's cell cx * H + cy if it is alive and no alive entry with a larger slot
    id stands there, else -1.  x, y: uint32 Q0.32 words, array order; slot: the entries' slot ids (None = array order is slot order).
    tests/test_grad_midsize_cpu.py checks it against the oracle-based rule of tests/test_gpu_field_step_grad.py."""
    N = len(x)
    slot = np.arange(N, dtype=np.int64) if slot is None else np.asarray(slot, dtype=np.int64)
    where = M.cell(x, W) * H + M.cell(y, H)
    idx = np.flatnonzero(np.asarray(alive) != 0)
    best = np.full(W * H, -1, dtype=np.int64)
    np.maximum.at(best, where[idx], slot[idx])
    won = (np.asarray(alive) != 0) & (best[where] == slot)
    return np.where(won, where, -1).astype(np.int32)


def scatter_world(W, H, N, rs):
    """(x, y uint32 words, grads float32 (3, N)) of N slots: uniform over the plane, a fifth of the gradient entries exactly 0."""
    x = rs.randint(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    y = rs.randint(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    grads = rs.standard_normal((3, N)).astype(np.float32)
    grads[rs.rand(3, N) < 0.2] = 0.0
    return x, y, grads


def scatter_reference(W, H, x, y, grads, coefs):
    """die_gather_scale_backward in float64 over the fp32 products the device forms exactly: (sum (3, W*H) float64, sum of |terms|
    float64, count of non-zero terms int64, the fp32 sum where a cell has exactly one non-zero term)."""
    where = M.cell(x, W) * H + M.cell(y, H)
    terms = np.asarray(grads, dtype=np.float32) * np.asarray(coefs, dtype=np.float32)[:, None]
    assert terms.dtype == np.float32
    total, mag = np.zeros((3, W * H)), np.zeros((3, W * H))
    count = np.zeros((3, W * H), dtype=np.int64)
    for q in range(3):
        np.add.at(total[q], where, terms[q].astype(np.float64))
        np.add.at(mag[q], where, np.abs(terms[q]).astype(np.float64))
        np.add.at(count[q], where, (terms[q] != 0).astype(np.int64))
    return total, mag, count


def check_scatter(got, total, mag, count, what=''):
    """A (3, W*H) float32 device result against scatter_reference: no contributor -> +0, one -> the term's bits, n -> within
    (n - 1) * 2^-24 * sum|terms| (Rump 2012: recursive fp32 summation of n terms in ANY order errs by at most (n - 1) u sum|t|, u =
    2^-24, no higher-order term) — derived, not measured: the atomics fix no order.  Returns (cells with one term, with several,
    worst error over its bound)."""
    got = np.asarray(got, dtype=np.float32).reshape(3, -1)
    none, one, many = count == 0, count == 1, count > 1
    assert np.all(got[none].view(np.uint32) == 0), (what, 'a cell without a contributor is not +0')
    assert np.array_equal(got[one], total[one].astype(np.float32)) and np.array_equal(got[one].astype(np.float64), total[one]), \
        (what, 'a cell with one contributor does not hold its term')
    bound = (count[many] - 1) * 2.0 ** -24 * mag[many]
    err = np.abs(got[many].astype(np.float64) - total[many])
    worst = float((err / bound).max()) if err.size else 0.0
    assert np.all(err <= bound), (what, 'beyond the summation bound', worst)
    return int(one.sum()), int(many.sum()), worst
