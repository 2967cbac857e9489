"""The counting-sort model of the agent sort and the tile binning (tests/reorder_model.py), CPU side: the model against brute
force, the checkers against outputs broken in one place, the case tables against the two host formulas, and the argument checks of
die_sort_workspace_bytes / die_agents_sort / die_pic_bin / die_pic_bin_momentum through the C ABI (fake device pointers: every call
is refused on the host, a launch would have failed).  No kernel is launched."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import reorder_model as M
from tests.reorder_model import Geo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20                       # never dereferenced
ARG, UNSUPPORTED = -1, -3


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


# ---------------------------------------------------------------- ideal outputs (what a correct device pass may write)
def _guard(values):
    v = M.bits(values)
    buf = M.guarded(len(v), v.dtype.itemsize)
    buf[M.GUARD:M.GUARD + len(v)] = v
    return buf


def ideal_sort(inp, geo, order=None):
    """A correct output: entries in the order `order` (default: stable by key)."""
    N = len(inp['x'])
    if order is None:
        order = np.argsort(M.sort_key(inp['x'], inp['y'], geo), kind='stable')
    ids = M._ids(inp, N)
    return dict(x=_guard(inp['x'][order]), y=_guard(inp['y'][order]), alive=_guard(inp['alive'][order]),
                agent_food=_guard(inp['agent_food'][order]), slot=_guard(ids[order]), extra=[_guard(e[order]) for e in inp['extra']])


def ideal_bin(inp, geo, tile, n_alive, rs=None):
    """A correct layout and its tables; `rs`: shuffle inside every segment and among the dead (the order there is free)."""
    N = len(inp['x'])
    mask, key, count = M.bin_tables(inp, geo, tile, n_alive)
    k = np.where(mask, key, len(count)).astype(np.float64)
    if rs is not None:
        k = k + rs.rand(N) * 0.5
    order = np.argsort(k, kind='stable')
    names = ['x', 'y', 'agent_food', 'heading_hi', 'heading_lo'] + (['prev_gx', 'prev_gy'] if inp['prev_gx'] is not None else [])
    lay = {n: _guard(inp[n][order]) for n in names}
    lay['slot'] = _guard(M._ids(inp, N)[order])
    meta = lambda: dict(off=_guard((np.cumsum(count) - count).astype(np.uint32)), n=_guard(count.astype(np.uint32)),
                        s=_guard(count.astype(np.uint32)), inc=_guard(np.zeros(len(count), dtype=np.uint32)))
    return lay, meta(), meta()


# ---------------------------------------------------------------- the model against brute force
def _cell_exact(X, n):
    """floor(X (n - 1) / 2**32 + 1/2) in Python integers."""
    return (2 * int(X) * (n - 1) + 2 ** 32) // 2 ** 33


@pytest.mark.parametrize('geo', [Geo(1, 1), Geo(15, 31), Geo(16, 32), Geo(40, 70), Geo(33, 65), Geo(80, 96, 256, 256, -11, 187),
                                 Geo(80, 96, 256, 256, 80, -11)], ids=str)
def test_sort_model_is_the_brute_force_bucket_sort(geo):
    N = 400
    inp = M.sort_inputs(geo, N, 2, True)
    gW, gH = M.world(geo)
    nby = (geo.H >> 5) + 1
    keys = []
    for X, Y in zip(inp['x'], inp['y']):
        ix = min(max(_cell_exact(X, gW) - (geo.ox if geo.gW else 0), 0), geo.W - 1)
        iy = min(max(_cell_exact(Y, gH) - (geo.oy if geo.gW else 0), 0), geo.H - 1)
        keys.append((ix // 16) * nby + iy // 32)
    assert keys == list(M.sort_key(inp['x'], inp['y'], geo))
    members = [[i for i in range(N) if keys[i] == b] for b in range(M.n_buckets(geo.W, geo.H))]     # per bucket, per agent
    assert sum(len(m) for m in members) == N
    order = np.array([i for m in members for i in reversed(m)], dtype=np.int64)                      # any order inside a bucket
    count = M.check_sort(inp, ideal_sort(inp, geo, order), geo)
    assert list(count) == [len(m) for m in members]
    M.check_sort(inp, ideal_sort(inp, geo), geo)


def test_cells_at_the_ends_of_the_coordinate_range():
    for n in (1, 2, 16, 300, 4096, 2 ** 21):
        X = np.array([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32)
        assert list(M.cells(X, n)) == [_cell_exact(v, n) for v in X]
        c = np.unique(np.r_[0, n // 2, n - 1])
        assert list(M.cells(M.coord_of_cell(c, n), n)) == list(c)
    rs = np.random.RandomState(0)
    X = M._u32(rs, 2000)
    assert list(M.cells(X, 2 ** 21)) == [_cell_exact(v, 2 ** 21) for v in X]


def _plane_coord_walk(c, o, n, gn):
    """Brute force: the plane element whose world cell is c, else the plane edge nearer on the world's circle (the last on a tie)."""
    for i in range(n):
        if (o + i) % gn == c:
            return i
    dist = lambda a, b: min((a - b) % gn, (b - a) % gn)
    first, last = o % gn, (o + n - 1) % gn
    return n - 1 if dist(c, last) <= dist(c, first) else 0


@pytest.mark.parametrize('n,gn', [(7, 24), (7, 25), (48, 112), (96, 208), (5, 5)])
def test_plane_coord_is_the_image_or_the_nearer_edge(n, gn):
    ties = 0
    for o in (-5, gn - n, n, 0, 3):
        want = [_plane_coord_walk(c, o, n, gn) for c in range(gn)]
        assert list(M.plane_coord(np.arange(gn), o, n, gn)) == want, (o, n, gn)
        first, last = o % gn, (o + n - 1) % gn
        ties += sum(1 for c in range(gn) if want[c] == n - 1 and (c - last) % gn == (first - c) % gn and (c - last) % gn > 0)
    assert (ties > 0) == ((gn - n) % 2 == 1 and gn > n)             # an odd gap has a middle cell: the tie rule is exercised


@pytest.mark.parametrize('ox', [-5, 64, 20])
@pytest.mark.parametrize('oy', [-5, 112, 20])
def test_decomposed_tile_key_over_every_cell_of_a_small_world(ox, oy):
    geo, tile = Geo(48, 96, 112, 208, ox, oy), (4, 5)
    rows = np.array([_plane_coord_walk(c, ox, 48, 112) for c in range(112)])
    cols = np.array([_plane_coord_walk(c, oy, 96, 208) for c in range(208)])
    cx, cy = np.meshgrid(np.arange(112), np.arange(208), indexing='ij')
    want = (rows[cx] >> 4) * (96 >> 5) + (cols[cy] >> 5)
    got = M.tile_key(M.coord_of_cell(cx.ravel(), 112), M.coord_of_cell(cy.ravel(), 208), geo, tile)
    assert np.array_equal(got, want.ravel())
    assert got.min() == 0 and got.max() == 8 and len(np.unique(got)) == 9
    # undivided: the cells themselves
    got = M.tile_key(M.coord_of_cell(cx.ravel(), 112), M.coord_of_cell(cy.ravel(), 208), Geo(112, 208), (4, 5))
    assert np.array_equal(got, ((cx >> 4) * (208 >> 5) + (cy >> 5)).ravel())


@pytest.mark.parametrize('form,crowd', M.BIN_VARIANTS)
def test_bin_model_is_the_brute_force_binning(form, crowd):
    geo, tile, N = Geo(48, 96), (4, 5), 700
    inp, n_alive = M.bin_inputs(geo, tile, N, form, crowd, True, True)
    alive = [True] * N if not 0 < n_alive < N else [bool(a) for a in inp['alive']]
    tile_of = [(_cell_exact(X, 48) // 16) * 3 + _cell_exact(Y, 96) // 32 for X, Y in zip(inp['x'], inp['y'])]
    members = [[i for i in range(N) if alive[i] and tile_of[i] == t] for t in range(9)]
    count = M.check_bin(inp, *ideal_bin(inp, geo, tile, n_alive, np.random.RandomState(1)), geo, tile, n_alive)
    assert list(count) == [len(m) for m in members] and sum(count) == (n_alive or N)
    if crowd == 'one_tile':
        assert sorted(set(tile_of)) == [5]
    if crowd == 'empty_row':
        assert list(count[3:6]) == [0, 0, 0] and (count[:3] > 0).all() and (count[6:] > 0).all()
    assert {'alive_null': inp['alive'] is None and n_alive == 0, 'all_alive': n_alive == N and inp['alive'].all(),
            'dead_85': n_alive == N - 595, 'one_dead': n_alive == N - 1, 'one_alive': n_alive == 1}[form]


def test_one_slot_worlds_have_no_dead_form():
    for form, crowd in M.BIN_VARIANTS:
        inp, n_alive = M.bin_inputs(Geo(48, 96), (4, 5), 1, form, crowd, False, False)
        assert n_alive in (0, 1) and (inp['alive'] is None or inp['alive'].all())
        M.check_bin(inp, *ideal_bin(inp, Geo(48, 96), (4, 5), n_alive), Geo(48, 96), (4, 5), n_alive)


# ---------------------------------------------------------------- the checkers' teeth
GEO_T, TILE_T = Geo(48, 96), (4, 5)


@pytest.fixture()
def good_sort():
    inp = M.sort_inputs(Geo(40, 70), 500, 2, True)
    out = ideal_sort(inp, Geo(40, 70))
    M.check_sort(inp, out, Geo(40, 70))
    return inp, out


@pytest.fixture()
def good_bin():
    inp, n_alive = M.bin_inputs(GEO_T, TILE_T, 900, 'dead_85', None, True, True)
    lay, m0, m1 = ideal_bin(inp, GEO_T, TILE_T, n_alive)
    M.check_bin(inp, lay, m0, m1, GEO_T, TILE_T, n_alive)
    return inp, n_alive, lay, m0, m1


def _swap(bufs, i, j):
    for b in bufs:
        v = M.body(b)
        v[i], v[j] = v[j], v[i]


def _all(out):
    return [out[k] for k in ('x', 'y', 'alive', 'agent_food', 'slot')] + list(out['extra'])


def test_sort_checker_sees_a_swap_across_a_bucket_border(good_sort):
    inp, out = good_sort
    key = M.sort_key(M.body(out['x']), M.body(out['y']), Geo(40, 70))
    j = int(np.flatnonzero(np.diff(key) > 0)[2])
    _swap(_all(out), j, j + 1)                         # whole records: still a permutation, every record intact
    with pytest.raises(AssertionError, match=f'keys decrease between output entries {j} and {j + 1}'):
        M.check_sort(inp, out, Geo(40, 70))


def test_sort_checker_sees_a_swap_inside_a_bucket_as_fine(good_sort):
    inp, out = good_sort
    key = M.sort_key(M.body(out['x']), M.body(out['y']), Geo(40, 70))
    j = int(np.flatnonzero(np.diff(key) == 0)[5])
    _swap(_all(out), j, j + 1)
    M.check_sort(inp, out, Geo(40, 70))


def test_sort_checker_sees_a_duplicated_slot_id(good_sort):
    inp, out = good_sort
    M.body(out['slot'])[101] = M.body(out['slot'])[100]
    with pytest.raises(AssertionError, match='appears twice, again at output entry 101'):
        M.check_sort(inp, out, Geo(40, 70))


def test_sort_checker_sees_an_attached_array_shifted_by_one(good_sort):
    inp, out = good_sort
    v = M.body(out['extra'][1])
    v[:] = np.roll(v, 1)
    with pytest.raises(AssertionError, match=r'extra\[1\] of output entry 0 '):
        M.check_sort(inp, out, Geo(40, 70))


def test_sort_checker_sees_a_nan_payload_and_a_zero_sign(good_sort):
    inp, out = good_sort
    food = M.body(out['agent_food'])
    j = int(np.flatnonzero(food == 0x7FC12345)[0])
    food[j] = 0x7FC00000                               # still a NaN
    with pytest.raises(AssertionError, match=f'agent_food of output entry {j} '):
        M.check_sort(inp, out, Geo(40, 70))
    food[j] = 0x7FC12345
    j = int(np.flatnonzero(food == 0x80000000)[0])
    food[j] = 0                                        # -0.0 == 0.0 as numbers
    with pytest.raises(AssertionError, match=f'agent_food of output entry {j} '):
        M.check_sort(inp, out, Geo(40, 70))


def test_sort_checker_sees_a_bucket_outside_its_range(good_sort):
    """Keys in order and every record intact, but an entry's position moved into the neighbouring bucket: only possible when the
    coordinates change too, which the record comparison reports first."""
    inp, out = good_sort
    key = M.sort_key(M.body(out['x']), M.body(out['y']), Geo(40, 70))
    j = int(np.flatnonzero(np.diff(key) > 0)[0])
    M.body(out['x'])[j], M.body(out['y'])[j] = M.body(out['x'])[j + 1], M.body(out['y'])[j + 1]
    with pytest.raises(AssertionError, match=f'x of output entry {j} |y of output entry {j} '):
        M.check_sort(inp, out, Geo(40, 70))


@pytest.mark.parametrize('name', ['x', 'y', 'alive', 'agent_food', 'slot', 'extra'])
@pytest.mark.parametrize('at', [0, M.GUARD - 1, -M.GUARD, -1])
def test_sort_checker_sees_one_guard_element_changed(good_sort, name, at):
    inp, out = good_sort
    buf = out[name] if name != 'extra' else out['extra'][0]
    M.bits(buf)[at] ^= 1
    with pytest.raises(AssertionError, match='the band (before|after) the array was written'):
        M.check_sort(inp, out, Geo(40, 70))


def test_bin_checker_sees_a_heading_half_left_behind(good_bin):
    inp, n_alive, lay, m0, m1 = good_bin
    v = M.body(lay['heading_lo'])
    v[7], v[8] = v[8], v[7]                            # the rest of the two records stayed
    with pytest.raises(AssertionError, match='heading_lo of output entry 7 '):
        M.check_bin(inp, lay, m0, m1, GEO_T, TILE_T, n_alive)


def test_bin_checker_sees_the_high_half_written_into_the_low_half(good_bin):
    inp, n_alive, lay, m0, m1 = good_bin
    M.body(lay['heading_lo'])[:] = M.body(lay['heading_hi'])
    with pytest.raises(AssertionError, match='heading_lo of output entry 0 '):
        M.check_bin(inp, lay, m0, m1, GEO_T, TILE_T, n_alive)


def test_bin_checker_sees_an_off_table_off_by_one(good_bin):
    inp, n_alive, lay, m0, m1 = good_bin
    M.body(m1['off'])[7:] += 1
    with pytest.raises(AssertionError, match=r'layout 1: off\[7\] is '):
        M.check_bin(inp, lay, m0, m1, GEO_T, TILE_T, n_alive)


def test_bin_checker_sees_stayers_that_are_not_the_count(good_bin):
    inp, n_alive, lay, m0, m1 = good_bin
    M.body(m0['s'])[4] -= 1
    with pytest.raises(AssertionError, match=r'layout 0: s\[4\] is '):
        M.check_bin(inp, lay, m0, m1, GEO_T, TILE_T, n_alive)
    M.body(m0['s'])[4] += 1
    M.body(m0['inc'])[8] = 1
    with pytest.raises(AssertionError, match=r'layout 0: inc\[8\] is 1'):
        M.check_bin(inp, lay, m0, m1, GEO_T, TILE_T, n_alive)


def test_bin_checker_sees_a_dead_record_inside_a_segment(good_bin):
    inp, n_alive, lay, m0, m1 = good_bin
    _swap(lay.values(), 50, n_alive + 3)               # whole records: an alive one behind the segments, a dead one inside
    with pytest.raises(AssertionError, match='bin: entry 50, inside the segment of tile .* holds the dead slot'):
        M.check_bin(inp, lay, m0, m1, GEO_T, TILE_T, n_alive)


def test_bin_checker_sees_a_record_in_the_wrong_segment(good_bin):
    inp, n_alive, lay, m0, m1 = good_bin
    first = int(M.body(m0['off'])[1])                  # first entry of tile 1 <-> last entry of tile 0
    _swap(lay.values(), first - 1, first)
    with pytest.raises(AssertionError, match=f'bin: entry {first - 1} lies in the segment of tile 0 and stands on tile 1'):
        M.check_bin(inp, lay, m0, m1, GEO_T, TILE_T, n_alive)
    _swap(lay.values(), first - 1, first)
    _swap(lay.values(), first, first + 1)              # inside a segment: free
    M.check_bin(inp, lay, m0, m1, GEO_T, TILE_T, n_alive)


def test_bin_checker_sees_a_carried_gradient_shifted_by_one(good_bin):
    inp, n_alive, lay, m0, m1 = good_bin
    v = M.body(lay['prev_gy'])
    v[:] = np.roll(v, -1)
    with pytest.raises(AssertionError, match='prev_gy of output entry 0 '):
        M.check_bin(inp, lay, m0, m1, GEO_T, TILE_T, n_alive)


@pytest.mark.parametrize('which', ['x', 'slot', 'heading_lo', 'prev_gx', 'meta0.off', 'meta1.inc'])
def test_bin_checker_sees_one_guard_element_changed(good_bin, which):
    inp, n_alive, lay, m0, m1 = good_bin
    buf = lay[which] if '.' not in which else {'meta0': m0, 'meta1': m1}[which.split('.')[0]][which.split('.')[1]]
    buf[len(buf) - M.GUARD] ^= 0x100
    with pytest.raises(AssertionError, match='the band after the array was written at element'):
        M.check_bin(inp, lay, m0, m1, GEO_T, TILE_T, n_alive)


def _scatter(inp, geo, cursor):
    """The scatter pass over given cursors, entry by entry: position = cursor[key]++ (a later write replaces an earlier one; what
    nobody writes keeps the sentinel)."""
    N = len(inp['x'])
    key = M.sort_key(inp['x'], inp['y'], geo)
    order = np.argsort(key, kind='stable')
    rank = np.empty(N, dtype=np.int64)
    start = np.cumsum(np.bincount(key, minlength=len(cursor))) - np.bincount(key, minlength=len(cursor))
    rank[order] = np.arange(N) - start[key[order]]
    pos = cursor[key] + rank
    assert pos.min() >= 0 and pos.max() < N             # (the edit below cannot leave an array)
    out = ideal_sort(inp, geo)
    ids = M._ids(inp, N)
    for name, src in [('x', inp['x']), ('y', inp['y']), ('alive', inp['alive']), ('agent_food', inp['agent_food']), ('slot', ids)]:
        b = M.body(out[name])
        b[:] = M.SENTINEL if b.dtype == np.uint8 else M.SENTINEL * 0x01010101
        b[pos] = M.bits(src)
    return out


def test_a_scan_that_sums_one_bucket_too_few_per_thread_is_caught():
    """k_sort_scan_big with `sum` over [lo, hi - 1) instead of [lo, hi): the threads' bases shrink, ranges overlap inside [0, N).
    The checker must see it at the first k_sort_scan_big shape with the inputs the GPU test uses — and accept the unedited scan."""
    W, H = 4096, 8160
    geo = Geo(W, H)
    kernel, per, nb4 = M.sort_scan(W, H)
    assert kernel == 'k_sort_scan_big'
    inp = M.sort_inputs(geo, M.MID_N, 0, False)
    hist = np.bincount(M.sort_key(inp['x'], inp['y'], geo), minlength=nb4)
    for short in (0, 1):
        sums = np.array([hist[t * per:max(min(t * per + per, nb4) - short, t * per)].sum() for t in range(M.SCAN_THREADS)])
        base = np.cumsum(sums) - sums
        cursor = np.empty(nb4, dtype=np.int64)
        for t in range(M.SCAN_THREADS):
            lo, hi = t * per, min(t * per + per, nb4)
            if lo < hi:
                cursor[lo:hi] = base[t] + np.cumsum(hist[lo:hi]) - hist[lo:hi]
        out = _scatter(inp, geo, cursor)
        if short:
            with pytest.raises(AssertionError):
                M.check_sort(inp, out, geo)
        else:
            M.check_sort(inp, out, geo)


# ---------------------------------------------------------------- the case tables
def test_sort_shapes_reach_the_scan_shapes_they_claim():
    for W, H, nb, nb4, kernel, per in M.SORT_SHAPES:
        assert M.n_buckets(W, H) == nb and M.sort_scan(W, H) == (kernel, per, nb4), (W, H)
        assert max(W, H) <= 2 ** 21
    pers = [(k, p) for *_, k, p in M.SORT_SHAPES]
    assert {p for k, p in pers if k == 'k_sort_scan'} == {4, 8, 64} and ('k_sort_scan_big', 65) in pers
    assert M.sort_scan(1023, 2047)[2] == 4 * M.SCAN_THREADS                     # per = 4 with every scan thread busy
    assert M.sort_scan(4095, 8191)[2] == M.SCAN_MAX_PER * M.SCAN_THREADS        # the last k_sort_scan shape …
    assert M.sort_scan(4096, 8160)[2] == M.SCAN_MAX_PER * M.SCAN_THREADS + 256  # … and the first past it,
    assert 65792 % 65 == 12 and 65792 // 65 == 1012                             # whose thread 1012 owns 12 buckets, 1013.. none
    assert M.n_buckets(4096, 8192) % 2 == 1 and M.sort_scan(4096, 8192)[2] == 66052
    assert M.sort_scan(300, 520)[2] // 4 == 81                                  # the old case: 81 of 1024 threads busy
    assert M.trips(M.ONE_TRIP) == (1, M.BLOCK) and M.trips(M.TRIP_PLUS) == (2, 37) and M.trips(M.MID_N) == (1, 224)
    assert M.trips(M.ONE_TRIP + 1) == (2, 1) and 37 % M.WAVE != 0
    assert [M.sort_ns(W, H)[len(M.SMALL_N):] for W, H, *_ in M.SORT_SHAPES] == \
        [(), (), (), (), (M.ONE_TRIP, M.TRIP_PLUS), (M.MID_N,), (M.MID_N,), (M.MID_N,), (M.MID_N, M.ONE_TRIP, M.TRIP_PLUS), (M.MID_N,)]


def test_bin_shapes_reach_the_scan_shapes_they_claim():
    for tile, W, H, nt, per in M.BIN_SHAPES:
        TX, TY = 1 << tile[0], 1 << tile[1]
        assert W % TX == 0 and H % TY == 0 and W // TX >= 3 and H // TY >= 3
        assert M.n_tiles(W, H, tile) == nt and M.bin_scan_per(W, H, tile) == per, (tile, W, H)
    assert {t for t, *_ in M.BIN_SHAPES} == {(6, 6), (5, 7), (5, 6), (4, 5)}
    assert [(W // (1 << t[0]), H // (1 << t[1])) for t, W, H, *_ in M.BIN_SHAPES[:4]] == [(3, 3)] * 4      # the smallest worlds
    assert 1056 // 2 == 528                                                     # 528 x 1024: 528 scan threads busy, 496 idle
    W, H = M.BIN_PLANE
    assert W % 16 == 0 and H % 32 == 0 and W // 16 >= 3 and H // 32 >= 3


@pytest.mark.parametrize('W,H', [(W, H) for W, H, nb, *_ in M.SORT_SHAPES if nb >= M.SORT_MID_MIN_BUCKETS])
def test_mid_n_fills_nine_buckets_in_ten_and_leaves_one_empty(W, H):
    count = M.mid_counts(W, H)
    assert count.sum() == M.MID_N and (count > 0).mean() >= 0.9 and (count == 0).any()
    assert ((count[1:-1] == 0) & (count[:-2] > 0) & (count[2:] > 0)).any()      # an empty bucket between two that are not


@pytest.mark.parametrize('W,H', [(W, H) for W, H, *_ in M.SORT_SHAPES])
def test_sort_inputs_hold_the_wave_patterns(W, H):
    geo = Geo(W, H)
    inp = M.sort_inputs(geo, 400, 0, False)
    key = M.sort_key(inp['x'], inp['y'], geo)
    assert len(set(key[64:256])) == 1                                           # three whole waves, one group each
    groups = min(64, len(M.reachable_buckets(W, H)))
    assert len(set(key[256:320])) == groups and (groups < 64 or key[319] not in key[256:319])      # lane 63 leads a group
    if W > 16 and H > 32:
        cx, cy = M.cells(inp['x'][320:324], W), M.cells(inp['y'][320:324], H)
        assert list(cx) == [15, 16, 15, 16] and list(cy) == [31, 32, 32, 31] and len(set(key[320:324])) == 4
    assert M.cells(inp['x'][324], W) == W - 1 and M.cells(inp['y'][324], H) == H - 1
    assert {int(v) for v in inp['x'][-4:]} == {0, 0xFFFFFFFF} and {int(v) for v in inp['y'][-4:]} == {0, 0xFFFFFFFF}
    f = M.bits(inp['agent_food'])
    assert all((f == s).any() for s in M.SPECIAL_F32)
    ids = M.sort_inputs(geo, 400, 1, True)['slot']
    assert len(set(ids)) == 400 and ids.min() >= 400


def test_decomposed_inputs_clamp_on_both_sides():
    for geo in M.sort_geos_decomposed():
        inp = M.sort_inputs(geo, 5000, 0, True)
        ix, iy = M.cells(inp['x'], 256) - geo.ox, M.cells(inp['y'], 256) - geo.oy
        assert ((ix < 0) | (ix >= geo.W)).mean() > 0.5 and ((iy < 0) | (iy >= geo.H)).mean() > 0.5      # most agents clamp …
        assert ((ix < 0).any() or geo.ox <= 0) and ((iy < 0).any() or geo.oy <= 0)                      # … below, where there is a below,
        assert ((ix >= geo.W).any() or geo.ox + geo.W >= 256) and ((iy >= geo.H).any() or geo.oy + geo.H >= 256)      # and above
    for geo in M.bin_geos_decomposed():
        inp, _ = M.bin_inputs(geo, M.BIN_PLANE_TILE, 5000, 'dead_85', None, True, True)
        up = np.mod(M.cells(inp['x'], 512) - geo.ox, 512)
        row = M.plane_coord(M.cells(inp['x'], 512), geo.ox, geo.W, 512)
        assert ((up >= geo.W) & (row == 0)).any() and ((up >= geo.W) & (row == geo.W - 1)).any()       # both edges catch agents


# ---------------------------------------------------------------- the refusals, through the C ABI
def medium_struct(L, geo):
    return L.Medium(W=geo.W, H=geo.H, gW=geo.gW, gH=geo.gH, ox=geo.ox, oy=geo.oy)


def pic_struct(L, tile, N, lay0, lay1, dep, dep_plane, part_gain, error, n_alive=0, prev_grad=((None, None), (None, None)), occ=None,
               rim=(None, None, None)):
    """die_pic for the binning: lay0 / lay1 = (x, y, agent_food, slot, heading_hi, heading_lo, off, n, s, inc) as addresses."""
    p = L.Pic(tile_xs=tile[0], tile_ys=tile[1], N=N, layout=(L.PicLayout * 2)(L.PicLayout(*lay0), L.PicLayout(*lay1)), dep=dep,
              dep_plane=dep_plane, part_gain=part_gain, error=error, rim=rim[0], rim_code=rim[1], rim_cnt=rim[2], n_alive=n_alive, occ=occ)
    for l in (0, 1):
        for axis in (0, 1):
            p.prev_grad[l][axis] = prev_grad[l][axis]
    return p


def _fakes(n, base=FAKE):
    return tuple(base + 4096 * k for k in range(n))


def _sort_call(L, *, W=300, H=520, gW=0, gH=0, N=1000, N_out=None, medium=True, agents_in=True, agents_out=True, ws=FAKE * 3, ws_short=0,
               out_slot=True, same=False, n_extra=0, extra_in='ok', extra_out='ok', in_x=True):
    m = L.Medium(W=W, H=H, gW=gW, gH=gH)
    fi, fo = _fakes(5), _fakes(5, FAKE * 2)
    a_in = L.Agents(N, fi[0] if in_x else None, fi[1], fi[2], fi[3], None)
    src = fi if same else fo
    a_out = L.Agents(N if N_out is None else N_out, src[0], src[1], src[2], src[3], fo[4] if out_slot else None)
    n = max(n_extra, 1)
    ein = None if extra_in is None else (C.c_void_p * 5)(*[None if extra_in == k else FAKE * 4 + 4096 * k for k in range(5)])
    eout = None if extra_out is None else (C.c_void_p * 5)(*[FAKE * 4 + 4096 * k if extra_out == k else FAKE * 5 + 4096 * k for k in range(5)])
    assert n <= 5
    need = M.sort_workspace_bytes(W, H, N)
    return L.lib.die_agents_sort(C.byref(m) if medium else None, C.byref(a_in) if agents_in else None, C.byref(a_out) if agents_out else None,
                                 n_extra, ein, eout, ws, max(need, 256) - ws_short, None)


SORT_REFUSALS = [
    ('null medium', dict(medium=False), b'null argument'),
    ('null in', dict(agents_in=False), b'null argument'),
    ('null out', dict(agents_out=False), b'null argument'),
    ('null workspace', dict(ws=None), b'null argument'),
    ('N 0', dict(N=0), b'bad slot counts'),
    ('unequal N', dict(N_out=999), b'bad slot counts'),
    ('N 2^31', dict(N=2 ** 31), b'bad slot counts'),
    ('null in->x', dict(in_x=False), b'null device pointer'),
    ('null out->slot', dict(out_slot=False), b'out->slot is required'),
    ('in is out', dict(same=True), b'in and out must be different arrays'),
    ('n_extra -1', dict(n_extra=-1), b'at most 4 attached arrays'),
    ('n_extra 5', dict(n_extra=5), b'at most 4 attached arrays'),
    ('attached inputs missing', dict(n_extra=2, extra_in=None), b'attached arrays missing'),
    ('attached outputs missing', dict(n_extra=2, extra_out=None), b'attached arrays missing'),
    ('attached input 1 null', dict(n_extra=2, extra_in=1), b'bad attached array 1'),
    ('attached array 3 is its output', dict(n_extra=4, extra_out=3), b'bad attached array 3'),
    ('workspace one byte short', dict(ws_short=1), b'workspace too small (3071 < 3072)'),
    ('W 0', dict(W=0), b'bad extents 0x520'),
    ('H 0', dict(H=0), b'bad extents 300x0'),
    ('W negative', dict(W=-16, H=32), b'bad extents -16x32'),
    ('H negative', dict(H=-1), b'bad extents 300x-1'),
    ('decomposed without gH', dict(gW=600, gH=0), b'bad world extents 600x0'),
]


@pytest.mark.parametrize('case,kw,needle', SORT_REFUSALS, ids=[c for c, *_ in SORT_REFUSALS])
def test_sort_refuses_bad_arguments_before_launch(lib, case, kw, needle):
    assert _sort_call(lib, **kw) == ARG, (case, lib.lib.die_last_error())
    msg = lib.lib.die_last_error()
    assert needle in msg and msg.startswith(b'die_agents_sort: '), (case, msg)


def test_non_positive_extents_no_longer_pass_the_workspace_check(lib):
    """die_sort_workspace_bytes is -1 for W < 1 or H < 1, and `ws_bytes >= -1` held for every workspace: the refusal must come from
    the extents themselves, whatever the workspace."""
    for W, H in ((0, 520), (300, 0), (-5, -5), (-2 ** 31, 64)):
        assert lib.lib.die_sort_workspace_bytes(W, H, 1000) == -1
        assert _sort_call(lib, W=W, H=H) == ARG and b'bad extents %dx%d' % (W, H) in lib.lib.die_last_error()


def test_sort_workspace_bytes_is_the_formula(lib):
    f = lib.lib.die_sort_workspace_bytes
    for W, H, N in ((0, 8, 8), (8, 0, 8), (-1, 8, 8), (8, -1, 8), (8, 8, 0), (8, 8, -1), (8, 8, 2 ** 31), (8, 8, 2 ** 40)):
        assert f(W, H, N) == -1 == M.sort_workspace_bytes(W, H, N), (W, H, N)
    for W, H, nb, nb4, *_ in M.SORT_SHAPES:
        for N in (1, 1000, 2 ** 31 - 1):
            got = f(W, H, N)
            assert got == M.sort_workspace_bytes(W, H, N) == 2 * ((4 * nb4 + 255) // 256 * 256), (W, H, N)
    assert f(300, 520, 1000) == 3072
    assert f(2 ** 31 - 1, 2 ** 31 - 1, 5) == M.sort_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1, 5)          # 64-bit arithmetic


def _bin_call(L, *, W=48, H=96, gW=0, gH=0, tile=(4, 5), N=100, a_N=None, into=1, held=None, n_alive=0, alive=False, pg=None,
              pg_out=True, momentum=False, error=True):
    m = L.Medium(W=W, H=H, gW=gW, gH=gH)
    lay0, lay1 = _fakes(10, FAKE * 2), _fakes(10, FAKE * 3)
    fa = _fakes(8)
    x = (lay0, lay1)[held][0] if held is not None else fa[0]
    a = L.Agents(N if a_N is None else a_N, x, fa[1], fa[2] if alive else None, fa[3], None)
    out_pg = ((FAKE * 6, FAKE * 6 + 4096), (FAKE * 7, FAKE * 7 + 4096)) if pg_out else ((None, None), (None, None))
    p = pic_struct(L, tile, N, lay0, lay1, FAKE * 4, FAKE * 4 + 4096, FAKE * 4 + 8192, FAKE * 4 + 12288 if error else None, n_alive=n_alive,
                   prev_grad=out_pg)
    if pg is None and not momentum:
        return L.lib.die_pic_bin(C.byref(m), C.byref(a), fa[4], fa[5], C.byref(p), into, None)
    gx, gy = pg if pg is not None else (None, None)
    return L.lib.die_pic_bin_momentum(C.byref(m), C.byref(a), fa[4], fa[5], gx, gy, C.byref(p), into, None)


BIN_REFUSALS = [
    ('tile 8x32', dict(tile=(3, 5)), ARG, b'tile shape 2^3 x 2^5 is not compiled in'),
    ('tile 64x32', dict(tile=(6, 5), W=192), ARG, b'tile shape 2^6 x 2^5 is not compiled in'),
    ('40 rows', dict(W=40), UNSUPPORTED, b'a 40x96 world does not split into at least 3x3 whole tiles of 16x32 cells'),
    ('two rows of tiles', dict(W=32), UNSUPPORTED, b'a 32x96 world does not split into at least 3x3 whole tiles'),
    ('two columns of tiles', dict(H=64), UNSUPPORTED, b'a 48x64 world does not split into at least 3x3 whole tiles'),
    ('no rows', dict(W=0), UNSUPPORTED, b'a 0x96 world does not split'),
    ('negative rows', dict(W=-48), UNSUPPORTED, b'a -48x96 world does not split'),
    ('a->N is not p->N', dict(a_N=99), ARG, b'bad agent arrays'),
    ('into 2', dict(into=2), ARG, b'layout index 2'),
    ('into -1', dict(into=-1), ARG, b'layout index -1'),
    ('into the layout that holds the agents', dict(into=0, held=0), ARG, b'already held in layout 0'),
    ('… layout 1', dict(into=1, held=1), ARG, b'already held in layout 1'),
    ('dead slots without flags', dict(n_alive=40), ARG, b'n_alive 40 of 100 slots needs the alive flags'),
    ('n_alive above N', dict(n_alive=101, alive=True), ARG, b'n_alive 101 of 100 slots'),
    ('n_alive negative', dict(n_alive=-1, alive=True), ARG, b'n_alive -1 of 100 slots'),
    ('no error word', dict(error=False), ARG, b'null workspace pointer'),
    ('decomposed without gH', dict(gW=512, gH=0), ARG, b'bad world extents 512x0'),
]
MOMENTUM_REFUSALS = [
    ('prev_gx alone', dict(pg=(FAKE * 8, None)), ARG, b'_prev_grad given without'),
    ('prev_gy alone', dict(pg=(None, FAKE * 8)), ARG, b'_prev_grad given without'),
    ('nowhere to carry it, layout 1', dict(pg=(FAKE * 8, FAKE * 9), pg_out=False), ARG, b'_prev_grad given without die_pic.prev_grad[1]'),
    ('nowhere to carry it, layout 0', dict(pg=(FAKE * 8, FAKE * 9), pg_out=False, into=0), ARG, b'_prev_grad given without die_pic.prev_grad[0]'),
    ('carried into itself', dict(pg=(FAKE * 7, FAKE * 9)), ARG, b'_prev_grad given without'),
]


@pytest.mark.parametrize('momentum', [False, True], ids=['die_pic_bin', 'die_pic_bin_momentum'])
@pytest.mark.parametrize('case,kw,status,needle', BIN_REFUSALS, ids=[c for c, *_ in BIN_REFUSALS])
def test_bin_refuses_bad_arguments_before_launch(lib, momentum, case, kw, status, needle):
    assert _bin_call(lib, momentum=momentum, **kw) == status, (case, lib.lib.die_last_error())
    msg = lib.lib.die_last_error()
    assert needle in msg and msg.startswith(b'die_pic_bin: '), (case, msg)


@pytest.mark.parametrize('case,kw,status,needle', MOMENTUM_REFUSALS, ids=[c for c, *_ in MOMENTUM_REFUSALS])
def test_bin_momentum_refuses_half_a_gradient(lib, case, kw, status, needle):
    assert _bin_call(lib, **kw) == status, (case, lib.lib.die_last_error())
    msg = lib.lib.die_last_error()
    assert needle in msg and msg.startswith(b'die_pic_bin: '), (case, msg)
