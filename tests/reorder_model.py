"""A counting-sort model of the two device passes that re-order the agent arrays: die_agents_sort (csrc/die_sort.hip) and
die_pic_bin / die_pic_bin_momentum (csrc/die_pic.hip).  numpy only; tests/test_reorder_cpu.py checks the model against brute force
and the checkers against broken outputs, tests/test_gpu_reorder.py hands them what the device wrote.

The cell of a Q0.32 coordinate X on an axis of n cells is oracle.cpu_ref.cell(X / 2**32, n): X / 2**32 is exact in float64, the
product with n - 1 has at most 32 + 21 = 53 significant bits for n <= 2**21 and the + 0.5 falls inside them, so the float64 value
IS the real one and its floor the cell — no integer multiply is restated here.

Order inside a bucket or a tile's segment is free.  Slot ids are distinct, so "the segment holds, as a set, exactly the records of
its tile" is checked as: the output's slot ids are a permutation of the input's, the record at every output entry is — bit for bit
— the input record of that slot id, and the key of the entry at position j is the key the counts put there.  Everything is compared
as bit patterns (uint32 / uint8 views): a NaN's payload and the sign of a zero count.

Every array the device writes lies between two bands of GUARD elements filled with SENTINEL bytes; the checkers take the whole
buffers and require the bands back untouched."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import cpu_ref as R

GUARD = 64                      # elements before and after every output array
SENTINEL = 0xA5                 # every byte of a band
SORT_XS, SORT_YS = 4, 5         # a sort bucket is 16 rows x 32 columns of cells
GRID_CAP, BLOCK, WAVE = 4096, 256, 64     # both passes: at most 4096 workgroups of 256 threads walk the entries in a strided loop
SCAN_THREADS, SCAN_MAX_PER = 1024, 64

# the planes' extents, the world's (gW == 0: the planes are the world) and the world cell of local element (0, 0)
Geo = namedtuple('Geo', 'W H gW gH ox oy', defaults=(0, 0, 0, 0))


def world(geo):
    return (geo.gW, geo.gH) if geo.gW > 0 else (geo.W, geo.H)


def bits(a):
    """The bit pattern of a 4-byte or 1-byte array as unsigned integers."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.itemsize == 1 else a.view(np.uint32)


def cells(X, n):
    return R.cell(np.asarray(X, dtype=np.uint32).astype(np.float64) / 2.0 ** 32, n)


def coord_of_cell(c, n):
    """A Q0.32 coordinate that stands on cell c of n: the label c / (n - 1) itself (the last label is 2**32, one above the range)."""
    c = np.asarray(c, dtype=np.float64)
    if n == 1:
        return np.zeros(c.shape, dtype=np.uint32)
    return np.minimum(np.rint(c / (n - 1) * 2.0 ** 32), 2.0 ** 32 - 1).astype(np.uint32)


# ---------------------------------------------------------------- keys
def n_buckets(W, H):
    return ((W >> SORT_XS) + 1) * ((H >> SORT_YS) + 1)


def sort_key(x, y, geo):
    gW, gH = world(geo)
    ox, oy = (geo.ox, geo.oy) if geo.gW > 0 else (0, 0)
    ix = np.clip(cells(x, gW) - ox, 0, geo.W - 1)
    iy = np.clip(cells(y, gH) - oy, 0, geo.H - 1)
    return (ix >> SORT_XS) * ((geo.H >> SORT_YS) + 1) + (iy >> SORT_YS)


def plane_coord(c, o, n, gn):
    """World cell c of an axis of gn cells -> row (or column) of planes that hold the n cells from world cell o on, periodically.
    Walk upwards from the planes' first cell, around the world: after `up` steps one stands on c.  up < n: the planes hold c, at
    element `up`.  Otherwise c lies outside, `up - (n - 1)` cells above the planes' last cell and `gn - up` cells below their first
    one: the nearer of the two edges, the last one when both are equally far."""
    up = np.mod(np.asarray(c, dtype=np.int64) - o, gn)
    above_last, below_first = up - (n - 1), gn - up
    return np.where(up < n, up, np.where(above_last <= below_first, n - 1, 0))


def tile_key(x, y, geo, tile):
    xs, ys = tile
    gW, gH = world(geo)
    row, col = cells(x, gW), cells(y, gH)
    if geo.gW > 0:
        row, col = plane_coord(row, geo.ox, geo.W, gW), plane_coord(col, geo.oy, geo.H, gH)
    return (row >> xs) * (geo.H >> ys) + (col >> ys)


def n_tiles(W, H, tile):
    return (W >> tile[0]) * (H >> tile[1])


# ---------------------------------------------------------------- the two host formulas (restated once, for the case tables)
def sort_workspace_bytes(W, H, N):
    if W < 1 or H < 1 or N < 1 or N >= 2 ** 31:
        return -1
    nb4 = (n_buckets(W, H) + 3) & ~3
    return 2 * ((nb4 * 4 + 255) & ~255)


def sort_scan(W, H):
    """(kernel, per, padded bucket count): `per` consecutive buckets per thread of the one-workgroup scan."""
    nb4 = (n_buckets(W, H) + 3) & ~3
    per = ((nb4 + SCAN_THREADS - 1) // SCAN_THREADS + 3) & ~3
    if per <= SCAN_MAX_PER:
        return 'k_sort_scan', per, nb4
    return 'k_sort_scan_big', (nb4 + SCAN_THREADS - 1) // SCAN_THREADS, nb4


def bin_scan_per(W, H, tile):
    return (n_tiles(W, H, tile) + SCAN_THREADS - 1) // SCAN_THREADS


def trips(N):
    """(trips of the strided loop, threads of the last trip's last workgroup that hold an entry)."""
    groups = (N + BLOCK - 1) // BLOCK
    return (groups + GRID_CAP - 1) // GRID_CAP, N - (groups - 1) * BLOCK


# ---------------------------------------------------------------- guarded buffers
def guarded(n, itemsize):
    """A host image of a guarded device buffer: (n + 2 GUARD) elements, every byte SENTINEL."""
    return np.full(n + 2 * GUARD, SENTINEL, dtype=np.uint8 if itemsize == 1 else np.uint32) * (1 if itemsize == 1 else 0x01010101)


def body(buf):
    return bits(buf)[GUARD:len(buf) - GUARD]


def _check_bands(name, buf):
    b = bits(buf)
    want = SENTINEL if b.dtype == np.uint8 else SENTINEL * 0x01010101
    for where, band, base in (('before', b[:GUARD], 0), ('after', b[len(b) - GUARD:], len(b) - GUARD)):
        bad = np.flatnonzero(band != want)
        assert bad.size == 0, f'{name}: the band {where} the array was written at element {base + int(bad[0]) - GUARD} (relative to the array)'


def _first(cond):
    bad = np.flatnonzero(cond)
    return int(bad[0]) if bad.size else None


def _ids(inp, N):
    return np.arange(N, dtype=np.uint32) if inp.get('slot') is None else bits(inp['slot'])


def _match_records(ids, out_slot, pairs, what):
    """out_slot is a permutation of ids, and every (input, output) pair of arrays holds at output entry j the input value of the entry
    whose id is out_slot[j].  Returns the input index of every output entry."""
    N = len(ids)
    assert len(out_slot) == N, f'{what}: {len(out_slot)} output entries for {N} inputs'
    order = np.argsort(ids, kind='stable')
    sorted_ids = ids[order]
    assert _first(sorted_ids[1:] == sorted_ids[:-1]) is None, f'{what}: the INPUT slot ids are not distinct'
    pos = np.minimum(np.searchsorted(sorted_ids, out_slot), N - 1)
    j = _first(sorted_ids[pos] != out_slot)
    assert j is None, f'{what}: output entry {j} carries slot id {int(out_slot[j])}, which no input entry has'
    seen = np.sort(out_slot, kind='stable')
    d = _first(seen[1:] == seen[:-1])
    if d is not None:
        j = int(np.flatnonzero(out_slot == seen[d])[1])
        raise AssertionError(f'{what}: slot id {int(seen[d])} appears twice, again at output entry {j}')
    src = order[pos]
    for name, a_in, a_out in pairs:
        j = _first(bits(a_in)[src] != a_out)
        assert j is None, (f'{what}: {name} of output entry {j} (slot id {int(out_slot[j])}) is {int(a_out[j]):#x}, '
                           f'its input record has {int(bits(a_in)[src[j]]):#x}')
    return src


# ---------------------------------------------------------------- checkers
def check_sort(inp, out, geo):
    """inp: x, y, alive, agent_food, slot (None: identity), extra (list of float32 arrays).  out: the guarded buffers the device wrote:
    x, y, alive, agent_food, slot, extra (list)."""
    N = len(inp['x'])
    extra_in, extra_out = list(inp.get('extra') or []), list(out.get('extra') or [])
    assert len(extra_in) == len(extra_out)
    named = [(k, out[k]) for k in ('x', 'y', 'alive', 'agent_food', 'slot')] + [(f'extra[{e}]', b) for e, b in enumerate(extra_out)]
    for name, buf in named:
        assert len(buf) == N + 2 * GUARD, f'{name}: a buffer of {len(buf)} elements for {N} entries'
        _check_bands(name, buf)
    pairs = [(k, inp[k], body(out[k])) for k in ('x', 'y', 'alive', 'agent_food')]
    pairs += [(f'extra[{e}]', a, body(b)) for e, (a, b) in enumerate(zip(extra_in, extra_out))]
    _match_records(_ids(inp, N), body(out['slot']), pairs, 'sort')
    key = sort_key(body(out['x']), body(out['y']), geo)
    j = _first(np.diff(key) < 0)
    assert j is None, f'sort: keys decrease between output entries {j} and {j + 1} ({int(key[j])} -> {int(key[j + 1])})'
    count = np.bincount(sort_key(inp['x'], inp['y'], geo), minlength=n_buckets(geo.W, geo.H))
    assert len(count) == n_buckets(geo.W, geo.H)
    want = np.repeat(np.arange(len(count)), count)        # bucket b owns [cumsum(count)[b] - count[b], cumsum(count)[b])
    j = _first(key != want)
    assert j is None, f'sort: output entry {j} has key {int(key[j])}, the counts put bucket {int(want[j])} there'
    return count


def bin_tables(inp, geo, tile, n_alive):
    """(alive mask, tile key of every entry, count per tile) as die_pic_bin reads its arguments: n_alive 0 or N = every slot alive."""
    N = len(inp['x'])
    dead = 0 < n_alive < N
    assert 0 <= n_alive <= N and (not dead or inp.get('alive') is not None)
    mask = (np.asarray(inp['alive']) != 0) if dead else np.ones(N, dtype=bool)
    assert int(mask.sum()) == (n_alive if dead else N), 'the inputs hold another number of alive slots than n_alive says'
    key = tile_key(inp['x'], inp['y'], geo, tile)
    count = np.bincount(key[mask], minlength=n_tiles(geo.W, geo.H, tile))
    assert len(count) == n_tiles(geo.W, geo.H, tile)
    return mask, key, count


def check_bin(inp, out_layout, meta0, meta1, geo, tile, n_alive):
    """inp: x, y, alive (or None), agent_food, slot (or None), heading_hi, heading_lo, prev_gx, prev_gy (or None: not carried).
    out_layout: the guarded buffers of the layout that was written (x, y, agent_food, slot, heading_hi, heading_lo and, when carried,
    prev_gx, prev_gy); meta0 / meta1: the guarded per-tile tables (off, n, s, inc) of layout 0 / 1."""
    N = len(inp['x'])
    mask, key, count = bin_tables(inp, geo, tile, n_alive)
    NT = len(count)
    off = np.cumsum(count) - count
    for l, meta in enumerate((meta0, meta1)):
        for name, want in (('off', off), ('n', count), ('s', count), ('inc', np.zeros(NT, dtype=np.int64))):
            buf = meta[name]
            assert len(buf) == NT + 2 * GUARD, f'layout {l} {name}: a buffer of {len(buf)} words for {NT} tiles'
            _check_bands(f'layout {l} {name}', buf)
            t = _first(body(buf).astype(np.int64) != want)
            assert t is None, f'layout {l}: {name}[{t}] is {int(body(buf)[t])}, the counts give {int(want[t])}'
    names = ['x', 'y', 'agent_food', 'heading_hi', 'heading_lo'] + (['prev_gx', 'prev_gy'] if inp.get('prev_gx') is not None else [])
    for name in names + ['slot']:
        assert len(out_layout[name]) == N + 2 * GUARD, f'{name}: a buffer of {len(out_layout[name])} elements for {N} entries'
        _check_bands(name, out_layout[name])
    src = _match_records(_ids(inp, N), body(out_layout['slot']), [(k, inp[k], body(out_layout[k])) for k in names], 'bin')
    n_seg = int(count.sum())
    want_tile = np.repeat(np.arange(NT), count)           # tile t owns [off[t], off[t] + count[t])
    j = _first(~mask[src[:n_seg]])
    assert j is None, f'bin: entry {j}, inside the segment of tile {int(want_tile[j])}, holds the dead slot {int(body(out_layout["slot"])[j])}'
    j = _first(key[src[:n_seg]] != want_tile)
    assert j is None, f'bin: entry {j} lies in the segment of tile {int(want_tile[j])} and stands on tile {int(key[src[j]])}'
    j = _first(mask[src[n_seg:]])
    assert j is None, f'bin: entry {n_seg + j}, behind the segments, holds the alive slot {int(body(out_layout["slot"])[n_seg + j])}'
    return count


# ---------------------------------------------------------------- inputs
SPECIAL_F32 = np.array([0x7FC12345, 0xFFA00001, 0x7F800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x00000000],
                       dtype=np.uint32)       # NaNs with payloads (quiet, negative, signalling), -0.0, +-inf, a subnormal, +0.0


def _f32(rs, N):
    """float32 values as bit patterns: ordinary numbers with SPECIAL_F32 strewn in (every third entry), at least the first eight."""
    v = bits(rs.standard_normal(N).astype(np.float32)).copy()
    at = np.arange(0, N, 3)
    v[at] = SPECIAL_F32[rs.randint(0, len(SPECIAL_F32), len(at))]
    v[:min(N, len(SPECIAL_F32))] = SPECIAL_F32[:N]
    return v.view(np.float32)


def _u32(rs, N):
    return rs.randint(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)


def _foreign_ids(rs, N):
    """Distinct ids that do not fit [0, N), shuffled — as a decomposed rank's world slot ids."""
    return (rs.permutation(N).astype(np.uint64) * 7 + 1_000_003).astype(np.uint32)


def _place(x, y, start, wx, wy, gW, gH):
    """Entries [start, start + len) stand on world cells (wx, wy), taken around the world; what does not fit the arrays is dropped."""
    n = max(0, min(len(wx), len(x) - start))
    x[start:start + n] = coord_of_cell(np.mod(wx[:n], gW), gW)
    y[start:start + n] = coord_of_cell(np.mod(wy[:n], gH), gH)


def _patterns(x, y, geo, groups, borders):
    """The wave patterns of a counting sort, written over uniform positions: entries [64, 256) — three whole waves — on ONE cell;
    entries [256, 320) — one wave — on 64 different groups' first cells (`groups`: local (row, col) per group; all of them where
    there are fewer: the wave then holds 64 groups, lane 63 leads one); then cells on both sides of the borders; the extremes
    of the coordinate range last."""
    N, (gW, gH) = len(x), world(geo)
    ox, oy = (geo.ox, geo.oy) if geo.gW > 0 else (0, 0)
    g = groups[np.linspace(0, len(groups) - 1, min(WAVE, len(groups))).astype(np.int64)]
    _place(x, y, 64, np.full(192, g[len(g) // 2][0] + ox), np.full(192, g[len(g) // 2][1] + oy), gW, gH)
    _place(x, y, 256, g[:, 0] + ox, g[:, 1] + oy, gW, gH)
    b = np.array(borders, dtype=np.int64).reshape(-1, 2)
    _place(x, y, 320, np.clip(b[:, 0], 0, geo.W - 1) + ox, np.clip(b[:, 1], 0, geo.H - 1) + oy, gW, gH)
    ext = [(0, 0xFFFFFFFF), (0xFFFFFFFF, 0), (0, 0), (0xFFFFFFFF, 0xFFFFFFFF)][:N]
    for k, (ex, ey) in enumerate(ext):
        x[N - 1 - k], y[N - 1 - k] = ex, ey


def reachable_buckets(W, H):
    """Local first cells (row, col) of the buckets a cell of the planes can fall into (the table has one more row / column of buckets
    than cells reach when an extent is a multiple of the bucket's)."""
    bx, by = np.arange(((W - 1) >> SORT_XS) + 1), np.arange(((H - 1) >> SORT_YS) + 1)
    return np.stack(np.meshgrid(bx << SORT_XS, by << SORT_YS, indexing='ij'), -1).reshape(-1, 2)


def sort_inputs(geo, N, n_extra, foreign_slots, seed=0):
    rs = np.random.RandomState((seed * 1_000_003 + N * 31 + n_extra * 7 + int(foreign_slots)) % 2 ** 31)
    x, y = _u32(rs, N), _u32(rs, N)
    W, H = geo.W, geo.H
    borders = [(15, 31), (16, 32), (15, 32), (16, 31), (W - 1, H - 1), (W - 1, 0), (0, H - 1), (W - 2, H - 2)]
    _patterns(x, y, geo, reachable_buckets(W, H), borders)
    if N >= MID_N and geo.gW == 0 and W > 2 << SORT_XS:
        # one bucket in the middle of the table stays EMPTY (its cursor equals its successor's): uniform positions alone leave none
        # empty where a bucket holds 73 agents on average (1023 x 2047).  Whoever stands there moves one bucket of rows on; the
        # buckets of the patterns above are left alone.
        key = sort_key(x, y, geo)
        taken = set(key[64:328]) | set(key[-4:])
        cand = [int(k) for k in sort_key(*(coord_of_cell(reachable_buckets(W, H)[:, a], n) for a, n in ((0, W), (1, H))), geo)]
        empty = next(k for k in cand[len(cand) // 3:] if k not in taken)
        on = key == empty
        row = cells(x[on], W)
        x[on] = coord_of_cell(np.where(row + (1 << SORT_XS) < W, row + (1 << SORT_XS), row - (1 << SORT_XS)), W)
    return dict(x=x, y=y, alive=rs.randint(0, 2, N).astype(np.uint8), agent_food=_f32(rs, N),
                slot=_foreign_ids(rs, N) if foreign_slots else None, extra=[_f32(rs, N) for _ in range(n_extra)])


ALIVE_FORMS = ('alive_null', 'all_alive', 'dead_85', 'one_dead', 'one_alive')
CROWDS = ('one_tile', 'empty_row')
BIN_VARIANTS = tuple((f, None) for f in ALIVE_FORMS) + tuple(('dead_85', c) for c in CROWDS)     # (alive form, crowding)


def bin_inputs(geo, tile, N, form, crowd, foreign_slots, momentum, seed=0):
    """-> (inputs, n_alive as die_pic.n_alive takes it).  N == 1 has no form with both kinds of slot: every slot is alive then."""
    rs = np.random.RandomState((seed * 1_000_003 + N * 31 + ALIVE_FORMS.index(form) * 7 + int(foreign_slots) * 3 + int(momentum)) % 2 ** 31)
    xs, ys = tile
    TX, TY, W, H = 1 << xs, 1 << ys, geo.W, geo.H
    gW, gH = world(geo)
    x, y = _u32(rs, N), _u32(rs, N)
    tiles = np.stack(np.meshgrid(np.arange(W >> xs) << xs, np.arange(H >> ys) << ys, indexing='ij'), -1).reshape(-1, 2)
    borders = [(TX - 1, TY - 1), (TX, TY), (TX - 1, TY), (TX, TY - 1), (W - 1, H - 1), (W - 1, 0), (0, H - 1), (W - TX, H - TY)]
    _patterns(x, y, geo, tiles, borders)
    if crowd == 'one_tile':                               # every agent on the tile (1, 2), the extremes of the range included
        assert geo.gW == 0
        x = coord_of_cell(TX + rs.randint(0, TX, N), W)
        y = coord_of_cell(2 * TY + rs.randint(0, TY, N), H)
    elif crowd == 'empty_row':                            # nobody on the tiles of row 1: whoever stands there moves one tile up
        assert geo.gW == 0
        row = cells(x, W)
        on = (row >> xs) == 1
        x[on] = coord_of_cell(row[on] + TX, W)
    if form in ('alive_null', 'all_alive') or N == 1:
        alive = None if form == 'alive_null' else np.ones(N, dtype=np.uint8)
        n_alive = 0 if form == 'alive_null' else N
    else:
        n_dead = {'dead_85': min(max(int(round(0.85 * N)), 1), N - 1), 'one_dead': 1, 'one_alive': N - 1}[form]
        alive = np.ones(N, dtype=np.uint8)
        alive[rs.permutation(N)[:n_dead]] = 0
        n_alive = N - n_dead
    inp = dict(x=x, y=y, alive=alive, agent_food=_f32(rs, N), slot=_foreign_ids(rs, N) if foreign_slots else None,
               heading_hi=_u32(rs, N), heading_lo=_u32(rs, N), prev_gx=_f32(rs, N) if momentum else None,
               prev_gy=_f32(rs, N) if momentum else None)
    return inp, n_alive


# ---------------------------------------------------------------- the case tables
ONE_TRIP = GRID_CAP * BLOCK                               # exactly one full trip of the strided loops
TRIP_PLUS = ONE_TRIP + 3 * BLOCK + 37                     # a second trip that ends in a partial workgroup and a partial wave
SMALL_N = (1, 63, 64, 65, 255, 256, 257)
MID_N = 300_000
N_EXTRA = (0, 1, 2, 3, 4)

# (W, H, buckets, padded buckets, scan kernel, per): what the issue's table claims; tests/test_reorder_cpu.py derives it again
SORT_SHAPES = (
    (1, 1, 1, 4, 'k_sort_scan', 4),
    (15, 31, 1, 4, 'k_sort_scan', 4),
    (16, 32, 4, 4, 'k_sort_scan', 4),
    (40, 70, 9, 12, 'k_sort_scan', 4),
    (300, 520, 323, 324, 'k_sort_scan', 4),
    (1023, 2047, 4096, 4096, 'k_sort_scan', 4),
    (1024, 2047, 4160, 4160, 'k_sort_scan', 8),
    (4095, 8191, 65536, 65536, 'k_sort_scan', 64),
    (4096, 8160, 65792, 65792, 'k_sort_scan_big', 65),
    (4096, 8192, 66049, 66052, 'k_sort_scan_big', 65),
)
SORT_BIG_SHAPES = ((300, 520), (4096, 8160))              # the two largest N run here only
SORT_MID_MIN_BUCKETS = 4096                               # MID_N runs where there are at least this many buckets

ORIGINS = (-11, 187, 80)                                  # halo across the world's seam; the planes end at the seam; inside
SORT_PLANE, SORT_WORLD = (80, 96), (256, 256)
BIN_PLANE, BIN_WORLD, BIN_PLANE_TILE = (96, 128), (512, 512), (4, 5)
DECOMPOSED_N = SMALL_N + (5000,)


def sort_ns(W, H):
    ns = list(SMALL_N)
    if n_buckets(W, H) >= SORT_MID_MIN_BUCKETS:
        ns.append(MID_N)
    if (W, H) in SORT_BIG_SHAPES:
        ns += [ONE_TRIP, TRIP_PLUS]
    return tuple(ns)


def sort_geos_decomposed():
    return tuple(Geo(*SORT_PLANE, *SORT_WORLD, ox, oy) for ox in ORIGINS for oy in ORIGINS)


# (tile, W, H, tiles, per of k_pic_bin_scan)
BIN_SHAPES = (
    ((4, 5), 48, 96, 9, 1),
    ((6, 6), 192, 192, 9, 1),
    ((5, 7), 96, 384, 9, 1),
    ((5, 6), 96, 192, 9, 1),
    ((4, 5), 512, 1024, 1024, 1),
    ((4, 5), 528, 1024, 1056, 2),
    ((4, 5), 2048, 4096, 16384, 16),
)
BIN_TRIP_PLUS_SHAPE = (528, 1024)


def bin_ns(W, H):
    ns = list(SMALL_N) + [MID_N, ONE_TRIP]
    if (W, H) == BIN_TRIP_PLUS_SHAPE:
        ns.append(TRIP_PLUS)
    return tuple(ns)


def bin_geos_decomposed():
    return tuple(Geo(*BIN_PLANE, *BIN_WORLD, ox, oy) for ox in ORIGINS for oy in ORIGINS)


@lru_cache(maxsize=None)
def mid_counts(W, H):
    """Bucket counts of the MID_N case at a shape (n_extra 0, identity slots): the 90 % condition is asserted on these."""
    inp = sort_inputs(Geo(W, H), MID_N, 0, False)
    return np.bincount(sort_key(inp['x'], inp['y'], Geo(W, H)), minlength=n_buckets(W, H))
