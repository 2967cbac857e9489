"""The host model of the order table (tests/order_model.py) on hand-made populations: what tests/test_gpu_crowds.py holds the
device's table to, checked against the specification case by case.  No GPU."""
import numpy as np
import pytest

from tests import order_model as M


@pytest.mark.parametrize('n,want', [(0, 7), (1, 6), (512, 6), (513, 5), (1024, 5), (1025, 4), (1536, 4), (1537, 3), (2048, 3),
                                    (2049, 2), (2560, 2), (2561, 1), (3072, 1), (3073, 0), (3584, 0), (3585, 0), (100000, 0)])
def test_class_boundaries(n, want):
    assert M.order_class(n) == want
    assert (M.rounds(n) >= M.CROWDED_ROUNDS) == (n > 1536)


def test_band_tiles_walk_rows_of_tiles():
    # nty = 16: bands of two tile columns; band 3 holds columns 6 and 7 of every row of tiles
    assert M.band_tiles(4, 16, 3).tolist() == [6, 7, 22, 23, 38, 39, 54, 55]
    t = M.band_order(8, 16)
    assert sorted(t.tolist()) == list(range(128))


def _world(ntx, nty, crowd):
    """Populations: 10 agents on every tile, `crowd` = {tile: n}."""
    pop = np.full(ntx * nty, 10, dtype=np.int64)
    for t, n in crowd.items():
        pop[t] = n
    return pop


def test_ties_keep_band_order_and_classes_sort():
    ntx, nty = 8, 16                                     # 128 tiles: bands of 16, threshold 3 crowded tiles
    b0 = M.band_tiles(ntx, nty, 0)
    # band 0: two of class 1 (later one first in band order must stay first), one of class 0 behind them, one of class 3
    crowd = {b0[2]: 2600, b0[5]: 1600, b0[9]: 2700, b0[12]: 3100}
    pop = _world(ntx, nty, crowd)
    assert M.crowded_tiles(pop, ntx, nty) == 4 and M.is_sorted(pop, ntx, nty)
    got = M.order_table(pop, ntx, nty)
    rest = [t for t in b0.tolist() if t not in crowd]
    assert got[:16].tolist() == [b0[12], b0[2], b0[9], b0[5]] + rest
    assert np.array_equal(got[16:], M.band_order(ntx, nty)[16:])    # the other bands: all ties, band order


@pytest.mark.parametrize('ntx,nty,blen', [(8, 16, 16), (64, 64, 512), (96, 64, 768), (160, 64, 1280)])
def test_only_the_last_span_is_sorted(ntx, nty, blen):
    q0, ln = M.last_span(ntx, nty)
    assert q0 + ln == blen and ln == min(blen, 512) and q0 == max(blen - 512, 0)
    b = [M.band_tiles(ntx, nty, j) for j in range(8)]
    crowd = {}
    for j in range(8):                                   # the most crowded tile of every band ahead of its last span (when there is one),
        if q0 > 0:                                       # a tile of class 0 at the very end of it
            crowd[b[j][q0 - 1]] = 4000
        crowd[b[j][-1]] = 3500
        for k in range(ln // 40 + 1):                    # enough crowded tiles for the threshold
            crowd.setdefault(b[j][q0 + 2 * k], 1600)
    pop = _world(ntx, nty, crowd)
    assert M.is_sorted(pop, ntx, nty)
    got = M.order_table(pop, ntx, nty)
    for j in range(8):
        band = got[j * blen:(j + 1) * blen]
        assert np.array_equal(band[:q0], b[j][:q0]), 'the tiles ahead of the last span keep the band order'
        assert sorted(band[q0:].tolist()) == sorted(b[j][q0:].tolist())
        assert band[q0] == b[j][-1], 'the class-0 tile of the last span comes first'
        cls = M.order_class(pop[band[q0:]])
        assert (np.diff(cls) >= 0).all()


@pytest.mark.parametrize('ntx,nty', [(8, 16), (96, 64), (64, 64)])
def test_threshold_met_and_one_short(ntx, nty):
    q0, ln = M.last_span(ntx, nty)
    need = -(-M.MIN_CROWDED * 8 * ln // 4096)            # ceil: 3 of 128 tiles, 96 of 8 · 512
    b = [M.band_tiles(ntx, nty, j)[q0:] for j in range(8)]
    tiles = [b[k % 8][-1 - k // 8] for k in range(need)]  # crowded tiles at the ends of the spans: sorting moves them
    for n_crowded, want in ((need, True), (need - 1, False)):
        pop = _world(ntx, nty, {t: 1537 for t in tiles[:n_crowded]})
        pop[b[0][0]] = 1536                              # four rounds less one agent: not crowded, but a class of its own
        assert M.crowded_tiles(pop, ntx, nty) == n_crowded
        assert M.is_sorted(pop, ntx, nty) == want
        got = M.order_table(pop, ntx, nty)
        if want:
            first = [t for k, t in enumerate(tiles[:n_crowded]) if k % 8 == 0][-1]      # band 0's crowded tile earliest in band order
            assert got[q0] == first and not np.array_equal(got, M.band_order(ntx, nty))
        else:
            assert np.array_equal(got, M.band_order(ntx, nty)), 'below the threshold every band keeps the band order'
    if ntx * nty == 128:
        assert need == 3


def test_crowded_tiles_ahead_of_the_last_span_do_not_count():
    ntx, nty = 96, 64                                    # bands of 768: q < 256 lies ahead of the last span
    q0, _ = M.last_span(ntx, nty)
    crowd = {M.band_tiles(ntx, nty, j)[q]: 3000 for j in range(8) for q in range(q0)}
    pop = _world(ntx, nty, crowd)
    assert M.crowded_tiles(pop, ntx, nty) == 0 and not M.is_sorted(pop, ntx, nty)
    assert np.array_equal(M.order_table(pop, ntx, nty), M.band_order(ntx, nty))
