"""Host model of the tile-binned step's order table (die_amd/csrc/die_pic.hip `k_pic_order`, include/die_hip.h `die_pic.order`),
written from its specification in the kernel's comments, not from the kernel:

- the world's tiles are cut into 8 XCD bands of wb = nty / 8 tile columns each; band j's q-th tile is (q // wb)·nty + j·wb + q % wb
  (rows of tiles walked one after the other), and the band occupies entries [j·blen, (j + 1)·blen) of the table, blen = wb·ntx
- only the band's last span, q ≥ max(blen − 512, 0), is ever out of band order
- a tile of population n costs rounds(n) = ceil(ceil(n / 64) / 8) 8-wave rounds; its class is 7 − min(rounds, 7) (0: the most
  crowded); inside the last span the tiles are sorted by class, stable (band order among equals)
- the spans are sorted, all eight of them, iff crowded · 4096 ≥ 96 · 8 · len, where `crowded` counts the tiles of four rounds and more
  in the last spans of all eight bands together and len is the length of one last span; otherwise every band keeps its band order."""
import numpy as np

SPAN = 512             # PIC_ORDER_SPAN
MIN_CROWDED = 96       # PIC_ORDER_MIN_CROWDED: crowded tiles per 4 096 of the eight last spans' tiles
CROWDED_ROUNDS = 4


def rounds(n):
    n = np.asarray(n, dtype=np.int64)
    return -(-(-(-n // 64)) // 8)


def order_class(n):
    return 7 - np.minimum(rounds(n), 7)


def band_tiles(ntx, nty, j):
    wb = nty // 8
    q = np.arange(wb * ntx)
    return (q // wb) * nty + j * wb + q % wb


def last_span(ntx, nty):
    """(q0, len): the first index of a band's last span and its length."""
    blen = (nty // 8) * ntx
    q0 = max(blen - SPAN, 0)
    return q0, blen - q0


def crowded_tiles(pop, ntx, nty):
    q0, _ = last_span(ntx, nty)
    pop = np.asarray(pop)
    return int(sum((rounds(pop[band_tiles(ntx, nty, j)[q0:]]) >= CROWDED_ROUNDS).sum() for j in range(8)))


def is_sorted(pop, ntx, nty):
    _, ln = last_span(ntx, nty)
    return crowded_tiles(pop, ntx, nty) * 4096 >= MIN_CROWDED * 8 * ln


def order_table(pop, ntx, nty):
    """The table k_pic_order builds from `pop` (populations per tile, index tx·nty + ty): int64 array of ntx·nty tiles."""
    assert nty % 8 == 0 and len(pop) == ntx * nty
    pop = np.asarray(pop)
    q0, _ = last_span(ntx, nty)
    sort = is_sorted(pop, ntx, nty)
    bands = []
    for j in range(8):
        band = band_tiles(ntx, nty, j)
        if sort:
            tail = band[q0:]
            band = np.concatenate([band[:q0], tail[np.argsort(order_class(pop[tail]), kind='stable')]])
        bands.append(band)
    return np.concatenate(bands)


def band_order(ntx, nty):
    return np.concatenate([band_tiles(ntx, nty, j) for j in range(8)])
