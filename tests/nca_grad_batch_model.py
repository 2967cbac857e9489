"""A numpy model of how die_nca_backward_batch folds the tiles' partial rows into the (C, P) gradient (tests/test_nca_grad_batch_cpu.py).

The first launch of a layer leaves workspace[r][tile][nw] fp32: replica r's partial row of every 16 x 64 tile, tile = row of tiles *
tiles per row + column.  The second launch runs one thread per (candidate c, weight j): it adds, in float64, the rows of the
candidate's E replicas r = c * E + e — episode e = 0 .. E - 1 outermost, tile index ascending inside — and rounds to fp32 once."""
import numpy as np

TX, TY = 16, 64                      # the kernels' tile (die_nca.h NCA_TX, NCA_TY)
MAX_ROW = 4 * 4 * 7 * 7              # the widest layer's cout * cin * k * k


def tiles(W: int, H: int) -> int:
    return -(-W // TX) * -(-H // TY)


def workspace_bytes(W: int, H: int, replicas: int, n_layers: int) -> int:
    """die_nca_backward_batch_workspace_bytes: the partial rows of the widest layer, then the planes the gradient travels through."""
    if W < 1 or H < 1 or not 1 <= replicas <= 64 or not 1 <= n_layers <= 8:
        return -1
    return 4 * (replicas * tiles(W, H) * MAX_ROW + min(n_layers - 1, 2) * replicas * 4 * W * H)


def fold_stand_alone(part: np.ndarray) -> np.ndarray:
    """die_conv2d_backward's second launch: part (tiles, nw) fp32 -> (nw,) fp32, tile-index order in float64."""
    s = np.zeros(part.shape[1], dtype=np.float64)
    for t in range(part.shape[0]):
        s = s + part[t].astype(np.float64)
    return s.astype(np.float32)


def fold_batch(part: np.ndarray, episodes: int) -> np.ndarray:
    """part (R, tiles, nw) fp32 -> (R / E, nw) fp32 in the device's order."""
    R, T, nw = part.shape
    assert R % episodes == 0
    out = np.empty((R // episodes, nw), dtype=np.float32)
    for c in range(R // episodes):
        s = np.zeros(nw, dtype=np.float64)
        for e in range(episodes):
            for t in range(T):
                s = s + part[c * episodes + e, t].astype(np.float64)
        out[c] = s.astype(np.float32)
    return out
