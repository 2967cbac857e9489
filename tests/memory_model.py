"""The numpy model of a NeuralAutomataAgent's memory channels (include/die_hip.h die_memory_planes /
die_gather_memory), on the stock channel's winners (tests/stock_plane_model.py):

    occ, win = stock_winners(W, H, x, y, alive)                      # alive slots only, the highest slot id on a shared cell
    P_j[c]      = mem[j][win[c]] if occ[c] else +0.0f                # the expand: fp32 planes, bits preserved
    mem[j][id_n] = S[3 + j][cell_n] if alive_n else +0.0f            # the read-out: every stored slot, no coefficient

Everything is moved as uint32 words, so negative zero, denormals and NaN payloads keep their bits.  `mem` is indexed by SLOT ID;
x, y, alive are given in SLOT order (a storage order plus its slot array is brought there by `to_slot_order`)."""
import numpy as np

from tests import stock_plane_model as S


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def to_slot_order(values, slot) -> np.ndarray:
    """Storage order -> slot order along the last axis (storage entry j holds slot `slot[j]`; None: identity)."""
    values = np.asarray(values)
    if slot is None:
        return values
    out = np.empty_like(values)
    out[..., np.asarray(slot, dtype=np.int64)] = values
    return out


def expand(W: int, H: int, x, y, alive, mem) -> np.ndarray:
    """Steps 1 and 2: the (M, W, H) float32 planes of an (M, N) memory.  x, y: uint32 words; all per slot, in SLOT order."""
    words = bits(mem)
    occ, win = S.stock_winners(W, H, x, y, alive)
    out = np.zeros((words.shape[0], W, H), dtype=np.uint32)
    for j in range(words.shape[0]):
        out[j][occ] = words[j][win[occ]]
    return out.view(np.float32)


def gather(W: int, H: int, x, y, alive, planes) -> np.ndarray:
    """Step 5: the (M, N) float32 memory read out of the (M, W, H) planes `planes` (the stack's planes 3..)."""
    words = bits(planes)
    ix, iy = S.cell(x, W), S.cell(y, H)
    out = np.zeros((words.shape[0], len(ix)), dtype=np.uint32)
    live = np.asarray(alive) > 0
    out[:, live] = words[:, ix[live], iy[live]]
    return out.view(np.float32)


def expand_of(W: int, H: int, agents: np.ndarray, mem) -> np.ndarray:
    """`expand` for a (4, N) agents array as `to_numpy()` returns it (x, y as fractions of the unit square, slot order)."""
    return expand(W, H, S.q32_words(agents[0]), S.q32_words(agents[1]), agents[2] > 0, mem)


def gather_of(W: int, H: int, agents: np.ndarray, planes) -> np.ndarray:
    return gather(W, H, S.q32_words(agents[0]), S.q32_words(agents[1]), agents[2] > 0, planes)
