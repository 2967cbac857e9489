"""The numpy model of the stock channel (include/die_hip.h die_stock_plane): the plane a NeuralAutomataAgent built
with `with_stock_channel=True` senses as its last observation channel, and the words the device keeps it in.

    S = zeros((W, H), float32)
    for n in ascending slot id, alive slots only:
        S[cell(x_n), cell(y_n)] = agent_food[n]

cell() is the library's nearest label of linspace(0, 1, n) to X / 2^32 for a Q0.32 coordinate word X: (X (n - 1) + 2^31) >> 32.
Several alive agents on one cell: the highest slot id wins (numpy's last writer).  Dead slots contribute nothing; negative and
denormal stocks keep their bits; the plane is fp32 whatever the field dtype."""
import numpy as np

EPOCH_SHIFT, EPOCH_MAX, SLOT_MASK = 27, 31, 0x07FFFFFF


def q32_words(v) -> np.ndarray:
    """Coordinates in [0, 1) as they come back from `to_numpy()` (X / 2^32, exact in float64) -> the uint32 words X."""
    return np.round(np.asarray(v, dtype=np.float64) * 4294967296.0).astype(np.uint64).astype(np.uint32)


def cell(X, n: int) -> np.ndarray:
    """The cell of Q0.32 words `X` (uint32) on an axis of n cells."""
    X = np.asarray(X, dtype=np.uint64)
    return ((X * np.uint64(n - 1) + np.uint64(1 << 31)) >> np.uint64(32)).astype(np.int64)


def stock_winners(W: int, H: int, x, y, alive):
    """(occupied (W, H) bool, slot (W, H) int64: the winning slot id, -1 on an empty cell).  x, y: uint32 words in SLOT order."""
    slot = np.full((W, H), -1, dtype=np.int64)
    ix, iy = cell(x, W), cell(y, H)
    for n in range(len(ix)):                                       # ascending slot id: the last writer wins
        if alive[n]:
            slot[ix[n], iy[n]] = n
    return slot >= 0, slot


def stock_plane(W: int, H: int, x, y, alive, agent_food) -> np.ndarray:
    """The (W, H) float32 plane of the Semantics.  x, y: uint32 words; alive, agent_food: per slot, all in SLOT order."""
    food = np.asarray(agent_food, dtype=np.float32)
    occ, slot = stock_winners(W, H, x, y, alive)
    S = np.zeros((W, H), dtype=np.float32)
    S[occ] = food[slot[occ]]
    return S


def stock_plane_of(W: int, H: int, agents: np.ndarray) -> np.ndarray:
    """The plane of a (4, N) agents array as `to_numpy()` returns it (x, y as fractions of the unit square)."""
    return stock_plane(W, H, q32_words(agents[0]), q32_words(agents[1]), agents[2] > 0, agents[3])


def decode(words, epoch: int):
    """A plane of uint64 stock words read at `epoch` -> (occupied bool, slot id int64 (-1 where empty), payload bits uint32
    (0 where empty), tag int64 of every word whatever the epoch)."""
    w = np.asarray(words).view(np.uint64) if np.asarray(words).dtype != np.uint64 else np.asarray(words)
    hi = (w >> np.uint64(32)).astype(np.uint64)
    tag = (hi >> np.uint64(EPOCH_SHIFT)).astype(np.int64)
    occ = tag == epoch
    slot = np.where(occ, (hi & np.uint64(SLOT_MASK)).astype(np.int64) - 1, -1)
    bits = np.where(occ, (w & np.uint64(0xFFFFFFFF)).astype(np.uint32), np.uint32(0)).astype(np.uint32)
    return occ, slot, bits, tag


def encode(epoch: int, slot, agent_food) -> np.ndarray:
    """The word die_claim(epoch, slot id, float bits of agent_food)."""
    bits = np.asarray(agent_food, dtype=np.float32).view(np.uint32).astype(np.uint64)
    hi = (np.uint64(epoch) << np.uint64(EPOCH_SHIFT)) | (np.asarray(slot).astype(np.uint64) + np.uint64(1))
    return (hi << np.uint64(32)) | bits
