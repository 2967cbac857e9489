"""TEST INFRASTRUCTURE ONLY: the shapes and sizes of the mid-size batched tests, in one place for the GPU tests that run them
(tests/test_gpu_batch_midsize.py, the large-n tests of tests/test_gpu_births.py and tests/test_gpu_stock.py) and for the CPU
module that recomputes why each was chosen (tests/test_batch_midsize_cpu.py).  numpy only."""
import numpy as np

from tests import stock_plane_model as M

# name: (replicas, W, H).  R·W·H crosses a step of rows_per_wave (2^19, 2^21, 2^23) that W·H alone does not; W is no multiple of
# the batch's rows per wave; H % 4 == 0 and H > 496; every replica stays below Env.PIC_MIN_CELLS, so the batched regime is taken.
SHAPES = {'S': (2, 514, 512), 'M': (2, 1028, 1024), 'L': (3, 1676, 1672)}

# die_agent_births: one workgroup past the rank pass's 256-wide sum, one chunk past the 512-workgroup cap, a longer chunk loop,
# and (with every second slot a parent) more pairs than the spawn grid's 4096 x 256 threads
BIRTH_NS = (65537, 131073, 262145, 2097665)
BIRTH_PATTERNS = ('interleaved at random', 'free slots before the parents', 'more parents than free', 'equal counts')
BIRTH_BATCH_NS = (131073, 65537, 300)           # one call: stride 131 073

# die_stock_plane: more slots than the grid's 8192 x 256 threads on a plane small enough that most cells are shared
STOCK_N = 2097665
STOCK_PLANE = (256, 256)
STOCK_BATCH_N = (STOCK_N, 300)


def stock_world(W, H, N, rs):
    """(x, y uint32 words, alive uint8, agent_food float32) of N slots in slot order, about half of them alive."""
    x = rs.randint(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    y = rs.randint(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    alive = (rs.rand(N) < 0.5).astype(np.uint8)
    food = (0.05 + rs.rand(N)).astype(np.float32)
    return x, y, alive, food


def stock_winners_fast(W, H, x, y, alive):
    """stock_plane_model.stock_winners without its Python loop (2 M slots): the highest alive slot id of every cell.
    tests/test_batch_midsize_cpu.py checks it against the model's loop."""
    idx = np.nonzero(np.asarray(alive) != 0)[0]
    cells = M.cell(x, W)[idx] * H + M.cell(y, H)[idx]
    slot = np.full(W * H, -1, dtype=np.int64)
    np.maximum.at(slot, cells, idx)
    slot = slot.reshape(W, H)
    return slot >= 0, slot


def stock_plane_fast(W, H, x, y, alive, agent_food):
    """stock_plane_model.stock_plane on the fast winners."""
    occ, slot = stock_winners_fast(W, H, x, y, alive)
    S = np.zeros((W, H), dtype=np.float32)
    S[occ] = np.asarray(agent_food, dtype=np.float32)[slot[occ]]
    return S
