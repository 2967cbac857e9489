"""The numpy model of the signal channels (include/die_hip.h die_signal_step): the field of K planes the agents of
a NeuralAutomataAgent(signal_channels=K) write and read.  One forward, with S the last layer's planes and F the field:

    1. occ   = the standing plane's occupancy: the cells of the stock / memory winners, alive slots only
    2. S     = stack(planes), F_k among them as plain fp32 planes          (the stack itself is torch's business in the tests)
    3. actions from S[0..2], the memory read-out from S[3 + K..]            (unchanged: tests/memory_model.py)
    4. E_k[c] = occ[c] ? deposit * S[3 + k][c] : +0
       F_k   <- (1 - decay) * gaussian(F_k + E_k, sigma, mode='wrap', truncate=4)

`update` is rule 4 in float64 (sigma, decay and deposit are the float32 numbers the library receives, widened); `emulate` the same
in fp32 in the kernels' order: one multiply, one add, the x pass (axis 0) then the y pass, each the centre tap times the cell and
then the symmetric pairs from the outermost inwards as fused multiply-adds, then one multiply by fp32(1 - decay).  `bound` is the
error the GPU test allows; the cases of that test are stated here so that the CPU test runs `emulate` over the very same grid."""
import numpy as np

from tests import stock_plane_model as S

f32 = np.float32
MAX_CHANNELS, MAX_RADIUS = 8, 8


def radius(sigma) -> int:
    """scipy's int(truncate * sigma + .5) with truncate 4, from the float32 sigma the library receives."""
    return int(4.0 * float(f32(sigma)) + 0.5)


def taps(sigma) -> np.ndarray:
    """The 2 R + 1 normalised gaussian weights in float64 (scipy.ndimage._gaussian_kernel1d; the kernels round them to fp32)."""
    s, R = float(f32(sigma)), radius(sigma)
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-0.5 / (s * s) * k * k)
    return w / w.sum()


def gaussian(a: np.ndarray, sigma) -> np.ndarray:
    """The separable periodic gaussian of the last two axes in float64: axis -2 (x) first, then axis -1 (y), as scipy does.  np.roll
    wraps as often as it takes, so a field narrower than the radius is no special case."""
    w, R = taps(sigma), radius(sigma)
    out = np.asarray(a, dtype=np.float64)
    for axis in (-2, -1):
        acc = np.zeros_like(out)
        for k in range(-R, R + 1):
            acc += w[k + R] * np.roll(out, -k, axis=axis)
        out = acc
    return out


def emission(occ, planes, deposit) -> np.ndarray:
    """E of rule 4 in float64: (K, W, H) from the occupancy (W, H) and the stack's planes 3 .. 3 + K - 1."""
    return np.where(occ[None], float(f32(deposit)) * np.asarray(planes, dtype=np.float64), 0.0)


def update(F, occ, planes, deposit, sigma, decay) -> np.ndarray:
    """Rule 4 in float64: the field after one forward."""
    return (1.0 - float(f32(decay))) * gaussian(np.asarray(F, dtype=np.float64) + emission(occ, planes, deposit), sigma)


def bound(F, occ, planes, deposit, sigma, decay) -> np.ndarray:
    """What |device - update| may be, cell by cell: 1e-5 (1 - decay) G(|F + E|) + 1e-7 — the project's fp32 diffusion constants, on the
    magnitude the summation error scales with (mixed signs cancel in the value, not in the error)."""
    mag = np.abs(np.asarray(F, dtype=np.float64) + emission(occ, planes, deposit))
    return 1e-5 * (1.0 - float(f32(decay))) * gaussian(mag, sigma) + 1e-7


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 numbers is exact in float64, the sum is rounded there and then to fp32."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(f32)


def _pass32(x, w, R, axis):
    t = (f32(w[R]) * x).astype(f32)                                   # the centre …
    for k in range(R):                                                # … then the pairs, outermost first
        pair = (np.roll(x, R - k, axis=axis) + np.roll(x, -(R - k), axis=axis)).astype(f32)
        t = _fma(pair, f32(w[k]), t)
    return t


def emulate(F, occ, planes, deposit, sigma, decay) -> np.ndarray:
    """Rule 4 as the kernels compute it, in fp32 and in their order."""
    w, R = taps(sigma).astype(f32), radius(sigma)
    e = np.where(occ[None], (f32(deposit) * np.asarray(planes, dtype=f32)).astype(f32), f32(0.0)).astype(f32)
    x = (np.asarray(F, dtype=f32) + e).astype(f32)
    keep = f32(1.0 - float(f32(decay)))
    return (_pass32(_pass32(x, w, R, -2), w, R, -1) * keep).astype(f32)


def occupancy_of(W: int, H: int, agents: np.ndarray) -> np.ndarray:
    """Rule 1 for a (4, N) agents array as `to_numpy()` returns it."""
    return S.stock_winners(W, H, S.q32_words(agents[0]), S.q32_words(agents[1]), agents[2] > 0)[0]


def standing_words(occ, epoch: int, rs) -> np.ndarray:
    """A standing plane with exactly `occ` occupied at `epoch`: arbitrary slot ids and stocks in the occupied words, and on a third
    of the empty cells a word of the epoch before — somebody stood there one build ago, nobody does now."""
    W, H = occ.shape
    slots = rs.randint(0, 1000, (W, H))
    stocks = (rs.rand(W, H) - 0.3).astype(f32)
    words = np.zeros((W, H), dtype=np.uint64)
    words[occ] = S.encode(epoch, slots, stocks)[occ]
    stale = ~occ & (rs.rand(W, H) < 1 / 3)
    words[stale] = S.encode((epoch - 2) % S.EPOCH_MAX + 1, slots, stocks)[stale]
    return words


# ---- the grid of tests/test_gpu_signal.py::test_kernel_against_the_model, run through `emulate` in tests/test_signal_model_cpu.py ----
SHAPES = [(3, 8), (5, 248), (7, 252), (17, 257)]      # narrower than the radius; one strip; a second strip of one lane; H % 4 != 0
SIGMAS = [0.25, 0.5, 1.0, 1.5]                        # radius 1, 2, 4, and 6 (the LDS-tiled kernel)
CHANNELS = [1, 3]
DEPOSIT, DECAY = 0.75, 0.1


def case(W: int, H: int, K: int, seed: int = 0):
    """(F (K, W, H), occ (W, H), planes (K, W, H)): mixed-sign field values on about 60 % of the cells, about 15 % of the cells
    occupied, emissions in [-1, 1]."""
    rs = np.random.RandomState(1000 * W + H + 7 * K + seed)
    F = (rs.uniform(-2, 2, (K, W, H)) * (rs.rand(K, W, H) < 0.6)).astype(f32)
    occ = rs.rand(W, H) < 0.15
    planes = np.tanh(rs.randn(K, W, H) * 2).astype(f32)
    return F, occ, planes
