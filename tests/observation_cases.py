"""Cases for the kernels that produce what an agent or a viewer sees (tests/test_observation_cases_cpu.py holds the models below
against scipy, matplotlib and the oracle and shows that the cases are sharp; tests/test_gpu_observation_domain.py runs the kernels
against the models).  numpy and oracle.cpu_ref only.

    die_sense_mask        ceil(round(gaussian(agents, sigma, 'nearest'), decimals)): two float64 passes, axis 0 then axis 1
    die_render_frames     the medium image (occ, food, chem), its uint8 form, the agent trace and its colormap image
    die_gradient_render   0.5 (stack(gx, gy, 0) + 1) of the normalised, clipped np.gradient field

Every model takes `bug=`: ONE planted error at a time, which the case list must tell from the true model (CPU test, part 6).

The sense mask is a threshold, so its cases carry a CONDITION: the reference value g of every cell keeps |g - 0.5 10^-d| >= 2^-40.
Two passes of at most 33 float64 multiply-adds on values <= 1 move a sum by about 2^-46 at the most, so no cell's side of the
threshold depends on the order of summation or on FMA contraction, and the mask is compared bit for bit."""
import functools

import numpy as np

from oracle import cpu_ref as R

OWNER_EPOCH_SHIFT, OWNER_EPOCH_MAX, OWNER_SLOT_MASK = 27, 31, 0x07FFFFFF      # die_amd/_lib.py (the GPU test asserts they agree)
GUARD = 64                                   # elements of NaN (floats) or 0xA5 (bytes) before and after every device output
GRID_BLOCKS, BLOCK = 8192, 256               # the kernels' grid cap: beyond GRID_BLOCKS * BLOCK cells the grid-stride loop trips twice
BIG_SHAPE = (1448, 1449)                     # 2 098 152 cells: the smallest near-square shape above 2 097 152

f32 = np.float32


def below32(v):
    """The fp32 value just below v (sigma crosses the C ABI as a float)."""
    return float(np.nextafter(f32(v), f32(0)))


# ---------------------------------------------------------------------------------------------------------------- claim words
def claim_words(occ, epoch, rs):
    """Raw int64 claim words (DeviceMedium.owner_slots shows the layout: bits 59..63 the epoch tag, 32..58 slot + 1, 0..31 the
    fp32 bits of a deposit).  Occupied cells carry `epoch`; EVERY empty cell carries a stale word — tag epoch - 1, epoch + 1
    (wrapped into 1..31) or 0 — and all words carry non-zero slot and deposit bits."""
    occ = np.asarray(occ, dtype=bool)
    assert 1 <= epoch <= OWNER_EPOCH_MAX
    stale = np.array([epoch - 1, epoch % OWNER_EPOCH_MAX + 1, 0], dtype=np.uint64)
    tag = np.where(occ, np.uint64(epoch), stale[rs.randint(0, 3, occ.shape)])
    slot = rs.randint(1, OWNER_SLOT_MASK + 1, occ.shape).astype(np.uint64)
    dep = rs.randint(1, 1 << 32, occ.shape, dtype=np.uint64)
    words = (((tag << np.uint64(OWNER_EPOCH_SHIFT)) | slot) << np.uint64(32)) | dep
    assert (words[~occ] != 0).all() and ((words >> np.uint64(32 + OWNER_EPOCH_SHIFT) == np.uint64(epoch)) == occ).all()
    return words.view(np.int64)


def occupied(words, epoch, bug=None):
    """die_claim_occupied on raw words."""
    w = np.asarray(words).view(np.uint64)
    if bug == 'nonzero_is_occupied':
        return w != 0
    return (w >> np.uint64(32 + OWNER_EPOCH_SHIFT)) == np.uint64(epoch)


def occupancy(W, H, density, rs):
    occ = rs.rand(W, H) < density
    if not occ.any():
        occ[rs.randint(W), rs.randint(H)] = True
    return occ


# ---------------------------------------------------------------------------------------------------------------- 1. sense mask
SM_SHAPES = ((1, 1), (1, 40), (40, 1), (2, 2), (5, 3), (17, 33), (96, 80))
SM_SIGMAS = (0.125, 0.3, below32(0.375), 0.375, 1.0, 2.0, 3.0, 4.0, below32(4.125))
SM_RADII = (1, 1, 1, 2, 4, 8, 12, 16, 16)
SM_DECIMALS = (0, 1, 3, 6, 9)
SM_DENSITIES = (0.002, 0.02, 0.3)
SM_MARGIN = 2.0 ** -40
SM_TMP_TOL = 2.0 ** -46
# refused by the entry: (sigma, decimals, epoch) overrides
SM_BAD_SIGMAS = (0.0, -2.0, float('nan'), below32(0.125), 4.125)
SM_BAD_DECIMALS = (-1, 10)
BAD_EPOCHS = (0, OWNER_EPOCH_MAX + 1)


def sense_radius(sigma, bug=None):
    s = float(f32(sigma))
    return int(4.0 * s) if bug == 'radius_truncated' else int(4.0 * s + 0.5)


def sense_cases():
    """The product shapes x sigmas x decimals x densities x epochs, thinned: every shape takes every (sigma, decimals) pair — the
    narrow ones so that taps clamp on both sides at once at every radius — while density and epoch cycle with coprime periods, so
    that every (decimals, density, epoch) triple meets every shape.  The shape above the grid cap runs once, at radius 1."""
    out, i = [], 0
    for W, H in SM_SHAPES:
        for sigma in SM_SIGMAS:
            for d in SM_DECIMALS:
                out.append(dict(shape=(W, H), sigma=sigma, decimals=d, density=SM_DENSITIES[i % 3],
                                epoch=(1, OWNER_EPOCH_MAX)[i % 2], seed=i))
                i += 1
    out.append(dict(shape=BIG_SHAPE, sigma=0.3, decimals=3, density=0.02, epoch=OWNER_EPOCH_MAX, seed=i))
    return out


def sense_id(c):
    W, H = c['shape']
    return f"{W}x{H}-s{c['sigma']:.7g}-d{c['decimals']}-e{c['epoch']}"


@functools.lru_cache(maxsize=None)
def _sense_words(shape, density, epoch, seed):
    rs = np.random.RandomState(1000 + seed)
    occ = occupancy(*shape, density, rs)
    words = claim_words(occ, epoch, rs)
    words.setflags(write=False)
    return words


def sense_inputs(c):
    """The raw claim plane of a case (read-only, shared)."""
    return _sense_words(c['shape'], c['density'], c['epoch'], c['seed'])


def sense_weights(sigma, radius):
    """The taps as die_sense_mask builds them: exp(-0.5 / sigma^2 k k) in double on the fp32 sigma, normalised by their
    left-to-right sum."""
    s = float(f32(sigma))
    w = [float(np.exp(-0.5 / (s * s) * k * k)) for k in range(-radius, radius + 1)]
    total = 0.0
    for v in w:
        total += v
    return np.array([v / total for v in w])


def _sense_pass(x, w, axis, wrap):
    Rr = len(w) // 2
    x = np.moveaxis(x, axis, 0)
    n = x.shape[0]
    t = np.zeros_like(x)
    for k in range(-Rr, Rr + 1):                       # left to right, as the kernel sums
        idx = np.arange(n) + k
        idx = idx % n if wrap else np.clip(idx, 0, n - 1)
        t = t + w[k + Rr] * x[idx]
    return np.moveaxis(t, 0, axis)


def sense_model(words, epoch, sigma, decimals, bug=None):
    """(mask uint8, tmp float64) as k_sense_x / k_sense_y compute them.  bug: 'wrap_edges', 'radius_truncated',
    'nonzero_is_occupied', 'threshold_positive', 'decimals_minus', 'decimals_plus'."""
    occ = occupied(words, epoch, bug).astype(np.float64)
    Rr = sense_radius(sigma, bug)
    w = sense_weights(sigma, Rr)
    wrap = bug == 'wrap_edges'
    tmp = _sense_pass(occ, w, 0, wrap)
    t = _sense_pass(tmp, w, 1, wrap)
    d = decimals + {'decimals_minus': -1, 'decimals_plus': 1}.get(bug, 0)
    if bug == 'threshold_positive':
        return (t > 0).astype(np.uint8), tmp
    return (np.rint(t * 10.0 ** d) >= 1.0).astype(np.uint8), tmp


SENSE_BUGS = ('wrap_edges', 'radius_truncated', 'nonzero_is_occupied', 'threshold_positive', 'decimals_minus', 'decimals_plus')


def sense_reference(words, epoch, sigma, decimals):
    """(mask, g): the issue's reference — scipy as the reference's Env calls it (through skimage's defaults) — and the blurred
    value g before the rounding."""
    import scipy.ndimage
    occ = occupied(words, epoch).astype(np.float64)
    g = scipy.ndimage.gaussian_filter(occ, sigma=float(f32(sigma)), mode='nearest', truncate=4.0)
    return np.ceil(g.round(decimals)).astype(np.uint8), g


def sense_margin(g, decimals):
    return float(np.abs(g - 0.5 * 10.0 ** -decimals).min())


# ---------------------------------------------------------------------------------------------------------------- 4. frames
LUT_SIZES = (1, 2, 7, 10, 255, 256)
RENDER_SHAPE = (40, 56)
RENDER_SHAPES = ((1, 1), (5, 3), (40, 56))
TRACE_DECAY = 0.875
U8_EITHER = 2.0 ** -15


def make_lut(N):
    """(N + 3, 4) float32: N random colours, then three distinct under / over / bad rows — the layout of matplotlib's
    Colormap._lut after _init() (the CPU test builds the same table through ListedColormap)."""
    rs = np.random.RandomState(7000 + N)
    lut = rs.rand(N + 3, 4).astype(f32)
    assert len({r.tobytes() for r in lut}) == N + 3
    return lut


def trace_probes(N):
    """The fp32 trace values of the colormap test for a table of N colours: k/N and both neighbours, signed zeros, the ends,
    values far outside, infinities, NaN, and uniform values in [-0.1, 1.1] up to the cell count of RENDER_SHAPE."""
    k = (np.arange(N + 1) / N).astype(f32)
    special = np.array([0.0, -0.0, 1.0, 1e-30, -1e-30, 2.5, 8.0, -3.0, np.inf, -np.inf, np.nan], dtype=f32)
    fixed = np.concatenate([k, np.nextafter(k, f32(-1)), np.nextafter(k, f32(2)), special])
    cells = RENDER_SHAPE[0] * RENDER_SHAPE[1]
    assert cells - len(fixed) >= 1000
    rs = np.random.RandomState(7100 + N)
    out = np.concatenate([fixed, rs.uniform(-0.1, 1.1, cells - len(fixed)).astype(f32)])
    return out.reshape(RENDER_SHAPE)


def cmap_index(t32, N, bug=None):
    """Row of the (N + 3)-row table for fp32 trace values: xa = float64(t) N (exact), NaN -> bad (N + 2), xa == N -> N - 1,
    xa < 0 -> under (N), xa >= N -> over (N + 1), else floor(xa).  bug: 'no_top_rule', 'under_over_swapped', 'round'."""
    t32 = np.asarray(t32)
    assert t32.dtype == np.float32
    xa = t32.astype(np.float64) * N
    under, over = (N + 1, N) if bug == 'under_over_swapped' else (N, N + 1)
    if bug != 'no_top_rule':
        xa = np.where(xa == N, N - 1, xa)
    with np.errstate(invalid='ignore'):
        inner = np.rint(xa) if bug == 'round' else np.floor(xa)
        inner = np.where(np.isfinite(inner), inner, 0).astype(np.int64)
        idx = np.where(xa < 0, under, np.where(xa >= N, over, inner))
    return np.where(np.isnan(xa), N + 2, idx)


CMAP_BUGS = ('no_top_rule', 'under_over_swapped', 'round')


def trace_step(t32, decay, occ):
    """The two values `trace * decay + occ` may take in fp32: (product rounded, then the sum rounded; the fused multiply-add,
    rounded once).  Both float32.  (-0.0 * decay + 0.0 is +0.0 either way.)"""
    t = np.asarray(t32)
    assert t.dtype == np.float32
    o = np.asarray(occ, dtype=f32)
    with np.errstate(invalid='ignore', over='ignore'):
        two = t * f32(decay) + o
        one = (t.astype(np.float64) * float(f32(decay)) + o.astype(np.float64)).astype(f32)     # the product is exact in float64
    return two, one


def u8_exact(v):
    """v 255 + 0.5 after the clamp, in float64 (exact for fp16 and fp32 inputs: 24 + 8 bits)."""
    v = np.clip(np.asarray(v).astype(np.float64), 0.0, 1.0)
    return v * 255.0 + 0.5


def to_u8_model(v, bug=None):
    """to_u8 in float64.  bug: 'truncate' (no + 0.5), 'no_clamp' (the cast wraps)."""
    v = np.asarray(v).astype(np.float64)
    if bug == 'no_clamp':
        x = np.clip(v, -1e9, 1e9) * 255.0 + 0.5
        return (np.floor(x).astype(np.int64) & 255).astype(np.uint8)
    x = u8_exact(v)
    if bug == 'truncate':
        x = x - 0.5
    return np.floor(x).astype(np.uint8)


U8_BUGS = ('truncate', 'no_clamp')


def all_f16():
    """(finite, rest): a 248 x 256 plane holding every finite fp16 value once, and one of the same shape holding both
    infinities among a shuffle of the same values."""
    bits = np.arange(1 << 16, dtype=np.uint16)
    v = bits.view(np.float16)
    finite = v[np.isfinite(v)]
    assert finite.size == 248 * 256
    rest = np.random.RandomState(5).permutation(finite)
    rest[[3, 60000]] = [np.inf, -np.inf]
    return finite.reshape(248, 256).copy(), rest.reshape(248, 256).copy()


U8_F32_SHAPE = (40, 56)


def u8_f32_inputs():
    """(plane, either): the fp32 inputs of the uint8 test in one U8_F32_SHAPE plane and the mask of the cells where either
    neighbouring byte is accepted — the exact v 255 + 0.5 lies within 2^-15 of an integer WITHOUT being one (at an integer, as
    for 0.5, the fp32 arithmetic is exact).  Those are the (2 j + 1) / 510 planted here (but for 0.5 itself), and nothing else (asserted)."""
    rs = np.random.RandomState(11)
    k255 = (np.arange(256) / 255.0).astype(f32)
    dyadic = (rs.randint(0, 4097, 600) / 4096.0).astype(f32)                      # at most 12 significant bits, 0 .. 1
    dyadic[:3] = [0.5, 0.25, 1.0]
    outside = np.array([-0.0, -1e-30, -0.5, -3.0, 1.0000001, 1.5, 300.0, 1e30, np.inf, -np.inf], dtype=f32)
    halves = ((2 * np.arange(255) + 1) / 510.0).astype(f32)                       # the planted near-ties
    n = U8_F32_SHAPE[0] * U8_F32_SHAPE[1] - (k255.size + dyadic.size + outside.size + halves.size)
    plane = np.concatenate([k255, dyadic, outside, halves, rs.uniform(0, 1, n).astype(f32)])
    planted = np.zeros(plane.size, dtype=bool)
    start = k255.size + dyadic.size + outside.size
    planted[start:start + halves.size] = halves != 0.5                            # (j = 127 is 0.5 itself: an exact integer)
    x = u8_exact(plane)
    dist = np.abs(x - np.rint(x))
    either = (dist > 0) & (dist <= U8_EITHER)
    assert np.array_equal(either, planted), 'accepted-either cells must be exactly the planted ones'
    return plane.reshape(U8_F32_SHAPE), either.reshape(U8_F32_SHAPE)


def field_plane(W, H, dtype, rs):
    """A food / chem plane for the `rgb` test: uniform values with negatives, values above 1, a subnormal, infinities and NaN."""
    p = rs.uniform(-0.5, 1.5, (W, H)).astype(dtype)
    flat = p.reshape(-1)
    sp = np.array([np.nan, np.inf, -np.inf, -0.0, 6e-8, 65504.0], dtype=dtype)
    n = min(flat.size, sp.size)
    flat[rs.permutation(flat.size)[:n]] = sp[:n]
    return p


# ---------------------------------------------------------------------------------------------------------------- 5. gradient image
GR_SHAPES = ((2, 2), (2, 9), (9, 2), (5, 3), (37, 24))
GR_CLIPS = (None, 0.0, 2.0 ** -11, 1e-5)
GR_TOL = 8 * 2.0 ** -24
GR_PATCH = (slice(4, 13), slice(4, 13))      # the flat patch of the 37 x 24 case, value 0.25, with one bump of 2^-10 in its middle
GR_BUMP = (8, 8)


def gradient_chem(W, H):
    """(chem float64 on the grid of multiples of 2^-10 in [0, 1], planted): `planted` marks the cells with |g| = 2^-11 exactly
    along one axis and 0 along the other — the four neighbours of the bump — on the shape that has room for the patch."""
    rs = np.random.RandomState(W * 101 + H)
    chem = rs.randint(0, 1025, (W, H)) / 1024.0
    planted = np.zeros((W, H), dtype=bool)
    if W >= 16 and H >= 16:
        chem[GR_PATCH] = 0.25
        i, j = GR_BUMP
        chem[i, j] += 2.0 ** -10
        for a, b in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
            planted[a, b] = True
    return chem, planted


def gradient_parts(chem, bug=None):
    """(gx, gy, norm) in float64: np.gradient's stencil written out — central differences halved, one-sided ones not."""
    c = np.asarray(chem, dtype=np.float64)

    def diff(a):
        g = np.empty_like(a)
        g[1:-1] = (a[2:] - a[:-2]) * 0.5
        side = 0.5 if bug == 'one_sided_halved' else 1.0
        g[0] = (a[1] - a[0]) * side
        g[-1] = (a[-1] - a[-2]) * side
        return g

    gx, gy = diff(c), diff(c.T).T
    return gx, gy, np.sqrt(gx * gx + gy * gy)


def gradient_image(chem, normalized=True, grad_clip=1e-5, bug=None):
    """die_gradient_render's image in float64: 0.5 (stack(gx, gy, 0) + 1); g / |g| with 0 / 0 -> 0 when `normalized`; the cells
    whose norm is below the fp32 value of `grad_clip` zeroed (None: no clip).  bug: 'one_sided_halved', 'clip_strict'."""
    gx, gy, norm = gradient_parts(chem, bug)
    if normalized:
        with np.errstate(divide='ignore', invalid='ignore'):
            gx, gy = np.nan_to_num(gx / norm), np.nan_to_num(gy / norm)
    if grad_clip is not None:
        clip = float(f32(grad_clip))
        keep = norm > clip if bug == 'clip_strict' else norm >= clip
        gx, gy = gx * keep, gy * keep
    return 0.5 * (np.stack([gx, gy, np.zeros_like(gx)], axis=-1) + 1.0)


GRADIENT_BUGS = ('one_sided_halved', 'clip_strict')


def gradient_ties(chem, grad_clip):
    """The cells whose norm is within 1e-6 relative of a positive clip (at clip 0 `>=` and `>` give the same image: a cell of
    norm 0 has no gradient to zero)."""
    if not grad_clip:
        return np.zeros(np.shape(chem), dtype=bool)
    clip = float(f32(grad_clip))
    return np.abs(gradient_parts(chem)[2] - clip) <= 1e-6 * clip


# ---------------------------------------------------------------------------------------------------------------- 2, 3. worlds
# W, H, slots, alive.  H % 4 == 0 (the fused launch applies) and not (the fallback).  At sigma 2 / 3 decimals an agent lights about 95
# cells, so a few agents leave a real share of these small fields hidden; the dead slots sense as well (core/agent/gradient.py has
# no alive masking) and mostly stand in the dark
MASKED_SHAPES = ((48, 40, 60, 16), (37, 23, 40, 8))
NCA_SHAPE = (48, 40, 60, 16)
ENV_SENSE_SIGMA, ENV_SENSE_DECIMALS = 2.0, 3                        # what Env._update_sense_mask passes (core/env.py:276-290)


def env_mask(agents_channel):
    """The oracle's mask of a world as booleans (RefEnv.sense_mask; the CPU test holds the two together)."""
    import scipy.ndimage
    a = np.asarray(agents_channel, dtype=np.float64)
    return np.ceil(scipy.ndimage.gaussian_filter(a, sigma=ENV_SENSE_SIGMA, mode='nearest', truncate=4.0).round(ENV_SENSE_DECIMALS)).astype(bool)
