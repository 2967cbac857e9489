"""Cases for the gaussian diffusion over its whole template grid (tests/test_diffuse_domain_cpu.py shows without a GPU that
the bounds below accuse nobody, tests/test_gpu_diffuse_domain.py runs the kernels against them).  numpy and oracle.cpu_ref only.

Two kernels of die_amd/csrc/die_env.hip carry every diffusion of the project:

    k_diffuse_rows<T, R, FUSED, WRAP>   the row sweep: wrap, radius 1..4, H % 4 == 0; strips of 248 columns (62 lanes x 4 cells
                                        between two halo lanes), two waves per workgroup, rows_per_wave rows per wave
    k_diffuse<T, R>                     the LDS kernel: everything else, R = 1..8, five boundary modes, 16 x 256 tiles

The reference is oracle.cpu_ref.diffuse_decay (scipy.ndimage.gaussian_filter in float64) on the float64 values of the inputs the
device gets, with sigma and decay carried as their fp32 values (the C ABI takes floats).

Bounds.  fp32: tests/test_gpu_parity.py's, |got - want| <= 1e-5 |want| + 1e-7.  fp16: DERIVED, not measured — the kernels
compute in fp32 and round once to half, so

    |got - want| <= 0.5 * spacing(float16(|want|)) + 1e-5 |want| + 1e-7

the half-ulp term being the rounding itself (it cannot be tighter), the rest the fp32 arithmetic's bound above.  `emulate` below
is that arithmetic in numpy, in the kernels' order; the CPU test holds it against both bounds on every case.

Inputs are non-negative and about 60 % dense, as the chem planes of the other tests are.  fp16 cases run at the scales 1 and
6e-6: at the second every input and output is a SUBNORMAL half (below 2^-14 = 6.1e-5), which a conversion that flushes would zero.
"""
import functools

import numpy as np

from oracle import cpu_ref as R

RTOL, ATOL = 1e-5, 1e-7                   # tests/test_gpu_parity.py: RTOL, and the atol of test_diffuse_decay_parity
DECAY = 0.1
MODES = ('wrap', 'nearest', 'reflect', 'mirror', 'constant')
GUARD = 64                                # elements of NaN before and after every dst plane of the GPU tests
F16_SCALES = (1.0, 6e-6)

# 1. the row sweep, direct (die_diffuse_decay, wrap): R = 1, 2, 3, 4, 4 — 0.375 and 0.875 sit ON the rounding edge of
#    int(4 sigma + .5) (4 sigma + .5 = 2.0 and 4.0 exactly).  Shapes (W, H): (1, 4) and (3, 8) have W < R rows (wrap_idx wraps more
#    than once) and, with R = 4, halo lanes that wrap onto the wave's own one or two groups of cells; H = 248 is exactly one strip
#    (lane 63 is the right halo lane and wraps to column 0); 252 leaves a second strip with ONE output lane; 500 puts a third strip
#    into a second workgroup whose other wave is idle.  Every W is odd: rows = min(rpw, W - x0) is ragged at rpw = 2.
ROWS_SIGMAS = (0.25, 0.375, 0.8, 0.875, 1.0)
ROWS_SHAPES = ((1, 4), (3, 8), (5, 248), (7, 252), (9, 500))

# 2. ragged rows at every other rows_per_wave (fp32, sigma 1.0).  rows_per_wave(W, H) is 2 below 2^19 cells, 4 from 2^19, 8 from
#    2^21, 16 from 2^23.  With H = 1024 = 2^10 (four whole strips and a fifth of 32 columns) the thresholds are W = 512, 2048, 8192,
#    each a multiple of its rpw; three rows further W % rpw = 3 at every one (515 % 4, 2051 % 8, 8195 % 16), so the last wave of
#    each column of workgroups has rows it sweeps and rows it must not touch.  At 0.6 % over the thresholds nothing usefully smaller reaches these rpw.
RAGGED_SIGMA = 1.0
RAGGED_SHAPES = ((515, 1024, 4), (2051, 1024, 8), (8195, 1024, 16))

# 3. the LDS kernel, direct (die_diffuse_decay_mode): R = 1..8, five modes.  (1, 1): n == 1 on both axes (mirror's period 2n - 2
#    is 0 there); (1, 7) and (3, 5): fields narrower than the radius, every reflection repeats; (16, 256): exactly one tile;
#    (17, 257): one past it on each axis, four workgroups, three of them nearly empty.
LDS_SIGMAS = (0.25, 0.5, 0.8, 1.0, 1.2, 1.5, 1.8, 2.1)
LDS_SHAPES = ((1, 1), (1, 7), (3, 5), (16, 256), (17, 257))

# 4. Env.step and 5. batched replicas: sigmas 0.25 and 1.0 are R = 1 and 4, the instantiations of the fused sweeps (FUSED = 1, with
#    and without the per-replica table) that no sigma in use (0.5, 0.8, 1.5) reaches
STEP_SIGMAS = (0.25, 1.0)
STEP_SHAPES = ((12, 252, 400, 300), (37, 24, 500, 300))         # W, H, slots, alive
BATCH_SHAPE = (12, 252)
BATCH_SIGMAS = (0.25, 0.5, 0.8, 1.0)


def radius(sigma):
    """The radius the library derives: scipy's int(4 sigma + .5) on the fp32 value of sigma."""
    return int(4.0 * float(np.float32(sigma)) + 0.5)


def rows_per_wave(W, H, replicas=1):
    cells = W * H * replicas
    return 16 if cells >= 1 << 23 else 8 if cells >= 1 << 21 else 4 if cells >= 1 << 19 else 2


def takes_row_sweep(W, H, sigma, mode='wrap'):
    """diffuse_decay_mode's choice of kernel (rows_kernel_applies)."""
    return mode == 'wrap' and radius(sigma) <= 4 and H % 4 == 0 and H >= 4 and W >= 1


def np_dtype(dtype):
    return {'f32': np.float32, 'f16': np.float16}[dtype]


def plane(W, H, dtype, scale=1.0, seed=0):
    """The input plane of a case, in the storage type: uniform [0, scale), about 40 % of the cells zero."""
    rs = np.random.RandomState((W * 1009 + H * 17 + seed) % (1 << 31))
    return (rs.rand(W, H) * (rs.rand(W, H) < 0.6) * scale).astype(np_dtype(dtype))


def oracle(chem, sigma, mode='wrap', decay=DECAY):
    return R.diffuse_decay(np.asarray(chem).astype(np.float64), float(np.float32(sigma)), float(np.float32(decay)), mode)


def bound(want, dtype):
    """The largest |got - want| a correct kernel may show, per cell."""
    a = np.abs(want)
    b = RTOL * a + ATOL
    if dtype == 'f16':
        b = b + 0.5 * np.spacing(a.astype(np.float16)).astype(np.float64)
    return b


def ratio(got, want, dtype):
    """max over the cells of error / bound: at most 1 for a correct kernel.  NaN (a cell never written) gives inf."""
    r = np.abs(np.asarray(got).astype(np.float64) - want) / bound(want, dtype)
    return float(np.where(np.isnan(r), np.inf, r).max())


# ---- the kernels' arithmetic in numpy (for the CPU test only)
def edge_index(n, Rr, mode):
    """edge_idx of die_env.hip for v = -R .. n + R - 1: the index that stands in for v, or -1 ('constant': a zero)."""
    v = np.arange(-Rr, n + Rr)
    inside = (v >= 0) & (v < n)
    if mode == 'wrap':
        out = v % n
    elif mode == 'nearest':
        out = np.clip(v, 0, n - 1)
    elif mode == 'reflect':                                   # d c b a | a b c d | d c b a
        m = v % (2 * n)
        out = np.where(m < n, m, 2 * n - 1 - m)
    elif mode == 'mirror':                                    # d c b | a b c d | c b a
        if n == 1:
            out = np.zeros_like(v)
        else:
            m = v % (2 * n - 2)
            out = np.where(m < n, m, 2 * n - 2 - m)
    elif mode == 'constant':
        out = np.full_like(v, -1)
    else:
        raise ValueError(mode)
    return np.where(inside, v, out)


def taps_f32(sigma):
    """The taps as the kernels get them: computed in double from the fp32 sigma, normalised, rounded to fp32."""
    s = float(np.float32(sigma))
    Rr = radius(sigma)
    k = np.arange(-Rr, Rr + 1)
    w = np.exp(-0.5 / (s * s) * k * k)
    return (w / w.sum()).astype(np.float32)


def _pass(x, w, axis, mode, fma):
    """One axis of the separable filter in fp32: the centre tap, then the symmetric pairs from the outermost inwards.  `fma`: the
    multiply-add contracted into one rounding, as the compiler is free to do (the fp32 product is exact in float64, so is the sum
    of it and an fp32 accumulator up to the final rounding)."""
    Rr = len(w) // 2
    x = np.moveaxis(x, axis, 0)
    n = x.shape[0]
    idx = edge_index(n, Rr, mode)
    pad = np.where((idx >= 0).reshape((-1,) + (1,) * (x.ndim - 1)), x[np.maximum(idx, 0)], np.float32(0))
    t = w[Rr] * pad[Rr:Rr + n]
    for k in range(Rr):
        pair = pad[k:k + n] + pad[2 * Rr - k:2 * Rr - k + n]
        if fma:
            t = (pair.astype(np.float64) * np.float64(w[k]) + t.astype(np.float64)).astype(np.float32)
        else:
            t = t + pair * w[k]
    assert t.dtype == np.float32
    return np.moveaxis(t, 0, axis)


def emulate(chem, sigma, decay, mode, dtype, fma=False):
    """(1 - decay) * G(chem) as k_diffuse and k_diffuse_rows compute it: fp32 throughout, axis 0 then axis 1, times `keep`, ONE
    rounding to the storage type.  Returns an array of that type."""
    w = taps_f32(sigma)
    keep = np.float32(1.0 - float(np.float32(decay)))
    x = np.asarray(chem).astype(np.float32)
    out = _pass(_pass(x, w, 0, mode, fma), w, 1, mode, fma) * keep
    return out.astype(np_dtype(dtype))


# ---- the list of cases the two files walk
def direct_cases():
    """Every direct call of the GPU file: dicts of group, dtype, sigma, mode, shape, scale."""
    out = []
    for dtype in ('f32', 'f16'):
        scales = (1.0,) if dtype == 'f32' else F16_SCALES
        for scale in scales:
            for sigma in ROWS_SIGMAS:
                for W, H in ROWS_SHAPES:
                    out.append(dict(group='rows', dtype=dtype, sigma=sigma, mode='wrap', shape=(W, H), scale=scale))
            for sigma in LDS_SIGMAS:
                for mode in MODES:
                    for W, H in LDS_SHAPES:
                        out.append(dict(group='lds', dtype=dtype, sigma=sigma, mode=mode, shape=(W, H), scale=scale))
    for W, H, _ in RAGGED_SHAPES:
        out.append(dict(group='ragged', dtype='f32', sigma=RAGGED_SIGMA, mode='wrap', shape=(W, H), scale=1.0))
    return out


@functools.lru_cache(maxsize=None)
def inputs(W, H, dtype, scale, sigma, mode):
    """(plane, oracle) of a case, computed once and shared; both read-only."""
    chem = plane(W, H, dtype, scale, seed=int(round(sigma * 1000)))
    want = oracle(chem, sigma, mode)
    chem.setflags(write=False)
    want.setflags(write=False)
    return chem, want
