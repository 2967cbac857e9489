"""Cases for the Gradient / Physarum forward pass (die_amd/csrc/die_forward.h `die_forward_agent_mem`) where its decisions are exact
ties, sit a derived margin off a threshold, or its inputs leave the O(1) range (tests/test_forward_ties_cpu.py checks the cases against
the oracle alone, tests/test_gpu_forward_ties.py runs the kernels on them).  numpy and oracle.cpu_ref only.

The world.  A lattice of 4 x 4-cell blocks, one agent per block at local cell (1, 1) (x = q32((4 bx + 1) / (W - 1))), chem inside a block
the ramp c0 + a (gx (i - 1) + gy (j - 1)) rounded to the storage type, food 0.25 everywhere.  With sense_offset = 0 the probe cell is the
agent's own and its four taps lie inside the block, so every slot is one independent case: (gx, gy, a, c0) and a float64 heading.
The oracle's direction `drads` is always taken from the STORED field (gradient_field + xy2polar in float64) and headings are placed
relative to it.  The two taps of an axis differ by less than a factor of two in every world here except the 2^126 one (c0 = 0: a doubling),
so the device's fp32 difference is exact and its gradient is the oracle's, but for the halving (see 4).

Groups.
  1  exact ties: axis-aligned, flat and sub-clip ramps; float64 headings drads + s b + w stepped by -3..+3 ulps around every threshold b.
     The device takes these decisions in float64 with the reference's operations: ZERO slots may differ.
  2  the same worlds through one Env.step, tile-binned against classic, plus agents on the world's first and last coordinates.
  3  generic directions, headings a margin m off each threshold.  Slots at m >= M must agree; M is derived below, not measured.
  4  chem amplitudes 2^-148 .. 2^126 (die_normalize2), both agent kinds, normalised and not.
  5  headings outside (-pi, pi] (set_state may hand them in): k pi/2 +- 1 ulp and 2000 uniform values in +-8 pi.

The margin M (group 3).  Off the axes the device decides on c = cd ux + sd uy = |u| cos(delta) and s = sd ux - cd uy = |u| sin(delta) in
fp32, (cd, sin) of the heading ROUNDED to fp32.  Against the float64 decision that costs

    the heading's rounding            H = 2^-24 hmax        (half an fp32 ulp is at most 2^-24 |h|; hmax = pi, 8 pi in group 5)
    the error of c (and of s)         E = 6 * 2^-23         one "ulp" = 2^-23, the relative spacing of fp32, |c| <= |u| = 1:
                                          2     each of cd, sd             (a good single-precision sincos)
                                          2     each of ux, uy             (a normalisation by one reciprocal square root)
                                          0.5   each product               -> (2 + 2 + 0.5) (|cd ux| + |sd uy|) <= 4.5, Cauchy-Schwarz
                                          0.5   the sum
                                          0.5   the rounded constant cos(theta), 0.5 its product with |u|

and an error E of cos moves the angle by E / |sin theta| (of sin: E / |cos theta|).  With a factor 2 of slack

    M(theta) = 2 (H + E / |sin theta|)     for x_turn and sense_rad          M(pi) = 2 (H + E / |cos pi|)     for the sign of s

(the linearisation needs M << theta: asserted by the CPU test).  The test on drads itself, |uy| <= tan(x_grad) ux, involves no heading:
five roundings (2 + 2 of ux, uy, 0.5 the constant, 0.5 the product) of a quantity x_grad large, M_grad = 2 * 6 * 2^-23 x_grad.
At the default parameters: M(x_turn = 0.0529) = 2.74e-5, M(sense = pi / 2) = 1.80e-6, M(pi) = 1.80e-6, M_grad = 1.43e-14.

Magnitudes (group 4).  The oracle works in float64 on the stored values, the device must give dx, dy within RTOL relative plus ONE fp32
denormal step absolute (scale = 1: the result itself may be denormal).  Cases whose expected action does not fit fp32 are dropped and
counted (`group4_drops`): none does at scale 1 (the largest expected |dx| is 2^126).
"""
import functools
import math
from fractions import Fraction

import numpy as np

from oracle import cpu_ref as R
from tests.physarum_pop_model import isclose_bound
from tests.test_gpu_parity import RTOL, f32, q32

B = 4                                              # cells per block edge
SHAPES = ((128, 96), (256, 192))                   # 768 and 3072 blocks; (128, 96) is the smallest shape the binned tests use
FOOD = 0.25
PI = math.pi

# (turn_angle, sense_angle, turn_tolerance): the default, tests/test_gpu_parity.py's 'wide', sense == turn, every angle seen
# (c_sense = -2), and x_turn = 0
PARAM_SETS = ((30, 90, 0.1), (35, 120, 0.05), (45, 45, 0.1), (22.5, 180, 0.2), (60, 60, 0.0))
GENERIC_SETS = (0, 1, 3)                           # group 3: the default, 'wide', and the one set in which |delta| = pi is seen
OUTSIDE_SETS = (0, 1)                              # group 5

EPS32 = 2.0 ** -23
E_C = 6 * EPS32
DENORM = 2.0 ** -149
GRID = 2.0 ** -51                                   # the ulp of pi
AMPLITUDES = tuple(2.0 ** e for e in (-148, -140, -127, -126, -60, 0, 60, 100, 126))
DROP_CAP = 0.05


class Consts:
    """What die_fill_fwd_args derives from the constructor arguments, in the same float64 operations."""

    def __init__(self, params):
        self.turn_angle, self.sense_angle, self.rtol = params
        self.turn_rad, self.sense_rad = math.radians(params[0]), math.radians(params[1])
        self.atol = self.turn_rad * self.rtol
        self.x_turn = isclose_bound(self.atol, 1e-2)
        self.x_grad = isclose_bound(1e-8, 1e-5)

    def kw(self):
        return dict(turn_angle=self.turn_angle, sense_angle=self.sense_angle, turn_tolerance=self.rtol)

    def margins(self, hmax=PI):
        """M per threshold (module docstring); sense_rad >= pi is no threshold (nothing is unseen)."""
        H = 2.0 ** -24 * hmax
        m = {'pi': 2 * (H + E_C), 'x_grad': 2 * E_C * self.x_grad}
        m['x_turn'] = 2 * (H + E_C / math.sin(self.x_turn)) if self.x_turn > 0 else math.inf
        m['sense'] = 2 * (H + E_C / abs(math.sin(self.sense_rad))) if self.sense_rad < PI else 0.0
        return m


def ulps(v, lo=-3, hi=3):
    """v stepped by lo..hi ulps (np.nextafter)."""
    out = []
    for k in range(lo, hi + 1):
        x = np.float64(v)
        for _ in range(abs(k)):
            x = np.nextafter(x, np.inf if k > 0 else -np.inf)
        out.append(float(x))
    return out


class World:
    """`fields`: (n, 4) rows (gx, gy, a, c0), one per block; the remaining blocks are flat (0, 0, 0, 1).  `headings` are set by the caller
    once `drads` is known; the padding keeps 0.5."""

    def __init__(self, fields, dtype='f32', normalized=True, grad_clip=1e-5, shape=None):
        fields = np.asarray(fields, dtype=np.float64).reshape(-1, 4)
        self.n = len(fields)
        self.W, self.H = shape or next(s for s in SHAPES if (s[0] // B) * (s[1] // B) >= self.n)
        W, H = self.W, self.H
        nbx, nby = W // B, H // B
        self.N = N = nbx * nby
        assert self.n <= N
        F = np.concatenate([fields, np.tile([0.0, 0.0, 0.0, 1.0], (N - self.n, 1))])
        self.fields, self.dtype, self.normalized, self.grad_clip = F, dtype, normalized, grad_clip
        i = np.arange(B) - 1.0
        gx, gy, a, c0 = (F[:, k, None, None] for k in range(4))
        block = c0 + a * (gx * i[None, :, None] + gy * i[None, None, :])
        block = block.astype(np.float32 if dtype == 'f32' else np.float16).astype(np.float64)
        assert np.isfinite(block).all()
        chem = block.reshape(nbx, nby, B, B).transpose(0, 2, 1, 3).reshape(W, H)
        k = np.arange(N)
        self.cx, self.cy = B * (k // nby) + 1, B * (k % nby) + 1
        self.agents = np.zeros((4, N))
        self.agents[0], self.agents[1] = q32(self.cx / (W - 1)), q32(self.cy / (H - 1))
        self.agents[2], self.agents[3] = 1.0, 0.5
        self.medium = np.stack([np.zeros((W, H)), np.full((W, H), FOOD), chem])
        self.medium[0][self.cx, self.cy] = 1.0
        with np.errstate(all='ignore'):
            G = R.gradient_field(chem, normalized, grad_clip)
        self.g = G[:, self.cx, self.cy]                                 # what the oracle's agent samples
        self.norm, self.drads = R.xy2polar(self.g[0], self.g[1])
        self.axis = (self.g[0] == 0) | (self.g[1] == 0)                 # the device's float64 branch (signed zeros included)
        self.headings = np.full(N, 0.5)

    def kw(self, consts=None, **over):
        """Constructor arguments of the device agent and of the oracle's alike."""
        kw = dict(scale=1.53 / (max(self.W, self.H) - 1), deposit=4.0, sense_offset=0.0, normalized_grad=self.normalized,
                  grad_clip=self.grad_clip)
        if consts is not None:
            kw.update(consts.kw())
        kw.update(over)
        return kw


def decisions(consts, drads, headings):
    """The lines of RefPhysarumAgent._choose_turn (core/agent/gradient.py:168-193) that decide: delta, und_grad, und_turn, unseen."""
    delta = R.renormalize_radians(headings - drads)
    return (delta, np.isclose(0, drads, rtol=1e-5), np.isclose(0, delta, rtol=1e-2, atol=consts.atol), np.abs(delta) > consts.sense_rad)


def threshold_margins(consts, drads, headings):
    """Distance of every slot from each threshold, {name: array}."""
    delta = np.abs(decisions(consts, drads, headings)[0])
    return {'x_turn': np.abs(delta - consts.x_turn), 'sense': np.abs(delta - consts.sense_rad), 'pi': PI - delta,
            'x_grad': np.abs(np.abs(drads) - consts.x_grad)}


def safe_slots(world, consts, hmax=PI):
    """Slots whose decisions the device must reproduce: the float64 branch, or every threshold at least its M away."""
    M, tm = consts.margins(hmax), threshold_margins(consts, world.drads, world.headings)
    ok = np.ones(world.N, dtype=bool)
    for name, m in tm.items():
        ok &= m >= M[name]
    return ok | world.axis


def expect(world, kind, kw, sign):
    """The oracle's forward from the world's set state: action (3, N), heading', deposit mask and 'undetermined' per slot."""
    N = world.N
    cls = R.RefPhysarumAgent if kind == 'physarum' else R.RefGradientAgent
    ref = cls(N, init_noise=np.ones((2, N)), **kw)
    ref._direction_rads = world.headings.copy()
    with np.errstate(all='ignore'):
        action = ref.forward((world.agents, world.medium), turn_sign=np.full(N, float(sign)))
    return dict(action=action, heading=np.array(ref._direction_rads), mask=np.array(getattr(ref, '_deposit_mask', np.ones(N)), dtype=bool),
                und=getattr(ref, 'last_undetermined', None))


@functools.lru_cache(maxsize=None)
def expected(key, kind, sign, kw_items):
    """`expect` for a cached world (key: the arguments of `world_of`), computed once and shared."""
    return expect(world_of(*key), kind, dict(kw_items), sign)


def heading_error(got, want):
    d = np.abs(R.renormalize_radians(np.asarray(got) - np.asarray(want)))
    return np.minimum(d, 2 * PI - d)


def slots_agree(world, got_action, got_heading, exp, scale, atol_xy=None, heading_tol=1e-9):
    """Per slot: the heading within heading_tol mod 2 pi (a wrong decision moves it by turn_rad or 2 turn_rad), the deposit
    deposit * food * {0.1 | 1.0} to RTOL, dx and dy within RTOL and atol_xy (default: test_physarum_forward_parity's 4e-7 scale)."""
    atol_xy = 4e-7 * abs(scale) if atol_xy is None else atol_xy
    want = exp['action']
    ok = heading_error(got_heading, exp['heading']) < heading_tol
    for c in (0, 1):
        ok &= np.abs(got_action[c] - want[c]) <= RTOL * np.abs(want[c]) + atol_xy
    ok &= np.abs(got_action[2] - want[2]) <= RTOL * np.abs(want[2])
    return ok


# ---------------------------------------------------------------- 1. exact ties
def tie_fields(dtype):
    """Axis ramps 0.75 / 1 / 1.25 and 0.5 / 1 / 1.5 (exact in fp16) in the four directions, the flat block, and sub-clip ramps
    2^-8 + 2^-18 (+-(i - 1) +- (j - 1)) (exact in fp16, |g| <= 1.42 * 2^-18 < grad_clip) in eight directions: the clip leaves SIGNED
    zeros and np.angle(-+0 -+0j) is 0 but for (-0, -0) -> pi."""
    f = []
    for g in (0.25, 0.5):
        f += [(g, 0, 1, 1), (-g, 0, 1, 1), (0, g, 1, 1), (0, -g, 1, 1)]
    f.append((0, 0, 0, 1))
    t = 2.0 ** -18
    f += [(sx * t, sy * t, 1, 2.0 ** -8) for sx in (1, -1, 0) for sy in (1, -1, 0) if sx or sy]
    return np.array(f, dtype=np.float64)


def tie_headings(consts, drads):
    """drads + s b + w stepped by -3..+3 ulps — its own, and pi's: delta passes through (x - pi) + pi and lives on the grid of pi's ulp, so
    around a small heading only steps of that size move it —, kept where they fall in (-pi, pi]; and -0.0."""
    bs = [0.0, consts.atol, consts.x_turn, consts.sense_rad, PI / 2, PI] + [k * consts.turn_rad for k in range(13)]
    out = {-0.0: None}
    for b in bs:
        for s in (1.0, -1.0):
            for w in (0.0, 2 * PI, -2 * PI):
                h0 = drads + s * b + w
                for h in ulps(h0) + [h0 + k * GRID for k in (-3, -2, -1, 1, 2, 3)]:
                    if -PI < h <= PI:
                        out[h] = None
    keys = list(out)
    return np.array(keys + ([0.0] if 0.0 not in keys else []))


@functools.lru_cache(maxsize=None)
def world_of(group, pset, dtype='f32', part=0, normalized=True, kind='physarum'):
    """The worlds by key (cached, never modified)."""
    return {1: _tie_worlds, 3: _generic_worlds, 4: _magnitude_worlds, 5: _outside_worlds}[group](pset, dtype, normalized, kind)[part]


def n_parts(group, pset, dtype='f32', normalized=True, kind='physarum'):
    return len({1: _tie_worlds, 3: _generic_worlds, 4: _magnitude_worlds, 5: _outside_worlds}[group](pset, dtype, normalized, kind))


def _split(fields, headings, **kw):
    """Worlds of at most 3072 blocks over the (field, heading) pairs."""
    cap = (SHAPES[-1][0] // B) * (SHAPES[-1][1] // B)
    worlds = []
    for at in range(0, len(fields), cap):
        w = World(fields[at:at + cap], **kw)
        w.headings[:w.n] = headings[at:at + cap]
        worlds.append(w)
    return worlds


def _probe_drads(fields, **kw):
    """drads of every field type as the oracle reads it from the stored ramp."""
    return World(fields, **kw).drads[:len(fields)]


@functools.lru_cache(maxsize=None)
def _tie_worlds(pset, dtype, normalized=True, kind='physarum'):
    consts = Consts(PARAM_SETS[pset])
    types = tie_fields(dtype)
    F, Hd = [], []
    for f, dr in zip(types, _probe_drads(types, dtype=dtype)):
        hs = tie_headings(consts, float(dr))
        F.append(np.tile(f, (len(hs), 1)))
        Hd.append(hs)
    return _split(np.concatenate(F), np.concatenate(Hd), dtype=dtype)


# ---------------------------------------------------------------- 3. generic directions
N_PHI = 64
MARGIN_FACTORS = (1.0, 1.5, 2.0, 4.0, 16.0, 0.5, 0.25, 0.125, 1 / 16, 1 / 64, 0.0)         # of M: the first five are asserted


def generic_fields(n=N_PHI, a=0.25, c0=1.0):
    """(gx, gy) = f32(cos phi, sin phi), phi = (k + 0.5) 2 pi / n: never on an axis or a diagonal."""
    phi = (np.arange(n) + 0.5) * 2 * PI / n
    return np.stack([f32(np.cos(phi)), f32(np.sin(phi)), np.full(n, a), np.full(n, c0)], axis=1)


def small_phi_fields(consts, a=0.25):
    """drads itself at the x_grad test: gx = 1, gy = tan(phi) for |phi| around x_grad = 1e-8 — with c0 = 0 the four taps are the fp32
    numbers -+a gx and -+a gy themselves."""
    M = consts.margins()['x_grad']
    f = []
    for s in (1.0, -1.0):
        for fac in MARGIN_FACTORS:
            for side in (1.0, -1.0):
                f.append((1.0, s * math.tan(consts.x_grad + side * fac * M), a, 0.0))
        for phi in (1e-12, 1e-9, 0.5e-8, 2e-8, 1e-7, 1e-6):
            f.append((1.0, s * math.tan(phi), a, 0.0))
    return np.array(f)


def margin_headings(consts, drads, thetas, factors, M, count=None):
    """For every field the headings drads + s (theta +- f M[theta]), renormalised into (-pi, pi] as real runs carry them."""
    F, Hd = [], []
    for k, dr in enumerate(drads):
        for name, theta in thetas:
            for s in (1.0, -1.0):
                for fac in factors:
                    for side in ((1.0, -1.0) if fac else (1.0,)):
                        F.append(k)
                        Hd.append(dr + s * (theta + side * fac * M[name]))
    return np.array(F), R.renormalize_radians(np.array(Hd))


def thresholds_of(consts):
    t = [('x_turn', consts.x_turn)]
    if consts.sense_rad < PI:
        t.append(('sense', consts.sense_rad))
    else:
        t.append(('pi', PI))
    return t


@functools.lru_cache(maxsize=None)
def _generic_worlds(pset, dtype='f32', normalized=True, kind='physarum'):
    consts = Consts(PARAM_SETS[pset])
    types = generic_fields()
    idx, hd = margin_headings(consts, _probe_drads(types, dtype=dtype), thresholds_of(consts), MARGIN_FACTORS, consts.margins())
    F, Hd = [types[idx]], [hd]
    if pset == 0:                                                      # the x_grad test: delta = 0.3, clear of the other thresholds
        sm = small_phi_fields(consts)
        F.append(sm)
        Hd.append(np.full(len(sm), 0.3))
    return _split(np.concatenate(F), np.concatenate(Hd), dtype=dtype)


# ---------------------------------------------------------------- 4. magnitudes
def magnitude_fields():
    """The group-3 ramps at every amplitude, c0 = 4 a (0 at 2^126: 4 a would overflow), and one flat block per amplitude."""
    base = generic_fields()
    F = []
    for a in AMPLITUDES:
        c0 = 0.0 if a > 2.0 ** 120 else 4 * a
        f = base.copy()
        f[:, 2], f[:, 3] = a, c0
        F.append(f)
        F.append(np.array([[0.0, 0.0, 0.0, c0 if c0 else a]]))
    return np.concatenate(F)


@functools.lru_cache(maxsize=None)
def _magnitude_worlds(pset, dtype='f32', normalized=True, kind='physarum'):
    consts = Consts(PARAM_SETS[pset])
    types = magnitude_fields()
    w = World(types, dtype='f32', normalized=normalized, grad_clip=0.0)
    if kind == 'physarum':                                             # one heading per block, cycling through thresholds, sides and margins >= M
        M, th = consts.margins(), thresholds_of(consts)
        k = np.arange(w.n)
        name = [th[i % len(th)] for i in k]
        s = np.where((k // 2) % 2 == 0, 1.0, -1.0)
        side = np.where((k // 4) % 2 == 0, 1.0, -1.0)
        fac = np.array([1.0, 4.0, 1e4])[(k // 8) % 3]
        off = np.array([t[1] for t in name]) + side * fac * np.array([M[t[0]] for t in name])
        w.headings[:w.n] = R.renormalize_radians(w.drads[:w.n] + s * off)
    else:
        w.headings[:w.n] = R.renormalize_radians(0.37 * np.arange(w.n))
    return [w]


def group4_drops(world, exp):
    """Slots whose expected action overflows fp32 (the reference's arithmetic cast to fp32): dropped from the asserts, counted."""
    with np.errstate(over='ignore'):
        return ~np.isfinite(exp['action'].astype(np.float32)).all(axis=0)


# ---------------------------------------------------------------- 5. headings outside (-pi, pi]
def outside_headings():
    special = [h for k in range(-16, 17) for h in ulps(k * PI / 2, -1, 1)]
    return np.array(special), np.random.RandomState(5).uniform(-8 * PI, 8 * PI, 2000)


@functools.lru_cache(maxsize=None)
def _outside_worlds(pset, dtype='f32', normalized=True, kind='physarum'):
    ties = tie_fields(dtype)
    axis = ties[[0, 1, 2, 3, 8, 13]]                                  # four axis ramps, the flat block, sub-clip (-, -) -> pi
    gen = generic_fields(8)
    types = np.concatenate([axis, gen])
    special, uniform = outside_headings()
    F = [np.repeat(types, len(special), axis=0)]
    Hd = [np.tile(special, len(types))]
    k = np.arange(len(uniform))
    F += [axis[k % len(axis)], gen[k % len(gen)]]
    Hd += [uniform, uniform]
    return _split(np.concatenate(F), np.concatenate(Hd), dtype=dtype)


HMAX_OUTSIDE = 8 * PI                   # the largest heading set_state hands in here


# ---------------------------------------------------------------- the design of the float64 branch, restated
PI_D, TWO_PI_D = 3.141592653589793, 6.283185307179586


def _fma(x, y, z):
    return float(Fraction(x) * Fraction(y) + Fraction(z))


def renorm_rad(r):
    """die_forward.h renorm_rad: numpy's (r - pi) % (-2 pi) + pi without fmod — a quotient estimate, one exact fma, a correction."""
    a, b = r - PI_D, -TWO_PI_D
    m = _fma(-float(np.trunc(a * (-1.0 / TWO_PI_D))), b, a)
    if m != 0.0 and (m < 0.0) != (a < 0.0):
        m += -TWO_PI_D if a < 0.0 else TWO_PI_D
    if abs(m) >= TWO_PI_D:
        m -= -TWO_PI_D if a < 0.0 else TWO_PI_D
    if m != 0.0:
        if not m < 0.0:
            m += b
    else:
        m = -0.0
    return m + PI_D


def renorm_rad_fast(r):
    """die_forward.h renorm_rad_fast: three additions where a = r - pi lies in (-3.5 pi, 2 pi), the general form elsewhere."""
    a = r - PI_D
    if not abs(a + 0.75 * PI_D) < 2.75 * PI_D:
        return renorm_rad(r)
    k = -TWO_PI_D if a > 0.0 else (TWO_PI_D if a <= -TWO_PI_D else 0.0)
    return (a + k) + PI_D


def axis_branch(consts, ux, uy, d64, sign):
    """The `im == 0 || re == 0` branch for one slot, float64 throughout: (und_grad, und_turn, unseen, heading')."""
    re = ux + (0.0 * uy - 0.0)
    im = 0.0 + (0.0 + uy)
    assert im == 0.0 or re == 0.0
    if im == 0.0:
        drads = PI_D if (re < 0.0 or (re == 0.0 and math.copysign(1.0, re) < 0)) else 0.0
    else:
        drads = math.copysign(0.5 * PI_D, im)
    delta = renorm_rad_fast(d64 - drads)
    und_grad, und_turn, unseen = abs(drads) <= consts.x_grad, abs(delta) <= consts.x_turn, abs(delta) > consts.sense_rad
    sgn = float(sign) if (und_grad or und_turn or unseen) else (-1.0 if delta > consts.atol else 1.0)
    return und_grad, und_turn, unseen, renorm_rad_fast(d64 + sgn * consts.turn_rad)


# ---------------------------------------------------------------- 2. the world's first and last coordinates
def edge_agents(world, sense_offset_cells=10.2):
    """A copy of the world's agents with the first slots moved to X, Y in {0, 1, 2^32 - 1} / 2^32 (and one axis mid-world), headings in
    the eight compass directions: probes sense_offset ahead leave the world on every side, so the carry / borrow clamp of
    die_cell_off has to agree with die_cell and the one-sided differences of the four edges and corners get read."""
    q = [0.0, 1.0 / 2 ** 32, (2.0 ** 32 - 1) / 2 ** 32]
    mid = 0.4375
    spots = [(x, y) for x in q for y in q] + [(x, mid) for x in q] + [(mid, y) for y in q]
    agents, headings = world.agents.copy(), world.headings.copy()
    k = 0
    for x, y in spots:
        for d in range(8):
            agents[0, k], agents[1, k] = x, y
            headings[k] = R.renormalize_radians(d * PI / 4)
            k += 1
    return agents, headings, k
