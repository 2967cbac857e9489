"""Case builders for the tile-binned step away from the benchmark's parameter point (tests/test_binned_lattice_cpu.py asserts
their witnesses without a GPU, tests/test_gpu_binned_lattice.py runs them against the oracle).  numpy and oracle.cpu_ref only.

The step's two kernels size their LDS windows and choose their launch form from host-derived numbers (die_pic_forward_env_step,
pic_two_launch_rule in die_amd/csrc/die_pic.hip), with lengths in cells of the world's LONGER axis, n = max(W, H):

    chem margin   P_raw = floor(|sense_offset|·(n − 1)) + 2, rounded up to whole 16-byte vectors (4 fp32 / 8 fp16 cells); > 24: unstaged
    food margin   fm_r  = floor(reach) + 2 rows, reach = |scale|·(n − 1)
    radius        R     = int(4σ + 0.5), 1..4: the rim width, the field kernel's instantiation
    two launches  floor(reach) + 2 + R <= min(TX, TY)

Every bound is attained only by the worst placement: an agent on its tile's outermost cell, at the cell's outer edge, heading
straight out.  The builders put groups of agents exactly there (on top of random_state's world: 15 % density, 0.3 forced
collisions — the random chem and food planes are what make a wrong cell visible) and compute, FROM THE ORACLE ALONE, how far the
step-0 probe taps / landing cells of the whole population lie beyond the agents' tiles: the witnesses.  A case whose witness falls
short of the bound proves nothing; the CPU test asserts each.

Geometry (labels linspace(0, 1, n): cell c covers [c − ½, c + ½) cells of the coordinate, the coordinate circle closes at cell
n − 1 ≡ cell 0, so the two seam cells are half cells):
  * a placed agent sits 0.43–0.45 cell from its cell's centre towards the outside (seam cells: 0.012–0.015 inside the world's end; no
    two agents of a group share a coordinate); offsets
    are chosen so that every probe / landing coordinate that matters stays ≥ 0.012 cell away from a cell-rounding boundary — the
    device's fp32 trigonometry (1e-7 cell) cannot move a probe cell or a landing cell;
  * a probe of length L (cells of the longer axis) from offset 0.45 reaches cell floor(L + 0.95), the gradient taps one further:
    floor(L) + 2 = P_raw beyond the tile's border whenever frac(L) >= 0.05 ("tight": L = k − 0.001); for an integer L the bound
    is a supremum (it needs an offset of 0.5) and the attained maximum is P_raw − 1;
  * along the SHORTER axis of a world a length spans (n_axis − 1) / (n − 1) as many cells, so there the bounds are not attainable:
    on the 3×3-tile worlds 48×96, 96×192, 96×384 the margin family attains P_raw on the y sides only, so every tile shape also runs the
    margin family on a SQUARE world (96×96, 192×192, 384×384), where all four sides of a tile are asserted — a tap on the last staged
    ROW as well as on the last staged column, for both dtypes; the reach and rule families, whose bounds are about rows (food margin
    rows; min(TX, TY) = TX for the tile shapes under test), use the square worlds throughout;
  * a PhysarumAgent always turns by ±turn_angle before it moves (core/agent/gradient.py:168-208), so movers are placed with headings
    axis ± 30°: about half of them end up heading exactly along the axis (the witnesses count those from the oracle's own action).
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import cpu_ref as R

WORLDS = {(4, 5): (48, 96), (5, 6): (96, 192), (6, 6): (192, 192), (5, 7): (96, 384)}       # 3×3 tiles
SQUARE = {(6, 6): (192, 192), (4, 5): (96, 96), (5, 6): (192, 192), (5, 7): (384, 384)}                          # W == H: lengths span their cells along x too
PIC_MAX_MARGIN = 24
SIGMA_OF_R = {1: 0.25, 2: 0.5, 3: 0.75, 4: 1.0}
TURN = np.radians(30)
EDGE, SEAM, SAFE = 0.45, 0.015, 0.012

Case = namedtuple('Case', 'medium agents dir0 dyn kw tile f16 form witnesses agent threads')


def q32(v):
    """Coordinates as the device holds them (die_amd/device_array.py to_q32 / from_q32)."""
    return np.clip(np.rint(np.asarray(v, dtype=np.float64) * 2.0 ** 32), 0, 2.0 ** 32 - 1) / 2.0 ** 32


def f32(v):
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def radius(sigma):
    return int(4.0 * float(np.float32(sigma)) + 0.5)


def reach_f32(scale, n):
    """|scale|·(n − 1) as the library computes it (float32)."""
    return float(np.float32(abs(np.float32(scale))) * np.float32(n - 1))


def margin_raw(sense_offset, n):
    return int(np.floor(np.float32(abs(np.float32(sense_offset))) * np.float32(n - 1))) + 2


def two_launch_rule(n, tile, scale, sigma):
    """pic_two_launch_rule, restated from its comment (the CPU test compares it with the library's die_pic_two_launch)."""
    Rr = radius(sigma)
    return 1 <= Rr <= 4 and int(np.floor(np.float32(reach_f32(scale, n)))) + 2 + Rr <= min(1 << tile[0], 1 << tile[1])


# ------------------------------------------------------------------------------------------------ worlds
@functools.lru_cache(maxsize=None)
def _background(W, H, density=0.15):
    """tests/test_gpu_parity.py random_state(W, H, N, N, rs, collide=0.3) with N = 15 % of the cells (`density`: see radius_case): built
    once per world shape, copied by every case."""
    rs = np.random.RandomState(7 * W + H)
    N = int(density * W * H)
    chem = R.diffuse_decay(rs.rand(W, H), 1.0, 0.0)
    chem[: W // 4, : H // 4] = 0.
    food = np.round(rs.rand(W, H) * 0.5 * (rs.rand(W, H) < 0.6), 3)
    x, y = q32(rs.rand(N) * 0.999999), q32(rs.rand(N) * 0.999999)
    nc = int(0.3 * N)
    src, dst = rs.randint(0, N, nc), rs.randint(0, N, nc)
    x[dst], y[dst] = x[src], y[src]
    head = f32(rs.uniform(-np.pi, np.pi, N))
    for a in (chem, food, x, y, head):
        a.setflags(write=False)
    return f32(food), f32(chem), x, y, head


def world(W, H, groups, f16, seed, density=0.15):
    """The background with the placed groups appended, as tests/test_gpu_crowds.py crowd_world builds its worlds: `groups` = list of
    (ux, uy, heading) in CELL units.  Returns medium, agents, dir0 and each group's slots."""
    food, chem, x, y, head = _background(W, H, density)
    rs = np.random.RandomState(seed)
    xs, ys, hs, slots, at = [x], [y], [head], [], len(x)
    for ux, uy, h in groups:
        assert ux.min() >= 0 and ux.max() <= W - 1 and uy.min() >= 0 and uy.max() <= H - 1
        xs.append(q32(ux / (W - 1))); ys.append(q32(uy / (H - 1))); hs.append(f32(h))
        slots.append(np.arange(at, at + len(ux)))
        at += len(ux)
    agents = np.zeros((4, at))
    agents[0], agents[1], agents[2] = np.concatenate(xs), np.concatenate(ys), 1.
    agents[3] = f32(0.1 + 0.9 * rs.rand(at))
    medium = np.stack([np.zeros((W, H)), food, chem])
    medium[0][R.cell(agents[0], W), R.cell(agents[1], H)] = 1.
    if f16:                                                   # fields the device holds exactly
        medium[1:] = medium[1:].astype(np.float16).astype(np.float64)
    return medium, agents, np.concatenate(hs), slots


JITTER = {False: 0.02, True: 0.003}                        # by which a placed agent's offset may fall short of 0.45 / 0.015 (seam cells)


def _offset(c, n, out, travel, rs=None, count=None):
    """Signed sub-cell offset of an agent placed on cell c of an axis of n cells, towards `out` (±1): 0.45 (a seam cell that looks out
    of the world: 0.015 inside its end), stepped back until c + offset + out·travel lies >= SAFE from a cell-rounding boundary.  With
    `rs`: `count` offsets, each up to JITTER short of that one, all reaching the same cell — agents of one group must not share a
    coordinate: they would share every later probe coordinate too, and ONE chance approach to a rounding boundary would count as many
    forward mismatches as the group has agents."""
    seam = (c == n - 1 and out > 0) or (c == 0 and out < 0)
    sign = -out if seam else out
    for o in ((SEAM, 0.03, 0.05, 0.08) if seam else (EDGE, 0.42, 0.38, 0.34)):
        ends = [sign * o + out * travel + 0.5, sign * (o - JITTER[seam]) + out * travel + 0.5]
        if np.floor(ends[0]) == np.floor(ends[1]) and all(SAFE <= e % 1.0 <= 1.0 - SAFE for e in ends):
            return sign * o if rs is None else sign * (o - rs.uniform(0, JITTER[seam], count))
    raise AssertionError((c, n, out, travel))


def _within(rs, c, n_axis):
    """Positions (cell units) on the cells `c`, at most 0.4 cell from their centres and inside the world: on the two seam cells (half
    cells) 0.02–0.4 cell inside the world's end — never ON it: a coordinate of exactly 0 is a cell centre, and from a cell centre a
    probe of k + 0.5 cells along an axis ends exactly on a rounding boundary."""
    c = np.asarray(c, dtype=np.float64)
    o = rs.uniform(-0.4, 0.4, c.shape)
    o = np.where(c <= 0, 0.02 + 0.38 * np.abs(o) / 0.4, np.where(c >= n_axis - 1, -0.02 - 0.38 * np.abs(o) / 0.4, o))
    return c + o


def _along(rs, lo, hi, n_axis, n):
    """n positions (cell units) on the cells lo..hi − 1 of the other axis (_within)."""
    return _within(rs, rs.randint(lo, hi, n), n_axis)


def border_lines(rs, W, H, tile, n, travel, spread, which=None, cells=None):
    """Groups on the tiles' outermost cells, heading out: for every tile border line of both axes (the world's seam included) and
    both directions, `n` agents per tile along the line.  `travel`: the length (cells of the longer axis) whose end point must
    stay clear of the rounding boundaries; `spread(rs, n)`: what is added to the outward heading; `which`: the axes to place on."""
    TX, TY = 1 << tile[0], 1 << tile[1]
    nmax = max(W, H)
    groups = []
    for axis, (na, nb, T, Tb) in enumerate(((W, H, TX, TY), (H, W, TY, TX))):
        if which is not None and axis not in which:
            continue
        tr = travel * (na - 1) / (nmax - 1)
        for t in range(na // T):
            for c, out in (((t + 1) * T - 1, 1), (t * T, -1)):
                if cells is not None and c not in cells[axis]:
                    continue
                main_of = lambda: c + _offset(c, na, out, tr, rs, n)
                for tb in range(nb // Tb):
                    other = _along(rs, tb * Tb, (tb + 1) * Tb, nb, n)
                    base = (0.0 if out > 0 else np.pi) if axis == 0 else out * np.pi / 2
                    h = base + spread(rs, n)
                    u = main_of()
                    groups.append((u, other, h) if axis == 0 else (other, u, h))
    return groups


def corner_groups(rs, W, H, tile, n, travel):
    """`n` agents on each corner cell of every tile, at the outer corner of the cell, heading diagonally out."""
    TX, TY = 1 << tile[0], 1 << tile[1]
    nmax = max(W, H)
    groups = []
    for tx in range(W // TX):
        for ty in range(H // TY):
            for ox in (-1, 1):
                for oy in (-1, 1):
                    cx = (tx + 1) * TX - 1 if ox > 0 else tx * TX
                    cy = (ty + 1) * TY - 1 if oy > 0 else ty * TY
                    ux = cx + _offset(cx, W, ox, travel * (W - 1) / (nmax - 1) / np.sqrt(2), rs, n)
                    uy = cy + _offset(cy, H, oy, travel * (H - 1) / (nmax - 1) / np.sqrt(2), rs, n)
                    groups.append((ux, uy, np.full(n, np.arctan2(oy, ox))))
    return groups


def _straight(rs, n):
    return np.zeros(n)


def _turned(rs, n):
    """± turn_angle: the PhysarumAgent's turn puts about half of these on the axis."""
    return np.where(np.arange(n) % 2 == 0, TURN, -TURN)


def physarum_kw(n, reach, probe):
    return dict(scale=reach / (n - 1), sense_offset=probe / (n - 1))


def gradient_kw(n, reach, probe):
    return dict(scale=reach / (n - 1), sense_offset=probe / (n - 1), inertia=0.0, noise_scale=0.0, normalized_grad=True)


def expected_form(W, H, tile, kw, dyn):
    return 'two launches' if two_launch_rule(max(W, H), tile, kw['scale'], dyn.get('diffuse_sigma', 0.5)) else 'three launches'


# ------------------------------------------------------------------------------------------------ witnesses (oracle only)
def oracle_agent(case):
    N = case.agents.shape[1]
    ref = (R.RefPhysarumAgent if case.agent == 'physarum' else R.RefGradientAgent)(N, seed=3, **case.kw)
    ref._direction_rads = case.dir0.copy()
    return ref


def tap_excess(case):
    """Step 0, every agent: how far its probe's gradient taps (np.gradient: the probe cell's two neighbours per axis, one-sided at the
    world's edge; probes clamp there — core/agent/gradient.py:55-76) lie beyond its own tile, per side (x low, x high, y low, y high),
    and the tile it stands on."""
    W, H = case.medium.shape[1:]
    xs, ys = case.tile
    off = np.stack(R.polar2xy(case.kw['sense_offset'], case.dir0))
    px, py = R.cell(case.agents[0] + off[0], W), R.cell(case.agents[1] + off[1], H)
    cx, cy = R.cell(case.agents[0], W), R.cell(case.agents[1], H)
    x0, y0 = (cx >> xs) << xs, (cy >> ys) << ys
    ex = np.stack([x0 - np.maximum(px - 1, 0), np.minimum(px + 1, W - 1) - (x0 + (1 << xs) - 1),
                   y0 - np.maximum(py - 1, 0), np.minimum(py + 1, H - 1) - (y0 + (1 << ys) - 1)])
    return np.maximum(ex, 0), (cx >> xs) * (H >> ys) + (cy >> ys)


def oracle_landing(case):
    """Step 0: the oracle's forward, then the oracle's move with its own action (core/env.py:163-172).  Returns the old and the new
    cells."""
    W, H = case.medium.shape[1:]
    action = oracle_agent(case).forward((case.agents, case.medium))
    new = R.move_handle_boundary(case.agents[:2] + action[:2], case.dyn.get('boundary', 'wrap'))
    return (R.cell(case.agents[0], W), R.cell(case.agents[1], H)), (R.cell(new[0], W), R.cell(new[1], H))


def beyond_tile(c_old, c_new, shift, n):
    """Cells from the agent's old tile to its landing cell along one axis (0: still on the tile's rows), on the coordinate circle, and
    whether the way led across the world's seam."""
    T = 1 << shift
    x0 = (c_old >> shift) << shift
    rel = (c_new - x0) % n
    rel = np.where(rel >= n // 2 + T // 2, rel - n, rel)
    far = np.where(rel > T - 1, rel - (T - 1), np.where(rel < 0, -rel, 0))
    seam = np.where(rel > T - 1, c_new < c_old, np.where(rel < 0, c_new > c_old, False))
    return far, seam


def margin_witnesses(case):
    W, H = case.medium.shape[1:]
    ex, t = tap_excess(case)
    NT = (W >> case.tile[0]) * (H >> case.tile[1])
    p_raw = margin_raw(case.kw['sense_offset'], max(W, H))
    at_bound = [int(np.bincount(t[ex[s] == p_raw], minlength=NT).max()) for s in range(4)]
    at_max = [int(np.bincount(t[ex[s] == ex[s].max()], minlength=NT).max()) for s in range(4)]
    return dict(p_raw=p_raw, max_excess=ex.max(axis=1).tolist(), at_bound=at_bound, at_max=at_max)


def reach_witnesses(case):
    W, H = case.medium.shape[1:]
    old, new = oracle_landing(case)
    fl = int(np.floor(np.float32(reach_f32(case.kw['scale'], max(W, H)))))
    out = dict(floor_reach=fl)
    for name, axis, shift, n in (('rows', 0, case.tile[0], W), ('cols', 1, case.tile[1], H)):
        far, seam = beyond_tile(old[axis], new[axis], shift, n)
        out[name] = dict(max_seam=int(far[seam].max(initial=0)), max_interior=int(far[~seam].max(initial=0)),
                         seam_at_bound=int((far[seam] == fl + 2).sum()), interior_at_bound=int((far[~seam] == fl + 1).sum()))
        # where the agents come to stand in the tile they walk onto, counted from its FAR border (the rule family)
        T = 1 << shift
        l_new = new[axis] & (T - 1)
        up = ((new[axis] - old[axis]) % n) < n // 2
        far_side = np.where(up, T - 1 - l_new, l_new)
        out[name]['nearest_far_border'] = int(far_side[far > 0].min(initial=T))
    return out


def rim_codes(case, new):
    """The agent kernel's rim test on the landing cells: per axis 0 within R of the tile's low border, 2 of its high border, else 1."""
    Rr = radius(case.dyn['diffuse_sigma'])
    TX, TY = 1 << case.tile[0], 1 << case.tile[1]
    lx, ly = new[0] & (TX - 1), new[1] & (TY - 1)
    ex = np.where(lx < Rr, 0, np.where(lx >= TX - Rr, 2, 1))
    ey = np.where(ly < Rr, 0, np.where(ly >= TY - Rr, 2, 1))
    return lx, ly, ex, ey


def radius_witnesses(case):
    W, H = case.medium.shape[1:]
    xs, ys = case.tile
    TX, TY = 1 << xs, 1 << ys
    Rr = radius(case.dyn['diffuse_sigma'])
    old, new = oracle_landing(case)
    lx, ly, ex, ey = rim_codes(case, new)
    t_old = (old[0] >> xs) * (H >> ys) + (old[1] >> ys)
    t_new = (new[0] >> xs) * (H >> ys) + (new[1] >> ys)
    stay = t_old == t_new
    listed = ~stay | (ex != 1) | (ey != 1)
    near = {f'{a - 1:+d}{b - 1:+d}': int(((ex == a) & (ey == b)).sum()) for a in range(3) for b in range(3) if (a, b) != (1, 1)}
    inside = dict(x_low=int((stay & (lx == Rr) & (ey == 1)).sum()), x_high=int((stay & (lx == TX - 1 - Rr) & (ey == 1)).sum()),
                  y_low=int((stay & (ly == Rr) & (ex == 1)).sum()), y_high=int((stay & (ly == TY - 1 - Rr) & (ex == 1)).sum()))
    last = dict(x_low=int((lx == Rr - 1).sum()), x_high=int((lx == TX - Rr).sum()), y_low=int((ly == Rr - 1).sum()), y_high=int((ly == TY - Rr).sum()))
    per_tile = np.bincount(t_old[listed], minlength=(W >> xs) * (H >> ys))
    return dict(R=Rr, near=near, just_inside_unlisted=inside, last_listed=last, min_listed=int(per_tile.min()), max_listed=int(per_tile.max()))


# ------------------------------------------------------------------------------------------------ the families
def _case(W, H, groups, f16, seed, dyn, kw, tile, agent, witness, threads=0, density=0.15):
    medium, agents, dir0, _ = world(W, H, groups, f16, seed, density)
    dyn = dict(dyn)
    c = Case(medium, agents, dir0, dyn, kw, tile, f16, expected_form(W, H, tile, kw, dyn), None, agent, threads)
    return c._replace(witnesses=witness(c))


def margin_case(tile, f16, boundary, agent, probe, threads=0, reach=1.53, square=False):
    """(a) probes of `probe` cells from the tiles' outermost cells, straight out and diagonally out of the corners.  `square`: on the
    tile shape's square world, where the probe spans its full length along both axes."""
    W, H = (SQUARE if square else WORLDS)[tile]
    rs = np.random.RandomState(int(probe * 1000) + W)
    groups = border_lines(rs, W, H, tile, 30, probe, _straight) + corner_groups(rs, W, H, tile, 3, probe)
    kw = (physarum_kw if agent == 'physarum' else gradient_kw)(max(W, H), reach, probe)
    return _case(W, H, groups, f16, 11, dict(boundary=boundary, diffuse_sigma=0.5), kw, tile, agent, margin_witnesses, threads)


def reach_case(tile, f16, reach, sigma=0.5, threads=0, which=(0, 1), probe=10.2):
    """(b), (d) steps of `reach` cells from the rows and columns next to the world's seam and next to interior tile borders, across
    them in both directions (headings axis ± 30°: see the module's text)."""
    W, H = SQUARE[tile]
    TX, TY = 1 << tile[0], 1 << tile[1]
    rs = np.random.RandomState(int(reach * 1000) + W)
    cells = [{0, T - 1, T, 2 * T - 1, 2 * T, n - 1} for T, n in ((TX, W), (TY, H))]      # the seam and the first two interior borders
    groups = []
    per_tile = {0: max(1, 270 // (H // TY)), 1: max(1, 270 // (W // TX))}                # ≈ 270 agents per line and direction
    for axis in which:
        groups += border_lines(rs, W, H, tile, per_tile[axis], reach, _turned, which=(axis,), cells=cells)
    groups += corner_groups(rs, W, H, tile, 1, reach)
    kw = physarum_kw(max(W, H), reach, probe)
    return _case(W, H, groups, f16, 13, dict(boundary='wrap', diffuse_sigma=sigma), kw, tile, 'physarum', reach_witnesses, threads)


def radius_case(tile, f16, sigma, overflow=False, world_shape=None, density=0.15):
    """(c) agents 0 .. R + 2 cells inside every border and corner of every tile, headings uniform: after the step's move (1.53 cells)
    they straddle the rim test on both sides.  `overflow`: 4·rim_cap more inside the centre tile's rim, so that its list
    overflows and the field kernels around it take the segment-scan fallback.  `density`: of the background (32×64 tiles with R = 4:
    their rim is 1 344 of 2 048 cells and at 15 % the world's own agents overflow every 112-entry list, so those cases run at 6 % and
    every list holds its tile's agents; the overflow cases keep 15 %)."""
    W, H = world_shape or WORLDS[tile]
    TX, TY = 1 << tile[0], 1 << tile[1]
    Rr = max(radius(sigma), 1)
    # (fewer placed agents where the rims are wide or the lists short — 112 entries on the small tiles —, so that not every list overflows)
    big = TX * TY >= 4096 and Rr <= 2
    rs = np.random.RandomState(int(sigma * 1000) + W + H)
    groups = []
    for tx in range(W // TX):
        for ty in range(H // TY):
            x0, y0 = tx * TX, ty * TY
            for d in range(min(Rr + 3, TX // 2)):
                n = 3 if big else 1
                for lx in (d, TX - 1 - d):
                    groups.append((_within(rs, np.full(n, x0 + lx), W), _along(rs, y0, y0 + TY, H, n), rs.uniform(-np.pi, np.pi, n)))
                for ly in (d, TY - 1 - d):
                    groups.append((_along(rs, x0, x0 + TX, W, n), _within(rs, np.full(n, y0 + ly), H), rs.uniform(-np.pi, np.pi, n)))
            for cx in (x0, x0 + TX - Rr - 2):                  # the corners: squares of (R + 2)² cells
                for cy in (y0, y0 + TY - Rr - 2):
                    n = max((Rr + 2) ** 2 // (2 if big else 6), 8)
                    groups.append((_along(rs, cx, cx + Rr + 2, W, n), _along(rs, cy, cy + Rr + 2, H, n), rs.uniform(-np.pi, np.pi, n)))
    if overflow:
        cap = 224 if TX * TY >= 4096 else 112                 # die_pic_rim_cap (the CPU test compares)
        n = 4 * cap
        x0, y0 = TX, TY
        side = rs.randint(0, 4, n)
        depth = rs.randint(0, Rr, n) + rs.uniform(-0.4, 0.4, n)
        ax, ay = _along(rs, x0, x0 + TX, W, n), _along(rs, y0, y0 + TY, H, n)
        ux = np.where(side == 0, x0 + depth, np.where(side == 1, x0 + TX - 1 - depth, ax))
        uy = np.where(side == 2, y0 + depth, np.where(side == 3, y0 + TY - 1 - depth, ay))
        groups.append((np.clip(ux, 0, W - 1), np.clip(uy, 0, H - 1), rs.uniform(-np.pi, np.pi, n)))
    kw = physarum_kw(max(W, H), 1.53, 10.2)
    return _case(W, H, groups, f16, 17, dict(boundary='wrap', diffuse_sigma=sigma), kw, tile, 'physarum', radius_witnesses, density=density)


# ------------------------------------------------------------------------------------------------ the lattice
def _spec(family, build, **args):
    ident = family + '-' + '-'.join(f'{k}{v}' for k, v in args.items())
    return dict(id=ident, family=family, build=build, args=args)


def margin_specs():
    """Per tile shape, boundary and agent kind: the tight probes k − 0.001 (P_raw = k + 1 a whole number of vectors: no slack from the
    round-up) and the integer probes k; the probes k + 0.5 with k + 1 a whole number of vectors (P_raw = k + 2 and the tap at k + 2: one
    cell fewer in the host's bound leaves P at k + 1, inside a STAGED window); 23.2 (P_raw 25: unstaged).  On the 3×3-tile worlds, and —
    the shapes whose 3×3-tile world is not square — the tight, half and unstaged probes again on the square worlds."""
    out = []
    for f16, tiles, ends in ((False, ((6, 6), (4, 5)), (4, 8, 12, 16, 20, 24)), (True, ((5, 7), (5, 6)), (8, 16, 24))):
        for tile in tiles:
            for boundary in ('wrap', 'limit'):
                for agent in ('physarum', 'gradient'):
                    common = dict(tile=tile, f16=f16, boundary=boundary, agent=agent)
                    tight = [e - 1 - 0.001 for e in ends]
                    half = [e - 1 + 0.5 for e in ends[:-1]]
                    for probe in sorted(tight + [float(e - 1) for e in ends] + half) + [23.2]:
                        out.append(_spec('margin', margin_case, **common, probe=probe))
                    if WORLDS[tile] != SQUARE[tile]:
                        for probe in sorted(tight + half) + [23.2]:
                            out.append(_spec('margin', margin_case, **common, probe=probe, square=True))
    return out


REACHES = (0.999, 1.53, 2.999, 4.5, 7.999, 13.5)


def reach_specs():
    return [_spec('reach', reach_case, tile=tile, f16=f16, reach=r) for tile, f16 in (((6, 6), False), ((5, 7), True)) for r in REACHES]


SIGMAS = (0.25, 0.375, 0.5, 0.625, 0.8, 0.875, 1.0)              # R = 1, 2, 2, 3, 3, 4, 4


def radius_specs():
    out = [_spec('radius', radius_case, tile=tile, f16=f16, sigma=s, **(dict(density=0.06) if tile == (5, 6) and radius(s) == 4 else {}))
           for tile in WORLDS for f16 in (False, True) for s in SIGMAS]
    out.append(_spec('radius', radius_case, tile=(4, 5), f16=False, sigma=0.25, overflow=True))
    out.append(_spec('radius', radius_case, tile=(6, 6), f16=False, sigma=1.0, overflow=True))
    out.append(_spec('radius', radius_case, tile=(5, 6), f16=True, sigma=0.25, overflow=True))
    out.append(_spec('radius', radius_case, tile=(5, 7), f16=True, sigma=1.0, overflow=True))
    return out


def rule_specs():
    """(d) the two-launch rule at equality, on the tile shapes' shorter side (rows): `side` two — reach (TX − 2 − R) + 0.999, the last
    reach of the two-launch form; three — (TX − 1 − R) + 0.001, the first of the three-launch form; three_far — (TX − 1 − R) + 0.999,
    where an agent across the seam lands INSIDE the far rim of the tile it walks onto (what the rule exists to keep out of the
    two-launch form); limit — TX − 1, the longest step the tiles take at all."""
    out = []
    for tile, f16 in (((4, 5), False), ((5, 7), True)):
        T = min(1 << tile[0], 1 << tile[1])
        for Rr in (1, 2, 3, 4):
            for side, reach in (('two', T - 2 - Rr + 0.999), ('three', T - 1 - Rr + 0.001), ('three_far', T - 1 - Rr + 0.999)):
                out.append(_spec('rule', reach_case, tile=tile, f16=f16, reach=reach, sigma=SIGMA_OF_R[Rr], which=(0,)) | dict(side=side))
        out.append(_spec('rule', reach_case, tile=tile, f16=f16, reach=float(T - 1), which=(0,)) | dict(side='limit'))
    return out


def special_specs():
    """The two parameter points of the agent kernel's specialised instantiations (fp32 64×64 tiles with chem margin 12, fp16 32×128
    tiles with chem margin 16; food margin 3, R = 2, wrap, 512 threads) at the tightest placement of the margin and reach families."""
    return [_spec('special', margin_case, tile=(6, 6), f16=False, boundary='wrap', agent='physarum', probe=10.999),
            _spec('special', margin_case, tile=(5, 7), f16=True, boundary='wrap', agent='physarum', probe=14.999, square=True),
            _spec('special', reach_case, tile=(6, 6), f16=False, reach=1.999),
            _spec('special', reach_case, tile=(5, 7), f16=True, reach=1.999)]


def thread_specs():
    """Other workgroup sizes of the agent kernel: the widest staged chem window (P = 24) and the tallest food block (the longest step)."""
    out = []
    for threads in (64, 320):
        for tile, f16 in (((6, 6), False), ((4, 5), False), ((5, 7), True), ((5, 6), True)):
            out.append(_spec('threads', margin_case, tile=tile, f16=f16, boundary='wrap', agent='physarum', probe=22.999, threads=threads, square=True))
        out.append(_spec('threads', reach_case, tile=(5, 7), f16=True, reach=31.0, which=(0,), threads=threads))
    return out


def outside_specs():
    """Gaussian radii the tile-binned step does not have (R = 0 and R = 5: the library's field kernels are compiled for 1..4 and Env.step
    takes the classic step there): the rule must say "not two launches", Env must not bin, and the step still agrees with the oracle."""
    return [_spec('outside', radius_case, tile=(6, 6), f16=False, sigma=0.12), _spec('outside', radius_case, tile=(4, 5), f16=False, sigma=1.125)]


def special_point(case):
    """Does the case sit on one of the agent kernel's two specialised parameter points (die_pic.hip PicK1Special, pic_k1_matches)?"""
    W, H = case.medium.shape[1:]
    P = {((6, 6), False): 12, ((5, 7), True): 16}.get((case.tile, case.f16))
    V = 8 if case.f16 else 4
    return (P is not None and case.agent == 'physarum' and case.form == 'two launches' and case.dyn.get('boundary', 'wrap') == 'wrap'
            and radius(case.dyn['diffuse_sigma']) == 2 and case.threads in (0, 512)
            and -(-margin_raw(case.kw['sense_offset'], max(W, H)) // V) * V == P
            and int(np.floor(np.float32(reach_f32(case.kw['scale'], max(W, H))))) + 2 == 3)


def lattice_specs():
    return margin_specs() + reach_specs() + radius_specs() + rule_specs() + thread_specs()


def build(spec):
    return spec['build'](**spec['args'])
