"""Crowded tiles on the benchmarked tile-binned step (die_amd/csrc/die_pic.hip: agent kernel k_pic_forward_move, field kernel
k_pic_resolve_diffuse, order table k_pic_order) — the paths that run on every step once the agents have aggregated (the README's
world steps 1 000–8 000) and that a uniform random world never reaches:

- crowd states teacher-forced against the float64 oracle, each test asserting from the device's own bookkeeping (the layouts'
  per-tile words, the rim counts, the order table) that the paths it is named for were taken;
- the order table compared EXACTLY with its host model (tests/order_model.py), at the first step, after the rebuild of step 32 and
  in between;
- the split-launch step (die_pic.stages, what bench.py times kernel by kernel) against the one-call step;
- the benchmark's own world after 1 024 free steps, one teacher-forced step (the table's rebuild) against the oracle.

Bookkeeping read here (die_amd/pic.py, die_pic.hip): meta[L] = (off, n, s, inc) per tile of layout L.  The step reading layout `in`
writes layout `out`: n_out[t] = the agents that stood on t when the step began (what the agent kernel's workgroup of t processed), s_out[t]
= those of them still on t (the field kernel's "stayers" of t).  The agent kernel's arrival candidates of t are the leavers of its 8
neighbours in `in`, n_in − s_in; it compacts PIC_LIST_CAP = 512 of them per round.  rim_cnt[t]: entries of t's rim list this step
(> die_pic_rim_cap: overflowed, the field kernels around t scan t's segment instead).  The field kernel rewrites `in`'s n / off for
the next step, so `in`'s words are read before the step."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import cpu_ref as R                                              # noqa: E402
from tests import order_model as OM                                          # noqa: E402
from tests.test_gpu_parity import (_binned_steps_against_the_oracle, applied, assert_forward_mismatches_explained,  # noqa: E402,F401
                                   f32, physarum_margins, q32, random_state, RTOL)

LIST_CAP = 512           # PIC_LIST_CAP: arrival candidates per round of the agent kernel


@pytest.fixture(scope='module')
def die():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import die_amd
    return die_amd


def _ceil(a, b):
    return -(-np.asarray(a, dtype=np.int64) // b)


def tile_populations(agents, W, H, tile):
    """Alive agents per tile (index tx·nty + ty) of an agent array: what a freshly binned layout holds."""
    xs, ys = tile
    live = agents[2] > 0
    t = (R.cell(agents[0, live], W) >> xs) * (H >> ys) + (R.cell(agents[1, live], H) >> ys)
    return np.bincount(t, minlength=(W >> xs) * (H >> ys))


def ring(t, ntx, nty):
    """The 9 tiles around t: (dx, dy) → tile, periodic."""
    tx, ty = divmod(int(t), nty)
    return {(dx, dy): ((tx + dx) % ntx) * nty + (ty + dy) % nty for dx in (-1, 0, 1) for dy in (-1, 0, 1)}


class Bookkeeping:
    """The callback of _binned_steps_against_the_oracle: per step, the device's per-tile words of the layout the step read (taken
    before it) and wrote, the rim counts and the order table (taken after)."""

    def __init__(self, agents, W, H, tile):
        self.W, self.H, self.tile = W, H, tile
        self.ntx, self.nty = W >> tile[0], H >> tile[1]
        self.first = tile_populations(agents, W, H, tile)
        self.steps = []

    def __call__(self, step, env, agent, when):
        pic = env._pic
        if when == 'before':
            if pic is None or not pic.is_current(env, agent):             # the step bins first: every agent a stayer
                n_in = s_in = self.first if pic is None else None
                assert n_in is not None, 'a re-bin in the middle of a teacher-forced run'
            else:
                n_in, s_in = (pic.meta[pic.cur][k].cpu().numpy().astype(np.int64) for k in (1, 2))
            self.steps.append(dict(calls=agent._calls, n_in=n_in, s_in=s_in))
            return
        d = self.steps[-1]
        d['n_out'], d['s_out'] = (pic.meta[pic.cur][k].cpu().numpy().astype(np.int64) for k in (1, 2))
        d['cap'] = pic.rim_cnt is not None and int(_lib().lib.die_pic_rim_cap(pic.xs, pic.ys))
        d['rim'] = pic.rim_cnt.cpu().numpy().astype(np.int64) if pic.rim_cnt is not None else None
        d['order'] = pic.order.cpu().numpy().astype(np.int64) & 0xFFFF if pic.order is not None else None
        d['k1_block'] = pic.k1_threads or (512 if (1 << (pic.xs + pic.ys)) >= 4096 else 256)
        d['kb_block'] = 512 if (1 << (pic.xs + pic.ys)) >= 4096 else 256
        d['x'] = env.agents.x.cpu().numpy().view(np.uint32).copy()

    # --- the paths, from the device's words
    def candidates(self, d, t):
        """Arrival candidates of tile t's agent-kernel workgroup: its 8 neighbours' leavers in the layout read."""
        leave = d['n_in'] - d['s_in']
        return sum(int(leave[u]) for k, u in ring(t, self.ntx, self.nty).items() if k != (0, 0))

    def report(self):
        out = []
        for d in self.steps:
            t = int(np.argmax(d['n_out']))
            ncand = max(self.candidates(d, u) for u in range(self.ntx * self.nty))
            over = np.nonzero(d['rim'] > d['cap'])[0].tolist() if d['rim'] is not None else []
            out.append(f"calls {d['calls']}: max population {d['n_out'][t]} (tile {t}, stayers {d['s_out'][t]}, "
                       f"{int(_ceil(d['n_out'][t], 512))} 8-wave rounds), max arrival candidates {ncand} ({max(1, int(_ceil(ncand, LIST_CAP)))} "
                       f"rounds), rim lists over cap {len(over)}")
        return '\n'.join(out)


def _lib():
    from die_amd import _lib as L
    return L


def crowd_agents(rs, n, rows, cols, W, H, heading, collide=0.01):
    """`n` agents at distinct continuous positions in the cell rectangle rows × cols (cell units, half-open), headings uniform in
    `heading` (radians) — away from the forward's float thresholds —, and a small deliberate subset of exact collisions."""
    x = q32((rows[0] + (rows[1] - rows[0]) * rs.rand(n)) / (W - 1))
    y = q32((cols[0] + (cols[1] - cols[0]) * rs.rand(n)) / (H - 1))
    nc = int(collide * n)
    src, dst = rs.choice(n, nc, replace=False), rs.choice(n, nc, replace=False)
    x[dst], y[dst] = x[src], y[src]
    return x, y, f32(rs.uniform(heading[0], heading[1], n))


def crowd_world(W, H, crowds, seed, dead=0.0, chem_patch=None, f16=False):
    """random_state's world (15 % of the cells, or half of them with dead slots) with the crowds put in: `crowds` = list of
    (n, rows, cols, heading).  Returns medium, agents, dir0, the crowd's slots."""
    rs = np.random.RandomState(seed)
    N0 = int(0.15 * W * H)
    N = N0 + sum(c[0] for c in crowds)
    K = N if not dead else N - int(dead * N)
    medium, agents = random_state(W, H, N, K, rs, collide=0.1)
    alive = np.nonzero(agents[2] > 0)[0]
    dir0 = f32(rs.uniform(-np.pi, np.pi, N))
    slots, at = [], 0
    for n, rows, cols, heading in crowds:
        idx = alive[at:at + n]
        at += n
        agents[0, idx], agents[1, idx], dir0[idx] = crowd_agents(rs, n, rows, cols, W, H, heading)
        slots.append(idx)
    agents[3, alive] = f32(0.1 + 0.9 * rs.rand(len(alive)))
    if chem_patch is not None:                                # no gradient around the crowd: it walks ahead, turning ±turn_angle
        (r0, r1), (c0, c1) = chem_patch
        medium[2, r0:r1, c0:c1] = 0.
    medium[0] = 0.
    medium[0][R.cell(agents[0, alive], W), R.cell(agents[1, alive], H)] = 1.
    if f16:
        medium[1:] = medium[1:].astype(np.float16).astype(np.float64)
    return medium, agents, dir0, slots


def physarum_kw(W, H):
    return dict(scale=1.53 / (max(W, H) - 1), sense_offset=10.2 / (max(W, H) - 1))


def dynamics(die, boundary='wrap', sigma=0.5):
    return die.Dynamics(boundary=die.BoundaryCondition(boundary), diffuse_sigma=sigma)


# ------------------------------------------------------------------------------------------------ 1. crowd states vs the oracle
# (three rows of tiles, eight columns: an order table of bands one tile wide, 24 tiles — ONE crowded tile passes its threshold)
INTERIOR_CASES = [
    dict(W=192, H=512, tile=(6, 6), at=(64, 256), size=64, form='two launches'),
    dict(W=192, H=512, tile=(6, 6), at=(64, 256), size=64, form='three launches', threads=64),
    dict(W=96, H=1024, tile=(5, 7), at=(32, 512), size=32, f16=True, form='two launches', threads=448),
]


@pytest.mark.parametrize('case', INTERIOR_CASES, ids=lambda c: '-'.join(f'{k}{v}' for k, v in c.items() if k in ('tile', 'form', 'f16', 'threads')))
def test_crowd_in_one_tile_interior_vs_oracle(die, case):
    """About 3 050 agents (a crowd of 2 450 and the world's 15 %) in the interior of one tile, most of them staying: the agent kernel's workgroup of that tile takes 6–7
    8-wave rounds (with 64 threads: ~46 chunk trips of one wave), the field kernel's stayer loop runs from 2·BLOCK (more than 1 024
    stayers, a count that is no multiple of 4·512: the loop's ragged last trip), and the order table (two-launch form) sorts the tile
    into class 0–1.  The agents' step counter runs 30 → 32: the first step builds the table, the third rebuilds it.  Every step
    teacher-forced against the oracle."""
    W, H, tile = case['W'], case['H'], case['tile']
    (x0, y0), TX, TY = case['at'], 1 << tile[0], 1 << tile[1]
    m = 6                                                      # agents stay ≥ 6 cells from the tile's borders for 3 steps of 1.53 cells
    medium, agents, dir0, (crowd,) = crowd_world(W, H, [(2450, (x0 + m, x0 + TX - m), (y0 + m, y0 + TY - m), (-np.pi, np.pi))], seed=W + H,
                                                 f16=case.get('f16', False))
    book = Bookkeeping(agents, W, H, tile)
    _binned_steps_against_the_oracle(die, medium, agents, dynamics(die), tile, 'physarum', physarum_kw(W, H), 3, f16=case.get('f16', False),
                                     form=case['form'], dir0=dir0, k1_threads=case.get('threads', 0), calls=30, callback=book)
    info = book.report()
    print(info)
    t = (x0 >> tile[0]) * (H >> tile[1]) + (y0 >> tile[1])
    kb = book.steps[0]['kb_block']
    for d in book.steps:
        n, s = int(d['n_out'][t]), int(d['s_out'][t])
        assert 2560 < n <= 3584, f"agent kernel: the crowded tile holds {n} agents, not 6–7 8-wave rounds\n{info}"
        if case['form'] == 'two launches':
            assert s > 2 * kb and (s - 2 * kb) % (4 * kb) != 0, f"field kernel: {s} stayers do not take the stayer loop from 2·BLOCK ({2 * kb})\n{info}"
    if case['form'] == 'two launches':
        ntx, nty = W >> tile[0], H >> tile[1]
        assert [d['calls'] for d in book.steps] == [30, 31, 32]
        for d in book.steps:
            want = OM.order_table(d['n_in'] if d['calls'] in (30, 32) else book.steps[0]['n_in'], ntx, nty)
            assert OM.is_sorted(d['n_in'], ntx, nty), f'order table: not sorted at step {d["calls"]}\n{info}'
            assert np.array_equal(d['order'], want), f'order table at step {d["calls"]}'
            j, blen = t % nty // (nty // 8), (nty // 8) * ntx
            assert d['order'][j * blen] == t, f'order table: the crowded tile is not first in its band\n{info}'
            assert OM.order_class(d['n_in'][t]) <= 1


CORNER_CASES = [
    dict(agent='physarum', sigma=0.8, threads=448),
    dict(agent='gradient', sigma=0.5, threads=0),
]


@pytest.mark.parametrize('case', CORNER_CASES, ids=lambda c: '-'.join(f'{k}{v}' for k, v in c.items()))
def test_crowd_crossing_into_a_tile_corner_vs_oracle(die, case):
    """A crowd of 2 400 agents packed into the last 1.7 cells before a tile corner (3 000 GradientAgents in the last 3), heading diagonally across it: the tiles beyond
    it see more than 1 024 arrival candidates (3 or more of the agent kernel's rounds of PIC_LIST_CAP), the rim lists overflow on both
    sides of the corner — the crowd's tile (its field kernel scans its own leavers: scan_segment with l == 0) and the diagonal tile
    it walks into —, with sigma 0.8 (rim width R = 3) and a 7-wave agent kernel, or as GradientAgents with momentum whose _prev_grad
    rides through the crowded segments.  Teacher-forced against the oracle; the step counter passes 32 (the order table's rebuild)."""
    W, H, tile = 192, 512, (6, 6)
    cx, cy = 128, 320                                          # the high corner of tile (1, 4)
    head = (0.55, 0.75)
    gradient = case['agent'] == 'gradient'
    n, depth = (3000, 3.0) if gradient else (2400, 1.7)
    # (cell c covers [c − 0.5, c + 0.5) cells of the coordinate: the tile border lies at cx − 0.5)
    medium, agents, dir0, (crowd,) = crowd_world(W, H, [(n, (cx - 0.5 - depth, cx - 0.53), (cy - 0.5 - depth, cy - 0.53), head)], seed=31,
                                                 chem_patch=((cx - 24, cx + 24), (cy - 24, cy + 24)))
    if gradient:
        kw = dict(scale=2.0 / (H - 1), sense_offset=6.0 / (H - 1), inertia=0.9, noise_scale=0.025, normalized_grad=True)
        pg = f32(R.RefGradientAgent(agents.shape[1], seed=3)._prev_grad)
        pg[:, crowd] = f32(np.stack([np.cos(dir0[crowd]), np.sin(dir0[crowd])]))         # the crowd's momentum points across the corner
        dir0 = f32(np.arctan2(pg[1], pg[0]))
    else:
        kw, pg = physarum_kw(W, H), None
    book = Bookkeeping(agents, W, H, tile)
    _binned_steps_against_the_oracle(die, medium, agents, dynamics(die, sigma=case['sigma']), tile, case['agent'], kw, 3, dir0=dir0, prev_grad=pg,
                                     k1_threads=case['threads'], calls=31, callback=book)
    info = book.report()
    print(info)
    ntx, nty = W >> tile[0], H >> tile[1]
    a = (cx // 64 - 1) * nty + cy // 64 - 1
    rg = ring(a, ntx, nty)
    diag, right, below = rg[(1, 1)], rg[(1, 0)], rg[(0, 1)]
    cap = book.steps[0]['cap']
    assert cap == 224
    s1 = book.steps[1]                                          # the second step: the first one's leavers are the arrival candidates
    ncand = {k: book.candidates(s1, u) for k, u in (('diag', diag), ('right', right), ('below', below))}
    assert min(ncand.values()) > 2 * LIST_CAP, f'agent kernel: arrival candidates {ncand}: fewer than 3 rounds of PIC_LIST_CAP\n{info}'
    s0 = book.steps[0]
    assert s0['rim'][a] > cap, f"field kernel: the crowd's own rim list did not overflow ({s0['rim'][a]}): no scan_segment(l = 0)\n{info}"
    assert s0['n_out'][a] - s0['s_out'][a] > 2 * LIST_CAP, f'the crowd did not leave its tile\n{info}'
    assert max(d['rim'][diag] for d in book.steps[1:]) > cap, f'field kernel: the diagonal tile\'s rim list never overflowed\n{info}'
    assert max(d['rim'][right] for d in book.steps[1:]) > cap and max(d['rim'][below] for d in book.steps[1:]) > cap, \
        f'field kernel: the rim lists beyond the corner never overflowed\n{info}'
    assert [d['calls'] for d in book.steps] == [31, 32, 33]
    assert OM.is_sorted(s0['n_in'], ntx, nty), f'order table: not sorted at the first step\n{info}'
    for d in book.steps:
        want = OM.order_table(d['n_in'] if d['calls'] in (31, 32) else book.steps[1]['n_in'], ntx, nty)
        assert np.array_equal(d['order'], want), f'order table at step {d["calls"]}'


EDGE_CASES = [
    dict(boundary='wrap', dead=0.6, form='two launches'),
    dict(boundary='limit', dead=0.0, form='three launches'),
    dict(boundary='limit', dead=0.0, form='two launches'),
]


@pytest.mark.parametrize('case', EDGE_CASES, ids=lambda c: '-'.join(f'{k}{v}' for k, v in c.items()))
def test_crowd_on_the_world_edge_vs_oracle(die, case):
    """A crowd of 2 400 agents on the world's edge, walking across it.  'wrap': from tile row 0 across the seam into the last row of
    tiles — rim lists overflow on both sides of the seam, so the field kernels read overflowed segments through the periodic distance
    of scan_segment (rr > W/2 and rr < −W/2) and ring tiles that wrap; with 60 % dead slots behind the segments.  'limit': from the
    last row of tiles against the high edge — the crowd is pressed to 1 − 2^-32.  Teacher-forced against the oracle."""
    W, H, tile = 192, 512, (6, 6)
    ntx, nty = W >> tile[0], H >> tile[1]
    wrap = case['boundary'] == 'wrap'
    if wrap:
        rows, head = (0.0, 0.45), (np.pi - 0.3, np.pi - 0.15)                  # row 0, heading −x (not at ±π: a threshold of the forward)
    else:
        rows, head = (W - 1 - 1.6, W - 1 - 0.02), (0.15, 0.3)                  # heading +x
    cols = (300.0, 340.0)
    medium, agents, dir0, (crowd,) = crowd_world(W, H, [(2400, rows, cols, head)], seed=47, dead=case['dead'],
                                                 chem_patch=((0, 24), (270, 370)) if wrap else ((W - 24, W), (270, 370)))
    book = Bookkeeping(agents, W, H, tile)
    _binned_steps_against_the_oracle(die, medium, agents, dynamics(die, boundary=case['boundary']), tile, 'physarum', physarum_kw(W, H), 3,
                                     form=case['form'], dir0=dir0, callback=book)
    info = book.report()
    print(info)
    if wrap:
        top = [r * nty + c for r in (0, ntx - 1) for c in (4, 5)]
        for r in (0, ntx - 1):                                  # both sides of the seam held an overflowed list at some step
            assert any(d['rim'][r * nty + c] > d['cap'] for d in book.steps for c in (4, 5)), \
                f'field kernel: no overflowed rim list in tile row {r}: the periodic distance of scan_segment is not on the path\n{info}'
        s0 = book.steps[0]
        assert sum(int(s0['n_out'][t] - s0['s_out'][t]) for t in top[:2]) > 2 * LIST_CAP, f'the crowd did not cross the seam\n{info}'
    else:
        pressed = [int((d['x'] == 0xFFFFFFFF).sum()) for d in book.steps]
        assert min(pressed) > 500, f'limit: agents pressed to 1 − 2^-32 per step: {pressed}\n{info}'
        if case['form'] == 'two launches':
            assert any((d['rim'] > d['cap']).any() for d in book.steps), f'field kernel: no overflowed rim list\n{info}'


# ------------------------------------------------------------------------------------------------ 2. the order table, exactly
def _order_world(W, H, tile, crowded, seed, background=8):
    """All-alive world of `background` agents per tile plus exact crowds: `crowded` = {tile: population}.  Positions uniform in the
    tile's cells, continuous and distinct."""
    rs = np.random.RandomState(seed)
    xs, ys = tile
    ntx, nty = W >> xs, H >> ys
    pop = np.full(ntx * nty, background, dtype=np.int64)
    for t, n in crowded.items():
        pop[t] = n
    t = np.repeat(np.arange(ntx * nty), pop)
    N = len(t)
    medium, agents = random_state(W, H, N, N, rs, collide=0.0)
    tx, ty = t // nty, t % nty
    # cell labels: cell(x, W) = round(x·(W − 1)); stay half a cell inside the tile's first and last cells
    for k, (u, s, L) in enumerate(((tx, xs, W), (ty, ys, H))):
        lo, hi = np.maximum((u << s) - 0.49, 0.0), np.minimum((u << s) + (1 << s) - 0.51, L - 1.001)
        agents[k] = q32((lo + (hi - lo) * rs.rand(N)) / (L - 1))
    medium[0] = 0.
    medium[0][R.cell(agents[0], W), R.cell(agents[1], H)] = 1.
    dir0 = f32(rs.uniform(-np.pi, np.pi, N))
    assert np.array_equal(tile_populations(agents, W, H, tile), pop)
    return medium, agents, dir0, pop


def _order_run(die, medium, agents, dir0, tile, steps, calls=0, events=False, form='two launches'):
    """`steps` device steps; per step the populations of the layout it read, the order table after it, actions and rewards."""
    W, H = medium.shape[1:]
    N = agents.shape[1]
    env = die.Env.from_numpy(medium, agents, sort_every=0, pic=True)
    env._pic_tile = tile
    env._pic_fused = form != 'three launches'
    ag = die.PhysarumAgent(max_agents=N, seed=5, **physarum_kw(W, H))
    ag.set_state(dir0)
    ag._calls = calls
    obs = env._get_current_obs
    pops, tables, acts, rewards = [], [], [], []
    first = tile_populations(agents, W, H, tile)
    for i in range(steps):
        pic = env._pic
        pops.append(first if pic is None else pic.meta[pic.cur][1].cpu().numpy().astype(np.int64))
        if events:
            env._pic_events = [torch.cuda.Event() for _ in range(3 if form == 'two launches' else 4)]
        a = ag.forward(obs)
        obs, rew, _, _, info = env.step(a)
        env._pic_events = None
        acts.append(a.to_numpy())
        rewards.append((rew, info['num_agents']))
        pic = env._pic
        assert pic is not None and pic.held[0] is env.agents.x and pic.two_launch(env, ag) == (form == 'two launches')
        tables.append(pic.order.cpu().numpy().astype(np.int64) & 0xFFFF if pic.order is not None else None)
    return env, ag, pops, tables, np.stack(acts), np.array(rewards)


SMALL = dict(W=128, H=512, tile=(4, 5))             # 8 × 16 tiles of 16 × 32 cells: 128 tiles, bands of 16, threshold 3 crowded tiles


def _small_crowds(n_crowded):
    ntx, nty = SMALL['W'] >> 4, SMALL['H'] >> 5
    b = [OM.band_tiles(ntx, nty, j) for j in range(8)]
    # band 0: a tile of 6 rounds ahead of one of 7 (classes 1 and 0: merged, they would keep this order), a class-4 tile (not crowded)
    # ahead of both; band 3: one of 4 rounds at its end.  Sorting moves all of them.
    crowd = {b[0][9]: 1536, b[0][13]: 2800, b[0][15]: 3300, b[3][14]: 1700}
    if n_crowded == 2:
        del crowd[b[3][14]]
    return crowd


@pytest.mark.parametrize('n_crowded', [3, 2], ids=['at the threshold', 'one crowded tile short'])
def test_order_table_equals_the_host_model(die, n_crowded):
    """The device's order table against tests/order_model.py, exactly: built at the first step from the populations the step reads,
    unchanged through step 31, rebuilt at step 32 from that step's read layout.  A world exactly at the all-bands threshold (3 crowded
    tiles of 128: sorted, with classes 0 and 1 in one band) and one crowded tile short of it (band order)."""
    W, H, tile = SMALL['W'], SMALL['H'], SMALL['tile']
    ntx, nty = W >> tile[0], H >> tile[1]
    medium, agents, dir0, pop = _order_world(W, H, tile, _small_crowds(n_crowded), seed=11 + n_crowded)
    assert OM.crowded_tiles(pop, ntx, nty) == n_crowded and OM.is_sorted(pop, ntx, nty) == (n_crowded == 3)
    env, ag, pops, tables, _, _ = _order_run(die, medium, agents, dir0, tile, 35)
    assert np.array_equal(pops[0], pop)
    first = OM.order_table(pop, ntx, nty)
    assert np.array_equal(tables[0], first), f'order table of the first step (crowded tiles: {n_crowded})'
    if n_crowded == 3:
        assert not np.array_equal(first, OM.band_order(ntx, nty))
    else:
        assert np.array_equal(first, OM.band_order(ntx, nty))
    # (the populations of step 16 must change the table, or the next check could not see a rebuild every 16th step)
    assert n_crowded == 2 or not np.array_equal(OM.order_table(pops[16], ntx, nty), first)
    for i in range(1, 32):
        assert np.array_equal(tables[i], first), f'order table changed at step {i}: rebuilt off the period of 32'
    rebuilt = OM.order_table(pops[32], ntx, nty)
    for i in range(32, 35):
        assert np.array_equal(tables[i], rebuilt), f'order table at step {i}: not the rebuild of step 32 from its read layout'


def test_order_table_of_bands_of_768_equals_the_host_model(die):
    """96 × 64 tiles (bands of 768: 256 tiles ahead of each band's last span of 512), a crowd in the last rows of tiles of the first
    band (test_order_table_of_the_two_launch_form's): the device's table equals the model at the first step and after the rebuild."""
    W, H, N, tile = 1536, 2048, 440000, (4, 5)
    ntx, nty = W >> tile[0], H >> tile[1]
    rs = np.random.RandomState(5)
    medium, agents = random_state(W, H, N, N, rs, collide=0.2)
    nc = 330000
    agents[0, :nc] = rs.uniform(0.80, 0.995, nc)
    agents[1, :nc] = rs.uniform(0.001, 0.115, nc)
    agents[:2] = q32(agents[:2])
    dir0 = f32(np.floor(rs.uniform(-np.pi, np.pi, N) / np.radians(30)) * np.radians(30))
    _, _, pops, tables, _, _ = _order_run(die, medium, agents, dir0, tile, 3, calls=31)
    assert OM.is_sorted(pops[0], ntx, nty) and OM.crowded_tiles(pops[0], ntx, nty) >= 96
    for i, built_from in ((0, 0), (1, 1), (2, 1)):
        assert np.array_equal(tables[i], OM.order_table(pops[built_from], ntx, nty)), f'order table at step {31 + i}'
    assert not np.array_equal(tables[0], OM.band_order(ntx, nty))


# ------------------------------------------------------------------------------------------------ 3. split launches
@pytest.mark.parametrize('form', ['two launches', 'three launches'])
def test_split_launch_step_equals_the_one_call_step(die, form):
    """Steps issued one library call per stage with events between them (die_pic.stages 1, 2 / 1, 2, 4: how bench.py times each
    kernel) give the bits of the one-call step — medium, agents, heading, actions, rewards — in a crowded world whose order table is
    sorted, across the table's rebuild at step 32."""
    W, H, tile = SMALL['W'], SMALL['H'], SMALL['tile']
    ntx, nty = W >> tile[0], H >> tile[1]
    medium, agents, dir0, pop = _order_world(W, H, tile, _small_crowds(3), seed=17)
    outs = []
    for events in (False, True):
        env, ag, pops, tables, acts, rewards = _order_run(die, medium, agents, dir0, tile, 5, calls=29, events=events, form=form)
        if form == 'two launches':
            assert OM.is_sorted(pops[0], ntx, nty) and np.array_equal(tables[0], OM.order_table(pops[0], ntx, nty))
            assert np.array_equal(tables[4], OM.order_table(pops[3], ntx, nty))          # (rebuilt at step 32 = the fourth)
        outs.append((env.medium.to_numpy(), env.agents.to_numpy(), ag.direction_rads_numpy(), acts, rewards))
    for name, a, b in zip(('medium', 'agents', 'heading', 'actions', 'rewards'), outs[0], outs[1]):
        assert np.array_equal(a, b), name


# ------------------------------------------------------------------------------------------------ 4. the aggregated benchmark world
def test_bench_world_after_1024_steps_teacher_forced_vs_oracle(die):
    """The benchmark's world (4096², ratio 0.15, max_agents='alive', its PhysarumAgent) run freely on the device for 1 024 steps
    (Env.run), then ONE step teacher-forced against the oracle: the agent's step 1 024, where the order table is rebuilt.  By then the
    agents have aggregated: the table is sorted and rim lists overflow — asserted before the comparison."""
    W = H = 4096
    env = die.Env((W, H), die.Dynamics(init_agent_ratio=0.15), seed=1234, max_agents='alive', sync=False)
    N = env.agents.N
    kw = dict(scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1), turn_angle=30, sense_angle=90, turn_tolerance=0.1, deposit=4.0)
    dev, ref = die.PhysarumAgent(max_agents=N, seed=1234, **kw), R.RefPhysarumAgent(N, seed=1234, **kw)
    env.run(dev, 1024)
    env.check()
    assert dev._calls == 1024
    ref._calls = dev._calls                                 # (the Philox step counter of the oracle's agent keeps pace)
    pic = env._pic
    assert pic is not None and pic.held[0] is env.agents.x and pic.two_launch(env, dev) and pic.order is not None
    ntx, nty = W >> pic.xs, H >> pic.ys
    pop = pic.meta[pic.cur][1].cpu().numpy().astype(np.int64)
    crowded = OM.crowded_tiles(pop, ntx, nty)
    assert OM.is_sorted(pop, ntx, nty), f'{crowded} crowded tiles at step 1 024: the order table does not sort'
    m0, a0 = env.medium.to_numpy(), env.agents.to_numpy()
    d0 = dev.direction_rads_numpy()
    ref._direction_rads = d0.copy()
    rd = R.RefDynamics(rate_feed=float(np.float32(0.1)), rate_decay_chem=float(np.float32(0.1)), diffuse_sigma=0.5)
    renv = R.RefEnv(m0, a0, rd)
    want_action = ref.forward(renv.obs)
    obs = env._get_current_obs
    action = dev.forward(obs)
    obs, res, *_ = env.step(action)
    reward, num_agents = env.read_result(res)
    cap = int(_lib().lib.die_pic_rim_cap(pic.xs, pic.ys))
    over = int((pic.rim_cnt.cpu().numpy() > cap).sum())
    assert over > 0, 'no rim list overflowed at step 1 024'
    table = pic.order.cpu().numpy().astype(np.int64) & 0xFFFF
    assert np.array_equal(table, OM.order_table(pop, ntx, nty)), 'order table rebuilt at step 1 024'
    assert not np.array_equal(table, OM.band_order(ntx, nty))
    print(f'bench world at step 1 024: {crowded} crowded tiles, {over} rim lists over {cap}, max population {pop.max()}')
    got_action = action.to_numpy()
    bad = ~np.isclose(got_action, want_action, rtol=RTOL, atol=1e-6 * kw['scale']).all(axis=0)
    assert_forward_mismatches_explained(bad, physarum_margins(ref, a0, m0, d0, W, H), N)
    _, want_reward, _, _, want_info = renv.step(applied(got_action))
    ga = env.agents.to_numpy()
    assert np.array_equal(ga[:3], renv.agents[:3])
    assert np.allclose(ga[3], renv.agents[3], rtol=RTOL, atol=1e-7)
    del ga
    owner = env.medium.owner_slots().cpu().numpy()
    ix, iy = R.cell(renv.agents[0], W), R.cell(renv.agents[1], H)
    want_owner = np.full((W, H), -1, dtype=np.int64)
    want_owner[ix, iy] = np.arange(N)
    assert np.array_equal(owner, want_owner)
    del owner, want_owner
    gm = env.medium.to_numpy()
    assert np.array_equal(gm[0], renv.medium[0])
    assert np.allclose(gm[1], renv.medium[1], rtol=RTOL, atol=1e-8)
    assert np.allclose(gm[2], renv.medium[2], rtol=RTOL, atol=1e-7)
    assert num_agents == want_info['num_agents'] == N
    assert abs(reward - want_reward) <= RTOL * np.abs(renv.last_gained).sum() + 1e-9
