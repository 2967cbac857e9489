"""The order table's tail form (die_amd/csrc/die_pic.hip `k_pic_order`, include/die_hip.h `die_pic.order`): below the crowd
threshold every XCD band keeps band order except for its share of the agent-kernel launch's last, partial round of workgroups, which
takes the band's lightest tiles.

The model here is written from that specification, not from the kernel.  NT tiles on `slots` resident workgroups end in a round of
r = NT mod slots workgroups, ids [NT − r, NT); band j's table place k belongs to workgroup 8k + j, so its share `tail` is the number of
k with 8k + j ≥ NT − r.  No tail is shaped (band order) when r = 0, when 8r > 7·slots, or when the largest share exceeds the band's
last span; a share of the whole span is band order again.  Otherwise the span's `tail` lightest tiles — among tiles of one population
the ones LAST in band order — fill the last `tail` places in band order, and the other tiles the places ahead, in band order.

`slots` is passed through the host glue (`env._pic_order_slots`), so that worlds of a few hundred tiles have a partial last round; the
library's own figure (the device's CUs × resident workgroups) exceeds their tile counts, which is the whole-span case.
DIE_PIC_ORDER_TAIL=0 / DIE_PIC_ORDER=0 are read when the step's state is created: fresh Env objects in one process."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import order_model as OM                                          # noqa: E402
from tests.test_gpu_crowds import _order_world, physarum_kw                  # noqa: E402
from tests.test_gpu_parity import f32, random_state                          # noqa: E402

TILE = (4, 5)                                  # 16 × 32 cells
BIG = dict(W=256, H=512)                       # 16 × 16 tiles: bands of 32 (two tile columns), crowd threshold 6 tiles
FLAT = dict(W=48, H=256)                       # 3 × 8 tiles: bands of 3 (one tile column)
STEPS = 35                                     # the agent's step counter passes 32: a rebuild mid-run


@pytest.fixture(scope='module')
def die():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import die_amd
    return die_amd


# ------------------------------------------------------------------------------------------------ the model
def shares(ntx, nty, slots):
    """Per band: table places whose workgroup lies in the launch's last partial round; None: no tail is shaped."""
    NT, blen = ntx * nty, ntx * (nty // 8)
    r = NT % slots
    if r == 0 or 8 * r > 7 * slots:
        return None
    sh = [sum(8 * k + j >= NT - r for k in range(blen)) for j in range(8)]
    return None if max(sh) > OM.last_span(ntx, nty)[1] else sh


def tail_table(pop, ntx, nty, slots):
    """The table of a world below the crowd threshold."""
    assert not OM.is_sorted(pop, ntx, nty)
    sh = shares(ntx, nty, slots)
    if sh is None:
        return OM.band_order(ntx, nty)
    q0, ln = OM.last_span(ntx, nty)
    out = []
    for j in range(8):
        band = OM.band_tiles(ntx, nty, j)
        span = band[q0:]
        if 0 < sh[j] < ln:
            light = sorted(range(ln), key=lambda i: (pop[span[i]], -i))[:sh[j]]
            keep = [i for i in range(ln) if i not in light]
            span = span[keep + sorted(light)]
        out += [band[:q0], span]
    return np.concatenate(out)


def check_shape(table, pop, ntx, nty, slots):
    """What the table must satisfy whatever the rule among equal populations."""
    sh = shares(ntx, nty, slots) or [0] * 8
    q0, ln = OM.last_span(ntx, nty)
    blen = ntx * (nty // 8)
    for j in range(8):
        band, got = OM.band_tiles(ntx, nty, j), table[j * blen:(j + 1) * blen]
        assert sorted(got.tolist()) == sorted(band.tolist()), f'band {j}: not a permutation of its tiles'
        tail = sh[j] if sh[j] < ln else 0
        place = {t: q for q, t in enumerate(band.tolist())}
        head, end = [place[t] for t in got[:blen - tail]], [place[t] for t in got[blen - tail:]]
        assert head == sorted(head), f'band {j}: the tiles ahead of the tail are not in band order'
        assert end == sorted(end), f'band {j}: the tail is not in band order'
        assert head[:q0] == list(range(q0)), f'band {j}: a tile ahead of the last span has moved'
        if tail:
            assert pop[got[blen - tail:]].max() <= pop[got[q0:blen - tail]].min(), f'band {j}: a tail tile is heavier than a tile left ahead'


# ------------------------------------------------------------------------------------------------ worlds and runs
def uneven_world(W, H, crowded=2, seed=3):
    """Populations 4 … 60 with many equal ones, `crowded` tiles of four rounds and more — put where band order would run them last."""
    ntx, nty = W >> TILE[0], H >> TILE[1]
    rs = np.random.RandomState(seed)
    pop = {t: int(n) for t, n in enumerate(rs.randint(2, 31, ntx * nty) * 2)}
    for j in range(crowded):
        pop[int(OM.band_tiles(ntx, nty, j % 8)[-1 - j // 8])] = 1600 + 40 * j
    return _order_world(W, H, TILE, pop, seed=seed)


def run(die, monkeypatch, world, steps, slots=0, tail='1', order='1', tile=TILE):
    """`steps` steps of a fresh Env: the table after every step, the populations every step read, and what the run leaves."""
    medium, agents, dir0 = world[:3]
    W, H = medium.shape[1:]
    N = agents.shape[1]
    monkeypatch.setenv('DIE_PIC_ORDER', order)
    monkeypatch.setenv('DIE_PIC_ORDER_TAIL', tail)
    env = die.Env.from_numpy(medium, agents, sort_every=0, pic=True)
    env._pic_tile = tile
    env._pic_order_slots = slots
    ag = die.PhysarumAgent(max_agents=N, seed=5, **physarum_kw(W, H))
    ag.set_state(dir0)
    obs = env._get_current_obs
    tables, pops, rewards = [], [], []
    for _ in range(steps):
        pic = env._pic
        pops.append(None if pic is None else pic.meta[pic.cur][1].cpu().numpy().astype(np.int64))
        obs, rew, _, _, info = env.step(ag.forward(obs))
        rewards.append((rew, info['num_agents']))
        pic = env._pic
        assert pic is not None and pic.held[0] is env.agents.x and pic.two_launch(env, ag), 'the two-launch tile-binned step did not run'
        tables.append(None if pic.order is None else pic.order.cpu().numpy().astype(np.int64) & 0xFFFF)
    return tables, pops, (env.medium.to_numpy(), env.agents.to_numpy(), ag.direction_rads_numpy(), np.array(rewards))


def same_bits(a, b, what):
    for name, u, v in zip(('medium', 'agents', 'heading', 'rewards'), a, b):
        assert np.array_equal(u, v), f'{what}: {name}'


@pytest.fixture(scope='module')
def big(die):
    """The 16 × 16-tile world over 35 steps in its three forms (and with a second `slots`): shared by the tests below."""
    world = uneven_world(**BIG)
    with pytest.MonkeyPatch.context() as mp:
        runs = {key: run(die, mp, world, STEPS, **kw) for key, kw in (
            (24, dict(slots=24)), (44, dict(slots=44)), ('no tail', dict(slots=24, tail='0')), ('no table', dict(slots=24, order='0')))}
    return world, runs


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize('slots', [24, 44])
def test_tail_form_on_an_uneven_world(big, slots):
    """256 tiles on 24 places: a last round of 16 workgroups, two per band; on 44 places: 36 workgroups, four in bands 0–3 and five
    in bands 4–7.  The table of the first step (from the binned populations) and of the rebuild at step 32 (from the layout that step
    read): a permutation of every band, both parts in band order, no tail tile heavier than a tile ahead — and exactly the model's."""
    world, runs = big
    pop0 = world[3]
    ntx, nty = BIG['W'] >> TILE[0], BIG['H'] >> TILE[1]
    sh = shares(ntx, nty, slots)
    assert sh == ([2] * 8 if slots == 24 else [4] * 4 + [5] * 4)
    tables, pops, _ = runs[slots]
    for i, pop in ((0, pop0), (31, pop0), (32, pops[32]), (STEPS - 1, pops[32])):
        check_shape(tables[i], pop, ntx, nty, slots)
        assert np.array_equal(tables[i], tail_table(pop, ntx, nty, slots)), f'order table after step {i}'
    # the crowded tiles, last in their bands, have left the tail; the table is not band order
    blen = ntx * (nty // 8)
    assert pop0[tables[0][blen - 1]] < 100 and pop0[OM.band_tiles(ntx, nty, 0)[-1]] >= 1600
    assert not np.array_equal(tables[0], OM.band_order(ntx, nty))
    assert not np.array_equal(tables[32], tables[0]), 'the rebuild at step 32 found the populations of the first step'


def test_tail_form_changes_no_result(big):
    """35 steps with the tail form, with DIE_PIC_ORDER_TAIL=0 (band order below the crowd threshold) and with DIE_PIC_ORDER=0 (no
    table): planes, agent arrays in slot order, headings and result words bit for bit."""
    _, runs = big
    ntx, nty = BIG['W'] >> TILE[0], BIG['H'] >> TILE[1]
    assert all(np.array_equal(t, OM.band_order(ntx, nty)) for t in runs['no tail'][0]), 'DIE_PIC_ORDER_TAIL=0: not band order'
    assert all(t is None for t in runs['no table'][0]), 'DIE_PIC_ORDER=0: a table exists'
    for key in (44, 'no tail', 'no table'):
        same_bits(runs[24][2], runs[key][2], f'tail form on 24 places against {key}')


@pytest.mark.parametrize('slots,want', [(16, [1] * 8), (20, [0] * 4 + [1] * 4), (32, [3] * 8), (24, None)])
def test_bands_of_three_tiles(die, monkeypatch, slots, want):
    """3 × 8 tiles, one tile column per band: a share of one tile, of none in some bands and one in the others (20 places: no multiple
    of 8), of the whole band (fewer tiles than places), and a full last round — each a valid permutation, the last two band order."""
    ntx, nty = FLAT['W'] >> TILE[0], FLAT['H'] >> TILE[1]
    world = uneven_world(**FLAT, crowded=0, seed=9)
    assert shares(ntx, nty, slots) == want
    tables, _, _ = run(die, monkeypatch, world, 1, slots=slots)
    check_shape(tables[0], world[3], ntx, nty, slots)
    assert np.array_equal(tables[0], tail_table(world[3], ntx, nty, slots))
    if slots in (32, 24):
        assert np.array_equal(tables[0], OM.band_order(ntx, nty))


def test_world_of_three_by_three_tiles_has_no_table(die, monkeypatch):
    """192 × 192 cells in 64 × 64 tiles: three tiles per row do not divide into eight bands, so no order table exists and the
    workgroups take the plain mapping — whatever the two switches say, with the same bits."""
    rs = np.random.RandomState(2)
    N = 6000
    medium, agents = random_state(192, 192, N, N, rs, collide=0.2)
    world = (medium, agents, f32(rs.uniform(-np.pi, np.pi, N)))
    outs = []
    for kw in (dict(), dict(tail='0'), dict(order='0')):
        tables, _, out = run(die, monkeypatch, world, STEPS, slots=4, tile=(6, 6), **kw)
        assert all(t is None for t in tables)
        outs.append(out)
    same_bits(outs[0], outs[1], 'DIE_PIC_ORDER_TAIL=0')
    same_bits(outs[0], outs[2], 'DIE_PIC_ORDER=0')


@pytest.mark.parametrize('slots', [32, 37], ids=['a full last round', 'a last round above 7/8'])
def test_no_tail_to_shape_is_band_order(die, monkeypatch, slots):
    """256 tiles on 32 places (eight full rounds) and on 37 (a last round of 34): band order, the table of DIE_PIC_ORDER_TAIL=0."""
    ntx, nty = BIG['W'] >> TILE[0], BIG['H'] >> TILE[1]
    world = uneven_world(**BIG)
    assert shares(ntx, nty, slots) is None
    on, _, _ = run(die, monkeypatch, world, 1, slots=slots)
    off, _, _ = run(die, monkeypatch, world, 1, slots=slots, tail='0')
    assert np.array_equal(on[0], OM.band_order(ntx, nty)) and np.array_equal(on[0], off[0])


def test_crowded_world_keeps_the_crowded_first_table(die, monkeypatch):
    """Six crowded tiles of 256 — the threshold — with a partial last round: the crowded-first table (tests/order_model.py: every
    band's last span sorted by rounds class, stable), not the tail form."""
    ntx, nty = BIG['W'] >> TILE[0], BIG['H'] >> TILE[1]
    world = uneven_world(**BIG, crowded=6)
    pop = world[3]
    assert OM.is_sorted(pop, ntx, nty) and shares(ntx, nty, 24) == [2] * 8
    on, _, _ = run(die, monkeypatch, world, 1, slots=24)
    want = OM.order_table(pop, ntx, nty)
    assert np.array_equal(on[0], want) and not np.array_equal(want, OM.band_order(ntx, nty))
