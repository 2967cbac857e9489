"""The agent kernel's bookkeeping off the serial path (die_amd/csrc/die_pic.hip `k_pic_forward_move`, round 9): the candidate search
from registers (`pic_cand_source`: the nine range lengths and bases read once, prefix sums per thread, comparisons and selects instead
of a loop of dependent LDS reads) and the epilogue's 64-bit sums without LDS shuffles (`die_wave_sum_i64_dpp`, die_common.h: one LDS
add per wave, one word read by thread 0).  None of it computes anything but indices and integer sums, so every world below is stepped by
the tile-binned step and by the classic step and compared bit for bit — fields, agents, headings, ownership, actions, reward and agent
count of every step —, the error word must stay 0 and the tiles' reward partials must add up to the step's reward.

Which range a candidate comes from: a tile's candidates are the LEAVERS of its eight neighbours in the layout the step reads — the
agents that walked off their tile in the step before.  A world whose agents stand in some tiles only therefore gives the other tiles
empty ranges between full ones; in 3 × 3 tiles every tile is every other tile's neighbour (through the seam), so one tile's leavers
show up as another range index in each of the eight others."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_parity import f32, q32, random_state                     # noqa: E402

STEPS = 4


@pytest.fixture(scope='module')
def die():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import die_amd
    return die_amd


def physarum(die, N, W, H, dir0):
    ag = die.PhysarumAgent(max_agents=N, seed=5, scale=1.53 / (max(W, H) - 1), sense_offset=10.2 / (max(W, H) - 1))
    ag.set_state(dir0)
    return ag


def binned_equals_classic(die, W, H, tile, medium, agents, dir0, f16=False, threads=0, steps=STEPS, expect_special=None):
    """`steps` steps by the tile-binned step and by the classic one: the same bits.  Returns the binned run's PicState and its
    per-step per-tile words (n, s of the layout each step wrote) for the caller's own assertions."""
    from die_amd import _lib
    N = agents.shape[1]
    outs, pic_state, words = [], None, []
    for pic in (True, False):
        env = die.Env.from_numpy(medium, agents, sort_every=0, pic=pic, field_dtype=torch.float16 if f16 else torch.float32)
        env._pic_tile = tile if pic else None
        if pic and threads:
            env._pic_k1_threads = threads
        ag = physarum(die, N, W, H, dir0)
        obs = env._get_current_obs
        acts, rewards = [], []
        before = int(_lib.lib.die_pic_k1_specialised_launches())
        for i in range(steps):
            action = ag.forward(obs)
            obs, rew, _, _, info = env.step(action)
            acts.append(action.to_numpy())
            rewards.append((rew, info['num_agents']))
            if pic:
                p = env._pic
                assert p is not None and p.held[0] is env.agents.x and p.two_launch(env, ag), 'the two-launch tile-binned step did not run'
                assert (p.xs, p.ys) == tuple(tile)
                assert int(p.error[0].item()) == 0, f'error word after step {i}'
                # the tiles' reward partials (32.32 fixed point) are the step's reward
                assert int(p.part[:p.NT].sum().item()) / 2.0 ** 32 == rew, f'part_gain total of step {i}'
                words.append((p.meta[p.cur][1].cpu().numpy().copy(), p.meta[p.cur][2].cpu().numpy().copy(), p.part[:p.NT].cpu().numpy().copy()))
        if pic:
            pic_state = env._pic
            special = int(_lib.lib.die_pic_k1_specialised_launches()) - before
            if expect_special is not None:
                assert (special == steps) if expect_special else (special == 0), f'{special} specialised launches of {steps}'
            env.check()
        outs.append((env.medium.to_numpy(), env.agents.to_numpy(), ag.direction_rads_numpy(), env.medium.owner_slots().cpu().numpy(),
                     np.stack(acts), np.array(rewards)))
    for name, a, b in zip(('medium', 'agents', 'heading', 'owners', 'actions', 'rewards'), outs[0], outs[1]):
        assert np.array_equal(a, b), name
    return pic_state, words


def placed_world(W, H, groups, seed, f16=False, flat=False):
    """random_state's fields with exactly the agents of `groups`: (n, rows, cols, heading range) — positions uniform in the cell
    rectangle rows × cols (cell units), headings uniform in the range.  flat: no chem, so nobody steers — everybody turns ± 30° and
    walks ≈ 1.3 cells ahead."""
    rs = np.random.RandomState(seed)
    N = sum(g[0] for g in groups)
    medium, agents = random_state(W, H, max(N, 2), max(N, 2), rs, collide=0.0)
    agents = agents[:, :N]
    dir0 = np.zeros(N)
    at = 0
    for n, rows, cols, heading in groups:
        agents[0, at:at + n] = q32((rows[0] + (rows[1] - rows[0]) * rs.rand(n)) / (W - 1))
        agents[1, at:at + n] = q32((cols[0] + (cols[1] - cols[0]) * rs.rand(n)) / (H - 1))
        dir0[at:at + n] = rs.uniform(heading[0], heading[1], n)
        at += n
    if flat:
        medium[2] = 0.
    if f16:
        medium[1:] = medium[1:].astype(np.float16).astype(np.float64)
    from oracle import cpu_ref as R
    medium[0] = 0.
    medium[0][R.cell(agents[0], W), R.cell(agents[1], H)] = 1.
    return medium, agents, f32(dir0)


@pytest.fixture(params=[False, True], ids=['specialised', 'DIE_PIC_K1_GENERIC=1'])
def generic(request, monkeypatch):
    monkeypatch.setenv('DIE_PIC_K1_GENERIC', '1' if request.param else '0')
    return request.param


ANY = (-np.pi, np.pi)


# ------------------------------------------------------------------------------------------------ 1. empty ranges in the search
def test_leavers_of_one_neighbour_only(die, generic):
    """192 × 192 in 3 × 3 tiles.  900 agents in the last rows of tile (0, 0) only, heading across its border with tile (1, 0): from
    the second step on, (0, 0)'s leavers are the ONLY candidates of every other tile — one full range between empty ones, at another
    range index in each —, and (0, 0) itself has no candidates at all."""
    medium, agents, dir0 = placed_world(192, 192, [(900, (58.0, 63.4), (8.0, 56.0), (-0.2, 0.2))], 3, flat=True)
    pic, words = binned_equals_classic(die, 192, 192, (6, 6), medium, agents, dir0, expect_special=not generic)
    n_last = words[-1][0]
    assert n_last[3] > 0 and n_last[0] + n_last[3] == 900, 'the agents did not cross into tile (1, 0) alone'
    assert sum(int(n[0] - s[0]) > 0 for n, s, _ in words[:-1]) >= 2, 'tile (0, 0) had leavers in fewer than two of the layouts a step read'


def test_some_ranges_empty_and_others_full(die, generic):
    """192 × 192 in 3 × 3 tiles.  Agents near the borders of tiles (0, 0), (1, 1) and (2, 0) only, headings anywhere: three of a
    tile's eight neighbour ranges hold leavers, the five between them are empty (equal consecutive prefixes in the search)."""
    groups = [(700, (0.5, 63.4), (0.5, 63.4), ANY), (650, (64.5, 127.4), (64.5, 127.4), ANY), (300, (128.5, 191.0), (0.5, 63.4), ANY)]
    groups += [(250, (60.0, 63.4), (1.0, 63.0), (-0.3, 0.3)), (250, (64.5, 68.0), (65.0, 127.0), (np.pi - 0.3, np.pi)),
               (200, (129.0, 190.0), (0.5, 3.0), (-np.pi / 2 - 0.3, -np.pi / 2 + 0.3))]
    medium, agents, dir0 = placed_world(192, 192, groups, 4)
    binned_equals_classic(die, 192, 192, (6, 6), medium, agents, dir0, expect_special=not generic)


# ------------------------------------------------------------------------------------------------ 2. second filter trip, later list rounds
@pytest.mark.parametrize('threads', [0, 192], ids=['512 threads', '192 threads'])
def test_crowd_of_1300_crossing_one_border(die, generic, threads):
    """192 × 192 in 3 × 3 tiles.  1 300 agents in a strip below the border at row 64, columns of tile (0, 1), all heading across it
    over a flat chem plane: tile (1, 1) then sees more than 1 024 candidates in ONE neighbour range — three rounds of the arrival list
    (512 per round), the later ones through the search of the `c0 > 0` trip.  With 192 threads per workgroup (always the generic
    instantiation) a round takes three filter trips."""
    groups = [(1300, (62.2, 63.45), (70.0, 120.0), (-0.05, 0.05)), (400, (0.5, 191.0), (0.5, 191.0), ANY)]
    medium, agents, dir0 = placed_world(192, 192, groups, 5, flat=True)
    pic, words = binned_equals_classic(die, 192, 192, (6, 6), medium, agents, dir0, threads=threads,
                                       expect_special=(not generic) and threads == 0)
    n0, s0, _ = words[0]                  # the layout step 1 wrote: tile (0, 1) = index 1 holds the crowd as leavers
    assert n0[1] - s0[1] > 1024, f'{n0[1] - s0[1]} leavers of tile (0, 1): the crowd did not cross'
    assert words[1][0][4] > 1024, 'tile (1, 1) did not take the crowd in'


# ------------------------------------------------------------------------------------------------ 3. tile populations at the chunk boundaries
POPULATIONS = [0, 1, 63, 64, 65, 512, 513, 1100, 200]


def test_tile_populations_at_the_chunk_boundaries(die, generic):
    """192 × 192 in 3 × 3 tiles holding 0, 1, 63, 64, 65, 512, 513, 1 100 and 200 agents, all at least 8 cells inside their tile (a step is
    1.53 cells: nobody leaves in four steps, the populations hold): a wave's first chunk is fixed, later chunks come from the
    counter — 512 and 513 agents are the last without and the first with a counter chunk.  The empty tile's sums are zero."""
    groups = []
    for t, n in enumerate(POPULATIONS):
        tx, ty = divmod(t, 3)
        if n:
            groups.append((n, (tx * 64 + 8.0, tx * 64 + 56.0), (ty * 64 + 8.0, ty * 64 + 56.0), ANY))
    medium, agents, dir0 = placed_world(192, 192, groups, 6)
    pic, words = binned_equals_classic(die, 192, 192, (6, 6), medium, agents, dir0, expect_special=not generic)
    for n, s, part in words:
        assert list(n) == POPULATIONS and list(s) == POPULATIONS, 'the populations moved'
        assert part[0] == 0, 'reward partial of the empty tile'
    assert int(pic.rim_cnt[0].item()) == 0


def test_populations_at_the_chunk_boundaries_on_the_move(die, generic):
    """The same populations spread over their whole tiles, so that they exchange agents while they stand at the boundaries."""
    groups = []
    for t, n in enumerate(POPULATIONS):
        tx, ty = divmod(t, 3)
        if n:
            groups.append((n, (tx * 64 + 0.0, tx * 64 + 63.4), (ty * 64 + 0.0, ty * 64 + 63.4), ANY))
    medium, agents, dir0 = placed_world(192, 192, groups, 7)
    binned_equals_classic(die, 192, 192, (6, 6), medium, agents, dir0, expect_special=not generic)


# ------------------------------------------------------------------------------------------------ other instantiations
def test_fp32_world_of_4_by_6_tiles(die):
    """256 × 384 fp32 in 4 × 6 tiles of 64 × 64, 15 % of the cells with 20 % forced collisions."""
    rs = np.random.RandomState(8)
    N = int(256 * 384 * 0.15)
    medium, agents = random_state(256, 384, N, N, rs, collide=0.2)
    binned_equals_classic(die, 256, 384, (6, 6), medium, agents, f32(rs.uniform(-np.pi, np.pi, N)), expect_special=True)


@pytest.mark.parametrize('threads', [0, 320], ids=['specialised fp16', 'generic fp16, 320 threads'])
def test_fp16_world_of_3_by_3_tiles(die, threads):
    """96 × 384 with fp16 planes in 3 × 3 tiles of 32 × 128: the fp16 default's specialised instantiation, and a generic one with
    five waves per workgroup."""
    rs = np.random.RandomState(9)
    N = int(96 * 384 * 0.15)
    medium, agents = random_state(96, 384, N, N, rs, collide=0.2)
    medium[1:] = medium[1:].astype(np.float16).astype(np.float64)
    binned_equals_classic(die, 96, 384, (5, 7), medium, agents, f32(rs.uniform(-np.pi, np.pi, N)), f16=True, threads=threads,
                          expect_special=threads == 0)


# ------------------------------------------------------------------------------------------------ die_wave_sum_i64_dpp on its own
def wave_sum_rows():
    rows, L = [], 64
    one = lambda lanes, v: np.array([v if i in lanes else 0 for i in range(L)], dtype=np.int64)
    rows.append(one({0}, 0x0123456789ABCDEF))
    rows.append(one({63}, -0x0123456789ABCDEF))
    for lane in (15, 16, 31, 32, 47, 48):                                  # row and half boundaries, each alone …
        rows.append(one({lane}, (lane + 1) << 33 | 0xFFFFFFFF))
    rows.append(np.array([(i + 1) << 40 if i in (15, 16, 31, 32, 47, 48) else 0 for i in range(L)], dtype=np.int64))     # … and together
    rows.append(np.array([(1 << 62) if i % 2 == 0 else -(1 << 62) for i in range(L)], dtype=np.int64))
    rows.append(np.array([-(1 << 62) if i % 2 == 0 else (1 << 62) for i in range(L)], dtype=np.int64))
    rows.append(np.full(L, 0xFFFFFFFF, dtype=np.int64))                    # every addition of low halves carries
    rows.append(np.array([0xFFFFFFFF - i for i in range(L)], dtype=np.int64))
    rows.append(np.array([(i << 32) | (0x80000000 + i) for i in range(L)], dtype=np.int64))
    rows.append(np.full(L, -1, dtype=np.int64))
    rows.append(np.arange(L, dtype=np.int64))                               # which lane went where: weights that tell lanes apart
    rows.append((np.int64(1) << np.arange(L, dtype=np.int64) % 63).astype(np.int64))
    rs = np.random.RandomState(10)
    for _ in range(12):                                                      # full-range values: the sum wraps modulo 2^64, as numpy's does
        rows.append(rs.randint(-2 ** 63, 2 ** 63 - 1, L, dtype=np.int64))
    return np.stack(rows)


def test_wave_sum_i64_dpp(die):
    """die_wave_sum_i64_check: one wave per row of 64 values, the total against numpy's int64 sum, exactly.  29 waves: more than one
    workgroup of four, the last one partly filled."""
    from die_amd import _lib
    rows = wave_sum_rows()
    with np.errstate(over='ignore'):
        want = rows.sum(axis=1, dtype=np.int64)
    dev = torch.device('cuda:0')
    src = torch.from_numpy(rows).to(dev).contiguous()
    out = torch.full((rows.shape[0],), 0x5A5A5A5A, dtype=torch.int64, device=dev)
    _lib.check(_lib.lib.die_wave_sum_i64_check(src.data_ptr(), rows.shape[0], out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
               'die_wave_sum_i64_check')
    torch.cuda.synchronize(dev)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.nonzero(got != want)[0]
    assert _lib.lib.die_wave_sum_i64_check(None, 1, out.data_ptr(), None) != 0 and _lib.lib.die_wave_sum_i64_check(src.data_ptr(), 0, out.data_ptr(), None) != 0
