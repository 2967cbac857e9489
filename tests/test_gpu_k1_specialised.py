"""The agent kernel's specialised instantiations (die_amd/csrc/die_pic.hip `PicK1Cfg`, include/die_hip.h `die_pic_k1_generic`): tile
shape, margins, workgroup size, boundary, cost operator and rim as compile-time constants.  A call that matches one takes it, every
other call the generic instantiation; DIE_PIC_K1_GENERIC=1 (read when the step's state is created) forces the generic one.  Only how
constants reach the instructions differs, so every case below runs twice — with the switch and without — and compares bit for bit.

A 10.2-cell probe and a 1.53-cell step (in cells of the world's longer axis) give the chem margin 12 (fp16: 16, whole 8-element
vectors) and the food margin 3 the specialised instantiations are compiled for.  `die_pic_k1_specialised_launches` counts the launches
that took one.

What is compared.  WHERE an agent lands inside its tile's segment is decided by the order in which the waves of a workgroup reach an
LDS counter, in either instantiation, so raw array order is no property of a step: the two layouts' live segments are compared
part by part — per tile the stayers, then the leavers (the per-tile words off / n / s / inc themselves are compared as they are) —
with the agents of one part in slot-id order: x, y, agent_food, slot, both heading halves, and the deposit array.  Planes, result words
and the action are compared as they are (the action in slot-id order, as `to_numpy` hands it out)."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests.test_gpu_parity import f32, q32, random_state                     # noqa: E402


@pytest.fixture(scope='module')
def die():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import die_amd
    return die_amd


def canonical(meta, tensors, dep=None):
    """The arrays of a layout (`meta`: its per-tile words off, n, s) with every tile's stayers and leavers each in slot-id order."""
    off, n, s = (meta[i].to(torch.int64) for i in range(3))
    N = int(tensors[0].numel())
    assert int(n.sum().item()) == N and bool((s <= n).all()), 'segments do not cover the arrays'
    # part p = 2·tile (stayers) / 2·tile + 1 (leavers) of every array index
    bounds = torch.stack([off, off + s], dim=1).reshape(-1)
    order = torch.argsort(bounds, stable=True)
    part = order[torch.searchsorted(bounds[order], torch.arange(N, device=bounds.device), right=True) - 1]
    slot = tensors[3].to(torch.int64) & 0xFFFFFFFF
    perm = torch.argsort(part * (1 << 32) + slot)
    out = [t[perm] for t in tensors[:6]] + [part[perm]]
    if dep is not None:
        out.append(dep[perm])
    return out


def run(die, monkeypatch, generic, W, H, tile, medium, agents, dir0, steps, f16=False, boundary='wrap', lazy=True, seed=5):
    """`steps` steps of a fresh Env; what the run leaves, and how many launches took a specialised instantiation."""
    from die_amd import _lib
    monkeypatch.setenv('DIE_PIC_K1_GENERIC', '1' if generic else '0')
    N = agents.shape[1]
    env = die.Env.from_numpy(medium, agents, die.Dynamics(boundary=die.BoundaryCondition(boundary)), sort_every=0, pic=True,
                             field_dtype=torch.float16 if f16 else torch.float32)
    env._pic_tile = tile
    env._pic_lazy_actions = lazy
    ag = die.PhysarumAgent(max_agents=N, seed=seed, scale=1.53 / (max(W, H) - 1), sense_offset=10.2 / (max(W, H) - 1))
    ag.set_state(dir0)
    obs = env._get_current_obs
    before = int(_lib.lib.die_pic_k1_specialised_launches())
    words, prev, act = [], None, None
    for i in range(steps):
        if i == steps - 1 and env._pic is not None:
            # the layout the last step reads: its arrays stay as they are (its per-tile words become the next step's sizes)
            prev = (env._pic.meta[env._pic.cur].clone(), env._pic.held)
        act = ag.forward(obs)
        obs, rew, _, _, info = env.step(act)
        words.append((rew, info['num_agents']))
    pic = env._pic
    assert pic is not None and pic.held[0] is env.agents.x and pic.two_launch(env, ag), 'the two-launch tile-binned step did not run'
    assert (pic.xs, pic.ys) == tuple(tile)
    special = int(_lib.lib.die_pic_k1_specialised_launches()) - before
    action = act.to_numpy()                                      # (lazy: re-derived from what the last step left behind)
    env.check()
    assert int(pic.error[0].item()) == 0, 'error word'
    out = dict(chem=env.medium.chem.clone(), food=env.medium.food.clone(), words=torch.tensor(np.array(words, dtype=np.float64)),
               action=torch.from_numpy(np.ascontiguousarray(action)), meta_out=pic.meta[pic.cur].clone(), rim_cnt=pic.rim_cnt.clone())
    if prev is not None:                                         # (a run of one step bins inside that step)
        out['meta_in'] = prev[0]
        for k, v in enumerate(canonical(prev[0], prev[1])):
            out[f'in_{k}'] = v
    for k, v in enumerate(canonical(pic.meta[pic.cur], pic.held, pic.dep)):
        out[f'out_{k}'] = v
    return out, special, info['num_agents']


def both(die, monkeypatch, steps, **kw):
    spec, n_spec, alive = run(die, monkeypatch, False, steps=steps, **kw)
    gen, n_gen, _ = run(die, monkeypatch, True, steps=steps, **kw)
    assert n_spec == steps, f'{n_spec} of {steps} launches took the specialised instantiation'
    assert n_gen == 0, 'DIE_PIC_K1_GENERIC=1: a specialised instantiation was launched'
    assert spec.keys() == gen.keys()
    for name in spec:
        assert torch.equal(spec[name], gen[name]), name
    return spec, alive


def dense(W, H, ratio, seed, f16=False):
    rs = np.random.RandomState(seed)
    N = int(W * H * ratio)
    medium, agents = random_state(W, H, N, N, rs, collide=0.2)
    if f16:
        medium[1:] = medium[1:].astype(np.float16).astype(np.float64)
    return dict(W=W, H=H, medium=medium, agents=agents, dir0=f32(rs.uniform(-np.pi, np.pi, N)))


@pytest.mark.parametrize('lazy', [True, False], ids=['action re-derived', 'action stored'])
def test_three_by_three_tiles_fp32(die, monkeypatch, lazy):
    """192 × 192 fp32 in 3 × 3 tiles of 64 × 64: every neighbour is a periodic image too.  Ratio 0.15, 35 steps.  Both instantiations
    of the pair: the action left in registers (re-derived afterwards) and stored by the kernel."""
    _, alive = both(die, monkeypatch, 35, tile=(6, 6), lazy=lazy, **dense(192, 192, 0.15, 11))
    assert alive == int(192 * 192 * 0.15)


def test_order_table_rebuilt_inside_the_run(die, monkeypatch):
    """192 × 512 fp32, 3 × 8 tiles: eight tiles per row make an order table (three per row make none), built at the first step from what
    the device says it holds of the SPECIALISED instantiation and rebuilt at step 32 of 35."""
    from die_amd import pic as P
    made = []
    init = P.PicState.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(P.PicState, '__init__', spy)
    both(die, monkeypatch, 35, tile=(6, 6), **dense(192, 512, 0.15, 12))
    assert len(made) == 2 and all(p.order is not None and p._order_ready for p in made)
    assert torch.equal(made[0].order, made[1].order)


def test_crowd_crossing_one_border(die, monkeypatch):
    """256 × 320 fp32, 4 × 5 tiles.  7 000 agents in a strip two cells wide below the border at row 64, all heading across it: more than
    1 500 arrive in one tile — a second round of the arrival list (512 per round) — and more border agents than a rim list holds."""
    W, H, N = 256, 320, 9000
    rs = np.random.RandomState(77)
    medium, agents = random_state(W, H, N, N, rs, collide=0.0)
    medium[2] = 0.                                          # no gradient: everybody turns ±30° and moves ≈ 1.3 cells ahead
    crowd = np.arange(N) < 7000
    agents[0, crowd] = q32((62.0 + 1.8 * rs.rand(crowd.sum())) / (W - 1))
    agents[1, crowd] = q32((70.0 + 50.0 * rs.rand(crowd.sum())) / (H - 1))       # within the tile columns 64..127
    dir0 = f32(np.where(crowd, 0.0, np.floor(rs.uniform(-np.pi, np.pi, N) / np.radians(30)) * np.radians(30)))
    # after ONE step: the crowd has crossed, its tile's list has overflowed
    one, _ = both(die, monkeypatch, 1, W=W, H=H, tile=(6, 6), medium=medium, agents=agents, dir0=dir0)
    rows = (one['out_0'].to(torch.int64) & 0xFFFFFFFF).double() * (W - 1) / 2.0 ** 32
    assert int((rows >= 63.5).sum().item()) - int((agents[0] * (W - 1) >= 63.5).sum()) > 1500, 'the crowd did not cross'
    from die_amd import _lib
    assert int(one['rim_cnt'].max().item()) > int(_lib.lib.die_pic_rim_cap(6, 6)), 'no rim list overflowed'
    both(die, monkeypatch, 4, W=W, H=H, tile=(6, 6), medium=medium, agents=agents, dir0=dir0)


def test_three_by_three_tiles_fp16(die, monkeypatch):
    """96 × 384 fp16 in 3 × 3 tiles of 32 × 128, 20 steps: the fp16 default's instantiation (chem margin 16)."""
    both(die, monkeypatch, 20, tile=(5, 7), f16=True, **dense(96, 384, 0.15, 13, f16=True))


def test_limit_boundary_takes_the_generic_instantiation(die, monkeypatch):
    """192 × 192 fp32 under the limit boundary: no specialised instantiation is compiled for it."""
    _, special, _ = run(die, monkeypatch, False, steps=3, tile=(6, 6), boundary='limit', **dense(192, 192, 0.15, 14))
    assert special == 0
