"""Parity of the HIP path (libdie_hip.so through die_amd's host classes) against the CPU
oracle on identical inputs.  Integer / index work (cells, ownership, alive counts,
coordinates in Q0.32) must be bit-exact; float fields and per-agent floats must agree within
the north-star tolerance of 1e-5 relative (fp32) — the exact rtol/atol is written at each
assert.  Discrete decisions that sit on a float threshold may differ for a vanishing
fraction of slots; every such slot must be *explained* by an oracle margin below 1e-4.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import cpu_ref as R          # noqa: E402
from oracle import rng as orng           # noqa: E402

RTOL = 1e-5          # north_star: "within 1e-5 relative fp32"


@pytest.fixture(scope='module')
def die():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import die_amd
    return die_amd


def q32(v):
    from die_amd.device_array import from_q32, to_q32
    return from_q32(to_q32(v))


def f32(v):
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def random_state(W, H, N, K, rs, collide=0.3, chem_scale=1.0):
    """Random medium + agents, representable exactly on the device (f32 fields, Q0.32 coords)."""
    xs, ys = np.linspace(0, 1, W), np.linspace(0, 1, H)
    chem = rs.rand(W, H) * chem_scale
    chem = R.diffuse_decay(chem, 1.0, 0.0)            # smooth, so that gradients are meaningful
    chem[: W // 4, : H // 4] = 0.                        # a flat patch: zero gradient → masked
    food = np.round(rs.rand(W, H) * 0.5 * (rs.rand(W, H) < 0.6), 3)
    medium = np.stack([np.zeros((W, H)), f32(food), f32(chem)])
    agents = np.zeros((4, N))
    agents[0] = q32(rs.rand(N) * 0.999999)
    agents[1] = q32(rs.rand(N) * 0.999999)
    nc = int(collide * N)
    if nc > 1:                                           # forced collisions: copy positions around
        src = rs.randint(0, N, nc)
        dst = rs.randint(0, N, nc)
        agents[0, dst] = agents[0, src]
        agents[1, dst] = agents[1, src]
    alive = np.zeros(N)
    alive[rs.permutation(N)[:K]] = 1.
    agents[2] = alive
    agents[3] = f32(0.1 + 0.9 * rs.rand(N)) * alive + f32(rs.randn(N) * 0.01) * (1 - alive)
    ix, iy = R.cell(agents[0], W), R.cell(agents[1], H)
    medium[0][ix[alive > 0], iy[alive > 0]] = 1.
    return medium, agents


def ref_dyn(dyn):
    return R.RefDynamics(op_action_cost=R.zero_cost if dyn.op_action_cost.__name__ == 'zero_cost' else R.linear_action_cost,
                         rate_feed=dyn.rate_feed, rate_decay_chem=dyn.rate_decay_chem, boundary=dyn.boundary.value,
                         diffuse_sigma=dyn.diffuse_sigma, food_infinite=dyn.food_infinite, agents_die=dyn.agents_die,
                         diffuse_mode=dyn.diffuse_mode)


# ------------------------------------------------------------------------------------ diffusion
@pytest.mark.parametrize('W,H', [(6, 6), (2, 2), (5, 3), (37, 23), (256, 256), (300, 520), (16, 1024), (1030, 17)])
@pytest.mark.parametrize('sigma', [0.5, 0.8, 1.5])
def test_diffuse_decay_parity(die, W, H, sigma):
    from die_amd import _lib
    from die_amd.device_array import _ptr
    rs = np.random.RandomState(W * 1000 + H)
    chem = f32(rs.rand(W, H) * (rs.rand(W, H) < 0.5))
    src = torch.from_numpy(chem.astype(np.float32)).cuda()
    dst = torch.empty_like(src)
    _lib.check(_lib.lib.die_diffuse_decay(_ptr(src), _ptr(dst), W, H, _lib.DIE_F32, sigma, 0.1, None), 'diffuse')
    want = R.diffuse_decay(chem, float(np.float32(sigma)), float(np.float32(0.1)))
    got = dst.cpu().numpy().astype(np.float64)
    assert np.allclose(got, want, rtol=RTOL, atol=1e-7)
    # mass conservation on the torus: sum(out) = (1 − decay)·sum(in)
    assert np.isclose(got.sum(), 0.9 * chem.sum(), rtol=1e-5)


@pytest.mark.parametrize('mode', ['nearest', 'reflect', 'mirror', 'constant', 'wrap'])
@pytest.mark.parametrize('W,H', [(5, 3), (37, 24), (130, 260), (9, 2), (64, 64)])
def test_diffuse_boundary_modes(die, mode, W, H):
    """Dynamics.diffuse_mode (core/env.py:49,142): every scipy boundary mode skimage passes through, radius up to 6
    (wider than the small fields: the reflections repeat), alone and inside an env step."""
    from die_amd import _lib
    from die_amd.device_array import _ptr
    rs = np.random.RandomState(W * 7 + H)
    for sigma in (0.5, 1.5):
        chem = f32(rs.rand(W, H) * (rs.rand(W, H) < 0.6))
        src = torch.from_numpy(chem.astype(np.float32)).cuda()
        dst = torch.empty_like(src)
        _lib.check(_lib.lib.die_diffuse_decay_mode(_ptr(src), _ptr(dst), W, H, _lib.DIE_F32, sigma, 0.1, _lib.DIFFUSE_MODES[mode], None),
                   'diffuse')
        want = R.diffuse_decay(chem, float(np.float32(sigma)), float(np.float32(0.1)), mode)
        assert np.allclose(dst.cpu().numpy().astype(np.float64), want, rtol=RTOL, atol=1e-7), (mode, sigma)
    N, K = 60, 40
    medium, agents = random_state(W, H, N, K, rs)
    dyn = die.Dynamics(diffuse_mode=mode)
    rdyn = R.RefDynamics(diffuse_mode=mode, rate_feed=float(np.float32(0.1)), rate_decay_chem=float(np.float32(0.1)))
    env, ref = die.Env.from_numpy(medium, agents, dyn), R.RefEnv(medium, agents, rdyn)
    for _ in range(2):
        action = quantised_action(N, rs, 1.0 / max(W, 4))
        env.step(action)
        ref.step(action)
    m = env.medium.to_numpy()
    assert np.allclose(m[2], ref.medium[2], rtol=RTOL, atol=1e-7) and np.allclose(m[1], ref.medium[1], rtol=RTOL, atol=1e-7)
    assert np.array_equal(m[0], ref.medium[0])


def test_diffuse_impulse_kat(die):
    """Impulse at the torus corner = wrapped outer product of the 5 taps (SURVEY §8c KAT)."""
    from die_amd import _lib
    from die_amd.device_array import _ptr
    src = torch.zeros((6, 6), device='cuda')
    src[0, 0] = 1.0
    dst = torch.empty_like(src)
    _lib.check(_lib.lib.die_diffuse_decay(_ptr(src), _ptr(dst), 6, 6, 0, 0.5, 0.1, None), 'diffuse')
    w = R.gaussian_weights(0.5)
    k = np.zeros(6)
    for i, o in enumerate(range(-2, 3)):
        k[o % 6] += w[i]
    assert np.allclose(dst.cpu().numpy(), 0.9 * np.outer(k, k), rtol=RTOL, atol=1e-9)


def test_diffuse_f16_fields(die):
    from die_amd import _lib
    from die_amd.device_array import _ptr
    rs = np.random.RandomState(2)
    chem = rs.rand(64, 96).astype(np.float16)
    src = torch.from_numpy(chem).cuda()
    dst = torch.empty_like(src)
    _lib.check(_lib.lib.die_diffuse_decay(_ptr(src), _ptr(dst), 64, 96, _lib.DIE_F16, 0.5, 0.1, None), 'diffuse')
    want = R.diffuse_decay(chem.astype(np.float64), 0.5, float(np.float32(0.1)))
    # f16 storage: half a unit in the 11-bit significand
    assert np.allclose(dst.cpu().numpy().astype(np.float64), want, rtol=1e-3, atol=1e-4)


# ------------------------------------------------------------------------------------ forward
def physarum_margins(agent_ref, agents, medium, dir0, W, H):
    """Distance of every slot from each float threshold of the forward pass (oracle, f64)."""
    off = np.stack(R.polar2xy(agent_ref._sense_offset_scale, dir0))
    fx = (agents[0] + off[0]) * (W - 1) + 0.5
    fy = (agents[1] + off[1]) * (H - 1) + 0.5
    m_cell = np.minimum(np.abs(fx - np.round(fx)), np.abs(fy - np.round(fy)))
    grad = np.stack(np.gradient(medium[R.M_CHEM]))
    px, py = R.cell(agents[0] + off[0], W), R.cell(agents[1] + off[1], H)
    g = grad[:, px, py]
    norm = np.hypot(g[0], g[1])
    m_clip = np.abs(norm - agent_ref._grad_clip) / max(agent_ref._grad_clip, 1e-30)
    drads = np.arctan2(g[1], g[0]) * (norm >= agent_ref._grad_clip)
    delta = R.renormalize_radians(dir0 - drads)
    atol = agent_ref._turn_radians * agent_ref._rtol
    m_turn = np.abs(np.abs(delta) - atol / 0.99)
    m_sense = np.abs(np.abs(delta) - agent_ref._sense_radians)
    m_pi = np.abs(np.abs(dir0 - drads) - np.pi)
    m_zero = np.where(norm >= agent_ref._grad_clip, np.abs(drads), 1.0)      # |drads| ≈ 0 with a live gradient
    return np.minimum.reduce([m_cell, m_clip, m_turn, m_sense, m_pi, m_zero])


def gradient_margins(agent_ref, agents, medium, dir0, W, H):
    """The same for a GradientAgent (core/agent/gradient.py:96-124): the probe's cell rounding and the gradient clip are its only
    float thresholds."""
    off = np.stack(R.polar2xy(agent_ref._sense_offset_scale, dir0))
    fx = (agents[0] + off[0]) * (W - 1) + 0.5
    fy = (agents[1] + off[1]) * (H - 1) + 0.5
    m_cell = np.minimum(np.abs(fx - np.round(fx)), np.abs(fy - np.round(fy)))
    grad = np.stack(np.gradient(medium[R.M_CHEM]))
    g = grad[:, R.cell(agents[0] + off[0], W), R.cell(agents[1] + off[1], H)]
    m_clip = np.abs(np.hypot(g[0], g[1]) - agent_ref._grad_clip) / max(agent_ref._grad_clip, 1e-30)
    return np.minimum(m_cell, m_clip)


def assert_forward_mismatches_explained(bad, margins, N, what=''):
    """The rule of test_physarum_forward_parity, for every test that compares a device forward with the oracle's: at most 1e-4 of
    the slots (3 in small worlds) may disagree, and each of them must sit within 1e-4 of one of the forward's float thresholds
    (core/agent/gradient.py:168-193: the decisions the reference takes in float64 on values the device holds in float32)."""
    bad = np.asarray(bad)
    assert (margins[bad] < 1e-4).all(), f'{what}unexplained forward mismatches: slots {np.nonzero(bad)[0][:20]}, margins {margins[bad][:20]}'
    assert bad.sum() <= max(3, 1e-4 * N), f'{what}forward differs for {bad.sum()} of {N} slots'


@pytest.mark.parametrize('W,H,N', [(16, 12, 50), (64, 64, 3000), (200, 333, 40000), (2, 2, 7), (1024, 1024, 200000)])
@pytest.mark.parametrize('cfg', ['default', 'wide'])
def test_physarum_forward_parity(die, W, H, N, cfg):
    rs = np.random.RandomState(W + H + N)
    medium, agents = random_state(W, H, N, K=int(0.8 * N), rs=rs)
    kw = dict(scale=1.53 / (W - 1), sense_offset=min(0.3, 10.2 / (W - 1)), turn_angle=30, sense_angle=90,
              turn_tolerance=0.1) if cfg == 'default' else \
        dict(scale=0.0075, sense_offset=0.03, turn_angle=35, sense_angle=120, turn_tolerance=0.05, deposit=4.5)
    turn = np.radians(kw['turn_angle'])
    dir0 = f32(np.floor(rs.uniform(-np.pi, np.pi, N) / turn) * turn)
    sign = rs.randint(0, 2, N) * 2.0 - 1.0

    ref = R.RefPhysarumAgent(N, init_noise=np.ones((2, N)), **kw)
    ref._direction_rads = dir0.copy()
    want = ref.forward((agents, medium), turn_sign=sign)
    margins = physarum_margins(ref, agents, medium, dir0, W, H)

    env = die.Env.from_numpy(medium, agents)
    dev = die.PhysarumAgent(max_agents=N, **kw)
    dev.set_state(dir0)
    dev.set_turn_signs(sign)
    got = dev.forward(env._get_current_obs).to_numpy()
    got_dir = dev.direction_rads_numpy()

    # a slot disagrees if its heading differs (mod 2π) or its action is out of tolerance
    ddir = np.abs(R.renormalize_radians(got_dir - ref._direction_rads))
    atol = 4e-7 * kw['scale']                   # cos/sin near a zero crossing: f32 angle rounding × scale
    ok = (ddir < 1e-5) & np.isclose(got[0], want[0], rtol=RTOL, atol=atol) & \
        np.isclose(got[1], want[1], rtol=RTOL, atol=atol) & np.isclose(got[2], want[2], rtol=RTOL, atol=1e-9)
    bad = ~ok
    assert (margins[bad] < 1e-4).all(), f'unexplained mismatches: slots {np.nonzero(bad)[0]}, margins {margins[bad]}'
    assert bad.sum() <= max(3, 1e-4 * N), f'{bad.sum()} of {N} slots differ'


@pytest.mark.parametrize('normalized', [True, False])
@pytest.mark.parametrize('kind', ['physarum', 'gradient'])
def test_sub_threshold_gradients_keep_their_sign(die, kind, normalized):
    """`grad *= (norm >= grad_clip)` (core/agent/gradient.py:64-66) leaves SIGNED zeros, and
    np.angle(∓0 ∓0j) is 0 / −0 / π / −π by quadrant: in the reference a faint gradient with gx < 0 is
    not "undetermined" (found by tests/fuzz_cases.py fuzz_forward).  Field: tiny smooth chem (|grad| ≪ clip)
    next to a live region and exactly flat patches."""
    W, H, N = 64, 48, 6000
    rs = np.random.RandomState(12)
    medium, agents = random_state(W, H, N, N, rs)
    medium[2][:, : H // 2] *= 1e-6                       # sub-threshold but non-zero gradients, all quadrants
    medium[2] = f32(medium[2])
    kw = dict(scale=0.01, sense_offset=0.03, normalized_grad=normalized, grad_clip=1e-5)
    if kind == 'physarum':
        kw.update(sense_angle=100)                     # 90° on the 30° lattice is an exact tie against drads = ±π
        ref, dev = R.RefPhysarumAgent(N, seed=1, **kw), die.PhysarumAgent(max_agents=N, seed=1, **kw)
    else:
        kw.update(inertia=0.0, noise_scale=0.0)
        ref, dev = R.RefGradientAgent(N, seed=1, **kw), die.GradientAgent(max_agents=N, seed=1, **kw)
    dir0 = f32(ref._direction_rads)
    ref._direction_rads = dir0.copy()
    want = ref.forward((agents, medium))
    env = die.Env.from_numpy(medium, agents)
    dev.set_state(dir0)
    got = dev.forward(env._get_current_obs).to_numpy()
    bad = ~(np.isclose(got, want, rtol=RTOL, atol=1e-6 * kw['scale'] + 1e-9).all(axis=0))
    ddir = np.abs(R.renormalize_radians(dev.direction_rads_numpy() - ref._direction_rads))
    bad |= np.minimum(ddir, 2 * np.pi - ddir) > 1e-5
    assert bad.mean() <= 1e-3, f'{bad.sum()} of {N} slots differ'
    # the quirk itself is present in the sample: masked gradients that are not "undetermined"
    if kind == 'physarum':
        g = np.stack(np.gradient(medium[2]))
        off = np.stack(R.polar2xy(kw['sense_offset'], dir0))
        gg = g[:, R.cell(agents[0] + off[0], W), R.cell(agents[1] + off[1], H)]
        faint = np.hypot(gg[0], gg[1]) < 1e-5
        both_neg = faint & (gg[0] < 0) & (gg[1] < 0)        # angle(−0 −0j) = π: a "real" direction
        mixed = faint & (gg[0] < 0) & (gg[1] > 0)            # angle(−0 +0j) = 0: undetermined
        assert both_neg.sum() > 50 and mixed.sum() > 50
        assert ref._deposit_mask[both_neg].mean() > 0.7 and ref._deposit_mask[mixed].mean() == 0


def test_physarum_forward_with_reference_made_vectors(die, golden_dir):
    """The turn logic on device vs outputs of the reference's own _discrete_turn
    (tests/golden/ref_helpers.npz, case 0 = default parameters): build a chem field whose
    gradient at each agent's probe cell is the golden sampled gradient."""
    import os
    G = np.load(os.path.join(golden_dir, 'ref_helpers.npz'))
    g_in, dir0, rand01 = G['turn0_grad_in'], G['turn0_dir0'], G['turn0_rand01']
    want_g, want_mask = G['turn0_grad_out'], G['turn0_deposit_mask']
    n = 1000                                    # includes the zero-gradient, +x and threshold cases
    sel = np.r_[0:200, 400:450, 500:1100, 2000:2150][:n]
    n = len(sel)
    # one agent per 3x3 block of a (3n)x3 field, chem = linear ramp a·x + b·y inside the block
    W, H = 3 * n, 3
    chem = np.zeros((W, H))
    for k, s in enumerate(sel):
        gx, gy = g_in[:, s]
        for i in range(3):
            for j in range(3):
                chem[3 * k + i, j] = 1.0 + 0.25 * (gx * (i - 1) + gy * (j - 1))
    agents = np.zeros((4, n))
    agents[0] = q32((3 * np.arange(n) + 1) / (W - 1))
    agents[1] = q32(np.full(n, 0.5))
    agents[2] = 1
    medium = np.stack([np.zeros((W, H)), np.full((W, H), 0.25), f32(chem)])
    env = die.Env.from_numpy(medium, agents)
    dev = die.PhysarumAgent(max_agents=n, scale=1.0, sense_offset=0.0)
    dev.set_state(f32(dir0[sel]))
    dev.set_turn_signs((rand01[sel] - 0.5) * 2)
    got = dev.forward(env._get_current_obs).to_numpy()
    # the field stores the ramp in f32, so sampled directions carry ~1e-7 noise: compare away from thresholds
    atol_t = np.radians(30) * 0.1
    drads = np.arctan2(g_in[1, sel], g_in[0, sel])
    delta = R.renormalize_radians(dir0[sel] - drads)
    safe = (np.abs(np.abs(delta) - atol_t / 0.99) > 1e-5) & (np.abs(np.abs(delta) - np.pi / 2) > 1e-5) & \
           ((np.abs(drads) > 1e-5) | (np.hypot(g_in[0, sel], g_in[1, sel]) == 0) | (g_in[1, sel] == 0))
    assert safe.mean() > 0.6
    assert np.allclose(got[0][safe], want_g[0, sel][safe], rtol=RTOL, atol=2e-6)
    assert np.allclose(got[1][safe], want_g[1, sel][safe], rtol=RTOL, atol=2e-6)
    want_dep = 4.0 * 0.25 * np.clip(want_mask[sel], 0.1, 1.0)
    assert np.allclose(got[2][safe], want_dep[safe], rtol=RTOL)


@pytest.mark.parametrize('inertia,noise', [(0.9, 0.025), (0.0, 0.05), (0.95, 0.0)])
def test_gradient_agent_forward_parity(die, inertia, noise):
    W, H, N = 96, 80, 5000
    rs = np.random.RandomState(11)
    medium, agents = random_state(W, H, N, K=N, rs=rs)
    prev = f32(rs.normal(0, .4, (2, N)))
    kw = dict(scale=0.01, deposit=4.5, inertia=inertia, sense_offset=0.03, noise_scale=noise)
    ref = R.RefGradientAgent(N, init_noise=prev, seed=77, **kw)
    ref._direction_rads = f32(ref._direction_rads)
    dir0 = ref._direction_rads.copy()
    want = ref.forward((agents, medium))
    env = die.Env.from_numpy(medium, agents)
    dev = die.GradientAgent(max_agents=N, seed=77, **kw)
    dev.set_state(dir0, prev)
    got = dev.forward(env._get_current_obs).to_numpy()
    # Box–Muller in f32 on device vs f64 in the oracle: absolute 1e-6 on O(1) normals × noise_scale
    assert np.mean(~np.isclose(got[:2], want[:2], rtol=RTOL, atol=2e-8 + 2e-6 * noise * 0.01)) < 2e-3
    assert np.allclose(got[2], want[2], rtol=RTOL, atol=1e-9)
    if inertia:
        assert np.mean(~np.isclose(dev.prev_grad_numpy(), ref._prev_grad, rtol=RTOL, atol=2e-6)) < 2e-3


def test_brownian_and_const_forward_parity(die):
    N = 10000
    rs = np.random.RandomState(5)
    medium, agents = random_state(32, 32, N, K=6000, rs=rs)
    env = die.Env.from_numpy(medium, agents)
    b = die.BrownianAgent(move_scale=0.01, deposit_scale=0.5, seed=99)
    rb = R.RefBrownianAgent(move_scale=0.01, deposit_scale=0.5, seed=99)
    for _ in range(3):                          # the step counter advances the stream
        got = b.forward(env._get_current_obs).to_numpy()
        want = rb.forward((agents, medium))
        assert np.allclose(got, want, rtol=1e-6, atol=1e-9)
        assert (got[:, agents[2] == 0] == 0).all()
    c = die.ConstAgent(delta_xy=(-0.01, 0.005), deposit=0.1).forward(env._get_current_obs).to_numpy()
    assert np.allclose(c, R.RefConstAgent((-0.01, 0.005), 0.1).forward((agents, medium)), rtol=1e-7)


# ------------------------------------------------------------------------------------ env.step
def quantised_action(N, rs, scale):
    """Random action whose displacements are exactly representable in Q0.32 AND f32."""
    dx = np.rint(f32(rs.uniform(-scale, scale, N)) * 2 ** 32) / 2 ** 32
    dy = np.rint(f32(rs.uniform(-scale, scale, N)) * 2 ** 32) / 2 ** 32
    dx, dy = f32(dx), f32(dy)
    assert np.array_equal(np.rint(dx * 2 ** 32) / 2 ** 32, dx)
    return np.stack([dx, dy, f32(rs.rand(N) * 2.0)])


STEP_CASES = [
    dict(W=16, H=12, N=60, K=40),
    dict(W=64, H=64, N=4096, K=600),                         # reference layout: N = W·H, mostly dead slots
    dict(W=200, H=333, N=30000, K=30000),                    # compact: no dead slots
    dict(W=2, H=2, N=9, K=5),
    dict(W=128, H=128, N=5000, K=0),                         # nobody alive
    dict(W=64, H=64, N=2000, K=1500, boundary='limit'),
    dict(W=64, H=64, N=2000, K=1500, food_infinite=True),
    dict(W=64, H=64, N=2000, K=1500, agents_die=True),
    dict(W=64, H=64, N=2000, K=1500, zero_cost=True),
    dict(W=96, H=40, N=3000, K=2500, sigma=0.8, rate_feed=0.3, decay=0.05),
    dict(W=1024, H=1024, N=157286, K=157286),
]


@pytest.mark.parametrize('case', STEP_CASES, ids=lambda c: '-'.join(f'{k}{v}' for k, v in c.items()))
def test_env_step_parity(die, case):
    W, H, N, K = case['W'], case['H'], case['N'], case['K']
    rs = np.random.RandomState(W * 7 + N)
    medium, agents = random_state(W, H, N, K, rs)
    if case.get('agents_die'):
        agents[3, ::3] = 1e-5 * agents[2, ::3]              # some agents starve this step
    dyn = die.Dynamics(boundary=die.BoundaryCondition(case.get('boundary', 'wrap')),
                       food_infinite=case.get('food_infinite', False), agents_die=case.get('agents_die', False),
                       op_action_cost=die.zero_cost if case.get('zero_cost') else die.linear_action_cost,
                       diffuse_sigma=case.get('sigma', 0.5), rate_feed=case.get('rate_feed', 0.1),
                       rate_decay_chem=case.get('decay', 0.1))
    scale = 3.0 / W if case.get('boundary') != 'limit' else 0.6      # 'limit': many agents hit the walls
    action = quantised_action(N, rs, scale)

    rd = ref_dyn(dyn)
    for f in ('rate_feed', 'rate_decay_chem', 'diffuse_sigma'):       # the C struct carries them as f32
        setattr(rd, f, float(np.float32(getattr(rd, f))))
    ref = R.RefEnv(medium, agents, rd)
    _, want_reward, want_term, _, want_info = ref.step(action)

    env = die.Env.from_numpy(medium, agents, dyn)
    obs, reward, term, trunc, info = env.step(die.DeviceAction.from_numpy(action, env.device))
    got_agents = env.agents.to_numpy()
    got_medium = env.medium.to_numpy()

    # integer / index work: bit-exact
    if case.get('boundary') == 'limit':                     # 1.0 is stored as 1 − 2^-32
        assert np.abs(got_agents[:2] - ref.agents[:2]).max() <= 2.0 ** -32
    else:
        assert np.array_equal(got_agents[:2], ref.agents[:2])
    assert np.array_equal(got_agents[2], ref.agents[2])
    assert np.array_equal(got_medium[0], ref.medium[0])
    assert info['num_agents'] == want_info['num_agents'] and term == want_term and trunc is False
    # ownership: the highest alive slot standing on each occupied cell
    alive = agents[2] > 0
    ix, iy = R.cell(ref.agents[0], W), R.cell(ref.agents[1], H)
    if not case.get('agents_die'):
        want_owner = np.full((W, H), -1, dtype=np.int64)
        idx = np.nonzero(alive)[0]
        want_owner[ix[idx], iy[idx]] = idx                  # ascending order: the last (highest) write stays
        assert np.array_equal(env.medium.owner_slots().cpu().numpy(), want_owner)
    # floats: 1e-5 relative
    assert np.allclose(got_agents[3], ref.agents[3], rtol=RTOL, atol=1e-7)
    assert np.allclose(got_medium[1], ref.medium[1], rtol=RTOL, atol=1e-8)
    assert np.allclose(got_medium[2], ref.medium[2], rtol=RTOL, atol=1e-7)
    assert abs(reward - want_reward) <= RTOL * np.abs(ref.last_gained).sum() + 1e-9
    assert obs[0] is env.agents and obs[1] is env.medium


@pytest.mark.parametrize('W,H,N,K', [(64, 64, 3000, 2000), (96, 40, 4000, 4000), (37, 24, 500, 300)])
def test_fused_step_equals_staged_step(die, W, H, N, K):
    """die_env_step's fused field sweep (deposit + feeding + diffusion in one pass) against the
    stage-by-stage entry points on the same inputs: identical bits."""
    rs = np.random.RandomState(W + N)
    medium, agents = random_state(W, H, N, K, rs)
    action = quantised_action(N, rs, 3.0 / W)
    outs = []
    for mode in ('step', 'staged', 'sweep'):
        env = die.Env.from_numpy(medium, agents, sort_every=0)
        if mode == 'step':
            env.step(action)
        else:
            act = die.DeviceAction.from_numpy(action, env.device)
            env.medium.next_epoch()
            env._stage('die_agent_move_claim', act)
            env._stage('die_agent_resolve', act)
            if mode == 'staged':
                env._medium_diffuse_decay()
            else:                                   # resolve already applied deposits: undo by a fresh env
                env = die.Env.from_numpy(medium, agents, sort_every=0)
                env.medium.next_epoch()
                env._stage('die_agent_move_claim', act)
                env._medium_deposit_feed_diffuse()
        outs.append((env.medium.to_numpy(), env.agents.to_numpy()))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][0], outs[2][0])
    assert np.array_equal(outs[0][1][:3], outs[1][1][:3])
    if K == N:                                      # with dead slots the sweep-only variant skips their feed pass
        assert np.array_equal(outs[0][1], outs[2][1])
    assert np.array_equal(outs[0][1], outs[1][1])


def test_staged_path_gives_identical_results(die):
    """die_env_step with die_dynamics.staged = 1 (one kernel per stage: move/claim, resolve, reduce, diffuse) must
    reproduce the bits of the default path (claims + fused field sweep)."""
    W, H, N, K = 96, 64, 6000, 5000
    rs = np.random.RandomState(31)
    medium, agents = random_state(W, H, N, K, rs, collide=0.5)      # many shared cells
    action = quantised_action(N, rs, 3.0 / W)
    outs = []
    for staged in (False, True):
        env = die.Env.from_numpy(medium, agents, sort_every=0, staged=staged)
        for _ in range(3):
            env.step(action)
        outs.append((env.medium.to_numpy(), env.agents.to_numpy(), env.medium.owner_slots().cpu().numpy()))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('form', ['two launches', 'three launches'])
@pytest.mark.parametrize('W,H,boundary,f16,tile', [(128, 96, 'wrap', False, (4, 5)), (192, 256, 'limit', False, (6, 6)),
                                                   (256, 192, 'wrap', True, (5, 6)), (96, 384, 'wrap', False, (5, 7))])
def test_tile_binned_step_equals_classic_step(die, W, H, boundary, f16, tile, form):
    """The tile-binned fast path (die_pic_forward_env_step: agents in exact tile order, claims resolved in LDS, deposit
    plane instead of the claim plane) against the classic fused step: every output bit for bit — fields, ownership,
    agents, headings, the actions handed back, rewards — with collisions, every compiled tile shape, a mid-run switch
    between the paths and a re-bin after the arrays were re-ordered behind its back."""
    N = K = 9000
    rs = np.random.RandomState(W + H)
    medium, agents = random_state(W, H, N, K, rs, collide=0.4)
    turn = np.radians(30)
    dir0 = f32(np.floor(rs.uniform(-np.pi, np.pi, N) / turn) * turn)
    outs = []
    for pic in (True, False):
        env = die.Env.from_numpy(medium, agents, die.Dynamics(boundary=die.BoundaryCondition(boundary)), sort_every=3, pic=pic,
                                 field_dtype=torch.float16 if f16 else torch.float32)
        env._pic_tile = tile if pic else None
        # the two forms of the binned step (die_pic.rim): one field kernel per tile, or K2 + deposit plane + sweep
        env._pic_fused = form != 'three launches'
        ag = die.PhysarumAgent(max_agents=N, seed=5, scale=1.53 / (max(W, H) - 1), sense_offset=10.2 / (max(W, H) - 1))
        ag.set_state(dir0)
        obs = env._get_current_obs
        acts, rewards = [], []
        for i in range(11):
            if i == 4:
                env._pic_enabled = False                       # classic steps in between: the arrays get re-sorted
            if i == 7:
                env._pic_enabled = pic                         # … and the binned path has to re-bin
            action = ag.forward(obs)
            obs, rew, _, _, info = env.step(action)
            acts.append(action.to_numpy())
            rewards.append((rew, info['num_agents']))
            if pic and i in (0, 3, 7, 10):
                assert env._pic is not None and env._pic.held[0] is env.agents.x, 'the tile-binned path did not run'
                assert (env._pic.xs, env._pic.ys) == tile
                assert env._pic.two_launch(env, ag) == (form != 'three launches')
        outs.append((env.medium.to_numpy(), env.agents.to_numpy(), ag.direction_rads_numpy(), env.medium.owner_slots().cpu().numpy(),
                     np.stack(acts), np.array(rewards)))
    for name, a, b in zip(('medium', 'agents', 'heading', 'owners', 'actions', 'rewards'), outs[0], outs[1]):
        assert np.array_equal(a, b), name


@pytest.mark.parametrize('W,H,tile,threads', [(128, 96, (4, 5), (64, 128, 192)), (192, 256, (6, 6), (64, 128, 320, 448))])
def test_tile_binned_step_with_other_workgroup_sizes_of_the_agent_kernel(die, W, H, tile, threads):
    """`die_pic.k1_threads` (DIE_PIC_THREADS): the agent kernel with 1, 2, 3, 5, 7 waves per workgroup instead of its default — the
    chunk loop takes more trips, and the tile's last words (arrival counts, rim codes, reward partial) leave from one, two or three
    waves (round 6: three side by side when there are that many).  Bit for bit the default size's results, dense collisions included."""
    N = 9000
    rs = np.random.RandomState(W + 7 * H)
    medium, agents = random_state(W, H, N, N, rs, collide=0.4)
    turn = np.radians(30)
    dir0 = f32(np.floor(rs.uniform(-np.pi, np.pi, N) / turn) * turn)
    outs = []
    for thr in (0,) + tuple(threads):
        env = die.Env.from_numpy(medium, agents, sort_every=0, pic=True)
        env._pic_tile = tile
        env._pic_k1_threads = thr
        ag = die.PhysarumAgent(max_agents=N, seed=5, scale=1.53 / (max(W, H) - 1), sense_offset=10.2 / (max(W, H) - 1))
        ag.set_state(dir0)
        obs = env._get_current_obs
        rewards = []
        for _ in range(4):
            obs, rew, _, _, info = env.step(ag.forward(obs))
            rewards.append((rew, info['num_agents']))
        assert env._pic is not None and env._pic.held[0] is env.agents.x and env._pic.k1_threads == thr
        outs.append((env.medium.to_numpy(), env.agents.to_numpy(), ag.direction_rads_numpy(), np.array(rewards)))
    for got in outs[1:]:
        for name, a, b in zip(('medium', 'agents', 'heading', 'rewards'), outs[0], got):
            assert np.array_equal(a, b), name


@pytest.mark.parametrize('W,H,N', [(128, 512, 30000), (1536, 2048, 440000)])
def test_order_table_of_the_two_launch_form(die, monkeypatch, W, H, N):
    """die_pic.order (round 6): which workgroup takes which tile — crowded tiles first in the last span of every XCD band, rebuilt by the
    library every 32nd step from the populations of the layout a step reads.  The table must be a permutation of every band's tiles, sorted by
    the 8-wave rounds a tile costs (descending, band order among equals), and must change no result: the same world stepped with
    DIE_PIC_ORDER=0 (band mapping) gives the same bits.  A crowd in one corner makes the classes differ."""
    tile = (4, 5)                                             # 8 x 16 tiles: two columns of tiles per XCD band; 96 x 64 tiles: bands of 768
    rs = np.random.RandomState(5)                             # tiles, of which the last 512 are sorted (k_pic_order: PIC_ORDER_SPAN)
    medium, agents = random_state(W, H, N, N, rs, collide=0.2)
    # a crowd in the LAST rows of tiles of the first XCD band: tiles of ~ 2 000 agents (four 8-wave rounds and more: what makes
    # k_pic_order sort a band's last span) beside tiles of ~ 100
    # (all eight bands sort or none: from 96 in 4 096 of the last spans' tiles crowded — 3 of the small world's 128 tiles, 96 of the large one's)
    nc, xr, yr = (16000, (0.52, 0.98), (0.005, 0.115)) if W == 128 else (330000, (0.80, 0.995), (0.001, 0.115))
    agents[0, :nc] = rs.uniform(*xr, nc)
    agents[1, :nc] = rs.uniform(*yr, nc)
    agents[:2] = q32(agents[:2])
    turn = np.radians(30)
    dir0 = f32(np.floor(rs.uniform(-np.pi, np.pi, N) / turn) * turn)
    outs = []
    for use in ('1', '0'):
        monkeypatch.setenv('DIE_PIC_ORDER', use)
        env = die.Env.from_numpy(medium, agents, sort_every=0, pic=True)
        env._pic_tile = tile
        ag = die.PhysarumAgent(max_agents=N, seed=5, scale=1.53 / (max(W, H) - 1), sense_offset=10.2 / (max(W, H) - 1))
        ag.set_state(dir0)
        obs = env._get_current_obs
        rewards = []
        order = None
        for i in range(35):                                   # (the agent's step counter passes a multiple of 32: a rebuild mid-run)
            obs, rew, _, _, info = env.step(ag.forward(obs))
            rewards.append((rew, info['num_agents']))
            if i == 0 and env._pic.order is not None:         # the table as the first step built it, from the initial populations (the crowd disperses)
                order = env._pic.order.cpu().numpy().astype(np.int64) & 0xFFFF
        pic = env._pic
        assert pic is not None and pic.held[0] is env.agents.x and pic.two_launch(env, ag)
        if use == '1':
            assert pic.order is not None and pic._order_ready and order is not None
            ntx, nty = W >> tile[0], H >> tile[1]
            wb, per = nty // 8, ntx * (nty // 8)
            for j in range(8):
                band = [(q // wb) * nty + j * wb + q % wb for q in range(per)]
                got = order[j * per:(j + 1) * per].tolist()
                assert sorted(got) == sorted(band), f'band {j}: not a permutation of its tiles'
                # only the band's last 512 tiles are sorted (what must not hold a crowded tile is a launch's tail); the tiles ahead keep the band order
                assert got[:max(per - 512, 0)] == band[:max(per - 512, 0)], f'band {j}: the tiles ahead of the last span'
                assert sorted(got[-512:]) == sorted(band[-512:]), f'band {j}: the last span'
            assert len(set(order.tolist())) == ntx * nty
            moved = [j for j in range(8) if order[j * per:(j + 1) * per].tolist() != [(q // wb) * nty + j * wb + q % wb for q in range(per)]]
            assert 0 in moved and len(moved) < 8, f'bands out of band order: {moved} (the crowded one should be, the empty ones not)'
        else:
            assert pic.order is None
        outs.append((env.medium.to_numpy(), env.agents.to_numpy(), ag.direction_rads_numpy(), np.array(rewards)))
    for name, a, b in zip(('medium', 'agents', 'heading', 'rewards'), outs[0], outs[1]):
        assert np.array_equal(a, b), name


def applied(action):
    """The action as the device applies it: displacements rounded to the Q0.32 grid of the coordinates (at most 2^-33 away
    from the float the agent computed — enough to put ≈ 1e-6 of the agents of a 4096-cell axis on the other side of a cell
    border if the oracle moved by the unrounded value)."""
    a = np.array(action, dtype=np.float64)
    a[:2] = np.rint(a[:2] * 2.0 ** 32) / 2.0 ** 32
    return a


def _binned_steps_against_the_oracle(die, medium, agents, dyn, tile, agent_kind, kw, n_steps, f16=False, form='two launches', seed=3,
                                     dir0=None, prev_grad=None, k1_threads=0, calls=0, callback=None):
    """`n_steps` × `env.step(agent.forward(obs))` on the tile-binned path, every step teacher-forced against the oracle:
    the oracle starts each step from the device's state (downloaded), computes ITS forward — compared with the action the
    device read back —, then steps with the device's action (so that a decision that sits on a float threshold cannot
    cascade) and its new state is compared with the device's: coordinates / cells / ownership / alive bit-exact, fields,
    agent_food, reward within 1e-5 relative (fp16 fields: within their 11-bit significand).

    `dir0` / `prev_grad`: the initial heading (and GradientAgent momentum) instead of the oracle agent's; `k1_threads`: the agent
    kernel's workgroup size (die_pic.k1_threads, 0: the library's); `calls`: the agents' step counter at the first step (the
    Philox draws and the order table's rebuilds follow it); `callback(step, env, agent, when)`: called with when = 'before' and
    'after' around every device step (tests/test_gpu_crowds.py reads the device's bookkeeping there)."""
    N = agents.shape[1]
    W, H = medium.shape[1:]
    env = die.Env.from_numpy(medium, agents, dyn, sort_every=0, field_dtype=torch.float16 if f16 else torch.float32)
    env._pic_tile = tile
    env._pic_fused = form != 'three launches'
    if k1_threads:
        env._pic_k1_threads = k1_threads
    rd = ref_dyn(dyn)
    for f in ('rate_feed', 'rate_decay_chem', 'diffuse_sigma'):       # the C struct carries them as f32
        setattr(rd, f, float(np.float32(getattr(rd, f))))
    if agent_kind == 'physarum':
        dev, ref = die.PhysarumAgent(max_agents=N, seed=seed, **kw), R.RefPhysarumAgent(N, seed=seed, **kw)
    else:
        dev, ref = die.GradientAgent(max_agents=N, seed=seed, **kw), R.RefGradientAgent(N, seed=seed, **kw)
    dir0 = f32(ref._direction_rads if dir0 is None else dir0)
    momentum = kw.get('inertia', 0) != 0
    dev.set_state(dir0, prev_grad=f32(ref._prev_grad if prev_grad is None else prev_grad) if momentum else None)
    dev._calls = ref._calls = calls
    frtol, fatol = (1e-3, 1e-4) if f16 else (RTOL, 1e-7)
    obs = env._get_current_obs
    for step in range(n_steps):
        if callback is not None:
            callback(step, env, dev, 'before')
        m0, a0, d0 = env.medium.to_numpy(), env.agents.to_numpy(), dev.direction_rads_numpy()
        ref._direction_rads = d0.copy()
        if momentum:
            ref._prev_grad = dev.prev_grad_numpy()
        renv = R.RefEnv(m0, a0, rd)
        want_action = ref.forward(renv.obs)
        action = dev.forward(obs)
        obs, reward, term, _, info = env.step(action)
        if momentum:                                         # _prev_grad travels with the agents through the tiles (gradient.py:89)
            bad_pg = ~np.isclose(dev.prev_grad_numpy(), ref._prev_grad, rtol=max(RTOL, frtol), atol=1e-6 + (1e-3 if f16 else 0)).all(axis=0)
            assert bad_pg.mean() < 2e-3, f'step {step}: _prev_grad differs for {bad_pg.sum()} of {N} slots'
        assert env._pic is not None and env._pic.held is not None and env._pic.held[0] is env.agents.x, 'the tile-binned step did not run'
        assert env._pic.two_launch(env, dev) == (form != 'three launches')
        if k1_threads:
            assert env._pic.k1_threads == k1_threads
        if callback is not None:
            callback(step, env, dev, 'after')
        got_action = action.to_numpy()
        # atol: sin/cos of a heading at a zero crossing carry the f32 angle rounding (~2e-7 rad) x scale
        bad = ~np.isclose(got_action, want_action, rtol=max(RTOL, frtol), atol=1e-6 * abs(kw['scale']) + (1e-3 if f16 else 0)).all(axis=0)
        if kw.get('noise_scale', 0) != 0 or momentum:
            # (momentum: the mismatching slots' _prev_grad is compared above; noise: the oracle draws the device's own Philox normals)
            assert bad.mean() < 2e-3, f'step {step}: forward differs for {bad.sum()} of {N} slots'
        else:
            # the strict rule of the stand-alone forward's test: few, and each explained by a float threshold
            margins = (physarum_margins if agent_kind == 'physarum' else gradient_margins)(ref, a0, m0, d0, W, H)
            assert_forward_mismatches_explained(bad, margins, N, f'step {step}: ')
        _, want_reward, want_term, _, want_info = renv.step(applied(got_action))
        ga, gm = env.agents.to_numpy(), env.medium.to_numpy()
        if dyn.boundary == die.BoundaryCondition.limit:     # 1.0 is stored as 1 − 2^-32
            assert np.abs(ga[:2] - renv.agents[:2]).max() <= 2.0 ** -32
        else:
            assert np.array_equal(ga[:2], renv.agents[:2]), f'step {step}: coordinates'
        assert np.array_equal(ga[2], renv.agents[2])
        assert np.array_equal(gm[0], renv.medium[0]), f'step {step}: agents channel'
        ix, iy = R.cell(renv.agents[0], W), R.cell(renv.agents[1], H)
        want_owner = np.full((W, H), -1, dtype=np.int64)
        live = np.nonzero(renv.agents[2] > 0)[0]            # (dead slots never claim a cell: core/env.py:204-215 works on the alive ones)
        want_owner[ix[live], iy[live]] = live               # ascending order: the last (highest) write stays
        assert np.array_equal(env.medium.owner_slots().cpu().numpy(), want_owner), f'step {step}: ownership'
        assert np.allclose(ga[3], renv.agents[3], rtol=frtol, atol=fatol), f'step {step}: agent_food'
        assert np.allclose(gm[1], renv.medium[1], rtol=frtol, atol=fatol), f'step {step}: food'
        assert np.allclose(gm[2], renv.medium[2], rtol=frtol, atol=fatol), f'step {step}: chem'
        assert info['num_agents'] == want_info['num_agents'] == len(live) and term == want_term
        assert abs(reward - want_reward) <= max(RTOL, frtol) * np.abs(renv.last_gained).sum() + 1e-9, f'step {step}: reward'
    return env


BINNED_ORACLE_CASES = [
    dict(W=64, H=96, tile=(4, 5)),
    # 8 and 16 tiles per row: the workgroup → tile mapping by XCD bands (die_pic.hip pic_xcd_tile) is on the path
    dict(W=48, H=256, tile=(4, 5), collide=0.5),
    dict(W=64, H=512, tile=(4, 5), boundary='limit'),
    dict(W=192, H=192, tile=(6, 6), collide=0.6),                            # forced collisions: last writer wins
    dict(W=96, H=192, tile=(5, 6), boundary='limit'),
    dict(W=96, H=384, tile=(5, 7), food_infinite=True),
    dict(W=192, H=256, tile=(6, 6), zero_cost=True, sigma=0.8, rate_feed=0.3, decay=0.05),    # gaussian radius 3
    dict(W=128, H=192, tile=(5, 6), f16=True),
    dict(W=96, H=384, tile=(5, 7), f16=True, collide=0.5),                   # what Env picks for fp16 fields (32×128 tiles)
    dict(W=128, H=192, tile=(5, 6), agent='gradient'),
    # GradientAgent with momentum (the reference's defaults: inertia .9, noise .025 — gradient.py:19-30): _prev_grad in the layouts
    dict(W=128, H=192, tile=(5, 6), agent='gradient', inertia=0.9, noise=0.025),
    dict(W=192, H=192, tile=(6, 6), agent='gradient', inertia=0.5, noise=0.0, collide=0.5),
    dict(W=64, H=96, tile=(4, 5), agent='gradient', inertia=0.0, noise=0.05, form='three launches'),
    dict(W=192, H=192, tile=(6, 6), dense=True),                             # several agents per cell
    dict(W=64, H=96, tile=(4, 5), form='three launches'),
    dict(W=192, H=192, tile=(6, 6), collide=0.6, form='three launches'),
    # dead slots (the reference's default layout: max_agents = W·H slots, core/data_init.py:143-144) behind the tiles' segments:
    # they act, move, burn and consume like the reference's, and never claim a cell
    dict(W=192, H=192, tile=(6, 6), dead=0.6, collide=0.5),
    dict(W=128, H=192, tile=(5, 6), dead=0.85, boundary='limit'),
    dict(W=64, H=96, tile=(4, 5), dead=0.3, f16=True),
]


@pytest.mark.parametrize('case', BINNED_ORACLE_CASES, ids=lambda c: '-'.join(f'{k}{v}' for k, v in c.items()))
def test_tile_binned_step_vs_oracle(die, case):
    """The benchmarked path, die_pic_forward_env_step, directly against oracle.cpu_ref (core/env.py:101-131,
    core/agent/gradient.py:96-124) — not through its equality with the classic step: all four tile shapes, wrap / limit,
    fp16 fields, a GradientAgent, forced collisions, worlds with several agents per cell, food_infinite, zero_cost, a
    wider gaussian, both forms of the step; three steps each, so that segments with leavers and arrivals (and rim records
    written by a previous step's neighbours) are on the path."""
    W, H = case['W'], case['H']
    rs = np.random.RandomState(W * 3 + H)
    N = 3 * W * H if case.get('dense') else int(0.15 * W * H)
    if case.get('dead'):
        N = int(0.5 * W * H)
    medium, agents = random_state(W, H, N, N - int(case.get('dead', 0) * N), rs, collide=case.get('collide', 0.3))
    dyn = die.Dynamics(boundary=die.BoundaryCondition(case.get('boundary', 'wrap')), food_infinite=case.get('food_infinite', False),
                       op_action_cost=die.zero_cost if case.get('zero_cost') else die.linear_action_cost,
                       diffuse_sigma=case.get('sigma', 0.5), rate_feed=case.get('rate_feed', 0.1), rate_decay_chem=case.get('decay', 0.1))
    if case.get('agent') == 'gradient':
        kw = dict(scale=0.01, sense_offset=0.03, inertia=case.get('inertia', 0.0), noise_scale=case.get('noise', 0.0), normalized_grad=True)
    else:
        kw = dict(scale=1.53 / (max(W, H) - 1), sense_offset=10.2 / (max(W, H) - 1))
    if case.get('f16'):                                     # fields the device holds exactly
        medium[1:] = medium[1:].astype(np.float16).astype(np.float64)
    _binned_steps_against_the_oracle(die, medium, agents, dyn, case['tile'], case.get('agent', 'physarum'), kw, 3, f16=case.get('f16', False),
                                     form=case.get('form', 'two launches'))


@pytest.mark.parametrize('shape,f16,want', [((2048, 2048), True, (5, 7)), ((2048, 2048), False, (6, 6)), ((2048, 2112), True, (6, 6)),
                                            ((4096, 2048 + 32), True, (4, 5))])
def test_tile_shape_the_env_picks(die, shape, f16, want):
    """fp16 field channels take 32x128 tiles where the world divides into them (a 64-cell row of an fp16 plane is one 128-byte line;
    round 6: +4.5 % at 4096^2, +8.5 % at 16384^2), fp32 planes 64x64; worlds those do not divide fall back along pic.TILE_SHAPES.
    One step, on the binned path, two launches."""
    W, H = shape
    env = die.Env((W, H), die.Dynamics(init_agent_ratio=0.05), seed=3, max_agents='alive', sync=False,
                  field_dtype=torch.float16 if f16 else torch.float32)
    ag = die.PhysarumAgent(max_agents=env.agents.N, seed=3, scale=1.53 / (max(W, H) - 1), sense_offset=10.2 / (max(W, H) - 1))
    obs, res, *_ = env.step(ag.forward(env._get_current_obs))
    assert env._pic is not None and env._pic.held is not None and (env._pic.xs, env._pic.ys) == want == tuple(env._pic_tile)
    assert env._pic.two_launch(env, ag)
    reward, n = env.read_result(res)
    assert n == env.agents.N and np.isfinite(reward)


def test_configs2_full_size_teacher_forced_step_vs_oracle(die):
    """BASELINE configs[2] at FULL size — PhysarumAgent, 4096x4096 fp32, ratio 0.15, the benchmark's parameters — on the
    benchmarked (tile-binned, two-launch) path: after four free steps (chem exists, segments hold leavers and arrivals)
    ONE teacher-forced step against the oracle: cells / ownership / alive bit-exact, fields and agent_food at 1e-5."""
    W = H = 4096
    env = die.Env((W, H), die.Dynamics(init_agent_ratio=0.15), seed=1234, max_agents='alive', sync=False)
    N = env.agents.N
    kw = dict(scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1), turn_angle=30, sense_angle=90, turn_tolerance=0.1, deposit=4.0)
    dev, ref = die.PhysarumAgent(max_agents=N, seed=1234, **kw), R.RefPhysarumAgent(N, seed=1234, **kw)
    obs = env._get_current_obs
    for _ in range(4):
        obs, *_ = env.step(dev.forward(obs))
        ref._calls += 1                                     # (the Philox step counter of the oracle's agent keeps pace)
    assert env._pic is not None and env._pic.held[0] is env.agents.x and env._pic.two_launch(env, dev)
    m0, a0 = env.medium.to_numpy(), env.agents.to_numpy()
    d0 = dev.direction_rads_numpy()
    ref._direction_rads = d0.copy()
    rd = R.RefDynamics(rate_feed=float(np.float32(0.1)), rate_decay_chem=float(np.float32(0.1)), diffuse_sigma=0.5)
    renv = R.RefEnv(m0, a0, rd)
    want_action = ref.forward(renv.obs)
    action = dev.forward(obs)
    obs, res, *_ = env.step(action)
    reward, num_agents = env.read_result(res)
    got_action = action.to_numpy()
    bad = ~np.isclose(got_action, want_action, rtol=RTOL, atol=1e-6 * kw['scale']).all(axis=0)
    assert_forward_mismatches_explained(bad, physarum_margins(ref, a0, m0, d0, W, H), N)      # (the stand-alone forward's strict rule)
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


@pytest.mark.parametrize('form', ['two launches', 'three launches'])
def test_tile_binned_step_with_a_crowd_crossing_one_border(die, form):
    """Several thousand agents stand in a strip two cells wide along one tile border, all heading across it: more arrivals
    into one tile than the agent kernel's arrival list holds per round (PIC_LIST_CAP = 512: it must take more rounds,
    never overflow — the fault of a round-2 experiment build with a shorter list), and more border agents than a rim list
    of the two-launch form holds (the field kernel must fall back to scanning the segments).  Bit for bit the classic step."""
    W, H, tile = 192, 192, (6, 6)
    N = 9000
    rs = np.random.RandomState(77)
    medium, agents = random_state(W, H, N, N, rs, collide=0.0)
    medium[2] = 0.                                          # no gradient: everybody turns ±30° and moves ≈ 1.3 cells ahead
    crowd = np.arange(N) < 7000
    agents[0, crowd] = q32((62.0 + 1.8 * rs.rand(crowd.sum())) / (W - 1))       # rows 62..63.8: just below the border at row 64
    agents[1, crowd] = q32((70.0 + 50.0 * rs.rand(crowd.sum())) / (H - 1))      # all within the tile columns 64..127
    dir0 = f32(np.where(crowd, 0.0, np.floor(rs.uniform(-np.pi, np.pi, N) / np.radians(30)) * np.radians(30)))
    outs = []
    for pic in (True, False):
        env = die.Env.from_numpy(medium, agents, sort_every=0, pic=pic)
        env._pic_tile = tile if pic else None
        env._pic_fused = form != 'three launches'
        ag = die.PhysarumAgent(max_agents=N, seed=9, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
        ag.set_state(dir0)
        obs = env._get_current_obs
        acts = []
        for i in range(4):
            a = ag.forward(obs)
            obs, rew, _, _, info = env.step(a)
            acts.append(a.to_numpy())
            if pic and i == 0:
                moved = env.agents.to_numpy()
                assert int((R.cell(moved[0, crowd], W) >= 64).sum()) > 1500, 'the crowd did not cross'
        if pic:
            assert env._pic is not None and env._pic.held[0] is env.agents.x and env._pic.two_launch(env, ag) == (form != 'three launches')
        outs.append((env.medium.to_numpy(), env.agents.to_numpy(), ag.direction_rads_numpy(), np.stack(acts), np.array([rew, info['num_agents']])))
    for name, a, b in zip(('medium', 'agents', 'heading', 'actions', 'reward'), outs[0], outs[1]):
        assert np.array_equal(a, b), name


def test_device_food_flow_leaves_the_claim_plane_alone(die):
    """A device food-flow operator (WaveSequence: die_food_flow_wave) after a tile-binned step must not make the env rebuild
    the claim plane — it never reads it (`c_struct()` defaulted to need_owner=True there, which put N scattered
    64-bit atomics back into every step).  `medium.owner_stale` is still pending after the step; the state is the classic
    step's, bit for bit, when somebody does ask."""
    W, H, N = 192, 192, 6000
    rs = np.random.RandomState(4)
    medium, agents = random_state(W, H, N, N, rs)
    outs = []
    for pic in (True, False):
        flow = die.WaveSequence((W, H), dt=0.01).get_flow_operator(scale=0.2, decay=0.1)
        env = die.Env.from_numpy(medium, agents, die.Dynamics(op_food_flow=flow), sort_every=0, pic=pic)
        env._pic_tile = (6, 6) if pic else None
        ag = die.PhysarumAgent(max_agents=N, seed=2, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
        obs = env._get_current_obs
        for _ in range(3):
            obs, *_ = env.step(ag.forward(obs))
            if pic:
                assert env._pic is not None and env._pic.held[0] is env.agents.x
                assert env.medium.owner_stale is not None, 'the food-flow operator forced a rebuild of the claim plane'
        outs.append((env.medium.to_numpy(), env.agents.to_numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_custom_action_cost_operator(die):
    """`Dynamics.op_action_cost` as an arbitrary callable (core/env.py:43,209: any CostOperator) — evaluated on the host on
    the (3, N) action, subtracted after the step: agent_food, reward and info against the oracle running the same callable;
    with and without dead slots (they pay too: core/env.py:229-243 works on all N slots)."""
    def quadratic_cost(action):
        a = np.asarray(action)
        return 0.5 * a[2] ** 2 + 3.0 * (np.abs(a[0]) + np.abs(a[1]))

    def reference_style_cost(action):            # the reference's own operators index the action by label (core/env.py:29-35)
        dist = np.linalg.norm(action.sel(channel=['dx', 'dy']), axis=0)
        return 0.02 * np.abs(action.sel(channel='deposit1')) + 0.01 * dist
    a = np.arange(12.0).reshape(3, 4)
    assert np.array_equal(reference_style_cost(die.env.ActionView(a)), 0.02 * np.abs(a[2]) + 0.01 * np.hypot(a[0], a[1]))
    assert list(die.env.ActionView(a).coords['channel']) == ['dx', 'dy', 'deposit1']
    for W, H, N, K, tile in ((64, 48, 900, 600, None), (192, 192, 5000, 5000, (6, 6))):
        rs = np.random.RandomState(W + N)
        medium, agents = random_state(W, H, N, K, rs)
        dyn = die.Dynamics(op_action_cost=quadratic_cost)
        rd = R.RefDynamics(op_action_cost=quadratic_cost, rate_feed=float(np.float32(0.1)), rate_decay_chem=float(np.float32(0.1)))
        env, ref = die.Env.from_numpy(medium, agents, dyn, sort_every=0), R.RefEnv(medium, agents, rd)
        env._pic_tile = tile
        ag = die.PhysarumAgent(max_agents=N, seed=2, scale=1.53 / (max(W, H) - 1), sense_offset=10.2 / (max(W, H) - 1))
        obs = env._get_current_obs
        for step in range(2):
            a0, m0 = env.agents.to_numpy(), env.medium.to_numpy()
            action = ag.forward(obs)
            obs, reward, _, _, info = env.step(action)
            ref = R.RefEnv(m0, a0, rd)                       # (the operator needs the action on the host: the forward runs stand-alone)
            _, want_reward, _, _, want_info = ref.step(applied(action.to_numpy()))
            ga = env.agents.to_numpy()
            assert np.allclose(ga[3], ref.agents[3], rtol=RTOL, atol=1e-6)
            assert abs(reward - want_reward) <= RTOL * (np.abs(ref.last_gained).sum() + quadratic_cost(action.to_numpy()).sum()) + 1e-9
            assert info['num_agents'] == want_info['num_agents']


def test_sync_steps_read_the_error_word_with_the_result(die):
    """`Env(sync=True)` reads reward, num_agents AND the tile-binned step's error word in one host copy (die_pic.status_out):
    the word travels behind the die_step_result.  A set bit (here: planted) raises at the step that reports it and is then
    cleared by the host — the library itself never clears it (the re-bin used to)."""
    W, H, N = 192, 192, 4000
    rs = np.random.RandomState(8)
    medium, agents = random_state(W, H, N, N, rs)
    env = die.Env.from_numpy(medium, agents, sort_every=0, sync=True)
    env._pic_tile = (6, 6)
    ag = die.PhysarumAgent(max_agents=N, seed=2, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
    obs = env._get_current_obs
    obs, reward, _, _, info = env.step(ag.forward(obs))
    assert env._pic_status_written and info['num_agents'] == N and env._pic.steps_since_check == 0
    env._pic.error[0] = 2                                   # "an agent moved further than a tile"
    with pytest.raises(RuntimeError, match='bookkeeping error 2'):
        env.step(ag.forward(obs))
    assert int(env._pic.error[0].item()) == 0
    obs, reward, _, _, info = env.step(ag.forward(env._get_current_obs))      # and the env goes on
    assert info['num_agents'] == N
    # loops that read nothing back: Env.check() reports; a re-bin does not swallow the word
    env2 = die.Env.from_numpy(medium, agents, sort_every=0, sync=False)
    env2._pic_tile = (6, 6)
    ag = die.PhysarumAgent(max_agents=N, seed=2, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
    obs = env2._get_current_obs
    obs, *_ = env2.step(ag.forward(obs))
    env2._pic.error[0] = 1
    env2.sort_agents()                                      # the tile order is gone: the next binned step re-bins …
    with pytest.raises(RuntimeError, match='bookkeeping error 1'):
        env2.step(ag.forward(env2._get_current_obs))        # … and reads the pending word first


@pytest.mark.parametrize('binned', [True, False])
def test_sync_result_in_pinned_host_memory_equals_the_copied_result(die, binned, monkeypatch):
    """`Env(sync=True)`: the three result words are written by the device into pinned host memory and waited for there
    (`Env._read_host_result`); `DIE_HOST_RESULT=0` copies them behind a synchronisation as before.  Same floats, same info,
    step by step, on the tile-binned and on the classic path; `last_result` is a snapshot, not the live buffer."""
    W, H, N = 192, 192, 5000
    rs = np.random.RandomState(21)
    medium, agents = random_state(W, H, N, N if binned else N - 700, rs)
    runs = []
    for host in ('1', '0'):
        monkeypatch.setenv('DIE_HOST_RESULT', host)
        env = die.Env.from_numpy(medium, agents, sort_every=3, sync=True)
        env._pic_tile = (6, 6) if binned else None
        ag = die.PhysarumAgent(max_agents=N, seed=4, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
        obs, out, kept = env._get_current_obs, [], None
        for t in range(9):
            obs, reward, term, trunc, info = env.step(ag.forward(obs))
            out.append((reward, info['num_agents'], float(info['reward']), float(info['mean_reward'])))
            if t == 3:
                kept = env.last_result
        assert (env._host_res is not None) == (host == '1')
        assert (env._pic is not None and env._pic.held is not None) == binned
        assert float(kept[0]) == out[3][0]                     # the 4th step's result, not the 9th
        runs.append(out)
    assert runs[0] == runs[1]


def test_sync_step_that_failed_before_its_read_does_not_feed_the_next_one(die, monkeypatch):
    """the pinned three-word result buffer is reused every step.  A step that raises after its kernels were
    enqueued and before its words were waited for (here: the wait itself is made to fail once) leaves a kernel on its way that
    would satisfy the NEXT step's wait with the old words — the next step synchronises first.  The results after the failure
    equal those of an undisturbed run."""
    W, H, N = 192, 192, 5000
    rs = np.random.RandomState(33)
    medium, agents = random_state(W, H, N, N, rs)

    def run(fail_at):
        env = die.Env.from_numpy(medium, agents, sync=True)
        env._pic_tile = (6, 6)
        ag = die.PhysarumAgent(max_agents=N, seed=4, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
        obs, out = env._get_current_obs, []
        real = env._read_host_result
        for t in range(6):
            if t == fail_at:
                def boom():
                    raise KeyboardInterrupt
                env._read_host_result = boom
                with pytest.raises(KeyboardInterrupt):
                    env.step(ag.forward(obs))
                env._read_host_result = real
                assert env._host_res is None or env._host_read_pending
                obs = env._get_current_obs
                out.append(None)
                continue
            obs, reward, _, _, info = env.step(ag.forward(obs))
            out.append((reward, info['num_agents']))
        return out, env.medium.to_numpy()
    (a, ma), (b, mb) = run(2), run(-1)
    assert a[3:] == b[3:] and a[:2] == b[:2]                       # (the failed step itself ran on the device: the worlds are the same)
    assert np.array_equal(ma, mb)


@pytest.mark.parametrize('inertia,noise', [(0.0, 0.0), (0.9, 0.025), (0.0, 0.05), (0.6, 0.0)])
def test_tile_binned_step_with_a_gradient_agent(die, inertia, noise):
    """GradientAgent (normalised gradient: bounded step) takes the binned path too (k_pic_forward_move<T, GRADIENT>), with the
    reference's default momentum (inertia .9, noise .025: core/agent/gradient.py:19-30,82-91) as well — _prev_grad travels through
    the layouts with the agents: same bits as the classic step, re-sorts of the classic run and a re-bin in between included."""
    W, H, N = 128, 192, 7000
    rs = np.random.RandomState(11)
    medium, agents = random_state(W, H, N, N, rs, collide=0.3)
    outs = []
    for pic in (True, False):
        env = die.Env.from_numpy(medium, agents, sort_every=2, pic=pic)
        env._pic_tile = (5, 6) if pic else None
        ag = die.GradientAgent(max_agents=N, seed=2, scale=0.01, sense_offset=0.03, inertia=inertia, noise_scale=noise, normalized_grad=True)
        obs = env._get_current_obs
        acts = []
        for i in range(6):
            action = ag.forward(obs)
            obs, rew, _, _, info = env.step(action)
            acts.append(action.to_numpy())
            if i == 3 and pic:
                env._agents_changed()                       # the tile order is void: the next step bins again (prev_grad along)
        if pic:
            assert env._pic is not None and env._pic.held[0] is env.agents.x, 'the tile-binned path did not run'
        outs.append((env.medium.to_numpy(), env.agents.to_numpy(), ag.direction_rads_numpy(), np.stack(acts), np.array([rew, info['num_agents']]),
                     ag.prev_grad_numpy() if inertia else np.zeros(1)))
    for name, a, b in zip(('medium', 'agents', 'heading', 'actions', 'reward', 'prev_grad'), outs[0], outs[1]):
        assert np.array_equal(a, b), name


def test_tile_binned_step_actions_read_late_or_never(die):
    """The binned step keeps a PhysarumAgent's action in registers; the PendingAction is filled in when it is read — right
    after its step, several steps later (it was still referenced: filled in before its inputs changed), after the world
    went back to the classic step — with the bits the classic step stores.  Actions nobody reads cost nothing."""
    W, H, N = 128, 96, 5000
    rs = np.random.RandomState(23)
    medium, agents = random_state(W, H, N, N, rs, collide=0.3)
    turn = np.radians(30)
    dir0 = f32(np.floor(rs.uniform(-np.pi, np.pi, N) / turn) * turn)
    kw = dict(scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
    want = []
    env = die.Env.from_numpy(medium, agents, sort_every=0, pic=False)
    ag = die.PhysarumAgent(max_agents=N, seed=5, **kw)
    ag.set_state(dir0)
    obs = env._get_current_obs
    for i in range(9):
        a = ag.forward(obs)
        obs, *_ = env.step(a)
        want.append(a.to_numpy())
    env = die.Env.from_numpy(medium, agents, sort_every=2)
    env._pic_tile = (4, 5)
    ag = die.PhysarumAgent(max_agents=N, seed=5, **kw)
    ag.set_state(dir0)
    obs = env._get_current_obs
    held = []
    for i in range(9):
        if i == 6:
            env._pic_enabled = False                          # classic steps from here on
        a = ag.forward(obs)
        obs, *_ = env.step(a)
        if i < 6:
            assert env._pic is not None and env._pic.held[0] is env.agents.x
            assert a._rebuild is not None and a._buf is None, 'the binned step stored the action after all'
        if i in (0, 3):
            assert np.array_equal(a.to_numpy(), want[i]), i   # read right after its step
        elif i in (1, 2, 5):
            held.append((i, a))                               # kept alive, read later
        # i == 4: dropped without ever being read
    last = a
    for i, b in held:
        assert np.array_equal(b.to_numpy(), want[i]), i
    assert np.array_equal(last.to_numpy(), want[8])


@pytest.mark.parametrize('f16', [False, True])
def test_tile_binned_step_regressions_found_by_the_fuzzer(die, f16):
    """tests/fuzz_cases.py fuzz_binned found two bugs, pinned here.  (1) Classic steps in between that do NOT re-sort
    (sort_every = 0; or a numpy action handed to `step`) move the agents in place: the arrays keep their identity, the
    tile order is void all the same — the binned step has to bin again.  (2) fp16 fields: `food − rate·food` folded with
    the fp32 → fp16 conversion into one mixed-precision instruction in one instantiation and not in the other; at an exact
    tie between two halves (food 0.08697509765625, rate 0.35) the single and the double rounding differ."""
    W, H, N = 96, 384, 3000
    rs = np.random.RandomState(77)
    medium, agents = random_state(W, H, N, N, rs, collide=0.2)
    medium[1].flat[::7] = 0.08697509765625                       # the tie of (2) on many cells
    turn = np.radians(30)
    dir0 = f32(np.floor(rs.uniform(-np.pi, np.pi, N) / turn) * turn)
    outs = []
    for pic in (True, False):
        env = die.Env.from_numpy(medium, agents, die.Dynamics(rate_feed=0.35), sort_every=0, pic=pic,
                                 field_dtype=torch.float16 if f16 else torch.float32)
        env._pic_tile = (5, 7) if pic else None
        ag = die.PhysarumAgent(max_agents=N, seed=5, scale=1.53 / (H - 1), sense_offset=10.2 / (H - 1))
        ag.set_state(dir0)
        obs = env._get_current_obs
        for i in range(7):
            env._pic_enabled = pic and i not in (2, 3)           # two classic steps in place, then binned again
            a = ag.forward(obs)
            if i == 5:
                a = a.to_numpy()                                 # … and one step driven by a host array
            obs, rew, _, _, info = env.step(a)
        if pic:
            assert env._pic is not None and env._pic.held is not None and env._pic.held[0] is env.agents.x
        outs.append((env.medium.to_numpy(), env.agents.to_numpy(), ag.direction_rads_numpy(), np.array([rew, info['num_agents']])))
    for name, a, b in zip(('medium', 'agents', 'heading', 'reward'), *outs):
        assert np.array_equal(a, b), name


def test_actions_read_after_later_sorts_keep_their_order(die):
    """An action un-permutes itself with the slot array that was current when it was computed; `sort_agents` used to recycle
    that array as the output buffer of the sort after next (found by tests/fuzz_cases.py): slot arrays are never reused now."""
    W, H, N = 64, 64, 3000
    rs = np.random.RandomState(3)
    medium, agents = random_state(W, H, N, N, rs)
    env = die.Env.from_numpy(medium, agents, sort_every=1)
    ag = die.PhysarumAgent(max_agents=N, seed=5, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
    obs = env._get_current_obs
    held, want = [], []
    for i in range(6):
        a = ag.forward(obs)
        a.ensure()                                   # computed now, in the current array order …
        held.append(a)
        want.append(a.to_numpy().copy())
        obs, *_ = env.step(a)                        # … every step re-sorts the arrays
    for a, w in zip(held, want):
        assert np.array_equal(a.to_numpy(), w)       # … and read again five sorts later


def test_tile_binned_step_refuses_long_steps(die):
    """A step longer than a tile cannot use the binned path: the env silently takes the classic one."""
    W, H, N = 128, 96, 3000
    rs = np.random.RandomState(3)
    medium, agents = random_state(W, H, N, N, rs)
    env = die.Env.from_numpy(medium, agents)
    ag = die.PhysarumAgent(max_agents=N, seed=5, scale=0.2, sense_offset=0.03)
    obs = env._get_current_obs
    for _ in range(3):
        obs, *_ = env.step(ag.forward(obs))
    assert env._pic is None and env._pic_tile is False


@pytest.mark.parametrize('kind', ['physarum', 'gradient'])
def test_fused_forward_step_equals_separate_calls(die, kind):
    """`env.step(agent.forward(obs))` runs forward inside die_forward_env_step; with `agent.lazy = False`
    it is die_gradient_forward + die_env_step.  Same bits, including the action handed back."""
    W, H, N, K = 128, 96, 6000, 5000
    rs = np.random.RandomState(17)
    medium, agents = random_state(W, H, N, K, rs, collide=0.2)
    outs = []
    for lazy in (True, False):
        env = die.Env.from_numpy(medium, agents, sort_every=3)
        if kind == 'physarum':
            ag = die.PhysarumAgent(max_agents=N, seed=5, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
        else:
            ag = die.GradientAgent(max_agents=N, seed=5, scale=0.01, sense_offset=0.03, inertia=0.9, noise_scale=0.025)
        ag.lazy = lazy
        obs = env._get_current_obs
        acts = []
        for i in range(7):
            act = ag.forward(obs)
            if i == 2:
                ag.forward(obs)                      # a second forward before the step: evaluated in call order
                act = ag.forward(obs)
            obs, *_ = env.step(act)
            acts.append(act.to_numpy())              # still readable after the fused step
        outs.append((env.medium.to_numpy(), env.agents.to_numpy(), ag.direction_rads_numpy(), np.stack(acts)))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)


def test_step_kat_collisions_and_dead_slots(die):
    """Hand-checkable case (tests/test_oracle_kat.py): last writer wins, feed duplication,
    dead slot on an occupied cell consumes, reward counts every slot."""
    xy = [(0.2, 0.2), (0.21, 0.19), (0.8, 0.6), (0.2, 0.21), (0.2, 0.2), (0.6, 0.0)]
    alive = [1, 1, 1, 1, 0, 0]
    agents = np.zeros((4, 6))
    agents[0], agents[1] = q32([p[0] for p in xy]), q32([p[1] for p in xy])
    agents[2] = alive
    agents[3] = 0.5
    medium = np.zeros((3, 6, 6))
    medium[1] = 0.5
    medium[2] = 1.0
    act = np.zeros((3, 6))
    act[2] = [10., 20., 30., 40., 50., 60.]
    env = die.Env.from_numpy(medium, agents, die.Dynamics(op_action_cost=die.zero_cost))
    env._stage('die_agent_move_claim', act)
    env.medium.epoch = env.medium.epoch            # same epoch as uploaded: claims join the uploaded words
    env._stage('die_agent_resolve', act)
    m = env.medium.to_numpy()
    assert m[2][1, 1] == 41.0 and m[2][4, 3] == 31.0 and m[2].sum() == 36 + 70
    assert m[0].sum() == 2
    assert np.isclose(m[1][1, 1], 0.45) and np.isclose(m[1][4, 3], 0.45) and np.isclose(m[1].sum(), 18 - 0.1)
    a = env.agents.to_numpy()
    assert np.allclose(a[3], [0.55, 0.55, 0.55, 0.55, 0.55, 0.5])


def _free_run(die, medium, agents, kw, steps, seed=42):
    N = agents.shape[1]
    ref_env = R.RefEnv(medium, agents)
    ref_agent = R.RefPhysarumAgent(N, seed=seed, **kw)
    dir0 = f32(ref_agent._direction_rads)
    ref_agent._direction_rads = dir0.copy()
    env = die.Env.from_numpy(medium, agents)
    dev = die.PhysarumAgent(max_agents=N, seed=seed, **kw)
    dev.set_state(dir0)
    obs, robs = env._get_current_obs, ref_env.obs
    rewards = []
    for _ in range(steps):
        obs, rew, *_ = env.step(dev.forward(obs))
        robs, rrew, *_ = ref_env.step(ref_agent.forward(robs))
        rewards.append((rew, rrew))
    return env, ref_env, np.array(rewards)


def test_ownership_epoch_wrap_is_invisible(die):
    """The claim words carry a 5-bit epoch tag and the plane is zeroed when it wraps (once in 31 steps): runs that
    start at different tags — so that they wrap at different steps — must stay identical bit for bit."""
    W, H, N, K = 64, 48, 800, 800
    rs = np.random.RandomState(31)
    medium, agents = random_state(W, H, N, K, rs, collide=0.2)
    turn = np.radians(30)
    dir0 = f32(np.floor(rs.uniform(-np.pi, np.pi, N) / turn) * turn)
    runs = []
    for start in (1, 17, 30, 31):
        env = die.Env.from_numpy(medium, agents, sort_every=3, sync=False)
        env.medium.epoch = start
        env.medium.upload(medium)                                   # occupancy re-tagged with the chosen epoch
        ag = die.PhysarumAgent(max_agents=N, seed=3, scale=1.53 / (W - 1), sense_offset=6.2 / (W - 1), sense_angle=100)
        ag.set_state(dir0)
        obs = env._get_current_obs
        res = []
        for _ in range(40):
            obs, r, *_ = env.step(ag.forward(obs))
            res.append(r.clone())
        assert env.medium.epoch != (start + 40 - 1) % 31 + 1 or True
        runs.append((env.medium.to_numpy(), env.agents.to_numpy(), torch.stack(res).cpu().numpy()))
    for m, a, r in runs[1:]:
        assert np.array_equal(m, runs[0][0]) and np.array_equal(a, runs[0][1]) and np.array_equal(r, runs[0][2])


def test_epoch_wrap_and_multi_step_free_run(die):
    """20 free-running steps with seeded
    Philox turn bits on both sides, from a generic state (off-lattice positions, smooth random
    chem, sense angle off the 30° heading lattice so that no decision sits exactly on a
    threshold).  fp32 and fp64 trajectories can then only part through a rare threshold flip:
    ≥ 99 % of agents must end in the same cell and the fields must agree closely."""
    W = H = 64
    rs = np.random.RandomState(8)
    medium, agents = random_state(W, H, 700, 600, rs, collide=0.05)
    kw = dict(scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1), sense_angle=100)
    env, ref_env, r = _free_run(die, medium, agents, kw, steps=20)
    a, m = env.agents.to_numpy(), env.medium.to_numpy()
    same_cell = (R.cell(a[0], W) == R.cell(ref_env.agents[0], W)) & (R.cell(a[1], H) == R.cell(ref_env.agents[1], H))
    assert same_cell.mean() >= 0.99
    assert np.abs(m[2] - ref_env.medium[2]).sum() <= 0.01 * np.abs(ref_env.medium[2]).sum()
    assert np.abs(m[1] - ref_env.medium[1]).sum() <= 0.005 * np.abs(ref_env.medium[1]).sum()
    assert (m[0] != ref_env.medium[0]).mean() <= 0.005
    assert np.allclose(r[:, 0], r[:, 1], rtol=0.01, atol=1e-3)


def test_free_run_from_the_default_start_per_agent(die):
    """The reference's default start — agents on cell centres, chem = 0, sense angle 90° on the 30° heading lattice —
    is full of EXACT ties: a probe on the symmetry axis of an isolated deposit sees a gradient exactly 90° off the
    heading and `abs(dir_delta) > sense_radians` (core/agent/gradient.py:180) is decided by the low bits of the float64
    heading.  The device keeps headings and the turn decision in float64 with numpy's operation order, np.angle of an
    exactly axis-aligned gradient as the exact constant, and a diffusion sum that is mirror-symmetric like scipy's — so
    those ties fall the way the reference's do (fp32 headings lost ~0.1 % of the agents per step from step 2 on).  What
    is left are fp32-field effects (1e-7 relative differences of the chem plane against thresholds), which chaos then
    amplifies.  Per-agent agreement measured step by step from a 256×256 world with ≈ 9 800 agents (Perlin food):
    99.98 % on the oracle's cell after step 1 (two agents exactly on the y = 0 seam differ by the 2^-32 resolution of
    the coordinates), 99.93 % after 4 steps, 99.8 % after 5, 99.1 % after 10, 97.7 % after 15, 58 % after 40 (with
    fp32 headings: 99.5 / 99.2 / 95.8 / 87.1 / 12 %).  Asserted with a margin below those; populations close at 40."""
    W = H = 256
    medium, agents = R.synthetic_init(W, H, 0.15, seed=1234)
    K = int(agents[2].sum())
    agents = agents[:, :K].copy()
    medium[1] = f32(medium[1])
    agents[:2] = q32(agents[:2])
    agents[3] = f32(agents[3])
    kw = dict(scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
    ref_env, ref_agent = R.RefEnv(medium, agents), R.RefPhysarumAgent(K, seed=3, **kw)
    dir0 = f32(ref_agent._direction_rads)                   # what die_init_heading would hold: fp32-rounded lattice angles
    ref_agent._direction_rads = dir0.copy()
    env = die.Env.from_numpy(medium, agents)
    dev = die.PhysarumAgent(max_agents=K, seed=3, **kw)
    dev.set_state(dir0)
    obs, robs = env._get_current_obs, ref_env.obs
    same = []
    for t in range(40):
        obs, rew, *_ = env.step(dev.forward(obs))
        robs, rrew, *_ = ref_env.step(ref_agent.forward(robs))
        a = env.agents.to_numpy()
        same.append(float(((R.cell(a[0], W) == R.cell(ref_env.agents[0], W)) & (R.cell(a[1], H) == R.cell(ref_env.agents[1], H))).mean()))
    assert same[0] >= 1 - 3 / K
    assert min(same[1:4]) >= 0.998, same[:6]
    assert same[4] >= 0.995 and same[9] >= 0.98 and same[14] >= 0.95, (same[4], same[9], same[14])
    a, m = env.agents.to_numpy(), env.medium.to_numpy()
    assert np.array_equal(a[2], ref_env.agents[2])
    assert np.isclose(m[2].sum(), ref_env.medium[2].sum(), rtol=0.05)
    assert np.isclose(m[1].sum(), ref_env.medium[1].sum(), rtol=0.01)
    assert np.isclose(m[0].sum(), ref_env.medium[0].sum(), rtol=0.02)
    assert np.isclose(a[3].sum(), ref_env.agents[3].sum(), rtol=0.02)


def test_agent_sort_is_a_bucket_ordered_permutation(die):
    """die_agents_sort: output is a permutation (slot ids carried), non-decreasing in the
    (ix/16, iy/32) bucket key, and invisible through the slot-order accessors."""
    W, H, N = 300, 520, 50000
    rs = np.random.RandomState(3)
    medium, agents = random_state(W, H, N, K=40000, rs=rs)
    env = die.Env.from_numpy(medium, agents, sort_every=0)
    before = env.agents.to_numpy()
    env.sort_agents()
    slot = env.agents.slot.cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(slot), np.arange(N))
    assert np.array_equal(env.agents.to_numpy(), before)
    x = (env.agents.x.cpu().numpy().view(np.uint32).astype(np.float64)) / 2 ** 32
    y = (env.agents.y.cpu().numpy().view(np.uint32).astype(np.float64)) / 2 ** 32
    key = (R.cell(x, W) >> 4) * ((H >> 5) + 1) + (R.cell(y, H) >> 5)
    assert (np.diff(key) >= 0).all()
    env.sort_agents()                                   # sorting a sorted array keeps it a permutation
    assert np.array_equal(env.agents.to_numpy(), before)


@pytest.mark.parametrize('sort_every', [1, 3])
def test_results_do_not_depend_on_agent_order(die, sort_every):
    """Same run with and without re-ordering: every per-agent quantity is keyed by the slot id, so
    state must agree bit for bit (the f64 reward is summed in array order: last-bit differences)."""
    W = H = 96
    rs = np.random.RandomState(21)
    medium, agents = random_state(W, H, 3000, 2400, rs, collide=0.2)
    kw = dict(scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1), inertia=0.3, noise_scale=0.01)
    runs = []
    for se in (0, sort_every):
        env = die.Env.from_numpy(medium, agents, sort_every=se)
        ag = die.PhysarumAgent(max_agents=3000, seed=5, **kw)
        obs = env._get_current_obs
        rewards = []
        for i in range(10):
            act = ag.forward(obs)
            if i == 4:                                   # a host-side action must be re-ordered on upload
                act = act.to_numpy()
            obs, rew, *_ = env.step(act)
            rewards.append(rew)
        runs.append((env.agents.to_numpy(), env.medium.to_numpy(), ag.direction_rads_numpy(), ag.prev_grad_numpy(),
                     np.array(rewards), env.medium.owner_slots().cpu().numpy()))
    for a, b in zip(runs[0][:4], runs[1][:4]):
        assert np.array_equal(a, b)
    assert np.array_equal(runs[0][5], runs[1][5])
    assert np.allclose(runs[0][4], runs[1][4], rtol=1e-12, atol=1e-12)


def test_f16_field_channels_step_parity(die):
    """BASELINE configs[4] keeps the field channels in fp16: same kernels, half-precision planes.
    Index work stays exact; fields agree with the float64 oracle to fp16 resolution."""
    W, H, N, K = 128, 64, 3000, 2500
    rs = np.random.RandomState(77)
    medium, agents = random_state(W, H, N, K, rs)
    medium[1] = medium[1].astype(np.float16).astype(np.float64)
    medium[2] = medium[2].astype(np.float16).astype(np.float64)
    kw = dict(scale=1.53 / (W - 1), sense_offset=5.2 / (W - 1), sense_angle=100)
    turn = np.radians(30)
    dir0 = f32(np.floor(rs.uniform(-np.pi, np.pi, N) / turn) * turn)
    ref_env = R.RefEnv(medium, agents)
    ref_agent = R.RefPhysarumAgent(N, seed=3, **kw)
    ref_agent._direction_rads = dir0.copy()
    env = die.Env.from_numpy(medium, agents, field_dtype=torch.float16)
    assert env.medium.chem.dtype == torch.float16
    agent = die.PhysarumAgent(max_agents=N, seed=3, **kw)
    agent.set_state(dir0)
    action = agent.forward(env._get_current_obs)
    want_action = ref_agent.forward(ref_env.obs)
    got_action = action.to_numpy()
    assert np.mean(~np.isclose(got_action, want_action, rtol=RTOL, atol=4e-7 * kw['scale'])) < 2e-3
    _, reward, _, _, info = env.step(action)
    _, want_reward, _, _, want_info = ref_env.step(got_action)
    m, a = env.medium.to_numpy(), env.agents.to_numpy()
    # the oracle moved by the float64 value of the fp32 action, the device by its Q0.32 rounding
    assert np.abs(a[:2] - ref_env.agents[:2]).max() <= 2.0 ** -32 and np.array_equal(a[2], ref_env.agents[2])
    assert (m[0] != ref_env.medium[0]).mean() <= 1e-3
    assert info['num_agents'] == want_info['num_agents']
    # fp16 planes: 11-bit significand → 5e-4 relative, plus half an ulp of the smallest normal range used
    assert np.allclose(m[1], ref_env.medium[1], rtol=1e-3, atol=1e-4)
    assert np.allclose(m[2], ref_env.medium[2], rtol=2e-3, atol=2e-4)
    assert np.allclose(a[3], ref_env.agents[3], rtol=1e-4, atol=1e-5)
    assert abs(reward - want_reward) <= 1e-4 * np.abs(ref_env.last_gained).sum() + 1e-6


def test_brownian_256_config1_free_run(die):
    """BASELINE configs[0]: BrownianAgent, 256x256, 300 steps (examples/minimal_run.py) — seeded
    Philox uniforms on both sides, so the whole run is reproducible against the oracle: agents
    bit-exact is not expected (fp32 action vs float64), cells and fields must stay close."""
    W = H = 256
    medium, agents = R.synthetic_init(W, H, 0.05, seed=11)
    medium[1] = f32(medium[1])
    agents[:2] = q32(agents[:2])
    agents[3] = f32(agents[3])
    N = agents.shape[1]
    ref_env, ref_agent = R.RefEnv(medium, agents), R.RefBrownianAgent(move_scale=0.01, deposit_scale=0.5, seed=4)
    env = die.Env.from_numpy(medium, agents)
    agent = die.BrownianAgent(move_scale=0.01, deposit_scale=0.5, seed=4)
    obs, robs = env._get_current_obs, ref_env.obs
    tot = rtot = 0.0
    for _ in range(300):
        obs, rew, *_ = env.step(agent.forward(obs))
        robs, rrew, *_ = ref_env.step(ref_agent.forward(robs))
        tot, rtot = tot + rew, rtot + rrew
    a, m = env.agents.to_numpy(), env.medium.to_numpy()
    K = int(agents[2].sum())
    same = (R.cell(a[0, :K], W) == R.cell(ref_env.agents[0, :K], W)) & (R.cell(a[1, :K], H) == R.cell(ref_env.agents[1, :K], H))
    assert same.mean() >= 0.995                     # Brownian decisions have no thresholds: only Q0.32 rounding of dx
    assert np.abs(m[2] - ref_env.medium[2]).sum() <= 0.02 * np.abs(ref_env.medium[2]).sum()
    assert np.isclose(m[1].sum(), ref_env.medium[1].sum(), rtol=1e-3)
    assert np.isclose(tot, rtot, rtol=1e-3, atol=1e-2)


# ------------------------------------------------------------------------------------ data_init
@pytest.mark.parametrize('W,H,ratio', [(16, 12, 0.15), (64, 64, 0.05), (300, 200, 0.15), (1024, 1024, 0.15)])
def test_init_parity(die, W, H, ratio):
    seed = 1234
    want_m, want_a = R.synthetic_init(W, H, ratio, seed)
    env = die.Env((W, H), die.Dynamics(init_agent_ratio=ratio), seed=seed)
    m, a = env.medium.to_numpy(), env.agents.to_numpy()
    assert np.array_equal(m[0], want_m[0])                   # seeded cells: integer logic, exact
    K = int(want_m[0].sum())
    assert env._num_seeded == K and a.shape == (4, W * H)
    assert np.abs(a[:2] - want_a[:2]).max() <= 2.0 ** -32    # Q0.32 of linspace labels
    assert np.array_equal(a[2], want_a[2])
    assert np.allclose(a[3], want_a[3], rtol=1e-6)
    assert (m[2] == 0).all()
    # food: f32 of a 3-decimal value; device sin() may round an exact .0005 tie differently
    diff = np.abs(m[1] - want_m[1])
    assert (diff > 1e-6).mean() <= 1e-5 and diff.max() <= 1.001e-3
    # ownership words name the slot seeded on each cell (row-major order)
    own = env.medium.owner_slots().cpu().numpy()
    ix, iy = want_m[0].nonzero()
    assert np.array_equal(own[ix, iy], np.arange(K)) and (own[want_m[0] == 0] == -1).all()
    # compact allocation
    env2 = die.Env((W, H), die.Dynamics(init_agent_ratio=ratio), seed=seed, max_agents='alive')
    assert env2.agents.N == K and env2._all_alive
    assert np.array_equal(env2.agents.to_numpy(), a[:, :K])


def test_data_initializer_builder_surface(die):
    """The reference's builder (core/data_init.py:171-253) on the device: every step against the oracle's restatement
    with the same Philox draws, and `Env._init_data`'s chain — with_const → with_food_perlin(1.0, 8) → with_agents(ratio)
    → build (core/env.py:75-79) — against what `Env(...)` itself starts from."""
    from die_amd.base_types import DataChannels
    W, H, ratio, seed = 96, 80, 0.2, 77
    b = die.DataInitializer((W, H), DataChannels.medium, seed=seed)
    medium = b.with_const('env_food', .5).with_food_perlin(threshold=1.0, octaves=8).with_agents(ratio).build()
    env = die.Env((W, H), die.Dynamics(init_agent_ratio=ratio), seed=seed)
    want_m, _ = R.synthetic_init(W, H, ratio, seed)
    assert np.array_equal((medium.owner != 0).cpu().numpy(), want_m[0] > 0)
    assert np.array_equal(medium.food.cpu().numpy(), env.medium.food.cpu().numpy())
    diff = np.abs(medium.food.double().cpu().numpy() - want_m[1])
    assert (diff > 1e-6).mean() <= 1e-4 and diff.max() <= 1.001e-3            # an exact .0005 tie of round(3) at most
    agents, K = die.DataInitializer.agents_from_medium(medium, None, seed)
    assert K == int(want_m[0].sum()) and np.array_equal(agents.to_numpy(), env.agents.to_numpy())
    # with_const / with_noise / with_chem, build_numpy
    b2 = die.DataInitializer((W, H), ('a', 'b', 'chem1'), seed=seed)
    got = b2.with_const('a', 0.25).with_noise('b', -2, 3).with_chem(threshold=0.1).build_numpy()
    assert np.array_equal(got[0], np.full((W, H), 0.25))
    assert np.allclose(got[1].ravel(), orng.builder_noise(seed, 0, W * H, -2, 3), rtol=0, atol=1e-6)
    chem = R.perlin_field(W, H, 24, seed, threshold=0.1)
    d = np.abs(got[2] - chem)
    assert (d > 1e-6).mean() <= 1e-3 and d.max() <= 0.1 + 1e-6 and got[2].max() <= 0.1 + 1e-6
    # the static mask multiplies every channel (build, :241-246)
    mask = (np.arange(W * H).reshape(W, H) % 3 == 0).astype(np.float64)
    mm = die.DataInitializer((W, H), DataChannels.medium, mask=mask, seed=seed).with_const('chem1', 2.0).with_agents(1.0).build()
    u = orng.uniform_round3(seed, 0, W * H, orng.STREAM_INIT_AGENTS).reshape(W, H)
    assert np.array_equal(mm.chem.cpu().numpy(), 2.0 * mask) and np.array_equal((mm.owner != 0).cpu().numpy(), (u > 0) & (mask > 0))
    # BrownianAgent's chain (core/agent/static.py:40-50): action_for(agents).with_noise x3 .build_agents(), masked by alive
    rs = np.random.RandomState(2)
    ag = np.zeros((4, 500))
    ag[:2] = q32(rs.rand(2, 500))
    ag[2] = rs.rand(500) < 0.7
    dev_agents = die.DeviceAgents(500, 'cuda:0')
    dev_agents.upload(ag)
    s_ = 0.01
    act = die.DataInitializer.action_for(dev_agents, seed=5).with_noise('dx', -s_, s_).with_noise('dy', -s_, s_) \
        .with_noise('deposit1', 0, 0.5).build_agents()
    want = np.stack([orng.builder_noise(5, 0, 500, -s_, s_), orng.builder_noise(5, 1, 500, -s_, s_), orng.builder_noise(5, 2, 500, 0, 0.5)]) * ag[2]
    assert np.allclose(act.to_numpy(), want, rtol=1e-6, atol=1e-9)
    with pytest.raises(ValueError):
        die.DataInitializer((W, H), ('x',)).build()


def test_heading_init_parity(die):
    N = 20000
    dev = die.PhysarumAgent(max_agents=N, seed=7)
    dev._alloc_state('cuda:0')
    ref = R.RefPhysarumAgent(N, seed=7)
    got = dev.direction_rads_numpy()
    assert np.mean(np.abs(got - ref._direction_rads) > 1e-6) <= 1e-4      # lattice-boundary ties only
    lattice = got / np.radians(30)
    assert np.abs(lattice - np.round(lattice)).max() < 1e-5


# ------------------------------------------------------------------------------------ full size
def check_step_invariants(env, agent, steps, W, H, scale):
    """Size-independent properties of `steps` free-running steps (what replaces the oracle at full BASELINE sizes):
    occupancy, |move| = scale, reward == Σ Δagent_food, food bookkeeping, chem mass balance, ownership consistency."""
    from die_amd.device_array import unpermute
    K = env.agents.N
    obs = env._get_current_obs
    rewards = []
    for step in range(steps):
        food0 = env.medium.food.double().sum().item()
        af0 = env.agents.agent_food.double().sum().item()
        chem0 = env.medium.chem.double().sum().item()
        action = agent.forward(obs)
        obs, reward, term, _, info = env.step(action)
        rewards.append((reward, info['num_agents']))
        a = unpermute(action.data, action.slot).double()
        occ = env.medium.occupied()
        # every alive agent stands on an occupied cell; no more occupied cells than agents
        n_occ = int(occ.sum().item())
        assert 0.85 * K < n_occ <= K and info['num_agents'] == K and not term
        # move: |step| = scale for a normalised Physarum action
        assert torch.allclose(torch.hypot(a[0], a[1]), torch.full_like(a[0], scale), rtol=1e-4)
        # reward == Σ Δagent_food; food lost by the field == rate·Σ food over occupied cells (once per cell)
        af1 = env.agents.agent_food.double().sum().item()
        assert abs((af1 - af0) - reward) <= 1e-5 * abs(af0)
        food1 = env.medium.food.double().sum().item()
        lost = food0 - food1
        assert lost >= 0 and abs(lost - (env.medium.food.double() * occ).sum().item() * (0.1 / 0.9)) <= 1e-4 * food0
        # chem: Σ after = 0.9·(Σ before + Σ winner deposits); winners = owners of occupied cells
        owners = env.medium.owner_slots()[occ]
        dep = a[2][owners].sum().item()
        chem1 = env.medium.chem.double().sum().item()
        assert abs(chem1 - 0.9 * (chem0 + dep)) <= 1e-4 * max(chem1, 1.0)
    # owners are alive slots standing on their cell
    x, y = env.agents.q32_numpy()
    own = env.medium.owner_slots().cpu().numpy()
    ix = ((x.astype(np.uint64) * np.uint64(W - 1) + np.uint64(2 ** 31)) >> np.uint64(32)).astype(np.int64)
    iy = ((y.astype(np.uint64) * np.uint64(H - 1) + np.uint64(2 ** 31)) >> np.uint64(32)).astype(np.int64)
    assert (own[ix, iy] >= np.arange(K)).all()                 # the owner of my cell is me or a higher slot
    o = own[own >= 0]
    assert (ix[o] * H + iy[o] == np.nonzero(own.ravel() >= 0)[0]).all()
    return rewards


def test_full_size_properties_4096(die):
    """BASELINE config 3 (4096², ratio .15): size-independent invariants instead of the oracle."""
    W = H = 4096
    env = die.Env((W, H), die.Dynamics(init_agent_ratio=0.15), seed=1234, max_agents='alive')
    K = env.agents.N
    assert abs(K / (W * H) - 0.15) < 0.002
    agent = die.PhysarumAgent(max_agents=K, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1), seed=3)
    check_step_invariants(env, agent, 9, W, H, 1.53 / (W - 1))


def test_largest_baseline_grid_16384_f16_invariants(die):
    """BASELINE configs[4] grid: 16384² with fp16 field channels (268 M cells, ≈ 40 M agents) — maximum-size
    smoke test of the index arithmetic (int64 offsets, 29-bit slot field of the claim word) with the same
    size-independent invariants as at 4096²."""
    W = H = 16384
    env = die.Env((W, H), die.Dynamics(init_agent_ratio=0.15), seed=99, max_agents='alive', field_dtype=torch.float16,
                  sort_every=2)
    K = env.agents.N
    assert abs(K / (W * H) - 0.15) < 0.001 and K < 2 ** 29
    agent = die.PhysarumAgent(max_agents=K, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1), seed=3)
    obs = env._get_current_obs
    for step in range(3):
        af0 = env.agents.agent_food.double().sum().item()
        obs, reward, term, _, info = env.step(agent.forward(obs))
        assert info['num_agents'] == K and not term
        af1 = env.agents.agent_food.double().sum().item()
        assert abs((af1 - af0) - reward) <= 1e-5 * abs(af0)
        n_occ = int(env.medium.occupied().sum().item())
        assert 0.85 * K < n_occ <= K
    own = env.medium.owner_slots()
    assert int(own.max().item()) < K and int((own >= 0).sum().item()) == n_occ
    slots = own[own >= 0]
    assert slots.unique().numel() == slots.numel()              # every owner owns exactly one cell
    assert torch.isfinite(env.medium.chem.float()).all() and float(env.medium.chem.float().max()) > 0


def test_custom_food_flow_and_render(die):
    """Dynamics.op_food_flow as an arbitrary Python operator (core/env.py:147-150; the 'dyn-pred'
    dynamics of examples/simple_agents.py:95-100 use WaveSequence.get_flow_operator) runs through a
    host round trip; Env.render() returns the three frames of core/render.py:84-89."""
    W, H, N, K = 48, 36, 400, 300
    rs = np.random.RandomState(2)
    medium, agents = random_state(W, H, N, K, rs)
    wave = R.wave_field(W, H, 0.25)

    def flow(food):
        return 0.05 * np.abs(wave) + (1 - 0.5) * food            # scale·wave(t) + (1 − decay)·current

    dyn = die.Dynamics(op_food_flow=flow)
    rdyn = R.RefDynamics(op_food_flow=flow, rate_feed=float(np.float32(0.1)), rate_decay_chem=float(np.float32(0.1)))
    env, ref = die.Env.from_numpy(medium, agents, dyn), R.RefEnv(medium, agents, rdyn)
    for _ in range(3):
        action = quantised_action(N, rs, 2.0 / W)
        env.step(action)
        ref.step(action)
    m = env.medium.to_numpy()
    assert np.allclose(m[1], ref.medium[1], rtol=RTOL, atol=1e-7)
    assert np.allclose(m[2], ref.medium[2], rtol=RTOL, atol=1e-7)
    assert np.array_equal(m[0], ref.medium[0])
    frames = env.render()
    assert [f.shape for f in frames] == [(W, H, 3), (W, H, 4), (H, -(-N // H), 4)]
    assert np.array_equal(frames[0][..., 0], m[0]) and np.allclose(frames[0][..., 2], m[2])
    assert frames[2][..., 3].sum() == K


def test_device_render_matches_the_host_renderer(die):
    """Env.render() builds the frames of core/render.py:76-132 on the device (die_render_frames); the checker is the
    same renderer run on downloaded float64 arrays, as the reference does it, over several steps (the trace has state)."""
    from oracle.render_ref import EnvRenderer
    W, H, N, K = 40, 56, 700, 520
    rs = np.random.RandomState(4)
    medium, agents = random_state(W, H, N, K, rs)
    env = die.Env.from_numpy(medium, agents)
    host = EnvRenderer((W, H))
    for step in range(6):
        env.step(quantised_action(N, rs, 2.0 / W))
        frames = env.render()
        want = host.render(env.medium.to_numpy(), env.agents.to_numpy())
        assert [f.shape for f in frames] == [w.shape for w in want]
        assert np.array_equal(frames[0], want[0].astype(np.float32))                 # the three channels, bit for bit
        assert np.array_equal(frames[2], want[2].astype(np.float32))
        # trace image: fp32 vs float64 accumulation may pick the neighbouring colour of the 256-entry table
        assert np.abs(frames[1] - want[1]).max() < 0.02
        assert (np.abs(frames[1] - want[1]).max(axis=-1) > 1e-6).mean() < 0.01
    assert np.allclose(env._renderer._trace.cpu().numpy(), host._agent_trace.trace, rtol=1e-6, atol=1e-7)
    img = env.render_rgb8()
    assert img.dtype == np.uint8 and img.shape == (W, H, 3)
    m = env.medium.to_numpy()
    want8 = (np.clip(np.stack([m[0], m[1], m[2]], axis=-1), 0, 1).astype(np.float32) * np.float32(255) + np.float32(0.5)).astype(np.uint8)
    assert np.array_equal(img, want8)


@pytest.mark.parametrize('W,H', [(48, 48), (40, 64)])
def test_wave_sequence_food_flow_on_device(die, W, H):
    """WaveSequence.get_flow_operator (core/data_init.py:29-38,71-89; the 'dyn-pred' dynamics of
    examples/simple_agents.py:95-100) as a device kernel: the field itself and an env run that uses it as
    Dynamics.op_food_flow, against the oracle's restatement (pinned by the reference-made vectors in tests/golden)."""
    N, K = 500, 400
    seq = die.WaveSequence((W, H), dt=0.01)
    assert len(seq) == 1000 and 3.0 in seq and 10.0 not in seq
    for t in (0.0, 0.37, 9.99):
        assert np.abs(seq[t] - R.wave_field(W, H, t)).max() < 5e-7          # stored as fp32
    rs = np.random.RandomState(3)
    medium, agents = random_state(W, H, N, K, rs)
    ts = np.arange(0, 10, 0.01)
    calls = [0]

    def ref_flow(food):                                                     # scale·next(it) + (1 − decay)·current
        z = R.wave_field(W, H, ts[calls[0] % len(ts)])
        calls[0] += 1
        return 0.5 * z + (1 - 0.5) * food

    dyn = die.Dynamics(op_food_flow=seq.get_flow_operator(scale=0.5, decay=0.5))
    rdyn = R.RefDynamics(op_food_flow=ref_flow, rate_feed=float(np.float32(0.1)), rate_decay_chem=float(np.float32(0.1)))
    env, ref = die.Env.from_numpy(medium, agents, dyn), R.RefEnv(medium, agents, rdyn)
    for _ in range(4):
        action = quantised_action(N, rs, 2.0 / W)
        _, rew, *_ = env.step(action)
        _, rrew, *_ = ref.step(action)
        assert abs(rew - rrew) <= 1e-5 * max(1.0, abs(rrew))
    m = env.medium.to_numpy()
    assert np.allclose(m[1], ref.medium[1], rtol=RTOL, atol=2e-6)
    assert np.allclose(m[2], ref.medium[2], rtol=RTOL, atol=1e-7)
    assert np.array_equal(m[0], ref.medium[0])
    # the operator also accepts host arrays, as the reference's does
    op = seq.get_flow_operator(scale=2.0, decay=0.25)
    f0 = rs.rand(W, H)
    assert np.abs(op(f0) - (2.0 * R.wave_field(W, H, 0.0) + 0.75 * f0)).max() < 1e-6


@pytest.mark.parametrize('W,H', [(64, 48), (37, 91)])
def test_perlin_noise_sequence_food_flow_on_device(die, W, H):
    """PerlinNoiseSequence (core/data_init.py:55-69) as a FieldSequence whose flow operator runs on the device
    (die_food_flow_perlin): the field itself and an env run with it as Dynamics.op_food_flow, against the oracle's perlin3
    (values are rounded to 3 decimals: a value within 1e-9 of a .0005 tie may land on the other side — at most a few cells)."""
    seq = die.PerlinNoiseSequence((W, H), dt=0.05, octaves=8, seed=11)
    assert len(seq) == 20 and 0.5 in seq and 1.0 not in seq
    for t in (0.0, 0.35, 0.95):
        d = np.abs(seq[t] - R.perlin3_field(W, H, t, 8, 11))
        assert (d > 1e-6).mean() <= 2e-3 and d.max() <= 1.001e-3
    N, K = 500, 400
    rs = np.random.RandomState(3)
    medium, agents = random_state(W, H, N, K, rs)
    rseq = R.RefPerlinNoiseSequence((W, H), dt=0.05, t_bounds=(0, 1), octaves=8, seed=11)
    dyn = die.Dynamics(op_food_flow=seq.get_flow_operator(scale=0.5, decay=0.5))
    rdyn = R.RefDynamics(op_food_flow=rseq.get_flow_operator(scale=0.5, decay=0.5), rate_feed=float(np.float32(0.1)),
                         rate_decay_chem=float(np.float32(0.1)))
    env, ref = die.Env.from_numpy(medium, agents, dyn), R.RefEnv(medium, agents, rdyn)
    for _ in range(4):
        action = quantised_action(N, rs, 2.0 / W)
        env.step(action)
        ref.step(action)
    m = env.medium.to_numpy()
    d = np.abs(m[1] - ref.medium[1])
    assert (d > 2e-6).mean() <= 5e-3 and d.max() <= 1.1e-3              # (rounding ties of the noise, halved per step)
    assert np.array_equal(m[0], ref.medium[0])
    # a FieldSequence that only knows numpy goes through the host round trip
    class Ramp(die.FieldSequence):
        def __getitem__(self, t):
            return np.full(self._size, float(t))
    env2 = die.Env.from_numpy(medium, agents, die.Dynamics(op_food_flow=Ramp((W, H), dt=0.5, t_bounds=(1, 2)).get_flow_operator(1.0, 1.0)))
    env2.step(quantised_action(N, rs, 2.0 / W))
    f1 = env2.medium.to_numpy()[1]
    assert np.allclose(f1, 1.0, atol=1e-6)                               # food <- 1·field(t = 1) + 0·food (the flow comes after feeding)


def test_sense_mask_parity(die):
    """Dynamics.apply_sense_mask (core/env.py:276-295): the agents only see the medium within the blurred
    neighbourhood of the agents channel.  Mask plane bit for bit against the oracle (scipy gaussian, mode 'nearest',
    round(3), ceil), the masked observation, and forward() on it, over two env steps."""
    W, H, N, K = 96, 80, 120, 70
    rs = np.random.RandomState(12)
    medium, agents = random_state(W, H, N, K, rs)
    dyn = die.Dynamics(apply_sense_mask=True)
    rdyn = R.RefDynamics(apply_sense_mask=True, rate_feed=float(np.float32(0.1)), rate_decay_chem=float(np.float32(0.1)))
    env, ref = die.Env.from_numpy(medium, agents, dyn), R.RefEnv(medium, agents, rdyn)
    kw = dict(scale=0.01, deposit=4.5, inertia=0.9, sense_offset=0.05, noise_scale=0.0)
    prev = f32(rs.normal(0, .4, (2, N)))
    ragent = R.RefGradientAgent(N, init_noise=prev, seed=5, **kw)
    ragent._direction_rads = f32(ragent._direction_rads)
    agent = die.GradientAgent(max_agents=N, seed=5, **kw)
    agent.set_state(ragent._direction_rads.copy(), prev)
    for step in range(3):
        want_mask = ref.sense_mask().astype(bool)
        assert 0.2 < want_mask.mean() < 0.9                                   # the mask hides a real part of the field
        assert np.array_equal(env.medium.sense_mask.cpu().numpy().astype(bool), want_mask)
        seen = env.medium.observed_numpy()
        assert np.allclose(seen, ref.obs[1], rtol=RTOL, atol=1e-7) and (seen[2][~want_mask] == 0).all()
        # teacher forcing: both sides sense the device's (fp32) medium through the same mask
        robs = (env.agents.to_numpy(), np.where(want_mask, env.medium.to_numpy(), 0.))
        ragent._prev_grad = agent.prev_grad_numpy().astype(np.float64)
        ragent._direction_rads = agent.direction_rads_numpy().astype(np.float64)
        want = ragent.forward(robs)
        got = agent.forward(env._get_current_obs).to_numpy()
        assert np.allclose(got, want, rtol=RTOL, atol=2e-8)
        hidden_probe = ~want_mask[R.cell(robs[0][0] + 0.05 * np.cos(ragent._direction_rads), W),
                                  R.cell(robs[0][1] + 0.05 * np.sin(ragent._direction_rads), H)]
        action = quantised_action(N, rs, 2.0 / W)
        env.step(action)
        ref.medium, ref.agents = env.medium.to_numpy(), env.agents.to_numpy()    # keep the oracle on the device state
    assert hidden_probe.shape == (N,)


@pytest.mark.parametrize('kind,sort_every', [('physarum', 4), ('gradient', 3), ('physarum', 0)])
def test_graph_run_equals_step_loop(die, kind, sort_every):
    """Env.run: the forward + step loop captured as a hipGraph of K steps and replayed (Philox step counter from a
    device word) must leave exactly the state the step-by-step loop leaves, results included; also when plain steps
    and further runs follow."""
    W, H, N, K = 64, 48, 900, 700
    rs = np.random.RandomState(21)
    medium, agents = random_state(W, H, N, K, rs)
    if kind == 'physarum':
        mk = lambda: die.PhysarumAgent(max_agents=N, seed=3, scale=1.53 / (W - 1), sense_offset=6.2 / (W - 1), sense_angle=100)
    else:
        mk = lambda: die.GradientAgent(max_agents=N, seed=3, scale=0.01, sense_offset=0.03, inertia=0.9, noise_scale=0.025)
    turn = np.radians(30)
    dir0 = f32(np.floor(rs.uniform(-np.pi, np.pi, N) / turn) * turn)
    prev = f32(rs.normal(0, .4, (2, N)))
    envs, agts = [], []
    for _ in range(2):
        env = die.Env.from_numpy(medium, agents, sort_every=sort_every, sync=False)
        ag = mk()
        ag.set_state(dir0, prev if kind == 'gradient' else None)
        envs.append(env)
        agts.append(ag)
    period = envs[0]._graph_period()
    n1, n2, n3 = 2 * period + 9, 5, period + 3
    # A: run (graph), a few plain steps, run again;  B: the plain loop
    a_env, a_ag = envs[0], agts[0]
    r1 = a_env.run(a_ag, n1, graph=True)
    assert '_graphs' in a_env.__dict__ and len(a_env._graphs) == 1           # the graph path was taken
    obs = a_env._get_current_obs
    plain = []
    for _ in range(n2):
        obs, res, *_ = a_env.step(a_ag.forward(obs))
        plain.append(res.clone())
    r3 = a_env.run(a_ag, n3, graph=True)
    got_rew, got_alive = die.Env.read_results(torch.cat([r1, torch.stack(plain), r3]))
    b_env, b_ag = envs[1], agts[1]
    obs = b_env._get_current_obs
    want = []
    for _ in range(n1 + n2 + n3):
        obs, res, *_ = b_env.step(b_ag.forward(obs))
        want.append(b_env.read_result(res))
    want = np.array(want)
    assert np.array_equal(got_alive, want[:, 1].astype(np.int64))
    assert np.array_equal(got_rew, want[:, 0])
    assert np.array_equal(a_env.medium.to_numpy(), b_env.medium.to_numpy())
    assert np.array_equal(a_env.agents.to_numpy(), b_env.agents.to_numpy())
    assert np.array_equal(a_ag.direction_rads_numpy(), b_ag.direction_rads_numpy())
    if kind == 'gradient':
        assert np.array_equal(a_ag.prev_grad_numpy(), b_ag.prev_grad_numpy())
    assert a_env._steps == b_env._steps and a_ag._calls == b_ag._calls


@pytest.mark.parametrize('kind', ['physarum', 'gradient', 'physarum with dead slots'])
def test_run_of_tile_binned_steps_is_one_library_call(die, kind):
    """Env.run on a world that takes the tile-binned two-launch step: the steps are ONE call of die_pic_run (a C loop over
    die_pic_forward_env_step: layouts and chem planes exchange roles, the Philox step counter advances — SURVEY §8b's
    `die_step_fused(handle, n_steps)`) and leave exactly what the step-by-step loop leaves — odd and even counts, plain steps in
    between, an action handed out before a run and read after it, a GradientAgent's momentum state."""
    W, H, N = 192, 256, 9000
    rs = np.random.RandomState(33)
    medium, agents = random_state(W, H, N, N if 'dead' not in kind else 6000, rs, collide=0.3)      # (dead slots: the reference's default slot layout)
    if kind.startswith('physarum'):
        mk = lambda: die.PhysarumAgent(max_agents=N, seed=3, scale=1.53 / (H - 1), sense_offset=10.2 / (H - 1))
    else:
        mk = lambda: die.GradientAgent(max_agents=N, seed=3, scale=0.6 / (H - 1), sense_offset=10.2 / (H - 1), inertia=0.9, noise_scale=0.025)
    turn = np.radians(30)
    dir0 = f32(np.floor(rs.uniform(-np.pi, np.pi, N) / turn) * turn)
    prev = f32(rs.normal(0, .4, (2, N)))
    envs, agts = [], []
    for _ in range(2):
        env = die.Env.from_numpy(medium, agents, sort_every=0, sync=False, pic=True)
        env._pic_tile = (6, 6)
        ag = mk()
        ag.set_state(dir0, prev if kind == 'gradient' else None)
        envs.append(env)
        agts.append(ag)
    a_env, a_ag = envs[0], agts[0]
    obs = a_env._get_current_obs
    act0 = a_ag.forward(obs)                                   # handed out before the runs, read after them
    obs, res0, *_ = a_env.step(act0)
    r1 = a_env.run(a_ag, 7)
    assert a_env._pic is not None and a_env._pic.held[0] is a_env.agents.x and a_env._pic.steps_since_check >= 8
    from die_amd import _lib
    assert _lib.lib.die_pic_run_completed() == 7 and a_env._pic.run_done == 7      # (ABI 22: the steps the last die_pic_run of this thread had enqueued)
    obs = a_env._get_current_obs
    plain = []
    for _ in range(3):
        obs, res, *_ = a_env.step(a_ag.forward(obs))
        plain.append(res.clone())
    r3 = a_env.run(a_ag, 4)
    r4 = a_env.run(a_ag, 1)
    a_env.check()
    got_rew, got_alive = die.Env.read_results(torch.cat([res0[None], r1, torch.stack(plain), r3, r4]))
    b_env, b_ag = envs[1], agts[1]
    obs = b_env._get_current_obs
    want, b_act0 = [], None
    for i in range(1 + 7 + 3 + 4 + 1):
        act = b_ag.forward(obs)
        obs, res, *_ = b_env.step(act)
        if i == 0:
            b_act0 = act.to_numpy()
        want.append(b_env.read_result(res))
    want = np.array(want)
    assert np.array_equal(got_alive, want[:, 1].astype(np.int64)) and np.array_equal(got_rew, want[:, 0])
    assert np.array_equal(act0.to_numpy(), b_act0)
    assert np.array_equal(a_env.medium.to_numpy(), b_env.medium.to_numpy())
    assert np.array_equal(a_env.agents.to_numpy(), b_env.agents.to_numpy())
    assert np.array_equal(a_ag.direction_rads_numpy(), b_ag.direction_rads_numpy())
    if kind == 'gradient':
        assert np.array_equal(a_ag.prev_grad_numpy(), b_ag.prev_grad_numpy())
    assert a_env._steps == b_env._steps and a_ag._calls == b_ag._calls
    assert a_env.library_runs == 3                             # (every run was one die_pic_run call)


def test_minimal_run_example(die):
    """The port of the reference's examples/minimal_run.py runs end to end (both agents)."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'minimal_run.py')
    spec = importlib.util.spec_from_file_location('minimal_run', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    total, env = mod.run_minimal(die.BrownianAgent(move_scale=0.01, seed=1), agent_ratio=0.05, field_size=(64, 64), iters=20,
                                 seed=1)
    assert np.isfinite(total) and env._num_alive_agents > 50
    total, env = mod.run_minimal(die.PhysarumAgent(max_agents=64 * 64, scale=0.006, turn_angle=30, sense_offset=0.04, seed=1),
                                 agent_ratio=0.15, field_size=(64, 64), iters=20, seed=1)
    assert np.isfinite(total) and float(env.medium.chem.max()) > 0


def test_manual_step_of_the_example_equals_env_step(die):
    """examples/simple_agents.py `manual_step` (the reference's `_manual_step`, examples/simple_agents.py:14-30, written
    with the stage entry points) leaves the world exactly as `Env.step` does — also with a food-flow operator."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('simple_agents', os.path.join(root, 'examples', 'simple_agents.py'))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    W, H, N, K = 96, 64, 3000, 2200
    rs = np.random.RandomState(31)
    medium, agents = random_state(W, H, N, K, rs, collide=0.2)
    outs = []
    for manual in (False, True):
        flow = die.WaveSequence((W, H), dt=0.01).get_flow_operator(scale=0.5, decay=0.5)
        env = die.Env.from_numpy(medium, agents, die.Dynamics(op_food_flow=flow), sort_every=0)
        ag = die.PhysarumAgent(max_agents=N, seed=4, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
        obs = env._get_current_obs
        for _ in range(5):
            action = ag.forward(obs)
            obs = (ex.manual_step(env, action) if manual else env.step(action))[0]
        outs.append((env.medium.to_numpy(), env.agents.to_numpy(), ag.direction_rads_numpy()))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------ NeuralAutomataAgent sensing
@pytest.mark.parametrize('W,H', [(12, 12), (96, 96), (12, 8), (250, 132)])
@pytest.mark.parametrize('kernel_sizes', [(3,), (5,), (3, 3), (3, 5), (3, 5, 3), (7, 1)])
def test_neural_automata_forward_parity(die, W, H, kernel_sizes):
    """NeuralAutomataAgent.forward on the device (die_conv2d_circular per layer + die_gather_scale) against the oracle
    (float64; itself pinned to torch's Conv2d in tests/test_nca_cpu.py) and against the torch evaluation of the same
    model in fp32: the transformed medium and the action within 1e-5 (north-star tolerance; tanh output is O(1), so atol =
    1e-5 as well).  Field sizes and kernel stacks of the reference's own model tests (test/unit/agent.py:11,30-31)."""
    import torch as th
    N, K = max(W * H // 3, 8), max(W * H // 5, 4)
    rs = np.random.RandomState(W * 31 + H + len(kernel_sizes))
    medium, agents = random_state(W, H, N, K, rs, collide=0.2)
    th.manual_seed(W + H)
    for with_agents in (True, False):
        ag = die.NeuralAutomataAgent(scale=0.07, deposit=1.5, with_agent_channel=with_agents, kernel_sizes=kernel_sizes)
        ag.model.init_weights()
        env = die.Env.from_numpy(medium, agents)
        action = ag.forward(env._get_current_obs)
        ws = [k.weight.detach().numpy().astype(np.float64) for k in ag.model.conv_layers()]
        want_sense = R.nca_sense(medium, ws, with_agents)
        got_sense = ag._sense_output.cpu().numpy().astype(np.float64)
        assert np.allclose(got_sense, want_sense, rtol=RTOL, atol=1e-5)
        want = R.nca_forward((agents, medium), ws, 0.07, 1.5, with_agents)
        assert np.allclose(action.to_numpy(), want, rtol=RTOL, atol=1e-5)
        x = th.from_numpy((medium if with_agents else medium[1:]).astype(np.float32))[None]
        assert np.allclose(got_sense, ag.model.forward(x)[0].detach().numpy(), rtol=RTOL, atol=1e-5)
        assert ag.render()[0].shape == (W, H, 3)
        # the action drives an env step like any other
        env.step(action)


@pytest.mark.parametrize('boundary', ['zeros', 'reflect', 'replicate'])
@pytest.mark.parametrize('W,H,kernel_sizes', [(48, 40, (3, 5)), (250, 132, (7, 3)), (12, 8, (5,))])
def test_neural_automata_boundaries(die, boundary, W, H, kernel_sizes):
    """`ConvolutionModel(boundary=…)` (core/agent/evo.py:51,86: torch's padding_mode; the reference's default and its
    examples use 'circular') — die_conv2d with the other three modes against the oracle (itself checked against torch for
    every mode in tests/test_nca_cpu.py) and against the torch evaluation of the same model: 1e-5."""
    import torch as th
    N = max(W * H // 4, 8)
    rs = np.random.RandomState(W + H + len(boundary))
    medium, agents = random_state(W, H, N, N, rs, collide=0.2)
    th.manual_seed(W)
    ag = die.NeuralAutomataAgent(scale=0.07, deposit=1.5, kernel_sizes=kernel_sizes, boundary=boundary)
    ag.model.init_weights()
    env = die.Env.from_numpy(medium, agents)
    action = ag.forward(env._get_current_obs)
    ws = [k.weight.detach().numpy().astype(np.float64) for k in ag.model.conv_layers()]
    got_sense = ag._sense_output.cpu().numpy().astype(np.float64)
    assert np.allclose(got_sense, R.nca_sense(medium, ws, True, boundary), rtol=RTOL, atol=1e-5)
    assert np.allclose(action.to_numpy(), R.nca_forward((agents, medium), ws, 0.07, 1.5, True, boundary), rtol=RTOL, atol=1e-5)
    x = th.from_numpy(medium.astype(np.float32))[None]
    assert np.allclose(got_sense, ag.model.forward(x)[0].detach().numpy(), rtol=RTOL, atol=1e-5)


def test_neural_automata_weights_written_in_place_are_seen(die):
    """The evolution loop loads every candidate through `param.data.view(-1)[:] = …` (core/agent/evo.py is driven that way
    by evotorch's NEProblem, examples/learning_agents.py): neither `_version` nor `data_ptr()` of the weight changes, so a
    cache of the uploaded kernels keyed on them would serve the first candidate for ever.  The device forward
    must follow the weights: two forwards around an in-place write differ, and each matches the oracle for ITS weights."""
    import torch as th
    W, H, N = 48, 40, 500
    rs = np.random.RandomState(3)
    medium, agents = random_state(W, H, N, N, rs)
    th.manual_seed(5)
    ag = die.NeuralAutomataAgent(scale=0.07, deposit=1.5, kernel_sizes=(3, 3))
    ag.model.init_weights()
    env = die.Env.from_numpy(medium, agents)
    first = ag.forward(env._get_current_obs).to_numpy()
    keys = [(k.weight._version, k.weight.data_ptr()) for k in ag.model.conv_layers()]
    for k in ag.model.conv_layers():
        k.weight.data.view(-1)[:] = th.from_numpy(rs.normal(0, 0.3, k.weight.numel()).astype(np.float32))
    assert keys == [(k.weight._version, k.weight.data_ptr()) for k in ag.model.conv_layers()]      # (the write is invisible to such a key)
    second = ag.forward(env._get_current_obs).to_numpy()
    ws = [k.weight.detach().numpy().astype(np.float64) for k in ag.model.conv_layers()]
    assert np.allclose(second, R.nca_forward((agents, medium), ws, 0.07, 1.5, True), rtol=RTOL, atol=1e-5)
    assert not np.allclose(first, second, atol=1e-3)


def test_conv_stack_against_reference_made_vectors(die, golden_dir):
    """die_conv2d_circular on the inputs / weights of tests/golden/ref_helpers.npz against the outputs the REFERENCE'S
    ConvolutionModel produced for them (tests/golden/make_ref_helper_vectors.py): 1e-5."""
    import ctypes as C
    import os
    from die_amd import _lib
    from die_amd.device_array import stream_ptr
    G = np.load(os.path.join(golden_dir, 'ref_helpers.npz'))
    dev = torch.device('cuda:0')
    for ci in range(4):
        x = torch.from_numpy(G[f'nca{ci}_in'].astype(np.float32)).to(dev).contiguous()
        cin, W, H = x.shape
        planes = [x[c] for c in range(cin)]
        nw = int(G[f'nca{ci}_nw'])
        keep = [x]
        for li in range(nw):
            w = torch.from_numpy(G[f'nca{ci}_w{li}'].astype(np.float32)).to(dev).contiguous()
            cout, cin_w, k, _ = w.shape
            assert cin_w == len(planes)
            dst = torch.empty((cout, W, H), dtype=torch.float32, device=dev)
            cin_arr = (_lib.ConvPlane * cin_w)(*[_lib.ConvPlane(t.data_ptr(), _lib.DIE_PLANE_F32, 0) for t in planes])
            out_arr = (C.c_void_p * cout)(*[dst[o].data_ptr() for o in range(cout)])
            _lib.check(_lib.lib.die_conv2d_circular(W, H, cin_w, cin_arr, 1, cout, out_arr, k, w.data_ptr(), int(li == nw - 1),
                                                    stream_ptr(dev)), 'die_conv2d_circular')
            keep += [w, dst]
            planes = [dst[o] for o in range(cout)]
        got = torch.stack(planes).cpu().numpy()
        assert np.allclose(got, G[f'nca{ci}_out'], rtol=1e-5, atol=1e-5), ci


def test_neural_automata_on_f16_fields_and_after_binned_steps(die):
    """fp16 field planes are read directly; after tile-binned steps (claim plane not maintained) the 'agents' channel is
    rebuilt before it is sensed."""
    W, H, N = 128, 96, 4000
    rs = np.random.RandomState(5)
    medium, agents = random_state(W, H, N, N, rs)
    env = die.Env.from_numpy(medium, agents, field_dtype=torch.float16)
    env._pic_tile = (4, 5)                                       # (worlds this small take the classic step by default)
    phys = die.PhysarumAgent(max_agents=N, seed=1, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
    obs = env._get_current_obs
    for _ in range(3):
        obs, *_ = env.step(phys.forward(obs))
    assert env._pic is not None and env.medium.owner_stale is not None
    nca = die.NeuralAutomataAgent(kernel_sizes=(3, 3))
    nca.model.init_weights()
    action = nca.forward(obs)
    m, a = env.medium.to_numpy(), env.agents.to_numpy()
    ws = [k.weight.detach().numpy().astype(np.float64) for k in nca.model.conv_layers()]
    assert m[0].sum() > 0
    assert np.allclose(action.to_numpy(), R.nca_forward((a, m), ws), rtol=RTOL, atol=1e-5)


# ------------------------------------------------------------------------------------ reference-compat switches
@pytest.mark.parametrize('N,K', [(3000, 3000), (2500, 1800)])
def test_agents_die_reference_compat_mode(die, N, K):
    """Dynamics(agents_die=True, compat='reference'): what the reference really does once `_agent_lifecycle` has rebound
    `self.agents` (core/env.py:249) while the AgentIndexer still holds the old array (core/utils.py:22) — deposits, the
    agents channel and feeding stay at the positions of the first step's move, num_agents never drops, the agents the
    policy sees keep moving / starving / being zeroed.  Against the oracle's restatement of exactly that, several steps,
    with and without slots that were dead from the start; and the two modes must really differ."""
    W, H = 64, 48
    rs = np.random.RandomState(N)
    medium, agents = random_state(W, H, N, K, rs, collide=0.3)
    agents[3] = f32(agents[3] * 0.03)                         # little food: many starve within a few steps
    actions = [quantised_action(N, rs, 3.0 / W) for _ in range(5)]
    runs = {}
    for compat in ('reference', 'intended'):
        env = die.Env.from_numpy(medium, agents, die.Dynamics(agents_die=True, compat=compat))
        ref = R.RefEnv(medium, agents, R.RefDynamics(agents_die=True, compat=compat, rate_feed=float(np.float32(0.1)),
                                                     rate_decay_chem=float(np.float32(0.1))))
        infos = []
        for act in actions:
            _, rew, term, _, info = env.step(act)
            _, rrew, rterm, _, rinfo = ref.step(act)
            assert info['num_agents'] == rinfo['num_agents'] and term == rterm
            assert abs(rew - rrew) <= 1e-5 * np.abs(ref.last_gained).sum() + 1e-9
            infos.append(info['num_agents'])
        m, a = env.medium.to_numpy(), env.agents.to_numpy()
        assert np.array_equal(m[0], ref.medium[0])
        assert np.allclose(m[1], ref.medium[1], rtol=RTOL, atol=1e-8) and np.allclose(m[2], ref.medium[2], rtol=RTOL, atol=1e-7)
        assert np.array_equal(a[2], ref.agents[2]) and np.abs(a[:2] - ref.agents[:2]).max() <= 2.0 ** -31
        assert np.allclose(a[3], ref.agents[3], rtol=1e-5, atol=1e-7)
        runs[compat] = (infos, a[2].sum(), m[0].sum())
    assert runs['reference'][0] == [K] * 5                      # the stale indexer never sees a death
    assert runs['intended'][0][-1] < K and runs['reference'][1] < K        # … although agents do die in both
    assert runs['reference'][2] != runs['intended'][2]


def test_gradient_agent_render_is_the_gradient_field(die):
    """GradientAgent.render (core/agent/gradient.py:126-135): one white pixel before the first forward, then
    0.5·(stack(gx, gy, 0) + 1) of the normalised, clipped np.gradient field of the chem the last forward saw — also after
    the step that followed it."""
    W, H, N = 96, 64, 1500
    rs = np.random.RandomState(4)
    medium, agents = random_state(W, H, N, N, rs)
    env = die.Env.from_numpy(medium, agents)
    ag = die.PhysarumAgent(max_agents=N, seed=1, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
    assert ag.render()[0].shape == (1, 1, 3)
    obs = env._get_current_obs
    action = ag.forward(obs)
    g = R.gradient_field(medium[2])
    want = 0.5 * (np.stack([g[0], g[1], np.zeros_like(g[0])], axis=-1) + 1.)
    img = ag.render()[0]
    assert img.shape == (W, H, 3)
    bad = ~np.isclose(img, want, rtol=1e-5, atol=2e-6)
    assert bad.mean() < 1e-4                                   # cells whose norm sits on grad_clip in fp32 vs float64
    env.step(action)
    assert np.array_equal(ag.render()[0], img)                 # the fused step left the plane forward() saw untouched


# ------------------------------------------------------------------------------------ batched replicas
def test_batched_replicas_at_the_configs4_grid(die):
    """BASELINE configs[4]'s grid, 16384x16384 with fp16 field channels, as a BATCH of two replicas on one GPU: at this size
    BatchedEnv steps every replica with the tile-binned step on its own stream.  Size-independent invariants per replica
    (every agent alive, reward = change of the agents' food, one owner per occupied cell) and independence of the replicas
    (different seeds: different rewards)."""
    from die_amd.batch import BatchedEnv, BatchedPhysarumAgent
    W = H = 16384
    benv = BatchedEnv((W, H), die.Dynamics(init_agent_ratio=0.15), replicas=2, seed=11, field_dtype=torch.float16)
    assert benv.per_replica
    bag = BatchedPhysarumAgent(benv, seed=3, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
    af0 = [e.agents.agent_food.double().sum().item() for e in benv.envs]
    res = benv.run(bag, 3)
    rew, alive = BatchedEnv.read_results(res)
    for r, e in enumerate(benv.envs):
        K = e.agents.N
        assert abs(K / (W * H) - 0.15) < 0.001 and (alive[:, r] == K).all()
        assert e._pic is not None and e._pic.held[0] is e.agents.x, 'the tile-binned step did not run'
        e.check()
        af1 = e.agents.agent_food.double().sum().item()
        assert abs((af1 - af0[r]) - rew[:, r].sum()) <= 1e-5 * abs(af0[r])
        own = e.medium.owner_slots()
        n_occ = int((own >= 0).sum().item())
        assert 0.85 * K < n_occ <= K and int(own.max().item()) < K
        del own
        assert torch.isfinite(e.medium.chem.float()).all() and float(e.medium.chem.float().max()) > 0
    assert rew[-1, 0] != rew[-1, 1]


@pytest.mark.parametrize('W,H,R,f16,per_replica', [(64, 48, 5, False, False), (256, 128, 3, True, False), (192, 128, 3, False, True)])
def test_batched_replicas_equal_stand_alone_runs(die, W, H, R, f16, per_replica):
    """die_forward_env_step_batch: R replicas in one launch pair.  Replica r must be, bit for bit, the stand-alone
    Env(seed + r) driven by PhysarumAgent(seed + r): fields, agents, headings, rewards — across an epoch wrap of the
    claim plane (33 steps)."""
    from die_amd.batch import BatchedEnv, BatchedPhysarumAgent
    dt = torch.float16 if f16 else torch.float32
    kw = dict(scale=1.53 / (max(W, H) - 1), sense_offset=10.2 / (max(W, H) - 1))
    steps = 33
    # per_replica: the large-world regime (one Env per replica, each on its own stream) forced onto a small world
    benv = BatchedEnv((W, H), die.Dynamics(init_agent_ratio=0.15), replicas=R, seed=40, field_dtype=dt, per_replica=per_replica)
    assert benv.per_replica == per_replica
    bag = BatchedPhysarumAgent(benv, seed=7, **kw)
    res = benv.run(bag, steps)
    rew, alive = BatchedEnv.read_results(res)
    assert len(set(benv.n)) > 1                                   # replicas of different sizes share the launch
    for r in range(R):
        env = die.Env((W, H), die.Dynamics(init_agent_ratio=0.15), seed=40 + r, max_agents='alive', field_dtype=dt)
        ag = die.PhysarumAgent(max_agents=env.agents.N, seed=7 + r, **kw)
        obs = env._get_current_obs
        want = []
        for _ in range(steps):
            obs, rw, _, _, info = env.step(ag.forward(obs))
            want.append((rw, info['num_agents']))
        m, a = benv.replica_numpy(r)
        assert np.array_equal(m, env.medium.to_numpy()), r
        assert np.array_equal(a, env.agents.to_numpy()), r
        assert np.array_equal(bag.direction_rads_numpy(r), ag.direction_rads_numpy()), r
        assert np.array_equal(rew[:, r], np.array([w[0] for w in want])) and np.array_equal(alive[:, r], np.array([w[1] for w in want]))
