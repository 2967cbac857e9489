"""The gaussian diffusion over every radius, dtype, boundary mode and tiling edge (tests/diffuse_domain_cases.py has the shapes, the
inputs and the derivation of the two bounds; tests/test_diffuse_domain_cpu.py holds an fp32 emulation of the kernels against them).

    1  k_diffuse_rows<T, R, 0>  through die_diffuse_decay: fp32 / fp16, R = 1..4 (two sigmas on the rounding edge of the radius),
       fields with fewer rows than the radius, one exact strip, a strip of one output lane, a workgroup with an idle wave
    2  the same sweep with a ragged last wave at rows_per_wave 4, 8 and 16
    3  k_diffuse<T, R> through die_diffuse_decay_mode: fp32 / fp16, R = 1..8, five boundary modes, n == 1, fields narrower than the
       radius, exactly one 16 x 256 tile and one past it
    4  Env.step at R = 1 and 4 (k_diffuse_rows<T, R, 1>): the fused step, the staged step and the sweep alone give the same bits,
       and agree with the oracle's RefEnv
    5  BatchedEnv at four radii in one step (the table sweep, one launch per radius) and with shared Dynamics at R = 1 and 4 (the
       replica in gridDim.z): every replica is its stand-alone Env, bit for bit

Every dst is a slice of one larger buffer with 64 elements of NaN on either side: the bands must come back untouched and no NaN
may be left inside (the sweep writes 16-byte groups).  In 4 that is the step's `chem_next`; in 5 the R planes of the batch's
`chem_next`, one stride apart between the two bands (a store past one replica's plane lands in the next one's, which is compared
bit for bit with its twin).  The stand-alone twins of 5 step on their own planes: they are the reference there, and 4 guards them.

Not here: the adjoint (die_env_step_backward launches exactly 1 and 3 on the gradient plane — it has no kernel of its own to
instantiate), die_diffuse_decay_tile and the decomposed path."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import cpu_ref as R                                                                  # noqa: E402
from tests import diffuse_domain_cases as D                                                      # noqa: E402
from tests.test_gpu_batch_step_action import NAMES, batch_state, build, draw_actions, run_twins  # noqa: E402
from tests.test_gpu_parity import RTOL, quantised_action, random_state, ref_dyn                  # noqa: E402

WORST = {}                                 # group -> the worst error / bound seen (printed as the module ends)


@pytest.fixture(scope='module')
def die():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import die_amd
    yield die_amd
    for key, r in sorted(WORST.items()):
        print(f'diffuse domain, device: {key}: worst error / bound {r:.3f}')


def _torch_dtype(dtype):
    return {'f32': torch.float32, 'f16': torch.float16}[dtype]


def guarded(W, H, tdtype):
    """(buffer, plane): a (W, H) plane between two bands of D.GUARD NaNs (the plane starts 256 or 128 bytes into the buffer)."""
    buf = torch.full((W * H + 2 * D.GUARD,), float('nan'), dtype=tdtype, device='cuda')
    return buf, buf[D.GUARD:D.GUARD + W * H].view(W, H)


def check_guard(buf, what=''):
    """The bands are untouched and the plane holds no NaN; returns the plane's values as float64."""
    out = buf.cpu().to(torch.float64).numpy()
    assert np.isnan(out[:D.GUARD]).all(), ('the band before dst was written', what)
    assert np.isnan(out[-D.GUARD:]).all(), ('the band after dst was written', what)
    assert not np.isnan(out[D.GUARD:-D.GUARD]).any(), ('cells of dst were never written', what)
    return out[D.GUARD:-D.GUARD]


def diffuse(chem, sigma, mode, dtype, entry):
    """One direct call on the plane `chem` (numpy, the storage type) into a guarded dst."""
    from die_amd import _lib
    from die_amd.device_array import _ptr
    W, H = chem.shape
    src = torch.from_numpy(np.array(chem)).cuda()
    buf, dst = guarded(W, H, src.dtype)
    code = _lib.DIE_F32 if dtype == 'f32' else _lib.DIE_F16
    if entry == 'die_diffuse_decay':
        assert mode == 'wrap'
        rc = _lib.lib.die_diffuse_decay(_ptr(src), _ptr(dst), W, H, code, sigma, D.DECAY, None)
    else:
        rc = _lib.lib.die_diffuse_decay_mode(_ptr(src), _ptr(dst), W, H, code, sigma, D.DECAY, _lib.DIFFUSE_MODES[mode], None)
    _lib.check(rc, entry)
    return check_guard(buf, (entry, W, H, sigma, mode, dtype)).reshape(W, H)


def _note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)


# ---------------------------------------------------------------- 1. the row sweep, direct
@pytest.mark.parametrize('W,H', D.ROWS_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
def test_row_sweep_direct(die, dtype, W, H):
    worst = 0.0
    for scale in (1.0,) if dtype == 'f32' else D.F16_SCALES:
        for sigma in D.ROWS_SIGMAS:
            assert D.takes_row_sweep(W, H, sigma)
            chem, want = D.inputs(W, H, dtype, scale, sigma, 'wrap')
            got = diffuse(chem, sigma, 'wrap', dtype, 'die_diffuse_decay')
            r = D.ratio(got, want, dtype)
            print(f'rows {dtype} {W}x{H} sigma {sigma} (R = {D.radius(sigma)}) scale {scale:g}: error / bound {r:.3f}')
            worst = max(worst, r)
            assert r <= 1.0, (dtype, W, H, sigma, scale, r)
            if dtype == 'f32':                     # mass on the torus: sum(out) = (1 - decay) sum(in)
                assert np.isclose(got.sum(), float(np.float32(1.0 - float(np.float32(D.DECAY)))) * chem.astype(np.float64).sum(), rtol=1e-5)
    _note(f'1 rows direct {dtype}', worst)


# ---------------------------------------------------------------- 2. ragged rows at rows_per_wave 4, 8, 16
@pytest.mark.parametrize('W,H,rpw', D.RAGGED_SHAPES, ids=lambda v: str(v))
def test_row_sweep_ragged_rows(die, W, H, rpw):
    assert D.rows_per_wave(W, H) == rpw and W % rpw != 0 and D.takes_row_sweep(W, H, D.RAGGED_SIGMA)
    chem, want = D.inputs.__wrapped__(W, H, 'f32', 1.0, D.RAGGED_SIGMA, 'wrap')
    got = diffuse(chem, D.RAGGED_SIGMA, 'wrap', 'f32', 'die_diffuse_decay')
    r = D.ratio(got, want, 'f32')
    print(f'ragged f32 {W}x{H} rpw {rpw}: error / bound {r:.3f}')
    _note('2 rows ragged f32', r)
    assert r <= 1.0


# ---------------------------------------------------------------- 3. the LDS kernel, direct
def _lds_id(mode, shape):
    W, H = shape
    if (W, H) == (16, 256) and mode == 'wrap':
        return f'{mode}-{W}x{H}-lds_from_sigma_1.2_row_sweep_below'
    return f'{mode}-{W}x{H}-lds'


LDS_PARAMS = [pytest.param(mode, shape, id=_lds_id(mode, shape)) for mode in D.MODES for shape in D.LDS_SHAPES]


@pytest.mark.parametrize('mode,shape', LDS_PARAMS)
def test_lds_kernel_direct(die, mode, shape):
    W, H = shape
    worst, lds = 0.0, 0
    for dtype in ('f32', 'f16'):
        for scale in (1.0,) if dtype == 'f32' else D.F16_SCALES:
            for sigma in D.LDS_SIGMAS:
                lds += not D.takes_row_sweep(W, H, sigma, mode)
                chem, want = D.inputs(W, H, dtype, scale, sigma, mode)
                got = diffuse(chem, sigma, mode, dtype, 'die_diffuse_decay_mode')
                r = D.ratio(got, want, dtype)
                worst = max(worst, r)
                _note(f'3 lds direct {dtype} {mode}', r)
                assert r <= 1.0, (mode, W, H, dtype, sigma, scale, r)
    assert lds == (12 if (W, H) == (16, 256) and mode == 'wrap' else 24)          # R = 5..8 there, R = 1..8 elsewhere; x 3 planes
    print(f'lds {mode} {W}x{H}: worst error / bound {worst:.3f}')


# ---------------------------------------------------------------- 4. Env.step at R = 1 and 4
def _guard_next(env):
    """Replace the plane the step's sweep writes by a guarded one."""
    M = env.medium
    buf, M.chem_next = guarded(M.W, M.H, M.dtype)
    return buf


@pytest.mark.parametrize('W,H,N,K', D.STEP_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize('sigma', D.STEP_SIGMAS)
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
def test_env_step_at_radius_1_and_4(die, dtype, sigma, W, H, N, K):
    rs = np.random.RandomState(W + N + int(sigma * 100))
    medium, agents = random_state(W, H, N, K, rs)                      # finite food, forced collisions
    if dtype == 'f16':
        medium[1] = medium[1].astype(np.float16).astype(np.float64)
        medium[2] = medium[2].astype(np.float16).astype(np.float64)
    action = quantised_action(N, rs, 3.0 / W)
    dyn = die.Dynamics(diffuse_sigma=sigma)
    assert not dyn.food_infinite and D.takes_row_sweep(W, H, sigma)
    make = lambda: die.Env.from_numpy(medium, agents, dyn, sort_every=0, field_dtype=_torch_dtype(dtype))
    outs = []
    for form in ('step', 'staged', 'sweep'):
        env = make()
        buf = _guard_next(env)
        if form == 'step':
            env.step(action)
        else:
            act = die.DeviceAction.from_numpy(action, env.device)
            env.medium.next_epoch()
            env._stage('die_agent_move_claim', act)
            if form == 'staged':
                env._stage('die_agent_resolve', act)
                env._medium_diffuse_decay()
            else:
                env._medium_deposit_feed_diffuse()
        assert env.medium.chem.data_ptr() == buf.data_ptr() + D.GUARD * buf.element_size()      # the guarded plane is the new chem
        check_guard(buf, (form, dtype, sigma, W, H))
        outs.append((env.medium.to_numpy(), env.agents.to_numpy()))
    # the three forms of tests/test_gpu_parity.py test_fused_step_equals_staged_step: identical bits
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][0], outs[2][0])
    assert np.array_equal(outs[0][1], outs[1][1])                      # (with dead slots the sweep alone skips their feed pass)
    # ... and the oracle
    rd = ref_dyn(dyn)
    for f in ('rate_feed', 'rate_decay_chem', 'diffuse_sigma'):        # the C struct carries them as f32
        setattr(rd, f, float(np.float32(getattr(rd, f))))
    ref = R.RefEnv(medium, agents, rd)
    ref.step(action)
    m, a = outs[0]
    assert np.array_equal(a[:3], ref.agents[:3]) and np.array_equal(m[0], ref.medium[0])
    if dtype == 'f32':                                                 # test_env_step_parity's tolerances
        assert np.allclose(a[3], ref.agents[3], rtol=RTOL, atol=1e-7)
        assert np.allclose(m[1], ref.medium[1], rtol=RTOL, atol=1e-8)
        assert np.allclose(m[2], ref.medium[2], rtol=RTOL, atol=1e-7)
    else:                                                              # test_f16_field_channels_step_parity's: the deposit is rounded
        assert np.allclose(m[1], ref.medium[1], rtol=1e-3, atol=1e-4)  # into the plane before the filter — two roundings
        assert np.allclose(m[2], ref.medium[2], rtol=2e-3, atol=2e-4)
        assert np.allclose(a[3], ref.agents[3], rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------- 5. batched replicas
def _build_four_radii(die, f16):
    """build() of tests/test_gpu_batch_step_action.py for Dynamics that differ in diffuse_sigma only: one replica per radius."""
    from die_amd.batch import BatchedEnv
    W, H = D.BATCH_SHAPE
    dt = torch.float16 if f16 else torch.float32
    dyns = lambda: [die.Dynamics(diffuse_sigma=s, init_agent_ratio=0.15) for s in D.BATCH_SIGMAS]
    benv = BatchedEnv((W, H), dyns(), replicas=len(D.BATCH_SIGMAS), seed=3, field_dtype=dt, per_replica=False, max_agents='alive')
    twins = [die.Env((W, H), d, seed=benv.seeds[r], max_agents='alive', field_dtype=dt, device=benv.device, sort_every=0, pic=False,
                     sync=False) for r, d in enumerate(dyns())]
    assert [e.agents.N for e in twins] == benv.n and benv._rows is not None
    return benv, twins


def _batch_equals_twins(case, benv, twins, steps=2):
    actions = draw_actions(case, benv, steps)
    want, shared = run_twins(case, benv, twins, actions)
    assert all(shared), f'replicas without a shared cell and a loser: {[r for r, s in enumerate(shared) if not s]}'
    dev_actions = torch.from_numpy(actions).to(benv.device)
    for t in range(steps):
        # the R planes the sweep writes (one stride of W * H apart, as in the batch's own allocation) between two NaN bands
        buf, planes = guarded(benv.R * benv.W, benv.H, benv.dtype)
        benv.chem_next = planes.view(benv.R, benv.W, benv.H)
        res = benv.step_action(dev_actions[t])
        assert benv.chem.data_ptr() == planes.data_ptr()
        check_guard(buf, ('batch', t))
        for r in range(benv.R):
            w = want[r][t]
            assert torch.equal(res[r].view(torch.int64), w[0].view(torch.int64)), (t, r, 'result words')
            for what, got, exp in zip(NAMES, batch_state(benv, r), w[1:]):
                assert torch.equal(got, exp), (t, r, what)
            assert bool(torch.isfinite(benv.chem[r]).all()) and float(benv.chem[r].float().sum()) > 0
    for r, env in enumerate(twins):
        m, a = benv.replica_numpy(r)
        assert np.array_equal(m, env.medium.to_numpy()) and np.array_equal(a, env.agents.to_numpy()), r


@pytest.mark.parametrize('f16', [False, True], ids=['f32', 'f16'])
def test_batched_replicas_at_four_radii_in_one_step(die, f16):
    benv, twins = _build_four_radii(die, f16)
    assert [D.radius(benv.replica_dynamics(r).diffuse_sigma) for r in range(benv.R)] == [1, 2, 3, 4]
    _batch_equals_twins(dict(shape=D.BATCH_SHAPE, seed=3), benv, twins)


@pytest.mark.parametrize('sigma', D.STEP_SIGMAS)
@pytest.mark.parametrize('f16', [False, True], ids=['f32', 'f16'])
def test_batched_replicas_with_shared_dynamics_at_radius_1_and_4(die, f16, sigma):
    case = dict(shape=D.BATCH_SHAPE, R=4, sigma=sigma, f16=f16)
    benv, twins = build(case)
    assert benv._rows is None and D.radius(benv.dynamics.diffuse_sigma) == D.radius(sigma)
    _batch_equals_twins(case, benv, twins)
