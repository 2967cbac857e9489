"""The kernels that produce what an agent or a viewer sees, over their argument domain (tests/observation_cases.py has the cases,
the inputs and the float64 models; tests/test_observation_cases_cpu.py holds the models against scipy, matplotlib and numpy and
shows that the cases tell every planted error from the true model).

    1  die_sense_mask against scipy, bit for bit: fields narrower than the radius, the rounding edges of the radius, every
       decimals value, stale claim words of other epochs in every empty cell, the second trip of the grid-stride loop; refusals
    2  the masked forward in every instantiation: `env.step(agent.forward(obs))` (k_forward_move_claim<T, KIND, true, LEAN>) against
       the materialised action (k_gradient_forward) on twin worlds, bit for bit; the oracle per kind; Env.run
    3  NeuralAutomataAgent under the mask against the oracle on the masked medium; the differentiable entries refuse a mask
    4  die_render_frames exactly: the colormap index over six table sizes, the trace update, rgb for both field types, every
       fp16 value through to_u8, fp32 values at its rounding edges, the pointer combinations, the grid-stride loop; refusals
    5  die_gradient_render on exactly representable fields: W = 2, H = 2, both field types, unnormalised, no clip, a clip with
       exact ties; refusals

Every device output is a slice of a larger buffer between two guard bands (a NaN of a payload no kernel produces for floats, 0xA5
for bytes): the bands must come back untouched and no sentinel may remain inside."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import cpu_ref as R                                                                  # noqa: E402
from tests import observation_cases as O                                                         # noqa: E402
from tests.test_gpu_parity import RTOL, f32, physarum_margins, random_state                      # noqa: E402

G = O.GUARD
SENTINEL = {torch.float32: (torch.int32, 0x7FC0A5A5), torch.float64: (torch.int64, 0x7FF8A5A5A5A5A5A5), torch.uint8: (torch.uint8, 0xA5)}


@pytest.fixture(scope='module')
def die():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import die_amd
    from die_amd import _lib
    assert (_lib.OWNER_EPOCH_SHIFT, _lib.OWNER_EPOCH_MAX, _lib.OWNER_SLOT_MASK) == (O.OWNER_EPOCH_SHIFT, O.OWNER_EPOCH_MAX, O.OWNER_SLOT_MASK)
    return die_amd


# ---------------------------------------------------------------------------------------------------------------- guarded buffers
def guarded(n, dtype, inner=None):
    """(buffer, view): n elements between two bands of G sentinels (64 floats: the view stays 16-byte aligned).  The inside starts
    as sentinels too (`inner`: another byte for uint8 outputs, where 0xA5 is a legitimate value)."""
    bits, s = SENTINEL[dtype]
    buf = torch.full((n + 2 * G,), s, dtype=bits, device='cuda')
    if inner is not None:
        buf[G:G + n] = inner
    buf = buf.view(dtype)
    view = buf[G:G + n]
    assert view.data_ptr() % 16 == 0
    return buf, view


def check_guard(buf, what='', written=True):
    """The bands are untouched; `written`: no sentinel is left inside — else: the inside is untouched as well.  Returns the inside
    (numpy)."""
    bits, s = SENTINEL[buf.dtype]
    raw = buf.view(bits).cpu().numpy()
    assert (raw[:G] == s).all(), ('the band before the output was written', what)
    assert (raw[-G:] == s).all(), ('the band after the output was written', what)
    inside = raw[G:-G]
    if written:
        assert not (inside == s).any(), ('cells of the output were never written', what)
    else:
        assert (inside == s).all(), ('a refused or unasked-for output was written', what)
    return buf.cpu().numpy()[G:-G]


def device_medium(words, epoch, dtype=torch.float32, food=None, chem=None):
    """A DeviceMedium whose claim plane holds the raw words at the given epoch."""
    from die_amd.device_array import DeviceMedium
    W, H = words.shape
    M = DeviceMedium((W, H), 'cuda', dtype)
    M.owner.copy_(torch.from_numpy(np.array(words)))
    M.epoch = epoch
    if food is not None:
        M.food.copy_(torch.from_numpy(np.array(food)))
    if chem is not None:
        M.chem.copy_(torch.from_numpy(np.array(chem)))
    return M


def refused(rc, entry):
    from die_amd import _lib
    assert rc != 0, entry
    assert _lib.lib.die_last_error().startswith(entry.encode() + b':'), _lib.lib.die_last_error()


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- 1. die_sense_mask
def sense_mask(M, sigma, decimals, mask=None, tmp=None, struct=None):
    """One call into guarded outputs; returns (rc, mask buffer, tmp buffer)."""
    from die_amd import _lib
    from die_amd.device_array import _ptr
    n = M.W * M.H
    mb, mv = guarded(n, torch.uint8)
    tb, tv = guarded(n, torch.float64)
    m = struct if struct is not None else M.c_struct()
    rc = _lib.lib.die_sense_mask(C.byref(m), sigma, decimals, _ptr(mv) if mask is None else mask[0], _ptr(tv) if tmp is None else tmp[0], None)
    return rc, mb, tb


def _check_sense_case(c):
    words = O.sense_inputs(c)
    W, H = c['shape']
    occ = O.occupied(words, c['epoch'])
    stale = words.view(np.uint64)[~occ]
    assert (stale != 0).all() and (stale.size > 0 or W * H <= 40)                # the case really holds stale non-zero words
    rc, mb, tb = sense_mask(device_medium(words, c['epoch']), c['sigma'], c['decimals'])
    assert rc == 0, O.sense_id(c)
    want, _ = O.sense_reference(words, c['epoch'], c['sigma'], c['decimals'])
    _, tmp = O.sense_model(words, c['epoch'], c['sigma'], c['decimals'])
    got = check_guard(mb, O.sense_id(c)).reshape(W, H)
    got_tmp = check_guard(tb, O.sense_id(c)).reshape(W, H)
    assert np.array_equal(got, want), (O.sense_id(c), int((got != want).sum()))
    assert np.abs(got_tmp - tmp).max() <= O.SM_TMP_TOL, O.sense_id(c)
    return stale.size


@pytest.mark.parametrize('shape', O.SM_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_sense_mask_is_scipys(die, shape):
    cases = [c for c in O.sense_cases() if c['shape'] == shape]
    assert len(cases) == len(O.SM_SIGMAS) * len(O.SM_DECIMALS)
    stale = sum(_check_sense_case(c) for c in cases)
    assert stale > 0 or shape == (1, 1)


def test_sense_mask_second_trip_of_the_grid_stride_loop(die):
    (c,) = [c for c in O.sense_cases() if c['shape'] == O.BIG_SHAPE]
    assert c['shape'][0] * c['shape'][1] > O.GRID_BLOCKS * O.BLOCK
    assert _check_sense_case(c) > 2_000_000


def test_sense_mask_refusals(die):
    from die_amd import _lib
    c = dict(shape=(5, 3), density=0.3, epoch=3, seed=1)
    words = O.sense_inputs(c)
    M = device_medium(words, 3)

    def bad(what, sigma=2.0, decimals=3, **kw):
        rc, mb, tb = sense_mask(M, sigma, decimals, **kw)
        refused(rc, 'die_sense_mask')
        check_guard(mb, what, written=False)
        check_guard(tb, what, written=False)

    for sigma in O.SM_BAD_SIGMAS:
        bad(('sigma', sigma), sigma=sigma)
    for d in O.SM_BAD_DECIMALS:
        bad(('decimals', d), decimals=d)
    for e in O.BAD_EPOCHS:
        m = M.c_struct()
        m.epoch = e
        bad(('epoch', e), struct=m)
    m = M.c_struct()
    m.gW, m.gH = 10, 6
    bad('a tile medium', struct=m)
    m = M.c_struct()
    m.owner = None
    bad('null owner', struct=m)
    bad('null mask_out', mask=(None,))
    bad('null tmp', tmp=(None,))
    rc, mb, tb = sense_mask(M, 2.0, 3)                                           # and the same medium is served when asked properly
    assert rc == 0 and np.array_equal(check_guard(mb).reshape(5, 3), O.sense_reference(words, 3, 2.0, 3)[0])
    assert _lib.OWNER_EPOCH_MAX + 1 in O.BAD_EPOCHS


# ---------------------------------------------------------------------------------------------------------------- 2. the masked forward
def _world(W, H, N, K, f16, seed):
    rs = np.random.RandomState(seed)
    medium, agents = random_state(W, H, N, K, rs)
    if f16:
        medium[1] = medium[1].astype(np.float16).astype(np.float64)
        medium[2] = medium[2].astype(np.float16).astype(np.float64)
    turn = np.radians(30)
    dir0 = f32(np.floor(rs.uniform(-np.pi, np.pi, N) / turn) * turn)
    prev = f32(rs.normal(0, .4, (2, N)))
    return medium, agents, dir0, prev


AGENTS = {
    'gradient-plain': ('gradient', dict(inertia=0.0, noise_scale=0.0)),
    'gradient-momentum': ('gradient', dict(inertia=0.9, noise_scale=0.025)),
    'physarum-lean': ('physarum', dict()),
    'physarum-momentum': ('physarum', dict(inertia=0.5, noise_scale=0.025)),       # fwd_is_lean: inertia and noise must be 0
}


def _agent(die, name, W, N, dir0, prev):
    kind, kw = AGENTS[name]
    if kind == 'gradient':
        ag = die.GradientAgent(max_agents=N, seed=5, scale=0.01, deposit=4.5, sense_offset=0.12, **kw)
    else:
        ag = die.PhysarumAgent(max_agents=N, seed=5, scale=1.53 / (W - 1), sense_offset=6.2 / (W - 1), sense_angle=100, **kw)
    ag.set_state(dir0, prev if kw.get('inertia') else None)
    return ag


def _state(env, ag):
    out = dict(medium=env.medium.to_numpy(), agents=env.agents.to_numpy(), headings=ag.direction_rads_numpy(),
               mask=env.medium.sense_mask.cpu().numpy())
    if ag._prev_grad is not None:
        out['prev_grad'] = ag.prev_grad_numpy()
    return out


def _probe_hidden(ag, agents, mask, W, H):
    d = ag.direction_rads_numpy()
    off = ag._sense_offset_scale
    return ~mask[R.cell(agents[0] + off * np.cos(d), W), R.cell(agents[1] + off * np.sin(d), H)]


@pytest.mark.parametrize('W,H,N,K', O.MASKED_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize('f16', [False, True], ids=['f32', 'f16'])
@pytest.mark.parametrize('name', list(AGENTS))
def test_masked_forward_fused_equals_materialised(die, name, f16, W, H, N, K):
    medium, agents, dir0, prev = _world(W, H, N, K, f16, seed=W + len(name))
    dt = torch.float16 if f16 else torch.float32
    dyn = lambda: die.Dynamics(apply_sense_mask=True)
    envs = [die.Env.from_numpy(medium, agents, dyn(), field_dtype=dt) for _ in range(2)]
    ags = [_agent(die, name, W, N, dir0, prev) for _ in range(2)]
    assert envs[0].medium.sense_mask is not None
    hidden_probes = 0
    for step in range(3):
        mask = envs[0].medium.sense_mask.cpu().numpy().astype(bool)
        assert 0.2 < mask.mean() < 0.9, mask.mean()                              # a real share of the cells is hidden
        assert np.array_equal(mask, O.env_mask(envs[0].medium.to_numpy()[0]))
        hidden_probes += int(_probe_hidden(ags[0], envs[0].agents.to_numpy(), mask, W, H).sum())
        # A: the pending action goes into the step (fused where the shape allows)
        act_a = ags[0].forward(envs[0]._get_current_obs)
        assert act_a.pending
        _, rew_a, *_ = envs[0].step(act_a)
        # B: the action is materialised first (the stand-alone forward), then stepped with
        act_b = ags[1].forward(envs[1]._get_current_obs)
        got_b = act_b.to_numpy()
        assert not act_b.pending
        _, rew_b, *_ = envs[1].step(act_b)
        assert np.array_equal(act_a.to_numpy(), got_b), (step, 'action')
        assert rew_a == rew_b, (step, 'reward')
        sa, sb = _state(envs[0], ags[0]), _state(envs[1], ags[1])
        assert sa.keys() == sb.keys() and ('prev_grad' in sa) == bool(AGENTS[name][1].get('inertia'))
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), (step, key)
    assert hidden_probes > 0                                                     # some probe fell on a hidden cell
    # the fused launch where H % 4 == 0; elsewhere the library refused it and the step fell back to two calls: the same bits
    assert envs[0]._fuse_forward == (H % 4 == 0)


@pytest.mark.parametrize('kind', ['gradient', 'physarum'])
def test_masked_forward_matches_the_oracle(die, kind):
    """Teacher-forced, as tests/test_gpu_parity.py::test_sense_mask_parity: both sides sense the device's medium through the
    oracle's mask; the oracle on the UNMASKED medium gives another action, so a kernel that ignores the mask fails."""
    W, H, N, K = O.MASKED_SHAPES[0]
    medium, agents, dir0, prev = _world(W, H, N, K, False, seed=7)
    env = die.Env.from_numpy(medium, agents, die.Dynamics(apply_sense_mask=True))
    sign = np.random.RandomState(1).randint(0, 2, N) * 2.0 - 1.0
    if kind == 'gradient':
        kw = dict(scale=0.01, deposit=4.5, inertia=0.9, sense_offset=0.12, noise_scale=0.0)
        ref, ag = R.RefGradientAgent(N, init_noise=prev, seed=5, **kw), die.GradientAgent(max_agents=N, seed=5, **kw)
        ag.set_state(dir0, prev)
    else:
        kw = dict(scale=1.53 / (W - 1), sense_offset=6.2 / (W - 1), sense_angle=100)
        ref, ag = R.RefPhysarumAgent(N, init_noise=np.ones((2, N)), **kw), die.PhysarumAgent(max_agents=N, **kw)
        ag.set_state(dir0)
        ag.set_turn_signs(sign)
    told_apart = 0
    for step in range(3):
        m, a = env.medium.to_numpy(), env.agents.to_numpy()
        mask = O.env_mask(m[0])
        assert 0.2 < mask.mean() < 0.9
        assert np.array_equal(env.medium.sense_mask.cpu().numpy().astype(bool), mask)
        d0 = ag.direction_rads_numpy().astype(np.float64)
        hidden = _probe_hidden(ag, a, mask, W, H)
        assert hidden.any()
        outs = []
        for seen in (np.where(mask, m, 0.), m):                                  # the masked observation, then the unmasked one
            ref._direction_rads = d0.copy()
            if kind == 'gradient':
                ref._prev_grad = ag.prev_grad_numpy().astype(np.float64)
                outs.append((ref.forward((a, seen)), ref._direction_rads.copy(), None))
            else:
                outs.append((ref.forward((a, seen), turn_sign=sign), ref._direction_rads.copy(), physarum_margins(ref, a, seen, d0, W, H)))
        (want, want_dir, margins), (other, _, _) = outs
        got = ag.forward(env._get_current_obs).to_numpy()
        if kind == 'gradient':
            assert np.allclose(got, want, rtol=RTOL, atol=2e-8)                  # test_sense_mask_parity's tolerances
            told_apart += int((np.abs(other - want) > 100 * (RTOL * np.abs(want) + 2e-8)).any(axis=0).sum())
        else:                                                                    # test_physarum_forward_parity's
            ddir = np.abs(R.renormalize_radians(ag.direction_rads_numpy() - want_dir))
            atol = 4e-7 * kw['scale']
            ok = (ddir < 1e-5) & np.isclose(got[0], want[0], rtol=RTOL, atol=atol) & np.isclose(got[1], want[1], rtol=RTOL, atol=atol) & \
                np.isclose(got[2], want[2], rtol=RTOL, atol=1e-9)
            assert (margins[~ok] < 1e-4).all() and (~ok).sum() <= 3, np.nonzero(~ok)[0]
            told_apart += int((np.abs(other - want) > 100 * (RTOL * np.abs(want) + atol)).any(axis=0).sum())
        env.step(got)
    assert told_apart > 0


@pytest.mark.parametrize('name', ['gradient-momentum', 'physarum-lean'])
def test_run_under_the_mask_equals_five_steps(die, name):
    W, H, N, K = O.MASKED_SHAPES[0]
    medium, agents, dir0, prev = _world(W, H, N, K, False, seed=11)
    envs = [die.Env.from_numpy(medium, agents, die.Dynamics(apply_sense_mask=True)) for _ in range(2)]
    ags = [_agent(die, name, W, N, dir0, prev) for _ in range(2)]
    res = envs[0].run(ags[0], 5)
    obs, want = envs[1]._get_current_obs, []
    for _ in range(5):
        obs, r, *_ = envs[1].step(ags[1].forward(obs))
        want.append(r)
    rew, alive = die.Env.read_results(res)
    assert np.array_equal(rew, np.array(want)) and (alive == K).all()
    sa, sb = _state(envs[0], ags[0]), _state(envs[1], ags[1])
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    assert 0.2 < sa['mask'].mean() < 0.9


# ---------------------------------------------------------------------------------------------------------------- 3. NeuralAutomataAgent
@pytest.mark.parametrize('f16', [False, True], ids=['f32', 'f16'])
@pytest.mark.parametrize('with_agents', [True, False], ids=['agents', 'no_agents'])
@pytest.mark.parametrize('kernel_sizes', [(3,), (3, 5)], ids=str)
def test_neural_automata_agent_senses_through_the_mask(die, kernel_sizes, with_agents, f16):
    """`sense` / `forward` read food and chem through `medium.sense_mask` (core/env.py:292-298).  Tolerances of
    tests/test_gpu_parity.py::test_neural_automata_forward_parity; the oracle on the unmasked medium lies more than 100 x that
    tolerance away somewhere, so an agent that senses the whole field fails."""
    W, H, N, K = O.NCA_SHAPE
    medium, agents, _, _ = _world(W, H, N, K, f16, seed=3 + len(kernel_sizes))
    torch.manual_seed(W + H)
    env = die.Env.from_numpy(medium, agents, die.Dynamics(apply_sense_mask=True), field_dtype=torch.float16 if f16 else torch.float32)
    ag = die.NeuralAutomataAgent(scale=0.07, deposit=1.5, with_agent_channel=with_agents, kernel_sizes=kernel_sizes)
    ag.model.init_weights()
    ws = [k.weight.detach().numpy().astype(np.float64) for k in ag.model.conv_layers()]
    for step in range(2):
        m, a = env.medium.to_numpy(), env.agents.to_numpy()
        mask = O.env_mask(m[0])
        assert 0.2 < mask.mean() < 0.9 and np.array_equal(env.medium.sense_mask.cpu().numpy().astype(bool), mask)
        seen = np.where(mask, m, 0.)
        action = ag.forward(env._get_current_obs)
        got_sense = ag._sense_output.cpu().numpy().astype(np.float64)
        got = action.to_numpy()
        want_sense, want = R.nca_sense(seen, ws, with_agents), R.nca_forward((a, seen), ws, 0.07, 1.5, with_agents)
        assert np.allclose(got_sense, want_sense, rtol=RTOL, atol=1e-5), step
        assert np.allclose(got, want, rtol=RTOL, atol=1e-5), step
        for w, other in ((want_sense, R.nca_sense(m, ws, with_agents)), (want, R.nca_forward((a, m), ws, 0.07, 1.5, with_agents))):
            assert (np.abs(other - w) > 100 * (RTOL * np.abs(w) + 1e-5)).any()
        assert np.array_equal(env.medium.to_numpy(), m)                          # the masked copies: the medium itself is untouched
        env.step(action)


@pytest.mark.parametrize('entry', ['differentiable_sense', 'differentiable_action', 'recurrent_action', 'signalling_action'])
def test_differentiable_entries_refuse_a_sense_mask(die, entry):
    W, H, N, K = O.NCA_SHAPE
    medium, agents, _, _ = _world(W, H, N, K, False, seed=5)
    env = die.Env.from_numpy(medium, agents, die.Dynamics(apply_sense_mask=True))
    kw = dict(recurrent_action=dict(memory_channels=2, hidden_channels=8), signalling_action=dict(signal_channels=2, hidden_channels=8)).get(entry, {})
    ag = die.NeuralAutomataAgent(scale=0.07, deposit=1.5, kernel_sizes=(3, 3), **kw)
    obs = env._get_current_obs
    with pytest.raises(NotImplementedError, match=f'{entry}: apply_sense_mask'):
        getattr(ag, entry)(obs[1] if entry == 'differentiable_sense' else obs)
    assert ag.memory is None and ag.signals is None and ag._sense_output is None and ag.dropout_step == 0      # nothing ran
    env.medium.sense_mask = None                                                 # the same call is served without the mask
    out = getattr(ag, entry)(obs[1] if entry == 'differentiable_sense' else obs)
    assert (out if isinstance(out, torch.Tensor) else out[0]).grad_fn is not None


# ---------------------------------------------------------------------------------------------------------------- 4. die_render_frames
def render(M, *, trace=None, decay=O.TRACE_DECAY, lut=None, lut_n=None, rgb=False, rgba=False, rgb8=False, struct=None, inner8=None,
           raw=None):
    """One call.  `trace`: a guarded (buffer, view) pair holding the state, or None.  Returns (rc, dict of guarded buffers)."""
    from die_amd import _lib
    from die_amd.device_array import _ptr
    n = M.W * M.H
    out = {}
    if rgb:
        out['rgb'] = guarded(3 * n, torch.float32)
    if rgba:
        out['rgba'] = guarded(4 * n, torch.float32)
    if rgb8:
        out['rgb8'] = guarded(3 * n, torch.uint8, inner8)
    ptr = {k: _ptr(v[1]) for k, v in out.items()}
    ptr.update(raw or {})
    m = struct if struct is not None else M.c_struct()
    rc = _lib.lib.die_render_frames(C.byref(m), _ptr(trace[1]) if trace is not None else None, decay, _ptr(lut) if lut is not None else None,
                                    (lut.shape[0] - 3 if lut is not None else 0) if lut_n is None else lut_n,
                                    ptr.get('rgb'), ptr.get('rgba'), ptr.get('rgb8'), None)
    return rc, {k: v[0] for k, v in out.items()}


def device_lut(N):
    """The table of N + 3 rows inside a guarded buffer of its own (16-byte aligned: the kernel reads float4 rows)."""
    lut = O.make_lut(N)
    buf, view = guarded(lut.size, torch.float32)
    view.copy_(torch.from_numpy(lut.reshape(-1)))
    return lut, view.view(N + 3, 4), buf


def trace_state(values):
    buf, view = guarded(values.size, torch.float32)
    view.copy_(torch.from_numpy(np.ascontiguousarray(values).reshape(-1)))
    return buf, view


def _same_bits_or_nan(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits32(got)[~nan], bits32(want)[~nan])


@pytest.mark.parametrize('N', O.LUT_SIZES)
def test_render_colormap_index_and_trace(die, N):
    W, H = O.RENDER_SHAPE
    lut, dlut, lbuf = device_lut(N)
    probes = O.trace_probes(N)
    rs = np.random.RandomState(N)
    # decay 1, nobody anywhere (every claim word stale): the trace keeps its bits — but for -0.0, which `+ 0.0` makes +0.0 —
    # and the image is the table row of the model's index, exactly
    nobody = np.zeros((W, H), dtype=bool)
    M = device_medium(O.claim_words(nobody, O.OWNER_EPOCH_MAX, rs), O.OWNER_EPOCH_MAX)
    tr = trace_state(probes)
    rc, out = render(M, trace=tr, decay=1.0, lut=dlut, rgba=True)
    assert rc == 0
    got_t = check_guard(tr[0], ('trace', N)).reshape(W, H)
    want_t = O.trace_step(probes, 1.0, nobody)[0]
    assert _same_bits_or_nan(got_t, want_t)
    negzero = (probes == 0) & np.signbit(probes)
    keep = ~np.isnan(probes) & ~negzero
    assert np.array_equal(bits32(got_t)[keep], bits32(probes)[keep]) and negzero.sum() == 1 and (bits32(got_t)[negzero] == 0).all()
    rgba = check_guard(out['rgba'], ('rgba', N)).reshape(W, H, 4)
    assert np.array_equal(bits32(rgba), bits32(lut[O.cmap_index(got_t, N)]))
    assert set(range(N + 3)) <= set(O.cmap_index(got_t, N).reshape(-1).tolist())              # every row was asked for
    # decay 0.875, a random crowd: trace * decay + occ rounded twice or (contracted) once; the image follows the trace WRITTEN
    occ = O.occupancy(W, H, 0.3, rs)
    M = device_medium(O.claim_words(occ, 1, rs), 1)
    tr = trace_state(probes)
    rc, out = render(M, trace=tr, decay=O.TRACE_DECAY, lut=dlut, rgba=True)
    assert rc == 0
    got_t = check_guard(tr[0], ('trace', N)).reshape(W, H)
    two, one = O.trace_step(probes, O.TRACE_DECAY, occ)
    nan = np.isnan(two)
    assert np.array_equal(np.isnan(got_t), nan)
    assert ((bits32(got_t) == bits32(two)) | (bits32(got_t) == bits32(one)))[~nan].all()
    rgba = check_guard(out['rgba'], ('rgba', N)).reshape(W, H, 4)
    assert np.array_equal(bits32(rgba), bits32(lut[O.cmap_index(got_t, N)]))
    check_guard(lbuf, 'the table')                                               # (read only: bands and rows as they were)
    assert np.array_equal(dlut.cpu().numpy(), lut)


@pytest.mark.parametrize('W,H', O.RENDER_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize('f16', [False, True], ids=['f32', 'f16'])
def test_render_rgb_is_the_medium(die, f16, W, H):
    npdt, dt = (np.float16, torch.float16) if f16 else (np.float32, torch.float32)
    for epoch in (1, O.OWNER_EPOCH_MAX):
        rs = np.random.RandomState(W * H + epoch)
        occ = O.occupancy(W, H, 0.3, rs)
        words = O.claim_words(occ, epoch, rs)
        food, chem = O.field_plane(W, H, npdt, rs), O.field_plane(W, H, npdt, rs)
        M = device_medium(words, epoch, dt, food, chem)
        rc, out = render(M, rgb=True)
        assert rc == 0
        rgb = check_guard(out['rgb'], (W, H, epoch)).reshape(W, H, 3)
        want = np.stack([occ.astype(np.float32), food.astype(np.float32), chem.astype(np.float32)], axis=-1)
        assert np.array_equal(rgb, want, equal_nan=True) and _same_bits_or_nan(rgb, want)
        assert W * H < 6 or np.isnan(want).any()


def test_render_rgb8_of_every_fp16_value(die):
    finite, rest = O.all_f16()
    W, H = finite.shape
    rs = np.random.RandomState(8)
    occ = O.occupancy(W, H, 0.3, rs)
    M = device_medium(O.claim_words(occ, 5, rs), 5, torch.float16, finite, rest)
    want = np.stack([O.to_u8_model(occ), O.to_u8_model(finite), O.to_u8_model(rest)], axis=-1)
    assert set(np.unique(want[..., 1]).tolist()) == set(range(256))
    for inner in (0xA5, 0x5A):                                                   # 0xA5 is a value of the image: two fills, one answer
        rc, out = render(M, rgb8=True, inner8=inner)
        assert rc == 0
        bits, s = SENTINEL[torch.uint8]
        raw = out['rgb8'].cpu().numpy()
        assert (raw[:G] == s).all() and (raw[-G:] == s).all()
        assert np.array_equal(raw[G:-G].reshape(W, H, 3), want), inner


def test_render_rgb8_of_fp32_values_at_the_rounding_edges(die):
    plane, either = O.u8_f32_inputs()
    W, H = plane.shape
    rs = np.random.RandomState(9)
    occ = O.occupancy(W, H, 0.3, rs)
    chem, either_c = plane[::-1, ::-1].copy(), either[::-1, ::-1]
    M = device_medium(O.claim_words(occ, 2, rs), 2, torch.float32, plane, chem)
    for inner in (0xA5, 0x5A):
        rc, out = render(M, rgb8=True, inner8=inner)
        assert rc == 0
        raw = out['rgb8'].cpu().numpy()
        assert (raw[:G] == 0xA5).all() and (raw[-G:] == 0xA5).all()
        got = raw[G:-G].reshape(W, H, 3)
        assert np.array_equal(got[..., 0], O.to_u8_model(occ))
        for ch, v, e in ((1, plane, either), (2, chem, either_c)):
            x = O.u8_exact(v)
            lo, hi = np.floor(x - O.U8_EITHER).astype(np.uint8), np.floor(x + O.U8_EITHER).astype(np.uint8)
            assert (lo != hi)[e].all()                                           # the planted cells have two answers, nobody else does:
            assert np.array_equal(got[..., ch][~e], O.to_u8_model(v)[~e])        # exact everywhere else (0.5 -> 128 included)
            assert ((got[..., ch] == lo) | (got[..., ch] == hi))[e].all()


def _render_world(W, H, seed, N=256):
    rs = np.random.RandomState(seed)
    occ = O.occupancy(W, H, 0.3, rs)
    food = rs.uniform(-0.2, 1.2, (W, H)).astype(np.float32)
    chem = rs.uniform(-0.2, 1.2, (W, H)).astype(np.float32)
    trace = rs.uniform(-0.1, 1.1, (W, H)).astype(np.float32)
    M = device_medium(O.claim_words(occ, 7, rs), 7, torch.float32, food, chem)
    return M, occ, food, chem, trace


def _check_frames(out, tr, occ, food, chem, trace, lut, N):
    """All three images and the trace of one call against the models."""
    W, H = occ.shape
    rgb = check_guard(out['rgb']).reshape(W, H, 3)
    assert np.array_equal(rgb, np.stack([occ.astype(np.float32), food, chem], axis=-1))
    raw8 = out['rgb8'].cpu().numpy()                                             # (filled 0x5A inside: 0xA5 is a value of the image)
    assert (raw8[:G] == 0xA5).all() and (raw8[-G:] == 0xA5).all()
    got8 = raw8[G:-G].reshape(W, H, 3)
    for ch, v in ((0, occ.astype(np.float32)), (1, food), (2, chem)):
        x = O.u8_exact(v)
        lo, hi = np.floor(x - O.U8_EITHER).astype(np.uint8), np.floor(x + O.U8_EITHER).astype(np.uint8)
        assert ((got8[..., ch] == lo) | (got8[..., ch] == hi)).all() and (lo != hi).mean() < 1e-3
    got_t = check_guard(tr[0]).reshape(W, H)
    two, one = O.trace_step(trace, O.TRACE_DECAY, occ)
    assert ((bits32(got_t) == bits32(two)) | (bits32(got_t) == bits32(one))).all()
    rgba = check_guard(out['rgba']).reshape(W, H, 4)
    assert np.array_equal(bits32(rgba), bits32(lut[O.cmap_index(got_t, N)]))


def test_render_pointer_combinations(die):
    W, H = O.RENDER_SHAPE
    M, occ, food, chem, trace = _render_world(W, H, 21)
    lut, dlut, _ = device_lut(256)
    # everything in one call
    tr_all = trace_state(trace)
    rc, all_ = render(M, trace=tr_all, lut=dlut, rgb=True, rgba=True, rgb8=True, inner8=0x5A)
    assert rc == 0
    _check_frames(all_, tr_all, occ, food, chem, trace, lut, 256)
    # rgb only: no trace, no table
    rc, a = render(M, rgb=True)
    assert rc == 0 and torch.equal(a['rgb'].view(torch.int32), all_['rgb'].view(torch.int32))
    # rgb8 only, trace NULL: the state keeps its bits
    tr = trace_state(trace)
    before = tr[0].clone()
    rc, b = render(M, rgb8=True, inner8=0x5A)
    assert rc == 0 and torch.equal(b['rgb8'], all_['rgb8']) and torch.equal(tr[0].view(torch.int32), before.view(torch.int32))
    # trace without an image: the state advances and nothing else is written (the table is not needed either)
    rgba_unasked = guarded(4 * W * H, torch.float32)
    rc, c = render(M, trace=tr, lut=None)
    assert rc == 0 and c == {} and torch.equal(tr[0].view(torch.int32), tr_all[0].view(torch.int32))
    check_guard(rgba_unasked[0], written=False)
    # trace + image from the same starting state: the image of the one call
    tr2 = trace_state(trace)
    rc, d = render(M, trace=tr2, lut=dlut, rgba=True)
    assert rc == 0 and torch.equal(d['rgba'].view(torch.int32), all_['rgba'].view(torch.int32))
    assert torch.equal(tr2[0].view(torch.int32), tr_all[0].view(torch.int32))


@pytest.mark.parametrize('W,H', [(1, 1), (5, 3), O.BIG_SHAPE], ids=lambda v: str(v))
def test_render_other_shapes(die, W, H):
    """One cell, an odd handful, and the shape above the grid cap (the second trip of the grid-stride loop), all outputs at once."""
    M, occ, food, chem, trace = _render_world(W, H, W + H)
    lut, dlut, _ = device_lut(256)
    tr = trace_state(trace)
    rc, out = render(M, trace=tr, lut=dlut, rgb=True, rgba=True, rgb8=True, inner8=0x5A)
    assert rc == 0
    _check_frames(out, tr, occ, food, chem, trace, lut, 256)


def test_render_refusals(die):
    W, H = 5, 3
    M, occ, food, chem, trace = _render_world(W, H, 4)
    lut, dlut, _ = device_lut(7)
    tr = trace_state(trace)
    before = tr[0].clone()

    def bad(what, **kw):
        rc, out = render(M, **kw)
        refused(rc, 'die_render_frames')
        for k, buf in out.items():
            check_guard(buf, (what, k), written=False)
        assert torch.equal(tr[0].view(torch.int32), before.view(torch.int32)), what

    bad('rgba without trace', lut=dlut, rgba=True)
    bad('rgba without a table', trace=tr, rgba=True)
    bad('rgba with lut_n = 0', trace=tr, lut=dlut, lut_n=0, rgba=True)
    for field, value in (('dtype', 2), ('dtype', -1), ('epoch', 0), ('epoch', O.OWNER_EPOCH_MAX + 1), ('owner', None), ('food', None),
                         ('chem', None)):
        m = M.c_struct()
        setattr(m, field, value)
        bad((field, value), struct=m, trace=tr, lut=dlut, rgb=True, rgba=True, rgb8=True)


# ---------------------------------------------------------------------------------------------------------------- 5. die_gradient_render
def gradient_render(chem, dtype, normalized, clip, W=None, H=None, raw_chem=False, raw_out=False, code=None):
    from die_amd import _lib
    from die_amd.device_array import _ptr
    src = torch.from_numpy(np.asarray(chem).astype(np.float16 if dtype == 'f16' else np.float32)).cuda()
    w, h = chem.shape
    buf, view = guarded(3 * w * h, torch.float32)
    rc = _lib.lib.die_gradient_render(None if raw_chem else _ptr(src), w if W is None else W, h if H is None else H,
                                      (_lib.DIE_F32 if dtype == 'f32' else _lib.DIE_F16) if code is None else code, int(normalized),
                                      -1.0 if clip is None else clip, None if raw_out else _ptr(view), None)
    return rc, buf


@pytest.mark.parametrize('W,H', O.GR_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
def test_gradient_render_is_the_gradient_field(die, dtype, W, H):
    chem, planted = O.gradient_chem(W, H)
    worst = 0.0
    for normalized in (True, False):
        for clip in O.GR_CLIPS:
            ties = O.gradient_ties(chem, clip)
            assert np.array_equal(ties, planted) if clip == 2.0 ** -11 else not ties.any()          # the condition on the inputs
            rc, buf = gradient_render(chem, dtype, normalized, clip)
            assert rc == 0
            got = check_guard(buf, (W, H, dtype, normalized, clip)).reshape(W, H, 3).astype(np.float64)
            want = O.gradient_image(chem, normalized, clip)
            err = np.abs(got - want).max()
            worst = max(worst, err)
            assert err <= O.GR_TOL, (normalized, clip, err)                      # every cell, none skipped
            assert (got[..., 2] == 0.5).all()
            if not normalized:
                assert np.array_equal(got, want)                                 # differences, halving, 0.5 (g + 1): exact in fp32
    print(f'gradient image {dtype} {W}x{H}: worst error {worst:.3g} (bound {O.GR_TOL:.3g})')


def test_gradient_render_refusals(die):
    chem, _ = O.gradient_chem(5, 3)
    for what, kw in (('W = 1', dict(W=1)), ('H = 1', dict(H=1)), ('W = 0', dict(W=0)), ('dtype 2', dict(code=2)), ('dtype -1', dict(code=-1)),
                     ('null chem', dict(raw_chem=True)), ('null rgb_out', dict(raw_out=True))):
        rc, buf = gradient_render(chem, 'f32', True, 1e-5, **kw)
        refused(rc, 'die_gradient_render')
        check_guard(buf, what, written=False)
