"""Signal channels on the device (die_signal.hip; NeuralAutomataAgent(signal_channels=K)): the update kernel against the numpy model
inside a derived bound, three replicas in one launch, one forward against torch, the loop over forward / step cycles link by link, a
hand-set policy that needs the channel, populations whose replica r is — field included — the stand-alone run of
`replica_agent(r)`, both searchers from a blank field every generation, populations taking turns, large worlds, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent
from die_amd.device_array import stream_ptr
from die_amd.search import CMAES, PGPE
from tests import memory_model as MM
from tests import signal_model as SM
from tests import stock_plane_model as S
from tests.test_gpu_memory import FLOW, REFERENCE_DYNAMICS, WIDE, _run_alone
from tests.test_gpu_stock import _medium, _world

pytestmark = pytest.mark.gpu

DEV = 'cuda'
RTOL = ATOL = 1e-5                   # tests/test_gpu_memory.py::test_one_forward_against_torch: `sense` against the torch model
GUARD = 8                            # fp32 words of NaN before, between and after the planes (a multiple of 4: 16-byte planes stay so)
NAN_BITS = MM.bits(np.float32('nan'))


def _bits(t):
    return MM.bits(t.cpu().numpy() if isinstance(t, torch.Tensor) else t)


def _guarded(planes, pad=GUARD):
    """(buffer, view): `planes` (n, W, H) as n planes of cells + pad words each, NaN in front of the first plane and in every gap."""
    n, W, H = planes.shape
    stride = W * H + pad
    buf = torch.full((pad + n * stride,), float('nan'), dtype=torch.float32, device=DEV)
    view = buf[pad:].view(n, stride)
    view[:, :W * H] = torch.from_numpy(np.ascontiguousarray(planes, dtype=np.float32)).to(DEV).view(n, W * H)
    return buf, view


def _gaps_untouched(buf, n, cells, pad=GUARD):
    host = _bits(buf)
    gaps = np.concatenate([host[:pad]] + [host[pad + k * (cells + pad) + cells:pad + (k + 1) * (cells + pad)] for k in range(n)])
    return gaps.size == (n + 1) * pad and (gaps == NAN_BITS).all()


def _signal_step(W, H, K, standing, epoch, emission, em_stride, field_in, field_out, field_stride, deposit, sigma, decay):
    _lib.check(_lib.lib.die_signal_step(C.byref(_medium(W, H)), standing.data_ptr(), epoch, K, emission.data_ptr(), em_stride, field_in.data_ptr(),
                                        field_out.data_ptr(), field_stride, deposit, sigma, decay, stream_ptr(field_out.device)), 'die_signal_step')


# ---------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize('K', SM.CHANNELS)
@pytest.mark.parametrize('sigma', SM.SIGMAS)
@pytest.mark.parametrize('W,H', SM.SHAPES)
def test_kernel_against_the_model(W, H, sigma, K):
    """|got - want| <= 1e-5 (1 - decay) G(|F + E|) + 1e-7 with `want` the float64 model and G the same gaussian: the project's fp32
    diffusion constants on the magnitude the summation error scales with (tests/signal_model.py `bound`: derived, not measured)."""
    epoch, cells = 9, W * H
    F, occ, planes = SM.case(W, H, K)
    rs = np.random.RandomState(W + H)
    standing = torch.from_numpy(SM.standing_words(occ, epoch, rs).view(np.int64)).to(DEV)
    em_buf, em = _guarded(planes)
    in_buf, fin = _guarded(F)
    out_buf, fout = _guarded(np.full((K, W, H), np.nan, dtype=np.float32))
    _signal_step(W, H, K, standing, epoch, em, cells + GUARD, fin, fout, cells + GUARD, SM.DEPOSIT, sigma, SM.DECAY)
    got = fout[:, :cells].reshape(K, W, H).cpu().numpy()
    assert not np.isnan(got).any()                                               # every cell of every output plane is written
    want = SM.update(F, occ, planes, SM.DEPOSIT, sigma, SM.DECAY)
    err, bound = np.abs(got.astype(np.float64) - want), SM.bound(F, occ, planes, SM.DEPOSIT, sigma, SM.DECAY)
    print(f'{W}x{H} sigma {sigma} K {K}: worst share of the bound {(err / bound).max():.4f}')
    assert (err <= bound).all(), (err / bound).max()
    assert _gaps_untouched(out_buf, K, cells) and _gaps_untouched(in_buf, K, cells) and _gaps_untouched(em_buf, K, cells)
    assert np.array_equal(_bits(fin[:, :cells]), MM.bits(F).reshape(K, cells))    # the input field is read, not written
    # the emission matters (the test would not see a kernel that forgot it) …
    assert (np.abs(got - SM.update(F, np.zeros_like(occ), planes, SM.DEPOSIT, sigma, SM.DECAY)) > 10 * bound).any()
    # … and read at another epoch nobody stands anywhere: unoccupied cells add exactly nothing, a field of zeros stays all +0.0
    _, zeros = _guarded(np.zeros((K, W, H), dtype=np.float32))                   # (the same stride as the output planes: one field_stride)
    fout.fill_(float('nan'))
    _signal_step(W, H, K, standing, epoch + 1, em, cells + GUARD, zeros, fout, cells + GUARD, SM.DEPOSIT, sigma, SM.DECAY)
    assert not _bits(fout[:, :cells]).any()


# ---------------------------------------------------------------------------------------------------- 2. three replicas
@pytest.mark.parametrize('sigma', [0.5, 1.5], ids=['row kernel', 'tile kernel'])
@pytest.mark.parametrize('pad', [0, 8, 6], ids=['dense', 'padded by 8', 'padded by 6'])
def test_three_replicas_in_one_launch_are_their_stand_alone_launches(pad, sigma):
    """Plane k of replica r at (k R + r) plane_stride.  Padded by 6 words the planes are no longer 16-byte aligned: both launches take
    the tile kernel.  Replica 2 has no occupied cell: it only diffuses — bit for bit die_diffuse_decay's result where that call runs
    the same kernel."""
    W, H, R, K, epoch = 20, 68, 3, 2, 31
    cells, ps = W * H, W * H + pad
    channels = 3 + K + 1                                                         # a replica stride above the planes that are read
    rs = np.random.RandomState(5 + pad)
    F = (rs.uniform(-2, 2, (K, R, W, H)) * (rs.rand(K, R, W, H) < 0.6)).astype(np.float32)
    sense = np.tanh(rs.randn(R, channels, W, H) * 2).astype(np.float32)
    occ = rs.rand(R, W, H) < 0.15
    occ[2] = False
    words = np.zeros((R, ps), dtype=np.uint64)
    for r in range(R):
        words[r, :cells] = SM.standing_words(occ[r], epoch, rs).reshape(-1)
    standing = torch.from_numpy(words.view(np.int64)).to(DEV)
    tsense = torch.from_numpy(sense).to(DEV)
    fin = torch.full((K, R, ps), float('nan'), dtype=torch.float32, device=DEV)
    fin[:, :, :cells] = torch.from_numpy(F).to(DEV).view(K, R, cells)
    fout = torch.full((K, R, ps), float('nan'), dtype=torch.float32, device=DEV)
    b = _lib.Batch(R, 0, ps, 10, 1, (C.c_int64 * 64)(*([10] * 64)))
    sp = stream_ptr(fout.device)
    _lib.check(_lib.lib.die_signal_step_batch(C.byref(_medium(W, H)), C.byref(b), standing.data_ptr(), epoch, K, tsense[0, 3].data_ptr(), cells,
                                              channels * cells, fin.data_ptr(), fout.data_ptr(), SM.DEPOSIT, sigma, SM.DECAY, sp),
               'die_signal_step_batch')
    got = _bits(fout)
    assert (got[:, :, cells:] == NAN_BITS).all() and not (got[:, :, :cells] == NAN_BITS).any()      # the gaps untouched, every cell written
    alone = torch.full((K, R, ps), float('nan'), dtype=torch.float32, device=DEV)
    for r in range(R):
        _signal_step(W, H, K, standing[r], epoch, tsense[r, 3], cells, fin[0, r], alone[0, r], R * ps, SM.DEPOSIT, sigma, SM.DECAY)
    assert np.array_equal(got, _bits(alone))
    for r in range(R):                                                           # … and both are the model's
        want = SM.update(F[:, r], occ[r], sense[r, 3:3 + K], SM.DEPOSIT, sigma, SM.DECAY)
        have = fout[:, r, :cells].reshape(K, W, H).cpu().numpy().astype(np.float64)
        assert (np.abs(have - want) <= SM.bound(F[:, r], occ[r], sense[r, 3:3 + K], SM.DEPOSIT, sigma, SM.DECAY)).all(), r
    plain = torch.empty((W, H), dtype=torch.float32, device=DEV)
    same_kernel = pad % 4 == 0 or sigma > 1.0                                    # (die_diffuse_decay sweeps rows wherever H % 4 == 0 and R <= 4)
    for k in range(K if same_kernel else 0):
        src = fin[k, 2, :cells].clone()                                          # (its own allocation: aligned whatever the pad)
        _lib.check(_lib.lib.die_diffuse_decay(src.data_ptr(), plain.data_ptr(), W, H, _lib.DIE_F32, sigma, SM.DECAY, sp), 'die_diffuse_decay')
        assert np.array_equal(_bits(plain).reshape(-1), got[k, 2, :cells]), k


# ---------------------------------------------------------------------------------------------------- 3. one forward
def _signal_agent(seed, K=2, M=0, **kw):
    torch.manual_seed(seed)
    ag = die.NeuralAutomataAgent(scale=0.01, deposit=2.0, signal_channels=K, memory_channels=M, signal_deposit=0.75, signal_sigma=0.8,
                                 signal_decay=0.05, **kw)
    ag.model.init_weights()
    return ag


def _model_planes(ag, env, field, mem):
    """The observation the torch model sees: the medium's planes, the field, the model's expand of `mem`, the model's stock plane."""
    m, a = env.medium.to_numpy(), env.agents.to_numpy()
    W, H = env.medium.W, env.medium.H
    parts = [m if 'agents' in ag.obs_channels else m[1:], field.astype(np.float64)]
    if ag.memory_channels:
        parts.append(MM.expand_of(W, H, a, mem).astype(np.float64))
    if ag.with_stock_channel:
        parts.append(S.stock_plane_of(W, H, a)[None].astype(np.float64))
    return np.concatenate(parts).astype(np.float32)


@pytest.mark.parametrize('M', [0, 2], ids=['no memory', 'memory'])
@pytest.mark.parametrize('stock', [False, True], ids=['no stock', 'stock'])
@pytest.mark.parametrize('f16', [False, True], ids=['fp32', 'fp16'])
def test_one_forward_against_torch(f16, stock, M):
    W, H, N, K = 24, 40, 200, 2
    rs = np.random.RandomState(3 + 2 * f16 + stock + 4 * M)
    medium, agents = _world(W, H, N, rs)
    env = die.Env.from_numpy(medium, agents, field_dtype=torch.float16 if f16 else torch.float32)
    ag = _signal_agent(5, K, M, kernel_sizes=[3, 3], hidden_channels=6, hidden_activation='tanh', with_stock_channel=stock)
    assert ag.obs_channels == ['agents', 'env_food', 'chem1', 'signal_0', 'signal_1'] + [f'memory_{j}' for j in range(M)] + \
        (['agent_food'] if stock else [])
    field = (rs.uniform(-1, 1, (K, W, H)) * (rs.rand(K, W, H) < 0.6)).astype(np.float32)
    mem = (rs.rand(M, N).astype(np.float32) - 0.5) * 2
    ag.signals = torch.from_numpy(field).to(env.device)
    if M:
        ag.memory = torch.from_numpy(mem).to(env.device)
    with torch.no_grad():
        want = ag.model.forward(torch.from_numpy(_model_planes(ag, env, field, mem))[None])[0].numpy()
    got = ag.sense(env.medium, env.agents).cpu().numpy().copy()
    assert got.shape == (3 + K + M, W, H) and np.allclose(got, want, rtol=RTOL, atol=ATOL)
    assert ag.signals.dtype == torch.float32 and np.array_equal(_bits(ag.signals), MM.bits(field))       # `sense` alone: pure in the field
    action = ag.forward(env._get_current_obs)
    sensed = action._keepalive.cpu().numpy()
    assert np.array_equal(sensed, got)                                           # the same launches: the same bits
    a = env.agents.to_numpy()
    occ = SM.occupancy_of(W, H, a)
    assert 0 < occ.sum() <= (a[2] > 0).sum() < N                                 # alive slots only, shared cells once
    deposit, sigma, decay = ag.signal_constants
    new = ag.signals.cpu().numpy().astype(np.float64)
    assert (np.abs(new - SM.update(field, occ, sensed[3:3 + K], deposit, sigma, decay)) <=
            SM.bound(field, occ, sensed[3:3 + K], deposit, sigma, decay)).all()
    if M:                                                                        # the memory rows follow the emissions
        assert np.array_equal(_bits(ag.memory), MM.bits(MM.gather_of(W, H, a, sensed[3 + K:])))
    assert np.array_equal(ag.render()[0], np.moveaxis(sensed[:3], 0, -1))        # render() keeps showing the first three planes


# ---------------------------------------------------------------------------------------------------- 4. the loop closes
def _standing_by_hand(env):
    """die_stock_plane on the agents as they stand now, at the medium's epoch, into a plane of this test's own."""
    medium, agents = env.medium, env.agents
    plane = torch.zeros((medium.W, medium.H), dtype=torch.int64, device=medium.device)
    m, a = medium.c_struct(need_owner=False), agents.c_struct()
    _lib.check(_lib.lib.die_stock_plane(C.byref(m), C.byref(a), medium.epoch, plane.data_ptr(), stream_ptr(medium.device)), 'die_stock_plane')
    return plane


def test_the_loop_closes_link_by_link():
    W, H, N, K = 24, 40, 300, 2
    rs = np.random.RandomState(8)
    medium, agents = _world(W, H, N, rs, alive_ratio=2.0)
    agents[3, ::3] = np.float32(1e-4)                                            # a third of them starve within a step or two
    medium[1] = 0.0
    env = die.Env.from_numpy(medium, agents, die.Dynamics(agents_die=True, food_infinite=False))
    ag = _signal_agent(9, K, kernel_sizes=[3, 3], hidden_channels=6, hidden_activation='tanh')
    deposit, sigma, decay = ag.signal_constants
    obs, alive_counts = env._get_current_obs, []
    for cycle in range(3):
        alive_counts.append(int((env.agents.to_numpy()[2] > 0).sum()))
        before = torch.zeros((K, W, H), dtype=torch.float32, device=env.device) if ag.signals is None else ag.signals.clone()
        action = ag.forward(obs)
        sensed = action._keepalive.clone()
        by_hand = torch.full((K, W, H), float('nan'), dtype=torch.float32, device=env.device)
        _lib.check(_lib.lib.die_signal_step(C.byref(env.medium.c_struct(need_owner=False)), _standing_by_hand(env).data_ptr(), env.medium.epoch,
                                            K, sensed[3].data_ptr(), W * H, before.data_ptr(), by_hand.data_ptr(), W * H, deposit, sigma, decay,
                                            stream_ptr(env.device)), 'die_signal_step')
        assert np.array_equal(_bits(ag.signals), _bits(by_hand)) and _bits(ag.signals).any(), cycle
        assert not np.array_equal(_bits(ag.signals), _bits(before)), cycle
        held = ag.signals.clone()
        again = ag.sense(env.medium, env.agents)                                 # `sense` alone leaves the field where it is
        assert np.array_equal(_bits(ag.signals), _bits(held)) and again.shape[0] == 3 + K, cycle
        obs, *_ = env.step(action)
    assert alive_counts[0] == N and alive_counts[-1] < alive_counts[0]           # somebody died on the way: dead slots stop emitting


# ---------------------------------------------------------------------------------------------------- 5. a policy that needs it
def _follower(signal_deposit, gain=200.0):
    """One 3 x 3 layer, K = 1: every occupied cell emits tanh(10) = 1, the deposit row is 0, dx and dy are `gain` times the field's
    central differences (cross-correlation: out[x] = sum_a w[a] in[x + a - 1])."""
    ag = die.NeuralAutomataAgent(scale=0.01, deposit=1.0, signal_channels=1, signal_deposit=signal_deposit, signal_sigma=1.0, signal_decay=0.1,
                                 kernel_sizes=[3])
    layer, = ag.model.conv_layers()
    assert ag.obs_channels == ['agents', 'env_food', 'chem1', 'signal_0'] and tuple(layer.weight.shape) == (4, 4, 3, 3)
    with torch.no_grad():
        layer.weight.zero_()
        layer.weight[0, 3, 2, 1], layer.weight[0, 3, 0, 1] = gain, -gain         # dx
        layer.weight[1, 3, 1, 2], layer.weight[1, 3, 1, 0] = gain, -gain         # dy
        layer.weight[3, 0, 1, 1] = 10.0                                          # the emission
    return ag


def test_a_hand_set_policy_follows_the_signal_and_does_not_without_it():
    W = H = 32
    runs = {}
    for signal_deposit in (1.0, 0.0):
        medium = np.zeros((3, W, H))
        agents = np.array([[10 / 31, 14 / 31], [16 / 31, 16 / 31], [1.0, 1.0], [1.0, 1.0]])      # four cells apart along x
        for n in range(2):
            medium[0, S.cell(S.q32_words(agents[0]), W)[n], S.cell(S.q32_words(agents[1]), H)[n]] = 1.0
        env = die.Env.from_numpy(medium, agents)
        ag = _follower(signal_deposit)
        start = env.agents.to_numpy()[:2].copy()
        obs, gaps, places = env._get_current_obs, [], []
        for step in range(4):
            obs, *_ = env.step(ag.forward(obs))
            a = env.agents.to_numpy()
            gaps.append(float(a[0, 1] - a[0, 0]) * (W - 1))
            places.append(a[:2].copy())
        runs[signal_deposit] = (start, gaps, places, ag.signals.cpu().numpy())
    start, gaps, places, field = runs[1.0]
    # the first forward senses a blank field; from the second on each agent climbs the other's signal (a numpy run of the model:
    # 4, 3.81, 3.23, 2.62 cells)
    assert np.array_equal(places[0], start) and abs(gaps[0] - 4.0) < 1e-6, gaps
    assert gaps[1] < gaps[0] and gaps[2] < gaps[1] and gaps[3] < gaps[2] and gaps[3] < 3.0, gaps
    assert all(abs(p[1] * (H - 1) - 16).max() < 0.05 for p in places) and field.max() > 0.1
    start, gaps, places, field = runs[0.0]
    assert all(np.array_equal(p, start) for p in places) and not field.any()      # the same weights, no channel: nobody moves


# ---------------------------------------------------------------------------------------------------- 6. populations
def _candidates(n, seed, K=2, M=0, scale=0.01, **kw):
    torch.manual_seed(seed)
    out = []
    for _ in range(n):
        ag = die.NeuralAutomataAgent(scale=scale, deposit=2.0, signal_channels=K, memory_channels=M, signal_sigma=0.8, signal_decay=0.05, **kw)
        ag.model.init_weights()
        out.append(ag)
    return out


def _assert_replica_is(benv, pop, r, env, ag, rew, alive, want_rew, want_alive):
    m, a = benv.replica_numpy(r)
    assert np.array_equal(m, env.medium.to_numpy()), r
    assert np.array_equal(a, env.agents.to_numpy()), r
    assert np.array_equal(rew[:, r], want_rew) and np.array_equal(alive[:, r], want_alive), r
    assert np.array_equal(pop.render(r), ag.render()[0]), r
    assert tuple(ag.signals.shape) == (pop._signal_channels, benv.W, benv.H) and _bits(ag.signals).any(), r
    assert np.array_equal(_bits(pop.signals[r]), _bits(ag.signals)), r
    if pop._memory_channels:
        assert np.array_equal(_bits(pop.memory[r, :, :benv.n[r]]), _bits(ag.memory)), r


DYN = lambda W, H: dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15)               # noqa: E731
POPULATIONS = {
    # E, model, memory channels, slots, reseed, Dynamics per replica (built anew for every Env), population arguments
    'plain': (1, WIDE, 0, 'alive', None, [DYN], {}),
    'episodes': (2, WIDE, 0, 'alive', None, [DYN], {}),
    'die_fixed_reseed': (1, WIDE, 0, 200, 31, [lambda W, H: dict(init_agent_ratio=0.15, agents_die=True, food_infinite=False)], {}),
    'flow': (1, WIDE, 0, 'alive', None, [lambda W, H: dict(init_agent_ratio=0.15, food_infinite=False, op_food_flow=FLOW(W, H))], {}),
    'dynamics_rows': (1, WIDE, 0, 'alive', None, [DYN, lambda W, H: dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15, diffuse_sigma=0.5,
                                                                       rate_decay_chem=0.05)], {}),
    'dropout': (1, dict(WIDE, p_agent_dropout=0.25), 0, 'alive', None, [DYN], dict(dropout_seed=1000, dropout_seed_stride=3)),
    'stock': (1, dict(WIDE, with_stock_channel=True, with_agent_channel=False), 0, 'alive', None,
              [lambda W, H: dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15, agents_die=True)], {}),
    'memory': (1, WIDE, 2, 'alive', None, [DYN], {}),
    'born': (1, WIDE, 0, 300, None, [lambda W, H: dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15, agents_die=True, agents_born=True)], {}),
}


@pytest.mark.parametrize('case', list(POPULATIONS))
def test_replica_is_the_stand_alone_agent_field_included(case):
    W, H, R, steps, K = 24, 40, 4, 3, 2
    E, model_kw, M, slots, reseed, dyn_kws, pop_kw = POPULATIONS[case]
    dyn = lambda r: die.Dynamics(**dyn_kws[r % len(dyn_kws)](W, H))               # noqa: E731
    cands = _candidates(R // E, W + R, K, M, **model_kw)
    benv = BatchedEnv((W, H), dyn(0) if len(dyn_kws) == 1 else [dyn(r) for r in range(R)], replicas=R, seed=11, max_agents=slots)
    pop = BatchedNeuralAutomataAgent.from_agents(benv, cands, E, **pop_kw)
    assert pop._signal_channels == K and tuple(pop.signals.shape) == (R, K, W, H) and not pop.signals.any()
    assert pop.P == sum(k.weight.numel() for k in cands[0].model.conv_layers())
    first_seed = 11
    if reseed is not None:
        benv.reset(seed=reseed)
        first_seed = reseed
    rew, alive = BatchedEnv.read_results(benv.run(pop, steps))
    for r in range(R):
        env = die.Env((W, H), dyn(r), seed=first_seed + r, max_agents=slots)
        ag = pop.replica_agent(r)
        assert ag.signal_channels == K and ag.signals is None and ag.memory_channels == M       # a blank field
        want_rew, want_alive = _run_alone(env, ag, steps)
        _assert_replica_is(benv, pop, r, env, ag, rew, alive, want_rew, want_alive)
    if E == 2:                                                                    # a field per replica, not per candidate
        assert not torch.equal(pop.signals[0], pop.signals[1])
    if case == 'die_fixed_reseed':
        assert all(benv.n[r] == 200 for r in range(R)) and (alive < 200).all()
    assert pop.candidate(0).signals is None and pop.reset.__func__ is BatchedNeuralAutomataAgent.reset_state
    pop.reset()
    assert not pop.signals.any() and (pop.memory is None or not pop.memory.any())


# ---------------------------------------------------------------------------------------------------- 7. search
@pytest.mark.parametrize('kind,R', [('pgpe', 4), ('cmaes', 5)])
def test_two_generations_of_search_score_every_candidate_from_a_blank_field(kind, R):
    W, H, T = 24, 40, 4
    template = _candidates(1, 0, 2, 0, **WIDE)[0]
    dyn = lambda: die.Dynamics(agents_die=True, **dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15))     # noqa: E731
    benv = BatchedEnv((W, H), dyn(), replicas=R, seeds=[9] * R)
    pop = BatchedNeuralAutomataAgent(benv, template)
    if kind == 'pgpe':
        s = PGPE(R, center_init=pop.parameters[0].cpu(), radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1,
                 optimizer_config=dict(max_speed=0.1, momentum=0.9), seed=11, device='cuda').for_population(pop, T)
    else:
        s = CMAES(R, center_init=pop.parameters[0].cpu(), stdev_init=0.1, seed=11, device='cuda').for_population(pop, T)
    assert s._pop_reset is not None and pop.memory is None                       # the hook exists with K > 0 alone
    for generation in range(2):
        s.step()
        assert pop.signals.any()                                                 # (what generation 2 must not start from)
        rows = pop.parameters.clone()
        fitness = s.fitness.cpu().tolist()
        for r in range(R):
            env = die.Env((W, H), dyn(), seed=9, max_agents='alive')
            ag = BatchedNeuralAutomataAgent.unpack(template, rows[r].cpu())
            assert ag.signals is None
            want_rew, _ = _run_alone(env, ag, T)
            assert fitness[r] == sum(want_rew.tolist()), (generation, r)


# ---------------------------------------------------------------------------------------------------- 8. taking turns
def test_signal_and_signal_less_populations_take_turns_on_one_batch():
    W, H, R = 24, 40, 3
    order = 'SPSSPPS'
    dyn = lambda: die.Dynamics(**dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15))   # noqa: E731
    with_signals = _candidates(R, 12, **WIDE)
    torch.manual_seed(13)
    plain = [die.NeuralAutomataAgent(scale=0.01, deposit=2.0, **WIDE) for _ in range(R)]
    for p in plain:
        p.model.init_weights()
    benv = BatchedEnv((W, H), dyn(), replicas=R, seed=21)
    pops = {'S': BatchedNeuralAutomataAgent.from_agents(benv, with_signals), 'P': BatchedNeuralAutomataAgent.from_agents(benv, plain)}
    assert getattr(pops['P'], 'reset', None) is None and pops['P'].signals is None and callable(pops['S'].reset)
    out = torch.stack([benv.step(pops[c]).clone() for c in order])
    rew, alive = BatchedEnv.read_results(out)
    for r in range(R):
        env = die.Env((W, H), dyn(), seed=21 + r, max_agents='alive')
        mine = {'S': pops['S'].replica_agent(r), 'P': pops['P'].replica_agent(r)}
        obs, want_rew, want_alive = env._get_current_obs, [], []
        for c in order:
            obs, rw, _, _, info = env.step(mine[c].forward(obs))
            want_rew.append(rw)
            want_alive.append(info['num_agents'])
        _assert_replica_is(benv, pops['S'], r, env, mine['S'], rew, alive, np.array(want_rew), np.array(want_alive))


# ---------------------------------------------------------------------------------------------------- 9. large worlds
def test_large_world_branch_keeps_a_field_per_stand_alone_agent():
    W, H, R, steps = 24, 40, 3, 4
    dyn = lambda: die.Dynamics(**dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15))   # noqa: E731
    cands = _candidates(R, 9, **WIDE)
    big, small = (BatchedEnv((W, H), dyn(), replicas=R, seed=4, per_replica=p) for p in (True, False))
    pb, ps = BatchedNeuralAutomataAgent.from_agents(big, cands), BatchedNeuralAutomataAgent.from_agents(small, cands)
    assert torch.equal(big.run(pb, steps), small.run(ps, steps)) and pb.signals is None
    for r in range(R):
        assert np.array_equal(_bits(pb.agents[r].signals), _bits(ps.signals[r])) and pb.agents[r].signals.any(), r
    assert not torch.equal(pb.agents[0].signals, pb.agents[1].signals)
    pb.reset()
    assert all(not ag.signals.any() for ag in pb.agents)


# ---------------------------------------------------------------------------------------------------- 10. refusals
def test_refusals_leave_signals_memory_dropout_step_and_the_world_untouched():
    W, H, N = 24, 40, 200
    rs = np.random.RandomState(10)
    medium, agents = _world(W, H, N, rs)
    env = die.Env.from_numpy(medium, agents)
    ag = _signal_agent(11, 2, 2, p_agent_dropout=0.25, dropout_seed=3, **WIDE)
    ag.forward(env._get_current_obs)
    field, held, step = ag.signals.clone(), ag.memory.clone(), ag.dropout_step
    world = [t.copy() for t in (env.medium.to_numpy(), env.agents.to_numpy())]
    for call in (lambda: ag.differentiable_sense(env.medium), lambda: ag.differentiable_action(env._get_current_obs),
                 lambda: ag.model.forward_device(torch.zeros((7, W, H), device=DEV)), lambda: ag.recurrent_action(env._get_current_obs)):
        with pytest.raises(NotImplementedError, match='signal'):
            call()
    other = die.Env.from_numpy(*_world(W, H + 4, N, rs))                          # a forward on a medium of another shape
    with pytest.raises(ValueError, match='reset_signals'):
        ag.forward(other._get_current_obs)
    with pytest.raises(ValueError, match='reset_signals'):
        ag.sense(other.medium, other.agents)

    def untouched(a, f, h, s):
        return torch.equal(a.signals.view(torch.int32), f.view(torch.int32)) and torch.equal(a.memory.view(torch.int32), h.view(torch.int32)) \
            and a.dropout_step == s

    assert untouched(ag, field, held, step) and step == 1
    assert all(np.array_equal(u, v) for u, v in zip(world, (env.medium.to_numpy(), env.agents.to_numpy())))
    ag.reset_signals()                                                            # … until reset_signals()
    assert not ag.signals.any()
    ag.forward(other._get_current_obs)
    assert tuple(ag.signals.shape) == (2, W, H + 4) and ag.signals.any()
    pop = BatchedNeuralAutomataAgent(BatchedEnv((W, H), die.Dynamics(init_agent_ratio=0.15), replicas=2, seed=1), ag, dropout_seed=3)
    pop.env.step(pop)
    field, held, step = pop.signals.clone(), pop.memory.clone(), pop.dropout_step
    before = [t.copy() for r in range(2) for t in pop.env.replica_numpy(r)]
    for call in (pop.differentiable_sense, pop.differentiable_action, pop.forward_device, pop.recurrent_action):
        with pytest.raises(NotImplementedError, match='signal'):
            call()
    assert untouched(pop, field, held, step) and step == 1
    assert all(np.array_equal(u, v) for u, v in zip(before, [t for r in range(2) for t in pop.env.replica_numpy(r)]))
