"""Memory channels on the device (die_memory.hip; NeuralAutomataAgent(memory_channels=M)): the expand and the read-out against the
numpy model word for word, one forward against torch, the loop over forward / step cycles link by link, a hand-set recurrent
policy, populations whose replica r is — memory included — the stand-alone run of `replica_agent(r)`, both searchers from blank
memory every generation, re-sorted storage, and the refusals."""
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
from tests import stock_plane_model as S
from tests.test_gpu_stock import _crowd, _dev, _i32, _label, _medium, _upload, _world

pytestmark = pytest.mark.gpu

DEV = 'cuda'
RTOL = ATOL = 1e-5                   # tests/test_gpu_stock.py: the same comparison of `sense` against the torch model
REFERENCE_DYNAMICS = dict(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8)     # examples/learning_agents.py
PADS = ['circular', 'zeros', 'reflect', 'replicate']


def _bits(t):
    return MM.bits(t.cpu().numpy() if isinstance(t, torch.Tensor) else t)


def _memory_values(rs, M, N):
    """(M, N) float32 with a negative zero, a denormal and negative values among them."""
    mem = (rs.rand(M, N).astype(np.float32) - 0.5) * 2
    mem[:, 7], mem[:, 11] = np.float32(-0.0), np.float32(1e-41)
    return mem


def _standing(W, H, N, tx, ty, ta, tf, ts, epoch):
    plane = torch.zeros((W, H), dtype=torch.int64, device=DEV)
    a = _lib.Agents(N, tx.data_ptr(), ty.data_ptr(), ta.data_ptr(), tf.data_ptr(), None if ts is None else ts.data_ptr())
    _lib.check(_lib.lib.die_stock_plane(C.byref(_medium(W, H)), C.byref(a), epoch, plane.data_ptr(), stream_ptr(plane.device)), 'die_stock_plane')
    return plane


# ---------------------------------------------------------------------------------------------------- 1. the expand
@pytest.mark.parametrize('W,H', [(20, 68), (19, 70)], ids=['16-byte stores', 'word stores'])
def test_expand_is_the_model_word_for_word(W, H):
    """20 x 68 crosses the 16 x 64 tile in both axes and takes the 16-byte path; 19 x 70 (H % 4 != 0) the word path."""
    N, M, epoch = 300, 3, 7
    rs = np.random.RandomState(1)
    x, y, alive, food = _crowd(W, H, N, rs)
    mem = _memory_values(rs, M, N)
    occ, win = S.stock_winners(W, H, x, y, alive)
    mem[:, win[0, 0]], mem[0, win[W - 1, H - 1]] = np.float32(-0.0), np.float32(1e-41)      # … and among the winners
    perm = rs.permutation(N)
    standing = _standing(W, H, N, *_upload(x, y, alive, food, perm), epoch)
    tmem = torch.from_numpy(mem).to(DEV)
    planes = torch.full((M, W, H), float('nan'), dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib.die_memory_planes(C.byref(_medium(W, H)), standing.data_ptr(), epoch, M, tmem.data_ptr(), N, N, planes.data_ptr(), W * H,
                                          stream_ptr(planes.device)), 'die_memory_planes')
    want = MM.expand(W, H, x, y, alive, mem)
    assert np.array_equal(_bits(planes), MM.bits(want))
    assert _bits(planes)[0, 0, 0] == 0x80000000 and _bits(planes)[0, W - 1, H - 1] == MM.bits(np.float32(1e-41))
    assert occ.sum() < alive.sum() and (MM.bits(want)[:, ~occ] == 0).all()       # shared cells; every empty cell +0.0
    # read at another epoch nobody stands anywhere: every cell is written, with +0.0
    planes.fill_(float('nan'))
    _lib.check(_lib.lib.die_memory_planes(C.byref(_medium(W, H)), standing.data_ptr(), epoch + 1, M, tmem.data_ptr(), N, N, planes.data_ptr(),
                                          W * H, stream_ptr(planes.device)), 'die_memory_planes')
    assert not _bits(planes).any()


@pytest.mark.parametrize('pad', [16, 6], ids=['16-byte stores', 'word stores'])
def test_expand_of_three_replicas_in_one_launch(pad):
    W, H, stride, epoch, R, M = 20, 68, 300, 31, 3, 3
    n = [300, 123, 41]
    rs = np.random.RandomState(2)
    worlds, arrays = [], [np.zeros((R, stride), dtype=t) for t in (np.uint32, np.uint32, np.uint8, np.float32)]
    for r in range(R):
        x, y, alive, food = (v[:n[r]] for v in _crowd(W, H, stride, rs))
        worlds.append((x, y, alive))
        for dst, src in zip(arrays, (x, y, alive, food)):
            dst[r, :n[r]] = src
        # the padding slots n >= n[r]: alive and standing on a cell of their own — they must not appear
        arrays[0][r, n[r]:], arrays[1][r, n[r]:], arrays[2][r, n[r]:], arrays[3][r, n[r]:] = _label(7, W), _label(33, H), 1, 99.0
    tx, ty, ta, tf = _i32(arrays[0]), _i32(arrays[1]), _dev(arrays[2], torch.uint8), _dev(arrays[3], torch.float32)
    ps = W * H + pad
    standing = torch.zeros((R, ps), dtype=torch.int64, device=DEV)
    a = _lib.Agents(stride, tx.data_ptr(), ty.data_ptr(), ta.data_ptr(), tf.data_ptr(), None)
    b = _lib.Batch(R, 0, ps, stride, 1, (C.c_int64 * 64)(*n))
    sp = stream_ptr(standing.device)
    _lib.check(_lib.lib.die_stock_plane_batch(C.byref(_medium(W, H)), C.byref(a), C.byref(b), epoch, standing.data_ptr(), sp), 'die_stock_plane_batch')
    mem = np.stack([_memory_values(rs, M, stride) for _ in range(R)])             # (R, M, stride): the padding slots hold values too
    tmem = torch.from_numpy(mem).to(DEV)
    planes = torch.full((M, R, ps), float('nan'), dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib.die_memory_planes_batch(C.byref(_medium(W, H)), C.byref(b), standing.data_ptr(), epoch, M, tmem.data_ptr(), stride,
                                                planes.data_ptr(), sp), 'die_memory_planes_batch')
    got = _bits(planes)
    for r in range(R):
        want = MM.expand(W, H, *worlds[r], mem[r, :, :n[r]])
        assert np.array_equal(got[:, r, :W * H].reshape(M, W, H), MM.bits(want)), r
        assert (got[:, r, :W * H].reshape(M, W, H)[:, 7, 33] == MM.bits(want)[:, 7, 33]).all()      # (the padding slots' cell)
    assert (got[:, :, W * H:] == MM.bits(np.float32('nan'))).all()                # the gap between two planes stays untouched


# ---------------------------------------------------------------------------------------------------- 2. the read-out
@pytest.mark.parametrize('with_slots', [True, False], ids=['slot array', 'slot order'])
def test_read_out_is_the_model_word_for_word(with_slots):
    W, H, N, M = 20, 68, 300, 3
    rs = np.random.RandomState(3)
    x, y, alive, food = _crowd(W, H, N, rs)
    perm = rs.permutation(N) if with_slots else np.arange(N)
    tx, ty, ta, tf, ts = _upload(x, y, alive, food, perm)
    sense = (rs.rand(3 + M, W, H).astype(np.float32) - 0.5)
    sense[3, 0, 0], sense[4, W - 1, H - 1] = np.float32(-0.0), np.float32(1e-41)
    tsense = torch.from_numpy(sense).to(DEV)
    mem = torch.full((M, N), float('nan'), dtype=torch.float32, device=DEV)
    a = _lib.Agents(N, tx.data_ptr(), ty.data_ptr(), ta.data_ptr(), None, ts.data_ptr() if with_slots else None)
    _lib.check(_lib.lib.die_gather_memory(C.byref(_medium(W, H)), C.byref(a), M, tsense[3].data_ptr(), W * H, mem.data_ptr(), N,
                                          stream_ptr(mem.device)), 'die_gather_memory')
    want = MM.gather(W, H, x, y, alive, sense[3:])                                # by SLOT ID, whatever the storage order
    assert np.array_equal(_bits(mem), MM.bits(want))
    assert (_bits(mem)[:, alive == 0] == 0).all() and (alive == 0).sum() == N // 5   # dead slots: +0.0
    on_corner = (S.cell(x, W) == 0) & (S.cell(y, H) == 0) & (alive > 0)
    assert on_corner.sum() >= 3 and (_bits(mem)[0, on_corner] == 0x80000000).all()   # a shared cell: the same bits for all


def test_read_out_of_three_replicas_leaves_the_padding_slots_alone():
    W, H, stride, R, M = 20, 68, 300, 3, 2
    n = [300, 123, 41]
    rs = np.random.RandomState(4)
    worlds, arrays = [], [np.zeros((R, stride), dtype=t) for t in (np.uint32, np.uint32, np.uint8)]
    for r in range(R):
        x, y, alive, _ = (v[:n[r]] for v in _crowd(W, H, stride, rs))
        worlds.append((x, y, alive))
        for dst, src in zip(arrays, (x, y, alive)):
            dst[r, :n[r]] = src
        arrays[0][r, n[r]:], arrays[1][r, n[r]:], arrays[2][r, n[r]:] = _label(7, W), _label(33, H), 1
    tx, ty, ta = _i32(arrays[0]), _i32(arrays[1]), _dev(arrays[2], torch.uint8)
    channels = 3 + M + 1                                                          # a replica stride above the planes that are read
    sense = rs.rand(R, channels, W, H).astype(np.float32) - 0.5
    tsense = torch.from_numpy(sense).to(DEV)
    mem = torch.full((R, M, stride), float('nan'), dtype=torch.float32, device=DEV)
    a = _lib.Agents(stride, tx.data_ptr(), ty.data_ptr(), ta.data_ptr(), None, None)
    b = _lib.Batch(R, 0, W * H, stride, 1, (C.c_int64 * 64)(*n))
    _lib.check(_lib.lib.die_gather_memory_batch(C.byref(_medium(W, H)), C.byref(a), C.byref(b), M, tsense[0, 3].data_ptr(), W * H,
                                                channels * W * H, mem.data_ptr(), stride, stream_ptr(mem.device)), 'die_gather_memory_batch')
    got = _bits(mem)
    for r in range(R):
        assert np.array_equal(got[r, :, :n[r]], MM.bits(MM.gather(W, H, *worlds[r], sense[r, 3:3 + M]))), r
        assert (got[r, :, n[r]:] == MM.bits(np.float32('nan'))).all(), r


# ---------------------------------------------------------------------------------------------------- 3. one forward
def _memory_agent(seed, M=2, **kw):
    torch.manual_seed(seed)
    ag = die.NeuralAutomataAgent(scale=0.01, deposit=2.0, memory_channels=M, **kw)
    ag.model.init_weights()
    return ag


def _model_planes(ag, env, mem):
    """The observation the torch model sees: the medium's planes, the model's expand of `mem`, the model's stock plane."""
    m, a = env.medium.to_numpy(), env.agents.to_numpy()
    W, H = env.medium.W, env.medium.H
    parts = [m if 'agents' in ag.obs_channels else m[1:], MM.expand_of(W, H, a, mem).astype(np.float64)]
    if ag.with_stock_channel:
        parts.append(S.stock_plane_of(W, H, a)[None].astype(np.float64))
    return np.concatenate(parts).astype(np.float32)


@pytest.mark.parametrize('stock', [False, True], ids=['no stock', 'stock'])
@pytest.mark.parametrize('f16', [False, True], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('pad', PADS)
def test_one_forward_against_torch(pad, f16, stock):
    W, H, N, M = 24, 40, 300, 2
    rs = np.random.RandomState(len(pad) + 2 * f16 + stock)
    medium, agents = _world(W, H, N, rs)
    env = die.Env.from_numpy(medium, agents, field_dtype=torch.float16 if f16 else torch.float32)
    ag = _memory_agent(5, M, kernel_sizes=[3, 3], hidden_channels=6, hidden_activation='tanh', boundary=pad, with_stock_channel=stock)
    assert ag.obs_channels == ['agents', 'env_food', 'chem1', 'memory_0', 'memory_1'] + (['agent_food'] if stock else [])
    mem = _memory_values(rs, M, N)
    ag.memory = torch.from_numpy(mem).to(env.device)
    with torch.no_grad():
        want = ag.model.forward(torch.from_numpy(_model_planes(ag, env, mem))[None])[0].numpy()
    got = ag.sense(env.medium, env.agents).cpu().numpy().copy()
    assert got.shape == (3 + M, W, H) and np.allclose(got, want, rtol=RTOL, atol=ATOL)
    assert np.array_equal(_bits(ag.memory), MM.bits(mem))                        # `sense` alone leaves the memory as it is
    assert np.array_equal(_bits(ag.memory_planes(env.medium, env.agents)), MM.bits(MM.expand_of(W, H, env.agents.to_numpy(), mem)))
    action = ag.forward(env._get_current_obs)
    sensed = action._keepalive.cpu().numpy()
    assert np.array_equal(sensed, got)                                           # the same launches: the same bits
    assert np.array_equal(_bits(ag.memory), MM.bits(MM.gather_of(W, H, env.agents.to_numpy(), sensed[3:])))
    assert np.array_equal(ag.render()[0], np.moveaxis(sensed[:3], 0, -1))        # render() keeps showing the first three planes
    dead = env.agents.to_numpy()[2] == 0
    assert dead.any() and not _bits(ag.memory)[:, dead].any() and _bits(ag.memory)[:, ~dead].any()


# ---------------------------------------------------------------------------------------------------- 4. the loop closes
def test_the_loop_closes_link_by_link():
    W, H, N, M = 24, 40, 300, 3
    rs = np.random.RandomState(8)
    medium, agents = _world(W, H, N, rs, alive_ratio=2.0)
    agents[3, ::3] = np.float32(1e-4)                                            # a third of them starve within a step or two
    medium[1] = 0.0
    env = die.Env.from_numpy(medium, agents, die.Dynamics(agents_die=True, food_infinite=False))
    ag = _memory_agent(9, M, kernel_sizes=[3, 3], hidden_channels=6, hidden_activation='tanh')
    obs = env._get_current_obs
    alive_counts = []
    for cycle in range(4):
        before = env.agents.to_numpy()
        alive_counts.append(int((before[2] > 0).sum()))
        held = np.zeros((M, N), dtype=np.float32) if ag.memory is None else ag.memory.cpu().numpy().copy()
        # the planes the coming forward senses: the expand of the device's own memory under the positions and aliveness of now
        assert np.array_equal(_bits(ag.memory_planes(env.medium, env.agents)), MM.bits(MM.expand_of(W, H, before, held))), cycle
        action = ag.forward(obs)
        sensed = action._keepalive.cpu().numpy()
        got = ag.memory.cpu().numpy().copy()
        assert np.array_equal(MM.bits(got), MM.bits(MM.gather_of(W, H, before, sensed[3:]))), cycle
        assert not MM.bits(got)[:, before[2] == 0].any(), cycle                  # agents that died hold zero
        assert MM.bits(got)[:, before[2] > 0].any(), cycle
        obs, *_ = env.step(action)
    assert alive_counts[0] == N and alive_counts[-1] < alive_counts[0]           # somebody died on the way


# ---------------------------------------------------------------------------------------------------- 5. recurrence
def _flip_flop(a=1.0, b=4.0, c=3.0, e=0.5):
    """Two 1 x 1 layers, no hidden activation: memory' = tanh(a agents - b memory_0), dx = scale tanh(c memory_0 + e agents)."""
    ag = die.NeuralAutomataAgent(scale=0.01, deposit=1.0, memory_channels=1, kernel_sizes=[1, 1])
    l0, l1 = ag.model.conv_layers()
    assert ag.obs_channels == ['agents', 'env_food', 'chem1', 'memory_0'] and tuple(l1.weight.shape) == (4, 4, 1, 1)
    with torch.no_grad():
        l0.weight.copy_(torch.eye(4).reshape(4, 4, 1, 1))
        l1.weight.zero_()
        l1.weight[0, 3], l1.weight[0, 0] = c, e                                  # dx
        l1.weight[3, 0], l1.weight[3, 3] = a, -b                                 # the new memory
    return ag


def _one_agent_world():
    W = H = 16
    medium = np.zeros((3, W, H))
    agents = np.array([[0.5], [0.5], [1.0], [1.0]])
    medium[0, S.cell(S.q32_words(agents[0]), W)[0], S.cell(S.q32_words(agents[1]), H)[0]] = 1.0
    return die.Env.from_numpy(medium, agents)


def test_a_hand_set_policy_alternates_and_does_not_without_its_memory():
    runs = {}
    for blank in (False, True):
        env, ag = _one_agent_world(), _flip_flop()
        obs, mems, dxs = env._get_current_obs, [], []
        for step in range(6):
            if blank:
                ag.reset_memory()
            action = ag.forward(obs)
            mems.append(float(ag.memory[0, 0]))
            dxs.append(float(action.to_numpy()[0, 0]))
            obs, *_ = env.step(action)
        runs[blank] = (mems, dxs)
    mems, dxs = runs[False]
    assert [m > 0 for m in mems] == [True, False, True, False, True, False] and min(abs(m) for m in mems) > 0.5
    assert [d > 0 for d in dxs[1:]] == [True, False, True, False, True] and min(abs(d) for d in dxs) > 1e-3
    mems, dxs = runs[True]
    assert len(set(dxs)) == 1 and dxs[0] > 0 and len(set(mems)) == 1               # from blank memory: the same every step


# ---------------------------------------------------------------------------------------------------- 6. populations
def _run_alone(env, ag, steps):
    obs, rew, alive = env._get_current_obs, [], []
    for _ in range(steps):
        obs, rw, _, _, info = env.step(ag.forward(obs))
        rew.append(rw)
        alive.append(info['num_agents'])
    return np.array(rew), np.array(alive)


def _candidates(n, seed, M=2, scale=0.01, **kw):
    torch.manual_seed(seed)
    out = []
    for _ in range(n):
        ag = die.NeuralAutomataAgent(scale=scale, deposit=2.0, memory_channels=M, **kw)
        ag.model.init_weights()
        out.append(ag)
    return out


def _assert_replica_is(benv, pop, r, env, ag, rew, alive, want_rew, want_alive):
    m, a = benv.replica_numpy(r)
    assert np.array_equal(m, env.medium.to_numpy()), r
    assert np.array_equal(a, env.agents.to_numpy()), r
    assert np.array_equal(rew[:, r], want_rew) and np.array_equal(alive[:, r], want_alive), r
    assert np.array_equal(pop.render(r), ag.render()[0]), r
    n = benv.n[r]
    assert tuple(ag.memory.shape) == (pop._memory_channels, n) and _bits(ag.memory).any(), r
    assert np.array_equal(_bits(pop.memory[r, :, :n]), _bits(ag.memory)), r
    assert not _bits(pop.memory[r, :, n:]).any(), r                              # the padding slots were never written


WIDE = dict(kernel_sizes=(3, 3), hidden_channels=6, hidden_activation='tanh')
FLOW = lambda W, H: die.WaveSequence((W, H), dt=0.01).get_flow_operator(scale=0.5, decay=0.5)     # noqa: E731
POPULATIONS = {
    # steps, E, model, slots, Dynamics per replica (built anew for every Env), population arguments
    'plain': (6, 1, WIDE, 'alive', [lambda W, H: dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15)], {}),
    'die_fixed_flow': (6, 1, WIDE, 200, [lambda W, H: dict(init_agent_ratio=0.15, agents_die=True, food_infinite=False,
                                                          op_food_flow=FLOW(W, H))], {}),
    'episodes': (6, 2, WIDE, 'alive', [lambda W, H: dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15)], {}),
    'dropout': (6, 1, dict(WIDE, p_agent_dropout=0.25), 'alive', [lambda W, H: dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15)],
                dict(dropout_seed=1000, dropout_seed_stride=1)),
    'stock': (6, 1, dict(WIDE, with_stock_channel=True, with_agent_channel=False), 'alive',
              [lambda W, H: dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15, agents_die=True)], {}),
    'dynamics_rows': (6, 1, WIDE, 'alive', [lambda W, H: dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15),
                                            lambda W, H: dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15, diffuse_sigma=0.5, rate_decay_chem=0.05)], {}),
    'single_layer': (6, 1, dict(kernel_sizes=(5,), boundary='zeros'), 'alive', [lambda W, H: dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15)], {}),
    # 33 steps: the epoch wraps once, and the standing planes are cleared with the claim planes
    'epoch_wrap': (33, 1, dict(WIDE, with_stock_channel=True), 'alive', [lambda W, H: dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15)], {}),
}


@pytest.mark.parametrize('case', list(POPULATIONS))
def test_replica_is_the_stand_alone_agent_memory_included(case):
    W, H, R = 24, 40, 4
    steps, E, model_kw, slots, dyn_kws, pop_kw = POPULATIONS[case]
    dyn = lambda r: die.Dynamics(**dyn_kws[r % len(dyn_kws)](W, H))               # noqa: E731
    cands = _candidates(R // E, W + R, **model_kw)
    benv = BatchedEnv((W, H), dyn(0) if len(dyn_kws) == 1 else [dyn(r) for r in range(R)], replicas=R, seed=11, max_agents=slots)
    pop = BatchedNeuralAutomataAgent.from_agents(benv, cands, E, **pop_kw)
    assert pop._memory_channels == 2 and tuple(pop.memory.shape) == (R, 2, benv.Nmax) and not pop.memory.any()
    assert pop.P == sum(k.weight.numel() for k in cands[0].model.conv_layers())
    rew, alive = BatchedEnv.read_results(benv.run(pop, steps))
    if case == 'epoch_wrap':
        assert benv.epoch == 3
    for r in range(R):
        env = die.Env((W, H), dyn(r), seed=11 + r, max_agents=slots)
        ag = pop.replica_agent(r)
        assert ag.memory_channels == 2 and ag.memory is None                     # blank memory
        want_rew, want_alive = _run_alone(env, ag, steps)
        _assert_replica_is(benv, pop, r, env, ag, rew, alive, want_rew, want_alive)
    if E == 2:                                                                    # a memory per replica, not per candidate
        assert not torch.equal(pop.memory[0], pop.memory[1])
    if case == 'die_fixed_flow':                                                  # the fixed layout: dead slots from the first step on
        assert (alive < 200).all() and all(benv.n[r] == 200 for r in range(R))
    assert pop.candidate(0).memory is None and pop.reset.__func__ is BatchedNeuralAutomataAgent.reset_memory
    pop.reset()
    assert not pop.memory.any()


def test_memory_and_memoryless_populations_take_turns_on_one_batch():
    W, H, R = 24, 40, 3
    order = 'MPMMPPM'
    dyn = lambda: die.Dynamics(**dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15))   # noqa: E731
    with_memory = _candidates(R, 12, **WIDE)
    torch.manual_seed(13)
    plain = [die.NeuralAutomataAgent(scale=0.01, deposit=2.0, **WIDE) for _ in range(R)]
    for p in plain:
        p.model.init_weights()
    benv = BatchedEnv((W, H), dyn(), replicas=R, seed=21)
    pops = {'M': BatchedNeuralAutomataAgent.from_agents(benv, with_memory), 'P': BatchedNeuralAutomataAgent.from_agents(benv, plain)}
    assert getattr(pops['P'], 'reset', None) is None and pops['P'].memory is None and callable(pops['M'].reset)
    out = torch.stack([benv.step(pops[c]).clone() for c in order])
    rew, alive = BatchedEnv.read_results(out)
    for r in range(R):
        env = die.Env((W, H), dyn(), seed=21 + r, max_agents='alive')
        mine = {'M': pops['M'].replica_agent(r), 'P': pops['P'].replica_agent(r)}
        obs, want_rew, want_alive = env._get_current_obs, [], []
        for c in order:
            obs, rw, _, _, info = env.step(mine[c].forward(obs))
            want_rew.append(rw)
            want_alive.append(info['num_agents'])
        _assert_replica_is(benv, pops['M'], r, env, mine['M'], rew, alive, np.array(want_rew), np.array(want_alive))


def test_large_world_branch_keeps_a_memory_per_stand_alone_agent():
    W, H, R, steps = 24, 40, 3, 5
    dyn = lambda: die.Dynamics(**dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15))   # noqa: E731
    cands = _candidates(R, 9, **WIDE)
    big, small = (BatchedEnv((W, H), dyn(), replicas=R, seed=4, per_replica=p) for p in (True, False))
    pb, ps = BatchedNeuralAutomataAgent.from_agents(big, cands), BatchedNeuralAutomataAgent.from_agents(small, cands)
    assert torch.equal(big.run(pb, steps), small.run(ps, steps)) and pb.memory is None
    for r in range(R):
        assert np.array_equal(_bits(pb.agents[r].memory), _bits(ps.memory[r, :, :small.n[r]])), r
    pb.reset()
    assert all(not ag.memory.any() for ag in pb.agents)


# ---------------------------------------------------------------------------------------------------- 7. search
@pytest.mark.parametrize('kind,R', [('pgpe', 4), ('cmaes', 5)])
def test_two_generations_of_search_score_every_candidate_from_blank_memory(kind, R):
    W, H, T = 24, 40, 5
    torch.manual_seed(0)
    template = die.NeuralAutomataAgent(scale=0.01, deposit=2.0, memory_channels=2, **WIDE)
    template.model.init_weights()
    dyn = lambda: die.Dynamics(agents_die=True, **dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15))     # noqa: E731
    benv = BatchedEnv((W, H), dyn(), replicas=R, seeds=[9] * R)
    pop = BatchedNeuralAutomataAgent(benv, template)
    if kind == 'pgpe':
        s = PGPE(R, center_init=pop.parameters[0].cpu(), radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1,
                 optimizer_config=dict(max_speed=0.1, momentum=0.9), seed=11, device='cuda').for_population(pop, T)
    else:
        s = CMAES(R, center_init=pop.parameters[0].cpu(), stdev_init=0.1, seed=11, device='cuda').for_population(pop, T)
    assert s._pop_reset is not None
    for generation in range(2):
        s.step()
        assert pop.memory.any()                                                   # (what generation 2 must not start from)
        rows = pop.parameters.clone()
        fitness = s.fitness.cpu().tolist()
        for r in range(R):
            env = die.Env((W, H), dyn(), seed=9, max_agents='alive')
            ag = BatchedNeuralAutomataAgent.unpack(template, rows[r].cpu())
            assert ag.memory is None
            want_rew, _ = _run_alone(env, ag, T)
            assert fitness[r] == sum(want_rew.tolist()), (generation, r)
    # a memoryless population's generation issues no extra call
    plain = die.NeuralAutomataAgent(scale=0.01, deposit=2.0, **WIDE)
    other = BatchedNeuralAutomataAgent(BatchedEnv((W, H), dyn(), replicas=R, seeds=[9] * R), plain)
    if kind == 'pgpe':
        t = PGPE(R, center_init=other.parameters[0].cpu(), radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1, seed=11,
                 device='cuda').for_population(other, T)
    else:
        t = CMAES(R, center_init=other.parameters[0].cpu(), stdev_init=0.1, seed=11, device='cuda').for_population(other, T)
    assert t._pop_reset is None and getattr(other, 'reset', None) is None


# ---------------------------------------------------------------------------------------------------- 8. re-sorted storage
def test_memory_follows_the_agents_through_re_sorted_storage():
    """2048^2, the smallest world that takes the tile-binned step: a PhysarumAgent's binned steps keep the arrays stored tile by
    tile, and the memory — by slot id — is bit for bit that of the same world stepped with pic=False, in slot order."""
    W = H = 2048
    mems = []
    for pic in (True, False):
        env = die.Env((W, H), die.Dynamics(init_agent_ratio=0.02), seed=3, max_agents='alive', pic=pic, sort_every=0)
        N = env.agents.N
        phys = die.PhysarumAgent(max_agents=N, seed=1, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
        ag = _memory_agent(7, 2, kernel_sizes=[1, 1], hidden_channels=4)
        obs = env._get_current_obs
        for cycle in range(3):
            obs, *_ = env.step(phys.forward(obs))                                # (binned where pic: the storage is re-sorted)
            if pic:
                assert env._pic is not None and env.agents.slot is not None
                assert not torch.equal(env.agents.slot.cpu().to(torch.int64), torch.arange(N))
            else:
                assert env.agents.slot is None
            obs, *_ = env.step(ag.forward(obs))
        mems.append(ag.memory.clone())
    assert tuple(mems[0].shape) == (2, N) and mems[0].any() and torch.equal(mems[0].view(torch.int32), mems[1].view(torch.int32))


# ---------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_leave_memory_dropout_step_and_the_world_untouched():
    W, H, N = 24, 40, 200
    rs = np.random.RandomState(10)
    medium, agents = _world(W, H, N, rs)
    env = die.Env.from_numpy(medium, agents)
    ag = _memory_agent(11, 2, p_agent_dropout=0.25, dropout_seed=3, **WIDE)
    ag.forward(env._get_current_obs)
    held, step = ag.memory.clone(), ag.dropout_step
    world = [t.copy() for t in (env.medium.to_numpy(), env.agents.to_numpy())]
    for call in (lambda: ag.differentiable_sense(env.medium), lambda: ag.differentiable_action(env._get_current_obs),
                 lambda: ag.model.forward_device(torch.zeros((5, W, H), device=DEV))):
        with pytest.raises(NotImplementedError, match='memory'):
            call()
    with pytest.raises(ValueError, match='agents'):
        ag.sense(env.medium)
    other = die.Env.from_numpy(*_world(W, H, N + 1, rs))                          # a forward with another N
    with pytest.raises(ValueError, match='reset_memory'):
        ag.forward(other._get_current_obs)
    assert torch.equal(ag.memory.view(torch.int32), held.view(torch.int32)) and ag.dropout_step == step == 1
    assert all(np.array_equal(u, v) for u, v in zip(world, (env.medium.to_numpy(), env.agents.to_numpy())))
    ag.reset_memory()                                                             # … until reset_memory()
    ag.forward(other._get_current_obs)
    assert tuple(ag.memory.shape) == (2, N + 1)
    # agents_born: where the Dynamics is known, the population's constructor
    benv = BatchedEnv((W, H), die.Dynamics(agents_die=True, agents_born=True, init_agent_ratio=0.15), replicas=2, seed=1, max_agents=300)
    with pytest.raises(NotImplementedError, match='agents_born'):
        BatchedNeuralAutomataAgent(benv, ag)
    pop = BatchedNeuralAutomataAgent(BatchedEnv((W, H), die.Dynamics(init_agent_ratio=0.15), replicas=2, seed=1), ag, dropout_seed=3)
    pop.env.step(pop)
    held, step = pop.memory.clone(), pop.dropout_step
    for call in (pop.differentiable_sense, pop.differentiable_action, pop.forward_device):
        with pytest.raises(NotImplementedError, match='memory'):
            call()
    assert torch.equal(pop.memory.view(torch.int32), held.view(torch.int32)) and pop.dropout_step == step == 1
