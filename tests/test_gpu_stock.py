"""The stock channel on the device (die_stock.hip; NeuralAutomataAgent(with_stock_channel=True)): the plane build against the
numpy model word for word (300 slots, and 2 M slots: more than the grid has threads), rebuilds on one plane, the conv loaders' fourth plane kind, the stand-alone agent, and populations
whose replica r is, bit for bit, the stand-alone run of a stock-channel agent — across the epoch wrap, interleaved with a plain
population on one BatchedEnv, and under both searchers."""
import ctypes as C

import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent
from die_amd.device_array import DeviceAgents, stream_ptr
from die_amd.search import CMAES, PGPE
from tests import stock_plane_model as M
from tests.midsize_shapes import STOCK_BATCH_N, STOCK_N, STOCK_PLANE, stock_plane_fast, stock_winners_fast, stock_world

pytestmark = pytest.mark.gpu

DEV = 'cuda'
RTOL = 1e-5                          # tests/test_gpu_parity.py::test_neural_automata_forward_parity: rtol 1e-5 with atol = 1e-5
ATOL = 1e-5
REFERENCE_DYNAMICS = dict(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8)     # examples/learning_agents.py
TOP = 2 ** 32 - 1
PADS = ['circular', 'zeros', 'reflect', 'replicate']
TORCH_PAD = {'circular': 'circular', 'zeros': 'constant', 'reflect': 'reflect', 'replicate': 'replicate'}


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _i32(words):
    """uint32 words as the int32 tensor the device arrays are."""
    return torch.from_numpy(np.asarray(words, dtype=np.uint32).view(np.int32).copy()).to(DEV)


def _label(c, n):
    """The Q0.32 word of label c of an axis of n cells (0 and 2^32 - 1 at the ends)."""
    return min(TOP, (int(c) << 32) // (n - 1))


def _crowd(W, H, N, rs, n_alive=None):
    """N slots in SLOT order: at least three alive agents on each of eight border / corner cells and two inner ones, dead slots
    interleaved (every fifth slot, crowded cells included), one negative and one denormal stock among the winners."""
    x = rs.randint(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    y = rs.randint(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    x[0], y[0], x[1], y[1] = 0, 0, TOP, TOP                                     # the coordinate range's two ends
    cells = [(0, 0), (W - 1, H - 1), (0, H - 1), (W - 1, 0), (0, H // 2), (W - 1, 5), (W // 2, 0), (3, H - 1), (W // 2, H // 2), (5, 9)]
    slot = 2
    for cx, cy in cells:
        for _ in range(5):                                                        # five slots a cell, at least three of them alive
            x[slot], y[slot] = _label(cx, W), _label(cy, H)
            slot += 4                                                             # (4 and 5 are coprime: one of the five is dead)
    alive = (np.arange(N) % 5 != 3).astype(np.uint8)
    if n_alive is not None:
        alive[n_alive:] = 0
    food = (0.05 + rs.rand(N)).astype(np.float32)
    occ, win = M.stock_winners(W, H, x, y, alive)
    assert all(occ[c] and (alive[(M.cell(x, W) == c[0]) & (M.cell(y, H) == c[1])] > 0).sum() >= 3 for c in cells)
    food[win[0, 0]], food[win[W - 1, H - 1]] = np.float32(-0.625), np.float32(1e-41)   # winners: a negative, a denormal stock
    return x, y, alive, food


def _upload(x, y, alive, food, perm):
    """The slots stored in the order `perm` (storage entry j holds slot perm[j]), with the `slot` array saying so."""
    return _i32(x[perm]), _i32(y[perm]), _dev(alive[perm], torch.uint8), _dev(food[perm], torch.float32), _i32(perm.astype(np.uint32))


def _assert_plane_is(words, epoch, W, H, x, y, alive, food, what):
    occ, slot, bits, _ = M.decode(words.cpu().numpy().view(np.uint64), epoch)
    want_occ, want_slot = M.stock_winners(W, H, x, y, alive)
    assert np.array_equal(occ, want_occ), what
    assert np.array_equal(slot, want_slot), what
    assert np.array_equal(bits, M.stock_plane(W, H, x, y, alive, food).view(np.uint32)), what


def _medium(W, H, epoch=1):
    return _lib.Medium(W, H, _lib.DIE_F32, epoch, None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, None)


# ---------------------------------------------------------------------------------------------------- 1. the build
def test_stock_plane_is_the_model_word_for_word():
    W, H, N, epoch = 20, 68, 300, 7
    rs = np.random.RandomState(1)
    x, y, alive, food = _crowd(W, H, N, rs)
    perm = rs.permutation(N)
    tx, ty, ta, tf, ts = _upload(x, y, alive, food, perm)
    plane = torch.zeros((W, H), dtype=torch.int64, device=DEV)
    a = _lib.Agents(N, tx.data_ptr(), ty.data_ptr(), ta.data_ptr(), tf.data_ptr(), ts.data_ptr())
    _lib.check(_lib.lib.die_stock_plane(C.byref(_medium(W, H)), C.byref(a), epoch, plane.data_ptr(), stream_ptr(plane.device)), 'die_stock_plane')
    _assert_plane_is(plane, epoch, W, H, x, y, alive, food, 'shuffled storage')
    host = plane.cpu().numpy().view(np.uint64)
    assert (M.decode(host, epoch)[3][host != 0] == epoch).all()                  # nothing but this build's words
    assert M.decode(host, epoch)[0].sum() < alive.sum()                          # (cells are shared: fewer winners than alive slots)
    # the same slots in slot order, without a slot array: the same words
    ident = np.arange(N)
    tx, ty, ta, tf, _ = _upload(x, y, alive, food, ident)
    again = torch.zeros_like(plane)
    a = _lib.Agents(N, tx.data_ptr(), ty.data_ptr(), ta.data_ptr(), tf.data_ptr(), None)
    _lib.check(_lib.lib.die_stock_plane(C.byref(_medium(W, H)), C.byref(a), epoch, again.data_ptr(), stream_ptr(plane.device)), 'die_stock_plane')
    assert torch.equal(again, plane)


def test_stock_planes_of_three_replicas_in_one_launch():
    W, H, stride, epoch, R = 20, 68, 300, 31, 3
    n = [300, 123, 41]
    pad = 16                                                                     # a plane_stride above a plane: the gap stays untouched
    rs = np.random.RandomState(2)
    worlds, arrays = [], [np.zeros((R, stride), dtype=t) for t in (np.uint32, np.uint32, np.uint8, np.float32, np.uint32)]
    for r in range(R):
        x, y, alive, food = _crowd(W, H, stride, rs, n_alive=None)
        x, y, alive, food = x[:n[r]], y[:n[r]], alive[:n[r]], food[:n[r]]
        perm = rs.permutation(n[r])
        worlds.append((x, y, alive, food))
        for dst, src in zip(arrays, (x[perm], y[perm], alive[perm], food[perm], perm.astype(np.uint32))):
            dst[r, :n[r]] = src
        # the padding slots n >= n[r]: alive, well fed and standing on a cell of their own — they must be skipped
        arrays[0][r, n[r]:], arrays[1][r, n[r]:], arrays[2][r, n[r]:], arrays[3][r, n[r]:] = _label(7, W), _label(33, H), 1, 99.0
        arrays[4][r, n[r]:] = np.arange(n[r], stride)
    tx, ty = _i32(arrays[0]), _i32(arrays[1])
    ta, tf, ts = _dev(arrays[2], torch.uint8), _dev(arrays[3], torch.float32), _i32(arrays[4])
    planes = torch.zeros((R, W * H + pad), dtype=torch.int64, device=DEV)
    a = _lib.Agents(stride, tx.data_ptr(), ty.data_ptr(), ta.data_ptr(), tf.data_ptr(), ts.data_ptr())
    b = _lib.Batch(R, 0, W * H + pad, stride, 1, (C.c_int64 * 64)(*n))
    _lib.check(_lib.lib.die_stock_plane_batch(C.byref(_medium(W, H)), C.byref(a), C.byref(b), epoch, planes.data_ptr(),
                                              stream_ptr(planes.device)), 'die_stock_plane_batch')
    for r in range(R):
        _assert_plane_is(planes[r, :W * H].reshape(W, H), epoch, W, H, *worlds[r], f'replica {r}')
    assert not planes[:, W * H:].any()


def _assert_plane_is_fast(words, epoch, W, H, x, y, alive, food, what):
    """_assert_plane_is at 2 M slots: the model's winners without its Python loop (tests/test_batch_midsize_cpu.py checks that
    they are the model's)."""
    occ, slot, bits, _ = M.decode(words.cpu().numpy().view(np.uint64), epoch)
    want_occ, want_slot = stock_winners_fast(W, H, x, y, alive)
    assert np.array_equal(occ, want_occ), what
    assert np.array_equal(slot, want_slot), what
    assert np.array_equal(bits, stock_plane_fast(W, H, x, y, alive, food).view(np.uint32)), what


def test_stock_plane_past_the_grid_cap():
    """2 097 665 slots, more than the 8192 x 256 threads of the grid: every thread takes a second slot, and the last 513 slots
    are reached only by that second trip.  256 x 256 cells for a million alive slots: every cell is shared, the highest slot
    id must win whichever trip issued it.  Stored shuffled, with a slot array, then in slot order without one."""
    (W, H), N, epoch = STOCK_PLANE, STOCK_N, 9
    rs = np.random.RandomState(1)
    x, y, alive, food = stock_world(W, H, N, rs)
    assert alive[-513:].any() and alive.sum() > 8 * W * H
    perm = rs.permutation(N)
    planes = []
    for order, with_slots in ((perm, True), (np.arange(N), False)):
        tx, ty, ta, tf, ts = _upload(x, y, alive, food, order)
        plane = torch.zeros((W, H), dtype=torch.int64, device=DEV)
        a = _lib.Agents(N, tx.data_ptr(), ty.data_ptr(), ta.data_ptr(), tf.data_ptr(), ts.data_ptr() if with_slots else None)
        _lib.check(_lib.lib.die_stock_plane(C.byref(_medium(W, H)), C.byref(a), epoch, plane.data_ptr(), stream_ptr(plane.device)), 'die_stock_plane')
        _assert_plane_is_fast(plane, epoch, W, H, x, y, alive, food, 'shuffled' if with_slots else 'slot order')
        planes.append(plane)
    assert torch.equal(planes[0], planes[1])
    host = planes[0].cpu().numpy().view(np.uint64)
    assert (M.decode(host, epoch)[3] == epoch).all()                             # every cell holds a word of this build


def test_stock_planes_past_the_grid_cap_two_replicas():
    """R = 2 in one launch, n = (2 097 665, 300): replica 1's threads beyond its 300 slots idle through both trips, and its
    plane holds its own 300 slots' words and nothing of replica 0's."""
    (W, H), n, epoch, R = STOCK_PLANE, STOCK_BATCH_N, 31, 2
    stride = max(n)
    rs = np.random.RandomState(2)
    worlds = [tuple(v[:n[r]] for v in stock_world(W, H, stride, rs)) for r in range(R)]
    arrays = [np.zeros((R, stride), dtype=t) for t in (np.uint32, np.uint32, np.uint8, np.float32)]
    for r in range(R):
        for dst, src in zip(arrays, worlds[r]):
            dst[r, :n[r]] = src
        # the padding slots n >= n[r]: alive, well fed and standing on a cell of their own — they must be skipped
        arrays[0][r, n[r]:], arrays[1][r, n[r]:], arrays[2][r, n[r]:], arrays[3][r, n[r]:] = _label(7, W), _label(33, H), 1, 99.0
    tx, ty, ta, tf = _i32(arrays[0]), _i32(arrays[1]), _dev(arrays[2], torch.uint8), _dev(arrays[3], torch.float32)
    planes = torch.zeros((R, W * H), dtype=torch.int64, device=DEV)
    a = _lib.Agents(stride, tx.data_ptr(), ty.data_ptr(), ta.data_ptr(), tf.data_ptr(), None)
    b = _lib.Batch(R, 0, W * H, stride, 1, (C.c_int64 * 64)(*n))
    _lib.check(_lib.lib.die_stock_plane_batch(C.byref(_medium(W, H)), C.byref(a), C.byref(b), epoch, planes.data_ptr(),
                                              stream_ptr(planes.device)), 'die_stock_plane_batch')
    for r in range(R):
        _assert_plane_is_fast(planes[r].reshape(W, H), epoch, W, H, *worlds[r], f'replica {r}')
    small = M.decode(planes[1].cpu().numpy().view(np.uint64), epoch)
    assert 0 < small[0].sum() <= worlds[1][2].sum() and small[1].max() < n[1]    # at most 300 words, of slots below 300


# ---------------------------------------------------------------------------------------------------- 2. rebuilds
def test_a_rebuild_leaves_no_cell_of_the_earlier_build_occupied():
    W, H, N = 20, 68, 300
    rs = np.random.RandomState(3)
    plane = torch.zeros((W, H), dtype=torch.int64, device=DEV)
    before = None
    for epoch in (29, 30, 31):                                                   # the agents move between the builds
        x, y, alive, food = _crowd(W, H, N, rs)
        perm = rs.permutation(N)
        tx, ty, ta, tf, ts = _upload(x, y, alive, food, perm)
        a = _lib.Agents(N, tx.data_ptr(), ty.data_ptr(), ta.data_ptr(), tf.data_ptr(), ts.data_ptr())
        _lib.check(_lib.lib.die_stock_plane(C.byref(_medium(W, H)), C.byref(a), epoch, plane.data_ptr(), stream_ptr(plane.device)), 'die_stock_plane')
        _assert_plane_is(plane, epoch, W, H, x, y, alive, food, epoch)
        occ = M.stock_winners(W, H, x, y, alive)[0]
        if before is not None:
            assert (before & ~occ).any()                                          # cells the agents left: they read as empty now
            tags = M.decode(plane.cpu().numpy().view(np.uint64), epoch)[3]
            assert (tags[before & ~occ] == epoch - 1).all()                        # (their old words are still there, and lose)
        before = occ


@pytest.mark.parametrize('wide', [False, True], ids=['narrow', 'wide'])
def test_the_agent_rebuilds_its_plane_across_the_epoch_wrap(wide):
    """The Python owner: builds at epochs 30, 31, then 1 after the wrap (where it starts the plane over), then 1 AGAIN (a second
    sense without a step) — every time the plane decodes to the agents of that moment and to nothing else."""
    W, H, N = 20, 68, 300
    rs = np.random.RandomState(4)
    kw = dict(kernel_sizes=(3, 3), hidden_channels=8) if wide else dict(kernel_sizes=(3,))
    ag = die.NeuralAutomataAgent(with_stock_channel=True, **kw)
    env = die.Env.from_numpy(*_world(W, H, N, rs))
    env.medium.epoch = 29
    for step in range(4):
        if step < 3:
            env.medium.next_epoch()
        want_epoch = (30, 31, 1, 1)[step]
        assert env.medium.epoch == want_epoch
        x, y, alive, food = _crowd(W, H, N, rs)
        agents = DeviceAgents(N, env.device)
        agents.x, agents.y, agents.alive, agents.agent_food = _i32(x), _i32(y), _dev(alive, torch.uint8), _dev(food, torch.float32)
        ag.sense(env.medium, agents)
        (plane, last), = ag._stock.values()
        assert last == want_epoch
        _assert_plane_is(plane, want_epoch, W, H, x, y, alive, food, step)
        tags = M.decode(plane.cpu().numpy().view(np.uint64), want_epoch)[3]
        if want_epoch == 1:
            assert set(np.unique(tags).tolist()) <= {0, 1}                       # started over: no word of the last cycle is left


# ---------------------------------------------------------------------------------------------------- 3. the loaders
def _world(W, H, N, rs, alive_ratio=0.8):
    """(medium (3, W, H), agents (4, N)) as float64 arrays the device represents exactly; stocks in (0.05, 1.05)."""
    food = np.round(rs.rand(W, H) * 0.5 * (rs.rand(W, H) < 0.6), 3).astype(np.float32).astype(np.float64)
    chem = rs.rand(W, H).astype(np.float32).astype(np.float64)
    xw, yw = rs.randint(0, 2 ** 32, N, dtype=np.uint64), rs.randint(0, 2 ** 32, N, dtype=np.uint64)
    alive = (rs.rand(N) < alive_ratio).astype(np.float64)
    agents = np.stack([xw / 4294967296.0, yw / 4294967296.0, alive, (0.05 + rs.rand(N)).astype(np.float32).astype(np.float64)])
    occ = np.zeros((W, H))
    occ[M.cell(xw.astype(np.uint32), W)[alive > 0], M.cell(yw.astype(np.uint32), H)[alive > 0]] = 1.
    return np.stack([occ, food, chem]), agents


def _reference_conv(x, w, pad, k):
    """tanh of torch's float64 cross-correlation with 'same' padding of mode `pad`."""
    xt = torch.from_numpy(x)[None]
    r = k // 2
    if r:
        xt = torch.nn.functional.pad(xt, (r, r, r, r), mode=TORCH_PAD[pad])
    return torch.tanh(torch.nn.functional.conv2d(xt, torch.from_numpy(w.astype(np.float64))))[0].numpy()


@pytest.mark.parametrize('pad', PADS)
@pytest.mark.parametrize('W,H', [(20, 68), (8, 12)])
def test_layers_read_a_stock_plane_as_its_model_plane(W, H, pad):
    """die_conv2d (k = 1, 3, 5, 7) and die_conv2d_wide (k = 1, 3, 5, cout 8) on (claim plane, fp16 plane, fp32 plane, STOCK plane):
    the same bits as with the model's plane uploaded as a plain fp32 plane, and torch's float64 Conv2d within the parity tolerance."""
    N, epoch = 3 * W * H // 4, 5
    rs = np.random.RandomState(W + len(pad))
    x, y, alive, food = _crowd(W, H, max(N, 75), rs) if W == 20 else (None,) * 4
    if x is None:                                                                # 8 x 12: no room for the crowd's cells; a random one
        n = 60
        x, y = (rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32) for _ in range(2))
        alive, food = (np.arange(n) % 4 != 1).astype(np.uint8), (rs.rand(n) - 0.3).astype(np.float32)
    n = len(x)
    perm = rs.permutation(n)
    tx, ty, ta, tf, ts = _upload(x, y, alive, food, perm)
    stock = torch.zeros((W, H), dtype=torch.int64, device=DEV)
    a = _lib.Agents(n, tx.data_ptr(), ty.data_ptr(), ta.data_ptr(), tf.data_ptr(), ts.data_ptr())
    sp = stream_ptr(stock.device)
    _lib.check(_lib.lib.die_stock_plane(C.byref(_medium(W, H)), C.byref(a), epoch, stock.data_ptr(), sp), 'die_stock_plane')
    S = M.stock_plane(W, H, x, y, alive, food)
    model = torch.from_numpy(S).to(DEV)
    # the other three kinds: a claim plane at the same epoch (other cells than the stock's), an fp16 and an fp32 field
    occ = rs.rand(W, H) < 0.3
    claim = _dev(np.where(occ, M.encode(epoch, 0, 0.0), M.encode(epoch - 1, 3, 1.0)).view(np.int64), torch.int64)
    f16 = torch.from_numpy(rs.rand(W, H).astype(np.float16)).to(DEV)
    f32 = torch.from_numpy(rs.rand(W, H).astype(np.float32)).to(DEV)
    seen = np.stack([occ.astype(np.float64), f16.cpu().numpy().astype(np.float64), f32.cpu().numpy().astype(np.float64), S.astype(np.float64)])
    fixed = [(claim, _lib.DIE_PLANE_AGENTS), (f16, _lib.DIE_PLANE_F16), (f32, _lib.DIE_PLANE_F32)]
    pm = _lib.PAD_MODES[pad]

    def planes(last):
        return (_lib.ConvPlane * 4)(*[_lib.ConvPlane(t.data_ptr(), kind, 0) for t, kind in fixed + [last]])

    for k in (1, 3, 5, 7):
        w = (rs.rand(3, 4, k, k).astype(np.float32) - 0.5) / k
        tw = torch.from_numpy(w).to(DEV)
        outs = []
        for last in ((stock, _lib.DIE_PLANE_STOCK), (model, _lib.DIE_PLANE_F32)):
            dst = torch.full((3, W, H), 7.0, dtype=torch.float32, device=DEV)
            out_arr = (C.c_void_p * 3)(*[dst[o].data_ptr() for o in range(3)])
            _lib.check(_lib.lib.die_conv2d(W, H, 4, planes(last), epoch, 3, out_arr, k, tw.data_ptr(), 1, pm, sp), 'die_conv2d')
            outs.append(dst.cpu().numpy())
        assert np.array_equal(outs[0], outs[1]), ('die_conv2d', k)
        assert np.allclose(outs[0], _reference_conv(seen, w, pad, k), rtol=RTOL, atol=ATOL), ('die_conv2d', k)
    for k in (1, 3, 5):
        w = (rs.rand(8, 4, k, k).astype(np.float32) - 0.5) / k
        tw = torch.from_numpy(w).to(DEV)
        outs = []
        for last in ((stock, _lib.DIE_PLANE_STOCK), (model, _lib.DIE_PLANE_F32)):
            dst = torch.full((8, W, H), 7.0, dtype=torch.float32, device=DEV)
            _lib.check(_lib.lib.die_conv2d_wide(W, H, 4, planes(last), epoch, 8, dst.data_ptr(), W * H, k, tw.data_ptr(), 1, pm, None, sp),
                       'die_conv2d_wide')
            outs.append(dst.cpu().numpy())
        assert np.array_equal(outs[0], outs[1]), ('die_conv2d_wide', k)
        assert np.allclose(outs[0], _reference_conv(seen, w, pad, k), rtol=RTOL, atol=ATOL), ('die_conv2d_wide', k)
    # read at another epoch the stock plane is empty: the layer sees zeros there
    dst = torch.empty((3, W, H), dtype=torch.float32, device=DEV)
    out_arr = (C.c_void_p * 3)(*[dst[o].data_ptr() for o in range(3)])
    w = np.zeros((3, 4, 1, 1), dtype=np.float32)
    w[:, 3] = 1.0
    tw = torch.from_numpy(w).to(DEV)
    _lib.check(_lib.lib.die_conv2d(W, H, 4, planes((stock, _lib.DIE_PLANE_STOCK)), epoch + 1, 3, out_arr, 1, tw.data_ptr(), 0, pm, sp), 'die_conv2d')
    assert not dst.any()


# ---------------------------------------------------------------------------------------------------- 4. stand-alone
STACKS = {'narrow': dict(kernel_sizes=(3, 3)), 'wide': dict(kernel_sizes=(3, 3), hidden_channels=8, with_agent_channel=False)}


def _stock_agent(seed, **kw):
    torch.manual_seed(seed)
    ag = die.NeuralAutomataAgent(scale=0.01, deposit=2.0, with_stock_channel=True, **kw)
    ag.model.init_weights()
    return ag


def _assert_sense_is_the_model(ag, env, what):
    """`sense` on the env's agents and medium against `model.forward` on the medium's planes stacked with the model's stock plane."""
    m, a = env.medium.to_numpy(), env.agents.to_numpy()
    S = M.stock_plane_of(env.medium.W, env.medium.H, a)
    x = np.concatenate([m if 'agents' in ag.obs_channels else m[1:], S[None].astype(np.float64)]).astype(np.float32)
    with torch.no_grad():
        want = ag.model.forward(torch.from_numpy(x)[None])[0].numpy()
    action = ag.forward(env._get_current_obs)
    got = ag._sense_output.cpu().numpy()
    assert np.allclose(got, want, rtol=RTOL, atol=ATOL), what
    return action, S


@pytest.mark.parametrize('stack', list(STACKS))
def test_stand_alone_sense_under_deaths_and_births(stack):
    W, H = 64, 48
    env = die.Env((W, H), die.Dynamics(agents_die=True, agents_born=True), seed=5)
    ag = _stock_agent(3, **STACKS[stack])
    assert ag.model.kernels[0].in_channels == (4 if stack == 'narrow' else 3)
    planes = []
    for step in range(5):
        action, S = _assert_sense_is_the_model(ag, env, (stack, step))
        planes.append(S)
        env.step(action)
    assert all(np.count_nonzero(S) > 0 for S in planes) and not np.array_equal(planes[0], planes[-1])      # the stocks moved on


def test_stand_alone_sense_after_tile_binned_steps():
    """The size and tile at which tests/test_gpu_parity.py::test_neural_automata_on_f16_fields_and_after_binned_steps takes the
    tile-binned step: the arrays are then stored tile by tile, and the build goes by their `slot` ids."""
    W, H, N = 128, 96, 4000
    rs = np.random.RandomState(5)
    medium, agents = _world(W, H, N, rs, alive_ratio=2.0)
    env = die.Env.from_numpy(medium, agents, field_dtype=torch.float16)
    env._pic_tile = (4, 5)
    phys = die.PhysarumAgent(max_agents=N, seed=1, scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1))
    obs = env._get_current_obs
    for _ in range(3):
        obs, *_ = env.step(phys.forward(obs))
    assert env._pic is not None and env.agents.slot is not None
    assert not torch.equal(env.agents.slot.cpu().to(torch.int64), torch.arange(N))           # a storage order of its own
    ag = _stock_agent(7, kernel_sizes=(3, 3))
    _, S = _assert_sense_is_the_model(ag, env, 'binned')
    assert np.count_nonzero(S) > N // 2


# ---------------------------------------------------------------------------------------------------- 5. the stock matters
def test_the_stock_changes_what_a_stock_agent_senses_and_nothing_else():
    W, H, N = 48, 40, 600
    rs = np.random.RandomState(6)
    medium, agents = _world(W, H, N, rs)
    other = agents.copy()
    other[3] = (agents[3] * 0.25 + 0.5).astype(np.float32)
    envs = [die.Env.from_numpy(medium, a) for a in (agents, other)]
    stock, plain = _stock_agent(8, kernel_sizes=(3, 3)), die.NeuralAutomataAgent(scale=0.01, deposit=2.0, kernel_sizes=(3, 3))
    plain.model.init_weights()
    seen = [stock.sense(e.medium, e.agents).cpu().numpy().copy() for e in envs]
    assert not np.array_equal(seen[0], seen[1])
    unseen = [plain.sense(e.medium).cpu().numpy().copy() for e in envs]
    assert np.array_equal(unseen[0], unseen[1])
    assert np.array_equal(plain.sense(envs[0].medium, envs[0].agents).cpu().numpy(), unseen[0])      # (agents given: unused)
    assert plain._stock == {} and plain.obs_channels == ['agents', 'env_food', 'chem1']
    # the plain agent's planes are those of the launches it has always made: die_conv2d per layer on the medium's three planes
    e = envs[0]
    src = [(e.medium.owner, _lib.DIE_PLANE_AGENTS), (e.medium.food, _lib.DIE_PLANE_F32), (e.medium.chem, _lib.DIE_PLANE_F32)]
    sp = stream_ptr(e.device)
    layers = plain.model.conv_layers()
    for li, layer in enumerate(layers):
        w = layer.weight.detach().to(e.device).contiguous()
        dst = torch.empty((3, W, H), dtype=torch.float32, device=e.device)
        arr = (_lib.ConvPlane * 3)(*[_lib.ConvPlane(t.data_ptr(), kind, 0) for t, kind in src])
        out_arr = (C.c_void_p * 3)(*[dst[o].data_ptr() for o in range(3)])
        _lib.check(_lib.lib.die_conv2d(W, H, 3, arr, e.medium.epoch, 3, out_arr, 3, w.data_ptr(), int(li == len(layers) - 1), 0, sp), 'die_conv2d')
        src = [(dst[o], _lib.DIE_PLANE_F32) for o in range(3)]
    assert np.array_equal(dst.cpu().numpy(), unseen[0])


# ---------------------------------------------------------------------------------------------------- 6. populations
def _run_alone(env, agent_at, steps):
    obs, rew, alive, ag = env._get_current_obs, [], [], None
    for i in range(steps):
        ag = agent_at(i)
        obs, rw, _, _, info = env.step(ag.forward(obs))
        rew.append(rw)
        alive.append(info['num_agents'])
    return ag, np.array(rew), np.array(alive)


def _assert_replica_is(benv, pop, r, env, ag, rew, alive, want_rew, want_alive):
    m, a = benv.replica_numpy(r)
    assert np.array_equal(m, env.medium.to_numpy()), r
    assert np.array_equal(a, env.agents.to_numpy()), r
    assert np.array_equal(rew[:, r], want_rew), r
    assert np.array_equal(alive[:, r], want_alive), r
    assert np.array_equal(pop.render(r), ag.render()[0]), r


def _candidates(n, seed, scale=0.01, **kw):
    torch.manual_seed(seed)
    out = []
    for _ in range(n):
        ag = die.NeuralAutomataAgent(scale=scale, deposit=2.0, with_stock_channel=True, **kw)
        ag.model.init_weights()
        out.append(ag)
    return out


POPULATIONS = {
    # W, H, R, E, fp16, model, slots, Dynamics per replica, population arguments
    'die_born_fixed': (96, 96, 4, 1, False, dict(kernel_sizes=(3, 3), boundary='circular'), 2500,
                       [dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15, agents_die=True, agents_born=True)], {}),
    'fp16_zeros_no_agents': (64, 48, 5, 1, True, dict(kernel_sizes=(3,), boundary='zeros', with_agent_channel=False), 'alive',
                             [dict(init_agent_ratio=0.15)], {}),
    'wide_episodes_dropout': (32, 32, 4, 2, False, dict(kernel_sizes=(3, 3), hidden_channels=8, with_agent_channel=False,
                                                        p_agent_dropout=0.25), 'alive',
                              [dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15)], dict(dropout_seed=1000, dropout_seed_stride=1)),
    'dynamics_rows': (32, 32, 4, 1, False, dict(kernel_sizes=(3, 3)), 'alive',
                      [dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15),
                       dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15, diffuse_sigma=0.5, rate_decay_chem=0.05)], {}),
}


@pytest.mark.parametrize('case', list(POPULATIONS))
def test_replica_is_the_stand_alone_stock_agent(case):
    """33 steps: the epoch wraps once, and the stock planes are cleared with the claim planes."""
    W, H, R, E, f16, model_kw, slots, dyn_kws, pop_kw = POPULATIONS[case]
    steps, dt = 33, torch.float16 if f16 else torch.float32
    dyns = [die.Dynamics(**dyn_kws[r % len(dyn_kws)]) for r in range(R)]
    cands = _candidates(R // E, W + R, **model_kw)
    benv = BatchedEnv((W, H), dyns[0] if len(dyn_kws) == 1 else dyns, replicas=R, seed=11, field_dtype=dt, max_agents=slots)
    pop = BatchedNeuralAutomataAgent.from_agents(benv, cands, E, **pop_kw)
    assert pop._stock_channel and pop.P == sum(k.weight.numel() for k in cands[0].model.conv_layers())
    rew, alive = BatchedEnv.read_results(benv.run(pop, steps))
    assert benv._stock is not None and benv.epoch == 3
    for r in range(R):
        env = die.Env((W, H), die.Dynamics(**dyn_kws[r % len(dyn_kws)]), seed=11 + r, max_agents=slots, field_dtype=dt)
        ag = pop.replica_agent(r)
        assert ag.with_stock_channel and ag.obs_channels[-1] == 'agent_food'
        ag, want_rew, want_alive = _run_alone(env, lambda i: ag, steps)
        _assert_replica_is(benv, pop, r, env, ag, rew, alive, want_rew, want_alive)
    if case == 'die_born_fixed':
        assert (np.diff(alive, axis=0) > 0).any()                                # somebody was born on the way
    # a plain twin of the same weights' first channels runs another course: the channel is read
    plain = [die.NeuralAutomataAgent(scale=0.01, deposit=2.0, **model_kw) for _ in cands]
    for p, c in zip(plain, cands):
        for lp, lc in zip(p.model.conv_layers(), c.model.conv_layers()):
            lp.weight.data.copy_(lc.weight.data[:lp.weight.shape[0], :lp.weight.shape[1]])
    twin = BatchedEnv((W, H), dyns[0] if len(dyn_kws) == 1 else dyns, replicas=R, seed=11, field_dtype=dt, max_agents=slots)
    twin.run(BatchedNeuralAutomataAgent.from_agents(twin, plain, E, **pop_kw), steps)
    assert twin._stock is None
    assert not np.array_equal(twin.replica_numpy(0)[1], benv.replica_numpy(0)[1])


def test_large_world_branch_goes_through_the_stand_alone_agents():
    W, H, R, steps = 32, 32, 3, 6
    dyn = lambda: die.Dynamics(**dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15))
    cands = _candidates(R, 9, kernel_sizes=(3, 3))
    big, small = (BatchedEnv((W, H), dyn(), replicas=R, seed=4, per_replica=p) for p in (True, False))
    a = big.run(BatchedNeuralAutomataAgent.from_agents(big, cands), steps)
    b = small.run(BatchedNeuralAutomataAgent.from_agents(small, cands), steps)
    assert torch.equal(a, b) and big._stock is None
    for r in range(R):
        for u, v in zip(big.replica_numpy(r), small.replica_numpy(r)):
            assert np.array_equal(u, v), r


# ---------------------------------------------------------------------------------------------------- 7. interleaving
def test_stock_and_plain_populations_take_turns_on_one_batch():
    """S, 31 x P, S, S (the stock planes still hold the first step's words, tagged 1, when the population comes back at epoch 2),
    then 30 x P and S again: that last step senses at epoch 3, as the step before the plain run did — words of that build
    would read as agents that have long moved on, had the BatchedEnv not zeroed the planes."""
    W, H, R = 32, 32, 3
    order = 'S' + 'P' * 31 + 'SS' + 'P' * 30 + 'S'
    dyn = lambda: die.Dynamics(**dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15))
    stock = _candidates(R, 12, kernel_sizes=(3, 3))
    torch.manual_seed(13)
    plain = [die.NeuralAutomataAgent(scale=0.01, deposit=2.0, kernel_sizes=(3, 3)) for _ in range(R)]
    for p in plain:
        p.model.init_weights()
    benv = BatchedEnv((W, H), dyn(), replicas=R, seed=21)
    pops = {'S': BatchedNeuralAutomataAgent.from_agents(benv, stock), 'P': BatchedNeuralAutomataAgent.from_agents(benv, plain)}
    out = torch.stack([benv.step(pops[c]).clone() for c in order])
    rew, alive = BatchedEnv.read_results(out)
    assert [(i % 31) + 1 for i, c in enumerate(order) if c == 'S'] == [1, 2, 3, 3]          # the epochs the stock steps sensed at
    for r in range(R):
        env = die.Env((W, H), dyn(), seed=21 + r, max_agents='alive')
        mine = {'S': pops['S'].replica_agent(r), 'P': pops['P'].replica_agent(r)}
        ag, want_rew, want_alive = _run_alone(env, lambda i: mine[order[i]], len(order))
        _assert_replica_is(benv, pops['S'], r, env, ag, rew, alive, want_rew, want_alive)


# ---------------------------------------------------------------------------------------------------- 8. search
@pytest.mark.parametrize('kind', ['pgpe', 'cmaes'])
def test_two_generations_of_search_score_every_candidate_as_its_stand_alone_run(kind):
    size, T, R = 32, 6, 4
    torch.manual_seed(0)
    template = die.NeuralAutomataAgent(kernel_sizes=(3, 3), scale=0.01, deposit=2.0, with_stock_channel=True)
    template.model.init_weights()
    dyn = lambda: die.Dynamics(agents_die=True, **dict(REFERENCE_DYNAMICS, init_agent_ratio=0.15))
    benv = BatchedEnv((size, size), dyn(), replicas=R, seeds=[9] * R)
    pop = BatchedNeuralAutomataAgent(benv, template)
    assert pop.P == 4 * 4 * 9 + 3 * 4 * 9
    if kind == 'pgpe':
        s = PGPE(R, center_init=pop.parameters[0].cpu(), radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1,
                 optimizer_config=dict(max_speed=0.1, momentum=0.9), seed=11, device='cuda').for_population(pop, T)
    else:
        s = CMAES(R, center_init=pop.parameters[0].cpu(), stdev_init=0.1, seed=11, device='cuda').for_population(pop, T)
    seen = []
    for generation in range(2):
        s.step()
        rows = pop.parameters.clone()
        fitness = s.fitness.cpu().tolist()
        for r in range(R):
            env = die.Env((size, size), dyn(), seed=9, max_agents='alive')
            ag = BatchedNeuralAutomataAgent.unpack(template, rows[r].cpu())
            assert ag.with_stock_channel
            _, want_rew, _ = _run_alone(env, lambda i: ag, T)
            assert fitness[r] == sum(want_rew.tolist()), (generation, r)
        seen.append(rows)
    assert s.history().shape[0] == 2 and not torch.isnan(s.history()).any() and not torch.equal(seen[0], seen[1])
