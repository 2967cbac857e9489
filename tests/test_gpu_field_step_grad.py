"""The differentiable Env.step on the GPU (die_deposit_cells, die_env_step_backward behind `Env.differentiable_step` /
`Env.differentiable_chem`, and the chem node entering `NeuralAutomataAgent.differentiable_sense`) against the float64 torch oracle
of tests/field_step_adjoint_model.py and the host oracle's ownership rule (oracle/cpu_ref.py RefEnv).

Ceilings, none of them taken from what the device gives:
  * test 1, 2, 6 and the gather of test 3: bits, or integers, compared exactly;
  * test 3's field part: the project's forward ceiling max|dev - f64| <= 1e-5 * max(1, max|f64|);
  * test 4: |<step(c, d), g> - (<c, grad_chem> + <d, grad_deposit>)| <= 1e-6 of the right-hand side (tests/test_gpu_conv_abi.py's
    read-out identity).  c, d, g are positive, so no term cancels: every product carries a relative rounding error of a few 2^-24
    (a tap sum of at most 7 x 7 fp32 terms per pass) with random signs over 1632 cells — about 1e-8 of the sum;
  * test 5: per weight tensor max|grad_dev - grad_f64| <= 1e-4 * max|grad_f64| (tests/test_gpu_nca_grad.py's);
    tests/test_field_step_adjoint_cpu.py holds a plain fp32 evaluation of the same cases to a tenth of that.

Every ctypes call writes into buffers with a sentinel tail that must come back untouched; a test enqueues its launches on one
stream and synchronises before it reads anything back.  Shapes: 16 x 64 is one conv tile, 24 x 68 straddles tiles with H % 4 == 0
(the row sweep), 17 x 66 takes the LDS-tiled diffusion, 8 x 12 is smaller than a tile.  The entry points at full blocks (LABBOOK
§33; sizes in tests/grad_midsize_shapes.py, their premises in tests/test_grad_midsize_cpu.py): the gather at 255 ... 8 389 637
entries, die_deposit_cells and die_gather_scale_backward at 2 097 665 slots."""
import ctypes as C

import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib as L
from die_amd.device_array import _ptr, stream_ptr, unpermute
from oracle import cpu_ref as R
from tests import dropout_model as D
from tests import field_step_adjoint_model as F
from tests import grad_midsize_shapes as S

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FWD_TOL, ID_TOL, GRAD_TOL = 1e-5, 1e-6, 1e-4
SENT = np.float32(-7.25e7)                                        # no result comes near it
SENT_I = 0x5A5A5A5A
TAIL = 64
Q32 = 4294967296.0


def _nca(sizes=(3, 3), boundary='circular', weights=None, seed=0, **kw):
    torch.manual_seed(seed)
    ag = die.NeuralAutomataAgent(kernel_sizes=sizes, boundary=boundary, scale=F.COEFS[0], deposit=F.COEFS[2], **kw)
    with torch.no_grad():
        for i, q in enumerate(ag.model.parameters()):
            if weights is None:
                q.uniform_(-0.5, 0.5)
            else:
                q.copy_(torch.as_tensor(weights[i], dtype=torch.float32))
    return ag


def _state(env):
    """Everything a step leaves, as host arrays (raw words: bits are compared).  The agent arrays in SLOT order: after a re-sort the
    order inside a bucket is whatever order the waves reached the cursors in (die_sort.hip) and differs from run to run."""
    torch.cuda.synchronize()
    M, A = env.medium, env.agents
    out = dict(chem=M.chem, food=M.food, owner=M.owner)
    out.update({k: unpermute(getattr(A, k), A.slot) for k in ('x', 'y', 'alive', 'agent_food')})
    out = {k: v.cpu().numpy().copy() for k, v in out.items()}
    out['sorted'] = A.slot is not None
    if A.slot is not None:
        assert np.array_equal(np.sort(A.slot.cpu().numpy()), np.arange(A.N))
    out['epoch'] = M.epoch
    return out


def _same_state(a, b):
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert b[k] is not None and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        else:
            assert a[k] == b[k] if a[k] is not None else b[k] is None, k


def _array_cells(env):
    """(cx, cy) of every array entry as the kernels compute them (die_cell_u on the Q0.32 words), array order."""
    W, H = env.medium.W, env.medium.H
    x = (env.agents.x.to(torch.int64) & 0xFFFFFFFF).cpu().numpy().astype(np.float64) / Q32
    y = (env.agents.y.to(torch.int64) & 0xFFFFFFFF).cpu().numpy().astype(np.float64) / Q32
    return R.cell(x, W), R.cell(y, H)


# ------------------------------------------------------------------------------------------------ 1. the same world
@pytest.mark.parametrize('sort_every', [None, 2])
@pytest.mark.parametrize('sigma', [0.5, 0.8])
@pytest.mark.parametrize('W,H', [(16, 64), (24, 68), (8, 12)])
def test_differentiable_step_equals_step(W, H, sigma, sort_every):
    dyn = lambda: die.Dynamics(diffuse_sigma=sigma)
    plain = die.Env((W, H), dyn(), seed=5, device=DEV, sort_every=sort_every)
    diff = die.Env((W, H), dyn(), seed=5, device=DEV, sort_every=sort_every)
    _same_state(_state(plain), _state(diff))
    ag = _nca()
    node = diff.differentiable_chem()
    assert node.is_leaf and not node.requires_grad and node is diff.differentiable_chem()
    assert torch.equal(node, diff.medium.chem) and node.data_ptr() != diff.medium.chem.data_ptr()
    for t in range(5):
        _, r_plain, term_p, trunc_p, info_p = plain.step(ag.forward(plain._get_current_obs))
        action = ag.differentiable_action(diff._get_current_obs)
        _, r_diff, term_d, trunc_d, info_d = diff.differentiable_step(action)
        assert r_plain == r_diff and (term_p, trunc_p) == (term_d, trunc_d) and info_p == info_d, t
        _same_state(_state(plain), _state(diff))
        node = diff.differentiable_chem()
        assert node is diff.medium.chem_node and node.grad_fn is not None and node is diff.differentiable_chem()
        assert np.array_equal(node.detach().cpu().numpy().view(np.uint32), diff.medium.chem.cpu().numpy().view(np.uint32))
    assert info_p['num_agents'] > 0 and float(diff.medium.chem.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 2. who deposited where
def ref_cells_of(medium, agents, slot=None):
    """The oracle's ownership on given (3, W, H) / (4, N) host arrays in slot order: RefEnv's cells and alive index, the reference's
    fancy-index assignment (the LAST alive slot in index order stays), entry n's cell if it is that slot."""
    a = np.asarray(agents)
    ref = R.RefEnv(medium, a)
    W, H = ref.field_size
    ix, iy = ref.cells_of(ref.agents[[0, 1]])
    idx = ref.alive_index()
    owner = np.full((W, H), -1, dtype=np.int64)
    owner[ix[idx], iy[idx]] = idx
    want = np.where((a[2] > 0) & (owner[ix, iy] == np.arange(a.shape[1])), ix * H + iy, -1).astype(np.int32)
    return want if slot is None else want[slot]


def _ref_cells(env, slot=None):
    """ref_cells_of on the device's coordinates."""
    return ref_cells_of(env.medium.to_numpy(), env.agents.to_numpy(), slot)


def _deposit_cells(env, agents_struct, N):
    buf = torch.full((N + TAIL,), SENT_I, dtype=torch.int32, device=DEV)
    m = env.medium.c_struct()
    L.check(L.lib.die_deposit_cells(C.byref(m), C.byref(agents_struct), _ptr(buf), stream_ptr(DEV)), 'die_deposit_cells')
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.all(h[N:] == SENT_I), 'die_deposit_cells wrote behind its N words'
    return h[:N]


def test_deposit_cells_against_the_oracle_ownership():
    W, H = 16, 64
    rs = np.random.RandomState(11)
    medium, agents = F.collision_world(W, H, rs)
    N = agents.shape[1]
    env = die.Env.from_numpy(medium, agents, die.Dynamics(), device=DEV, sort_every=0)
    perm = rs.permutation(N)
    epochs, winners, top = [], 0, 0
    for t in range(33):
        action = np.stack([rs.uniform(-0.05, 0.05, N), rs.uniform(-0.05, 0.05, N), rs.uniform(0.5, 2.0, N)]).astype(np.float32)
        action[:, [3, 7]] = action[:, [11]]                       # the three keep sharing a cell
        action[:, 5] = action[:, 2]                               # the dead slot stays where slot 2 stands
        env.step(action)
        assert env.agents.slot is None
        epochs.append(env.medium.epoch)
        want = _ref_cells(env)
        assert want[3] == -1 and want[7] == -1 and want[5] == -1 and want[6] == -1, t          # two losers, two dead slots
        top += int(want[11] >= 0)
        cx, cy = _array_cells(env)
        assert cx[3] == cx[7] == cx[11] and cy[3] == cy[7] == cy[11] and (cx[5], cy[5]) == (cx[2], cy[2]), t
        got = _deposit_cells(env, env.agents.c_struct(), N)
        assert np.array_equal(got, want), (t, np.flatnonzero(got != want)[:8])
        # the same world held in another array order, slot ids alongside
        A = env.agents
        p = torch.from_numpy(perm).to(DEV)
        x, y, alive, slot = A.x[p].contiguous(), A.y[p].contiguous(), A.alive[p].contiguous(), p.to(torch.int32).contiguous()
        got = _deposit_cells(env, L.Agents(N, _ptr(x), _ptr(y), _ptr(alive), _ptr(A.agent_food), _ptr(slot)), N)
        assert np.array_equal(got, _ref_cells(env, perm)), t
        winners += int((want >= 0).sum())
    assert max(epochs) == L.OWNER_EPOCH_MAX and sum(b < a for a, b in zip(epochs, epochs[1:])) == 1 and epochs.count(1) == 1   # wrapped once
    # 111 alive slots hop over 1024 cells: about six more lose a cell they walked onto, per step; slot 11 keeps its cell unless a
    # higher slot id walks onto it
    assert winners > 33 * 0.8 * N and top >= 17


def stepped_slot_env(W, H, N, rs):
    """An Env of N slots in slot order, about half of them alive anywhere on the plane, after one step of random hops and deposits:
    its claim plane is what die_deposit_cells reads.  Returns (env, x words, y words, alive) of the device's arrays after the step."""
    alive = rs.rand(N) < 0.5
    agents = np.stack([rs.rand(N), rs.rand(N), alive.astype(np.float64), np.ones(N)])
    occ = np.zeros((W, H))
    occ[R.cell(agents[0][alive], W), R.cell(agents[1][alive], H)] = 1.0
    env = die.Env.from_numpy(np.stack([occ, rs.rand(W, H), rs.rand(W, H)]), agents, die.Dynamics(), device=DEV, sort_every=0)
    env.step(np.stack([rs.uniform(-0.05, 0.05, N), rs.uniform(-0.05, 0.05, N), rs.uniform(0.5, 2.0, N)]).astype(np.float32))
    assert env.agents.slot is None and env.agents.N == N
    x, y, up = (t.cpu().numpy() for t in (env.agents.x, env.agents.y, env.agents.alive))
    return env, x.view(np.uint32), y.view(np.uint32), up


def test_deposit_cells_past_the_grid_cap():
    """Gap 2 of LABBOOK §33 (k_deposit_cells): 2 097 665 slots, more than the 8192 x 256 threads of the capped grid — every thread
    takes a second slot and the last 513 slots are reached only by that second trip.  About half the slots are alive on 256 x 256
    cells, so nearly every cell is shared and the highest alive slot id must own it whichever trip read it.  The claim plane is
    the one an Env of that many slots leaves after one step; the winners are the loop-free rule of tests/grad_midsize_shapes.py
    (checked against `ref_cells_of` in tests/test_grad_midsize_cpu.py).  In slot order, and permuted with a slot array."""
    (W, H), N = S.DEPOSIT_PLANE, S.SLOT_N
    rs = np.random.RandomState(21)
    env, x, y, up = stepped_slot_env(W, H, N, rs)
    A = env.agents
    want = S.winner_cells(W, H, x, y, up)
    n_alive, n_won = int((up > 0).sum()), int((want >= 0).sum())
    assert 0.4 * N < n_alive < 0.6 * N and up[-513:].any()
    assert n_won > 0.99 * W * H and n_won < n_alive // 8             # nearly every cell is owned, and by one of many standing on it
    assert (want[-513:] >= 0).any()                                  # the second trip alone reaches a winner
    got = _deposit_cells(env, A.c_struct(), N)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    perm = rs.permutation(N)
    p = torch.from_numpy(perm).to(DEV)
    xs, ys, al, slot = A.x[p].contiguous(), A.y[p].contiguous(), A.alive[p].contiguous(), p.to(torch.int32).contiguous()
    got = _deposit_cells(env, L.Agents(N, _ptr(xs), _ptr(ys), _ptr(al), _ptr(A.agent_food), _ptr(slot)), N)
    assert np.array_equal(got, want[perm]), np.flatnonzero(got != want[perm])[:8]
    assert np.array_equal(got, S.winner_cells(W, H, x[perm], y[perm], up[perm], perm))


# ------------------------------------------------------------------------------------------------ 3. the entry point
def _sentinel(n):
    return torch.full((n,), float(SENT), dtype=torch.float32, device=DEV)


def _step_backward(W, H, g, sigma, decay, cells, N=None, with_deposit=True, grad_chem=None):
    """One die_env_step_backward into sentinel buffers: (status, grad_chem buffer, grad_deposit buffer)."""
    N = (0 if cells is None else cells.numel()) if N is None else N
    gc = _sentinel(max(W * H, 0) + TAIL) if grad_chem is None else grad_chem
    gd = _sentinel(max(N, 0) + TAIL)
    rc = L.lib.die_env_step_backward(W, H, _ptr(g), sigma, decay, N, _ptr(cells), _ptr(gc), _ptr(gd) if with_deposit else None, stream_ptr(DEV))
    return rc, gc, gd


def _host(buf, n, what):
    h = buf.cpu().numpy()
    assert np.all(h[n:] == SENT), f'{what}: written behind what the call was given'
    return h[:n]


@pytest.mark.parametrize('W,H,sigma', [(24, 68, 0.8), (24, 68, 0.5), (17, 66, 0.5), (17, 66, 0.8), (8, 12, 0.8), (3, 5, 0.8), (16, 256, 1.2)])
def test_env_step_backward_entry_point(W, H, sigma):
    rs = np.random.RandomState(W * 1000 + H)
    decay, N = 0.1, 50
    g_host = rs.standard_normal((W, H)).astype(np.float32)
    cells_host = rs.randint(0, W * H, N).astype(np.int32)
    cells_host[rs.rand(N) < 0.3] = -1
    cells_host[:4] = [0, W * H - 1, -1, cells_host[4]]            # both ends of the plane, a loser, one cell read twice
    g, cells = torch.from_numpy(g_host).to(DEV), torch.from_numpy(cells_host).to(DEV)
    runs = [_step_backward(W, H, g, sigma, decay, cells) for _ in range(2)]
    field_only = [_step_backward(W, H, g, sigma, decay, cells, N=0), _step_backward(W, H, g, sigma, decay, cells, with_deposit=False),
                  _step_backward(W, H, g, sigma, decay, None, N=0, with_deposit=False)]
    # refusals: nothing may be written
    in_place = _step_backward(W, H, g, sigma, decay, cells, grad_chem=g)
    bad = [_step_backward(0, H, g, sigma, decay, cells), _step_backward(W, -1, g, sigma, decay, cells),
           _step_backward(W, H, g, sigma, decay, cells, N=-5), _step_backward(W, H, g, 0.0, decay, cells)]
    torch.cuda.synchronize()
    assert all(rc == 0 for rc, _, _ in runs + field_only), L.lib.die_last_error()
    gc = _host(runs[0][1], W * H, 'grad_chem')
    gd = _host(runs[0][2], N, 'grad_deposit')
    want_gd = np.where(cells_host >= 0, gc[np.maximum(cells_host, 0)], np.float32(0))
    assert np.array_equal(gd.view(np.uint32), want_gd.view(np.uint32))
    assert np.all(gd[cells_host < 0].view(np.uint32) == 0)       # exactly +0
    ref = F.diffuse_decay(torch.as_tensor(g_host.astype(np.float64)), sigma, decay).numpy().reshape(-1)
    err = float(np.abs(gc - ref).max() / max(1.0, np.abs(ref).max()))
    print(f'env_step_backward {W}x{H} sigma {sigma}: grad_chem apart from float64 by {err:.3e} of max(1, max|ref|) (ceiling {FWD_TOL:.0e})')
    assert err <= FWD_TOL
    assert np.array_equal(_host(runs[1][1], W * H, 'grad_chem'), gc) and np.array_equal(_host(runs[1][2], N, 'grad_deposit'), gd)
    for _, c2, d2 in field_only:                                  # the field part alone: same plane, grad_deposit untouched
        assert np.array_equal(_host(c2, W * H, 'grad_chem'), gc) and np.all(d2.cpu().numpy() == SENT)
    assert in_place[0] == -1
    assert np.array_equal(g.cpu().numpy(), g_host) and np.all(in_place[2].cpu().numpy() == SENT)
    for rc, c2, d2 in bad:
        assert rc == -1 and np.all(c2.cpu().numpy() == SENT) and np.all(d2.cpu().numpy() == SENT)


@pytest.mark.parametrize('N', S.GATHER_NS)
def test_env_step_backward_gathers_full_blocks(N):
    """Gap 1 of LABBOOK §33 (k_gather_cells): a workgroup takes 4 runs of 256 entries, n = base + q * 256, and no test had more than
    about 150 entries — q >= 1 had never loaded or stored, no second workgroup (N > 1024) and no second grid-stride trip
    (N > 8192 * 1024) had run.  Every size around a run, around a workgroup, four workgroups with a ragged last one, and 8 389 637
    entries (the second trip fills workgroup 0 and starts workgroup 1).  grad_deposit word for word against the device's own
    grad_chem; an index at or past W * H and INT32_MIN store +0; the tail stays; two runs give the same bits."""
    (W, H), sigma, decay = S.GATHER_PLANE, 0.8, 0.1
    g_host, cells_host = S.gather_case(N)
    g, cells = torch.from_numpy(g_host).to(DEV), torch.from_numpy(cells_host).to(DEV)
    runs = [_step_backward(W, H, g, sigma, decay, cells) for _ in range(2)]
    torch.cuda.synchronize()
    assert all(rc == 0 for rc, _, _ in runs), L.lib.die_last_error()
    gc = _host(runs[0][1], W * H, 'grad_chem')
    gd = _host(runs[0][2], N, 'grad_deposit')
    ref = F.diffuse_decay(torch.as_tensor(g_host.astype(np.float64)), sigma, decay).numpy().reshape(-1)
    assert float(np.abs(gc - ref).max() / max(1.0, np.abs(ref).max())) <= FWD_TOL
    want = S.gather_want(gc, cells_host)
    assert np.array_equal(gd.view(np.uint32), want.view(np.uint32)), np.flatnonzero(gd.view(np.uint32) != want.view(np.uint32))[:8]
    out = (cells_host < 0) | (cells_host >= W * H)
    assert np.all(gd[out].view(np.uint32) == 0)                   # exactly +0: losers, an index past the plane, INT32_MIN
    assert {int(S.INT32_MIN), W * H, -1} <= set(cells_host[:7].tolist()) and {int(S.INT32_MIN), W * H, -1} <= set(cells_host[-7:].tolist())
    assert 0.25 * N < out.sum() < 0.4 * N and np.count_nonzero(gd[~out]) == (~out).sum()      # the rest carries a gradient
    assert gd[0] == gc[0] and gd[1] == gc[W * H - 1] and gd[-1] == gc[0] and gd[-2] == gc[W * H - 1]
    assert np.array_equal(_host(runs[1][1], W * H, 'grad_chem').view(np.uint32), gc.view(np.uint32))
    assert np.array_equal(_host(runs[1][2], N, 'grad_deposit').view(np.uint32), gd.view(np.uint32))
    assert np.array_equal(cells.cpu().numpy(), cells_host)


def test_gather_scale_backward_past_the_grid_cap():
    """Gap 2 of LABBOOK §33 (k_gather_scale_backward): 2 097 665 slots, more than the capped grid's 8192 x 256 threads, on
    1028 x 1024 cells — two slots a cell on average.  Against the float64 sum of the fp32 products the device forms exactly: a cell
    with one non-zero term holds that term's bits, a cell with n terms is within (n - 1) * 2^-24 * sum|terms| (the worst case of an
    fp32 sum in any order; the atomics fix none), a cell without a term is +0.  Both kinds of cell occur in good number."""
    (W, H), N, coefs = S.SCATTER_PLANE, S.SLOT_N, S.SCATTER_COEFS
    x, y, grads = S.scatter_world(W, H, N, np.random.RandomState(31))
    xd, yd = (torch.from_numpy(v.view(np.int32).copy()).to(DEV) for v in (x, y))
    g_dev = torch.from_numpy(grads).to(DEV)
    planes = _sentinel(3 * W * H + TAIL)
    m = L.Medium(W, H, L.DIE_F32, 1, None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, None)         # the read-out reads the geometry only
    a = L.Agents(N, _ptr(xd), _ptr(yd), None, None, None)
    u = L.Action(N, g_dev[0].data_ptr(), g_dev[1].data_ptr(), g_dev[2].data_ptr())
    ptrs = (C.c_void_p * 3)(*[planes.data_ptr() + 4 * q * W * H for q in range(3)])
    L.check(L.lib.die_gather_scale_backward(C.byref(m), C.byref(a), C.byref(u), (C.c_float * 3)(*coefs), ptrs, stream_ptr(DEV)),
            'die_gather_scale_backward')
    torch.cuda.synchronize()
    got = _host(planes, 3 * W * H, 'grad planes')
    one, many, worst = S.check_scatter(got, *S.scatter_reference(W, H, x, y, grads, coefs))
    print(f'gather_scale_backward {N} slots on {W}x{H}: {one} cells with one term (bits), {many} with several: worst error {worst:.3f} of '
          f'the bound (n - 1) * 2^-24 * sum|terms|')
    assert one > 3 * W * H // 4 and many > 3 * W * H * 2 // 5        # about 0.32 and 0.47 of the 3 * W * H cells (1.6 terms a cell)
    assert np.array_equal(g_dev.cpu().numpy(), grads)


# ------------------------------------------------------------------------------------------------ 4. <A x, y> = <x, A^T y>
@pytest.mark.parametrize('sigma,radius', [(0.5, 2), (0.8, 3)])
def test_adjoint_identity_on_the_device(sigma, radius):
    W, H = 24, 68
    assert len(F.taps(sigma)) == 2 * radius + 1
    rs = np.random.RandomState(radius)
    medium, agents = F.collision_world(W, H, rs)
    N = agents.shape[1]
    c = rs.uniform(0.0, 1.0, (W, H)).astype(np.float32)
    d = rs.uniform(0.5, 2.0, N).astype(np.float32)
    g_host = rs.uniform(0.0, 1.0, (W, H)).astype(np.float32)
    medium[2] = c
    decay = 0.1
    env = die.Env.from_numpy(medium, agents, die.Dynamics(diffuse_sigma=sigma, rate_decay_chem=decay), device=DEV, sort_every=0)
    env.step(np.stack([np.zeros(N), np.zeros(N), d]).astype(np.float32))
    cells_host = _deposit_cells(env, env.agents.c_struct(), N)
    assert np.array_equal(cells_host, _ref_cells(env)) and (cells_host >= 0).sum() == N - 4       # two losers, two dead
    rc, gc, gd = _step_backward(W, H, torch.from_numpy(g_host).to(DEV), sigma, decay, torch.from_numpy(cells_host).to(DEV))
    torch.cuda.synchronize()
    assert rc == 0, L.lib.die_last_error()
    chem_next = env.medium.chem.cpu().numpy().astype(np.float64)
    grad_chem, grad_dep = _host(gc, W * H, 'grad_chem').reshape(W, H).astype(np.float64), _host(gd, N, 'grad_deposit').astype(np.float64)
    lhs = float((chem_next * g_host).sum())
    rhs = float((c.astype(np.float64) * grad_chem).sum() + (d.astype(np.float64) * grad_dep).sum())
    print(f'field step radius {radius}: <step(c, d), g> = {lhs:.9e}, <c, grad_chem> + <d, grad_deposit> = {rhs:.9e}, '
          f'apart by {abs(lhs - rhs) / abs(rhs):.2e} (ceiling {ID_TOL:.0e})')
    assert abs(lhs - rhs) <= ID_TOL * abs(rhs)
    assert float((d.astype(np.float64) * grad_dep).sum()) > 0.05 * rhs        # the deposit term is a real share of it


# ------------------------------------------------------------------------------------------------ 5. unrolled gradients
def _case_env(name, W, H):
    c = F.CASES[name]
    medium, agents = F.world_of(name, W, H)
    env = die.Env.from_numpy(medium, agents, die.Dynamics(diffuse_sigma=c['sigma'], rate_decay_chem=F.DECAY), device=DEV,
                             sort_every=c.get('sort_every', 0))
    ag = _nca(c['sizes'], c['boundary'], F.weights_of(name, W, H), with_agent_channel=c.get('with_agent_channel', True),
              p_agent_dropout=c.get('p', 0.), dropout_seed=c.get('seed'))
    assert ag.model.training
    return env, ag


def _frame(env, ag, name):
    c = F.CASES[name]
    m = env.medium.to_numpy()
    cx, cy = _array_cells(env)
    mask = D.mask(c['seed'], ag.dropout_step, env.medium.W, env.medium.H, c['p']).astype(np.float64) if 'p' in c else None
    return dict(occ=m[0], food=m[1], cx=cx, cy=cy, mask=mask), m[2]


def _one_per_cell(env):
    """bool (N,), array order: alive, and of the alive slots on its cell the one with the smallest slot id."""
    cx, cy = _array_cells(env)
    alive = env.agents.alive.cpu().numpy() > 0
    slot = np.arange(env.agents.N) if env.agents.slot is None else env.agents.slot.cpu().numpy()
    idx = np.argsort(slot)
    idx = idx[alive[idx]]
    _, first = np.unique((cx * env.medium.H + cy)[idx], return_index=True)
    keep = np.zeros(env.agents.N, dtype=bool)
    keep[idx[first]] = True
    return keep


def _unroll(name, W, H, T, plain_at=(), reset_before_backward=False, exact=False):
    """T steps on the device, the last action sensed on the final field, loss = <c, chem_T> + <u, action_T>, backward.
    Returns (device gradients, frames, cells, chem0, c, u, env).  u is drawn per SLOT and handed over in the array order of the moment
    action_T is sensed.  `plain_at`: steps taken by Env.step instead.  `exact`: u is zeroed on every slot but one alive slot per
    cell — the read-out's adjoint adds the slots of a cell with fp32 atomics in arrival order, and bits are fixed only when no two
    slots with a non-zero gradient share a cell (die_gather_scale_backward)."""
    env, ag = _case_env(name, W, H)
    N = env.agents.N
    cvec, u_slot = F.loss_vectors(name, W, H, N)
    frames, cells, chem0 = [], [], None
    for t in range(T):
        f, chem = _frame(env, ag, name)
        chem0 = chem if t == 0 else chem0
        frames.append(f)
        if t in plain_at:
            env.step(ag.forward(env._get_current_obs))
            assert env.medium.chem_node is None
            cells.append(None)
            continue
        env.differentiable_step(ag.differentiable_action(env._get_current_obs))
        node = env.differentiable_chem()
        cells.append(node.grad_fn.saved_tensors[0].cpu().numpy().copy())
    frames.append(_frame(env, ag, name)[0])
    u = u_slot if env.agents.slot is None else u_slot[:, env.agents.slot.cpu().numpy()]
    if exact:
        u = u * _one_per_cell(env)[None]
    action = ag.differentiable_action(env._get_current_obs)
    node = env.differentiable_chem()
    loss = (torch.as_tensor(cvec, dtype=torch.float32, device=DEV) * node).sum() + (torch.as_tensor(u, dtype=torch.float32, device=DEV) * action).sum()
    if reset_before_backward:
        env.reset()
    for q in ag.model.parameters():
        q.grad = None
    loss.backward()
    torch.cuda.synchronize()
    grads = [q.grad.detach().cpu().numpy().copy() for q in ag.model.parameters()]
    return grads, frames, cells, chem0, cvec, u, env


@pytest.mark.parametrize('W,H,T', F.SHAPES)
@pytest.mark.parametrize('name', sorted(F.CASES))
def test_unrolled_gradients_match_the_float64_model(name, W, H, T):
    c = F.CASES[name]
    grads, frames, cells, chem0, cvec, u, env = _unroll(name, W, H, T)
    if c.get('sort_every'):
        assert env.agents.slot is not None                        # the arrays were re-ordered between the steps
    if c.get('collisions'):
        assert all(int((cl < 0).sum()) >= 4 for cl in cells)      # two losers and two dead slots at least, every step
    ref = F.rollout(F.weights_of(name, W, H), c['boundary'], chem0, frames, cells, cvec, u, c['sigma'],
                    with_agent_channel=c.get('with_agent_channel', True))
    assert [g.shape for g in grads] == [g.shape for g in ref['grads']]
    chem_err = float(np.abs(env.medium.chem.cpu().numpy() - ref['chem']).max() / max(1.0, np.abs(ref['chem']).max()))
    err = [float(np.abs(g - w).max() / np.abs(w).max()) for g, w in zip(grads, ref['grads'])]
    print(f'field_step_grad {name} {W}x{H} T={T}: device', ' '.join(f'{e:.3e}' for e in err),
          f'(of max|grad_f64| per layer; ceiling {GRAD_TOL:.0e}); chem_T apart by {chem_err:.2e}')
    # the model followed the same trajectory: at most three fp32 steps, each within the forward ceiling of 1e-5, deposits of an
    # fp32 conv stack (1e-5 of their size) added in between
    assert chem_err <= 1e-4
    assert all(e <= GRAD_TOL for e in err), err
    # and the path through the field is a real share of this gradient: without it the model gives another one
    cut = F.rollout(F.weights_of(name, W, H), c['boundary'], chem0, frames, [np.full_like(cl, -1) for cl in cells], cvec, u, c['sigma'],
                    with_agent_channel=c.get('with_agent_channel', True))
    assert max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(cut['grads'], ref['grads'])) > 100 * GRAD_TOL


# ------------------------------------------------------------------------------------------------ 6. the graph's edges
def test_a_plain_step_cuts_the_graph():
    name, W, H = 'two_layers', 24, 68
    cut, *_ = _unroll(name, W, H, 3, plain_at=(1,), exact=True)   # differentiable, plain, differentiable
    short, *_ = _unroll(name, W, H, 3, plain_at=(0, 1), exact=True)   # plain, plain, differentiable: the same world, the shorter graph
    full, *_ = _unroll(name, W, H, 3, exact=True)
    for a, b, f in zip(cut, short, full):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert not np.array_equal(a, f)                           # (the uncut graph reaches further back)


def test_backward_after_reset_gives_the_same_bits():
    name, W, H = 'sort_every_1', 24, 68
    before, *_ = _unroll(name, W, H, 3, exact=True)
    after, *_, env = _unroll(name, W, H, 3, reset_before_backward=True, exact=True)
    assert env.medium.chem_node is None and env._steps == 0
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.abs(a).max() > 0


def test_without_a_node_the_library_calls_are_the_old_ones(monkeypatch):
    env, ag = _case_env('two_layers', 24, 68)
    calls = []
    orig = L.lib.die_conv2d_backward

    def spy(*args):
        calls.append(args)
        return orig(*args)

    monkeypatch.setattr(L.lib, 'die_conv2d_backward', spy)
    assert env.medium.chem_node is None
    ag.differentiable_sense(env.medium).sum().backward()
    assert len(calls) == 2 and calls[1][10] is None and calls[0][10] is not None      # last layer first; layer 1 without grad_in
    # a leaf node that asks for nothing changes nothing either
    del calls[:]
    node = env.differentiable_chem()
    ag.differentiable_sense(env.medium).sum().backward()
    assert len(calls) == 2 and calls[1][10] is None and node.grad is None
    # one that asks gets the chem channel's plane of the first layer's grad_in
    del calls[:]
    node.requires_grad_(True)
    ag.differentiable_sense(env.medium).sum().backward()
    torch.cuda.synchronize()
    assert len(calls) == 2 and calls[1][10] is not None
    assert node.grad is not None and tuple(node.grad.shape) == (24, 68) and float(node.grad.abs().max()) > 0
    # after a step the node is gone and the call is the old one again
    del calls[:]
    env.step(ag.forward(env._get_current_obs))
    assert env.medium.chem_node is None
    ag.differentiable_sense(env.medium).sum().backward()
    assert len(calls) == 2 and calls[1][10] is None


def test_a_stale_node_is_dropped_silently():
    env, ag = _case_env('two_layers', 24, 68)
    env.differentiable_step(ag.differentiable_action(env._get_current_obs))
    node = env.differentiable_chem()
    assert node.grad_fn is not None
    env.run(ag, 2)
    assert env.medium.chem_node is None
    fresh = env.differentiable_chem()
    assert fresh is not node and fresh.is_leaf and not fresh.requires_grad and torch.equal(fresh, env.medium.chem)
    env._medium_diffuse_decay()
    assert env.medium.chem_node is None


@pytest.mark.parametrize('what', ['fp16', 'reflect', 'sense_mask', 'frozen_indexer', 'decomposed', 'shape', 'dtype', 'host', 'numpy'])
def test_refusals_raise_before_any_launch(what):
    W, H = 16, 64
    kw, dyn = {}, {}
    if what == 'fp16':
        kw['field_dtype'] = torch.float16
    dyn = {'reflect': dict(diffuse_mode='reflect'), 'sense_mask': dict(apply_sense_mask=True),
           'frozen_indexer': dict(agents_die=True, compat='reference')}.get(what, {})
    env = die.Env((W, H), die.Dynamics(**dyn), seed=2, device=DEV, **kw)
    N = env.agents.N
    action = torch.zeros((3, N), dtype=torch.float32, device=DEV)
    if what == 'shape':
        action = torch.zeros((3, N + 1), dtype=torch.float32, device=DEV)
    elif what == 'dtype':
        action = action.double()
    elif what == 'host':
        action = action.cpu()
    elif what == 'numpy':
        action = np.zeros((3, N), dtype=np.float32)
    elif what == 'decomposed':
        env.medium.world = (2 * W, H, 0, 0)
    before, steps = _state(env), env._steps
    with pytest.raises(NotImplementedError, match='differentiable_step'):
        env.differentiable_step(action)
    if what in ('fp16', 'reflect', 'sense_mask', 'frozen_indexer', 'decomposed'):
        with pytest.raises(NotImplementedError, match='differentiable_chem'):
            env.differentiable_chem()
    env.medium.world = None
    _same_state(before, _state(env))
    assert env._steps == steps and env.medium.chem_node is None
