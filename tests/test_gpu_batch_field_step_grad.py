"""The batched step adjoint on the GPU (die_deposit_cells_batch, die_env_step_backward_batch, die_nca_backward_batch_inputs behind
`BatchedEnv.differentiable_step` / `differentiable_chem` and the chem node entering `BatchedNeuralAutomataAgent.differentiable_sense`):
every layer against what already exists — the stand-alone path, replica by replica, bit for bit — and the unrolled gradients against
the float64 torch model of tests/field_step_batch_model.py.

Ceilings, none of them taken from what the device gives:
  * tests 1, 2, 4, 6 and the twin half of test 5: bits, compared exactly;
  * test 3: |<step(c, d), g> - (<c, grad_chem> + <d, grad_deposit>)| <= 1e-6 of the right-hand side per replica, the ceiling
    tests/test_gpu_field_step_grad.py holds the stand-alone call to (c, d, g positive: no term cancels);
  * test 5: per candidate and weight tensor max|grad_dev - grad_f64| <= 1e-4 * max|grad_f64|, the stand-alone rollout's ceiling.

Every ctypes call writes into buffers with a sentinel tail that must come back untouched.  Shapes: 24 x 68 straddles conv tiles with
H % 4 == 0, 16 x 64 is one tile, 8 x 12 is smaller than one (sigma 0.8 -> radius 3); R = 3 with differing n[r], R = 6 as 2
candidates x 3 worlds, R = 64 once (the end of the index list of a sweep launch and of n[64]).  The entry points at full blocks
(LABBOOK §33; sizes in tests/grad_midsize_shapes.py): the batched gather at a stride of 3077 entries, die_deposit_cells_batch and
die_gather_scale_backward_batch with a row of 2 097 665 slots beside short ones."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch
from torch.nn.utils import parameters_to_vector

import die_amd as die
from die_amd import _lib as L
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent
from die_amd.device_array import DeviceAction, _ptr, stream_ptr
from tests import dropout_model as D
from tests import field_step_adjoint_model as F
from tests import field_step_batch_model as B
from tests import grad_midsize_shapes as S
from tests.test_gpu_batch_step_action import CASES as WORLDS, _cell, build, draw_actions

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ID_TOL, GRAD_TOL = 1e-6, 1e-4
SENT = np.float32(-7.25e7)
SENT_I = 0x5A5A5A5A
TAIL = 64


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. who deposited where
@pytest.mark.parametrize('name', ['f32_alive', 'f32_agents_die', 'f16_rows_flow_die_fixed'])
def test_deposit_cells_batch_is_deposit_cells_per_replica(name):
    case = WORLDS[name]
    benv, twins = build(case)
    actions = draw_actions(case, benv)
    dev_actions = torch.from_numpy(actions).to(benv.device)
    stride, losers, starved = benv.Nmax, [0] * benv.R, 0
    for t in range(actions.shape[0]):
        alive_before = benv.alive.clone()
        benv.step_action(dev_actions[t])
        buf = torch.full((benv.R * stride + TAIL,), SENT_I, dtype=torch.int32, device=benv.device)
        m, a, _, b = benv._structs()
        L.check(L.lib.die_deposit_cells_batch(C.byref(m), C.byref(a), C.byref(b), _ptr(buf), stream_ptr(benv.device)), 'die_deposit_cells_batch')
        got = buf.cpu().numpy()
        assert np.all(got[benv.R * stride:] == SENT_I), 'written behind R * agent_stride words'
        got = got[:benv.R * stride].reshape(benv.R, stride)
        died = (alive_before > 0) & (benv.alive == 0)
        for r, env in enumerate(twins):
            k = benv.n[r]
            act = DeviceAction(k, env.device)
            act.data = dev_actions[t, :, r, :k].contiguous()
            env.step(act)
            want = torch.full((k + TAIL,), SENT_I, dtype=torch.int32, device=env.device)
            ms, as_ = env.medium.c_struct(), env.agents.c_struct()
            L.check(L.lib.die_deposit_cells(C.byref(ms), C.byref(as_), _ptr(want), stream_ptr(env.device)), 'die_deposit_cells')
            want = want.cpu().numpy()[:k]
            assert np.array_equal(got[r, :k], want), (t, r)
            assert np.all(got[r, k:] == -1), (t, r, 'padding')
            alive = env.agents.alive.cpu().numpy() > 0
            losers[r] += int((alive & (want < 0)).sum())
            gone = died[r, :k].cpu().numpy()
            assert np.all(want[gone] == -1)                         # starved by this very step: dead when the record is made
            starved += int(gone.sum())
    assert all(losers), losers                                      # every replica had alive slots that lost a shared cell
    if case.get('agents_die'):
        assert starved > 0


def test_deposit_cells_batch_past_the_grid_cap():
    """Gap 2 of LABBOOK §33 (k_deposit_cells_batch): one launch sized by the largest row, n = (2 097 665, 65 537, 300) at stride
    2 097 665 — row 0 strides through the capped 8192-workgroup grid a second time, rows 1 and 2 end after 257 and 2 workgroups and
    write -1 from there on.  Every replica's claim plane and arrays are those of a stand-alone Env of n[r] slots after one step;
    replica r equals die_deposit_cells on that Env and the loop-free winners' rule, the padding (alive slots on real cells) is -1."""
    from tests.test_gpu_field_step_grad import stepped_slot_env
    (W, H), n, R = S.DEPOSIT_PLANE, S.DEPOSIT_BATCH_N, 3
    stride = max(n)
    rs = np.random.RandomState(23)
    owner = torch.zeros((R, W * H), dtype=torch.int64, device=DEV)
    x = torch.from_numpy(rs.randint(-2 ** 31, 2 ** 31, (R, stride)).astype(np.int32)).to(DEV)      # the padding: alive, anywhere
    y = torch.from_numpy(rs.randint(-2 ** 31, 2 ** 31, (R, stride)).astype(np.int32)).to(DEV)
    alive = torch.ones((R, stride), dtype=torch.uint8, device=DEV)
    wants, epoch = [], None
    for r in range(R):
        env, xw, yw, up = stepped_slot_env(W, H, n[r], rs)
        epoch = env.medium.epoch if epoch is None else epoch
        assert env.medium.epoch == epoch
        owner[r].copy_(env.medium.owner.view(-1))
        x[r, :n[r]].copy_(env.agents.x); y[r, :n[r]].copy_(env.agents.y); alive[r, :n[r]].copy_(env.agents.alive)
        want = torch.full((n[r] + TAIL,), SENT_I, dtype=torch.int32, device=DEV)
        ms, as_ = env.medium.c_struct(), env.agents.c_struct()
        L.check(L.lib.die_deposit_cells(C.byref(ms), C.byref(as_), _ptr(want), stream_ptr(DEV)), 'die_deposit_cells')
        want = want.cpu().numpy()
        assert np.all(want[n[r]:] == SENT_I)
        assert np.array_equal(want[:n[r]], S.winner_cells(W, H, xw, yw, up)), r
        assert (want[:n[r]] >= 0).sum() > min(n[r] // 4, W * H // 2)                  # winners, and in the crowded rows losers
        assert n[r] < W * H // 4 or ((want[:n[r]] < 0) & (up > 0)).sum() > n[r] // 16
        wants.append(want[:n[r]])
        del env
    buf = torch.full((R * stride + TAIL,), SENT_I, dtype=torch.int32, device=DEV)
    m = L.Medium(W, H, L.DIE_F32, epoch, _ptr(owner), None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, None)
    a = L.Agents(stride, _ptr(x), _ptr(y), _ptr(alive), None, None)
    b = L.Batch(R, 0, W * H, stride, 1, (C.c_int64 * 64)(*(list(n) + [0] * (64 - R))))
    L.check(L.lib.die_deposit_cells_batch(C.byref(m), C.byref(a), C.byref(b), _ptr(buf), stream_ptr(DEV)), 'die_deposit_cells_batch')
    got = buf.cpu().numpy()
    assert np.all(got[R * stride:] == SENT_I), 'written behind R * agent_stride words'
    got = got[:R * stride].reshape(R, stride)
    for r in range(R):
        assert np.array_equal(got[r, :n[r]], wants[r]), (r, np.flatnonzero(got[r, :n[r]] != wants[r])[:8])
        assert np.all(got[r, n[r]:] == -1), (r, 'padding')


def test_gather_scale_backward_batch_past_the_grid_cap():
    """Gap 2 of LABBOOK §33 (k_gather_scale_backward_batch): the launch is sized by the largest n[r] — n = (2 097 665, 300) on
    1028 x 1024, so row 0 takes the stride loop's second trip while row 1's threads idle from its second workgroup on.  The
    reference and the bound are those of the stand-alone test (float64 over the exact fp32 products; one term: its bits; n terms:
    (n - 1) * 2^-24 * sum|terms|); the planes of the short replica are +0 wherever none of its 300 slots stands."""
    (W, H), n, coefs, R = S.SCATTER_PLANE, S.SCATTER_BATCH_N, S.SCATTER_COEFS, 2
    stride = max(n)
    worlds = [S.scatter_world(W, H, stride, np.random.RandomState(41 + r)) for r in range(R)]        # (the padding holds slots and gradients too)
    x, y = (torch.from_numpy(np.stack([w[q] for w in worlds]).view(np.int32).copy()).to(DEV) for q in (0, 1))
    grads = np.ascontiguousarray(np.stack([w[2] for w in worlds], axis=1))                           # (3, R, stride)
    g_dev = torch.from_numpy(grads).to(DEV)
    planes = _sentinel(R * 3 * W * H + TAIL)
    m = L.Medium(W, H, L.DIE_F32, 1, None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, None)
    a = L.Agents(stride, _ptr(x), _ptr(y), None, None, None)
    u = L.Action(stride, g_dev[0].data_ptr(), g_dev[1].data_ptr(), g_dev[2].data_ptr())
    b = L.Batch(R, 0, W * H, stride, 1, (C.c_int64 * 64)(*(list(n) + [0] * (64 - R))))
    L.check(L.lib.die_gather_scale_backward_batch(C.byref(m), C.byref(a), C.byref(b), C.byref(u), (C.c_float * 3)(*coefs), _ptr(planes),
                                                  3 * W * H, stream_ptr(DEV)), 'die_gather_scale_backward_batch')
    torch.cuda.synchronize()
    got = planes.cpu().numpy()
    assert np.all(got[R * 3 * W * H:] == SENT), 'written behind the planes'
    got = got[:R * 3 * W * H].reshape(R, 3, W * H)
    for r in range(R):
        xw, yw, gr = (v[..., :n[r]] for v in worlds[r])
        total, mag, count = S.scatter_reference(W, H, xw, yw, gr, coefs)
        one, many, worst = S.check_scatter(got[r], total, mag, count, f'replica {r}')
        print(f'gather_scale_backward_batch replica {r}, {n[r]} slots on {W}x{H}: {one} cells with one term (bits), {many} with several: '
              f'worst error {worst:.3f} of the bound')
        if r == 0:
            assert one > 3 * W * H // 4 and many > 3 * W * H * 2 // 5
        else:
            assert 0 < np.count_nonzero(got[r]) <= 3 * n[r] and one > 2 * n[r]     # 300 slots' terms and nothing of replica 0's


# ------------------------------------------------------------------------------------------------ 2. the entry point
def _rows_tables(dyns, W, H):
    R = len(dyns)
    host = (L.DynamicsRow * R)()
    structs = (L.Dynamics * R)(*[L.Dynamics(d.rate_feed, d.rate_decay_chem, d.diffuse_sigma, L.DIE_BOUNDARY_WRAP, L.DIE_COST_LINEAR, 0.02, 0.01,
                                            int(d.food_infinite), 0, 0, 0, 0) for d in dyns])
    L.check(L.lib.die_dynamics_rows(structs, R, W, H, host), 'die_dynamics_rows')
    return torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(DEV), host


def _sentinel(n):
    return torch.full((n,), float(SENT), dtype=torch.float32, device=DEV)


BACKWARD_CASES = {
    'shared_radius_2': dict(shape=(24, 68), R=3, sigma=0.5),
    'shared_radius_3': dict(shape=(24, 68), R=3, sigma=0.8),
    'one_tile_one_replica': dict(shape=(16, 64), R=1, sigma=0.8),
    'rows_both_radii': dict(shape=(24, 68), R=5, rows=True),
    'rows_one_radius': dict(shape=(8, 12), R=2, rows=True, one_radius=True),
    '64_replicas': dict(shape=(8, 12), R=64, sigma=0.8),
    '64_replicas_rows': dict(shape=(8, 12), R=64, rows=True),
}


@pytest.mark.parametrize('name', list(BACKWARD_CASES))
def test_env_step_backward_batch_is_env_step_backward_per_replica(name):
    case = BACKWARD_CASES[name]
    (W, H), R = case['shape'], case['R']
    rs = np.random.RandomState(W * 1000 + H + R)
    stride = 50
    n = [stride - (r % 4) * 7 for r in range(R)]                    # differing counts: padding behind most replicas
    dyns = [die.Dynamics(diffuse_sigma=case.get('sigma', (0.8 if case.get('one_radius') else (0.8, 0.5)[r % 2])),
                         rate_decay_chem=(0.1, 0.025, 0.06)[r % 3] if case.get('rows') else 0.1) for r in range(R)]
    rows_dev, rows_host = _rows_tables(dyns, W, H) if case.get('rows') else (None, None)
    if case.get('rows') and not case.get('one_radius'):
        assert {rows_host[r].radius for r in range(R)} == {2, 3}
    g_host = rs.standard_normal((R, W, H)).astype(np.float32)
    cells_host = rs.randint(0, W * H, (R, stride)).astype(np.int32)
    cells_host[rs.rand(R, stride) < 0.3] = -1
    cells_host[:, :5] = [0, W * H - 1, -1, W * H, 7]                # both ends of a plane, a loser, one past the plane (counts as -1)
    g, cells = torch.from_numpy(g_host).to(DEV), torch.from_numpy(cells_host).to(DEV)
    b = L.Batch(R, 0, W * H, stride, 1, (C.c_int64 * 64)(*(n + [0] * (64 - R))))
    tables = (None, None) if rows_dev is None else (_ptr(rows_dev), rows_host)

    def call(with_deposit=True):
        gc, gd = _sentinel(R * W * H + TAIL), _sentinel(R * stride + TAIL)
        rc = L.lib.die_env_step_backward_batch(W, H, C.byref(b), _ptr(g), 0.8 if rows_dev is not None else dyns[0].diffuse_sigma,
                                               dyns[0].rate_decay_chem, *tables, _ptr(cells), _ptr(gc), _ptr(gd) if with_deposit else None,
                                               stream_ptr(DEV))
        assert rc == 0, L.lib.die_last_error()
        return gc, gd

    runs = [call(), call()]
    field_only = call(with_deposit=False)
    torch.cuda.synchronize()
    gc, gd = runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy()
    assert np.all(gc[R * W * H:] == SENT) and np.all(gd[R * stride:] == SENT), 'written behind the buffers'
    assert np.array_equal(runs[1][0].cpu().numpy().view(np.uint32), gc.view(np.uint32))             # two runs, the same bits
    assert np.array_equal(runs[1][1].cpu().numpy().view(np.uint32), gd.view(np.uint32))
    assert np.array_equal(field_only[0].cpu().numpy().view(np.uint32), gc.view(np.uint32)) and np.all(field_only[1].cpu().numpy() == SENT)
    assert np.array_equal(g.cpu().numpy(), g_host) and np.array_equal(cells.cpu().numpy(), cells_host)
    gc, gd = gc[:R * W * H].reshape(R, W * H), gd[:R * stride].reshape(R, stride)
    for r in range(R):
        want_c, want_d = _sentinel(W * H + TAIL), _sentinel(n[r] + TAIL)
        rc = L.lib.die_env_step_backward(W, H, _ptr(g[r]), dyns[r].diffuse_sigma, dyns[r].rate_decay_chem, n[r], _ptr(cells[r]), _ptr(want_c),
                                         _ptr(want_d), stream_ptr(DEV))
        assert rc == 0, L.lib.die_last_error()
        assert np.array_equal(gc[r].view(np.uint32), want_c.cpu().numpy()[:W * H].view(np.uint32)), r
        assert np.array_equal(gd[r, :n[r]].view(np.uint32), want_d.cpu().numpy()[:n[r]].view(np.uint32)), r
        assert np.all(gd[r, n[r]:].view(np.uint32) == 0), (r, 'padding')                          # exactly +0
        assert gd[r, 2] == 0 and gd[r, 3] == 0 and gd[r, 0] == gc[r, 0] and gd[r, 1] == gc[r, W * H - 1]
    assert np.abs(gc).max() > 0


def test_env_step_backward_batch_gathers_full_blocks():
    """Gap 1 of LABBOOK §33 (k_gather_cells_batch): R = 3 rows of agent_stride = 3 * 1024 + 5 entries with n = (3077, 1025, 0) —
    four workgroups a row, every run q = 0 .. 3 loaded and stored, row 1's n[r] inside workgroup 1's first run while agent_stride
    goes on (the padding store of +0 from later runs and later workgroups), row 2 padding only.  Behind n[r] the cells hold valid
    indices of the plane: read as an index they would fetch a gradient.  Replica r is the stand-alone call on its row, bit for bit."""
    (W, H), R, stride, n = S.GATHER_PLANE, 3, S.GATHER_BATCH_STRIDE, S.GATHER_BATCH_N
    sigma, decay = 0.8, 0.1
    g_host, cells_host, junk = S.gather_batch_case()
    g, cells = torch.from_numpy(g_host).to(DEV), torch.from_numpy(cells_host).to(DEV)
    b = L.Batch(R, 0, W * H, stride, 1, (C.c_int64 * 64)(*(list(n) + [0] * (64 - R))))
    runs = []
    for _ in range(2):
        gc, gd = _sentinel(R * W * H + TAIL), _sentinel(R * stride + TAIL)
        rc = L.lib.die_env_step_backward_batch(W, H, C.byref(b), _ptr(g), sigma, decay, None, None, _ptr(cells), _ptr(gc), _ptr(gd), stream_ptr(DEV))
        assert rc == 0, L.lib.die_last_error()
        runs.append((gc, gd))
    torch.cuda.synchronize()
    gc, gd = runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy()
    assert np.all(gc[R * W * H:] == SENT) and np.all(gd[R * stride:] == SENT), 'written behind the buffers'
    assert np.array_equal(runs[1][0].cpu().numpy().view(np.uint32), gc.view(np.uint32))             # two runs, the same bits
    assert np.array_equal(runs[1][1].cpu().numpy().view(np.uint32), gd.view(np.uint32))
    assert np.array_equal(cells.cpu().numpy(), cells_host)
    gc, gd = gc[:R * W * H].reshape(R, W * H), gd[:R * stride].reshape(R, stride)
    for r in range(R):
        want_c, want_d = _sentinel(W * H + TAIL), _sentinel(n[r] + TAIL)
        rc = L.lib.die_env_step_backward(W, H, _ptr(g[r]), sigma, decay, n[r], _ptr(cells[r]), _ptr(want_c), _ptr(want_d), stream_ptr(DEV))
        assert rc == 0, L.lib.die_last_error()
        want_d = want_d.cpu().numpy()
        assert np.all(want_d[n[r]:] == SENT)
        assert np.array_equal(gc[r].view(np.uint32), want_c.cpu().numpy()[:W * H].view(np.uint32)), r
        assert np.array_equal(gd[r, :n[r]].view(np.uint32), want_d[:n[r]].view(np.uint32)), r
        assert np.array_equal(gd[r, :n[r]].view(np.uint32), S.gather_want(gc[r], cells_host[r, :n[r]]).view(np.uint32)), r
        assert np.all(gd[r, n[r]:].view(np.uint32) == 0), (r, 'padding')                          # exactly +0
        assert junk[r, n[r]:].all() and np.count_nonzero(S.gather_want(gc[r], cells_host[r, n[r]:])) == stride - n[r]   # (read, it would show)
        assert n[r] == 0 or np.count_nonzero(gd[r, :n[r]]) > n[r] // 2


# ------------------------------------------------------------------------------------------------ 3. <A x, y> = <x, A^T y>
@pytest.mark.parametrize('listed', [False, True])
def test_adjoint_identity_per_replica_on_the_device(listed):
    W, H, R = 24, 68, 4
    dyns = [die.Dynamics(diffuse_sigma=(0.8, 0.5)[r % 2] if listed else 0.8, rate_decay_chem=(0.1, 0.025, 0.06)[r % 3] if listed else 0.1,
                         init_agent_ratio=0.15) for r in range(R)]
    benv = BatchedEnv((W, H), dyns if listed else dyns[0], replicas=R, seed=3)
    rs = np.random.RandomState(7 + listed)
    c = torch.from_numpy(rs.uniform(0.0, 1.0, (R, W, H)).astype(np.float32)).to(DEV)
    g = torch.from_numpy(rs.uniform(0.0, 1.0, (R, W, H)).astype(np.float32)).to(DEV)
    benv.chem.copy_(c)
    case = dict(shape=(W, H), seed=5)
    action = torch.from_numpy(draw_actions(case, benv, 1)[0]).to(DEV)        # hops: shared cells, losers; deposits in (0.5, 2)
    node = benv.differentiable_chem().requires_grad_(True)
    assert torch.equal(node, c)
    leaf = action.clone().nan_to_num_(0.0).requires_grad_(True)
    benv.differentiable_step(leaf)
    out = benv.differentiable_chem()
    assert out.grad_fn is not None and torch.equal(out, benv.chem)
    cells = out.grad_fn.saved_tensors[0].cpu().numpy()
    out.backward(g)
    torch.cuda.synchronize()
    assert torch.all(leaf.grad[:2] == 0)
    for r in range(R):
        k = benv.n[r]
        assert (cells[r, :k] >= 0).sum() < k and np.all(cells[r, k:] == -1)      # losers exist
        d = leaf[2, r, :k].detach().double()
        lhs = float((benv.chem[r].double() * g[r].double()).sum())
        dep = float((d * leaf.grad[2, r, :k].double()).sum())
        rhs = float((c[r].double() * node.grad[r].double()).sum()) + dep
        print(f'batched field step replica {r}: <step(c, d), g> = {lhs:.9e}, <c, grad_chem> + <d, grad_deposit> = {rhs:.9e}, '
              f'apart by {abs(lhs - rhs) / abs(rhs):.2e} (ceiling {ID_TOL:.0e})')
        assert abs(lhs - rhs) <= ID_TOL * abs(rhs)
        assert dep > 0.05 * rhs                                     # the deposit term is a real share of it
        assert torch.all(leaf.grad[2, r, k:] == 0)


# ------------------------------------------------------------------------------------------------ 4. the first layer's input gradient
def _template(sizes=(3, 3), boundary='circular', weights=None, seed=0, **kw):
    torch.manual_seed(seed)
    ag = die.NeuralAutomataAgent(kernel_sizes=sizes, boundary=boundary, scale=F.COEFS[0], deposit=F.COEFS[2], **kw)
    with torch.no_grad():
        for i, q in enumerate(ag.model.parameters()):
            if weights is None:
                q.uniform_(-0.5, 0.5)
            else:
                q.copy_(torch.as_tensor(weights[i], dtype=torch.float32))
    return ag


def _rows_of(template, C_):
    """(C, P): candidate c's weights are the template's plus c / 100."""
    v = parameters_to_vector(template.model.parameters()).detach()
    return torch.stack([v + 0.01 * c for c in range(C_)])


INPUT_CASES = {
    'two_3x3_circular': dict(sizes=(3, 3), boundary='circular'),
    'one_5x5_zeros': dict(sizes=(5,), boundary='zeros'),
    'no_agent_channel': dict(sizes=(3, 3), boundary='circular', with_agent_channel=False),
    'dropout': dict(sizes=(3, 3), boundary='circular', p_agent_dropout=0.25),
}


@pytest.mark.parametrize('name', list(INPUT_CASES))
def test_backward_batch_inputs_against_the_existing_calls(name):
    W, H, R = 24, 68, 3
    kw = INPUT_CASES[name]
    drop = dict(dropout_seed=7, dropout_seed_stride=3) if 'p_agent_dropout' in kw else {}
    dyn = lambda: die.Dynamics(diffuse_sigma=0.8, init_agent_ratio=0.15)
    benv = BatchedEnv((W, H), dyn(), replicas=R, seed=3)
    benv.chem.copy_(torch.rand((R, W, H), device=DEV))
    template = _template(**kw)
    rs = np.random.RandomState(3)
    gs = torch.from_numpy(rs.standard_normal((R, 3, W, H)).astype(np.float32)).to(DEV)

    def batched(with_node):
        pop = BatchedNeuralAutomataAgent(benv, template, _rows_of(template, R), **drop)
        pop.parameters.requires_grad_(True)
        benv.chem_node = None
        node = benv.differentiable_chem().requires_grad_(True) if with_node else None
        (pop.differentiable_sense() * gs).sum().backward()
        torch.cuda.synchronize()
        return pop, _bits(pop.parameters.grad), None if node is None else node.grad

    pop, plain, _ = batched(False)
    _, with_inputs, node_grad = batched(True)
    assert np.array_equal(plain, with_inputs)                       # die_nca_backward_batch's weight gradient, bit for bit
    assert tuple(node_grad.shape) == (R, W, H) and float(node_grad.abs().max()) > 0
    for r in range(R):
        env = die.Env((W, H), dyn(), seed=benv.seeds[r], max_agents='alive', device=DEV, sort_every=0, pic=False)
        env.medium.upload_channel('chem1', benv.chem[r].cpu().numpy())
        ag = pop.replica_agent(r)
        node = env.differentiable_chem().requires_grad_(True)
        (ag.differentiable_sense(env.medium) * gs[r]).sum().backward()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(node_grad[r]), _bits(node.grad)), r
        twin = parameters_to_vector([q.grad for q in ag.model.parameters()])
        assert np.array_equal(_bits(pop.parameters.grad[r]), _bits(twin)), r


# ------------------------------------------------------------------------------------------------ 5. unrolled gradients
def _worlds(name, W, H, R):
    """R made-up worlds of a case (tests/field_step_adjoint_model.py's generators, one random stream per replica): same slot count,
    a fifth of the slots dead (three alive slots on one cell in the collision case)."""
    make = F.collision_world if F.CASES[name].get('collisions') else F.plain_world
    return [make(W, H, np.random.RandomState(100 + 17 * r)) for r in range(R)]


def _batch_of(worlds, dyns, listed):
    """(batch, twins): a fixed-layout batch whose replicas are set to the given worlds, and the stand-alone Env of every world.  The
    batch is built from seeds (the only constructor) with as many slots as the worlds hold, then every replica's state is overwritten
    with its twin's, as BatchedEnv.__init__ copies the Envs it builds."""
    (_, W, H), N, R = worlds[0][0].shape, worlds[0][1].shape[1], len(worlds)
    twins = [die.Env.from_numpy(m, a, dyns[r], device=DEV, sort_every=0, pic=False) for r, (m, a) in enumerate(worlds)]
    seeded = [dataclasses.replace(d, init_agent_ratio=0.02) for d in dyns]      # (few seeded agents: they fit the worlds' slot count)
    benv = BatchedEnv((W, H), seeded if listed else seeded[0], replicas=R, seed=1, max_agents=N)
    assert benv.n == [N] * R and benv.epoch == 1
    for r, e in enumerate(twins):
        assert e.medium.epoch == 1 and e.agents.N == N
        e.medium._ensure_owner()
        benv.owner[r].copy_(e.medium.owner); benv.food[r].copy_(e.medium.food); benv.chem[r].copy_(e.medium.chem)
        benv.x[r].copy_(e.agents.x); benv.y[r].copy_(e.agents.y)
        benv.alive[r].copy_(e.agents.alive); benv.agent_food[r].copy_(e.agents.agent_food)
    return benv, twins


def _cells_of(x, y, W, H):
    return _cell(x.cpu().numpy().view(np.uint32), W), _cell(y.cpu().numpy().view(np.uint32), H)


def _one_per_cell(cx, cy, alive, H):
    """bool (N,): alive, and of the alive slots on its cell the one with the smallest slot id."""
    idx = np.flatnonzero(alive)
    _, first = np.unique((cx * H + cy)[idx], return_index=True)
    keep = np.zeros(cx.size, dtype=bool)
    keep[idx[first]] = True
    return keep


UNROLL = {name: dict(case=name) for name in sorted(F.CASES) if 'sort_every' not in F.CASES[name]}     # (a batch never re-sorts)
UNROLL['episodes_2x3'] = dict(case='two_layers', R=6, episodes=3)
UNROLL['per_replica_dynamics'] = dict(case='collisions', listed=True)


def _unroll(key, T, reset_before_backward=False, plain_at=(), with_twins=True):
    spec = UNROLL[key]
    name, W, H = spec['case'], 24, 68
    c = F.CASES[name]
    R, E = spec.get('R', 3), spec.get('episodes', 1)
    listed = bool(spec.get('listed'))
    dyns = [die.Dynamics(diffuse_sigma=(c['sigma'], 0.5, 0.8)[r % 3] if listed else c['sigma'],
                         rate_decay_chem=(F.DECAY, 0.025, 0.06)[r % 3] if listed else F.DECAY) for r in range(R)]
    benv, twins = _batch_of(_worlds(name, W, H, R), dyns, listed)
    N = benv.Nmax
    template = _template(c['sizes'], c['boundary'], F.weights_of(name, W, H), with_agent_channel=c.get('with_agent_channel', True),
                         p_agent_dropout=c.get('p', 0.))
    drop = dict(dropout_seed=c['seed'], dropout_seed_stride=5) if 'p' in c else {}
    pop = BatchedNeuralAutomataAgent(benv, template, _rows_of(template, R // E), episodes=E, **drop)
    pop.parameters.requires_grad_(True)
    rs = np.random.RandomState(T)
    cvec = [F.loss_vectors(name, W, H, N)[0] * rs.uniform(0.5, 1.5) for r in range(R)]
    uvec = [F.loss_vectors(name, W, H, N)[1] * rs.uniform(0.5, 1.5) for r in range(R)]

    def frames_now():
        out = []
        for r in range(R):
            m, _ = benv.replica_numpy(r)
            cx, cy = _cells_of(benv.x[r], benv.y[r], W, H)
            mask = D.mask(c['seed'] + 5 * r, pop.dropout_step, W, H, c['p']).astype(np.float64) if 'p' in c else None
            out.append((dict(occ=m[0], food=m[1], cx=cx, cy=cy, mask=mask), m[2]))
        return out

    frames, cells, results = [[] for _ in range(R)], [[] for _ in range(R)], []
    chem0 = None
    for t in range(T):
        now = frames_now()
        chem0 = [ch for _, ch in now] if t == 0 else chem0
        for r in range(R):
            frames[r].append(now[r][0])
        if t in plain_at:
            benv.step(pop)
            assert benv.chem_node is None
            continue
        results.append(benv.differentiable_step(pop.differentiable_action()).clone())
        recorded = benv.differentiable_chem().grad_fn.saved_tensors[0].cpu().numpy()
        for r in range(R):
            cells[r].append(recorded[r].copy())
    now = frames_now()
    for r in range(R):
        frames[r].append(now[r][0])
    # bits are fixed only where no two slots with a non-zero gradient share a cell (the read-out's adjoint adds them with fp32
    # atomics in arrival order, LABBOOK §20): u is zeroed on all but one alive slot per cell
    alive = benv.alive.cpu().numpy() > 0
    uvec = [uvec[r] * _one_per_cell(now[r][0]['cx'], now[r][0]['cy'], alive[r], H)[None] for r in range(R)]
    action = pop.differentiable_action()
    node = benv.differentiable_chem()
    ct = torch.as_tensor(np.stack(cvec), dtype=torch.float32, device=DEV)
    ut = torch.as_tensor(np.stack(uvec, axis=1), dtype=torch.float32, device=DEV)
    loss = (ct * node).sum() + (ut * action).sum()
    if reset_before_backward:
        benv.reset()
    loss.backward()
    torch.cuda.synchronize()
    out = dict(grad=pop.parameters.grad.detach().clone(), frames=frames, cells=cells, chem0=chem0, c=cvec, u=uvec, benv=benv, pop=pop,
               node=node.detach(), action=action.detach(), results=results, dyns=dyns, episodes=E, name=name)
    if not with_twins:
        return out
    # the stand-alone rollouts of the same worlds: Env.differentiable_step with replica r's agent
    out['twin'] = []
    for r, env in enumerate(twins):
        ag = pop.replica_agent(r)
        res = []
        for t in range(T):
            _, reward, _, _, info = env.differentiable_step(ag.differentiable_action(env._get_current_obs))
            res.append((reward, info['num_agents']))
        a = ag.differentiable_action(env._get_current_obs)
        nd = env.differentiable_chem()
        ls = (ct[r] * nd).sum() + (ut[:, r] * a).sum()
        ls.backward()
        torch.cuda.synchronize()
        out['twin'].append(dict(node=nd.detach(), action=a.detach(), results=res,
                                grad=parameters_to_vector([q.grad for q in ag.model.parameters()]).detach()))
    return out


def _layer_grads(pop, row):
    return [row[off:off + cout * cin * k * k].reshape(cout, cin, k, k) for k, cin, cout, off in pop._layers]


@pytest.mark.parametrize('T', [1, 2, 3])
@pytest.mark.parametrize('key', list(UNROLL))
def test_unrolled_gradients(key, T):
    got = _unroll(key, T)
    benv, pop, E, name = got['benv'], got['pop'], got['episodes'], got['name']
    c = F.CASES[name]
    R = benv.R
    if c.get('collisions'):
        assert all(int((cl < 0).sum()) >= 4 for r in range(R) for cl in got['cells'][r])        # two losers and two dead slots, every step
    # against the stand-alone path: the same bits
    rewards = [BatchedEnv.read_results(res) for res in got['results']]
    for r, twin in enumerate(got['twin']):
        assert np.array_equal(_bits(got['node'][r]), _bits(twin['node'])), (r, 'chem_T')
        assert np.array_equal(_bits(got['action'][:, r]), _bits(twin['action'])), (r, 'action_T')
        for t, (reward, num) in enumerate(twin['results']):
            assert rewards[t][0][r] == reward and rewards[t][1][r] == num, (r, t)
        if E == 1 and T == 1:
            assert np.array_equal(_bits(got['grad'][r]), _bits(twin['grad'])), (r, 'parameters.grad')
    # against float64
    weights = [[w + 0.01 * cand for w in F.weights_of(name, 24, 68)] for cand in range(R // E)]
    kw = dict(boundary=c['boundary'], chem0=got['chem0'], frames=got['frames'], c=got['c'], u=got['u'],
              sigma=[d.diffuse_sigma for d in got['dyns']], decay=[d.rate_decay_chem for d in got['dyns']],
              with_agent_channel=c.get('with_agent_channel', True), episodes=E)
    ref = B.rollout(weights, cells=got['cells'], **kw)
    cut = B.rollout(weights, cells=[[np.full_like(cl, -1) for cl in got['cells'][r]] for r in range(R)], **kw)
    grad = got['grad'].cpu().numpy().astype(np.float64)
    worst, moved = 0.0, 0.0
    for cand in range(R // E):
        for dev, want, other in zip(_layer_grads(pop, grad[cand]), ref['grads'][cand], cut['grads'][cand]):
            worst = max(worst, float(np.abs(dev - want).max() / np.abs(want).max()))
            moved = max(moved, float(np.abs(other - want).max() / np.abs(want).max()))
    chem_err = max(float(np.abs(got['node'][r].cpu().numpy() - ref['chem'][r]).max() / max(1.0, np.abs(ref['chem'][r]).max())) for r in range(R))
    print(f'batch_field_step_grad {key} T={T} R={R} E={E}: device {worst:.3e} of max|grad_f64| per candidate and layer (ceiling '
          f'{GRAD_TOL:.0e}); chem_T apart by {chem_err:.2e}; without the field path the model moves by {moved:.2e}')
    assert chem_err <= 1e-4
    assert worst <= GRAD_TOL
    assert moved > 100 * GRAD_TOL                                   # the path through the field is what is being measured


# ------------------------------------------------------------------------------------------------ 6. the graph's edges
def test_a_plain_step_cuts_the_graph():
    cut = _unroll('two_layers', 3, plain_at=(1,), with_twins=False)['grad']           # differentiable, plain, differentiable
    short = _unroll('two_layers', 3, plain_at=(0, 1), with_twins=False)['grad']       # the same worlds, the shorter graph
    full = _unroll('two_layers', 3, with_twins=False)['grad']
    assert np.array_equal(_bits(cut), _bits(short)) and not torch.equal(cut, full)


def test_backward_after_reset_gives_the_same_bits():
    before = _unroll('collisions', 3, with_twins=False)
    after = _unroll('collisions', 3, reset_before_backward=True, with_twins=False)
    assert after['benv'].chem_node is None and after['benv']._steps == 0
    assert np.array_equal(_bits(before['grad']), _bits(after['grad'])) and float(before['grad'].abs().max()) > 0


@pytest.fixture
def calls(monkeypatch):
    log = []
    for name in ('die_nca_backward_batch', 'die_nca_backward_batch_inputs', 'die_env_step_batch', 'die_deposit_cells_batch',
                 'die_env_step_backward_batch', 'die_nca_sense_batch_store', 'die_gather_scale_batch', 'die_gather_scale_backward_batch'):
        def recorder(*args, _fn=getattr(L.lib, name), _name=name):
            log.append(_name)
            return _fn(*args)
        monkeypatch.setattr(L.lib, name, recorder)
    return log


def test_nodes_come_and_go_and_the_calls_follow(calls):
    W, H, R = 24, 68, 3
    benv = BatchedEnv((W, H), die.Dynamics(diffuse_sigma=0.8, init_agent_ratio=0.15), replicas=R, seed=3)
    pop = BatchedNeuralAutomataAgent(benv, _template())
    pop.parameters.requires_grad_(True)
    old = ['die_nca_sense_batch_store', 'die_gather_scale_batch', 'die_gather_scale_backward_batch', 'die_nca_backward_batch']
    assert benv.chem_node is None
    pop.differentiable_action().sum().backward()                    # without a node: the calls it made before
    assert calls == old
    del calls[:]
    leaf = benv.differentiable_chem()                               # a leaf that asks for nothing changes nothing either
    assert leaf.is_leaf and not leaf.requires_grad and leaf is benv.differentiable_chem() and torch.equal(leaf, benv.chem)
    pop.differentiable_action().sum().backward()
    assert calls == old and leaf.grad is None
    del calls[:]
    benv.differentiable_step(pop.differentiable_action())
    node = benv.differentiable_chem()
    assert node.grad_fn is not None and node is benv.chem_node and torch.equal(node, benv.chem)
    assert calls == old[:2] + ['die_env_step_batch', 'die_deposit_cells_batch']
    del calls[:]
    (pop.differentiable_action().sum() + node.sum()).backward()
    assert sorted(calls) == sorted(old[:3] + ['die_nca_backward_batch_inputs', 'die_env_step_backward_batch', 'die_gather_scale_backward_batch',
                                              'die_nca_backward_batch'])
    # anything else that changes the worlds drops the node
    for change in (lambda: benv.step(pop), lambda: benv.step_action(torch.zeros((3, R, benv.Nmax), dtype=torch.float32, device=DEV)),
                   lambda: benv.run(pop, 2), benv.reset):
        benv.differentiable_step(pop.differentiable_action())
        assert benv.chem_node is not None
        change()
        assert benv.chem_node is None
        fresh = benv.differentiable_chem()
        assert fresh.is_leaf and not fresh.requires_grad and torch.equal(fresh, benv.chem)
    torch.cuda.synchronize()


@pytest.mark.parametrize('what', ['fp16', 'per_replica', 'shape', 'dtype', 'host'])
def test_refusals_leave_the_state_untouched(what, calls):
    W, H, R = 24, 68, 2
    kw = dict(field_dtype=torch.float16) if what == 'fp16' else dict(per_replica=True) if what == 'per_replica' else {}
    benv = BatchedEnv((W, H), die.Dynamics(diffuse_sigma=0.8, init_agent_ratio=0.15), replicas=R, seed=3, **kw)
    action = torch.zeros((3, R, benv.Nmax), dtype=torch.float32, device=DEV)
    action = {'shape': action[:, :, 1:], 'dtype': action.double(), 'host': action.cpu()}.get(what, action)
    before = [tuple(x.copy() for x in benv.replica_numpy(r)) for r in range(R)]
    with pytest.raises(NotImplementedError if what in ('fp16', 'per_replica') else ValueError):
        benv.differentiable_step(action)
    if what in ('fp16', 'per_replica'):
        with pytest.raises(NotImplementedError):
            benv.differentiable_chem()
    assert calls == [] and benv._steps == 0 and benv.chem_node is None
    for r in range(R):
        for x, y in zip(before[r], benv.replica_numpy(r)):
            assert np.array_equal(x, y)
