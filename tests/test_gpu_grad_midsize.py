"""The differentiable paths on the GPU at mid-size worlds (LABBOOK §33): the conv adjoints with tens and hundreds of tiles, and one
whole unrolled path each for the batch and for a stand-alone world large enough for the default re-sort.  The shapes are those of
tests/grad_midsize_shapes.py; tests/test_grad_midsize_cpu.py recomputes from the sources why each reaches its branch.  (The
full-block tests of the gather, deposit-cells and scatter entry points are in tests/test_gpu_field_step_grad.py and
tests/test_gpu_batch_field_step_grad.py.)

Ceilings, none of them taken from what the device gives:
  * the layer entry points against float64: the project's backward tolerance, 1e-4 * max|ref| per array; the CPU module shows
    that a plain fp32 evaluation of every case stays within 1e-5.  The reference (tests/grad_midsize_model.py) shares no device
    code and is handed the DEVICE's fp32 forward output as t, so relu's kink cannot split the two;
  * batched against stand-alone, E = 1, and the batched whole path: bits, compared exactly;
  * E = 2: the float64 sum of the two worlds' gradients, 1e-4 * max|ref| per layer block;
  * the stand-alone whole path: tests/test_gpu_field_step_grad.py::test_unrolled_gradients_match_the_float64_model's three
    assertions, unchanged.

Every ctypes call writes into buffers with a NaN guard band behind them that must come back NaN, the workspace has exactly the bytes
the query names, and every partial row of it must have been written (no NaN left)."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch.nn.utils import parameters_to_vector

import die_amd as die
from die_amd import _lib as L
from die_amd import functional as Fn
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent
from die_amd.device_array import _ptr, stream_ptr
from tests import field_step_adjoint_model as F
from tests import grad_midsize_model as GM
from tests import grad_midsize_shapes as S
from tests import nca_grad_model as NG
from tests import nca_wide_grad_batch_model as WB
from tests import nca_wide_grad_model as G
from tests.test_gpu_batch_step_action import _cell
from tests.test_gpu_field_step_grad import GRAD_TOL, _array_cells, _nca
from tests.test_gpu_nca_wide_grad import _guarded, _host

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BWD_TOL = 1e-4
F32, F16, AGENTS = L.DIE_PLANE_F32, L.DIE_PLANE_F16, L.DIE_PLANE_AGENTS


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _tiles(W, H):
    return -(-W // 16) * -(-H // 64)


def _rel(got, want):
    top = np.abs(want).max()
    assert top > 0
    return float(np.abs(got - want).max() / top)


# ------------------------------------------------------------------------------------------------ 1. the layer entry points
def _case_planes(c, inp):
    """(tensors kept alive, die_conv_plane array, the float64 values the device reads, claim epoch) of a case's input planes.  A
    first layer reads the claim plane and the fp16 fields of an Env of the case's size after two steps."""
    W, H = S.CONV_FIELDS[c['field']]
    if not c.get('first_layer'):
        keep = [torch.from_numpy(inp['x'][ch]).to(DEV) for ch in range(c['cin'])]
        return keep, (L.ConvPlane * c['cin'])(*[L.ConvPlane(t.data_ptr(), F32, 0) for t in keep]), inp['x'].astype(np.float64), 1
    env = die.Env((W, H), die.Dynamics(diffuse_sigma=0.8), seed=3, device=DEV, field_dtype=torch.float16, sort_every=0)
    rs = np.random.RandomState(3)
    N = env.agents.N
    for _ in range(2):
        env.step(np.stack([rs.uniform(-0.01, 0.01, N), rs.uniform(-0.01, 0.01, N), rs.uniform(0.5, 2.0, N)]).astype(np.float32))
    M = env.medium
    M._ensure_owner()
    assert M.food.dtype == torch.float16 and M.chem.dtype == torch.float16 and M.epoch == 3
    seen = M.to_numpy()
    assert 0.02 < seen[0].mean() < 0.9 and set(np.unique(seen[0])) == {0.0, 1.0} and np.abs(seen[2]).max() > 0
    keep = [M.owner, M.food, M.chem, env]
    kinds = (AGENTS, F16, F16)
    return keep, (L.ConvPlane * 3)(*[L.ConvPlane(t.data_ptr(), kind, 0) for t, kind in zip(keep, kinds)]), seen, M.epoch


@pytest.mark.parametrize('name', list(GM.WIDE_CASES))
def test_wide_backward_with_many_tiles(name):
    """Gap 3 of LABBOOK §33 (the fold of the conv adjoints behind die_conv2d_wide_backward): 264 tiles on 514 x 512 (33 tile rows
    of 8, whole unrolled trips of the fold, a last tile row of 2 rows, interior tiles far from any border) and 81 on 130 x 515
    (ragged both ways, ten unrolled trips and a remainder, H % 4 != 0: the scalar stores) — the largest count before was 9."""
    c = GM.WIDE_CASES[name]
    (W, H), k, cin, cout, mode, act = S.CONV_FIELDS[c['field']], c['k'], c['cin'], c['cout'], c['mode'], c['act']
    inp = GM.case_inputs(c)
    keep, arr, seen, epoch = _case_planes(c, inp)
    pad, a = L.PAD_MODES[mode], L.NCA_ACTIVATIONS[act]
    w_dev, g_dev = torch.from_numpy(inp['w']).to(DEV), torch.from_numpy(inp['g']).to(DEV)
    drop = L.nca_dropout(GM.DROP_P, inp['seed'], 0, GM.DROP_STEP) if c['masked'] else None
    nw, sp = cout * cin * k * k, stream_ptr(DEV)
    need = L.lib.die_conv2d_wide_backward_workspace_bytes(W, H, cin, cout, k)
    assert need == _tiles(W, H) * nw * 4
    t_dev = None
    if act is not None or c['masked']:
        t_dev = torch.empty((cout, W, H), dtype=torch.float32, device=DEV)
        L.check(L.lib.die_conv2d_wide(W, H, cin, arr, epoch, cout, _ptr(t_dev), W * H, k, _ptr(w_dev), a, pad, None, sp), 'die_conv2d_wide')
    runs = []
    for _ in range(2):
        gw, ws, gin = _guarded(nw), _guarded(need // 4), _guarded(cin * W * H)
        L.check(L.lib.die_conv2d_wide_backward(W, H, cin, arr, epoch, cout, _ptr(g_dev), W * H, _ptr(t_dev), W * H, k, _ptr(w_dev), a, pad,
                                               None if drop is None else C.byref(drop), _ptr(gw), _ptr(gin), W * H, _ptr(ws), need, sp),
                'die_conv2d_wide_backward')
        runs.append((gw, gin, ws))
    torch.cuda.synchronize()
    _check_layer(name, c, inp, seen, None if t_dev is None else t_dev.cpu().numpy(), runs)


def _check_layer(name, c, inp, seen, t, runs):
    (W, H), k, cin, cout = S.CONV_FIELDS[c['field']], c['k'], c['cin'], c['cout']
    nw = cout * cin * k * k
    got = []
    for gw, gin, ws in runs:
        _host(ws, _tiles(W, H) * nw, (-1,), f'{name}: workspace')                  # every partial row written, nothing behind them
        got.append((_host(gw, nw, (cout, cin, k, k), f'{name}: grad_weights'), _host(gin, cin * W * H, (cin, W, H), f'{name}: grad_in')))
    z, want_w, want_in = GM.reference(seen, inp['w'], inp['g'], t, c['act'], GM.case_mask(c, inp), c['mode'])
    if t is not None:                                                               # (a wiring check of the forward the model is handed)
        ref = G.act_forward(z, c['act'])
        assert np.abs(t - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max()), (name, 'forward')
    errs = (_rel(got[0][0], want_w), _rel(got[0][1], want_in))
    print(f'mid-size conv adjoint {name} on {W} x {H} ({_tiles(W, H)} tiles): device grad_w {errs[0]:.2e}  grad_in {errs[1]:.2e}  '
          f'(of max|f64| per array; ceiling {BWD_TOL:.0e})')
    assert max(errs) <= BWD_TOL, errs
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), (name, 'two calls, two results')


def _ptrs(buf, n, cells):
    return (C.c_void_p * n)(*[buf.data_ptr() + 4 * o * cells for o in range(n)])


@pytest.mark.parametrize('name', list(GM.NARROW_CASES))
def test_narrow_backward_with_many_tiles(name):
    """Gap 3 of LABBOOK §33 (the fold behind die_conv2d_backward, and k_conv_backward's partial row index blockIdx.y * gridDim.x +
    blockIdx.x with many tile rows): k = 7 on 130 x 515 with grad_in (81 tiles, scalar stores), k = 3 with the tanh and the mask on
    514 x 512 (264 tiles)."""
    c = GM.NARROW_CASES[name]
    (W, H), k, cin, cout, mode = S.CONV_FIELDS[c['field']], c['k'], c['cin'], c['cout'], c['mode']
    inp = GM.case_inputs(c)
    keep, arr, seen, epoch = _case_planes(c, inp)
    pad, sp, cells = L.PAD_MODES[mode], stream_ptr(DEV), W * H
    w_dev, g_dev = torch.from_numpy(inp['w']).to(DEV), torch.from_numpy(inp['g']).to(DEV)
    drop = L.nca_dropout(GM.DROP_P, inp['seed'], 0, GM.DROP_STEP) if c['masked'] else None
    nw = cout * cin * k * k
    need = L.lib.die_conv2d_backward_workspace_bytes(W, H, cin, cout, k)
    assert need == _tiles(W, H) * nw * 4
    t_dev = None
    if c['act'] == 'tanh':
        t_dev = torch.empty((cout, W, H), dtype=torch.float32, device=DEV)
        L.check(L.lib.die_conv2d(W, H, cin, arr, epoch, cout, _ptrs(t_dev, cout, cells), k, _ptr(w_dev), 1, pad, sp), 'die_conv2d')
    runs = []
    for _ in range(2):
        gw, ws, gin = _guarded(nw), _guarded(need // 4), _guarded(cin * cells)
        L.check(L.lib.die_conv2d_backward(W, H, cin, arr, epoch, cout, _ptrs(g_dev, cout, cells), k, _ptr(w_dev), _ptr(gw), _ptrs(gin, cin, cells),
                                          None if t_dev is None else _ptrs(t_dev, cout, cells), None if drop is None else C.byref(drop),
                                          pad, _ptr(ws), need, sp), 'die_conv2d_backward')
        runs.append((gw, gin, ws))
    torch.cuda.synchronize()
    _check_layer(name, c, inp, seen, None if t_dev is None else t_dev.cpu().numpy(), runs)


# ------------------------------------------------------------------------------------------------ 2. the batched stacks
WIDE_SPEC = dict(width=16, sizes=(3, 3), act='tanh')
COEFS = dict(scale=0.1, deposit=2.0)
DYN = dict(rate_decay_chem=0.025, diffuse_sigma=.8)


def _population(benv, E, wide, **coefs):
    torch.manual_seed(1)
    kw = dict(hidden_channels=WIDE_SPEC['width'], hidden_activation=WIDE_SPEC['act']) if wide else {}
    template = die.NeuralAutomataAgent(kernel_sizes=(3, 3), boundary='circular', **kw, **{**COEFS, **coefs})
    assert template.model.wide == wide
    P = sum(k.weight.numel() for k in template.model.conv_layers())
    rows = torch.rand((benv.R // E, P), generator=torch.Generator().manual_seed(5)) - 0.5
    return BatchedNeuralAutomataAgent(benv, template, rows, E)


def _batch_world(E, wide):
    R, W, H = S.BATCH_SHAPE
    benv = BatchedEnv((W, H), die.Dynamics(**DYN), replicas=R, seed=11, device=DEV)
    assert not benv.per_replica
    pop = _population(benv, E, wide)
    benv.run(pop, 2)
    g = torch.randn((R, 3, W, H), generator=torch.Generator().manual_seed(3)).to(DEV)
    return benv, pop, g


def _layer_blocks(pop, row):
    return [row[off:off + cout * cin * k * k].reshape(cout, cin, k, k) for k, cin, cout, off in pop._layers]


@pytest.mark.parametrize('E', [1, 2])
def test_wide_backward_batch_with_many_tiles(E):
    """Gap 3 of LABBOOK §33 (die_nca_wide_backward_batch: the replica offset z * tiles * nw, the workspace's split into gradient
    planes first and partial rows second, the fold over E * tiles rows) on S = 2 x 514 x 512: 3 -> 16 -> 3, tanh, with and without
    grad_in.  E = 1: row r of the (C, P) gradient is die_conv2d_wide_backward on replica r's world, bit for bit, and so is the chem
    channel's grad_in.  E = 2: the float64 sum of the two worlds' gradients."""
    benv, pop, g = _batch_world(E, True)
    R = benv.R
    planes = benv.medium_tensor().clone()
    assert planes.dtype == torch.float32 and tuple(planes.shape) == (R, 3, benv.W, benv.H)

    def batched(with_node):
        benv.chem_node = None
        node = benv.differentiable_chem().requires_grad_() if with_node else None
        p = pop.parameters.detach().clone().requires_grad_()
        (pop.forward_device(p) * g).sum().backward()
        torch.cuda.synchronize()
        return p.grad.detach().clone(), None if node is None else node.grad.detach().clone()

    plain, _ = batched(False)
    again, _ = batched(False)
    with_in, node_grad = batched(True)
    assert np.array_equal(_bits(plain), _bits(again)) and np.array_equal(_bits(plain), _bits(with_in)) and float(plain.abs().max()) > 0
    assert tuple(node_grad.shape) == (R, benv.W, benv.H)
    alone = []
    for r in range(R):
        ag = pop.replica_agent(r)
        x = planes[r].clone().requires_grad_()
        (ag.model.forward_device(x) * g[r]).sum().backward()
        torch.cuda.synchronize()
        alone.append(parameters_to_vector([q.grad for q in ag.model.parameters()]).detach())
        assert np.array_equal(_bits(node_grad[r]), _bits(x.grad[-1])) and float(x.grad[-1].abs().max()) > 0, (r, 'grad_in of the chem channel')
        if E == 1:
            assert np.array_equal(_bits(plain[r]), _bits(alone[r])), (r, float((plain[r] - alone[r]).abs().max()))
    if E == 1:
        return
    rows = pop.parameters.detach().cpu().numpy()
    weights = [b.reshape(cout, cin, k, k) for b, (k, cin, cout) in zip(WB.blocks(WIDE_SPEC, rows[0]), WB.layer_shapes(WIDE_SPEC))]
    want = 0.0
    for r in range(R):
        stack = WB.torch_stack(weights, WIDE_SPEC['act'], 'circular', torch.float64)
        (stack(planes[r].cpu().double()[None])[0] * g[r].cpu().double()).sum().backward()
        want = want + np.concatenate([m.weight.grad.numpy().ravel() for m in stack if hasattr(m, 'weight')])
    got = plain[0].cpu().numpy().astype(np.float64)
    for li, (have, f64) in enumerate(zip(WB.blocks(WIDE_SPEC, got), WB.blocks(WIDE_SPEC, want))):
        err = _rel(have, f64)
        print(f'mid-size wide batch E = 2 layer {li}: device {err:.3e} of max|sum grad_f64| (ceiling {BWD_TOL:.0e})')
        assert err <= BWD_TOL, (li, err)
    assert not np.array_equal(_bits(plain[0]), _bits(alone[0]))                   # the episodes were folded


@pytest.mark.parametrize('E', [1, 2])
def test_narrow_backward_batch_inputs_with_many_tiles(E):
    """Gap 3 of LABBOOK §33 (die_nca_backward_batch_inputs: k_conv_backward with the replica in blockIdx.z and its block of partial
    rows, k_conv_backward_sum_batch over E * 264 rows) on S: 3 -> 3 -> 3 with a chem node that asks for its gradient.  E = 1: row r
    and the node's plane r are the stand-alone differentiable_sense on replica r's world (die_conv2d_backward per layer), bit for
    bit.  E = 2: the float64 sum of the two worlds' gradients."""
    benv, pop, g = _batch_world(E, False)
    R, W, H = benv.R, benv.W, benv.H
    pop.parameters.requires_grad_(True)
    node = benv.differentiable_chem().requires_grad_(True)
    (pop.differentiable_sense() * g).sum().backward()
    torch.cuda.synchronize()
    grad, node_grad = pop.parameters.grad.detach().clone(), node.grad.detach().clone()
    assert tuple(node_grad.shape) == (R, W, H) and float(grad.abs().max()) > 0
    want = 0.0
    for r in range(R):
        medium, agents = benv.replica_numpy(r)
        env = die.Env.from_numpy(medium, agents, die.Dynamics(**DYN), device=DEV, sort_every=0, pic=False)
        env.medium._ensure_owner()
        assert np.array_equal(env.medium.chem.cpu().numpy(), benv.chem[r].cpu().numpy())
        ag = pop.replica_agent(r)
        nd = env.differentiable_chem().requires_grad_(True)
        (ag.differentiable_sense(env.medium) * g[r]).sum().backward()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(node_grad[r]), _bits(nd.grad)) and float(nd.grad.abs().max()) > 0, r
        twin = parameters_to_vector([q.grad for q in ag.model.parameters()]).detach()
        if E == 1:
            assert np.array_equal(_bits(grad[r]), _bits(twin)), (r, float((grad[r] - twin).abs().max()))
            continue
        convs = NG.layers([w.astype(np.float64) for w in _layer_blocks(pop, pop.parameters.detach().cpu().numpy()[0])], 'circular')
        (NG.sense(convs, torch.as_tensor(medium.astype(np.float64))) * g[r].cpu().double()).sum().backward()
        want = want + np.concatenate([cv.weight.grad.numpy().ravel() for cv in convs])
    if E == 2:
        got = grad[0].cpu().numpy().astype(np.float64)
        for li, (have, f64) in enumerate(zip(_layer_blocks(pop, got), _layer_blocks(pop, want))):
            err = _rel(have, f64)
            print(f'mid-size narrow batch E = 2 layer {li}: device {err:.3e} of max|sum grad_f64| (ceiling {BWD_TOL:.0e})')
            assert err <= BWD_TOL, (li, err)


# ------------------------------------------------------------------------------------------------ 3. whole paths
@pytest.mark.parametrize('sigma,radius', [(0.5, 2), (0.8, 3)])
def test_env_step_backward_batch_sweeps_four_rows_a_wave(sigma, radius):
    """Gap 4 of LABBOOK §33, at the entry points: die_env_step_backward_batch on S = 2 x 514 x 512 runs the row sweep on the
    gradient planes with 4 rows a wave (a partial last wave: 514 % 4 = 2) and three strips a row, die_env_step_backward on one
    plane of it with 2.  Replica r is the stand-alone call bit for bit — planes and gathered deposits — and both are within the
    forward ceiling, 1e-5 * max(1, max|f64|), of the float64 sweep."""
    R, W, H = S.BATCH_SHAPE
    assert len(F.taps(sigma)) == 2 * radius + 1
    decay, stride, n = 0.1, S.GATHER_BATCH_STRIDE, S.GATHER_BATCH_N[:R]
    rs = np.random.RandomState(radius)
    g_host = rs.standard_normal((R, W, H)).astype(np.float32)
    cells_host = np.stack([S.gather_cells(W * H, stride, rs) for _ in range(R)])
    g, cells = torch.from_numpy(g_host).to(DEV), torch.from_numpy(cells_host).to(DEV)
    b = L.Batch(R, 0, W * H, stride, 1, (C.c_int64 * 64)(*(list(n) + [0] * (64 - R))))
    gc, gd = _guarded(R * W * H), _guarded(R * stride)
    rc = L.lib.die_env_step_backward_batch(W, H, C.byref(b), _ptr(g), sigma, decay, None, None, _ptr(cells), _ptr(gc), _ptr(gd), stream_ptr(DEV))
    assert rc == 0, L.lib.die_last_error()
    alone = []
    for r in range(R):
        one_c, one_d = _guarded(W * H), _guarded(n[r])
        rc = L.lib.die_env_step_backward(W, H, _ptr(g[r]), sigma, decay, n[r], _ptr(cells[r]), _ptr(one_c), _ptr(one_d), stream_ptr(DEV))
        assert rc == 0, L.lib.die_last_error()
        alone.append((one_c, one_d))
    torch.cuda.synchronize()
    gc, gd = _host(gc, R * W * H, (R, W * H), 'grad_chem'), _host(gd, R * stride, (R, stride), 'grad_deposit')
    for r in range(R):
        want_c, want_d = _host(alone[r][0], W * H, (-1,), 'grad_chem alone'), _host(alone[r][1], n[r], (-1,), 'grad_deposit alone')
        assert np.array_equal(gc[r], want_c), (r, np.flatnonzero(gc[r] != want_c)[:8] // H)
        assert np.array_equal(gd[r, :n[r]], want_d) and not gd[r, n[r]:].any(), r
        assert np.array_equal(gd[r, :n[r]], S.gather_want(gc[r], cells_host[r, :n[r]]).astype(np.float64)), r
        ref = F.diffuse_decay(torch.as_tensor(g_host[r].astype(np.float64)), sigma, decay).numpy().reshape(-1)
        err = float(np.abs(gc[r] - ref).max() / max(1.0, np.abs(ref).max()))
        print(f'env_step_backward_batch {W}x{H} radius {radius} replica {r}: grad_chem apart from float64 by {err:.3e} (ceiling 1e-05)')
        assert err <= 1e-5


def _shared_cells(benv, r):
    """How many alive slots of replica r stand on a cell that another alive slot of it stands on."""
    k = benv.n[r]
    alive = benv.alive[r, :k].cpu().numpy() > 0
    x, y = benv.x[r, :k].cpu().numpy().view(np.uint32)[alive], benv.y[r, :k].cpu().numpy().view(np.uint32)[alive]
    _, counts = np.unique(_cell(x, benv.W) * benv.H + _cell(y, benv.H), return_counts=True)
    return int(counts[counts > 1].sum())


def test_batched_unrolled_steps_are_the_stand_alone_ones():
    """Gap 4 of LABBOOK §33 (the adjoint's field sweep through die_env_step_backward_batch and its own argument handling): two
    steps of BatchedEnv.differentiable_step on S = 2 x 514 x 512, driven by a wide population (forward_device and gather_scale_batch:
    a wide stack's differentiable action), loss = a fixed random plane dotted with the final chem.  R * W * H >= 2^19, so the batch
    sweeps 4 rows a wave through three strips a row, and each stand-alone twin (W * H < 2^19) 2: replica r's chem, actions and
    gradient row equal the stand-alone Env + agent run, bit for bit.

    Bits are defined only while no two slots with a non-zero gradient are SENSED on one cell (the read-out's adjoint adds them with
    fp32 atomics in arrival order), and through this loss every winner of a step has one.  The population's hop is therefore 0.6
    of a cell's half width in a world with clamped edges: nobody leaves its cell in the first step — every alive slot is sensed alone both times, which is
    asserted — and the second step carries a part of them onto a neighbour's cell, so that the recorded winners include cells that
    were fought over (alive slots that lost)."""
    R, W, H = S.BATCH_SHAPE
    # (clamped at the world's edge: on the torus a hop off row 0 lands on row W - 1's cell, whatever its length)
    dyn = lambda: die.Dynamics(diffuse_sigma=0.8, init_agent_ratio=0.15, boundary=die.BoundaryCondition.limit)
    benv = BatchedEnv((W, H), dyn(), replicas=R, seed=3, max_agents='alive', device=DEV)
    twins = [die.Env((W, H), dyn(), seed=benv.seeds[r], max_agents='alive', device=DEV, sort_every=0, pic=False, sync=False) for r in range(R)]
    assert not benv.per_replica and [e.agents.N for e in twins] == benv.n
    pop = _population(benv, 1, True, scale=0.6 * 0.5 / (W - 1))
    p = pop.parameters.detach().clone().requires_grad_()
    cvec = torch.randn((R, W, H), generator=torch.Generator().manual_seed(9)).to(DEV)
    actions, losers = [], []
    for t in range(2):
        assert [_shared_cells(benv, r) for r in range(R)] == [0] * R, t            # sensed alone: one term a cell in the read-out's adjoint
        actions.append(Fn.gather_scale_batch(pop.forward_device(p), pop))
        benv.differentiable_step(actions[-1])
        recorded = benv.differentiable_chem().grad_fn.saved_tensors[0]
        for r in range(R):
            k = benv.n[r]
            won, alive = int((recorded[r, :k] >= 0).sum()), int((benv.alive[r, :k] > 0).sum())
            assert 0 < won <= alive and bool((recorded[r, k:] == -1).all())
            losers.append(alive - won)
    assert losers[:R] == [0] * R and all(v > 100 for v in losers[R:]), losers      # the second step's cells were fought over
    node = benv.differentiable_chem()
    (cvec * node).sum().backward()
    torch.cuda.synchronize()
    assert float(p.grad.abs().max()) > 0
    for r, env in enumerate(twins):
        ag = pop.replica_agent(r)
        k = benv.n[r]
        for t in range(2):
            obs = env._get_current_obs
            obs[1].sensed()
            planes = torch.stack([obs[1].sel('agents'), obs[1].sel('env_food').float(), env.differentiable_chem()])
            act = Fn.gather_scale(ag.model.forward_device(planes), obs, ag.action_coefs)
            assert np.array_equal(_bits(actions[t][:, r, :k]), _bits(act)), (r, t, 'action')
            env.differentiable_step(act)
        nd = env.differentiable_chem()
        assert np.array_equal(_bits(node[r]), _bits(nd)), (r, 'chem_T')
        (cvec[r] * nd).sum().backward()
        torch.cuda.synchronize()
        twin = parameters_to_vector([q.grad for q in ag.model.parameters()]).detach().to(DEV)
        differing = int((p.grad[r] != twin).sum())
        assert np.array_equal(_bits(p.grad[r]), _bits(twin)) and float(twin.abs().max()) > 0, (r, differing, float((p.grad[r] - twin).abs().max()))


def test_stand_alone_unrolled_steps_through_the_default_resort():
    """Gaps 4 and 5 of LABBOOK §33: a stand-alone world of 1028 x 1024 (>= 2^19 cells: the sweep and its adjoint take 4 rows a wave
    and 5 strips a row, and `sort_every` is left to Env, which re-sorts such a world every 8 steps).  Seven plain steps first, so
    that the first of the two unrolled steps is the 8th and ends with the re-sort: differentiable_step records the winners
    before it, die_deposit_cells and the second step then work on permuted arrays with a slot array.  The weight gradients of a
    narrow 3 -> 3 -> 3 agent against the float64 model, with test_unrolled_gradients_match_the_float64_model's assertions."""
    W, H = S.ALONE_SHAPE
    sigma = 0.8
    env = die.Env((W, H), die.Dynamics(diffuse_sigma=sigma, rate_decay_chem=F.DECAY), seed=5, device=DEV)
    assert env._sort_every == 8
    ag = _nca((3, 3), 'circular')
    weights = [q.detach().cpu().numpy().astype(np.float64) for q in ag.model.parameters()]
    N = env.agents.N
    for _ in range(7):
        env.step(ag.forward(env._get_current_obs))
    assert env.agents.slot is None and env._steps == 7
    rs = np.random.RandomState(33)
    cvec, u_slot = rs.standard_normal((W, H)), rs.standard_normal((3, N))

    def frame():
        m = env.medium.to_numpy()
        cx, cy = _array_cells(env)
        return dict(occ=m[0], food=m[1], cx=cx, cy=cy, mask=None), m[2]

    frames, cells, chem0 = [], [], None
    for t in range(2):
        f, chem = frame()
        chem0 = chem if t == 0 else chem0
        frames.append(f)
        env.differentiable_step(ag.differentiable_action(env._get_current_obs))
        assert env.agents.slot is not None                           # re-sorted at the end of the first unrolled step, and since
        cells.append(env.differentiable_chem().grad_fn.saved_tensors[0].cpu().numpy().copy())
    slot = env.agents.slot.cpu().numpy()
    assert np.array_equal(np.sort(slot), np.arange(N)) and not np.array_equal(slot, np.arange(N))
    assert all(0 < (cl >= 0).sum() < N for cl in cells)
    frames.append(frame()[0])
    u = u_slot[:, slot]
    action = ag.differentiable_action(env._get_current_obs)
    node = env.differentiable_chem()
    loss = (torch.as_tensor(cvec, dtype=torch.float32, device=DEV) * node).sum() + (torch.as_tensor(u, dtype=torch.float32, device=DEV) * action).sum()
    for q in ag.model.parameters():
        q.grad = None
    loss.backward()
    torch.cuda.synchronize()
    grads = [q.grad.detach().cpu().numpy().copy() for q in ag.model.parameters()]
    ref = F.rollout(weights, 'circular', chem0, frames, cells, cvec, u, sigma)
    chem_err = float(np.abs(env.medium.chem.cpu().numpy() - ref['chem']).max() / max(1.0, np.abs(ref['chem']).max()))
    err = [float(np.abs(g - w).max() / np.abs(w).max()) for g, w in zip(grads, ref['grads'])]
    print(f'field_step_grad default re-sort {W}x{H} T=2, {N} slots: device', ' '.join(f'{e:.3e}' for e in err),
          f'(of max|grad_f64| per layer; ceiling {GRAD_TOL:.0e}); chem_T apart by {chem_err:.2e}')
    assert chem_err <= 1e-4
    assert all(e <= GRAD_TOL for e in err), err
    cut = F.rollout(weights, 'circular', chem0, frames, [np.full_like(cl, -1) for cl in cells], cvec, u, sigma)
    assert max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(cut['grads'], ref['grads'])) > 100 * GRAD_TOL
