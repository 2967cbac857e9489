"""The differentiable population of WIDE NeuralAutomataAgent stacks on the GPU: die_nca_wide_sense_batch_store and
die_nca_wide_backward_batch behind BatchedNeuralAutomataAgent.forward_device, and die_amd.functional.gather_scale_batch.

The invariant is the batch's: replica r is, bit for bit, the stand-alone computation on replica r's world — here
`replica_agent(r).model.forward_device` (die_conv2d_wide / die_conv2d_wide_backward per layer) on replica r's fp32 planes.  The
kernels of the two paths are one body (die_nca_wide_grad.hip), no float atomics anywhere in the conv adjoint, so the E = 1 checks
have no exclusions.  E > 1 rows are held to the float64 model of tests/nca_wide_grad_batch_model.py at the project's ceiling,
1e-4 * max|ref| per layer block; tests/test_nca_wide_grad_batch_cpu.py shows that a plain fp32 evaluation of every case stays
below 1e-5 (worst 2.7e-6), and the tests here print the device's error next to fp32 torch's.

Shapes: the smallest that cross the 16 x 64 tile's edges in both axes with H % 4 == 0 (which the batched step requires), 24 x 72 and
20 x 136; the first case also on 17 x 68 and 33 x 132.  Every world is stepped twice first; the weights are uniform in +-0.5."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
from torch.nn.utils import parameters_to_vector

import die_amd as die
from die_amd import _lib as L
from die_amd import functional as F
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent, BatchedPhysarumAgent
from die_amd.device_array import _ptr, stream_ptr
from oracle import cpu_ref as R
from tests import dropout_model as D
from tests import nca_wide_grad_batch_model as M

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
COEFS = dict(scale=0.1, deposit=2.0)
DYN = dict(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8)
CASES = M.CASES
E1 = sorted(k for k, c in CASES.items() if c.get('E', 1) == 1)
EN = sorted(k for k, c in CASES.items() if c.get('E', 1) > 1)
WORLD_SEED = 11


def _dynamics(c):
    if not c.get('rows'):
        return die.Dynamics(**DYN)
    return [die.Dynamics(food_infinite=True, rate_decay_chem=0.02 + 0.01 * r, diffuse_sigma=0.6 + 0.2 * r) for r in range(c['R'])]


def _template(c):
    torch.manual_seed(1)
    ag = die.NeuralAutomataAgent(kernel_sizes=c['sizes'], boundary=c.get('boundary', 'circular'), with_agent_channel=c.get('with_agent_channel', True),
                                 p_agent_dropout=M.DROP_P if 'seed' in c else 0., hidden_channels=c['width'], hidden_activation=c['act'], **COEFS)
    assert ag.model.training and ag.model.wide
    return ag


def _build(name, seed=WORLD_SEED):
    """(BatchedEnv, population) of a case: weights uniform in +-0.5, the worlds stepped twice."""
    c = CASES[name]
    W, H = M.field_of(c)
    benv = BatchedEnv((W, H), _dynamics(c), replicas=c['R'], seed=seed, field_dtype=torch.float16 if c.get('f16') else torch.float32,
                      max_agents=None if c.get('fixed') else 'alive', device=DEV)
    template = _template(c)
    E = c.get('E', 1)
    P = sum(k.weight.numel() for k in template.model.conv_layers())
    assert P == M.row_length(c)
    rows = torch.rand((c['R'] // E, P), generator=torch.Generator().manual_seed(5)) - 0.5
    drop = dict(dropout_seed=c['seed'], dropout_seed_stride=c['stride']) if 'seed' in c else {}
    bag = BatchedNeuralAutomataAgent(benv, template, rows, E, **drop)
    benv.run(bag, 2)
    return benv, bag


def _planes(benv, bag):
    """(R, cin, W, H) float32: every replica's planes in the first layer's channel order ([agents,] food, chem; fp16 fields widen exactly)."""
    cin = bag._layers[0][1]
    t = benv.medium_tensor()
    assert t.dtype == torch.float32 and tuple(t.shape) == (benv.R, 3, benv.W, benv.H)
    return t[:, 3 - cin:].clone()


def _batched(benv, bag, g, steps_between=0):
    """One batched forward + backward: (sense (R, 3, W, H), (C, P) gradient) as numpy."""
    p = bag.parameters.detach().clone().requires_grad_()
    s = bag.forward_device(p)
    assert s.grad_fn is not None and s.dtype == torch.float32 and tuple(s.shape) == (benv.R, 3, benv.W, benv.H)
    for _ in range(steps_between):
        benv.step(bag)
    (s * g).sum().backward()
    torch.cuda.synchronize()
    assert tuple(p.grad.shape) == tuple(bag.parameters.shape)
    return s.detach().cpu().numpy(), p.grad.cpu().numpy().copy()


def _drop_of(name, r, step):
    c = CASES[name]
    return (M.DROP_P, c['seed'] + r * c['stride'], step) if 'seed' in c else None


def _stand_alone(name, bag, planes, g, r, step, want_grad_in=False):
    """Replica r's planes through replica r's stand-alone model: (sense, flat gradient, grad at the planes or None)."""
    ag = bag.replica_agent(r)
    x = planes[r].clone().requires_grad_(want_grad_in)
    out = ag.model.forward_device(x, dropout=_drop_of(name, r, step))
    (out * g[r]).sum().backward()
    torch.cuda.synchronize()
    grad = parameters_to_vector([q.grad for q in ag.model.parameters()]).cpu().numpy()
    return out.detach().cpu().numpy(), grad, x.grad.cpu().numpy() if want_grad_in else None


@functools.lru_cache(maxsize=None)
def _case(name):
    """Everything the checks of a case share, computed once: the batched values and gradient (twice), the stand-alone ones, and
    what the step that follows senses.  The worlds of `benv` have been stepped once more when this returns."""
    benv, bag = _build(name)
    g = torch.randn((benv.R, 3, benv.W, benv.H), generator=torch.Generator().manual_seed(3)).to(DEV)
    step = bag.dropout_step
    planes = _planes(benv, bag)
    out = dict(benv=benv, bag=bag, g=g, step=step, planes=planes)
    out['sense'], out['grad'] = _batched(benv, bag, g)
    out['step_after'] = bag.dropout_step
    bag.dropout_step = step
    _, out['grad_again'] = _batched(benv, bag, g)
    out['alone'] = [_stand_alone(name, bag, planes, g, r, step) for r in range(benv.R)]
    bag.dropout_step = step
    benv.step(bag)
    out['rendered'] = [bag.render(r) for r in range(benv.R)]
    return out


# ------------------------------------------------------------------------------------------------ 1. the values
@pytest.mark.parametrize('name', sorted(CASES))
def test_values_are_the_stand_alone_ones_and_what_the_step_senses(name):
    c = _case(name)
    benv = c['benv']
    assert c['step_after'] == c['step'] + (1 if 'seed' in CASES[name] else 0)      # once per call
    for r in range(benv.R):
        want = c['alone'][r][0]
        assert np.array_equal(c['sense'][r], want), r
        assert np.array_equal(np.moveaxis(c['sense'][r], 0, -1), c['rendered'][r]), r
        assert np.abs(want).max() > 0
    if 'seed' in CASES[name]:
        spec = CASES[name]
        zero = c['sense'][:, 0] == 0
        assert zero.mean() > 0.1                                                    # the mask was on
        for r in range(benv.R):
            mask = D.mask(spec['seed'] + r * spec['stride'], c['step'], benv.W, benv.H, M.DROP_P)
            assert np.array_equal(zero[r], mask == 0), r
        assert np.array_equal(zero[0], zero[1]) == (spec['stride'] == 0)


# ------------------------------------------------------------------------------------------------ 2. E = 1: bit for bit
@pytest.mark.parametrize('name', E1)
def test_gradient_rows_are_the_stand_alone_gradients(name):
    c = _case(name)
    for r in range(c['benv'].R):
        for li, (got, want) in enumerate(zip(M.blocks(CASES[name], c['grad'][r]), M.blocks(CASES[name], c['alone'][r][1]))):
            assert np.array_equal(got, want), (r, li, np.abs(got - want).max())
            assert np.abs(want).max() > 0, (r, li)


# ------------------------------------------------------------------------------------------------ 3. E > 1: the float64 model
def _weights_of(spec, row):
    return [b.reshape(cout, cin, k, k) for b, (k, cin, cout) in zip(M.blocks(spec, row), M.layer_shapes(spec))]


@pytest.mark.parametrize('name', EN)
def test_episode_rows_match_the_float64_sum(name):
    c = _case(name)
    benv, bag, spec = c['benv'], c['bag'], CASES[name]
    E, mode = spec['E'], spec.get('boundary', 'circular')
    planes = c['planes'].cpu().numpy()
    g = c['g'].cpu().numpy()
    rows = bag.parameters.detach().cpu().numpy()
    weights = [_weights_of(spec, rows[cand]) for cand in range(benv.R // E)]
    want, _ = M.population_backward(list(planes), weights, list(g), spec['act'], mode, None, E)
    for cand in range(benv.R // E):
        f32 = None
        for e in range(E):                                           # the yardstick: torch fp32 on the CPU, summed in fp32
            r = cand * E + e
            stack = M.torch_stack(weights[cand], spec['act'], mode, torch.float32)
            (stack(torch.as_tensor(planes[r])[None])[0] * torch.as_tensor(g[r])).sum().backward()
            row = np.concatenate([m.weight.grad.numpy().ravel() for m in stack if hasattr(m, 'weight')])
            f32 = row if f32 is None else f32 + row
        for li, (got, f64, ref) in enumerate(zip(M.blocks(spec, c['grad'][cand]), M.blocks(spec, want[cand]), M.blocks(spec, f32))):
            top = np.abs(f64).max()
            err, yard = float(np.abs(got - f64).max() / top), float(np.abs(ref - f64).max() / top)
            print(f'nca_wide_grad_batch {name} candidate {cand} layer {li}: device {err:.3e}  fp32 torch {yard:.3e}  (of max|sum grad_f64|; '
                  f'ceiling {M.TOL:.0e})')
            assert err <= M.TOL, (cand, li, err)
        assert not np.array_equal(c['grad'][cand], c['alone'][cand * E][1])         # the episodes were folded


# ------------------------------------------------------------------------------------------------ 4. reproducible
@pytest.mark.parametrize('name', sorted(CASES))
def test_two_backward_passes_give_identical_bits(name):
    c = _case(name)
    assert np.array_equal(c['grad'], c['grad_again']) and np.abs(c['grad']).max() > 0


# ------------------------------------------------------------------------------------------------ 5. the action level
def _upstream(benv, seed=3):
    """tests/test_gpu_nca_grad_batch.py's rule: (3, R, Nmax) standard normal, zero on dead and padding slots and on every alive
    slot that stands on a cell an earlier alive slot of its replica stands on (the read-out's adjoint adds the slots of one cell with
    fp32 atomics in arrival order).  Also returns, per replica, (alive slots, alive slots that keep a gradient)."""
    g = torch.randn((3, benv.R, benv.Nmax), generator=torch.Generator().manual_seed(seed)).to(DEV)
    live = (benv.alive > 0).cpu().numpy()
    counts = []
    for r in range(benv.R):
        live[r, benv.n[r]:] = False
        alive = int(live[r].sum())
        _, a = benv.replica_numpy(r)
        cells = R.cell(a[0], benv.W).astype(np.int64) * benv.H + R.cell(a[1], benv.H)
        seen = set()
        for n in np.flatnonzero(live[r]):
            if int(cells[n]) in seen:
                live[r, n] = False
            seen.add(int(cells[n]))
        counts.append((alive, int(live[r].sum())))
    return g * torch.as_tensor(live, device=DEV)[None], counts


def test_actions_and_their_gradients_are_the_stand_alone_ones():
    name = 'tanh 8'
    benv, bag = _build(name)
    g, counts = _upstream(benv)
    print('nca_wide_grad_batch action level: (alive slots, of them with a gradient) per replica:', counts)
    for alive, kept in counts:
        assert alive > 0 and kept >= 0.9 * alive, counts                           # the exclusion is capped
    p = bag.parameters.detach().clone().requires_grad_()
    act = F.gather_scale_batch(bag.forward_device(p), bag)
    assert act.grad_fn is not None and act.dtype == torch.float32 and tuple(act.shape) == (3, benv.R, benv.Nmax)
    (act * g).sum().backward()
    torch.cuda.synchronize()
    act, grad = act.detach().cpu().numpy(), p.grad.cpu().numpy()
    for r in range(benv.R):
        medium, agents = benv.replica_numpy(r)
        env = die.Env.from_numpy(medium, agents, field_dtype=benv.dtype, device=DEV)
        ag = bag.replica_agent(r)
        obs = env._get_current_obs
        obs[1].sensed()
        planes = torch.stack([obs[1].sel(ch).float() for ch in ag.obs_channels])
        alone = F.gather_scale(ag.model.forward_device(planes), obs, ag.action_coefs)
        n = benv.n[r]
        assert tuple(alone.shape) == (3, n)
        (alone * g[:, r, :n]).sum().backward()
        torch.cuda.synchronize()
        assert np.array_equal(act[:, r, :n], alone.detach().cpu().numpy()), r
        assert np.all(act[:, r, n:] == 0) and np.abs(act[:, r, :n]).max() > 0, r
        want = parameters_to_vector([q.grad for q in ag.model.parameters()]).cpu().numpy()
        assert np.array_equal(grad[r], want) and np.abs(want).max() > 0, (r, np.abs(grad[r] - want).max())


# ------------------------------------------------------------------------------------------------ 6. backward after the worlds moved
@pytest.mark.parametrize('name', ['tanh 8', 'dropout stride 1', 'fp16 fields'])
def test_backward_after_two_steps_is_the_gradient_at_the_sensed_worlds(name):
    c = _case(name)
    benv, bag = _build(name)                                        # the same worlds again, stepped here
    assert bag.dropout_step == c['step']
    before = benv.replica_numpy(0)[0]
    _, got = _batched(benv, bag, c['g'], steps_between=2)
    assert not np.array_equal(benv.replica_numpy(0)[0], before)     # the worlds did change under the graph
    assert np.array_equal(got, c['grad'])


# ------------------------------------------------------------------------------------------------ 7. the unrolled step
def test_chem_channel_grad_in_is_the_stand_alone_one():
    name = 'tanh 8'
    c = _case(name)
    benv, bag = _build(name)
    node = benv.differentiable_chem()
    assert node is benv.chem_node and not node.requires_grad
    p = bag.parameters.detach().clone().requires_grad_()
    (bag.forward_device(p) * c['g']).sum().backward()               # a node that asks for nothing: no grad_in, the same weights' gradient
    assert node.grad is None and np.array_equal(p.grad.cpu().numpy(), c['grad'])
    node.requires_grad_()
    p = bag.parameters.detach().clone().requires_grad_()
    (bag.forward_device(p) * c['g']).sum().backward()
    torch.cuda.synchronize()
    assert np.array_equal(p.grad.cpu().numpy(), c['grad'])
    got = node.grad.cpu().numpy()
    assert got.shape == (benv.R, benv.W, benv.H)
    for r in range(benv.R):
        _, _, gin = _stand_alone(name, bag, c['planes'], c['g'], r, c['step'], want_grad_in=True)
        assert np.array_equal(got[r], gin[-1]) and np.abs(gin[-1]).max() > 0, r


@pytest.mark.parametrize('name', ['tanh 8', 'two episodes'])
def test_unrolled_steps_match_the_float64_model(name):
    spec = CASES[name]
    benv, bag = _build(name)
    R_, W, H, E = benv.R, benv.W, benv.H, spec.get('E', 1)
    p = bag.parameters.detach().clone().requires_grad_()
    frames, cells, chem0 = [[] for _ in range(R_)], [[] for _ in range(R_)], []
    for t in range(2):
        for r in range(R_):
            m, a = benv.replica_numpy(r)
            frames[r].append(dict(occ=m[0], food=m[1], cx=R.cell(a[0], W), cy=R.cell(a[1], H)))
            if t == 0:
                chem0.append(m[2])
        benv.differentiable_step(F.gather_scale_batch(bag.forward_device(p), bag))
        recorded = benv.differentiable_chem().grad_fn.saved_tensors[0].cpu().numpy()
        for r in range(R_):
            assert np.all(recorded[r, benv.n[r]:] < 0)
            cells[r].append(recorded[r, :benv.n[r]].copy())
    node = benv.differentiable_chem()
    cvec = torch.randn((R_, W, H), generator=torch.Generator().manual_seed(9))
    (cvec.to(DEV) * node).sum().backward()
    torch.cuda.synchronize()
    grad = p.grad.cpu().numpy().astype(np.float64)
    rows = bag.parameters.detach().cpu().numpy()
    coefs = (COEFS['scale'], COEFS['scale'], COEFS['deposit'])
    worst, moved = 0.0, 0.0
    for cand in range(R_ // E):
        weights = _weights_of(spec, rows[cand])
        want, cut = 0.0, 0.0
        for e in range(E):
            r = cand * E + e
            kw = dict(chem0=chem0[r], frames=frames[r], c=cvec[r].numpy(), sigma=DYN['diffuse_sigma'], decay=DYN['rate_decay_chem'], coefs=coefs)
            row, chem = M.rollout(weights, spec['act'], 'circular', cells=cells[r], **kw)
            assert np.abs(node[r].detach().cpu().numpy() - chem).max() <= 1e-4 * max(1.0, np.abs(chem).max()), r
            want = want + row
            # without the path through the first step's field the model is visibly another one
            cut = cut + M.rollout(weights, spec['act'], 'circular', cells=[np.full_like(cells[r][0], -1), cells[r][1]], **kw)[0]
        for got, f64, other in zip(M.blocks(spec, grad[cand]), M.blocks(spec, want), M.blocks(spec, cut)):
            worst = max(worst, float(np.abs(got - f64).max() / np.abs(f64).max()))
            moved = max(moved, float(np.abs(other - f64).max() / np.abs(f64).max()))
    print(f'nca_wide_grad_batch unrolled {name}: device {worst:.3e} of max|grad_f64| per candidate and layer (ceiling {M.TOL:.0e}); '
          f'without the first step\'s deposits the model moves by {moved:.2e}')
    assert worst <= M.TOL
    assert moved > 100 * M.TOL


# ------------------------------------------------------------------------------------------------ 8. the ABI
TAIL = 64


def _guarded(n):
    return torch.full((n + TAIL,), float('nan'), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize('E,mode', [(1, 'circular'), (2, 'zeros')])
def test_abi_on_a_field_with_scalar_stores(E, mode):
    """die_nca_wide_backward_batch through ctypes on 17 x 66 (H % 4 != 0: the cell-by-cell stores), a hand-built die_medium and
    die_batch, every stride with a gap, NaN-guarded buffers and the workspace at exactly the stated bytes."""
    W, H, R_ = 17, 66, 2
    cells = W * H
    layers = ((3, 2, 5, 'relu'), (1, 5, 4, 'relu'), (5, 4, 3, 'tanh'))
    shapes = [(k, cin, cout) for k, cin, cout, _ in layers]
    P = sum(k * k * cin * cout for k, cin, cout in shapes)
    Cn, cmax = R_ // E, 5
    plane_stride, sense_stride, grad_stride, gin_stride = cells + 6, 3 * cells + 2, P + 3, 2 * cells + 1
    rs = np.random.RandomState(17 + E)
    fields = torch.full((2, R_ * plane_stride), float('nan'), dtype=torch.float32, device=DEV)
    planes = rs.rand(R_, 2, W, H).astype(np.float32)
    for r in range(R_):
        for q in range(2):
            fields[q, r * plane_stride:r * plane_stride + cells] = torch.from_numpy(planes[r, q].ravel()).to(DEV)
    rows = rs.uniform(-0.5, 0.5, (Cn, P)).astype(np.float32)
    w_dev = torch.from_numpy(rows).to(DEV)
    g = rs.standard_normal((R_, 3, W, H)).astype(np.float32)
    g_dev = torch.full((R_ * sense_stride,), float('nan'), dtype=torch.float32, device=DEV)
    for r in range(R_):
        g_dev[r * sense_stride:r * sense_stride + 3 * cells] = torch.from_numpy(g[r].ravel()).to(DEV)
    m = L.Medium(W, H, L.DIE_F32, 1, None, fields[0].data_ptr(), fields[1].data_ptr(), None, 0, 0, 0, 0, 0, 0, 0, 0, None)
    b = L.Batch(R_, 0, plane_stride, 1, 1, (C.c_int64 * 64)(*([0] * 64)))
    arr, off = [], 0
    for k, cin, cout, act in layers:
        arr.append(L.NcaLayer(k, cin, cout, L.NCA_ACTIVATIONS[act], w_dev.data_ptr() + 4 * off, P))
        off += k * k * cin * cout
    arr = (L.NcaLayer * 3)(*arr)
    nca = L.NcaBatch(3, L.PAD_MODES[mode], 0, 1, arr, (C.c_float * 3)(0.1, 0.1, 2.0), 0 if E == 1 else E, None, 0)
    store_bytes = L.lib.die_nca_wide_sense_batch_store_bytes(W, H, R_, 3, cmax)
    need = L.lib.die_nca_wide_backward_batch_workspace_bytes(W, H, R_, C.byref(nca))
    assert store_bytes == M.store_bytes(W, H, R_, 3, cmax) and need == M.workspace_bytes(W, H, R_, shapes)
    store, ws = _guarded(store_bytes // 4), _guarded(need // 4)
    grad, gin = _guarded(Cn * grad_stride), _guarded(R_ * gin_stride)
    sp = stream_ptr(DEV)
    L.check(L.lib.die_nca_wide_sense_batch_store(C.byref(m), C.byref(b), C.byref(nca), _ptr(store), store_bytes, None, None, sp),
            'die_nca_wide_sense_batch_store')
    L.check(L.lib.die_nca_wide_backward_batch(C.byref(m), C.byref(b), C.byref(nca), _ptr(store), _ptr(g_dev), sense_stride, _ptr(grad),
                                              grad_stride, None, _ptr(ws), need, _ptr(gin), gin_stride, sp), 'die_nca_wide_backward_batch')
    torch.cuda.synchronize()
    st = store.cpu().numpy()
    assert np.isnan(st[store_bytes // 4:]).all() and np.isnan(ws.cpu().numpy()[need // 4:]).all()
    st = st[:store_bytes // 4].reshape(3, R_, cmax, W, H)
    ts = [[st[l, r, :shapes[l][2]].astype(np.float64) for l in range(3)] for r in range(R_)]
    for l in range(3):                                               # channels past a layer's cout are never written
        assert not np.isnan(st[l, :, :shapes[l][2]]).any() and np.isnan(st[l, :, shapes[l][2]:]).all(), l
    weights = [[blk.reshape(cout, cin, k, k) for blk, (k, cin, cout) in zip(np.split(rows[c], np.cumsum([k * k * ci * co for k, ci, co in shapes])[:-1]), shapes)]
               for c in range(Cn)]
    sense = M.sense(planes[0], weights[0], 'relu', mode)
    assert np.abs(ts[0][2] - sense).max() <= 1e-5
    want, want_in = M.population_backward(list(planes), weights, list(g), 'relu', mode, None, E, ts=ts)
    host = grad.cpu().numpy()
    assert np.isnan(host[Cn * grad_stride:]).all()
    host = host[:Cn * grad_stride].reshape(Cn, grad_stride)
    assert np.isnan(host[:, P:]).all() and not np.isnan(host[:, :P]).any()
    for c in range(Cn):
        off = 0
        for k, cin, cout in shapes:
            nw = k * k * cin * cout
            got, ref = host[c, off:off + nw], want[c][off:off + nw]
            err = float(np.abs(got - ref).max() / np.abs(ref).max())
            print(f'nca_wide_grad_batch abi E={E} {mode} candidate {c} layer {cin}->{cout} k={k}: device {err:.3e} (ceiling {M.TOL:.0e})')
            assert err <= M.TOL, (c, k, cin, cout, err)
            off += nw
    hin = gin.cpu().numpy()
    assert np.isnan(hin[R_ * gin_stride:]).all()
    hin = hin[:R_ * gin_stride].reshape(R_, gin_stride)
    assert np.isnan(hin[:, 2 * cells:]).all()
    for r in range(R_):
        got = hin[r, :2 * cells].reshape(2, W, H)
        assert np.abs(got - want_in[r]).max() <= M.TOL * np.abs(want_in[r]).max(), r
    assert np.isnan(g_dev.cpu().numpy().reshape(R_, sense_stride)[:, 3 * cells:]).all()       # (inputs: read only)


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_narrow_large_worlds_and_reflect_raise_before_any_launch():
    spec = CASES['tanh 8']
    W, H = M.field_of(spec)
    benv = BatchedEnv((W, H), die.Dynamics(**DYN), replicas=2, seed=11, device=DEV)
    before = [benv.replica_numpy(r) for r in range(2)]
    narrow = BatchedNeuralAutomataAgent(benv, die.NeuralAutomataAgent(kernel_sizes=(3, 3), **COEFS), dropout_seed=1)
    with pytest.raises(ValueError, match='narrow'):
        narrow.forward_device()
    assert narrow.dropout_step == 0 and narrow._calls == 0
    ag = die.NeuralAutomataAgent(kernel_sizes=(3, 3), boundary='reflect', hidden_channels=8, hidden_activation='tanh', **COEFS)
    bag = BatchedNeuralAutomataAgent(benv, ag, dropout_seed=1)
    with pytest.raises(NotImplementedError, match='reflect'):
        bag.forward_device()
    assert bag.dropout_step == 0 and bag._calls == 0
    ok = BatchedNeuralAutomataAgent(benv, _template(spec), dropout_seed=1)
    with pytest.raises(ValueError):
        ok.forward_device(torch.zeros((3, ok.P), device=DEV))
    with pytest.raises(ValueError):
        F.gather_scale_batch(torch.zeros((2, 3, W, H + 1), device=DEV), ok)
    assert ok.dropout_step == 0 and ok._calls == 0
    for r in range(2):
        assert all(np.array_equal(x, y) for x, y in zip(before[r], benv.replica_numpy(r)))
    assert benv.epoch == 1 and benv._steps == 0 and benv.chem_node is None
    big = BatchedEnv((W, H), die.Dynamics(**DYN), replicas=2, seed=11, per_replica=True, device=DEV)
    bag = BatchedNeuralAutomataAgent(big, _template(spec), dropout_seed=1)
    with pytest.raises(NotImplementedError, match='per_replica'):
        bag.forward_device()
    with pytest.raises(NotImplementedError, match='per_replica'):
        F.gather_scale_batch(torch.zeros((2, 3, W, H), device=DEV), bag)
    assert bag.dropout_step == 0 and bag._calls == 0


# ------------------------------------------------------------------------------------------------ 10. it learns
def test_ten_adam_steps_of_batched_imitation_lower_the_loss():
    """tests/test_gpu_nca_grad_batch.py's imitation loop with two wide students (3 -> 8 -> 3, tanh) on four worlds, two each."""
    R_, Cn, scale = 4, 2, 0.05
    benv = BatchedEnv((24, 72), die.Dynamics(**DYN), replicas=R_, seed=1, device=DEV)
    teacher = BatchedPhysarumAgent(benv, scale=scale, deposit=0.5, seed=0)
    torch.manual_seed(0)
    template = die.NeuralAutomataAgent(kernel_sizes=(3, 3), scale=scale, deposit=2.0, hidden_channels=8, hidden_activation='tanh')
    students = []
    for _ in range(Cn):
        template.model.init_weights()
        students.append(parameters_to_vector(template.model.parameters()).detach().clone())
    bag = BatchedNeuralAutomataAgent(benv, template, torch.stack(students), R_ // Cn)
    bag.parameters.requires_grad_()
    opt = torch.optim.Adam([bag.parameters], lr=0.02)
    target = torch.zeros((3, R_, benv.Nmax), device=DEV)
    for _ in range(10):                                             # let the teacher lay a trail before the lesson
        benv.step(teacher)
    exists = torch.zeros((R_, benv.Nmax), dtype=torch.bool, device=DEV)
    for r in range(R_):
        exists[r, :benv.n[r]] = True
    losses = []
    for _ in range(11):
        got = F.gather_scale_batch(bag.forward_device(), bag)      # looks at the worlds before the teacher moves them …
        live = exists & (benv.alive > 0)
        benv.step(teacher, action=target)                           # … and the teacher's action on those worlds is the target
        loss = (((got[:2] - target[:2]) / scale)[:, live] ** 2).mean()
        losses.append(float(loss.detach()))
        if len(losses) == 11:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    print('nca_wide_grad_batch imitation losses:', ' '.join(f'{v:.3e}' for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
