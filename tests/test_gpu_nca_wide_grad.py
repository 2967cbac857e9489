"""The wide layer's adjoint on the GPU (die_nca_wide_grad.hip): die_conv2d_wide_backward through ctypes on every layer case of
tests/nca_wide_grad_model.py against its float64 model, the adjoint identity on the device's own values, bit-reproducibility,
untouched surroundings, die_amd.functional.conv2d_wide, ConvolutionModel.forward_device against NeuralAutomataAgent.sense and
torch's float64 autograd, and ten Adam steps of the imitation loop with a wide student.

Ceiling: the project's backward tolerance, 1e-4 * max|ref| per array (tests/test_gpu_nca_grad.py, tests/test_gpu_conv_abi.py);
tests/test_nca_wide_grad_cpu.py shows that a plain fp32 evaluation of every case stays within 1e-5 (worst 2.1e-6).  The model is
handed the DEVICE's fp32 forward output as t, so relu's kink cannot split the two.  Every output buffer and the workspace (exactly
the bytes the query names) have a NaN guard band behind them that must come back untouched.  A test enqueues all its launches on
one stream and synchronises once before it reads anything back."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib as L
from die_amd import functional as F
from die_amd.device_array import _ptr, stream_ptr
from tests import dropout_model as D
from tests import nca_wide_grad_model as G

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BWD_TOL = 1e-4
TAIL = 64                                                         # NaN floats behind every buffer
F32, F16, AGENTS = L.DIE_PLANE_F32, L.DIE_PLANE_F16, L.DIE_PLANE_AGENTS
FIRST_LAYER_KINDS = (AGENTS, F16, F32)


@functools.lru_cache(maxsize=None)
def _world():
    """The one small world whose claim plane an 'agents' input reads (G.occupancy: a (W, H) case takes its first W * H words)."""
    from tests import conv_adjoint_model as A
    occ = A.WORLD_OCC
    rs = np.random.RandomState(1)
    env = die.Env.from_numpy(np.stack([occ, rs.rand(*occ.shape), rs.rand(*occ.shape)]), np.array([[0.5], [0.5], [1.0], [1.0]]), device=DEV)
    env.medium._ensure_owner()
    assert np.array_equal(env.medium.to_numpy()[0], occ)
    return env


def _guarded(n):
    return torch.full((n + TAIL,), float('nan'), dtype=torch.float32, device=DEV)


def _planes(x, kinds=None):
    """(tensors kept alive, die_conv_plane array, the float64 values the device reads) of a (cin, W, H) float32 array."""
    cin, W, H = x.shape
    kinds = (F32,) * cin if kinds is None else kinds
    keep, seen = [], np.empty(x.shape)
    for c, kind in enumerate(kinds):
        if kind == AGENTS:
            keep.append(_world().medium.owner.view(-1)[:W * H])
            seen[c] = G.occupancy(W, H)
        elif kind == F16:
            half = x[c].astype(np.float16)
            keep.append(torch.from_numpy(half).to(DEV))
            seen[c] = half
        else:
            keep.append(torch.from_numpy(x[c]).to(DEV))
            seen[c] = x[c]
    return keep, (L.ConvPlane * cin)(*[L.ConvPlane(t.data_ptr(), kind, 0) for t, kind in zip(keep, kinds)]), seen


def _forward(W, H, arr, cin, cout, k, w_dev, act, pad, drop=None):
    out = torch.empty((cout, W, H), dtype=torch.float32, device=DEV)
    L.check(L.lib.die_conv2d_wide(W, H, cin, arr, _world().medium.epoch, cout, _ptr(out), W * H, k, _ptr(w_dev), act, pad,
                                  None if drop is None else C.byref(drop), stream_ptr(DEV)), 'die_conv2d_wide')
    return out


def _backward(W, H, arr, cin, cout, k, w_dev, g_dev, t_dev, act, pad, drop, want_gin=True):
    """One die_conv2d_wide_backward into guarded buffers: (grad_weights, grad_in or None, workspace)."""
    nw = cout * cin * k * k
    need = L.lib.die_conv2d_wide_backward_workspace_bytes(W, H, cin, cout, k)
    assert need == -(-W // 16) * -(-H // 64) * nw * 4
    gw, ws = _guarded(nw), _guarded(need // 4)
    gin = _guarded(cin * W * H) if want_gin else None
    L.check(L.lib.die_conv2d_wide_backward(W, H, cin, arr, _world().medium.epoch, cout, _ptr(g_dev), W * H, _ptr(t_dev), W * H, k, _ptr(w_dev),
                                           act, pad, None if drop is None else C.byref(drop), _ptr(gw), _ptr(gin), W * H, _ptr(ws), need,
                                           stream_ptr(DEV)), 'die_conv2d_wide_backward')
    return gw, gin, ws


def _host(buf, n, shape, what):
    """The first n floats of a guarded buffer as `shape`: all written (no NaN left), and the guard band still NaN."""
    h = buf.cpu().numpy()
    assert np.isnan(h[n:]).all() and h.size == n + TAIL, f'{what}: written behind what the call was given'
    assert not np.isnan(h[:n]).any(), f'{what}: {int(np.isnan(h[:n]).sum())} of {n} elements were never written'
    return h[:n].reshape(shape).astype(np.float64)


def _launch_case(k, mode, cin, cout, W, H, act, masked, kinds=None, want_gin=True):
    c = G.case_inputs(k, mode, cin, cout, W, H)
    pad, a = L.PAD_MODES[mode], L.NCA_ACTIVATIONS[act]
    w_dev, g_dev = torch.from_numpy(c['w']).to(DEV), torch.from_numpy(c['g']).to(DEV)
    keep, arr, seen = _planes(c['x'], kinds)
    drop = L.nca_dropout(G.DROP_P, c['seed'], 0, G.DROP_STEP) if masked else None
    t_dev = _forward(W, H, arr, cin, cout, k, w_dev, a, pad) if act is not None or masked else None
    run = _backward(W, H, arr, cin, cout, k, w_dev, g_dev, t_dev, a, pad, drop, want_gin)
    return dict(c=c, seen=seen, t=t_dev, run=run, keep=(keep, w_dev, g_dev), shape=(k, mode, cin, cout, W, H, act, masked))


def _check_case(job, worst):
    k, mode, cin, cout, W, H, act, masked = job['shape']
    c, where = job['c'], str(job['shape'])
    gw_buf, gin_buf, ws_buf = job['run']
    nw = cout * cin * k * k
    _host(ws_buf, -(-W // 16) * -(-H // 64) * nw, (-1,), f'{where}: workspace')
    t = None if job['t'] is None else job['t'].cpu().numpy()
    if t is not None:
        # the forward the model is handed IS this layer's forward (a wiring check, not the forward's test, which is
        # tests/test_gpu_nca_wide.py: a wrong plane or weight is off by O(1); fp32 sums of up to 800 products of order 0.1 are
        # off by a few 1e-6 of max|z|, about 1e-5 at the largest)
        ref = G.act_forward(G.conv(job['seen'], c['w'], mode), act)
        assert np.abs(t - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max()), (where, 'forward')
    want_w, want_in = G.layer_backward(job['seen'], c['w'], c['g'], t, act, G.case_mask(c, W, H, masked), mode)
    got = [('grad_w', _host(gw_buf, nw, (cout, cin, k, k), f'{where}: grad_weights'), want_w)]
    if gin_buf is not None:
        got.append(('grad_in', _host(gin_buf, cin * W * H, (cin, W, H), f'{where}: grad_in'), want_in))
    for name, have, want in got:
        top, err = np.abs(want).max(), np.abs(have - want).max()
        worst[name] = max(worst.get(name, 0.0), err / top if top > 0 else err)
        assert err <= BWD_TOL * top, (where, name, err / top if top > 0 else err)
    return got


# ------------------------------------------------------------------------------------------------ a. the ABI against the model
@pytest.mark.parametrize('mode', G.MODES)
@pytest.mark.parametrize('k', G.KS)
def test_backward_matches_the_model_on_every_layer_case(k, mode):
    jobs = [_launch_case(k, mode, *case) for case in G.layer_cases(k, mode)]
    # the stack's first layer with a claim plane and an fp16 field among its inputs
    jobs += [_launch_case(k, mode, 3, 16, W, H, None, False, kinds=FIRST_LAYER_KINDS) for W, H in G.SHAPES]
    torch.cuda.synchronize()
    worst = {}
    for job in jobs:
        _check_case(job, worst)
    print(f'wide adjoint abi k = {k} {mode}: ' + '  '.join(f'{n} {v:.2e}' for n, v in worst.items()) +
          f'  (of max|ref| per array; ceiling {BWD_TOL:.0e}; {len(jobs)} cases)')


# ------------------------------------------------------------------------------------------------ b. the adjoint identity
@pytest.mark.parametrize('mode', G.MODES)
@pytest.mark.parametrize('W,H', [(17, 66), (33, 130)])
def test_adjoint_identity_on_the_devices_own_values(W, H, mode):
    k, cin, cout = 5, 32, 32
    c = G.case_inputs(k, mode, cin, cout, W, H)
    pad = L.PAD_MODES[mode]
    w_dev, g_dev = torch.from_numpy(c['w']).to(DEV), torch.from_numpy(c['g']).to(DEV)
    keep, arr, seen = _planes(c['x'])
    y = _forward(W, H, arr, cin, cout, k, w_dev, 0, pad)
    gw, gin, ws = _backward(W, H, arr, cin, cout, k, w_dev, g_dev, None, 0, pad, None)
    torch.cuda.synchronize()
    g64 = c['g'].astype(np.float64)
    lhs = float((y.cpu().numpy().astype(np.float64) * g64).sum())
    via_in = float((seen * _host(gin, cin * W * H, (cin, W, H), 'grad_in')).sum())
    via_w = float((c['w'].astype(np.float64) * _host(gw, cout * cin * k * k, (cout, cin, k, k), 'grad_weights')).sum())
    print(f'wide adjoint identity {W} x {H} {mode}: <conv(x, w), g> = {lhs:.9e}, <x, grad_in> = {via_in:.9e} (apart {abs(lhs - via_in) / abs(lhs):.2e}), '
          f'<w, grad_w> = {via_w:.9e} (apart {abs(lhs - via_w) / abs(lhs):.2e}); ceiling 1e-5')
    assert abs(lhs - via_in) <= 1e-5 * abs(lhs) and abs(lhs - via_w) <= 1e-5 * abs(lhs)


# ------------------------------------------------------------------------------------------------ c. the same bits on every run
def test_two_calls_give_the_same_bits():
    runs = [_launch_case(3, 'circular', 17, 16, 33, 130, 'tanh', True) for _ in range(2)]
    torch.cuda.synchronize()
    (gw0, gin0, _), (gw1, gin1, _) = runs[0]['run'], runs[1]['run']
    nw, n_in = 16 * 17 * 9, 17 * 33 * 130
    assert torch.equal(gw0[:nw], gw1[:nw]) and torch.equal(gin0[:n_in], gin1[:n_in])
    assert not torch.isnan(gw0[:nw]).any() and not torch.isnan(gin0[:n_in]).any() and float(gw0[:nw].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ d. untouched surroundings
@pytest.mark.parametrize('W,H', [(20, 68), (33, 130), (5, 4)])
def test_nothing_is_written_outside_the_calls_buffers(W, H):
    """Both store paths of grad_in (16 bytes where H % 4 == 0, cell by cell otherwise), with and without grad_in: the workspace is
    exactly the stated bytes, and the NaN guard bands behind grad_in, grad_weights and the workspace stay NaN (_host)."""
    jobs = [_launch_case(5, 'zeros', 17, 16, W, H, 'relu', True, want_gin=want) for want in (True, False)]
    jobs.append(_launch_case(3, 'circular', 32, 32, W, H, None, False))
    torch.cuda.synchronize()
    first, without = _check_case(jobs[0], {}), _check_case(jobs[1], {})
    _check_case(jobs[2], {})
    assert len(first) == 2 and len(without) == 1
    assert np.array_equal(first[0][1], without[0][1]), 'grad_weights depend on whether grad_in was asked for'


# ------------------------------------------------------------------------------------------------ e. functional.conv2d_wide
@pytest.mark.parametrize('case', [(3, 'zeros', 17, 16, 17, 66, 'tanh', True), (5, 'circular', 32, 32, 20, 68, 'relu', False),
                                  (1, 'circular', 3, 16, 33, 130, None, False), (3, 'circular', 16, 3, 20, 68, None, True)])
def test_functional_conv2d_wide_values_and_gradients(case, monkeypatch):
    k, mode, cin, cout, W, H, act, masked = case
    c = G.case_inputs(k, mode, cin, cout, W, H)
    dropout = (G.DROP_P, c['seed'], G.DROP_STEP) if masked else None
    drop = L.nca_dropout(G.DROP_P, c['seed'], 0, G.DROP_STEP) if masked else None
    x = torch.from_numpy(c['x']).to(DEV).requires_grad_(True)
    w = torch.from_numpy(c['w']).to(DEV).requires_grad_(True)
    g = torch.from_numpy(c['g']).to(DEV)
    calls = []
    real = F._launch_backward
    monkeypatch.setattr(F, '_launch_backward', lambda *a: calls.append(a[-1]) or real(*a))
    y = F.conv2d_wide(x, w, activation=act, padding_mode=mode, dropout=dropout)
    assert y.grad_fn is not None and y.shape == (cout, W, H)
    keep, arr, seen = _planes(c['x'])
    direct = _forward(W, H, arr, cin, cout, k, w.detach(), L.NCA_ACTIVATIONS[act], L.PAD_MODES[mode], drop)
    t = _forward(W, H, arr, cin, cout, k, w.detach(), L.NCA_ACTIVATIONS[act], L.PAD_MODES[mode])
    assert torch.equal(y.detach(), direct)
    gw, gx = torch.autograd.grad(y, (w, x), g)
    # the weight alone: no gradient at the input is computed (grad_in = NULL: the input-gradient kernel is not launched)
    x2 = x.detach().clone()
    y2 = F.conv2d_wide(x2, w, activation=act, padding_mode=mode, dropout=dropout)
    (gw2,) = torch.autograd.grad(y2, (w,), g)
    assert calls == [True, False] and torch.equal(y2.detach(), direct) and torch.equal(gw2, gw)
    want_w, want_in = G.layer_backward(seen, c['w'], c['g'], t.cpu().numpy(), act, G.case_mask(c, W, H, masked), mode)
    for name, have, want in (('grad_w', gw, want_w), ('grad_in', gx, want_in)):
        err, top = np.abs(have.cpu().numpy() - want).max(), np.abs(want).max()
        print(f'functional.conv2d_wide {case}: {name} {err / top:.2e} of max|ref| (ceiling {BWD_TOL:.0e})')
        assert err <= BWD_TOL * top, (name, err / top)
    with torch.no_grad():
        assert F.conv2d_wide(x, w, activation=act, padding_mode=mode, dropout=dropout).grad_fn is None


@pytest.mark.parametrize('mode', ['reflect', 'replicate'])
def test_functional_refuses_the_forward_only_paddings_with_a_gradient_and_computes_them_without(mode, monkeypatch):
    c = G.case_inputs(3, 'zeros', 3, 16, 17, 66)
    x, w = torch.from_numpy(c['x']).to(DEV), torch.from_numpy(c['w']).to(DEV).requires_grad_(True)
    launched = []
    real = F._launch_forward
    monkeypatch.setattr(F, '_launch_forward', lambda *a: launched.append(1) or real(*a))
    with pytest.raises(NotImplementedError, match=mode):
        F.conv2d_wide(x, w, activation='tanh', padding_mode=mode)
    assert not launched
    with torch.no_grad():
        y = F.conv2d_wide(x, w, activation='tanh', padding_mode=mode)
    keep, arr, _ = _planes(c['x'])
    assert launched == [1] and torch.equal(y, _forward(17, 66, arr, 3, 16, 3, w.detach(), 1, L.PAD_MODES[mode]))


# ------------------------------------------------------------------------------------------------ f. a whole stack
def _stack_agent(width, ks, act, weights, **kw):
    ag = die.NeuralAutomataAgent(kernel_sizes=ks, hidden_channels=width, hidden_activation=act, scale=0.07, deposit=1.5, **kw)
    with torch.no_grad():
        for layer, w in zip(ag.model.conv_layers(), weights):
            assert layer.weight.shape == w.shape
            layer.weight.copy_(torch.from_numpy(w))
    return ag


@pytest.mark.parametrize('W,H', G.STACK_FIELDS)
@pytest.mark.parametrize('stack', G.STACKS, ids=lambda s: f'{s[0]}-{s[2]}')
def test_forward_device_is_sense_and_its_gradients_match_torch_float64(stack, W, H):
    width, ks, act, seed = stack
    planes, weights, g = G.stack_case(width, ks, act, seed, W, H)
    q32 = lambda v: np.floor(v * 2.0 ** 32) / 2.0 ** 32
    rs = np.random.RandomState(seed)
    agents = np.stack([q32(rs.rand(24) * 0.999999), q32(rs.rand(24) * 0.999999), np.ones(24), np.ones(24)])
    env = die.Env.from_numpy(planes.astype(np.float64), agents, device=DEV)
    p, dseed = G.STACK_DROP
    ag = _stack_agent(width, ks, act, weights)
    model = ag.model
    dev_planes = torch.stack([env.medium.sel(c).float() for c in ag.obs_channels])
    assert np.array_equal(dev_planes.cpu().numpy(), planes)
    # values: the same launches as sense, plain and with the seeded mask at dropout_step 0 and 1
    with torch.no_grad():
        assert torch.equal(model.forward_device(dev_planes), ag.sense(env.medium))
    masked = _stack_agent(width, ks, act, weights, p_agent_dropout=p, dropout_seed=dseed)
    masked.train()
    for step in (0, 1):
        assert masked.dropout_step == step
        want = masked.sense(env.medium).clone()
        with torch.no_grad():
            got = masked.model.forward_device(dev_planes, dropout=(p, dseed, step))
        assert torch.equal(got, want)
        assert np.array_equal((want.cpu().numpy() == 0).all(axis=0) | (D.mask(dseed, step, W, H, p) != 0), np.ones((W, H), dtype=bool))
    # parameter gradients, plain and masked at step 1, against torch float64 autograd of the same module on the CPU
    g_dev = torch.from_numpy(g).to(DEV)
    for dropout in (None, (p, dseed, 1)):
        model.zero_grad()
        out = model.forward_device(dev_planes, dropout=dropout)
        assert out.grad_fn is not None
        (out * g_dev).sum().backward()
        m64 = copy.deepcopy(model).double()
        m64.zero_grad()
        ref = m64.kernels(torch.from_numpy(planes.astype(np.float64))[None])[0]
        if dropout is not None:
            ref = ref * torch.from_numpy(D.mask(dseed, 1, W, H, p).astype(np.float64))
            assert torch.equal(out.detach(), got)
        assert np.abs(out.detach().cpu().numpy() - ref.detach().numpy()).max() <= 1e-5
        (ref * torch.from_numpy(g.astype(np.float64))).sum().backward()
        for li, (layer, layer64) in enumerate(zip(model.conv_layers(), m64.conv_layers())):
            have, want = layer.weight.grad.numpy().astype(np.float64), layer64.weight.grad.numpy()
            err, top = np.abs(have - want).max(), np.abs(want).max()
            print(f'forward_device {width}-{act} {W} x {H} mask={dropout is not None}: layer {li} grad {err / top:.2e} of max|ref| (ceiling {BWD_TOL:.0e})')
            assert top > 0 and err <= BWD_TOL * top, (li, err / top)


def test_forward_device_refuses_a_narrow_model():
    model = die.ConvolutionModel(kernel_sizes=(3, 3))
    with pytest.raises(ValueError, match='narrow'):
        model.forward_device(torch.zeros((3, 8, 8), device=DEV))


# ------------------------------------------------------------------------------------------------ g. it learns
def test_ten_adam_steps_of_the_imitation_loop_lower_the_loss_of_a_wide_student():
    W = H = 32
    env = die.Env((W, H), die.Dynamics(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8), seed=1, device=DEV)
    scale = 0.05
    teacher = die.GradientAgent(max_agents=env.agents.capacity, scale=scale, deposit=2.0, inertia=0.0, noise_scale=0.0, seed=0)
    teacher.lazy = False
    torch.manual_seed(0)
    student = die.NeuralAutomataAgent(kernel_sizes=(3, 3), hidden_channels=8, hidden_activation='tanh', scale=scale, deposit=2.0)
    student.model.init_weights()
    opt = torch.optim.Adam(student.model.parameters(), lr=0.01)
    for _ in range(10):                                           # let the teacher lay a trail to follow before the lesson
        env.step(teacher.forward(env._get_current_obs))
    losses = []
    for _ in range(11):
        obs = env._get_current_obs
        agents, medium = obs
        N = agents.N
        action = teacher.forward(obs)
        target = action.data[:2, :N].clone()
        alive = agents.alive[:N] > 0
        planes = torch.stack([medium.sel(c).float() for c in student.obs_channels])
        got = F.gather_scale(student.model.forward_device(planes), obs, student.action_coefs)
        loss = (((got[:2] - target) / scale)[:, alive] ** 2).mean()
        losses.append(float(loss.detach()))
        if len(losses) == 11:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
        env.step(action)
    print('wide imitation losses:', ' '.join(f'{v:.3e}' for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
