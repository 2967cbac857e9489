"""The differentiable NeuralAutomataAgent on the GPU (die_conv2d_backward, die_gather_scale_backward behind
`differentiable_sense` / `differentiable_action`) against the float64 torch oracle of tests/nca_grad_model.py.

Shapes: the smallest that cross every edge of the kernels' 16 x 64 tile and both store paths (H % 4 == 0 and not).  Every case
has weights uniform in +-0.5, N = W * H // 7 slots of which a fifth are dead (the alive ones on distinct cells, the dead ones
anywhere), and a standard normal grad_action.

Tolerance (check 2): per layer max|grad_dev - grad_f64| <= 1e-4 * max|grad_f64|.  fp32 torch on a CPU stays at 3e-7 to 9e-7 of
max|grad_f64| on exactly these shapes, two orders below the ceiling, while a wrong tap, halo or flip moves a gradient by about
1 / sqrt(W * H) ~ 3e-2 of it.  The test prints, per layer, the device's error, fp32 torch's and their ratio."""
import functools

import numpy as np
import pytest
import torch

import die_amd as die
from oracle import cpu_ref as R
from tests import dropout_model as M
from tests import nca_grad_model as G

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TOL = 1e-4
COEFS = dict(scale=0.1, deposit=2.0)
CASES = {
    1: dict(W=24, H=40, sizes=(3, 3), boundary='circular'),
    2: dict(W=17, H=66, sizes=(5, 3), boundary='circular'),       # H % 4 != 0, one row and two columns past a tile
    3: dict(W=17, H=66, sizes=(3,), boundary='zeros'),
    4: dict(W=20, H=68, sizes=(3, 3, 3), boundary='circular'),
    5: dict(W=33, H=130, sizes=(7, 1), boundary='zeros'),
    6: dict(W=24, H=40, sizes=(3, 3), boundary='circular', with_agent_channel=False),
    7: dict(W=24, H=40, sizes=(3, 3), boundary='circular', f16=True),
    8: dict(W=24, H=40, sizes=(3, 3), boundary='circular', p=0.25, seed=7),
}
STEP = 5                                                          # the forward-call counter every masked evaluation is made at


def _world(case, shared=False):
    """(env, host medium as the device holds it, cells of every slot, alive flags).  shared: three dead slots on one free cell."""
    c = CASES[case]
    W, H = c['W'], c['H']
    rs = np.random.RandomState(100 + case)
    N = W * H // 7
    dead = rs.permutation(N) < N // 5
    cells = rs.choice(W * H, N, replace=False)
    cx, cy = cells // H, cells % H
    x, y = cx / (W - 1), cy / (H - 1)                             # a cell's own label: the nearest label is that cell
    x[dead], y[dead] = rs.rand(dead.sum()), rs.rand(dead.sum())
    if shared:
        three = np.flatnonzero(dead)[:3]
        x[three], y[three] = x[three[0]], y[three[0]]
    occ = np.zeros((W, H))
    occ[cx[~dead], cy[~dead]] = 1.0
    medium = np.stack([occ, rs.rand(W, H), rs.rand(W, H)])
    agents = np.stack([x, y, (~dead).astype(np.float64), np.ones(N)])
    env = die.Env.from_numpy(medium, agents, field_dtype=torch.float16 if c.get('f16') else torch.float32, device=DEV)
    seen = env.medium.to_numpy()                                  # fp16 fields: the rounded values; the claim plane as 0 / 1
    assert np.array_equal(seen[0], occ)
    a = env.agents.to_numpy()
    return env, seen, (R.cell(a[0], W), R.cell(a[1], H)), ~dead


def _agent(case, device='cpu'):
    c = CASES[case]
    torch.manual_seed(case)
    ag = die.NeuralAutomataAgent(kernel_sizes=c['sizes'], boundary=c['boundary'], with_agent_channel=c.get('with_agent_channel', True),
                                 p_agent_dropout=c.get('p', 0.), dropout_seed=c.get('seed'), **COEFS)
    with torch.no_grad():
        for q in ag.model.parameters():
            q.uniform_(-0.5, 0.5)
    ag.model.to(device)
    assert ag.model.training
    return ag


def _device_grads(ag, env, grad_action, step_world=0):
    """One forward + backward on the device: (action values, [weight gradients])."""
    ag.dropout_step = STEP
    for q in ag.model.parameters():
        q.grad = None
    obs = env._get_current_obs
    act = ag.differentiable_action(obs)
    assert act.requires_grad and act.dtype == torch.float32 and tuple(act.shape) == (3, env.agents.N)
    for _ in range(step_world):                                   # the world moves on between forward and backward
        env.step(ag.forward(env._get_current_obs))
    (act * torch.as_tensor(grad_action, dtype=torch.float32, device=DEV)).sum().backward()
    torch.cuda.synchronize()
    return act.detach().cpu().numpy(), [q.grad.detach().cpu().numpy().copy() for q in ag.model.parameters()]


def _oracle(case, ag, seen, cells, grad_action, dtype=torch.float64):
    c = CASES[case]
    weights = [q.detach().cpu().numpy().astype(np.float64) for q in ag.model.parameters()]
    planes = seen if c.get('with_agent_channel', True) else seen[1:]
    mask = M.mask(c['seed'], STEP, c['W'], c['H'], c['p']).astype(np.float64) if 'p' in c else None
    coefs = (COEFS['scale'], COEFS['scale'], COEFS['deposit'])
    return G.gradients(weights, c['boundary'], planes, cells[0], cells[1], coefs, grad_action, mask, dtype)


def _errors(got, want):
    return [float(np.abs(g - w).max() / np.abs(w).max()) for g, w in zip(got, want)]


@functools.lru_cache(maxsize=None)
def _case(case):
    """Everything the checks of one case share, computed once: the oracle's float64 and float32 gradients, the device's for a full
    grad_action, and twice for one that is zero on the dead slots."""
    env, seen, cells, alive = _world(case)
    ag = _agent(case)
    N = alive.size
    rs = np.random.RandomState(200 + case)
    full = rs.standard_normal((3, N))
    sparse = full * alive[None]
    out = dict(env=env, ag=ag, seen=seen, cells=cells, alive=alive, full=full, sparse=sparse)
    out['act'], out['dev_full'] = _device_grads(ag, env, full)
    _, out['dev_sparse_1'] = _device_grads(ag, env, sparse)
    _, out['dev_sparse_2'] = _device_grads(ag, env, sparse)
    out['act_f64'], out['f64_full'] = _oracle(case, ag, seen, cells, full)
    _, out['f32_full'] = _oracle(case, ag, seen, cells, full, torch.float32)
    _, out['f64_sparse'] = _oracle(case, ag, seen, cells, sparse)
    return out


def _report(case, what, got, f64, f32=None):
    err = _errors(got, f64)
    ref = _errors(f32, f64) if f32 is not None else [float('nan')] * len(err)
    for li, (e, r) in enumerate(zip(err, ref)):
        print(f'nca_grad case {case} {what} layer {li}: device {e:.3e}  fp32 torch {r:.3e}  ratio {e / r if r > 0 else float("nan"):.2f}'
              f'  (of max|grad_f64|; ceiling {TOL:.0e})')
    return err


# ------------------------------------------------------------------------------------------------ 1. the values
@pytest.mark.parametrize('case', sorted(CASES))
def test_values_are_those_of_forward_and_sense(case):
    c = _case(case)
    env, ag = c['env'], c['ag']
    obs = env._get_current_obs
    ag.dropout_step = STEP
    action = ag.forward(obs)
    want = action.data[:, :env.agents.N].cpu().numpy().copy()
    assert ag.dropout_step == STEP + (1 if 'seed' in CASES[case] else 0)
    assert np.array_equal(c['act'], want)
    ag.dropout_step = STEP
    plain = ag.sense(env.medium).cpu().numpy().copy()
    ag.dropout_step = STEP
    diff = ag.differentiable_sense(env.medium)
    assert diff.grad_fn is not None and diff.dtype == torch.float32 and tuple(diff.shape) == (3, env.medium.W, env.medium.H)
    assert ag.dropout_step == STEP + (1 if 'seed' in CASES[case] else 0)          # the counter advances once per differentiable call too
    assert np.array_equal(diff.detach().cpu().numpy(), plain)
    if 'p' in CASES[case]:
        assert (plain == 0).mean() > 0.1                          # the mask was on
    # and the oracle computes the same action (tanhf and fp32 sums against float64)
    assert np.abs(c['act'] - c['act_f64']).max() <= 1e-5 * np.abs(c['act_f64']).max()


# ------------------------------------------------------------------------------------------------ 2. the gradients
@pytest.mark.parametrize('case', sorted(CASES))
def test_weight_gradients_match_the_float64_oracle(case):
    c = _case(case)
    assert [g.shape for g in c['dev_full']] == [w.shape for w in c['f64_full']]
    err = _report(case, 'full', c['dev_full'], c['f64_full'], c['f32_full'])
    assert all(e <= TOL for e in err), err
    err = _report(case, 'dead slots zero', c['dev_sparse_1'], c['f64_sparse'])
    assert all(e <= TOL for e in err), err


# ------------------------------------------------------------------------------------------------ 3. reproducible
@pytest.mark.parametrize('case', sorted(CASES))
def test_two_backward_passes_give_identical_bits(case):
    c = _case(case)
    assert len(set(zip(c['cells'][0][c['alive']].tolist(), c['cells'][1][c['alive']].tolist()))) == int(c['alive'].sum())
    for a, b in zip(c['dev_sparse_1'], c['dev_sparse_2']):
        assert np.array_equal(a, b)
        assert np.abs(a).max() > 0


# ------------------------------------------------------------------------------------------------ 4. slots sharing a cell
def test_slots_sharing_a_cell_add_up():
    case = 1
    env, seen, cells, alive = _world(case, shared=True)
    three = np.flatnonzero(~alive)[:3]
    assert len({(cells[0][n], cells[1][n]) for n in three}) == 1
    ag = _agent(case)
    rs = np.random.RandomState(7)
    grad_action = rs.standard_normal((3, alive.size)) * alive[None]
    grad_action[:, three] = [[1.5, -0.75, 2.25], [0.5, 1.25, -3.0], [-2.0, 0.25, 1.0]]
    _, got = _device_grads(ag, env, grad_action)
    _, want = _oracle(case, ag, seen, cells, grad_action)
    err = _report(case, 'three slots on one cell', got, want)
    assert all(e <= TOL for e in err), err
    # and they matter: without the three the gradient is another one
    grad_action[:, three] = 0
    _, without = _oracle(case, ag, seen, cells, grad_action)
    assert max(_errors(without, want)) > 100 * TOL


# ------------------------------------------------------------------------------------------------ 5. where the model lives
def test_gradients_reach_a_host_model_and_a_device_model():
    c = _case(1)
    host = c['ag']
    assert all(q.device.type == 'cpu' for q in host.model.parameters())
    _, on_host = _device_grads(host, c['env'], c['sparse'])
    assert all(q.grad is not None and q.grad.device.type == 'cpu' and q.grad.shape == q.shape for q in host.model.parameters())
    dev = _agent(1, DEV)
    assert all(q.device.type == 'cuda' for q in dev.model.parameters())
    _, on_dev = _device_grads(dev, c['env'], c['sparse'])
    assert all(q.grad is not None and q.grad.device.type == 'cuda' and q.grad.shape == q.shape for q in dev.model.parameters())
    for a, b, w in zip(on_host, on_dev, c['dev_sparse_1']):
        assert np.array_equal(a, b) and np.array_equal(a, w)
    # a model that asks for no gradients gets a plain tensor
    frozen = _agent(1)
    frozen.model.requires_grad_(False)
    assert not frozen.differentiable_action(c['env']._get_current_obs).requires_grad


# ------------------------------------------------------------------------------------------------ 6. backward after the world moved
@pytest.mark.parametrize('case', [1, 7, 8])
def test_backward_after_env_step_is_the_gradient_at_the_sensed_medium(case):
    c = _case(case)
    env, seen, cells, alive = _world(case)                        # the same world again, stepped here
    assert np.array_equal(seen, c['seen'])
    ag = _agent(case)
    _, got = _device_grads(ag, env, c['sparse'], step_world=3)
    assert not np.array_equal(env.medium.to_numpy(), seen)        # the medium did change under the graph
    err = _report(case, 'after 3 steps', got, c['f64_sparse'])
    assert all(e <= TOL for e in err), err
    for a, b in zip(got, c['dev_sparse_1']):                      # the copies the graph owns are what it read: the same bits
        assert np.array_equal(a, b)


def test_second_backward_without_retain_graph_raises():
    c = _case(1)
    ag, weight = c['ag'], torch.as_tensor(c['sparse'], dtype=torch.float32, device=DEV)      # (zero on the dead slots: fixed bits)
    loss = (ag.differentiable_action(c['env']._get_current_obs) * weight).sum()
    loss.backward()
    with pytest.raises(RuntimeError):
        loss.backward()
    loss = (ag.differentiable_action(c['env']._get_current_obs) * weight).sum()
    grads = []
    for retain in (True, False):                                  # with retain_graph the graph's planes serve a second pass
        for q in ag.model.parameters():
            q.grad = None
        loss.backward(retain_graph=retain)
        grads.append([q.grad.clone() for q in ag.model.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    assert all(np.array_equal(a.numpy(), w) for a, w in zip(grads[0], c['dev_sparse_1']))


def test_torch_rng_mask_is_a_torch_multiply_after_the_function():
    c = _case(1)
    torch.manual_seed(3)
    ag = die.NeuralAutomataAgent(kernel_sizes=(3, 3), p_agent_dropout=0.5, **COEFS)          # no key: nn.Dropout's own mask
    s = ag.differentiable_sense(c['env'].medium)
    assert ag.dropout_step == 0 and s.grad_fn is not None
    host = s.detach().cpu().numpy()
    assert 0.3 < (host[0] == 0).mean() < 0.7 and np.array_equal(host[0] == 0, host[1] == 0)
    s.sum().backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in ag.model.parameters())


# ------------------------------------------------------------------------------------------------ 7. it learns
def test_ten_sgd_steps_towards_a_gradient_agent_lower_the_loss():
    W = H = 32
    env = die.Env((W, H), die.Dynamics(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8), seed=1, device=DEV)
    scale = 0.05
    teacher = die.GradientAgent(max_agents=env.agents.capacity, scale=scale, deposit=2.0, inertia=0.0, noise_scale=0.0, seed=0)
    teacher.lazy = False
    torch.manual_seed(0)
    student = die.NeuralAutomataAgent(kernel_sizes=(3, 3), scale=scale, deposit=2.0)
    student.model.init_weights()
    # the loss is a mean of squares of (scale * tanh - target), |both| <= scale: in units of scale^2 it and its gradient are O(1),
    # and its curvature is bounded by the squared inputs a weight sees (27 taps of fields of order 1, through a second layer of
    # weights below 1): a rate of 0.02 / scale^2 stays well under 2 / curvature, so to first order every step lowers the loss
    opt = torch.optim.SGD(student.model.parameters(), lr=0.02 / scale ** 2)
    for _ in range(10):                                           # a seeded world has no chem yet, and a teacher without a trail to
        env.step(teacher.forward(env._get_current_obs))           # follow asks for nothing: let it lay one before the lesson
    losses = []
    for _ in range(11):
        obs = env._get_current_obs
        N = env.agents.N
        action = teacher.forward(obs)
        target = action.data[:2, :N].clone()
        alive = env.agents.alive[:N] > 0
        got = student.differentiable_action(obs)
        loss = ((got[:2] - target)[:, alive] ** 2).mean()
        losses.append(float(loss.detach()))
        if len(losses) == 11:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
        env.step(action)
    print('nca_grad imitation losses:', ' '.join(f'{v:.3e}' for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


# ------------------------------------------------------------------------------------------------ 8. reflect is refused
@pytest.mark.parametrize('boundary', ['reflect', 'replicate'])
def test_reflect_and_replicate_raise_before_any_launch(boundary):
    c = _case(1)
    env = c['env']
    ag = die.NeuralAutomataAgent(kernel_sizes=(3, 3), boundary=boundary, dropout_seed=1, **COEFS)
    before = env.medium.to_numpy()
    with pytest.raises(NotImplementedError, match='differentiable'):
        ag.differentiable_sense(env.medium)
    with pytest.raises(NotImplementedError, match='differentiable'):
        ag.differentiable_action(env._get_current_obs)
    assert ag.dropout_step == 0 and np.array_equal(env.medium.to_numpy(), before)
    assert tuple(ag.sense(env.medium).shape) == (3, env.medium.W, env.medium.H)               # the forward keeps all four modes
