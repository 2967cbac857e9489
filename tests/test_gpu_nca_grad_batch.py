"""The differentiable NeuralAutomataAgent population on the GPU (die_nca_sense_batch_store, die_gather_scale_batch and their adjoints
die_gather_scale_backward_batch, die_nca_backward_batch behind BatchedNeuralAutomataAgent.differentiable_sense / _action), and
BatchedEnv.step(..., action=...).

The invariant is the batch's: replica r is, bit for bit, the stand-alone computation on replica r's world — here the stand-alone
NeuralAutomataAgent.differentiable_action of tests/test_gpu_nca_grad.py on the world `replica_numpy(r)` loaded into an Env.

Shapes: the smallest that cross the kernels' 16 x 64 tile's edges with H % 4 == 0 (which the batched step requires).  Every world is
stepped twice first, so that there is a trail to sense.  The weights are uniform in +-0.5; the upstream gradient is standard normal,
zero on dead and padding slots and on alive slots that share a cell with an earlier one (`_upstream`: the read-out's adjoint has
fixed bits only when no two slots with a non-zero gradient share a cell).

Tolerance of the E > 1 check: per layer max|row_c - sum_e grad_f64(c, e)| <= 1e-4 * max|sum_e grad_f64|, the ceiling
tests/test_gpu_nca_grad.py derives (fp32 torch stays two orders below it; a wrong tap, halo, flip or fold moves a gradient by a few
per cent of it); the test prints the device's error next to fp32 torch's."""
import functools

import numpy as np
import pytest
import torch
from torch.nn.utils import parameters_to_vector

import die_amd as die
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent, BatchedPhysarumAgent
from oracle import cpu_ref as R
from tests import dropout_model as M
from tests import nca_grad_model as G

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TOL = 1e-4
COEFS = dict(scale=0.1, deposit=2.0)
DYN = dict(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8)
CASES = {
    'two layers': dict(W=24, H=40, sizes=(3, 3), R=3),
    'three layers': dict(W=20, H=68, sizes=(3, 3, 3), R=2),
    'k7 k1 zeros': dict(W=33, H=132, sizes=(7, 1), R=2, boundary='zeros'),
    'no agent channel': dict(W=24, H=40, sizes=(3, 3), R=3, with_agent_channel=False),
    'fp16 fields': dict(W=24, H=40, sizes=(3, 3), R=3, f16=True),
    'dropout stride 0': dict(W=24, H=40, sizes=(3, 3), R=3, p=0.25, seed=7, stride=0),
    'dropout stride 1': dict(W=24, H=40, sizes=(3, 3), R=3, p=0.25, seed=7, stride=1),
    'fixed slots': dict(W=24, H=40, sizes=(3, 3), R=3, fixed=True),              # max_agents=None: W * H slots, a dead tail
    'per-replica dynamics': dict(W=24, H=40, sizes=(3, 3), R=3, rows=True),
    'two episodes': dict(W=24, H=40, sizes=(3, 3), R=4, E=2),
    'one candidate': dict(W=24, H=40, sizes=(3, 3), R=3, E=3),
}
E1 = [k for k, c in CASES.items() if c.get('E', 1) == 1]
EN = [k for k, c in CASES.items() if c.get('E', 1) > 1]


def _dynamics(c):
    if not c.get('rows'):
        return die.Dynamics(**DYN)
    return [die.Dynamics(food_infinite=True, rate_decay_chem=0.02 + 0.01 * r, diffuse_sigma=0.6 + 0.2 * r) for r in range(c['R'])]


def _template(c):
    torch.manual_seed(1)
    ag = die.NeuralAutomataAgent(kernel_sizes=c['sizes'], boundary=c.get('boundary', 'circular'),
                                 with_agent_channel=c.get('with_agent_channel', True), p_agent_dropout=c.get('p', 0.), **COEFS)
    assert ag.model.training
    return ag


def _build(name):
    """(BatchedEnv, population) of a case: weights uniform in +-0.5, the worlds stepped twice."""
    c = CASES[name]
    benv = BatchedEnv((c['W'], c['H']), _dynamics(c), replicas=c['R'], seed=11, field_dtype=torch.float16 if c.get('f16') else torch.float32,
                      max_agents=None if c.get('fixed') else 'alive', device=DEV)
    template = _template(c)
    E = c.get('E', 1)
    P = sum(k.weight.numel() for k in template.model.conv_layers())
    rows = (torch.rand((c['R'] // E, P), generator=torch.Generator().manual_seed(5)) - 0.5)
    drop = dict(dropout_seed=c['seed'], dropout_seed_stride=c['stride']) if 'p' in c else {}
    bag = BatchedNeuralAutomataAgent(benv, template, rows, E, **drop)
    benv.run(bag, 2)
    return benv, bag


def _upstream(benv, seed=3):
    """(3, R, Nmax) standard normal, zero on dead and padding slots — and on every alive slot that stands on a cell an earlier alive
    slot of its replica stands on.  Agents that have moved may meet on a cell, and the read-out's adjoint adds the slots of one cell
    with fp32 atomics in arrival order: its bits (stand-alone and batched alike) are fixed only when no two slots with a non-zero
    gradient share a cell, which is the condition under which "bit for bit" is promised."""
    g = torch.randn((3, benv.R, benv.Nmax), generator=torch.Generator().manual_seed(seed)).to(DEV)
    live = (benv.alive > 0).cpu().numpy()
    shared = 0
    for r in range(benv.R):
        live[r, benv.n[r]:] = False
        _, a = benv.replica_numpy(r)
        cells = R.cell(a[0], benv.W).astype(np.int64) * benv.H + R.cell(a[1], benv.H)
        seen = set()
        for n in np.flatnonzero(live[r]):
            if int(cells[n]) in seen:
                live[r, n] = False
                shared += 1
            seen.add(int(cells[n]))
    print(f'nca_grad_batch upstream: {int(live.sum())} slots with a gradient, {shared} alive slots zeroed for sharing a cell')
    return g * torch.as_tensor(live, device=DEV)[None]


def _batched(benv, bag, g, steps_between=0):
    """One batched forward + backward: (action, (C, P) gradient) as numpy."""
    p = bag.parameters.detach().clone().requires_grad_()
    act = bag.differentiable_action(p)
    assert act.grad_fn is not None and act.dtype == torch.float32 and tuple(act.shape) == (3, benv.R, benv.Nmax)
    for _ in range(steps_between):
        benv.step(bag)
    (act * g).sum().backward()
    torch.cuda.synchronize()
    assert tuple(p.grad.shape) == tuple(bag.parameters.shape)
    return act.detach().cpu().numpy(), p.grad.cpu().numpy().copy()


def _stand_alone(benv, bag, g, r, step):
    """Replica r's world in a stand-alone Env, sensed by replica r's stand-alone agent: (action, flat gradient, env, agent)."""
    medium, agents = benv.replica_numpy(r)
    env = die.Env.from_numpy(medium, agents, field_dtype=benv.dtype, device=DEV)
    ag = bag.replica_agent(r)
    ag.dropout_step = step
    act = ag.differentiable_action(env._get_current_obs)
    assert tuple(act.shape) == (3, benv.n[r])
    (act * g[:, r, :benv.n[r]]).sum().backward()
    torch.cuda.synchronize()
    grad = parameters_to_vector([q.grad for q in ag.model.parameters()]).cpu().numpy()
    return act.detach().cpu().numpy(), grad, env, ag


@functools.lru_cache(maxsize=None)
def _case(name):
    """Everything the checks of a case share, computed once: the batched action and gradient (twice), the stand-alone ones."""
    benv, bag = _build(name)
    g = _upstream(benv)
    step = bag.dropout_step
    out = dict(benv=benv, bag=bag, g=g, step=step)
    out['act'], out['grad'] = _batched(benv, bag, g)
    out['step_after'] = bag.dropout_step
    bag.dropout_step = step
    _, out['grad_again'] = _batched(benv, bag, g)
    out['alone'] = [_stand_alone(benv, bag, g, r, step) for r in range(benv.R)]
    return out


def _layers(bag, row):
    """A flat (P,) row cut into the layers' blocks."""
    return [row[off:off + cout * cin * k * k] for k, cin, cout, off in bag._layers]


# ------------------------------------------------------------------------------------------------ 1. the values
@pytest.mark.parametrize('name', sorted(CASES))
def test_values_are_the_stand_alone_ones(name):
    c = _case(name)
    benv = c['benv']
    assert c['step_after'] == c['step'] + (1 if 'seed' in CASES[name] else 0)      # once per call, as the stand-alone twin
    for r in range(benv.R):
        want = c['alone'][r][0]
        assert np.array_equal(c['act'][:, r, :benv.n[r]], want), r
        assert np.all(c['act'][:, r, benv.n[r]:] == 0), r
        assert np.abs(want).max() > 0
    if 'p' in CASES[name]:
        assert (c['act'][0] == 0).mean() > 0.1                                      # the mask was on


def test_differentiable_sense_is_the_stand_alone_one():
    c = _case('dropout stride 1')
    benv, bag = c['benv'], c['bag']
    bag.dropout_step = c['step']
    s = bag.differentiable_sense()
    assert s.grad_fn is None and tuple(s.shape) == (benv.R, 3, benv.W, benv.H) and s.dtype == torch.float32     # no leaf asked for a gradient
    assert bag.dropout_step == c['step'] + 1
    p = bag.parameters.detach().clone().requires_grad_()
    bag.dropout_step = c['step']
    s = bag.differentiable_sense(p)
    assert s.grad_fn is not None
    for r in range(benv.R):
        _, _, env, ag = c['alone'][r]
        ag.dropout_step = c['step']
        assert np.array_equal(s[r].detach().cpu().numpy(), ag.sense(env.medium).cpu().numpy()), r
    keys = [bag._replica_dropout_seed(r) for r in range(benv.R)]
    assert keys == [7, 8, 9]
    mask0 = M.mask(7, c['step'], benv.W, benv.H, 0.25)
    assert np.array_equal(s[0, 0].detach().cpu().numpy() == 0, mask0 == 0)


# ------------------------------------------------------------------------------------------------ 2. E = 1: bit for bit
@pytest.mark.parametrize('name', E1)
def test_gradient_rows_are_the_stand_alone_gradients(name):
    c = _case(name)
    bag = c['bag']
    for r in range(c['benv'].R):
        for li, (got, want) in enumerate(zip(_layers(bag, c['grad'][r]), _layers(bag, c['alone'][r][1]))):
            assert np.array_equal(got, want), (r, li, np.abs(got - want).max())
            assert np.abs(want).max() > 0, (r, li)


# ------------------------------------------------------------------------------------------------ 3. E > 1: the float64 oracle
@pytest.mark.parametrize('name', EN)
def test_episode_rows_match_the_float64_sum(name):
    c = _case(name)
    benv, bag, spec = c['benv'], c['bag'], CASES[name]
    E = spec['E']
    coefs = (COEFS['scale'], COEFS['scale'], COEFS['deposit'])
    g = c['g'].cpu().numpy().astype(np.float64)
    for cand in range(benv.R // E):
        weights = [q.detach().cpu().numpy().astype(np.float64) for q in bag.candidate(cand).model.parameters()]
        total = {torch.float64: None, torch.float32: None}
        for e in range(E):
            r = cand * E + e
            env = c['alone'][r][2]
            a = env.agents.to_numpy()
            cx, cy = R.cell(a[0], benv.W), R.cell(a[1], benv.H)
            for dt in total:
                _, grads = G.gradients(weights, 'circular', env.medium.to_numpy(), cx, cy, coefs, g[:, r, :benv.n[r]], None, dt)
                total[dt] = grads if total[dt] is None else [x + y for x, y in zip(total[dt], grads)]
        for li, (got, f64, f32) in enumerate(zip(_layers(bag, c['grad'][cand]), total[torch.float64], total[torch.float32])):
            top = np.abs(f64).max()
            err, ref = float(np.abs(got - f64.ravel()).max() / top), float(np.abs(f32 - f64).max() / top)
            print(f'nca_grad_batch {name} candidate {cand} layer {li}: device {err:.3e}  fp32 torch {ref:.3e}  (of max|sum grad_f64|; '
                  f'ceiling {TOL:.0e})')
            assert err <= TOL, (cand, li, err)
        # and the row is not one replica's gradient: the episodes were folded
        assert not np.array_equal(c['grad'][cand], c['alone'][cand * E][1])


# ------------------------------------------------------------------------------------------------ 4. reproducible
@pytest.mark.parametrize('name', sorted(CASES))
def test_two_backward_passes_give_identical_bits(name):
    c = _case(name)
    assert np.array_equal(c['grad'], c['grad_again']) and np.abs(c['grad']).max() > 0


# ------------------------------------------------------------------------------------------------ 5. backward after the worlds moved
@pytest.mark.parametrize('name', ['two layers', 'dropout stride 1', 'fp16 fields'])
def test_backward_after_two_steps_is_the_gradient_at_the_sensed_worlds(name):
    c = _case(name)
    benv, bag = _build(name)                                        # the same worlds again, stepped here
    assert bag.dropout_step == c['step']
    before = benv.replica_numpy(0)[0]
    _, got = _batched(benv, bag, c['g'], steps_between=2)
    assert not np.array_equal(benv.replica_numpy(0)[0], before)     # the worlds did change under the graph
    assert np.array_equal(got, c['grad'])


# ------------------------------------------------------------------------------------------------ 6. the graph is freed
def test_second_backward_without_retain_graph_raises():
    c = _case('two layers')
    benv, bag = c['benv'], c['bag']
    p = bag.parameters.detach().clone().requires_grad_()
    loss = (bag.differentiable_action(p) * c['g']).sum()
    loss.backward()
    with pytest.raises(RuntimeError):
        loss.backward()
    loss = (bag.differentiable_action(p) * c['g']).sum()
    grads = []
    for retain in (True, False):
        p.grad = None
        loss.backward(retain_graph=retain)
        grads.append(p.grad.clone())
    assert torch.equal(grads[0], grads[1]) and np.array_equal(grads[0].cpu().numpy(), c['grad'])


def test_parameters_may_be_the_leaf_itself():
    """`self.parameters` marked requires_grad_(): the gradient lands there, steps and set_parameters keep working."""
    c = _case('two layers')
    benv, bag = _build('two layers')
    bag.parameters.requires_grad_()
    (bag.differentiable_action() * c['g']).sum().backward()
    assert np.array_equal(bag.parameters.grad.cpu().numpy(), c['grad'])
    benv.step(bag)
    bag.set_parameters(torch.zeros_like(bag.parameters))
    assert bag.parameters.requires_grad and float(bag.parameters.detach().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_large_worlds_and_reflect_raise_before_any_launch():
    c = CASES['two layers']
    big = BatchedEnv((c['W'], c['H']), die.Dynamics(**DYN), replicas=2, seed=11, per_replica=True, device=DEV)
    bag = BatchedNeuralAutomataAgent(big, _template(c), dropout_seed=1)
    for call in (bag.differentiable_action, bag.differentiable_sense):
        with pytest.raises(NotImplementedError, match='per_replica'):
            call()
    with pytest.raises(NotImplementedError, match='per_replica'):
        big.step(bag, action=torch.zeros((3, 2, big.Nmax), device=DEV))
    assert bag.dropout_step == 0
    benv = BatchedEnv((c['W'], c['H']), die.Dynamics(**DYN), replicas=2, seed=11, device=DEV)
    before = [benv.replica_numpy(r) for r in range(2)]
    for boundary in ('reflect', 'replicate'):
        ag = die.NeuralAutomataAgent(kernel_sizes=(3, 3), boundary=boundary, **COEFS)
        bag = BatchedNeuralAutomataAgent(benv, ag, dropout_seed=1)
        for call in (bag.differentiable_action, bag.differentiable_sense):
            with pytest.raises(NotImplementedError, match='differentiable'):
                call()
        assert bag.dropout_step == 0
    drop = BatchedNeuralAutomataAgent(benv, die.NeuralAutomataAgent(kernel_sizes=(3, 3), p_agent_dropout=0.5, **COEFS))
    with pytest.raises(NotImplementedError, match='dropout'):       # no dropout_seed: the existing refusal
        drop.differentiable_action()
    ok = BatchedNeuralAutomataAgent(benv, _template(c))
    with pytest.raises(ValueError):
        ok.differentiable_action(torch.zeros((3, ok.P), device=DEV))
    with pytest.raises(ValueError):
        benv.step(ok, action=torch.zeros((3, 2, benv.Nmax + 1), device=DEV))
    for r in range(2):
        assert all(np.array_equal(x, y) for x, y in zip(before[r], benv.replica_numpy(r)))
    assert benv.epoch == 1 and benv._steps == 0


# ------------------------------------------------------------------------------------------------ 8. step(action=...)
def _worlds(seed, R=3, **kw):
    return BatchedEnv((24, 40), die.Dynamics(**DYN), replicas=R, seed=seed, device=DEV, **kw)


@pytest.mark.parametrize('kind', ['physarum', 'nca'])
def test_step_writes_the_actions_the_stand_alone_agents_took(kind):
    W, H, R_, steps = 24, 40, 3, 3
    pkw = dict(scale=0.05, sense_offset=0.2)
    sizes = (3, 3)

    def agent_of(benv):
        if kind == 'physarum':
            return BatchedPhysarumAgent(benv, seed=7, **pkw)
        return BatchedNeuralAutomataAgent(benv, _template(dict(sizes=sizes)),
                                          torch.rand((R_, 162), generator=torch.Generator().manual_seed(2)) - 0.5)

    with_out, without = _worlds(40), _worlds(40)
    a, b = agent_of(with_out), agent_of(without)
    out = torch.full((3, R_, with_out.Nmax), 123.0, device=DEV)
    res_a, res_b = [], []
    for _ in range(steps):
        res_a.append(with_out.step(a, action=out).clone())
        res_b.append(without.step(b).clone())
    torch.cuda.synchronize()
    assert len(set(with_out.n)) > 1
    # the step itself does not change with it
    assert torch.equal(torch.stack(res_a), torch.stack(res_b))
    for r in range(R_):
        assert all(np.array_equal(x, y) for x, y in zip(with_out.replica_numpy(r), without.replica_numpy(r))), r
    # the last step's actions are the stand-alone agents'
    host = out.cpu().numpy()
    for r in range(R_):
        env = die.Env((W, H), die.Dynamics(**DYN), seed=40 + r, max_agents='alive', device=DEV)
        ag = die.PhysarumAgent(max_agents=env.agents.N, seed=7 + r, **pkw) if kind == 'physarum' else a.replica_agent(r)
        obs = env._get_current_obs
        for _ in range(steps):
            action = ag.forward(obs)
            obs = env.step(action)[0]
        torch.cuda.synchronize()
        n = with_out.n[r]
        assert n == env.agents.N
        assert np.array_equal(host[:, r, :n], action.data[:3, :n].cpu().numpy()), r
        assert np.all(host[:, r, n:] == 123.0), r                   # the padding is left alone
        assert np.array_equal(with_out.replica_numpy(r)[0], env.medium.to_numpy()), r


# ------------------------------------------------------------------------------------------------ 9. it learns
def test_ten_adam_steps_of_batched_imitation_lower_the_loss():
    """The batched twin of test_ten_sgd_steps_towards_a_gradient_agent_lower_the_loss: four worlds, four students side by side, the
    teacher a BatchedPhysarumAgent whose actions come out of step(action=...).  A Physarum's heading is a state, not a function of
    the cells around it, so what can be learnt at once is mostly to shrink the outputs towards the targets' size — enough for a loss
    that is a mean of squares in units of scale^2 to fall."""
    R_, scale = 4, 0.05
    benv = _worlds(1, R=R_)
    teacher = BatchedPhysarumAgent(benv, scale=scale, deposit=0.5, seed=0)
    torch.manual_seed(0)
    template = die.NeuralAutomataAgent(kernel_sizes=(3, 3), scale=scale, deposit=2.0)
    students = []
    for _ in range(R_):
        template.model.init_weights()
        students.append(parameters_to_vector(template.model.parameters()).detach().clone())
    bag = BatchedNeuralAutomataAgent(benv, template, torch.stack(students))
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
        got = bag.differentiable_action()                          # looks at the worlds before the teacher moves them …
        live = exists & (benv.alive > 0)
        benv.step(teacher, action=target)                           # … and the teacher's action on those worlds is the target
        loss = (((got[:2] - target[:2]) / scale)[:, live] ** 2).mean()
        losses.append(float(loss.detach()))
        if len(losses) == 11:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    print('nca_grad_batch imitation losses:', ' '.join(f'{v:.3e}' for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
