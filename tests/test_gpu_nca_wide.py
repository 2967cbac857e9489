"""Wide NeuralAutomataAgent stacks on the GPU (die_conv2d_wide, die_nca_wide_env_step_batch): the stand-alone agent and the layer
entry point against the float64 model of tests/nca_wide_model.py and torch's fp32 evaluation at 1e-5 (the project's parity
tolerance, tests/test_gpu_parity.py), the dropout mask exactly, replica r of a batched population against its stand-alone run bit
for bit, the searchers on the larger parameter vector, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent
from die_amd.device_array import _ptr
from die_amd.search import CMAES, PGPE
from tests import dropout_model as D
from tests import nca_wide_model as M

pytestmark = pytest.mark.gpu

REFERENCE_DYNAMICS = dict(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8)     # examples/learning_agents.py
DEV = 'cuda:0'
ATOL = 1e-5
WIDTHS = [5, 16, 17, 32]            # one padded N-block, an exact one, two with a ragged second, the maximum
SCALE, DEPOSIT = 0.07, 1.5


def _world(W, H, f16=False, n=24):
    """(medium, agents) numpy arrays the device holds exactly: Q0.32 coordinates, fields rounded to their dtype."""
    rs = np.random.RandomState(W * 31 + H)
    field = lambda: rs.rand(W, H).astype(np.float16 if f16 else np.float32).astype(np.float64)
    medium = np.stack([(rs.rand(W, H) < 0.15).astype(np.float64), field(), field()])
    q32 = lambda v: np.floor(v * 2.0 ** 32) / 2.0 ** 32
    agents = np.stack([q32(rs.rand(n) * 0.999999), q32(rs.rand(n) * 0.999999), np.ones(n), np.ones(n)])
    return medium, agents


def _agent(seed, **kw):
    torch.manual_seed(seed)
    ag = die.NeuralAutomataAgent(scale=SCALE, deposit=DEPOSIT, **kw)
    ag.model.init_weights()
    return ag


def _check_agent(ag, medium, agents, f16=False, step=False):
    """forward on the device against the float64 model and torch's fp32 forward of the same module."""
    env = die.Env.from_numpy(medium, agents, field_dtype=torch.float16 if f16 else torch.float32)
    action = ag.forward(env._get_current_obs)
    got = ag._sense_output.cpu().numpy().astype(np.float64)
    planes = medium if len(ag.obs_channels) == 3 else medium[1:]
    ws = [k.weight.detach().numpy() for k in ag.model.conv_layers()]
    boundary = ag.model.conv_layers()[0].padding_mode
    want = M.sense(planes, ws, ag.model.hidden_activation, boundary)
    err = float(np.abs(got - want).max())
    assert got.shape == want.shape and err <= ATOL, err
    with torch.no_grad():
        fp32 = ag.model(torch.from_numpy(planes.astype(np.float32))[None])[0].numpy()
    assert np.abs(got - fp32).max() <= ATOL
    want_action = M.read_out(want, agents[0], agents[1], SCALE, DEPOSIT)
    assert np.abs(action.to_numpy() - want_action).max() <= ATOL
    assert ag.render()[0].shape == (*medium.shape[1:], 3)
    if step:
        env.step(action)                                          # the action drives an env step like any other
        torch.cuda.synchronize()
    return err


# ---------------------------------------------------------------------------------------------------- a. stand-alone parity
@pytest.mark.parametrize('kernel_sizes', [(3, 3), (3, 1, 3), (5, 3)])
@pytest.mark.parametrize('W,H', [(12, 8), (30, 50), (64, 130), (96, 96)])     # below a tile; H % 4 != 0; three ragged column tiles
def test_stand_alone_forward_parity(W, H, kernel_sizes):
    medium, agents = _world(W, H)
    worst = 0.0
    for width in WIDTHS:
        for activation in (None, 'tanh', 'relu'):
            ag = _agent(W + width, kernel_sizes=kernel_sizes, hidden_channels=width, hidden_activation=activation)
            worst = max(worst, _check_agent(ag, medium, agents, step=width == 32 and activation == 'tanh'))
    print(f'{W}x{H} {kernel_sizes}: device against the float64 model: {worst:.2e}')


@pytest.mark.parametrize('W,H,kw,f16', [
    (30, 50, dict(boundary='zeros', hidden_channels=17, hidden_activation='relu', kernel_sizes=(5, 3)), False),
    (12, 8, dict(boundary='reflect', hidden_channels=16, hidden_activation='tanh', kernel_sizes=(3, 5, 3)), False),
    (64, 130, dict(boundary='replicate', hidden_channels=32, kernel_sizes=(3, 3)), False),
    (96, 96, dict(hidden_channels=16, hidden_activation='tanh', kernel_sizes=(3, 1, 3)), True),                # fp16 fields
    (30, 50, dict(boundary='zeros', hidden_channels=5, kernel_sizes=(3, 3)), True),
    (96, 96, dict(with_agent_channel=False, hidden_channels=32, hidden_activation='relu', kernel_sizes=(3, 3)), False),
    (17, 23, dict(with_agent_channel=False, hidden_activation='tanh', kernel_sizes=(3, 3)), True),             # an activation alone
], ids=['zeros', 'reflect', 'replicate', 'fp16', 'fp16_zeros', 'no_agent_channel', 'activation_only_fp16'])
def test_stand_alone_boundaries_dtypes_channels(W, H, kw, f16):
    medium, agents = _world(W, H, f16)
    _check_agent(_agent(W + H, **kw), medium, agents, f16, step=True)


def test_narrow_default_takes_the_narrow_kernels_and_a_wide_width_3_agrees():
    """Routing: width 3 with no activation is the same function as the default stack; the two paths agree within the parity
    tolerance (they sum in different orders), and the default's result does not depend on the wide path at all."""
    W, H = 30, 50
    medium, agents = _world(W, H)
    narrow = _agent(4, kernel_sizes=(3, 3))
    wide = _agent(4, kernel_sizes=(3, 3), hidden_channels=3)
    assert not narrow.model.wide and wide.model.wide
    for p, q in zip(narrow.model.parameters(), wide.model.parameters()):
        assert torch.equal(p, q)
    env = die.Env.from_numpy(medium, agents)
    a = narrow.sense(env.medium).cpu().numpy().copy()
    b = wide.sense(env.medium).cpu().numpy()
    assert np.abs(a - b).max() <= ATOL


# ---------------------------------------------------------------------------------------------------- b. die_conv2d_wide by ctypes
SENTINEL = -7.0


def _conv_wide(W, H, x, w, k, act, pad, stride, tail=64, drop=None, out=None, in_arr=None, weights=True):
    cout, cin = w.shape[:2]
    if out is None:
        out = torch.full((cout * stride + tail,), SENTINEL, dtype=torch.float32, device=DEV)
    planes = (_lib.ConvPlane * cin)(*[_lib.ConvPlane(x[c].data_ptr(), _lib.DIE_PLANE_F32, 0) for c in range(cin)]) if in_arr is None else in_arr
    rc = _lib.lib.die_conv2d_wide(W, H, cin, planes, 1, cout, _ptr(out), stride, k, _ptr(w) if weights else None, act, pad,
                                  None if drop is None else C.byref(drop), None)
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize('W,H', [(30, 50), (17, 23)])
def test_conv2d_wide_against_the_model_and_writes_only_its_planes(W, H):
    rs = np.random.RandomState(W)
    acts, pads = [None, 'tanh', 'relu'], list(_lib.PAD_MODES)
    stride, i = W * H + 5, 0                                      # a plane stride larger than a plane
    for cin, cout in [(3, 5), (5, 3), (16, 16), (17, 32), (32, 17), (32, 3)]:
        for k in (1, 3, 5):
            act, pad = acts[i % 3], pads[i % 4]
            i += 1
            x = rs.rand(cin, W, H).astype(np.float32)
            w = M.xavier(rs, cout, cin, k)
            rc, out = _conv_wide(W, H, torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV), k, _lib.NCA_ACTIVATIONS[act],
                                 _lib.PAD_MODES[pad], stride)
            assert rc == 0, _lib.lib.die_last_error()
            host = out.cpu().numpy()
            got = host[:cout * stride].reshape(cout, stride)
            want = M.ACTIVATIONS[act](M.conv(x, w, pad))
            assert np.abs(got[:, :W * H].reshape(cout, W, H) - want).max() <= ATOL, (cin, cout, k, act, pad)
            assert (got[:, W * H:] == SENTINEL).all() and (host[cout * stride:] == SENTINEL).all(), (cin, cout, k)


def test_conv2d_wide_vector_stores_and_stride():
    """H % 4 == 0: the 16-byte stores, with a stride that keeps them aligned and one that does not (then 4-byte stores)."""
    W, H, cin, cout, k = 20, 72, 8, 20, 3
    rs = np.random.RandomState(2)
    x, w = rs.rand(cin, W, H).astype(np.float32), M.xavier(rs, cout, cin, k)
    want = np.tanh(M.conv(x, w, 'circular'))
    for stride in (W * H, W * H + 8, W * H + 3):
        rc, out = _conv_wide(W, H, torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV), k, 1, 0, stride)
        assert rc == 0, _lib.lib.die_last_error()
        host = out.cpu().numpy()
        got = host[:cout * stride].reshape(cout, stride)
        assert np.abs(got[:, :W * H].reshape(cout, W, H) - want).max() <= ATOL, stride
        assert (got[:, W * H:] == SENTINEL).all() and (host[cout * stride:] == SENTINEL).all(), stride


def test_conv2d_wide_refusals_launch_nothing():
    W, H = 17, 23
    x = torch.rand((33, W, H), device=DEV)
    w = torch.rand((33 * 33 * 49,), device=DEV)
    shaped = lambda cout, cin, k: w[:cout * cin * k * k].view(cout, cin, k, k)
    stride = W * H
    cases = {
        '33 channels in': dict(w=shaped(3, 33, 3), k=3),
        '33 channels out': dict(w=shaped(33, 3, 3), k=3),
        'k = 7': dict(w=shaped(3, 3, 7), k=7),
        'k = 2': dict(w=shaped(3, 3, 2), k=2),
        'null weights': dict(w=shaped(3, 3, 3), k=3, weights=False),
        'bad padding mode': dict(w=shaped(3, 3, 3), k=3, pad=4),
        'bad activation': dict(w=shaped(3, 3, 3), k=3, act=3),
        'stride below a plane': dict(w=shaped(3, 3, 3), k=3, stride=W * H - 1),
        'reflect wider than the field': dict(w=shaped(3, 3, 5), k=5, pad=2, W=2),
    }
    for name, kw in cases.items():
        kw = dict(dict(act=1, pad=0, stride=stride), **kw)
        rc, out = _conv_wide(kw.pop('W', W), H, x, **kw)
        assert rc == -1 and (out == SENTINEL).all(), (name, _lib.lib.die_last_error())
    # in-place: an input plane that begins inside the output planes (at their start, in the last one, at their last cell)
    buf = torch.full((16 * stride,), SENTINEL, dtype=torch.float32, device=DEV)
    for off in (0, 2 * stride, 3 * stride - 1):
        planes = (_lib.ConvPlane * 3)(*[_lib.ConvPlane(buf.data_ptr() + 4 * (off + c * 4 * stride), _lib.DIE_PLANE_F32, 0) for c in range(3)])
        rc, out = _conv_wide(W, H, None, shaped(3, 3, 3), 3, 1, 0, stride, out=buf, in_arr=planes)
        assert rc == -1 and b'in-place' in _lib.lib.die_last_error() and (buf == SENTINEL).all(), off
    # a null input plane, a plane of no kind, a null output
    for plane in (_lib.ConvPlane(None, 0, 0), _lib.ConvPlane(x.data_ptr(), 3, 0)):
        planes = (_lib.ConvPlane * 3)(_lib.ConvPlane(x.data_ptr(), 0, 0), plane, _lib.ConvPlane(x[2].data_ptr(), 0, 0))
        rc, out = _conv_wide(W, H, None, shaped(3, 3, 3), 3, 1, 0, stride, in_arr=planes)
        assert rc == -1 and (out == SENTINEL).all()
    planes = (_lib.ConvPlane * 3)(*[_lib.ConvPlane(x[c].data_ptr(), 0, 0) for c in range(3)])
    assert _lib.lib.die_conv2d_wide(W, H, 3, planes, 1, 3, None, stride, 3, _ptr(w), 1, 0, None, None) == -1
    assert _lib.lib.die_conv2d_wide(W, H, 3, None, 1, 3, _ptr(buf), stride, 3, _ptr(w), 1, 0, None, None) == -1
    bad_drop = _lib.nca_dropout(0.0, 1, 0, 0)
    rc, out = _conv_wide(W, H, x, shaped(3, 3, 3), 3, 1, 0, stride, drop=bad_drop)
    assert rc == -1 and (out == SENTINEL).all()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- c. dropout
@pytest.mark.parametrize('W,H,kw', [
    (96, 96, dict(kernel_sizes=(3, 3), hidden_channels=16, hidden_activation='tanh')),                       # one Philox block per thread
    (30, 50, dict(kernel_sizes=(3, 1, 3), hidden_channels=17, hidden_activation='relu', boundary='zeros')),  # cell by cell
])
def test_masked_planes_are_eval_planes_times_the_twin_mask(W, H, kw):
    p, S = 0.25, 2 ** 40 + 9
    medium, agents = _world(W, H)
    env = die.Env.from_numpy(medium, agents)
    ag = _agent(W + H, p_agent_dropout=p, dropout_seed=S, **kw)
    ag.model.eval()
    plain = ag.sense(env.medium).cpu().numpy().copy()
    assert ag.dropout_step == 1
    ag.model.train()
    for step in (1, 2, 2 ** 32 + 5):
        ag.dropout_step = step
        got = ag.sense(env.medium).cpu().numpy()
        assert ag.dropout_step == step + 1
        assert np.array_equal(got, (plain * D.mask(S, step, W, H, p)[None]).astype(np.float32)), step
        assert not np.array_equal(got, plain)
    one = _agent(W + H, p_agent_dropout=1.0, dropout_seed=S, **kw)                                            # p = 1: all zeros
    assert (one.sense(env.medium).cpu().numpy() == 0).all()


# ---------------------------------------------------------------------------------------------------- d. batched = stand-alone
def _population(R, seed, **kw):
    torch.manual_seed(seed)
    agents = []
    for _ in range(R):
        ag = die.NeuralAutomataAgent(scale=0.01, deposit=2.0, **kw)
        ag.model.init_weights()
        agents.append(ag)
    return agents


def _run_alone(env, agent, steps):
    obs, rew, alive, acts = env._get_current_obs, [], [], []
    for _ in range(steps):
        action = agent.forward(obs)
        acts.append(action.to_numpy())
        obs, rw, _, _, info = env.step(action)
        rew.append(rw)
        alive.append(info['num_agents'])
    return np.array(rew), np.array(alive), acts


CASES = ['plain', 'fp16_zeros', 'episodes_die_fixed', 'wave_flow', 'dynamics_rows', 'dropout_stride_0', 'dropout_stride_1', 'action']


@pytest.mark.parametrize('W,H', [(32, 32), (24, 40)])
@pytest.mark.parametrize('case', CASES)
def test_batched_replica_is_the_stand_alone_run(case, W, H):
    """8 steps of 4 replicas, widths 5 and 32 with a tanh hidden activation: medium, agents, rewards, alive counts and render(r)."""
    _batched_case(case, W, H)


def test_large_world_branch_is_the_stand_alone_run():
    """per_replica forced at the smallest size (as tests/test_gpu_dropout.py does): every replica a stand-alone Env and agent."""
    _batched_case('per_replica', 32, 32)


def _batched_case(case, W, H):
    R, T, E, dt, slots, per_replica, boundary = 4, 8, 1, torch.float32, 'alive', False, 'circular'
    model_kw, pop_kw = {}, {}
    dyns = [lambda: die.Dynamics(init_agent_ratio=0.15, **REFERENCE_DYNAMICS)] * R
    if case == 'fp16_zeros':
        dt, boundary = torch.float16, 'zeros'
    elif case == 'episodes_die_fixed':
        E, slots = 2, 300
        dyns = [lambda: die.Dynamics(agents_die=True, init_agent_ratio=0.15, **dict(REFERENCE_DYNAMICS, food_infinite=False))] * R
    elif case == 'wave_flow':
        flow = lambda: die.WaveSequence((W, H), dt=0.01).get_flow_operator(scale=0.5, decay=0.5)
        dyns = [lambda: die.Dynamics(init_agent_ratio=0.15, food_infinite=False, op_food_flow=flow())] * R
    elif case == 'dynamics_rows':                                 # two gaussian radii: 3 (sigma 0.8) and 2 (sigma 0.5)
        two = [dict(REFERENCE_DYNAMICS), dict(REFERENCE_DYNAMICS, diffuse_sigma=0.5, rate_decay_chem=0.05)]
        dyns = [lambda q=two[r % 2]: die.Dynamics(init_agent_ratio=0.15, **q) for r in range(R)]
    elif case.startswith('dropout'):
        model_kw = dict(p_agent_dropout=0.25)
        pop_kw = dict(dropout_seed=1000, dropout_seed_stride=int(case[-1]))
    elif case == 'per_replica':
        per_replica = True
    seeds = [11 + 5 * r for r in range(R)]
    for width in (5, 32):
        cands = _population(R // E, W + width, kernel_sizes=(3, 3), boundary=boundary, hidden_channels=width, hidden_activation='tanh',
                            **model_kw)
        shared = dyns[0]() if case != 'dynamics_rows' else [f() for f in dyns]
        benv = BatchedEnv((W, H), shared, replicas=R, seeds=seeds, field_dtype=dt, max_agents=slots, per_replica=per_replica)
        assert benv.per_replica == per_replica
        pop = BatchedNeuralAutomataAgent.from_agents(benv, cands, E, **pop_kw)
        assert pop._wide and pop.P == sum(k.weight.numel() for k in cands[0].model.conv_layers())
        if case == 'action':
            buf = torch.full((T, 3, R, benv.Nmax), SENTINEL, dtype=torch.float32, device=DEV)
            res = torch.stack([benv.step(pop, action=buf[t]).clone() for t in range(T)])
        else:
            res = benv.run(pop, T)
        rew, alive = BatchedEnv.read_results(res)
        for r in range(R):
            env = die.Env((W, H), dyns[r](), seed=seeds[r], max_agents=slots, field_dtype=dt)
            ag = pop.replica_agent(r)
            want_rew, want_alive, acts = _run_alone(env, ag, T)
            m, a = benv.replica_numpy(r)
            assert np.array_equal(m, env.medium.to_numpy()), (width, r)
            assert np.array_equal(a, env.agents.to_numpy()), (width, r)
            assert np.array_equal(rew[:, r], want_rew) and np.array_equal(alive[:, r], want_alive), (width, r)
            assert np.array_equal(pop.render(r), ag.render()[0]), (width, r)
            if case == 'action':
                host = buf[:, :, r].cpu().numpy()
                for t in range(T):
                    n = acts[t].shape[1]
                    assert np.array_equal(host[t, :, :n].astype(np.float64), acts[t]), (width, r, t)
                    assert (host[t, :, benv.n[r]:] == SENTINEL).all()
            if case.startswith('dropout'):
                assert ag.dropout_seed == 1000 + r * pop.dropout_seed_stride
                assert (pop.render(r)[..., 0] == 0).mean() > 0.1  # the planes that stay in scratch hold the masked values
        assert pop.candidate(0).model.hidden_channels == width and pop.candidate(0).model.hidden_activation == 'tanh'


def test_architectures_must_agree_in_width_and_activation():
    benv = BatchedEnv((32, 32), die.Dynamics(init_agent_ratio=0.15, **REFERENCE_DYNAMICS), replicas=2, seed=1)
    base = dict(kernel_sizes=(3, 3), hidden_channels=8, hidden_activation='tanh')
    for other in (dict(base, hidden_channels=9), dict(base, hidden_activation='relu'), dict(base, hidden_activation=None),
                  dict(kernel_sizes=(3, 3))):
        with pytest.raises(ValueError, match='architecture'):
            BatchedNeuralAutomataAgent.from_agents(benv, [_agent(1, **base), _agent(2, **other)])
    # width 3 without an activation has the default stack's weight shapes, and still is another architecture
    with pytest.raises(ValueError, match='architecture'):
        BatchedNeuralAutomataAgent.from_agents(benv, [_agent(1, kernel_sizes=(3, 3)), _agent(2, kernel_sizes=(3, 3), hidden_channels=3)])


# ---------------------------------------------------------------------------------------------------- e. the searchers
@pytest.mark.parametrize('kind', ['pgpe', 'cmaes'])
def test_searchers_run_on_the_wide_parameter_vector(kind):
    size, T = 32, 4
    R = 4 if kind == 'pgpe' else 5
    torch.manual_seed(0)
    template = die.NeuralAutomataAgent(kernel_sizes=[3, 3, 3], hidden_channels=16, hidden_activation='tanh', scale=0.01, deposit=2.0)
    dyn = lambda: die.Dynamics(init_agent_ratio=0.15, **REFERENCE_DYNAMICS)
    benv = BatchedEnv((size, size), dyn(), replicas=R, seeds=[9] * R)
    pop = BatchedNeuralAutomataAgent(benv, template)
    assert pop.P == 3168
    if kind == 'pgpe':
        s = PGPE(R, center_init=pop.parameters[0].cpu(), radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1,
                 optimizer_config=dict(max_speed=0.1, momentum=0.9), seed=11, device='cuda').for_population(pop, T)
    else:
        s = CMAES(R, center_init=pop.parameters[0].cpu(), stdev_init=0.1, seed=11, device='cuda').for_population(pop, T)
    s.step()                                                      # generation 0
    rows = pop.parameters.clone()
    fitness = s.fitness.cpu().tolist()
    fresh = BatchedEnv((size, size), dyn(), replicas=R, seeds=[9] * R)
    rewards, _ = BatchedEnv.read_results(fresh.run(BatchedNeuralAutomataAgent(fresh, template, rows), T))
    assert fitness == [sum(rewards[:, r].tolist()) for r in range(R)]
    s.step()                                                      # generation 1
    assert s.history().shape[0] == 2 and not torch.isnan(s.history()).any()
    assert not torch.equal(pop.parameters, rows)


# ---------------------------------------------------------------------------------------------------- f. no gradients
def test_differentiable_calls_are_refused_before_anything_moves():
    W, H, R = 32, 32, 2
    medium, agents = _world(W, H)
    env = die.Env.from_numpy(medium, agents)
    ag = _agent(1, kernel_sizes=(3, 3), hidden_channels=8, hidden_activation='tanh', p_agent_dropout=0.25, dropout_seed=3)
    before = env.medium.to_numpy()
    for call in (lambda: ag.differentiable_sense(env.medium), lambda: ag.differentiable_action(env._get_current_obs)):
        with pytest.raises(NotImplementedError, match='wide stack'):
            call()
    assert ag.dropout_step == 0 and np.array_equal(env.medium.to_numpy(), before)
    benv = BatchedEnv((W, H), die.Dynamics(init_agent_ratio=0.15, **REFERENCE_DYNAMICS), replicas=R, seed=2)
    pop = BatchedNeuralAutomataAgent(benv, ag, dropout_seed=5)
    torch.cuda.synchronize()
    state = benv._state.clone()
    for call in (pop.differentiable_sense, pop.differentiable_action):
        with pytest.raises(NotImplementedError, match='wide stack'):
            call()
    torch.cuda.synchronize()
    assert pop.dropout_step == 0 and pop._calls == 0 and benv.epoch == 1 and torch.equal(benv._state, state)
