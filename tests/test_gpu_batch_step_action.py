"""`BatchedEnv.step_action` (die_env_step_batch / die_env_step_batch_rows): R worlds stepped with the caller's actions must be, bit
for bit, R stand-alone `Env.step(action)` calls — occupancy, food, chem, x, y, alive, agent_food and both result words, every step,
across the claim plane's epoch wrap.  Also here: the replay of recorded actions (`step(agent, action=buf)` against `step_action(buf)`,
with seeded dropout), the large-world fan-out, `medium_tensor()`, and the library calls the existing paths make.

Shapes are the smallest at which the kernels can go wrong: 16 x 64 (one conv tile), 24 x 68 (one row and four columns past it; more
than one claim workgroup), 8 x 12 (below a tile, sigma 0.8 -> radius 3).  The actions are drawn here — every slot hops by up to two
cells per axis and deposits a positive amount — and before the batch is launched the host rule `deposit_cells` must find, in every
replica, a cell shared by several alive slots at some step: otherwise the losers' path was never run."""
import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent, BatchedPhysarumAgent
from die_amd.device_array import DeviceAction
from tests.field_step_adjoint_model import deposit_cells

pytestmark = pytest.mark.gpu

STEPS = 33                            # the 5-bit claim epoch wraps at 31


def _wave(W, H):
    return die.WaveSequence((W, H), dt=0.01).get_flow_operator(scale=0.5, decay=0.5)


def make_dynamics(case, W, H, R, op):
    """The batch's `dynamics` argument of a case: one Dynamics, or R of them (radii 2 and 3 both present, decay and rate_feed
    differing, the flow on some).  `op`: the flow operator object to name, or None."""
    kw = dict(init_agent_ratio=case.get('ratio', 0.15), agents_die=case.get('agents_die', False))
    if not case.get('listed'):
        flow = dict(op_food_flow=op) if op is not None else {}
        return die.Dynamics(diffuse_sigma=case.get('sigma', 0.8), food_infinite=case.get('food_infinite', False), **flow, **kw)
    out = []
    for r in range(R):
        flow = dict(op_food_flow=op) if op is not None and r % 3 != 1 else {}
        out.append(die.Dynamics(diffuse_sigma=(0.8, 0.5)[r % 2], rate_decay_chem=(0.025, 0.1, 0.06)[r % 3], rate_feed=(0.1, 0.25)[(r // 2) % 2],
                                food_infinite=bool(r % 2) if case.get('food_infinite') is None else case['food_infinite'], **flow, **kw))
    return out


def build(case, per_replica=False):
    """(batch, twins): the batch of a case and the stand-alone Env of every replica, built as BatchedEnv.__init__ builds its own."""
    W, H = case['shape']
    R = case['R']
    dt = torch.float16 if case.get('f16') else torch.float32
    slots = case.get('max_agents', 'alive')
    op = _wave(W, H) if case.get('flow') else None
    benv = BatchedEnv((W, H), make_dynamics(case, W, H, R, op), replicas=R, seed=case.get('seed', 3), field_dtype=dt, per_replica=per_replica,
                      max_agents=slots)
    assert per_replica is None or benv.per_replica == per_replica      # (None: the regime BatchedEnv picks by the world's size)
    twins = []
    for r in range(R):
        d = make_dynamics(case, W, H, R, _wave(W, H) if case.get('flow') else None)      # (a fresh operator at the same counter)
        d = d[r] if case.get('listed') else d
        twins.append(die.Env((W, H), d, seed=benv.seeds[r], max_agents=slots, field_dtype=dt, device=benv.device, sort_every=0, pic=False,
                             sync=False))
    assert [e.agents.N for e in twins] == benv.n
    return benv, twins


def draw_actions(case, benv, steps=STEPS):
    """(steps, 3, R, Nmax) float32: every slot hops by -2..2 cells per axis (dx = k / (W - 1) lands on a cell's own label again) and
    deposits a positive amount; the padding of the 'alive' layout is filled with NaN — it must never be read."""
    W, H = case['shape']
    rs = np.random.RandomState(case.get('seed', 3) * 101 + W * 7 + H)
    act = np.full((steps, 3, benv.R, benv.Nmax), np.nan, dtype=np.float32)
    top = 12.0 if case.get('agents_die') else 2.0         # (deposit 12 costs 0.24 a step: more than the poorer cells feed)
    for r, k in enumerate(benv.n):
        act[:, 0, r, :k] = (rs.randint(-2, 3, (steps, k)) / (W - 1)).astype(np.float32)
        act[:, 1, r, :k] = (rs.randint(-2, 3, (steps, k)) / (H - 1)).astype(np.float32)
        act[:, 2, r, :k] = rs.uniform(0.5, top, (steps, k)).astype(np.float32)
    return act


def _moved(X, d, limit):
    """_agent_move on Q0.32 coordinates, exactly: the increment is the fp32 product rounded to nearest even."""
    q = np.rint((d.astype(np.float32) * np.float32(4294967296.0)).astype(np.float64)).astype(np.int64)
    P = X.astype(np.int64) + q
    return (np.clip(P, 0, 0xFFFFFFFF) if limit else P & 0xFFFFFFFF).astype(np.uint64)


def _cell(X, n):
    return ((X.astype(np.uint64) * np.uint64(n - 1) + np.uint64(0x80000000)) >> np.uint64(32)).astype(np.int64)


def host_winners(env, action, W, H):
    """deposit_cells of the step `action` is about to drive on the stand-alone `env` (read before that step): the slots' cells after
    the move, the alive flags of the claim pass."""
    limit = env.dynamics.boundary == die.BoundaryCondition.limit
    x = env.agents.x.cpu().numpy().view(np.uint32)
    y = env.agents.y.cpu().numpy().view(np.uint32)
    alive = env.agents.alive.cpu().numpy()
    cx, cy = _cell(_moved(x, action[0], limit), W), _cell(_moved(y, action[1], limit), H)
    return deposit_cells(cx, cy, alive, None, H), cx * H + cy, alive > 0


def run_twins(case, benv, twins, actions, winners=None):
    """The stand-alone runs: per replica the result words of every step, the state after every step (device tensors), and whether
    the drawn actions made alive slots share a cell and lose it.  `winners`: host_winners, or a faster twin of it (millions of
    slots: tests/test_gpu_batch_midsize.py)."""
    W, H = case['shape']
    want, shared = [], []
    for r, env in enumerate(twins):
        k, seen, rows = benv.n[r], False, []
        for t in range(actions.shape[0]):
            a = actions[t, :, r, :k]
            cells, where, alive = (winners or host_winners)(env, a, W, H)
            losers = alive & (cells < 0)
            seen |= bool(losers.any()) and len(set(where[alive])) < int(alive.sum())
            act = DeviceAction(k, env.device)
            act.data = torch.from_numpy(np.ascontiguousarray(a)).to(env.device)
            _, res, *_ = env.step(act)
            M, A = env.medium, env.agents
            occ = ((M.owner >> (32 + _lib.OWNER_EPOCH_SHIFT)) & _lib.OWNER_EPOCH_MAX) == M.epoch
            rows.append((res.clone(), occ, M.food.clone(), M.chem.clone(), A.x.clone(), A.y.clone(), A.alive.clone(), A.agent_food.clone()))
        want.append(rows)
        shared.append(seen)
    return want, shared


def batch_state(benv, r):
    k = benv.n[r]
    occ = ((benv.owner[r] >> (32 + _lib.OWNER_EPOCH_SHIFT)) & _lib.OWNER_EPOCH_MAX) == benv.epoch
    return occ, benv.food[r], benv.chem[r], benv.x[r, :k], benv.y[r, :k], benv.alive[r, :k], benv.agent_food[r, :k]


NAMES = ('occupancy', 'food', 'chem', 'x', 'y', 'alive', 'agent_food')

CASES = {
    'f32_alive': dict(shape=(24, 68), R=3, food_infinite=True),
    'f32_alive_finite_one_tile': dict(shape=(16, 64), R=3, sigma=0.5),
    'f16_fixed_layout': dict(shape=(24, 68), R=3, f16=True, max_agents=400),
    'f32_agents_die': dict(shape=(24, 68), R=3, agents_die=True),
    'f16_agents_die_fixed_infinite': dict(shape=(16, 64), R=2, f16=True, agents_die=True, max_agents=256, food_infinite=True),
    'f32_wave_flow': dict(shape=(24, 68), R=2, flow=True),
    'f32_rows': dict(shape=(24, 68), R=4, listed=True, food_infinite=None),
    'f16_rows_flow_die_fixed': dict(shape=(24, 68), R=3, listed=True, f16=True, flow=True, agents_die=True, max_agents=None, food_infinite=False),
    'f32_below_a_tile_one_replica': dict(shape=(8, 12), R=1, ratio=0.3),
    'f32_64_replicas': dict(shape=(8, 12), R=64, ratio=0.3),
}


@pytest.mark.parametrize('name', list(CASES))
def test_step_action_equals_stand_alone_steps(name):
    case = CASES[name]
    benv, twins = build(case)
    if benv.R > 1 and case.get('max_agents', 'alive') == 'alive':
        assert len(set(benv.n)) > 1                               # padding exists: replicas of different sizes share the launches
    actions = draw_actions(case, benv)
    want, shared = run_twins(case, benv, twins, actions)
    assert all(shared), f'replicas without a shared cell and a loser: {[r for r, s in enumerate(shared) if not s]}'
    dev_actions = torch.from_numpy(actions).to(benv.device)
    for t in range(STEPS):
        res = benv.step_action(dev_actions[t])
        assert benv.epoch == (t + 1) % _lib.OWNER_EPOCH_MAX + 1         # 2 … 31, then 1 again: the wrap is crossed
        for r in range(benv.R):
            w = want[r][t]
            assert torch.equal(res[r].view(torch.int64), w[0].view(torch.int64)), (t, r, 'result words')
            for what, got, exp in zip(NAMES, batch_state(benv, r), w[1:]):
                assert torch.equal(got, exp), (t, r, what)
    assert benv._steps == STEPS and benv.chem_node is None
    if case.get('agents_die'):
        _, alive = BatchedEnv.read_results(res)
        assert (alive < np.array(benv.n)).any()                    # slots starved: the lifecycle pass was part of it
    for r, env in enumerate(twins):                                # … and what the public accessors say
        m, a = benv.replica_numpy(r)
        assert np.array_equal(m, env.medium.to_numpy()) and np.array_equal(a, env.agents.to_numpy()), r


# ---------------------------------------------------------------- replay
def _template(p=0.0):
    torch.manual_seed(5)
    return die.NeuralAutomataAgent(scale=0.05, deposit=2.0, kernel_sizes=(3,), boundary='circular', p_agent_dropout=p)


def _driver(kind, benv):
    if kind == 'physarum':
        return BatchedPhysarumAgent(benv, seed=7, scale=0.05, sense_offset=0.1)
    return BatchedNeuralAutomataAgent(benv, _template(0.25), dropout_seed=11)


@pytest.mark.parametrize('kind', ['physarum', 'nca_dropout'])
def test_recorded_actions_replay(kind):
    """A batch driven by an agent records its actions; a second batch driven by `step_action` of the record stays bit-equal —
    the whole state allocation, claim words included.  (With dropout this is what a replay through `step(agent, action=...)`
    after a `differentiable_action` would get wrong: that call advances `dropout_step` itself.)"""
    make = lambda: BatchedEnv((24, 68), die.Dynamics(diffuse_sigma=0.8, init_agent_ratio=0.15), replicas=3, seed=3)
    one, two = make(), make()
    agent = _driver(kind, one)
    buf = torch.zeros((3, one.R, one.Nmax), dtype=torch.float32, device=one.device)
    moved = False
    for t in range(8):
        first = one.step(agent, action=buf)
        moved |= bool((buf[:2] != 0).any())
        second = two.step_action(buf)
        assert torch.equal(first.view(torch.int64), second.view(torch.int64)), t
        assert one.epoch == two.epoch and torch.equal(one._state, two._state), t
        assert one.chem.data_ptr() - one._state.data_ptr() == two.chem.data_ptr() - two._state.data_ptr()
    assert moved
    if kind == 'nca_dropout':
        assert agent.dropout_step == 8


# ---------------------------------------------------------------- large worlds, the observation, the calls
def test_per_replica_fan_out_equals_the_small_world_batch():
    case = dict(shape=(24, 68), R=3, agents_die=True)
    small, _ = build(case)
    large, _ = build(case, per_replica=True)
    actions = torch.from_numpy(draw_actions(case, small, 12)).to(small.device)
    for t in range(12):
        a, b = small.step_action(actions[t]), large.step_action(actions[t])
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), t
        for r in range(small.R):
            for x, y in zip(small.replica_numpy(r), large.replica_numpy(r)):
                assert np.array_equal(x, y), (t, r)
    assert large._steps == 12 and all(e._steps == 12 for e in large.envs)


@pytest.mark.parametrize('f16', [False, True])
def test_medium_tensor_is_replica_numpy(f16):
    case = dict(shape=(24, 68), R=3, f16=f16)
    benv, _ = build(case)
    actions = torch.from_numpy(draw_actions(case, benv, 3)).to(benv.device)
    for t in range(3):
        obs = benv.medium_tensor()
        assert obs.shape == (3, 3, 24, 68) and obs.dtype == torch.float32 and obs.device == benv.device
        for r in range(benv.R):
            assert np.array_equal(obs[r].to(torch.float64).cpu().numpy(), benv.replica_numpy(r)[0]), (t, r)
        assert obs[:, 0].sum() > 0
        benv.step_action(actions[t])


RECORDED = ('die_forward_env_step_batch', 'die_forward_env_step_batch_rows', 'die_nca_env_step_batch', 'die_nca_env_step_batch_rows',
            'die_nca_env_step_batch_dropout', 'die_env_step_batch', 'die_env_step_batch_rows', 'die_food_flow_batch',
            'die_food_flow_batch_masked', 'die_deposit_cells_batch', 'die_env_step_backward_batch', 'die_nca_backward_batch',
            'die_nca_backward_batch_inputs')


@pytest.fixture
def calls(monkeypatch):
    log = []
    for name in RECORDED:
        def recorder(*args, _fn=getattr(_lib.lib, name), _name=name):
            log.append(_name)
            return _fn(*args)
        monkeypatch.setattr(_lib.lib, name, recorder)
    return log


@pytest.mark.parametrize('listed, flow', [(False, False), (False, True), (True, True)])
def test_the_calls_the_steps_make(calls, listed, flow):
    case = dict(shape=(24, 68), R=3, listed=listed, flow=flow, food_infinite=False)
    benv, _ = build(case)
    flows = ['die_food_flow_batch_masked' if listed else 'die_food_flow_batch'] if flow else []
    rows = '_rows' if listed else ''
    agent = BatchedPhysarumAgent(benv, seed=7)
    del calls[:]
    benv.step(agent)                                               # the existing path: what it called before this entry point existed
    assert calls == ['die_forward_env_step_batch' + rows] + flows
    pop = BatchedNeuralAutomataAgent(benv, _template())
    del calls[:]
    benv.step(pop)
    assert calls == ['die_nca_env_step_batch' + rows] + flows
    action = torch.from_numpy(draw_actions(case, benv, 1)[0]).to(benv.device)
    del calls[:]
    benv.step_action(action)
    assert calls == ['die_env_step_batch' + rows] + flows
    torch.cuda.synchronize()


def _snapshot(benv):
    torch.cuda.synchronize()
    return (benv.epoch, benv._steps), benv._state.clone()


def test_a_refused_step_action_changes_nothing(calls):
    """A wrong action is refused in Python (ValueError naming the shape); H % 4 != 0 is accepted by the constructor and refused by
    the library before any launch (UNSUPPORTED): either way epoch, counters and every byte of the state stay."""
    benv = BatchedEnv((32, 30), die.Dynamics(diffuse_sigma=0.8, init_agent_ratio=0.15), replicas=3, seed=3, per_replica=False)
    good = torch.zeros((3, benv.R, benv.Nmax), dtype=torch.float32, device=benv.device)
    before = _snapshot(benv)
    shape = rf'\(3, {benv.R}, {benv.Nmax}\)'
    for bad in (good[:, :2], good.double(), good.cpu(), good.transpose(1, 2).contiguous().transpose(1, 2), good.permute(1, 0, 2), None,
                good.cpu().numpy()):
        with pytest.raises(ValueError, match=shape):
            benv.step_action(bad)
    assert calls == []
    with pytest.raises(NotImplementedError, match='H % 4 == 0'):
        benv.step_action(good)
    assert calls == ['die_env_step_batch']                          # the library was asked, and refused
    after = _snapshot(benv)
    assert after[0] == before[0] == (1, 0) and torch.equal(after[1], before[1])
    ok = BatchedEnv((24, 68), die.Dynamics(diffuse_sigma=0.8, init_agent_ratio=0.15), replicas=2, seed=3)
    graph = torch.zeros((3, ok.R, ok.Nmax), dtype=torch.float32, device=ok.device, requires_grad=True) * 1.0
    ok.step_action(graph)                                           # a tensor with a graph is read detached
    assert ok._steps == 1 and ok.epoch == 2
