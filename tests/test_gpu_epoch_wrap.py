"""The stateful agent paths across the wrap of the claim epoch (the 5-bit tag 1 .. 31 of the claim plane, the stock / standing planes
and the records of the gradient paths): a word left from a build one cycle ago reads as "occupied" again exactly 31 steps later,
unless the library (`nca_env_step_batch` at sense epoch 31), the BatchedEnv (`_stock_planes`) or the stand-alone agent
(`_stock_plane`) has started the plane over.  Every world here gets to the wrap by real steps from a fresh world — an assigned
epoch leaves no stale words — and every test asserts that a stale word would have mattered: cells occupied under a tag in the first
cycle that stand empty under the same tag in the second (schedules and orders: tests/epoch_wrap_cases.py).

  1. populations are their stand-alone runs over 40 steps, bit for bit (device against device);
  2. link by link against the numpy models at sense epochs 30, 31, 1, 2 (the independent check);
  3. signal, memory, stock and plain populations and `step_action` taking turns on one batch, every pair at 31, 1;
  4. the stand-alone agent's plane rule under irregular forwards, against a twin with a blank plane;
  5. gradient windows of five links at sense epochs 29, 30, 31, 1, 2 against the float64 loops, and the bit-for-bit
     "is `forward`" comparisons over 34 steps;
  6. a backward taken after the tags of its forward have come round again, once and twice.

Tolerances are the existing files': CEILING of max|grad_f64| per array, FORWARD for the trajectory, tests/signal_model.py `bound`."""
import numpy as np
import pytest
import torch

import die_amd as die
from die_amd import _lib
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent
from die_amd.device_array import DeviceAction
from tests import epoch_wrap_cases as EW
from tests import field_step_adjoint_model as F
from tests import memory_grad_model as MG
from tests import memory_model as MM
from tests import nca_grad_model as G
from tests import signal_model as SM
from tests import stock_plane_model as S
from tests import test_gpu_heredity as HT
from tests import test_gpu_memory as MT
from tests import test_gpu_memory_grad as MGT
from tests import test_gpu_memory_grad_batch as MGB
from tests import test_gpu_signal as ST
from tests import test_gpu_signal_grad as SGT
from tests import test_gpu_signal_grad_batch as SGB
from tests import test_gpu_stock as KT
from tests.test_gpu_signal_grad_batch import CEILING, FORWARD

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SCALE = 0.05                         # of the forward-only agents: up to one cell of 24 a step, so that nobody stands still for a cycle
WIDE = MT.WIDE
REFERENCE = MT.REFERENCE_DYNAMICS
WINDOW_EPOCHS = (29, 30, 31, 1, 2)


def _bits(t):
    return MM.bits(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)


def _tags(owner):
    """The epoch tag of every word of a claim plane, whatever the current epoch."""
    return ((owner >> (32 + _lib.OWNER_EPOCH_SHIFT)) & _lib.OWNER_EPOCH_MAX).cpu().numpy()


# ---------------------------------------------------------------------------------------------------- who stood where, step by step
def _occupancy_alone(env):
    return SM.occupancy_of(env.medium.W, env.medium.H, env.agents.to_numpy())


def _occupancy_batch(benv):
    return np.stack([SM.occupancy_of(benv.W, benv.H, benv.replica_numpy(r)[1]) for r in range(benv.R)])


class _Watch:
    """Notes who stands where before every step of a world, through the world's own step methods (an Env's `step`, which
    `differentiable_step` goes through; a BatchedEnv's `step` and `step_action`): `occ[i]` is what step i sensed, and `seen()` adds
    the cells of now — what a forward after the last step senses."""

    def __init__(self, world):
        batched = isinstance(world, BatchedEnv)
        self.world, self.occ = world, []
        self._occupancy = _occupancy_batch if batched else _occupancy_alone
        for name in ('step', 'step_action') if batched else ('step',):
            setattr(world, name, self._watched(getattr(world, name)))

    def _watched(self, call):
        def step(*args, **kw):
            self.occ.append(self._occupancy(self.world))
            return call(*args, **kw)
        return step

    def seen(self):
        return self.occ + [self._occupancy(self.world)]


def _assert_a_stale_word_would_matter(occ):
    """`occ[i]`: the cells occupied when step i sensed.  Under each of the tags 1 and 2 somebody stood in the first cycle on a cell
    that is empty when the second cycle reads at the same tag — a word kept from then would read as an agent there."""
    for e, (first, second) in EW.SECOND_CYCLE.items():
        assert len(occ) > second, (len(occ), second)
        assert (np.asarray(occ[first]) & ~np.asarray(occ[second])).any(), e


def _warm_up(watches):
    """A helper's `before`: EW.WARM_UP real forward + step cycles of the stand-alone agent on its fresh world, no graph, then a
    blank field and blank memory — the window's first link senses at epoch 29.  The world's watch is appended to `watches`."""
    def before(env, ag):
        assert env.medium.epoch == 1
        watches.append(_Watch(env))
        with torch.no_grad():
            obs = env._get_current_obs
            for _ in range(EW.WARM_UP):
                obs, *_ = env.step(ag.forward(obs))
        assert env.medium.epoch == EW.sense_epoch(EW.WARM_UP) == WINDOW_EPOCHS[0]
        if ag.signal_channels:
            ag.reset_signals()
        if ag.memory_channels:
            ag.reset_memory()
    return before


def _warm_up_batch(watches):
    """The same for a population on its batch."""
    def before(benv, pop):
        assert benv.epoch == 1
        watches.append(_Watch(benv))
        with torch.no_grad():
            for _ in range(EW.WARM_UP):
                benv.step(pop)
        assert benv.epoch == EW.sense_epoch(EW.WARM_UP) == WINDOW_EPOCHS[0]
        if callable(getattr(pop, 'reset', None)):
            pop.reset()
    return before


def _window_crossed(watch, epoch_of):
    """After a window of EW.WINDOW links behind the warm-up: the world stands at sense epoch 2 of the second cycle, and a stale
    word would have mattered on the way."""
    assert epoch_of(watch.world) == WINDOW_EPOCHS[-1]
    occ = watch.seen()
    assert len(occ) == EW.WARM_UP + EW.WINDOW
    _assert_a_stale_word_would_matter(occ)


def _hops(rs, W, H, n):
    """(3, n) float32: every slot hops by one or two cells per axis, either way, and deposits a positive amount."""
    hop = lambda size, cells: (rs.choice([-2, -1, 1, 2], size) / (cells - 1))     # noqa: E731
    return np.stack([hop(n, W), hop(n, H), rs.uniform(0.5, 2.0, n)]).astype(np.float32)


def _drive(env, steps, rs):
    """`steps` steps of a stand-alone world under random non-zero actions that carry no agent."""
    for _ in range(steps):
        act = DeviceAction(env.agents.N, env.device, env.agents.slot)
        act.data = torch.from_numpy(_hops(rs, env.medium.W, env.medium.H, env.agents.N)).to(env.device)
        env.step(act)


def _drive_batch(benv, steps, rs):
    for _ in range(steps):
        act = np.zeros((3, benv.R, benv.Nmax), dtype=np.float32)
        for r, n in enumerate(benv.n):
            act[:, r, :n] = _hops(rs, benv.W, benv.H, n)
        benv.step_action(torch.from_numpy(act).to(benv.device))


def test_the_tables_speak_of_this_library():
    assert EW.EPOCH_MAX == _lib.OWNER_EPOCH_MAX
    assert tuple(EW.sense_epoch(EW.WARM_UP + t) for t in range(EW.WINDOW)) == WINDOW_EPOCHS


# ---------------------------------------------------------------------------------------------------- 1. populations over 40 steps
DYN = dict(REFERENCE, init_agent_ratio=0.15)
POPULATIONS = {
    # K, M, model, slots, Dynamics per replica (built anew for every Env), population arguments
    'signal': (2, 0, WIDE, 'alive', [DYN], {}),
    'signal_memory': (2, 2, WIDE, 'alive', [DYN], {}),
    'signal_stock_no_agents_die': (2, 0, dict(WIDE, with_stock_channel=True, with_agent_channel=False), 'alive', [dict(DYN, agents_die=True)], {}),
    'signal_die_born': (2, 0, WIDE, 600, [dict(DYN, agents_die=True, agents_born=True)], {}),      # (600 slots: the colonies still grow at step 40)
    'memory_no_stock': (0, 2, WIDE, 'alive', [DYN], {}),
    'narrow_stock': (0, 0, dict(kernel_sizes=(3, 3)), 'alive', [DYN], {}),
    'signal_dropout': (2, 0, dict(WIDE, p_agent_dropout=0.25), 'alive', [DYN], dict(dropout_seed=1000, dropout_seed_stride=3)),
    'signal_dynamics_rows': (2, 0, WIDE, 'alive', [DYN, dict(DYN, diffuse_sigma=0.5, rate_decay_chem=0.05)], {}),
}


def _population_candidates(n, seed, K, M, model_kw):
    if K:
        return ST._candidates(n, seed, K, M, scale=SCALE, **model_kw), ST._assert_replica_is
    if M:
        return MT._candidates(n, seed, M, scale=SCALE, **model_kw), MT._assert_replica_is
    return KT._candidates(n, seed, scale=SCALE, **model_kw), KT._assert_replica_is


@pytest.mark.parametrize('case', list(POPULATIONS))
def test_replica_is_the_stand_alone_agent_over_40_steps(case):
    W, H, R, steps = 24, 40, 4, EW.POPULATION_STEPS
    K, M, model_kw, slots, dyn_kws, pop_kw = POPULATIONS[case]
    dyn = lambda r: die.Dynamics(**dyn_kws[r % len(dyn_kws)])                     # noqa: E731
    cands, assert_replica_is = _population_candidates(R, W + R, K, M, model_kw)
    benv = BatchedEnv((W, H), dyn(0) if len(dyn_kws) == 1 else [dyn(r) for r in range(R)], replicas=R, seed=11, max_agents=slots)
    pop = BatchedNeuralAutomataAgent.from_agents(benv, cands, **pop_kw)
    assert pop._signal_channels == K and pop._memory_channels == M and not benv.per_replica
    assert pop._builds_stock_planes                                               # every case builds the batch's planes, step after step
    rew, alive = BatchedEnv.read_results(benv.run(pop, steps))
    assert benv.epoch == EW.sense_epoch(steps) == 10 and benv._stock is not None
    for r in range(R):
        env = die.Env((W, H), dyn(r), seed=11 + r, max_agents=slots)
        watch = _Watch(env)
        ag = pop.replica_agent(r)
        want_rew, want_alive = MT._run_alone(env, ag, steps)
        assert_replica_is(benv, pop, r, env, ag, rew, alive, want_rew, want_alive)
        _assert_a_stale_word_would_matter(watch.occ)
    if case == 'signal_die_born':                                                 # children are born on both sides of the wrap
        print(f'signal_die_born: alive per step, replica 0: {alive[:, 0].tolist()}')
        assert (alive[EW.AT_30] > alive[0]).all() and (alive[-1] > alive[EW.AT_1 + 1]).all()
    if case == 'signal_stock_no_agents_die':
        assert pop._stock_channel and not pop._arch['with_agent_channel']


def test_large_world_branch_over_40_steps():
    """One smoke case of the per_replica regime: every replica a stand-alone Env and agent of its own, against the small-world
    batch that the cases above hold to the stand-alone runs."""
    W, H, R, steps = 24, 40, 2, EW.POPULATION_STEPS
    dyn = lambda: die.Dynamics(**DYN)                                             # noqa: E731
    cands = ST._candidates(R, 9, 2, 2, scale=SCALE, **WIDE)
    big, small = (BatchedEnv((W, H), dyn(), replicas=R, seed=4, per_replica=p) for p in (True, False))
    pb, ps = BatchedNeuralAutomataAgent.from_agents(big, cands), BatchedNeuralAutomataAgent.from_agents(small, cands)
    assert torch.equal(big.run(pb, steps), small.run(ps, steps)) and pb.signals is None
    for r in range(R):
        assert np.array_equal(_bits(pb.agents[r].signals), _bits(ps.signals[r])) and pb.agents[r].signals.any(), r
        assert np.array_equal(_bits(pb.agents[r].memory), _bits(ps.memory[r, :, :small.n[r]])), r
        for u, v in zip(big.replica_numpy(r), small.replica_numpy(r)):
            assert np.array_equal(u, v), r


# ---------------------------------------------------------------------------------------------------- 2. link by link at 30, 31, 1, 2
def _stateful_agent(seed, K, M, **kw):
    torch.manual_seed(seed)
    signal = dict(signal_channels=K, signal_deposit=0.75, signal_sigma=0.8, signal_decay=0.05) if K else {}
    ag = die.NeuralAutomataAgent(scale=SCALE, deposit=2.0, memory_channels=M, **signal, **dict(WIDE, **kw))
    ag.model.init_weights()
    return ag


@pytest.mark.parametrize('K,M', [(2, 0), (0, 2), (2, 2)], ids=['signals', 'memory', 'signals and memory'])
def test_links_against_the_models_at_sense_epochs_30_31_1_2(K, M):
    W, H = 24, 40
    env = die.Env((W, H), die.Dynamics(**dict(DYN, agents_die=True)), seed=8, max_agents='alive', sort_every=0)
    ag = _stateful_agent(9, K, M)
    N = env.agents.N
    obs, occs = env._get_current_obs, {}
    for i in range(EW.LINKS_AT[-1] + 1):
        a = env.agents.to_numpy()
        occ = occs[i] = SM.occupancy_of(W, H, a)
        if i in EW.LINKS_AT:
            epoch = env.medium.epoch
            assert epoch == EW.sense_epoch(i) and 0 < occ.sum() <= (a[2] > 0).sum()
            field = ag.signals.cpu().numpy().copy() if K else None
            held = ag.memory.cpu().numpy().copy() if M else None
        action = ag.forward(obs)
        if i in EW.LINKS_AT:
            sensed = action._keepalive.cpu().numpy()
            # the standing plane this forward built, read at its epoch: the model's occupancy and nothing else
            words = ag._standing.cpu().numpy()
            assert np.array_equal(S.decode(words, epoch)[0], occ), i
            assert len(np.unique(S.decode(words, epoch)[3])) > 2 or epoch <= 2, i    # (words of earlier builds are still there, and lose)
            if K:
                deposit, sigma, decay = ag.signal_constants
                err = np.abs(ag.signals.cpu().numpy().astype(np.float64) - SM.update(field, occ, sensed[3:3 + K], deposit, sigma, decay))
                bound = SM.bound(field, occ, sensed[3:3 + K], deposit, sigma, decay)
                print(f'K={K} M={M} step {i} (sense epoch {epoch}): worst share of the bound {(err / bound).max():.4f}')
                assert (err <= bound).all(), (i, (err / bound).max())
                assert (np.abs(SM.update(field, occ, sensed[3:3 + K], deposit, sigma, decay) -
                               SM.update(field, np.zeros_like(occ), sensed[3:3 + K], deposit, sigma, decay)) > 10 * bound).any(), i
            if M:
                planes, = ag._memory_planes.values()                              # the expand this forward sensed
                assert np.array_equal(_bits(planes), MM.bits(MM.expand_of(W, H, a, held))) and _bits(planes).any(), i
                assert np.array_equal(_bits(ag.memory), MM.bits(MM.gather_of(W, H, a, sensed[3 + K:]))), i
        obs, *_ = env.step(action)
    assert env.agents.N == N
    _assert_a_stale_word_would_matter(occs)


# ---------------------------------------------------------------------------------------------------- 3. taking turns at the wrap
def _plain(n, seed, **kw):
    torch.manual_seed(seed)
    out = [die.NeuralAutomataAgent(scale=SCALE, deposit=2.0, **kw) for _ in range(n)]
    for p in out:
        p.model.init_weights()
    return out


@pytest.mark.parametrize('order', EW.ORDERS)
def test_five_kinds_take_turns_across_the_wrap(order):
    """S, M, K: a signal, a memory and a narrow stock population (the builders of the batch's stock / standing planes); P: a plain
    population; A: `step_action` with the actions the replicas' stand-alone plain agents compute.  Replica r is, bit for bit, the
    stand-alone world stepped by its five stand-alone agents in the same order."""
    W, H, R = 24, 40, 3
    dyn = lambda: die.Dynamics(**DYN)                                             # noqa: E731
    groups = {'S': ST._candidates(R, 12, scale=SCALE, **WIDE), 'M': MT._candidates(R, 14, scale=SCALE, **WIDE),
              'K': KT._candidates(R, 15, scale=SCALE, kernel_sizes=(3, 3)), 'P': _plain(R, 13, **WIDE)}
    drivers = _plain(R, 16, kernel_sizes=(3, 3))
    benv = BatchedEnv((W, H), dyn(), replicas=R, seed=21)
    pops = {c: BatchedNeuralAutomataAgent.from_agents(benv, g) for c, g in groups.items()}
    assert [bool(pops[c]._builds_stock_planes) for c in 'SMKP'] == [True, True, True, False] and set(EW.BUILDERS) == set('SMK')
    envs = [die.Env((W, H), dyn(), seed=21 + r, max_agents='alive') for r in range(R)]
    mine = [dict({c: pops[c].replica_agent(r) for c in pops}, A=drivers[r]) for r in range(R)]
    obs = [env._get_current_obs for env in envs]
    buf = torch.zeros((3, R, benv.Nmax), dtype=torch.float32, device=benv.device)
    out, want_rew, want_alive, occ = [], [[] for _ in envs], [[] for _ in envs], [{} for _ in envs]
    noted = {i for pair in EW.SECOND_CYCLE.values() for i in pair}
    for i, c in enumerate(order):
        assert benv.epoch == EW.sense_epoch(i)
        acts = [mine[r][c].forward(obs[r]) for r in range(R)]
        if c == 'A':
            for r, act in enumerate(acts):
                buf[:, r, :benv.n[r]] = torch.stack([act.sel(ch)[:benv.n[r]] for ch in act.channels])
            out.append(benv.step_action(buf).clone())
        else:
            out.append(benv.step(pops[c]).clone())
        for r, env in enumerate(envs):
            if i in noted:
                occ[r][i] = _occupancy_alone(env)
            obs[r], rw, _, _, info = env.step(acts[r])
            want_rew[r].append(rw)
            want_alive[r].append(info['num_agents'])
    rew, alive = BatchedEnv.read_results(torch.stack(out))
    assert len(set(benv.n)) > 1                                                   # padding slots: step_action's buffer holds zeros there
    for r, env in enumerate(envs):
        ST._assert_replica_is(benv, pops['S'], r, env, mine[r]['S'], rew, alive, np.array(want_rew[r]), np.array(want_alive[r]))
        n = benv.n[r]
        assert np.array_equal(_bits(pops['M'].memory[r, :, :n]), _bits(mine[r]['M'].memory)) and _bits(mine[r]['M'].memory).any(), r
        assert np.array_equal(pops['K'].render(r), mine[r]['K'].render()[0]) and np.array_equal(pops['M'].render(r), mine[r]['M'].render()[0]), r
        full = [occ[r].get(i) for i in range(max(noted) + 1)]
        _assert_a_stale_word_would_matter(full)


# ---------------------------------------------------------------------------------------------------- 4. the stand-alone agent's plane rule
SENSING = {
    'signals': dict(signal_channels=2, signal_deposit=0.75, signal_sigma=0.8, signal_decay=0.05),
    'memory': dict(memory_channels=2),
    'stock': dict(with_stock_channel=True),
}


@pytest.mark.parametrize('kind', list(SENSING))
def test_the_agents_plane_rule_under_irregular_forwards(kind):
    """The agent senses at EW.SENSE_AT only (gaps 0, 1, 30, 31, 32, 62) while random actions drive the world; at every sense a
    twin made at that moment — the same weights, field and memory, a plane it has never built on — returns the same bits."""
    W, H = 24, 40
    env = die.Env((W, H), die.Dynamics(**DYN), seed=5, max_agents='alive', sort_every=0)
    make = lambda: die.NeuralAutomataAgent(scale=SCALE, deposit=2.0, **WIDE, **SENSING[kind])      # noqa: E731
    torch.manual_seed(3)
    ag = make()
    ag.model.init_weights()
    N, rs, step, occ, last = env.agents.N, np.random.RandomState(6), 0, {}, None
    for at in EW.SENSE_AT:
        _drive(env, at - step, rs)
        step = at
        epoch = env.medium.epoch
        assert epoch == EW.sense_epoch(at)
        occ[at] = _occupancy_alone(env)
        twin = make()
        twin.model.load_state_dict(ag.model.state_dict())
        twin.signals = None if ag.signals is None else ag.signals.clone()
        twin.memory = None if ag.memory is None else ag.memory.clone()
        assert not twin._stock
        obs = env._get_current_obs
        got = ag.forward(obs)
        want = twin.forward(obs)
        assert np.array_equal(_bits(got.data[:, :N]), _bits(want.data[:, :N])) and _bits(got.data[:, :N]).any(), at
        assert np.array_equal(_bits(got._keepalive), _bits(want._keepalive)), at
        if ag.signal_channels:
            assert np.array_equal(_bits(ag.signals), _bits(twin.signals)) and _bits(ag.signals).any(), at
        if ag.memory_channels:
            assert np.array_equal(_bits(ag.memory), _bits(twin.memory)) and _bits(ag.memory).any(), at
        (plane, built), = ag._stock.values()
        assert built == epoch and np.array_equal(S.decode(plane.cpu().numpy(), epoch)[0], occ[at]), at
        if last is not None and epoch > last:                                     # not started over: the earlier build's words are still there
            assert last in np.unique(S.decode(plane.cpu().numpy(), epoch)[3]), at
        last = epoch
    for early, late in EW.SAME_TAG:                                               # a word kept from `early` would read as an agent at `late`
        assert (occ[early] & ~occ[late]).any(), (early, late)


# ---------------------------------------------------------------------------------------------------- 5. windows that straddle the wrap
def _narrow_agent():
    torch.manual_seed(0)
    ag = die.NeuralAutomataAgent(kernel_sizes=(3, 3), boundary='circular', scale=F.COEFS[0], deposit=F.COEFS[2])
    with torch.no_grad():
        for q in ag.model.parameters():
            q.uniform_(-0.5, 0.5)
    return ag


@pytest.mark.parametrize('W,H', [(13, 10), (16, 12)], ids=['13x10', '16x12'])
def test_differentiable_action_window_straddles_the_wrap(W, H):
    """The narrow stack: five forwards with a graph, the world stepped by the detached actions between them, one backward at the
    end — the graph of every link keeps its own copy of the claim plane and the epoch it was read at."""
    env, ag, watches = MGT._env(W, H), _narrow_agent(), []
    _warm_up(watches)(env, ag)
    N = env.agents.N
    rs = np.random.RandomState(4)
    weights = [k.weight.detach().cpu().double().numpy() for k in ag.model.conv_layers()]
    loss, ref, fwd = 0., None, 0.
    for t in range(EW.WINDOW):
        assert env.medium.epoch == WINDOW_EPOCHS[t] and env.agents.slot is None
        frame = MGT._frame(env, ag)
        g = rs.standard_normal((3, N)) * (env.agents.alive.cpu().numpy() > 0)[None]
        action = ag.differentiable_action(env._get_current_obs)
        loss = loss + (action * torch.as_tensor(g, dtype=torch.float32, device=DEV)).sum()
        planes = np.stack([frame['occ'], frame['food'], frame['chem']])
        act64, grads = G.gradients(weights, 'circular', planes, frame['cx'], frame['cy'], ag.action_coefs, g)
        fwd = max(fwd, MG.rel_err(action.detach().cpu().numpy(), act64))
        ref = grads if ref is None else [a + b for a, b in zip(ref, grads)]
        if t < EW.WINDOW - 1:
            MGT._step_with(env, action)
    loss.backward()
    err = MGT._errors(MGT._device_grads(ag), ref)
    print(f'narrow window {W}x{H} at {WINDOW_EPOCHS}: device', ' '.join(f'{e:.3e}' for e in err), f'(ceiling {CEILING:.0e}); forward apart by {fwd:.2e}')
    assert fwd <= FORWARD and all(e <= CEILING for e in err), (fwd, err)
    _window_crossed(watches[0], lambda env: env.medium.epoch)


@pytest.mark.parametrize('W,H', [(13, 10), (16, 12)], ids=['13x10', '16x12'])
def test_recurrent_action_window_straddles_the_wrap(W, H):
    watches = []
    ag, got, ref, leaf, ref_m, (action, memory, out) = MGT._bptt(False, leaf=True, T=EW.WINDOW, shape=(W, H), before=_warm_up(watches))
    fwd = max(MG.rel_err(action.detach().cpu().numpy(), out['actions'][-1].detach().numpy()),
              MG.rel_err(memory.detach().cpu().numpy(), out['memories'][-1].detach().numpy()))
    err = MGT._errors(got + [leaf.grad.cpu().numpy()], ref + [ref_m])
    print(f'memory window {W}x{H} at {WINDOW_EPOCHS}: device', ' '.join(f'{e:.3e}' for e in err), f'(layers, d loss / d memory0; ceiling '
          f'{CEILING:.0e}); forward apart by {fwd:.2e}')
    assert fwd <= FORWARD and np.abs(ref_m).max() > 0 and all(e <= CEILING for e in err), (fwd, err)
    _window_crossed(watches[0], lambda env: env.medium.epoch)


@pytest.mark.parametrize('M', [0, 2], ids=['K', 'K and M'])
@pytest.mark.parametrize('W,H', [(13, 10), (16, 12)], ids=['13x10', '16x12'])
def test_signalling_action_window_straddles_the_wrap(W, H, M):
    watches = []
    ag, got, ref, leaf, ref_s, (action, signals, out) = SGT._bptt(T=EW.WINDOW, M=M, shape=(W, H), before=_warm_up(watches))
    fwd = max(MG.rel_err(action.detach().cpu().numpy(), out['actions'][-1].detach().numpy()),
              MG.rel_err(signals.detach().cpu().numpy(), out['signals'][-1].detach().numpy()))
    err = MGT._errors(got + [leaf.grad.cpu().numpy()], ref + [ref_s])
    print(f'signal window {W}x{H} M={M} at {WINDOW_EPOCHS}: device', ' '.join(f'{e:.3e}' for e in err), f'(layers, d loss / d signals0; '
          f'ceiling {CEILING:.0e}); forward apart by {fwd:.2e}')
    assert fwd <= FORWARD and np.abs(ref_s).max() > 0 and all(e <= CEILING for e in err), (fwd, err)
    if M:                                                                         # the memory rows of the last layer are reached
        assert np.abs(ref[-1][3 + 2:]).max() > 0
    _window_crossed(watches[0], lambda env: env.medium.epoch)


def test_signalling_action_and_differentiable_step_window_straddles_the_wrap():
    watches = []
    fwd, err, got, ref = SGT._through_the_world(T=EW.WINDOW, before=_warm_up(watches))
    print(f'field, memory and world window 16x12 at {WINDOW_EPOCHS}: device', ' '.join(f'{e:.3e}' for e in err), f'(ceiling {CEILING:.0e}); '
          f'forward apart by {fwd:.2e}')
    assert fwd <= FORWARD and all(e <= CEILING for e in err), (fwd, err)
    assert np.abs(ref[-1][3:]).max() > 0
    watch = watches[0]                                                            # (every link is followed by its step: one step more)
    assert watch.world.medium.epoch == 3 and len(watch.occ) == EW.WARM_UP + EW.WINDOW
    _assert_a_stale_word_would_matter(watch.occ)


# Under the Dynamics of tests/test_gpu_heredity.py nobody breeds after the first pass (a cell feeds 0.1 of at most 0.5 a step, a deposit
# of 2 costs 0.04): here a cell's food lasts and feeds six times as much, and a parent needs a stock of 1.2 — every agent reaches
# it at a step of its own, so children keep being born up to the window and in it, and 1000 slots are not filled before it ends.
BREEDING = dict(dyn=dict(init_agent_ratio=0.2, food_infinite=True, rate_feed=0.6, born_threshold=1.2), slots=1000)


@pytest.mark.parametrize('mode,a', [('copy', 0.25), ('blank', 0.0)], ids=['copy 0.25', 'blank'])
def test_heredity_window_straddles_the_wrap(mode, a):
    watches = []
    run, got = HT._window(mode, a, T=EW.WINDOW, before=_warm_up(watches), **BREEDING)
    assert int((watches[0].world.agents.alive == 0).sum()) > 0                    # free slots to the end: nothing but the rule limits the births
    ref_w, ref_m, out = HT._float64(run)
    fwd = max(MG.rel_err(run['dev_mems'][-1].detach().cpu().numpy(), out['memories'][-1].detach().numpy()),
              MG.rel_err(run['dev_acts'][-1].detach().cpu().numpy(), out['actions'][-1].detach().numpy()))
    errs = [MG.rel_err(g, r) for g, r in zip(got, ref_w)] + [MG.rel_err(run['leaf'].grad.cpu().numpy(), ref_m)]
    print(f'heredity window 24x24 {mode} a={a} at {WINDOW_EPOCHS}: births per link {run["births"]}; device', ' '.join(f'{e:.3e}' for e in errs),
          f'(layers, d loss / d memory; ceiling {CEILING:.0e}); forward apart by {fwd:.2e}')
    assert all(np.abs(r).max() > 0 for r in ref_w) and np.abs(ref_m).max() > 0
    assert fwd <= FORWARD and all(e <= CEILING for e in errs), (fwd, errs)
    watch = watches[0]
    assert watch.world.medium.epoch == 3 and len(watch.occ) == EW.WARM_UP + EW.WINDOW
    _assert_a_stale_word_would_matter(watch.occ)


# ---- the batched twins
def test_batched_differentiable_action_window_straddles_the_wrap():
    W, H, R = 16, 12, 3
    benv = BatchedEnv((W, H), die.Dynamics(init_agent_ratio=0.3), replicas=R, seed=11, device=DEV)
    template = _narrow_agent()
    rows = torch.rand((R, sum(k.weight.numel() for k in template.model.conv_layers())), generator=torch.Generator().manual_seed(5)) - 0.5
    pop = BatchedNeuralAutomataAgent(benv, template, rows)
    watches = []
    _warm_up_batch(watches)(benv, pop)
    p = pop.parameters.detach().clone().requires_grad_()
    host = p.detach().cpu().double().numpy()
    rs = np.random.RandomState(4)
    loss, fwd = 0., 0.
    ref = [None] * R
    for t in range(EW.WINDOW):
        assert benv.epoch == WINDOW_EPOCHS[t]
        g = rs.standard_normal((3, R, benv.Nmax)) * (benv.alive.cpu().numpy() > 0)[None]
        for r in range(R):
            g[:, r, benv.n[r]:] = 0.
        frames = [SGB._frame(benv, pop, r) for r in range(R)]
        action = pop.differentiable_action(p)
        loss = loss + (action * torch.as_tensor(g, dtype=torch.float32, device=DEV)).sum()
        for r, f in enumerate(frames):
            n = benv.n[r]
            act64, grads = G.gradients(SGB._layer_grads(pop, host[r]), 'circular', np.stack([f['occ'], f['food'], f['chem']]), f['cx'], f['cy'],
                                       template.action_coefs, g[:, r, :n])
            fwd = max(fwd, MG.rel_err(action[:, r, :n].detach().cpu().numpy(), act64))
            ref[r] = grads if ref[r] is None else [a + b for a, b in zip(ref[r], grads)]
        if t < EW.WINDOW - 1:
            benv.step_action(action)
    loss.backward()
    torch.cuda.synchronize()
    got = p.grad.cpu().numpy()
    errs = [MG.rel_err(a, b) for r in range(R) for a, b in zip(SGB._layer_grads(pop, got[r]), ref[r])]
    print(f'batched narrow window 16x12 R=3 at {WINDOW_EPOCHS}: device', ' '.join(f'{e:.3e}' for e in errs), f'(ceiling {CEILING:.0e}); '
          f'forward apart by {fwd:.2e}')
    assert got.shape == (R, pop.P) and fwd <= FORWARD and max(errs) <= CEILING, (fwd, errs)
    _window_crossed(watches[0], lambda benv: benv.epoch)


def test_batched_recurrent_action_window_straddles_the_wrap():
    watches = []
    run = MGB._unrolled('one_tile', T=EW.WINDOW, before=_warm_up_batch(watches))
    run['loss'].backward()
    torch.cuda.synchronize()
    pop, benv = run['pop'], run['benv']
    ref_w, ref_m, outs = MGB._float64_loop(run)
    got, gm = pop.parameters.grad.cpu().numpy(), run['leaf'].grad.cpu().numpy()
    assert got.shape == (pop.candidates, pop.P)
    errs = [MG.rel_err(g, ref) for c in range(pop.candidates) for g, ref in zip(MGB._layer_grads(pop, got[c]), ref_w[c])]
    errs += [MG.rel_err(gm[r, :, :benv.n[r]], ref_m[r]) for r in range(benv.R)]
    fwd = max(MG.rel_err(pop.memory[r, :, :benv.n[r]].cpu().numpy(), outs[r]['memories'][-1].detach().numpy()) for r in range(benv.R))
    print(f'batched memory window 16x12 at {WINDOW_EPOCHS}: device worst {max(errs):.3e} of max|grad_f64| per array (ceiling {CEILING:.0e}); '
          f'forward apart by {fwd:.2e}')
    assert all(np.abs(m).max() > 0 for m in ref_m) and fwd <= FORWARD and max(errs) <= CEILING, (fwd, errs)
    _window_crossed(watches[0], lambda benv: benv.epoch)


@pytest.mark.parametrize('R,E', [(3, 1), (4, 2)], ids=['E=1', 'E=2'])
def test_batched_signalling_action_window_straddles_the_wrap(R, E):
    """16 x 12, the worlds stepped by the detached actions; with E = 2 row c of the (C, P) gradient is the sum over its two worlds."""
    watches = []
    run = SGB._bptt(16, 12, R, E, T=EW.WINDOW, before=_warm_up_batch(watches))
    errs = [MG.rel_err(g, ref) for gc, rc in zip(run['got'], run['ref']) for g, ref in zip(gc, rc)]
    errs_s = [MG.rel_err(run['got_s'][r], run['ref_s'][r]) for r in range(R)]
    print(f'batched signal window 16x12 R={R} E={E} at {WINDOW_EPOCHS}: device', ' '.join(f'{e:.3e}' for e in errs + errs_s),
          f'(ceiling {CEILING:.0e}); forward apart by {run["fwd"]:.2e}')
    assert len(run['got']) == R // E and run['fwd'] <= FORWARD
    assert np.abs(run['ref_s']).max() > 0 and max(errs + errs_s) <= CEILING, (errs, errs_s)
    _window_crossed(watches[0], lambda benv: benv.epoch)


def test_batched_signalling_action_and_differentiable_step_window_straddles_the_wrap():
    watches = []
    fwd, errs = SGB._through_the_worlds(T=EW.WINDOW, before=_warm_up_batch(watches))
    print(f'batched field, memory and worlds window 16x12 R=3 at {WINDOW_EPOCHS}: device worst {max(errs):.3e} (ceiling {CEILING:.0e}); '
          f'forward apart by {fwd:.2e}')
    assert fwd <= FORWARD and max(errs) <= CEILING, (fwd, errs)
    watch = watches[0]
    assert watch.world.epoch == 3 and len(watch.occ) == EW.WARM_UP + EW.WINDOW
    _assert_a_stale_word_would_matter(watch.occ)


@pytest.mark.parametrize('mode,a', [('copy', 0.25), ('blank', 0.0)], ids=['copy 0.25', 'blank'])
def test_batched_heredity_window_straddles_the_wrap(mode, a):
    watches = []
    births, errs, fwd = HT._batched_window(mode, a, T=EW.WINDOW, before=_warm_up_batch(watches), **BREEDING)
    assert all(sum(b[:-1]) > 0 for b in births) and int((watches[0].world.alive == 0).sum(dim=1).min()) > 0      # births in every replica's window
    print(f'batched heredity window 24x24 R=3 {mode} a={a} at {WINDOW_EPOCHS}: births {births}; device worst {max(errs):.3e} (ceiling '
          f'{CEILING:.0e}); forward apart by {fwd:.2e}')
    assert fwd <= FORWARD and max(errs) <= CEILING, (fwd, errs)
    watch = watches[0]
    assert watch.world.epoch == 3 and len(watch.occ) == EW.WARM_UP + EW.WINDOW
    _assert_a_stale_word_would_matter(watch.occ)


# ---- the same as forward, for 34 steps
def _twin_worlds_crossed(watches):
    def before(*worlds):
        watches.extend(_Watch(w) for w in worlds)
    return before


def test_recurrent_action_is_forward_for_34_steps():
    watches = []
    MGT.test_recurrent_action_is_forward_bit_for_bit(13, 10, False, True, links=EW.SAME_AS_FORWARD_STEPS, before=_twin_worlds_crossed(watches))
    assert len(watches) == 2 and all(w.world.medium.epoch == EW.sense_epoch(EW.SAME_AS_FORWARD_STEPS) == 4 for w in watches)
    _assert_a_stale_word_would_matter(watches[1].occ)


@pytest.mark.parametrize('M', [0, 2], ids=['no memory', 'memory'])
def test_signalling_action_is_forward_for_34_steps(M):
    watches = []
    SGT.test_signalling_action_is_forward_bit_for_bit(13, 10, M, False, links=EW.SAME_AS_FORWARD_STEPS, before=_twin_worlds_crossed(watches))
    assert len(watches) == 2 and all(w.world.medium.epoch == 4 for w in watches)
    _assert_a_stale_word_would_matter(watches[1].occ)


def test_batched_recurrent_action_is_the_step_for_34_steps():
    watches = []
    MGB.test_recurrent_action_is_the_step_and_the_stand_alone_call_bit_for_bit('one_tile', links=EW.SAME_AS_FORWARD_STEPS,
                                                                               before=_twin_worlds_crossed(watches))
    assert len(watches) == 2 and all(w.world.epoch == 4 for w in watches)
    _assert_a_stale_word_would_matter(watches[1].occ)


def test_batched_signalling_action_is_the_step_for_34_steps():
    watches = []
    SGB.test_signalling_action_is_the_step_and_the_stand_alone_call_bit_for_bit('24x68 memory', links=EW.SAME_AS_FORWARD_STEPS,
                                                                                before=_twin_worlds_crossed(watches))
    assert len(watches) == 2 and all(w.world.epoch == 4 for w in watches)
    _assert_a_stale_word_would_matter(watches[1].occ)


# ---------------------------------------------------------------------------------------------------- 6. backward after the tags came round
def _crowd_of(W, H, agents):
    """The largest number of alive slots on one cell, for a (4, N) agents array as `to_numpy()` returns it."""
    alive = agents[2] > 0
    cells = S.cell(S.q32_words(agents[0]), W)[alive] * H + S.cell(S.q32_words(agents[1]), H)[alive]
    return int(np.bincount(cells).max())


def _still_agent(kind):
    """An agent of `_two_links`: scale 0, so nobody moves under its own action."""
    return SGT._agent(2, scale=0.0) if kind == 'signals' else MGT._agent(scale=0.0)


def _assert_others_stand_under_the_same_tag(owner, links):
    """`links`: (sense epoch, occupancy) of a graph's links.  The claim plane as it is now holds words of each link's tag on cells
    where that link saw nobody, and none on some cell where it saw somebody: read at that tag, the plane shows other agents."""
    tags = _tags(owner)
    for epoch, occ in links:
        assert ((tags == epoch) & ~occ).any() and ((tags != epoch) & occ).any(), epoch


def _two_links_alone(kind, onward):
    """tests/test_gpu_signal_grad.py `_two_links` for a field or a memory: two links on cells of their own, nobody moving; then the
    world is driven on by `onward` steps of random non-zero actions, re-sorted, the agent's state reset, and the backward taken."""
    W, H = 13, 10
    medium, agents = F.plain_world(W, H, np.random.RandomState(2))
    env = die.Env.from_numpy(medium, agents, device=DEV)
    ag = _still_agent(kind)
    rs, N = np.random.RandomState(8), env.agents.N
    shape = (2, W, H) if kind == 'signals' else (2, N)
    u, v = (torch.as_tensor(a, dtype=torch.float32, device=DEV) for a in (rs.standard_normal((3, N)), rs.standard_normal(shape)))
    state, loss, links = None, 0., []
    for t in range(2):
        occ = SGT._occupancy(env)
        assert int(occ.sum()) == int((env.agents.to_numpy()[2] > 0).sum())        # nobody shares a cell
        links.append((env.medium.epoch, occ))
        if kind == 'signals':
            action, state, _ = ag.signalling_action(env._get_current_obs, state)
        else:
            action, state = ag.recurrent_action(env._get_current_obs, state)
        loss = loss + (u * action).sum()
        MGT._step_with(env, action)
    assert np.array_equal(links[0][1], links[1][1]) and [e for e, _ in links] == [1, 2]
    loss = loss + (v * state).sum()
    if onward:
        _drive(env, onward, np.random.RandomState(9))
        assert env.medium.epoch == EW.sense_epoch(2 + onward) == 3
        _assert_others_stand_under_the_same_tag(env.medium.owner, links)
        env.sort_agents()
        ag.reset_signals()
        ag.reset_memory()
        assert (ag.signals is None or not ag.signals.any()) and (ag.memory is None or not ag.memory.any())
    loss.backward()
    return [MM.bits(g) for g in MGT._device_grads(ag)]


@pytest.mark.parametrize('kind', ['signals', 'memory'])
def test_backward_after_the_tags_came_round_gives_the_same_bits(kind):
    at_once = _two_links_alone(kind, 0)
    assert all(g.any() for g in at_once)
    for onward in EW.MOVED_ON:
        later = _two_links_alone(kind, onward)
        assert all(np.array_equal(a, b) for a, b in zip(at_once, later)), onward


def _two_links_batch(kind, onward):
    """The batched twin on three 16 x 12 worlds (the stacks read the agents channel): the population's calls, the (C, P) gradient."""
    W, H, R = 16, 12, 3
    benv = BatchedEnv((W, H), die.Dynamics(init_agent_ratio=0.3), replicas=R, seed=5, device=DEV)
    gen, cands = torch.Generator().manual_seed(W + R), []
    for _ in range(R):                                                            # (`_agent` seeds torch itself: the rows from a generator of their own)
        ag = _still_agent(kind)
        with torch.no_grad():
            for q in ag.model.parameters():
                q.uniform_(-0.5, 0.5, generator=gen)
        cands.append(ag)
    pop = BatchedNeuralAutomataAgent.from_agents(benv, cands)
    assert pop._arch['with_agent_channel'] and len(set(benv.n)) > 1
    pop.parameters.requires_grad_()
    rs = np.random.RandomState(8)
    shape = (R, 2, W, H) if kind == 'signals' else (R, 2, benv.Nmax)
    u, v = (torch.as_tensor(a, dtype=torch.float32, device=DEV) for a in (rs.standard_normal((3, R, benv.Nmax)), rs.standard_normal(shape)))
    state, loss, links = None, 0., []
    for t in range(2):
        occ = _occupancy_batch(benv)
        # at most two alive slots on a cell: two addends commute, so the read-out's atomics leave the bits a function of the graph
        assert max(_crowd_of(W, H, benv.replica_numpy(r)[1]) for r in range(R)) <= 2
        links.append((benv.epoch, occ))
        if kind == 'signals':
            action, state, _ = pop.signalling_action(state)
        else:
            action, state = pop.recurrent_action(state)
        loss = loss + (u * (benv.alive > 0) * action).sum()
        benv.step_action(action)
    assert np.array_equal(links[0][1], links[1][1]) and [e for e, _ in links] == [1, 2]
    loss = loss + (v * state).sum()
    if onward:
        _drive_batch(benv, onward, np.random.RandomState(9))
        assert benv.epoch == EW.sense_epoch(2 + onward) == 3
        for r in range(R):
            _assert_others_stand_under_the_same_tag(benv.owner[r], [(e, occ[r]) for e, occ in links])
        pop.reset()
        assert (pop.signals is None or not pop.signals.any()) and (pop.memory is None or not pop.memory.any())
    loss.backward()
    torch.cuda.synchronize()
    return _bits(pop.parameters.grad)


@pytest.mark.parametrize('kind', ['signals', 'memory'])
def test_batched_backward_after_the_tags_came_round_gives_the_same_bits(kind):
    at_once = _two_links_batch(kind, 0)
    assert at_once.any()
    for onward in EW.MOVED_ON:
        assert np.array_equal(at_once, _two_links_batch(kind, onward)), onward
