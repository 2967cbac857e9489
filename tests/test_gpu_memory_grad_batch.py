"""Batched BPTT on the device (BatchedNeuralAutomataAgent.recurrent_action; die_memory_cells_batch /
die_memory_planes_backward_batch / die_gather_memory_backward_batch; die_nca_wide_sense_batch_store_memory /
die_nca_wide_backward_batch_memory; die_amd.functional.memory_record_batch / memory_planes_batch / gather_memory_batch):

  1. the three index entry points by ctypes against tests/memory_grad_batch_model.py word for word, guard bands included;
  2. `recurrent_action` bit for bit against `env.step(pop, action=buf)` on twin batches and against
     `replica_agent(r).recurrent_action` on `Env.from_numpy(*benv.replica_numpy(r))`;
  3. gradients at T = 1, E = 1: bit for bit the stand-alone ones, 0 in the padding and on dead slots, the same bits twice;
  4. gradients at T = 3, E = 1 and 2, against the float64 loop fed the device's own records; detached memory;
  5. through the worlds (BatchedEnv.differentiable_step) against the stand-alone twins, and after further steps and a reset;
  6. the refusals, which leave everything alone;
  7. ten Adam steps of examples/recurrent_agent.py --replicas.

The ceiling of every gradient comparison that is not bit for bit is 1e-4 of max|reference| per array, the project's backward
tolerance (CEILING in tests/test_gpu_memory_grad.py, GRAD_TOL in tests/test_gpu_field_step_grad.py);
tests/test_memory_grad_batch_cpu.py holds a plain fp32 evaluation of the batched loop below a tenth of it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from torch.nn.utils import parameters_to_vector

import die_amd as die
from die_amd import _lib, functional
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent
from die_amd.device_array import stream_ptr
from tests import field_step_adjoint_model as F
from tests import memory_grad_batch_model as MB
from tests import memory_grad_model as MG
from tests import memory_model as MM
from tests import stock_plane_model as S

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CEILING = 1e-4
TAIL = 64
NAN_BITS = MM.bits(np.float32('nan'))
SENT_I = 0x5A5A5A5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sp():
    return stream_ptr(torch.device(DEV))


def _bits(t):
    return MM.bits(t.detach().cpu().numpy())


def _nan(n):
    return torch.full((n + TAIL,), float('nan'), dtype=torch.float32, device=DEV)


def _batch(R, cells, Nmax, n):
    return _lib.Batch(R, 0, cells, Nmax, 1, (C.c_int64 * 64)(*n))


# ---------------------------------------------------------------------------------------------------- 1. the index entry points
RECORDS = {
    # the made-up 24 x 68 record of 300 slots (two blocks), replicated with different n[r]; one replica without a slot
    'crowded': ('crowded', (300, 257, 0, 40)),
    'pairs': ('pairs', (300, 256, 1)),
}


@pytest.mark.parametrize('Mc', [1, 8])
@pytest.mark.parametrize('case', list(RECORDS))
@pytest.mark.parametrize('layout', ['replica-major', 'plane-major'])
def test_memory_planes_backward_batch_is_the_model_bit_for_bit(case, Mc, layout):
    kind, n = RECORDS[case]
    W, H, Nmax, cell, win = MB.replicated_record(kind, n)
    R, cells = len(n), W * H
    rs = np.random.RandomState(Mc)
    row = Nmax + 5
    if layout == 'replica-major':                                    # [R][M] planes with gaps: a sense gradient's shape
        ps, rep = cells + 6, Mc * (cells + 6) + 10
    else:                                                            # [M][R] planes: die_memory_planes_batch's layout
        rep, ps = cells + 2, R * (cells + 2) + 4
    span = (R - 1) * rep + (Mc - 1) * ps + cells
    flat = rs.standard_normal(span).astype(np.float32)
    gp = np.stack([[flat[r * rep + j * ps:r * rep + j * ps + cells] for j in range(Mc)] for r in range(R)])
    planes, twin = torch.from_numpy(flat).to(DEV), torch.from_numpy(win).to(DEV)
    for index, tindex in ((win, twin), (cell, torch.from_numpy(cell).to(DEV))):        # the expand's adjoint; the read-out's forward
        out = _nan(R * Mc * row)
        _lib.check(_lib.lib.die_memory_planes_backward_batch(W, H, Mc, C.byref(_batch(R, cells, Nmax, n)), tindex.data_ptr(), planes.data_ptr(),
                                                             ps, rep, out.data_ptr(), row, _sp()), 'die_memory_planes_backward_batch')
        got = _bits(out)
        rows = got[:R * Mc * row].reshape(R, Mc, row)
        want = MM.bits(MB.expand_adjoint_batch(W, H, index, gp.reshape(R, Mc, W, H), np.float32))
        assert np.array_equal(rows[:, :, :Nmax], want)               # a gather: bit for bit, every word of every row written
        assert (rows[:, :, Nmax:] == NAN_BITS).all() and (got[R * Mc * row:] == NAN_BITS).all()      # the gaps, the guard band
        for r in range(R):
            assert not rows[r, :, n[r]:Nmax].any()                   # the padding: +0


@pytest.mark.parametrize('Mc', [1, 8])
@pytest.mark.parametrize('case', list(RECORDS))
def test_gather_memory_backward_batch_against_the_model(case, Mc):
    kind, n = RECORDS[case]
    W, H, Nmax, cell, _ = MB.replicated_record(kind, n)
    R, cells = len(n), W * H
    rs = np.random.RandomState(10 + Mc)
    row, lead = Nmax + 5, 3                                          # `lead` planes in front of a replica's M: a sense gradient
    rep = (lead + Mc) * cells
    gm = rs.standard_normal((R, Mc, row)).astype(np.float32)
    gm[0, 0, np.flatnonzero(cell[0] >= 0)[5]] = 0.0                  # a zero term is skipped
    tgm, tcell = torch.from_numpy(gm).to(DEV), torch.from_numpy(cell).to(DEV)
    runs = []
    for _ in range(2):
        out = _nan(R * rep)
        _lib.check(_lib.lib.die_gather_memory_backward_batch(W, H, Mc, C.byref(_batch(R, cells, Nmax, n)), tcell.data_ptr(), tgm.data_ptr(), row,
                                                             out[lead * cells:].data_ptr(), cells, rep, _sp()), 'die_gather_memory_backward_batch')
        runs.append(out)
    torch.cuda.synchronize()
    got = [r.cpu().numpy() for r in runs]
    for g in got:
        body = g[:R * rep].reshape(R, lead + Mc, cells)
        assert (MM.bits(body[:, :lead]) == NAN_BITS).all() and (MM.bits(g[R * rep:]) == NAN_BITS).all()      # not ours: untouched
        assert not np.isnan(body[:, lead:]).any()                    # ours: fully written
    planes = got[0][:R * rep].reshape(R, lead + Mc, W, H)[:, lead:]
    ref = MB.gather_adjoint_batch(W, H, cell, gm[:, :, :Nmax].astype(np.float64))
    for r in range(R):
        err = MG.rel_err(planes[r], ref[r])
        assert err <= CEILING, (r, err)
        assert n[r] > 0 or not MM.bits(planes[r]).any()              # a replica without a slot: cleared planes
    if kind == 'pairs':                                              # two addends commute: the model's fp32 bits, the same on every run
        assert max(np.bincount(c[c >= 0]).max() for c in cell if (c >= 0).any()) == 2
        assert np.array_equal(MM.bits(planes), MM.bits(MB.gather_adjoint_batch(W, H, cell, gm[:, :, :Nmax], np.float32)))
        assert np.array_equal(MM.bits(got[0]), MM.bits(got[1]))
    else:
        assert np.bincount(cell[0][cell[0] >= 0]).max() >= 3


# ---------------------------------------------------------------------------------------------------- populations and worlds
def _cands(n, seed, M=2, p=0.0, **kw):
    torch.manual_seed(seed)
    out = []
    for _ in range(n):
        ag = die.NeuralAutomataAgent(scale=F.COEFS[0], deposit=F.COEFS[2], memory_channels=M, p_agent_dropout=p, **kw)
        with torch.no_grad():
            for q in ag.model.parameters():
                q.uniform_(-0.5, 0.5)
        out.append(ag)
    return out


WIDE = dict(kernel_sizes=(3, 3), hidden_channels=8, hidden_activation='tanh')
FLOW = lambda W, H: die.WaveSequence((W, H), dt=0.01).get_flow_operator(scale=0.5, decay=0.5)     # noqa: E731


def _two_dynamics(W, H):
    """Per-replica Dynamics for R = 4, E = 2 (candidate-major): every candidate's world 0 plain, its world 1 under a food flow
    (one operator object for the batch) with another diffusion and decay."""
    flow = FLOW(W, H)
    return [dict(init_agent_ratio=0.3), dict(init_agent_ratio=0.3, diffuse_sigma=0.5, rate_decay_chem=0.05, op_food_flow=flow)] * 2


CASES = {
    # (W, H), R, E, M, model, slots, Dynamics (built anew for every env), population arguments, dropout p
    # 13 x 10: H % 4 != 0, scalar stores, one tile; a single layer (no ping-pong sets), k = 5, zero padding, no agents channel
    'odd_single_layer': ((13, 10), 3, 1, 1, dict(kernel_sizes=(5,), boundary='zeros', with_agent_channel=False), 'alive',
                         lambda W, H: dict(init_agent_ratio=0.3), {}, 0.0),
    # 16 x 12: one tile, two layers
    'one_tile': ((16, 12), 3, 1, 2, WIDE, 'alive', lambda W, H: dict(init_agent_ratio=0.3), {}, 0.0),
    # 24 x 68: four 16 x 64 tiles; at ratio 0.2 more than 256 slots; a mask every replica shares (stride 0); three layers, k = 1, 3, 5
    'tiles_mask': ((24, 68), 3, 1, 2, dict(kernel_sizes=(1, 3, 5), hidden_channels=6, hidden_activation='relu'), 'alive',
                   lambda W, H: dict(init_agent_ratio=0.2), dict(dropout_seed=40, dropout_seed_stride=0), 0.25),
    # E = 2 with R = 4, M = 8, a mask per replica (stride 1), per-replica Dynamics (one of the two with a food flow)
    'episodes_mask': ((16, 12), 4, 2, 8, WIDE, 'alive', lambda W, H: _two_dynamics(W, H), dict(dropout_seed=7, dropout_seed_stride=1), 0.25),
    # agents_die on the fixed layout: dead slots from the first step on
    'die_fixed': ((24, 68), 3, 1, 2, WIDE, 400, lambda W, H: dict(init_agent_ratio=0.2, agents_die=True, food_infinite=False), {}, 0.0),
}


def _make(case, seed=11):
    (W, H), R, E, M, model_kw, slots, dyn_kw, pop_kw, p = CASES[case]
    d = dyn_kw(W, H)
    dynamics = [die.Dynamics(**q) for q in d] if isinstance(d, list) else die.Dynamics(**d)
    benv = BatchedEnv((W, H), dynamics, replicas=R, seed=seed, max_agents=slots, device=DEV)
    pop = BatchedNeuralAutomataAgent.from_agents(benv, _cands(R // E, W + R, M, p, **model_kw), E, **pop_kw)
    assert pop._memory_channels == M and not benv.per_replica
    return benv, pop


def _alone(benv, pop, r):
    """Replica r as a stand-alone world and agent, as they stand now (blank memory; the population's dropout counter)."""
    env = die.Env.from_numpy(*benv.replica_numpy(r), device=DEV, sort_every=0)
    ag = pop.replica_agent(r)
    ag.dropout_step = pop.dropout_step
    return env, ag


def _world_bits(benv):
    return benv._state.cpu().numpy().copy(), benv.epoch


def _same_world(a, b):
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]


# ---------------------------------------------------------------------------------------------------- 1d. the record on real worlds
@pytest.mark.parametrize('case', ['odd_single_layer', 'tiles_mask', 'die_fixed'])
def test_memory_cells_batch_against_the_model_on_real_worlds(case):
    benv, pop = _make(case)
    if case == 'die_fixed':
        benv.run(pop, 2)                                             # somebody has died
    R, W, H, Nmax = benv.R, benv.W, benv.H, benv.Nmax
    if case == 'tiles_mask':
        assert Nmax > 256                                            # two blocks of slots
    rec = functional.memory_record_batch(pop)
    again = functional.memory_record_batch(pop)                      # two calls at one epoch: the population's own planes, zeroed
    assert (rec.R, rec.W, rec.H, rec.Nmax, rec.n) == (R, W, H, Nmax, tuple(benv.n)) and rec.cell.dtype == rec.win.dtype == torch.int32
    cell, win = rec.cell.cpu().numpy(), rec.win.cpu().numpy()
    assert np.array_equal(cell, again.cell.cpu().numpy()) and np.array_equal(win, again.win.cpu().numpy())
    for r in range(R):
        n = benv.n[r]
        want_cell, want_win = MG.record_of(W, H, benv.replica_numpy(r)[1])
        assert np.array_equal(cell[r, :n], want_cell) and np.array_equal(win[r, :n], want_win), r
        assert (cell[r, n:] == -1).all() and (win[r, n:] == -1).all(), r
    assert len(set(benv.n)) > 1 or benv._fixed is not None           # differing n[r], or the fixed layout
    if case == 'die_fixed':
        assert (cell[:, :Nmax] < 0).any()
    # by ctypes into guarded buffers: nothing beyond the R rows is written
    out = torch.full((2, R * Nmax + TAIL), SENT_I, dtype=torch.int32, device=DEV)
    m, a, _, b = benv._structs()
    _lib.check(_lib.lib.die_memory_cells_batch(C.byref(m), C.byref(a), C.byref(b), rec._standing.data_ptr(), benv.epoch, out[0].data_ptr(),
                                               out[1].data_ptr(), _sp()), 'die_memory_cells_batch')
    host = out.cpu().numpy()
    assert (host[:, R * Nmax:] == SENT_I).all()
    assert np.array_equal(host[0, :R * Nmax].reshape(R, Nmax), cell) and np.array_equal(host[1, :R * Nmax].reshape(R, Nmax), win)


def test_the_two_functional_ops_alone():
    """memory_planes_batch and gather_memory_batch on plain tensors: the model's values, gradients through a slice of a larger
    sense tensor (read where it lies) and through contiguous planes, the shape refusals."""
    benv, pop = _make('one_tile')
    R, W, H, Nmax, M = benv.R, benv.W, benv.H, benv.Nmax, 2
    rec = functional.memory_record_batch(pop)
    cell, win = rec.cell.cpu().numpy(), rec.win.cpu().numpy()
    rs = np.random.RandomState(8)
    mem = torch.from_numpy(rs.standard_normal((R, M, Nmax)).astype(np.float32)).to(DEV).requires_grad_()
    sense = torch.from_numpy(rs.standard_normal((R, 3 + M, W, H)).astype(np.float32)).to(DEV).requires_grad_()
    planes = functional.memory_planes_batch(mem, rec)
    out = functional.gather_memory_batch(sense[:, 3:], rec)
    assert planes.shape == (M, R, W, H) and out.shape == (R, M, Nmax) and planes.grad_fn is not None and out.grad_fn is not None
    want = MB.expand_batch(W, H, win, mem.detach().cpu().numpy(), np.float32)
    assert np.array_equal(_bits(planes.permute(1, 0, 2, 3)), MM.bits(want))
    assert np.array_equal(_bits(out), MM.bits(MB.gather_batch(W, H, cell, sense.detach().cpu().numpy()[:, 3:], np.float32)))
    gp = torch.from_numpy(rs.standard_normal((M, R, W, H)).astype(np.float32)).to(DEV)
    gm = torch.from_numpy(rs.standard_normal((R, M, Nmax)).astype(np.float32)).to(DEV)
    ((planes * gp).sum() + (out * gm).sum()).backward()
    assert np.array_equal(_bits(mem.grad), MM.bits(MB.expand_adjoint_batch(W, H, win, gp.permute(1, 0, 2, 3).cpu().numpy(), np.float32)))
    assert not _bits(sense.grad[:, :3]).any()
    assert np.array_equal(_bits(sense.grad[:, 3:]), MM.bits(MB.gather_adjoint_batch(W, H, cell, gm.cpu().numpy(), np.float32)))      # (one slot a cell)
    for bad in (torch.zeros((R - 1, M, Nmax), device=DEV), torch.zeros((R, 9, Nmax), device=DEV), torch.zeros((R, M, Nmax + 1), device=DEV),
                torch.zeros((R, M, Nmax), device=DEV, dtype=torch.float64)):
        with pytest.raises(ValueError, match='memory'):
            functional.memory_planes_batch(bad, rec)
    with pytest.raises(ValueError, match='sense_tail'):
        functional.gather_memory_batch(torch.zeros((R, M, W, H + 1), device=DEV), rec)


# ---------------------------------------------------------------------------------------------------- 2. the values
@pytest.mark.parametrize('case', list(CASES))
def test_recurrent_action_is_the_step_and_the_stand_alone_call_bit_for_bit(case, links=3, before=None):
    """(`links`, `before` — a callable of the two fresh batches: tests/test_gpu_epoch_wrap.py runs the same checks across the epoch wrap.)"""
    (benv_s, pop_s), (benv_d, pop_d) = _make(case), _make(case)
    if before is not None:
        before(benv_s, benv_d)
    R, M, Nmax = benv_s.R, pop_s._memory_channels, benv_s.Nmax
    _same_world(_world_bits(benv_s), _world_bits(benv_d))
    steps = benv_s.H % 4 == 0                                        # (the batched step takes H % 4 == 0: a 13 x 10 world stands still)
    buf = torch.zeros((3, R, Nmax), dtype=torch.float32, device=DEV)
    pop_d.parameters.requires_grad_()                                # (a graph hangs on what asks for a gradient: here the weights)
    memory = None
    for t in range(links):
        mem_in = pop_d.memory.clone()
        alone = [_alone(benv_d, pop_d, r) for r in range(R)]
        action, memory = pop_d.recurrent_action(memory)
        assert action.shape == (3, R, Nmax) and memory.shape == (R, M, Nmax) and action.dtype == memory.dtype == torch.float32
        assert action.grad_fn is not None and memory.grad_fn is not None
        if steps:
            benv_s.step(pop_s, action=buf)
        for r in range(R):
            n = benv_d.n[r]
            assert not steps or np.array_equal(_bits(action[:, r, :n]), _bits(buf[:, r, :n])), (t, r)
            assert not _bits(action[:, r, n:]).any() and not _bits(memory[r, :, n:]).any(), (t, r)        # the padding: 0
            env, ag = alone[r]
            a, m = ag.recurrent_action(env._get_current_obs, mem_in[r, :, :n].contiguous())
            assert np.array_equal(_bits(a), _bits(action[:, r, :n])) and np.array_equal(_bits(m), _bits(memory[r, :, :n])), (t, r)
        assert np.array_equal(_bits(pop_d.memory), _bits(memory)) and pop_d.memory.data_ptr() != memory.data_ptr(), t
        assert pop_d.dropout_step == (t + 1 if pop_d.dropout_seed is not None else 0)
        if steps:
            assert np.array_equal(_bits(pop_s.memory), _bits(memory)) and pop_s.dropout_step == pop_d.dropout_step, t
            benv_d.step_action(action)
            _same_world(_world_bits(benv_s), _world_bits(benv_d))
    assert float(memory.detach().abs().max()) > 0
    if case == 'die_fixed':
        assert int((benv_d.alive == 0).sum()) > 0


# ---------------------------------------------------------------------------------------------------- 3. gradients at T = 1
def _row_of(ag):
    return parameters_to_vector([q.grad for q in ag.model.parameters()]).detach().cpu().numpy()


@pytest.mark.parametrize('case', ['odd_single_layer', 'one_tile', 'tiles_mask', 'die_fixed'])
def test_one_step_gradients_are_the_stand_alone_ones_bit_for_bit(case):
    benv, pop = _make(case)                                          # (die_fixed: the fixed layout has a dead tail from the start)
    R, M, Nmax = benv.R, pop._memory_channels, benv.Nmax
    # bit equality holds where no cell holds more than two alive slots with a non-zero gradient: so it is in a fresh world
    cell = functional.memory_record_batch(pop).cell.cpu().numpy()
    crowd = max(int(np.bincount(c[c >= 0]).max()) for c in cell)
    print(f'{case}: at most {crowd} alive slot(s) on a cell')
    assert crowd <= 2
    rs = np.random.RandomState(3)
    u = torch.from_numpy(rs.standard_normal((3, R, Nmax)).astype(np.float32)).to(DEV)
    v = torch.from_numpy(rs.standard_normal((R, M, Nmax)).astype(np.float32)).to(DEV)
    leaf = torch.from_numpy(rs.standard_normal((R, M, Nmax)).astype(np.float32)).to(DEV).requires_grad_()
    # the loss is on the alive agents' actions, as a training loss is: dead slots lie piled on a few cells, and the read-out's
    # adjoint adds in arrival order where more than two slots with a non-zero gradient share one (include/die_hip.h)
    u = u * (benv.alive > 0)
    alone = [_alone(benv, pop, r) for r in range(R)]
    pop.parameters.requires_grad_()
    action, memory = pop.recurrent_action(leaf)
    loss = (u * action).sum() + (v * memory).sum()
    loss.backward(retain_graph=True)
    got_p, got_m = pop.parameters.grad.clone(), leaf.grad.clone()
    pop.parameters.grad = leaf.grad = None
    loss.backward()
    assert np.array_equal(_bits(got_p), _bits(pop.parameters.grad)) and np.array_equal(_bits(got_m), _bits(leaf.grad))        # the same bits twice
    alive = benv.alive.cpu().numpy() > 0
    for r in range(R):
        n = benv.n[r]
        env, ag = alone[r]
        mem = leaf.detach()[r, :, :n].clone().requires_grad_()
        a, m = ag.recurrent_action(env._get_current_obs, mem)
        ((u[:, r, :n] * a).sum() + (v[r, :, :n] * m).sum()).backward()
        assert np.array_equal(_bits(got_p[r]), MM.bits(_row_of(ag))), r
        assert np.array_equal(_bits(got_m[r, :, :n]), _bits(mem.grad)), r
        assert not _bits(got_m[r, :, n:]).any(), r                   # the padding: exactly 0
        assert not _bits(got_m[r, :, :n][:, ~alive[r, :n]]).any(), r                # dead slots: exactly 0
    assert float(got_m.abs().max()) > 0 and float(got_p.abs().max()) > 0
    if case == 'die_fixed':
        assert (~alive[:, :min(benv.n)]).any()


# ---------------------------------------------------------------------------------------------------- 4. BPTT
def _frame(benv, pop, r, p):
    W, H, n = benv.W, benv.H, benv.n[r]
    m, _ = benv.replica_numpy(r)
    cx = S.cell(benv.x[r, :n].cpu().numpy().view(np.uint32), W)
    cy = S.cell(benv.y[r, :n].cpu().numpy().view(np.uint32), H)
    mask = None
    if p > 0:
        mask = MG.mask_of(pop.dropout_seed + r * pop.dropout_seed_stride, pop.dropout_step, W, H, p).astype(np.float64)
    return dict(occ=m[0], food=m[1], chem=m[2], cx=cx, cy=cy, mask=mask)


def _layer_grads(pop, row):
    """A (P,) row as the list of its layers' (cout, cin, k, k) arrays."""
    return [np.asarray(row[off:off + cout * cin * k * k]).reshape(cout, cin, k, k) for k, cin, cout, off in pop._layers]


def _unrolled(case, T=3, detach=False, leaf=True, before=None):
    """T rounds chained through memory_next, the worlds stepped by the detached actions between them, a loss term at every round:
    the device's gradients and everything the float64 loop needs to repeat them.  `before`: a callable of (benv, pop) run on the
    fresh worlds first (tests/test_gpu_epoch_wrap.py: real steps up to the epoch wrap)."""
    benv, pop = _make(case)
    if before is not None:
        before(benv, pop)
    p = CASES[case][8]
    R, M, Nmax, E = benv.R, pop._memory_channels, benv.Nmax, pop.episodes
    rs = np.random.RandomState(4)
    us, vs = rs.standard_normal((T, 3, R, Nmax)), rs.standard_normal((T, R, M, Nmax))
    mem0 = rs.standard_normal((R, M, Nmax)).astype(np.float32)
    leaf_memory = torch.from_numpy(mem0).to(DEV).requires_grad_(leaf)
    pop.parameters.requires_grad_()
    memory, frames, records, loss, per_step = leaf_memory, [[] for _ in range(R)], [[] for _ in range(R)], 0., []
    for t in range(T):
        rec = functional.memory_record_batch(pop)                    # the device's own record of this round
        cell, win = rec.cell.cpu().numpy(), rec.win.cpu().numpy()
        for r in range(R):
            frames[r].append(_frame(benv, pop, r, p))
            records[r].append((cell[r, :benv.n[r]].copy(), win[r, :benv.n[r]].copy()))
        action, memory = pop.recurrent_action(memory.detach() if detach else memory)
        term = (torch.as_tensor(us[t], dtype=torch.float32, device=DEV) * action).sum() + \
            (torch.as_tensor(vs[t], dtype=torch.float32, device=DEV) * memory).sum()
        per_step.append(term)
        loss = loss + term
        if t < T - 1:
            benv.step_action(action)
    return dict(benv=benv, pop=pop, loss=loss, per_step=per_step, leaf=leaf_memory, mem0=mem0, us=us, vs=vs, frames=frames, records=records,
                E=E, p=p, case=case)


def _float64_loop(run, detach=False):
    """([C rows of d loss / d parameters as layer lists], [R arrays d loss / d mem0[r]]) of the float64 loop on the device's data."""
    pop, benv = run['pop'], run['benv']
    model_kw = CASES[run['case']][4]
    R, E, T = benv.R, run['E'], len(run['us'])
    host = pop.parameters.detach().cpu().double().numpy()
    ws = [[torch.tensor(w, requires_grad=True) for w in _layer_grads(pop, host[c])] for c in range(pop.candidates)]
    m0 = [torch.tensor(run['mem0'][r, :, :benv.n[r]].astype(np.float64), requires_grad=True) for r in range(R)]
    outs = MB.unroll_batch(ws, model_kw.get('boundary', 'circular'), model_kw.get('hidden_activation'), run['frames'], run['records'], m0,
                           pop.template.action_coefs, E, pop._arch['with_agent_channel'], detach_at=range(T) if detach else ())
    loss = 0.
    for r, out in enumerate(outs):
        n = benv.n[r]
        for t in range(T):
            loss = loss + (torch.as_tensor(run['us'][t][:, r, :n]) * out['actions'][t]).sum() + \
                (torch.as_tensor(run['vs'][t][r, :, :n]) * out['memories'][t + 1]).sum()
    loss.backward()
    zero = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()     # noqa: E731
    return [[zero(w) for w in row] for row in ws], [zero(m) for m in m0], outs


@pytest.mark.parametrize('case', ['one_tile', 'tiles_mask', 'episodes_mask'])
def test_bptt_gradients_match_the_float64_loop(case):
    run = _unrolled(case)
    run['loss'].backward()
    torch.cuda.synchronize()
    pop, benv = run['pop'], run['benv']
    ref_w, ref_m, outs = _float64_loop(run)
    got = pop.parameters.grad.cpu().numpy()
    assert got.shape == (pop.candidates, pop.P)
    errs = []
    for c in range(pop.candidates):
        for g, ref in zip(_layer_grads(pop, got[c]), ref_w[c]):
            assert np.abs(ref).max() > 0
            errs.append(MG.rel_err(g, ref))
    gm = run['leaf'].grad.cpu().numpy()
    for r in range(benv.R):
        n = benv.n[r]
        assert np.abs(ref_m[r]).max() > 0
        errs.append(MG.rel_err(gm[r, :, :n], ref_m[r]))
        assert not MM.bits(gm[r, :, n:]).any()
    fwd = max(MG.rel_err(pop.memory[r, :, :benv.n[r]].cpu().numpy(), outs[r]['memories'][-1].detach().numpy()) for r in range(benv.R))
    print(f'bptt {case} T=3 E={run["E"]}: device worst {max(errs):.3e} of max|grad_f64| per array (ceiling {CEILING:.0e}); forward apart by {fwd:.2e}')
    assert fwd <= 1e-5                                               # the model followed the same trajectory
    assert max(errs) <= CEILING, errs
    if run['E'] == 1:
        shared = max(int((np.bincount(c[c >= 0]) > 1).sum()) for recs in run['records'] for c, _ in recs)
        print(f'  cells shared on the way: {shared}')


def test_detached_memory_gives_the_sum_of_the_one_step_gradients():
    run = _unrolled('one_tile', detach=True)
    run['loss'].backward()
    pop = run['pop']
    got = pop.parameters.grad.cpu().double().numpy()
    assert run['leaf'].grad is None                                  # nothing reaches the memory leaf behind a detach
    # the same rounds, one backward each
    twin = _unrolled('one_tile', detach=True)
    total = np.zeros_like(got)
    for term in twin['per_step']:
        twin['pop'].parameters.grad = None
        term.backward()
        total += twin['pop'].parameters.grad.cpu().double().numpy()
    for c in range(pop.candidates):
        assert np.abs(total[c]).max() > 0 and MG.rel_err(got[c], total[c]) <= CEILING, c
    ref_w, _, _ = _float64_loop(run, detach=True)
    for c in range(pop.candidates):
        for g, ref in zip(_layer_grads(pop, got[c]), ref_w[c]):
            assert MG.rel_err(g, ref) <= CEILING


# ---------------------------------------------------------------------------------------------------- 5. through the worlds
def _through_the_worlds(later: bool):
    W, H, R, sigma = 16, 12, 3, 0.8
    dyn = lambda: die.Dynamics(init_agent_ratio=0.3, diffuse_sigma=sigma, rate_decay_chem=F.DECAY, diffuse_mode='wrap')       # noqa: E731
    benv = BatchedEnv((W, H), dyn(), replicas=R, seed=5, device=DEV)
    pop = BatchedNeuralAutomataAgent.from_agents(benv, _cands(R, 9, 2, **WIDE))
    pop.parameters.requires_grad_()
    cvec = torch.from_numpy(np.random.RandomState(6).standard_normal((R, W, H)).astype(np.float32)).to(DEV)
    benv.differentiable_chem()
    memory = None
    for _ in range(2):
        action, memory = pop.recurrent_action(memory)
        benv.differentiable_step(action)
    loss = (cvec * benv.differentiable_chem()).sum()
    if later:                                                        # the records are the graph's: the worlds may go on, and start over
        benv.run(pop, 2)
        benv.reset()
    loss.backward()
    return benv, pop, cvec, dyn, pop.parameters.grad.clone()


def test_gradients_through_the_memory_and_the_worlds():
    benv, pop, cvec, dyn, got = _through_the_worlds(False)
    _, _, _, _, got_later = _through_the_worlds(True)
    assert np.array_equal(_bits(got), _bits(got_later))
    errs = []
    for r in range(benv.R):
        env = die.Env((benv.W, benv.H), dyn(), seed=benv.seeds[r], max_agents='alive', device=DEV, sort_every=0)
        ag = pop.replica_agent(r)
        env.differentiable_chem()
        memory = None
        for _ in range(2):
            action, memory = ag.recurrent_action(env._get_current_obs, memory)
            env.differentiable_step(action)
        (cvec[r] * env.differentiable_chem()).sum().backward()
        ref = _row_of(ag)
        assert np.abs(ref).max() > 0
        for g, want in zip(_layer_grads(pop, got[r].cpu().numpy()), _layer_grads(pop, ref)):
            errs.append(MG.rel_err(g, want))
        # the last layer's rows 3.. produce memory: they reach this loss through the memory AND the world only
        assert np.abs(_layer_grads(pop, ref)[-1][3:]).max() > 0
    print(f'through the worlds 16x12 T=2: worst {max(errs):.3e} of max|stand-alone grad| per layer (ceiling {CEILING:.0e})')
    assert max(errs) <= CEILING, errs


# ---------------------------------------------------------------------------------------------------- 6. the refusals
@pytest.mark.parametrize('what', ['stock', 'fp16', 'reflect', 'per_replica', 'wrong shape', 'wrong dtype', 'no memory'])
def test_refusals_on_the_device_leave_everything_alone(what):
    W, H, R = 13, 10, 2
    kw = dict(with_stock_channel=True) if what == 'stock' else dict(boundary='reflect') if what == 'reflect' else {}
    benv = BatchedEnv((W, H), die.Dynamics(init_agent_ratio=0.3), replicas=R, seed=2, device=DEV,
                      field_dtype=torch.float16 if what == 'fp16' else torch.float32, per_replica=True if what == 'per_replica' else None)
    pop = BatchedNeuralAutomataAgent.from_agents(benv, _cands(R, 1, 0 if what == 'no memory' else 2, 0.25, **WIDE, **kw), dropout_seed=3)
    pop.dropout_step = 4
    held = None
    if pop.memory is not None:
        pop.memory.fill_(0.5)
        held = pop.memory
    before = None if benv.per_replica else _world_bits(benv)
    memory = None
    if what == 'wrong shape':
        memory = torch.zeros((R, 2, benv.Nmax + 1), device=DEV)
    if what == 'wrong dtype':
        memory = torch.zeros((R, 2, benv.Nmax), device=DEV, dtype=torch.float64)
    with pytest.raises(ValueError if what in ('wrong shape', 'wrong dtype', 'no memory') else NotImplementedError, match='recurrent_action'):
        pop.recurrent_action(memory)
    assert pop.dropout_step == 4 and pop.memory is held and (held is None or bool((held == 0.5).all()))
    if before is not None:
        _same_world(before, _world_bits(benv))
    if what == 'wrong shape':                                        # what the issue keeps refused stays refused
        for call in (pop.differentiable_sense, pop.differentiable_action, pop.forward_device):
            with pytest.raises(NotImplementedError, match='memory'):
                call()
        assert pop.dropout_step == 4 and bool((pop.memory == 0.5).all())
        _same_world(before, _world_bits(benv))


# ---------------------------------------------------------------------------------------------------- 7. training
def test_ten_adam_steps_of_the_batched_example_decrease_the_loss():
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    try:
        import recurrent_agent
    finally:
        sys.path.pop(0)
    pop, losses = recurrent_agent.train_batched(24, 2, 3, 0, 10, replicas=4, students=2, log=lambda *_: None)
    print('recurrent_agent --replicas 4 --students 2 --size 24 --unroll 3, ten Adam steps:', ' '.join(f'{v:.4f}' for v in losses))
    assert len(losses) == 10 and np.isfinite(losses).all() and losses[-1] < losses[0]
    assert pop.candidates == 2 and float(pop.memory.abs().max()) > 0
