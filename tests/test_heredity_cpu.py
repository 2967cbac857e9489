"""Heredity without a GPU: tests/heredity_model.py checked on its own (the record's two sets are disjoint, no mutation moves words,
a mutation stays within its half-width, channels 4.. draw from a second Philox block, the adjoint is the transpose), and the host
rules that need no device — NeuralAutomataAgent's two arguments, their ValueErrors, and their way through `init_params`, `save` /
`load` and `BatchedNeuralAutomataAgent.unpack`."""
import io

import numpy as np
import pytest
import torch

import die_amd as die
from die_amd.batch import BatchedNeuralAutomataAgent, _architecture
from oracle.rng import _draw
from tests import births_model as B
from tests import heredity_model as HM
from tests import memory_model as MM

SEED, STEP = 0x0123456789ABCDEF, 41


def _world(n, rs):
    role = rs.choice([0, 1, 2], n, p=[0.2, 0.4, 0.4])                # poor, parent, free
    alive = (role != 2).astype(np.uint8)
    food = np.where(role == 1, rs.uniform(0.51, 9.0, n), np.where(role == 0, rs.uniform(0, 0.5, n), 0)).astype(np.float32)
    return alive, food


@pytest.mark.parametrize('n', [1, 2, 65, 1000])
def test_the_record_pairs_disjoint_sets_in_slot_order(n):
    rs = np.random.RandomState(n)
    alive, food = _world(n, rs)
    parent_of, child_of = HM.record(alive, food, 0.5)
    parents, free = B.match(alive, food, 0.5)
    par, chi = HM.pairs(parent_of)
    assert parent_of.dtype == child_of.dtype == np.int32 and len(parent_of) == len(child_of) == n
    assert np.array_equal(np.sort(par), parents) and np.array_equal(chi, free)
    assert not set(par.tolist()) & set(chi.tolist())                 # nobody is parent and child in one pass
    assert len(set(par.tolist())) == len(par)                        # a parent has one child a pass
    assert np.array_equal(child_of[par], chi) and np.array_equal(parent_of[chi], par)
    assert (alive[par] == 1).all() and (alive[chi] == 0).all()
    padded = HM.record(alive, food, 0.5, n + 7)
    assert all(np.array_equal(p[:n], q) and (p[n:] == -1).all() for p, q in zip(padded, (parent_of, child_of)))


@pytest.mark.parametrize('M', [1, 4, 5, 8])
def test_inherit_moves_words_or_stays_within_the_mutation(M):
    n = 300
    rs = np.random.RandomState(M)
    alive, food = _world(n, rs)
    parent_of, _ = HM.record(alive, food, 0.5)
    par, chi = HM.pairs(parent_of)
    assert len(par) > 20
    mem = rs.standard_normal((M, n)).astype(np.float32)
    words = mem.view(np.uint32)
    specials = (0x80000000, 0x00000123, 0x7F800000, 0x7FC12345)      # -0.0, a denormal, inf, a NaN payload
    for j, w in enumerate(specials):
        words[j % M, par[j]] = w
    before = MM.bits(mem).copy()
    others = np.setdiff1d(np.arange(n), chi)
    copy = MM.bits(HM.inherit(mem, parent_of, 'copy'))
    assert np.array_equal(MM.bits(mem), before)                      # the input is left alone
    assert np.array_equal(copy[:, chi], before[:, par]) and np.array_equal(copy[:, others], before[:, others])
    blank = MM.bits(HM.inherit(mem, parent_of, 'blank'))
    assert not blank[:, chi].any() and np.array_equal(blank[:, others], before[:, others])
    a = 0.25
    clean = rs.standard_normal((M, n)).astype(np.float32)
    got = HM.inherit(clean, parent_of, 'copy', a, SEED, STEP)
    assert np.array_equal(MM.bits(got[:, others]), MM.bits(clean[:, others]))          # the parents keep theirs
    d = np.abs(got[:, chi].astype(np.float64) - clean[:, par].astype(np.float64))
    assert (d <= a + np.spacing(np.maximum(np.abs(got[:, chi]), np.abs(clean[:, par])))).all() and d.max() > a / 2 and (d > 0).mean() > 0.99
    u = HM.unit_noise(SEED, STEP, par, M)
    assert u.dtype == np.float32 and np.abs(u).max() <= 1.0 and abs(float(u.mean())) < 0.1 and u.min() < -0.8 and u.max() > 0.8
    want = (clean[:, par] + (np.float32(a) * u).astype(np.float32)).astype(np.float32)   # two roundings, never one
    assert np.array_equal(MM.bits(got[:, chi]), MM.bits(want))
    assert not np.array_equal(got, HM.inherit(clean, parent_of, 'copy', a, SEED, STEP + 1))
    assert not np.array_equal(got, HM.inherit(clean, parent_of, 'copy', a, SEED + 1, STEP))


def test_channels_four_and_up_draw_from_a_second_philox_block():
    par = np.array([0, 5, 2 ** 31 + 3, 0x07FFFFFE], dtype=np.uint64)
    u = HM.unit_noise(SEED, STEP, par, 8)
    first = _draw(SEED, STEP, par, HM.STREAM_HEREDITY)
    second = _draw(SEED, STEP, par | (np.uint64(1) << np.uint64(32)), HM.STREAM_HEREDITY)
    as_u = lambda w: np.asarray(w, dtype=np.uint32).view(np.int32).astype(np.float32) * np.float32(2.0 ** -31)
    for m in range(8):
        assert np.array_equal(u[m], as_u((first if m < 4 else second)[m & 3])), m
    assert not np.array_equal(u[0], u[4])
    # the conversion rounds to nearest even (2^31 - 1 -> 2^31: u = 1 exactly) and the scaling is exact
    assert as_u(np.array([0x7FFFFFFF, 0x80000000, 0x00000001, 0x7FFFFF40], dtype=np.uint32)).tolist() == [1.0, -1.0, 2.0 ** -31, (2 ** 31 - 256) / 2 ** 31]


@pytest.mark.parametrize('mode', HM.MODES)
def test_the_adjoint_is_the_transpose_exactly_on_an_integer_lattice(mode):
    n, M = 400, 5
    rs = np.random.RandomState(3)
    alive, food = _world(n, rs)
    parent_of, child_of = HM.record(alive, food, 0.5)
    x = rs.randint(-50, 51, (M, n)).astype(np.float64)
    y = rs.randint(-50, 51, (M, n)).astype(np.float64)
    Jx = HM.jacobian_apply(x, parent_of, mode)
    Jty = HM.inherit_adjoint(y, parent_of, child_of, mode, np.float64)
    assert float((Jx * y).sum()) == float((x * Jty).sum())            # <J x, y> = <x, Jt y>: integers, so exactly
    assert np.array_equal(HM.inherit_adjoint(y, parent_of, child_of, mode, np.float32), Jty.astype(np.float32))
    par, chi = HM.pairs(parent_of)
    assert not Jty[:, chi].any() and (Jty[:, par] != y[:, par]).any() == (mode == 'copy')
    # the model's own forward has this Jacobian: the mutation is an additive constant
    base = rs.randint(-50, 51, (M, n)).astype(np.float32)
    f = lambda v: HM.inherit(v, parent_of, mode, 0.25 if mode == 'copy' else 0.0, SEED, STEP).astype(np.float64)
    step = f(base + x.astype(np.float32) * np.float32(64)) - f(base)
    # (exact up to the rounding of the two mutated sums: below 4096 an fp32 sum is off by at most 2^-13, their difference by 2^-12)
    assert np.abs(step - 64 * Jx).max() <= 2.0 ** -12
    t = torch.tensor(base.astype(np.float64), requires_grad=True)
    added = HM.noise(SEED, STEP, par, M, 0.25) if mode == 'copy' else None
    (HM.t_inherit(t, parent_of, mode, added) * torch.as_tensor(y)).sum().backward()
    assert np.array_equal(t.grad.numpy(), Jty)


# ---------------------------------------------------------------------------------------------------- the host rules
KW = dict(kernel_sizes=(3, 3), hidden_channels=4)


@pytest.mark.parametrize('kw', [
    dict(memory_channels=2, memory_inherit='clone'),
    dict(memory_channels=2, memory_inherit=True),
    dict(memory_channels=2, memory_inherit=['copy']),
    dict(memory_channels=2, memory_inherit='copy', memory_mutation=-0.1),
    dict(memory_channels=2, memory_inherit='copy', memory_mutation=float('nan')),
    dict(memory_channels=2, memory_inherit='copy', memory_mutation=float('inf')),
    dict(memory_channels=2, memory_inherit='copy', memory_mutation=1e39),          # not a finite float32
    dict(memory_channels=2, memory_inherit='copy', memory_mutation='0.1'),
    dict(memory_channels=2, memory_inherit='copy', memory_mutation=None),
    dict(memory_channels=2, memory_inherit='copy', memory_mutation=True),
    dict(memory_channels=2, memory_inherit='blank', memory_mutation=0.1),          # a mutation with 'blank'
    dict(memory_channels=2, memory_mutation=0.1),                                  # ... or without a mode
    dict(memory_inherit='copy'),                                                   # either argument without memory
    dict(memory_inherit='blank'),
    dict(memory_mutation=0.1),
    dict(memory_channels=0, memory_inherit='copy', memory_mutation=0.1),
], ids=str)
def test_bad_heredity_arguments_raise_value_error(kw):
    with pytest.raises(ValueError, match='memory_inherit|memory_mutation'):
        die.NeuralAutomataAgent(**KW, **kw)


def test_the_arguments_stay_out_of_init_params_until_a_mode_is_set():
    plain = die.NeuralAutomataAgent(**KW, memory_channels=2)
    assert plain.memory_inherit is None and plain.memory_mutation == 0.0
    assert 'memory_inherit' not in plain.init_params and 'memory_mutation' not in plain.init_params
    assert plain.init_params == die.NeuralAutomataAgent(**KW, memory_channels=2, memory_inherit=None, memory_mutation=0.0).init_params
    bare = die.NeuralAutomataAgent(kernel_sizes=(3,))
    assert not {'memory_inherit', 'memory_mutation', 'memory_channels'} & set(bare.init_params)
    assert _architecture(plain)['memory_inherit'] is None


@pytest.mark.parametrize('mode,a', [('blank', 0.0), ('copy', 0.0), ('copy', 0.125)])
def test_save_load_and_unpack_carry_the_rule(mode, a):
    ag = die.NeuralAutomataAgent(**KW, memory_channels=3, memory_inherit=mode, memory_mutation=a)
    assert (ag.memory_inherit, ag.memory_mutation) == (mode, a)
    assert ag.init_params['memory_inherit'] == mode and ag.init_params['memory_mutation'] == a and isinstance(ag.init_params['memory_mutation'], float)
    f = io.BytesIO()
    ag.save(f)
    f.seek(0)
    back = die.NeuralAutomataAgent.load(f)
    assert (back.memory_inherit, back.memory_mutation, back.memory_channels) == (mode, a, 3) and back.init_params == ag.init_params
    assert all(torch.equal(p, q) for p, q in zip(ag.model.parameters(), back.model.parameters()))
    row = torch.nn.utils.parameters_to_vector(ag.model.parameters()).detach()
    twin = BatchedNeuralAutomataAgent.unpack(ag, row)
    assert (twin.memory_inherit, twin.memory_mutation) == (mode, a) and _architecture(twin) == _architecture(ag)
    other = die.NeuralAutomataAgent(**KW, memory_channels=3, memory_inherit='copy', memory_mutation=0.5)
    assert _architecture(other) != _architecture(ag)                 # a population of one rule: from_agents refuses a mix
    # an integer mutation is a number too, saved as the float it means
    assert die.NeuralAutomataAgent(**KW, memory_channels=1, memory_inherit='copy', memory_mutation=1).init_params['memory_mutation'] == 1.0


def test_inherit_memory_refuses_before_it_needs_a_device():
    with pytest.raises(ValueError, match='memory_channels=0'):
        die.NeuralAutomataAgent(kernel_sizes=(3,)).inherit_memory(None)
    with pytest.raises(ValueError, match='memory_inherit=None'):
        die.NeuralAutomataAgent(**KW, memory_channels=2).inherit_memory(None)
    with pytest.raises(ValueError, match='BirthsRecord'):
        die.NeuralAutomataAgent(**KW, memory_channels=2, memory_inherit='copy').inherit_memory(object())
