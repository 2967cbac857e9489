"""PhysarumAgent populations (die_physarum_decode_batch / die_physarum_heading_batch / die_physarum_env_step_batch,
die_amd.batch.BatchedPhysarumPopulation), CPU side: the library exports and the header declares the three entry points with
the ABI unchanged, every bad argument is refused on the host before any launch, the host validity checks of natural rows and
of a ParameterSpace raise as specified, the searchers refuse a natural-mode population, and the float32 model of
tests/physarum_pop_model.py agrees with math.radians and with the ParameterSpace's own host decode.  No kernel is launched
here: the device pointers below are never dereferenced."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import physarum_pop_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ENTRY_POINTS = ('die_physarum_decode_batch', 'die_physarum_heading_batch', 'die_physarum_env_step_batch')


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


def test_entry_points_exported_declared_and_abi_unchanged(lib):
    so = C.CDLL(lib.LIB_PATH)
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'die_hip.h')).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert hasattr(so, name) and name in lib.EXPORTS
        assert re.search(r'\bint\s+' + name + r'\s*\(', text), name
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    # die_physarum_row: six floats, five doubles — one 64-byte row; die_parameter_space: lo[6], hi[6]
    assert C.sizeof(lib.PhysarumRow) == 6 * 4 + 5 * 8 == 64
    assert C.sizeof(lib.ParameterSpace) == 2 * 6 * 4
    assert lib.PhysarumRow.turn_radians.offset == 24 and lib.PhysarumRow.atol.offset == 56
    import die_amd
    from die_amd import batch
    assert die_amd.BatchedPhysarumPopulation is batch.BatchedPhysarumPopulation and die_amd.ParameterSpace is batch.ParameterSpace
    assert batch.BatchedPhysarumPopulation.PARAMETER_NAMES == M.NAMES and batch.BatchedPhysarumPopulation.P == 6


FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host
R, N, W, H = 4, 10, 96, 96


def _refused(lib, fn, *args, match, rc_want=-1):
    rc = getattr(lib.lib, fn)(*args)
    assert rc == rc_want, (fn, rc)
    msg = lib.lib.die_last_error().decode()
    assert match in msg, msg


def _space(lib, lo=(0.001, 0.5, 0.005, 5, 10, 0.0), hi=(0.02, 8, 0.1, 90, 180, 0.5)):
    return lib.ParameterSpace((C.c_float * 6)(*lo), (C.c_float * 6)(*hi))


def test_decode_refusals(lib):
    sp = _space(lib)
    dec = lambda *a, match: _refused(lib, 'die_physarum_decode_batch', *a, None, match=match)
    dec(None, R, 0, None, FAKE, FAKE, match='null rows, table or values')
    dec(FAKE, R, 0, None, None, FAKE, match='null rows, table or values')
    dec(FAKE, R, 0, None, FAKE, None, match='null rows, table or values')
    dec(FAKE, 0, 0, None, FAKE, FAKE, match='replicas 0: in 1..64')
    dec(FAKE, 65, 1, C.byref(sp), FAKE, FAKE, match='replicas 65')
    dec(FAKE, R, 2, C.byref(sp), FAKE, FAKE, match='mode 2')
    dec(FAKE, R, 1, None, FAKE, FAKE, match='unit mode needs a parameter space')


@pytest.mark.parametrize('kw, match', [
    (dict(lo=(0.03, 0.5, 0.005, 5, 10, 0.0)), 'column 0: bounds'),                  # lo > hi
    (dict(hi=(0.02, math.inf, 0.1, 90, 180, 0.5)), 'column 1: bounds'),
    (dict(lo=(0.001, 0.5, math.nan, 5, 10, 0.0)), 'column 2: bounds'),
    (dict(lo=(-0.001, 0.5, 0.005, 5, 10, 0.0)), 'column 0: lower bound'),
    (dict(lo=(0.001, 0.5, -0.005, 5, 10, 0.0)), 'column 2: lower bound'),
    (dict(lo=(0.001, 0.5, 0.005, 0, 10, 0.0)), 'turn_angle must be positive'),
    (dict(lo=(0.001, 0.5, 0.005, 5, -10, 0.0)), 'column 4: lower bound'),
    (dict(lo=(0.001, 0.5, 0.005, 5, 10, -0.1)), 'column 5: lower bound'),
    (dict(hi=(0.02, 8, 0.1, 181, 180, 0.5)), 'column 3: an angle beyond 180'),
    (dict(hi=(0.02, 8, 0.1, 90, 180.5, 0.5)), 'column 4: an angle beyond 180'),
])
def test_decode_refuses_a_bad_parameter_space(lib, kw, match):
    sp = _space(lib, **kw)
    _refused(lib, 'die_physarum_decode_batch', FAKE, R, 1, C.byref(sp), FAKE, FAKE, None, match=match)


def _batch(lib, replicas=R, stride=N, n=None):
    return lib.Batch(replicas, 0, W * (H + 8), stride, 1, (C.c_int64 * 64)(*([N] * 64 if n is None else n)))


def test_heading_refusals(lib):
    hd = lambda *a, match: _refused(lib, 'die_physarum_heading_batch', *a, 7, None, match=match)
    b = _batch(lib)
    hd(None, FAKE, C.byref(b), FAKE, match='null argument')
    hd(FAKE, None, C.byref(b), FAKE, match='null argument')
    hd(FAKE, FAKE, None, FAKE, match='null argument')
    hd(FAKE, FAKE, C.byref(b), None, match='null argument')
    hd(FAKE, FAKE, C.byref(_batch(lib, replicas=0)), FAKE, match='1..64 replicas')
    hd(FAKE, FAKE, C.byref(_batch(lib, replicas=65)), FAKE, match='1..64 replicas')
    hd(FAKE, FAKE, C.byref(_batch(lib, stride=0)), FAKE, match='bad agent stride 0')
    hd(FAKE, FAKE, C.byref(_batch(lib, n=[N, 0, N, N] + [0] * 60)), FAKE, match='replica 1 has 0 agents')
    hd(FAKE, FAKE, C.byref(_batch(lib, n=[N, N, N + 1, N] + [0] * 60)), FAKE, match='replica 2 has 11 agents')


def _step(lib, null=None, ws_bytes=None, rc_want=-1, match='', **kw):
    m = dict(W=W, H=H, dtype=lib.DIE_F32, epoch=2, owner=FAKE, food=FAKE, chem=FAKE, chem_next=FAKE + 8, gW=0, gH=0, ox=0, oy=0,
             own_x0=0, own_y0=0, own_x1=0, own_y1=0, sense_mask=None)
    g = dict(kind=lib.DIE_AGENT_PHYSARUM, normalized_grad=1, scale=0.0, deposit=0.0, inertia=0.0, sense_offset=0.0, noise_scale=0.0,
             grad_clip=1e-5, turn_radians=0.0, sense_radians=0.0, turn_tolerance=0.0, heading_hi=FAKE, heading_lo=FAKE, prev_gx=None,
             prev_gy=None, turn_sign=None, seed=7, step=0, reserved2=0, step_base=None)
    d = dict(rate_feed=0.1, rate_decay_chem=0.025, diffuse_sigma=0.8, boundary=lib.DIE_BOUNDARY_WRAP, cost=lib.DIE_COST_LINEAR,
             cost_w_deposit=0.02, cost_w_dist=0.01, food_infinite=1, agents_die=0, has_dead_slots=0, diffuse_mode=0, staged=0)
    bkw = {}
    for k, v in kw.items():
        (m if k in m else g if k in g else d if k in d else bkw)[k] = v
    ms, gs, ds = lib.Medium(**m), lib.GradientAgent(**g), lib.Dynamics(**d)
    a = lib.Agents(bkw.pop('agents_N', N), FAKE, FAKE, FAKE, FAKE, None)
    b = _batch(lib, **bkw)
    args = dict(m=C.byref(ms), a=C.byref(a), g=C.byref(gs), table=FAKE, d=C.byref(ds), b=C.byref(b), results=FAKE, ws=FAKE)
    if null:
        args[null] = None
    ws_bytes = lib.lib.die_batch_lifecycle_workspace_bytes(R, N) if ws_bytes is None else ws_bytes
    _refused(lib, 'die_physarum_env_step_batch', args['m'], args['a'], args['g'], args['table'], None, args['d'], args['b'],
             args['results'], args['ws'], ws_bytes, None, match=match, rc_want=rc_want)


@pytest.mark.parametrize('null', ['m', 'a', 'g', 'd', 'b', 'results', 'ws'])
def test_step_refuses_null_arguments(lib, null):
    _step(lib, null=null, match='null argument')


def test_step_refusals(lib):
    _step(lib, null='table', match='null parameter table')
    _step(lib, replicas=0, match='1..64 replicas')
    _step(lib, replicas=65, match='1..64 replicas')
    _step(lib, ws_bytes=lib.lib.die_batch_workspace_bytes(R) - 1, match='workspace too small')
    for die, dead in ((1, 0), (0, 1)):              # the dead-slot stash, as die_forward_env_step_batch
        _step(lib, ws_bytes=lib.lib.die_batch_workspace_bytes(R), agents_die=die, has_dead_slots=dead,
              match='workspace too small for dead slots')
    _step(lib, sense_mask=FAKE, match='no sense mask')
    _step(lib, gW=W, gH=H, match='periodic single-tile replicas')
    _step(lib, staged=1, match='periodic single-tile replicas')
    _step(lib, chem_next=FAKE, match='chem_next must be a second plane')
    _step(lib, chem_next=None, match='chem_next must be a second plane')
    _step(lib, agents_N=N + 1, match='strides smaller than a replica')
    _step(lib, H=H + 2, match='H % 4 == 0', rc_want=-3)
    _step(lib, diffuse_sigma=2.0, match='gaussian radius 1..4', rc_want=-3)
    _step(lib, kind=lib.DIE_AGENT_GRADIENT, match='a population of PhysarumAgents')
    _step(lib, inertia=0.5, prev_gx=FAKE, prev_gy=FAKE, match='no inertia, noise, prev_g* or step_base')
    _step(lib, noise_scale=0.1, match='no inertia, noise, prev_g* or step_base')
    _step(lib, step_base=FAKE, match='no inertia, noise, prev_g* or step_base')
    _step(lib, heading_hi=None, match='null device pointer')
    _step(lib, dtype=7, match='bad field dtype 7')
    _step(lib, epoch=0, match='bad medium / agents')
    _step(lib, epoch=32, match='bad medium / agents')
    _step(lib, boundary=lib.DIE_BOUNDARY_NONE, match='not representable', rc_want=-3)
    _step(lib, cost=5, match='bad cost operator 5')
    _step(lib, n=[N, N, 0, N] + [0] * 60, match='replica 2 has 0 agents')
    _step(lib, n=[N, N, N, N + 1] + [0] * 60, match='replica 3 has 11 agents')


# ---------------------------------------------------------------------------------------------------- host checks
GOOD = [0.005, 4.0, 0.03, 30.0, 90.0, 0.1]


def _fake_env(R=3):
    return types.SimpleNamespace(R=R, device=torch.device('cpu'), per_replica=False, Nmax=4, n=[4] * R, W=16, H=16)


@pytest.mark.parametrize('col, bad, what', [
    ('scale', -0.001, '>= 0'), ('sense_offset', -1.0, '>= 0'), ('turn_angle', 0.0, 'in (0, 180]'), ('turn_angle', 180.5, 'in (0, 180]'),
    ('sense_angle', -1.0, 'in [0, 180]'), ('sense_angle', 181.0, 'in [0, 180]'), ('turn_tolerance', -0.1, '>= 0'),
    ('deposit', math.nan, 'not finite'), ('scale', math.inf, 'not finite'),
])
def test_natural_rows_are_checked_on_the_host_naming_row_and_column(lib, col, bad, what):
    from die_amd.batch import BatchedPhysarumPopulation
    rows = np.tile(f32(GOOD), (3, 1))
    rows[1, M.NAMES.index(col)] = bad
    with pytest.raises(ValueError, match=re.escape(f'row 1, column {col}') + '.*' + re.escape(what)):
        BatchedPhysarumPopulation(_fake_env(), rows)


def test_population_argument_refusals(lib):
    from die_amd.batch import BatchedPhysarumPopulation, ParameterSpace
    rows = np.tile(f32(GOOD), (3, 1))
    with pytest.raises(ValueError, match='not both'):
        BatchedPhysarumPopulation(_fake_env(), rows, parameters=rows)
    with pytest.raises(ValueError, match='space= goes with parameters='):
        BatchedPhysarumPopulation(_fake_env(), rows, space=ParameterSpace())
    with pytest.raises(TypeError, match='a ParameterSpace'):
        BatchedPhysarumPopulation(_fake_env(), parameters=rows, space=(0, 1))
    with pytest.raises(ValueError, match=r'values of shape \(2, 6\): \(3, 6\) expected'):
        BatchedPhysarumPopulation(_fake_env(), rows[:2])
    with pytest.raises(ValueError, match=r'parameters of shape \(3, 5\)'):
        BatchedPhysarumPopulation(_fake_env(), parameters=rows[:, :5])


def test_parameter_space_checks(lib):
    from die_amd.batch import ParameterSpace
    sp = ParameterSpace()
    assert sp.lo.dtype == f32 and sp.hi.dtype == f32
    assert np.all(sp.lo < f32(GOOD)) and np.all(f32(GOOD) < sp.hi)                 # brackets the reference's defaults
    with pytest.raises(ValueError, match='6 values each'):
        ParameterSpace(lo=(0, 1), hi=(1, 2))
    with pytest.raises(ValueError, match='column scale: bounds'):
        ParameterSpace(lo=(0.03, 0.5, 0.005, 5, 10, 0.0))
    with pytest.raises(ValueError, match='column deposit: bounds'):
        ParameterSpace(hi=(0.02, math.inf, 0.1, 90, 180, 0.5))
    with pytest.raises(ValueError, match='row lo, column turn_angle'):
        ParameterSpace(lo=(0.001, 0.5, 0.005, 0, 10, 0.0))
    with pytest.raises(ValueError, match='row hi, column turn_angle'):
        ParameterSpace(hi=(0.02, 8, 0.1, 181, 180, 0.5))
    with pytest.raises(ValueError, match='row lo, column sense_offset'):
        ParameterSpace(lo=(0.001, 0.5, -0.005, 5, 10, 0.0))
    with pytest.raises(ValueError, match='row hi, column sense_angle'):
        ParameterSpace(hi=(0.02, 8, 0.1, 90, 180.5, 0.5))
    with pytest.raises(ValueError, match='row lo, column turn_tolerance'):
        ParameterSpace(lo=(0.001, 0.5, 0.005, 5, 10, -0.5))
    one = ParameterSpace(lo=GOOD, hi=GOOD)                                        # a point is a space
    assert np.array_equal(one.decode(np.random.RandomState(0).randn(4, 6)), np.tile(f32(GOOD), (4, 1)))
    # the library's check of the same space agrees
    s = sp._struct()
    assert list(s.lo) == sp.lo.tolist() and list(s.hi) == sp.hi.tolist()


@pytest.mark.parametrize('searcher', ['pgpe', 'cmaes'])
def test_for_population_refuses_natural_mode(lib, searcher):
    from die_amd.batch import BatchedPhysarumPopulation
    from die_amd.search import CMAES, PGPE
    pop = object.__new__(BatchedPhysarumPopulation)
    pop.R, pop.natural, pop.env = 6, True, _fake_env(6)
    pop.parameters = torch.zeros((6, 6), dtype=torch.float32)
    s = (PGPE(6, 6, radius_init=0.3, center_learning_rate=0.1, stdev_learning_rate=0.1, device='cpu') if searcher == 'pgpe'
         else CMAES(6, 6, stdev_init=0.2, device='cpu'))
    with pytest.raises(ValueError, match='natural rows: one step size does not suit six units'):
        s.for_population(pop, epoch_iters=5)
    with pytest.raises(TypeError, match='BatchedPhysarumPopulation'):
        s.for_population(object(), epoch_iters=5)
    pop.natural = False                             # unit mode binds (nothing is launched by binding)
    pop.reset = lambda: None
    assert s.for_population(pop, epoch_iters=5) is s and s._pop_reset is pop.reset


# ---------------------------------------------------------------------------------------------------- the model
def test_model_natural_rows_agree_with_math_radians():
    rng = np.random.RandomState(1)
    rows = np.stack([rng.uniform(0, 0.05, 40), rng.uniform(-2, 9, 40), rng.uniform(0, 0.2, 40), rng.uniform(0.1, 180, 40),
                     rng.uniform(0, 180, 40), rng.uniform(0, 0.6, 40)], axis=1).astype(f32)
    rows[0] = GOOD
    rows[1, 3:] = (180.0, 180.0, 0.0)
    rows[2, 4] = 0.0
    values, table = M.decode(rows)
    assert values.dtype == f32 and np.array_equal(values, rows)
    for v, t in zip(rows, table):
        assert t['turn_radians'] == math.radians(float(v[3])) and t['sense_radians'] == math.radians(float(v[4]))
        assert t['turn_tolerance'] == float(v[5]) and t['atol'] == math.radians(float(v[3])) * float(v[5])
        assert (t['scale'], t['deposit'], t['sense_offset']) == (v[0], v[1], v[2])
        # x_turn is the last double np.isclose(0, x, rtol=1e-2, atol) accepts
        x = t['x_turn']
        assert x >= 0 and np.isclose(0.0, x, rtol=1e-2, atol=t['atol']) and not np.isclose(0.0, np.nextafter(x, np.inf), rtol=1e-2, atol=t['atol'])
        assert t['c_turn'] == f32(math.cos(x))
        assert t['c_sense'] == (f32(-2.0) if t['sense_radians'] >= math.pi else f32(math.cos(t['sense_radians'])))
    assert table[0]['turn_radians'] == math.radians(30) and table[0]['sense_radians'] == math.radians(90)
    assert table[1]['c_sense'] == f32(-2.0) and table[1]['x_turn'] == 0.0 and table[1]['c_turn'] == f32(1.0)   # 180 degrees: every angle is seen
    assert table[2]['c_sense'] == f32(1.0)


def test_model_unit_rows_follow_the_host_decode_and_stay_valid():
    from die_amd.batch import ParameterSpace, _check_physarum_values
    sp = ParameterSpace()
    rng = np.random.RandomState(2)
    u = rng.uniform(-0.5, 1.5, (64, 6)).astype(f32)
    u[0], u[1], u[2, 0], u[3] = 0.0, 1.0, np.nan, (-np.inf, np.inf, -1e30, 1e30, -0.0, 1.0000001)
    values = M.decode_values(u, sp.lo, sp.hi)
    assert values.dtype == f32 and np.array_equal(values, sp.decode(u))
    assert np.array_equal(values[0], sp.lo) and np.array_equal(values[2, :1], sp.lo[:1])
    assert np.array_equal(values[3], [sp.lo[0], values[1, 1], sp.lo[2], values[1, 3], sp.lo[4], values[1, 5]])
    assert np.all(values >= sp.lo) and np.all(values <= values[1])
    _check_physarum_values(values, range(64))
    # by hand, each operation rounded to float32
    c = f32(0.3)
    assert values.dtype == f32 and M.decode_values([[c] * 6], sp.lo, sp.hi)[0, 3] == f32(f32(5) + f32(f32(f32(90) - f32(5)) * c))
    assert np.allclose(sp.encode(sp.decode(u[4:])), np.clip(u[4:], 0, 1), atol=1e-5)
