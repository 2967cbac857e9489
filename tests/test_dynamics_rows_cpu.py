"""Per-replica Dynamics on batched replicas, CPU side: the die_dynamics_row layout, die_dynamics_rows (taps, keep, refusals), the
host-side refusals of the *_rows step entry points and of die_food_flow_batch_masked (fake pointers: every call is refused before
any launch), the validation of `BatchedEnv(dynamics=[...])` and the layout of `episode_dynamics`.  No kernel is launched here."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


NEW_SYMBOLS = ('die_dynamics_rows', 'die_forward_env_step_batch_rows', 'die_physarum_env_step_batch_rows', 'die_nca_env_step_batch_rows',
               'die_food_flow_batch_masked')


def test_struct_and_symbols(lib):
    R = lib.DynamicsRow
    assert C.sizeof(R) == 64                                      # one scalar load per workgroup
    assert [(n, getattr(R, n).offset) for n, _ in R._fields_] == [('rate_feed', 0), ('keep', 4), ('food_infinite', 8), ('radius', 12),
                                                                  ('w', 16), ('reserved', 52)]
    assert R.w.size == 36 and R.reserved.size == 12
    so = C.CDLL(lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(so, name), name
        assert name in lib.EXPORTS, name
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    assert C.sizeof(lib.Dynamics) == 48 and C.sizeof(lib.Batch) == 32 + 8 * 64      # added within ABI 24: nothing existing moved


def _dyn(lib, sigma=0.5, decay=0.1, feed=0.1, boundary=0, cost=0, infinite=0, die=0, dead=0, mode=0, staged=0, w_dep=0.02, w_dist=0.01):
    return lib.Dynamics(feed, decay, sigma, boundary, cost, w_dep, w_dist, infinite, die, dead, mode, staged)


def _rows(lib, dyns, W=64, H=48, n=None):
    n = len(dyns) if n is None else n
    arr = (lib.Dynamics * max(len(dyns), 1))(*dyns)
    out = (lib.DynamicsRow * 64)()
    for row in out:
        row.radius = -7                                           # a refused call must leave this
    rc = lib.lib.die_dynamics_rows(arr, n, W, H, out)
    return rc, out


@pytest.mark.parametrize('sigma', [0.3, 0.5, 0.8, 1.1])
def test_rows_hold_the_library_taps(lib, sigma):
    gaussian_taps = getattr(C.CDLL(lib.LIB_PATH), '_Z17die_gaussian_tapsfPd')      # int die_gaussian_taps(float, double*), C++ linkage
    gaussian_taps.restype, gaussian_taps.argtypes = C.c_int, [C.c_float, C.POINTER(C.c_double)]
    decay, feed = 0.025, 0.07
    rc, out = _rows(lib, [_dyn(lib, sigma=sigma, decay=decay, feed=feed, infinite=1), _dyn(lib)])
    assert rc == 0, lib.lib.die_last_error()
    row = out[0]
    radius = int(4.0 * float(np.float32(sigma)) + 0.5)
    assert row.radius == radius and 1 <= radius <= 4
    buf = (C.c_double * 17)()
    assert gaussian_taps(sigma, buf) == radius
    w = np.array(buf[:2 * radius + 1])
    assert abs(w.sum() - 1.0) < 1e-12 and np.array_equal(w, w[::-1])
    assert np.array_equal(np.array(row.w[:2 * radius + 1], dtype=np.float32), w.astype(np.float32))
    assert all(v == 0.0 for v in row.w[2 * radius + 1:]) and all(v == 0.0 for v in row.reserved)
    assert np.float32(row.keep) == np.float32(1.0 - float(np.float32(decay)))      # the float of the double expression
    assert np.float32(row.rate_feed) == np.float32(feed) and row.food_infinite == 1
    assert out[1].radius == 2 and out[1].food_infinite == 0 and np.float32(out[1].keep) == np.float32(1.0 - float(np.float32(0.1)))


@pytest.mark.parametrize('case, kw, rc_want, needle', [
    ('no row', dict(n=0), -1, b'0 rows, 1..64 expected'),
    ('65 rows', dict(n=65), -1, b'65 rows, 1..64 expected'),
    ('radius 0', dict(bad=dict(sigma=0.1)), -3, b'gaussian radius 1..4'),
    ('radius 5', dict(bad=dict(sigma=1.2)), -3, b'gaussian radius 1..4'),
    ('H = 50', dict(H=50), -3, b'H % 4 == 0'),
    ('boundary', dict(bad=dict(boundary=1)), -1, b'row 2 disagrees with row 0 in boundary'),
    ('cost', dict(bad=dict(cost=1)), -1, b'row 2 disagrees with row 0 in cost'),
    ('cost weights', dict(bad=dict(w_dist=0.5)), -1, b'row 2 disagrees with row 0 in the cost weights'),
    ('agents_die', dict(bad=dict(die=1)), -1, b'row 2 disagrees with row 0 in agents_die'),
    ('has_dead_slots', dict(bad=dict(dead=1)), -1, b'row 2 disagrees with row 0 in has_dead_slots'),
    ('diffuse_mode', dict(bad=dict(mode=1)), -1, b'only WRAP'),
    ('staged', dict(bad=dict(staged=1)), -1, b'staged'),
])
def test_rows_refusals_write_nothing(lib, case, kw, rc_want, needle):
    dyns = [_dyn(lib), _dyn(lib, sigma=0.8), _dyn(lib, **kw.get('bad', {})), _dyn(lib)]
    rc, out = _rows(lib, dyns, H=kw.get('H', 48), n=kw.get('n'))
    assert rc == rc_want, (case, rc, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error(), (case, lib.lib.die_last_error())
    assert all(row.radius == -7 for row in out), case            # refused before anything is written


def test_rows_null_arguments(lib):
    out = (lib.DynamicsRow * 2)()
    assert lib.lib.die_dynamics_rows(None, 2, 64, 48, out) == -1 and b'null argument' in lib.lib.die_last_error()
    assert lib.lib.die_dynamics_rows((lib.Dynamics * 2)(_dyn(lib), _dyn(lib)), 2, 64, 48, None) == -1
    assert b'null argument' in lib.lib.die_last_error()


FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host


def _step_structs(lib, W=64, H=48, replicas=4, N=10):
    L = lib
    m = L.Medium(W, H, L.DIE_F32, 2, FAKE, FAKE, FAKE, FAKE + 8, 0, 0, 0, 0, 0, 0, 0, 0, None)
    a = L.Agents(N, FAKE, FAKE, FAKE, FAKE, None)
    d = _dyn(lib)
    b = L.Batch(replicas, 0, W * H, N, 1, (C.c_int64 * 64)(*([N] * 64)))
    return m, a, d, b


def _host_rows(lib, n=4):
    rc, out = _rows(lib, [_dyn(lib)] * n)
    assert rc == 0
    return out


def _forward(lib, *, null=None, replicas=4, rows=FAKE, host=True):
    L = lib
    m, a, d, b = _step_structs(lib, replicas=replicas)
    g = L.GradientAgent(L.DIE_AGENT_PHYSARUM, 1, 0.005, 4.0, 0.0, 0.03, 0.0, 1e-5, 0.5, 1.5, 0.1, FAKE, FAKE, None, None, None, 0, 0, 0, None)
    ws = int(L.lib.die_batch_workspace_bytes(4))
    return L.lib.die_forward_env_step_batch_rows(None if null == 'm' else C.byref(m), C.byref(a), C.byref(g), None,
                                                 None if null == 'd' else C.byref(d), C.byref(b), FAKE, FAKE, ws, rows,
                                                 _host_rows(lib) if host else None, None)


def _physarum(lib, *, null=None, replicas=4, rows=FAKE, host=True):
    L = lib
    m, a, d, b = _step_structs(lib, replicas=replicas)
    g = L.GradientAgent(L.DIE_AGENT_PHYSARUM, 1, 0.0, 0.0, 0.0, 0.0, 0.0, 1e-5, 0.0, 0.0, 0.0, FAKE, FAKE, None, None, None, 0, 0, 0, None)
    ws = int(L.lib.die_batch_workspace_bytes(4))
    return L.lib.die_physarum_env_step_batch_rows(None if null == 'm' else C.byref(m), C.byref(a), C.byref(g), None if null == 'table' else FAKE,
                                                  None, None if null == 'd' else C.byref(d), C.byref(b), FAKE, FAKE, ws, rows,
                                                  _host_rows(lib) if host else None, None)


def _nca(lib, *, null=None, replicas=4, rows=FAKE, host=True):
    L = lib
    m, a, d, b = _step_structs(lib, replicas=replicas)
    m.epoch = 2
    layers = (L.NcaLayer * 1)(L.NcaLayer(3, 3, 3, 0, FAKE, 81))
    scratch = int(L.lib.die_nca_batch_scratch_bytes(64, 48, 4, 1))
    nca = L.NcaBatch(1, 0, 1, 1, layers, (C.c_float * 3)(0.01, 0.01, 2.0), 0, FAKE, scratch)
    ws = int(L.lib.die_batch_workspace_bytes(4))
    return L.lib.die_nca_env_step_batch_rows(None if null == 'm' else C.byref(m), C.byref(a), None if null == 'nca' else C.byref(nca), None,
                                             None if null == 'd' else C.byref(d), C.byref(b), FAKE, FAKE, ws, None, rows,
                                             _host_rows(lib) if host else None, None)


@pytest.mark.parametrize('call, who', [(_forward, b'die_forward_env_step_batch_rows'), (_physarum, b'die_physarum_env_step_batch_rows'),
                                       (_nca, b'die_nca_env_step_batch_rows')])
def test_step_entry_points_refuse_on_the_host(lib, call, who):
    for null in ('m', 'd'):
        assert call(lib, null=null) == -1
        assert lib.lib.die_last_error() == who + b': null argument'
    for replicas in (0, 65):
        assert call(lib, replicas=replicas) == -1
        assert lib.lib.die_last_error() == who + b': 1..64 replicas'
    # every check of the parent passes with these arguments; then the table is asked for
    assert call(lib, rows=None) == -1
    assert who in lib.lib.die_last_error() and b'rows == NULL' in lib.lib.die_last_error(), lib.lib.die_last_error()
    assert call(lib, host=False) == -1
    assert who in lib.lib.die_last_error() and b'rows_host == NULL' in lib.lib.die_last_error(), lib.lib.die_last_error()


def test_physarum_rows_null_table_is_the_parents_refusal(lib):
    assert _physarum(lib, null='table') == -1
    assert lib.lib.die_last_error() == b'die_physarum_env_step_batch_rows: null parameter table'


def _masked(lib, *, mask=0xF, replicas=4, null=None, H=48, kind=None):
    L = lib
    m = L.Medium(64, H, L.DIE_F32, 1, FAKE, FAKE, FAKE, FAKE + 8, 0, 0, 0, 0, 0, 0, 0, 0, None)
    if null == 'food':
        m.food = None
    b = L.Batch(replicas, 0, 64 * H, 10, 1, (C.c_int64 * 64)(*([10] * 64)))
    return L.lib.die_food_flow_batch_masked(None if null == 'm' else C.byref(m), None if null == 'b' else C.byref(b),
                                            L.DIE_FLOW_WAVE if kind is None else kind, 0.25, 0.5, 0.5, 0, 0, mask, None)


@pytest.mark.parametrize('case, kw, needle', [
    ('null medium', dict(null='m'), b'die_food_flow_batch_masked: null argument'),
    ('null batch', dict(null='b'), b'die_food_flow_batch_masked: null argument'),
    ('null food plane', dict(null='food'), b'die_food_flow_batch_masked: null argument'),
    ('no replica', dict(replicas=0), b'die_food_flow_batch_masked: 0 replicas, 1..64 expected'),
    ('65 replicas', dict(replicas=65), b'die_food_flow_batch_masked: 65 replicas, 1..64 expected'),
    ('kind 0', dict(kind=0), b'unknown flow kind 0'),
    ('H % 4', dict(H=46), b'H % 4'),
    ('a bit past the replicas', dict(mask=0x10), b'bits beyond the 4 replicas'),
])
def test_masked_flow_refused_before_launch(lib, case, kw, needle):
    assert _masked(lib, **kw) == -1, case
    assert needle in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


def test_masked_flow_empty_mask_launches_nothing(lib):
    assert _masked(lib, mask=0) == 0                              # (fake pointers: a launch would have failed)


# ---- BatchedEnv(dynamics=[...]) validation: everything is refused before the device is touched -----------------------------------
def _three(die, size=(64, 48), **kw):
    op = die.WaveSequence(size, dt=0.01).get_flow_operator(scale=0.5, decay=0.5)
    return [die.Dynamics(food_infinite=True, **kw), die.Dynamics(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8, **kw),
            die.Dynamics(food_infinite=False, op_food_flow=op, **kw)]


def test_constructor_refuses_a_list_of_the_wrong_length(lib):
    import die_amd as die
    from die_amd.batch import BatchedEnv
    with pytest.raises(ValueError, match='3 dynamics for 4 replicas'):
        BatchedEnv((64, 48), _three(die), replicas=4, device='cpu')
    with pytest.raises(TypeError, match=r'dynamics\[1\]'):
        BatchedEnv((64, 48), [die.Dynamics(), 'st-perlin'], replicas=2, device='cpu')


@pytest.mark.parametrize('field, value', [
    ('boundary', 'limit'), ('op_action_cost', 'zero'), ('strict_cost', False), ('agents_die', True), ('compat', 'reference'),
    ('init_agent_ratio', 0.2), ('apply_sense_mask', True), ('diffuse_mode', 'nearest'),
])
def test_constructor_names_the_first_replica_that_disagrees(lib, field, value):
    import dataclasses

    import die_amd as die
    from die_amd.batch import BatchedEnv
    from die_amd.env import BoundaryCondition
    if field == 'boundary':
        value = next(b for b in BoundaryCondition if b != BoundaryCondition.wrap)
    if field == 'op_action_cost':
        value = lambda *a, **k: 0.0                                # noqa: E731
    dyn = _three(die) * 2
    dyn[4] = dataclasses.replace(dyn[4], **{field: value})
    dyn[5] = dataclasses.replace(dyn[5], **{field: value})
    with pytest.raises(ValueError, match=rf'replica 4: dynamics\[4\]\.{field}'):
        BatchedEnv((64, 48), dyn, replicas=6, device='cpu')


def test_constructor_keeps_todays_refusals(lib):
    import die_amd as die
    from die_amd.batch import BatchedEnv
    with pytest.raises(NotImplementedError, match='apply_sense_mask'):
        BatchedEnv((64, 48), _three(die, apply_sense_mask=True), replicas=3, device='cpu')
    with pytest.raises(NotImplementedError, match='diffuse_mode'):
        BatchedEnv((64, 48), _three(die, diffuse_mode='nearest'), replicas=3, device='cpu')
    with pytest.raises(ValueError, match='1..64 replicas'):
        BatchedEnv((64, 48), [die.Dynamics()] * 65, replicas=65, device='cpu')


def test_constructor_refuses_a_second_flow_operator(lib):
    import die_amd as die
    from die_amd.batch import BatchedEnv
    dyn = _three(die) + _three(die)                               # two operator objects over equal sequences: still two counters
    with pytest.raises(ValueError, match=r'replica 5: dynamics\[5\]\.op_food_flow is a second food-flow operator'):
        BatchedEnv((64, 48), dyn, replicas=6, device='cpu')


def test_shared_dynamics_and_flow_mask(lib):
    import die_amd as die
    from die_amd.batch import _shared_dynamics
    from die_amd.env import _identity_food_flow
    three = _three(die)
    shared, dyn, mask = _shared_dynamics(three * 2, 6)
    assert mask == 0b100100 and dyn == three * 2
    assert shared.op_food_flow is three[2].op_food_flow and shared.rate_decay_chem == three[0].rate_decay_chem
    shared, _, mask = _shared_dynamics(three[:2], 2)
    assert mask == 0 and shared.op_food_flow is _identity_food_flow


def test_episode_dynamics_layout(lib):
    import die_amd as die
    from die_amd.batch import episode_dynamics, episode_seeds
    three = _three(die)
    dyn = episode_dynamics(three, 4)
    assert len(dyn) == 12 == len(episode_seeds(0, 4, 3))
    for c in range(4):
        for e in range(3):
            assert dyn[c * 3 + e] is three[e]                     # candidate-major: replica c·E + e lives under dynamics[e]
    assert episode_dynamics(three[:1], 2) == [three[0]] * 2
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match='candidates'):
            episode_dynamics(three, bad)
    with pytest.raises(ValueError, match='sequence of Dynamics'):
        episode_dynamics([], 2)
    with pytest.raises(ValueError, match='sequence of Dynamics'):
        episode_dynamics(['st-perlin'], 2)
