"""Batched replicas under Dynamics(agents_die=True), CPU side: the lifecycle workspace query, the host-side refusals of both
batched entry points (workspace too small for the dead-slot stash, null arguments) and of BatchedEnv (compat='reference',
a sense mask).  Nothing is launched: the device pointers below are never dereferenced."""
import ctypes as C
import os

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


def test_lifecycle_workspace_query(lib):
    assert 'die_batch_lifecycle_workspace_bytes' in lib.EXPORTS
    assert hasattr(C.CDLL(lib.LIB_PATH), 'die_batch_lifecycle_workspace_bytes')
    q, base = lib.lib.die_batch_lifecycle_workspace_bytes, lib.lib.die_batch_workspace_bytes
    for R, stride in ((1, 1), (1, 1000), (16, 922), (5, 777), (64, 1 << 16), (3, 10**7)):
        got = q(R, stride)
        # the partials of every replica, then a (consumed, cost) float pair per slot of every replica
        assert got >= base(R) + R * stride * 2 * 4, (R, stride)
        assert got % 256 == 0 and got - (base(R) + R * stride * 2 * 4) < 256, (R, stride)
    assert q(4, 100) <= q(4, 101) < q(4, 200) and q(4, 100) < q(5, 100)
    assert base(16) == 16 * base(1)                                  # the old query keeps its meaning
    for bad in ((0, 10), (65, 10), (-1, 10), (4, 0), (4, -3)):
        assert q(*bad) == -1, bad


FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host
R, N, W, H = 4, 10, 96, 96


def _dyn(lib, agents_die=1, has_dead=0):
    return lib.Dynamics(0.1, 0.025, 0.8, lib.DIE_BOUNDARY_WRAP, lib.DIE_COST_LINEAR, 0.02, 0.01, 1, agents_die, has_dead, 0, 0)


def _common(lib):
    m = lib.Medium(W, H, lib.DIE_F32, 2, FAKE, FAKE, FAKE, FAKE + 8, 0, 0, 0, 0, 0, 0, 0, 0, None)
    a = lib.Agents(N, FAKE, FAKE, FAKE, FAKE, None)
    b = lib.Batch(R, 0, W * H, N, 1, (C.c_int64 * 64)(*([N] * 64)))
    return m, a, b


def _forward(lib, ws_bytes, dyn, null=None):
    m, a, b = _common(lib)
    g = lib.GradientAgent(lib.DIE_AGENT_PHYSARUM, 1, 0.01, 4.0, 0.0, 0.1, 0.0, 1e-5, 0.5, 1.5, 0.1, FAKE, FAKE, None, None, None,
                          7, 0, 0, None)
    args = dict(m=C.byref(m), a=C.byref(a), g=C.byref(g), d=C.byref(dyn), b=C.byref(b), results=FAKE, ws=FAKE)
    if null:
        args[null] = None
    return lib.lib.die_forward_env_step_batch(args['m'], args['a'], args['g'], None, args['d'], args['b'], args['results'], args['ws'],
                                              ws_bytes, None)


def _nca(lib, ws_bytes, dyn, null=None):
    m, a, b = _common(lib)
    layers = (lib.NcaLayer * 2)(*[lib.NcaLayer(3, 3, 3, 0, FAKE, 81) for _ in range(2)])
    nca = lib.NcaBatch(2, 0, 1, 1, layers, (C.c_float * 3)(0.01, 0.01, 2.0), 0, FAKE,
                       lib.lib.die_nca_batch_scratch_bytes(W, H, R, 2))
    args = dict(m=C.byref(m), a=C.byref(a), nca=C.byref(nca), d=C.byref(dyn), b=C.byref(b), results=FAKE, ws=FAKE)
    if null:
        args[null] = None
    return lib.lib.die_nca_env_step_batch(args['m'], args['a'], args['nca'], None, args['d'], args['b'], args['results'], args['ws'],
                                          ws_bytes, None)


@pytest.mark.parametrize('entry', [_forward, _nca], ids=['physarum', 'nca'])
@pytest.mark.parametrize('agents_die, has_dead', [(1, 0), (0, 1), (1, 1)])
def test_entry_points_refuse_a_workspace_without_the_stash(lib, entry, agents_die, has_dead):
    old = lib.lib.die_batch_workspace_bytes(R)
    need = lib.lib.die_batch_lifecycle_workspace_bytes(R, N)
    assert need > old
    for ws_bytes in (old, need - 1):
        rc = entry(lib, ws_bytes, _dyn(lib, agents_die, has_dead))
        assert rc != lib.DIE_OK
        assert b'workspace too small' in lib.lib.die_last_error(), ws_bytes


@pytest.mark.parametrize('entry', [_forward, _nca], ids=['physarum', 'nca'])
@pytest.mark.parametrize('null', ['m', 'a', 'd', 'b', 'results', 'ws'])
def test_entry_points_refuse_null_arguments_with_agents_die(lib, entry, null):
    rc = entry(lib, lib.lib.die_batch_lifecycle_workspace_bytes(R, N), _dyn(lib), null=null)
    assert rc != lib.DIE_OK
    assert b'null argument' in lib.lib.die_last_error()


def test_batched_env_refuses_reference_compat_before_any_device_work(lib):
    import die_amd as die
    from die_amd.batch import BatchedEnv
    with pytest.raises(NotImplementedError, match='compat'):
        BatchedEnv((64, 64), die.Dynamics(agents_die=True, compat='reference'), replicas=3, device='cpu')


def test_batched_env_refuses_a_sense_mask_with_agents_die(lib):
    import die_amd as die
    from die_amd.batch import BatchedEnv
    with pytest.raises(NotImplementedError, match='sense_mask'):
        BatchedEnv((64, 64), die.Dynamics(agents_die=True, apply_sense_mask=True), replicas=3, device='cpu')
    with pytest.raises(NotImplementedError, match='diffuse_mode'):
        BatchedEnv((64, 64), die.Dynamics(agents_die=True, diffuse_mode='reflect'), replicas=3, device='cpu')
