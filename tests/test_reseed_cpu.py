"""Reseeded batched worlds, CPU side: die_init_batch and its workspace query are exported and declared, every host-side refusal
of die_init_batch returns DIE_ERR_ARG with its message before any launch, and BatchedEnv(max_agents=...) /
for_population(reseed=...) refuse bad arguments.  Nothing is launched: the device pointers below are never dereferenced."""
import ctypes as C
import os
import re
import types

import pytest
import torch

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


def test_symbols_exported_and_declared(lib):
    so = C.CDLL(lib.LIB_PATH)
    text = open(os.path.join(ROOT, 'include', 'die_hip.h')).read()
    for name in ('die_init_batch', 'die_init_batch_workspace_bytes'):
        assert name in lib.EXPORTS and hasattr(so, name)
        assert re.search(r'\b' + name + r'\(', text), name
    assert lib.lib.die_abi_version() == 24


def test_workspace_query(lib):
    q, scan = lib.lib.die_init_batch_workspace_bytes, lib.lib.die_workspace_bytes
    one = q(96, 96, 1)
    assert one > 0 and one % 256 == 0
    for R in (2, 16, 64):
        assert q(96, 96, R) == R * one
    assert q(96, 96, 4) <= q(192, 96, 4) < q(2048, 2048, 4)
    for bad in ((0, 96, 4), (96, 0, 4), (-1, 96, 4), (96, 96, 0), (96, 96, 65), (96, 96, -2)):
        assert q(*bad) == -1, bad
    assert scan(96, 96, 10) > 0                                      # the old query keeps its meaning


FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host
R, N, W, H = 4, 100, 96, 96


def _args(lib):
    m = lib.Medium(W, H, lib.DIE_F32, 1, FAKE, FAKE, FAKE, FAKE + 8, 0, 0, 0, 0, 0, 0, 0, 0, None)
    a = lib.Agents(N, FAKE, FAKE, FAKE, FAKE, None)
    b = lib.Batch(R, 0, W * H, N, 1, (C.c_int64 * 64)(*([N] * 64)))
    from die_amd.data_init import food_spec_from_seed
    spec = food_spec_from_seed(3, scale=0.5, perlin_octaves=8, threshold=1.0)
    return dict(m=m, a=a, b=b, spec=spec, counts=FAKE, ws=FAKE, ws_bytes=lib.lib.die_init_batch_workspace_bytes(W, H, R), stride=1)


def _call(lib, x, null=None):
    ref = {k: C.byref(x[k]) for k in ('m', 'a', 'b', 'spec')}
    ptr = dict(ref, counts=x['counts'], ws=x['ws'])
    if null:
        ptr[null] = None
    return lib.lib.die_init_batch(ptr['m'], ptr['a'], ptr['b'], 0.1, 3, x['stride'], ptr['spec'], ptr['counts'], ptr['ws'],
                                  x['ws_bytes'], None)


def _refused(lib, x, what, null=None):
    rc = _call(lib, x, null)
    assert rc == -1, what                                    # DIE_ERR_ARG
    msg = lib.lib.die_last_error().decode()
    assert msg.startswith('die_init_batch'), msg
    return msg


@pytest.mark.parametrize('null', ['m', 'a', 'b', 'spec', 'counts', 'ws'])
def test_null_arguments(lib, null):
    assert 'null argument' in _refused(lib, _args(lib), null, null)


def test_refusals(lib):
    cases = []
    x = _args(lib); x['m'].owner = None; cases.append((x, 'bad medium'))
    x = _args(lib); x['m'].W = 0; cases.append((x, 'bad medium'))
    x = _args(lib); x['m'].dtype = 7; cases.append((x, 'bad dtype'))
    x = _args(lib); x['m'].gW = 192; x['m'].gH = 96; cases.append((x, 'whole world'))
    x = _args(lib); x['a'].N = 0; cases.append((x, 'bad agents'))
    x = _args(lib); x['a'].alive = None; cases.append((x, 'bad agents'))
    for reps in (0, -1, 65):
        x = _args(lib); x['b'].replicas = reps; cases.append((x, 'replicas'))
    x = _args(lib); x['b'].plane_stride = W * H - 1; cases.append((x, 'strides smaller'))
    x = _args(lib); x['b'].agent_stride = N - 1; cases.append((x, 'strides smaller'))
    for r, n in ((0, 0), (2, -5), (3, N + 1)):
        x = _args(lib); x['b'].n[r] = n; cases.append((x, f'replica {r} has'))
    x = _args(lib); x['ws_bytes'] -= 1; cases.append((x, 'workspace too small'))
    x = _args(lib); x['spec'].n_waves = 9; cases.append((x, 'n_waves'))
    x = _args(lib); x['spec'].perlin_octaves = -1; cases.append((x, 'perlin_octaves'))
    x = _args(lib); x['spec'].perlin_octaves = 0; cases.append((x, 'wave-mix'))          # one spec cannot serve several seeds
    for x, what in cases:
        assert what in _refused(lib, x, what), what


def test_wave_spec_with_stride_zero_passes_the_host_checks(lib):
    # the one accepted wave-mix form (one world for every replica): refused here only for the fake workspace size
    x = _args(lib)
    x['spec'].perlin_octaves = 0
    x['stride'] = 0
    x['ws_bytes'] = 0
    assert 'workspace too small' in _refused(lib, x, 'ws')


def test_batched_env_refuses_bad_max_agents(lib):
    from die_amd.batch import BatchedEnv
    for bad in (0, -3, 2.5, True, 'all'):
        with pytest.raises(ValueError, match='max_agents'):
            BatchedEnv((96, 96), replicas=2, max_agents=bad)


def _fake_population(fixed):
    from die_amd.batch import BatchedNeuralAutomataAgent
    pop = BatchedNeuralAutomataAgent.__new__(BatchedNeuralAutomataAgent)
    pop.R, pop.P = 10, 162
    pop.parameters = torch.zeros((10, 162))
    pop.env = types.SimpleNamespace(_fixed=fixed)
    return pop


@pytest.mark.parametrize('kind', ['pgpe', 'cmaes'])
def test_for_population_reseed_arguments(lib, kind):
    from die_amd.search import CMAES, PGPE
    s = (PGPE(10, 162, radius_init=1.5, center_learning_rate=0.05, stdev_learning_rate=0.1, device='cpu') if kind == 'pgpe'
         else CMAES(10, 162, stdev_init=0.1, device='cpu'))
    fixed = _fake_population(96 * 96)
    for bad in dict(reseed=1.5), dict(reseed='7'), dict(reseed=True), dict(reseed=3, reseed_stride=-1), dict(reseed=3, reseed_stride=0.5):
        with pytest.raises(ValueError, match='reseed'):
            s.for_population(fixed, 4, **bad)
    with pytest.raises(ValueError, match='max_agents'):
        s.for_population(_fake_population(None), 4, reseed=3)
    assert s.for_population(fixed, 4, reseed=3, reseed_stride=1) is s
    assert (s._reseed, s._reseed_stride) == (3, 1)
    assert s.for_population(_fake_population(None), 4) is s and s._reseed is None
