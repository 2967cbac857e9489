"""Dynamics(agents_born=True), CPU side: the rules as tests/births_model.py states them (matching order, the cap, the exact share,
both boundaries, the displacement's range), the workspace query and the host-side refusals of both entry points, and the
refusals of the Python layer that need no device.  Nothing is launched: the device pointers below are never dereferenced."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import births_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the model's rules
def _world(alive, food, seed=0):
    rs = np.random.RandomState(seed)
    n = len(alive)
    return (rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32), rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32),
            np.array(alive, dtype=np.uint8), np.array(food, dtype=np.float32))


def test_matching_is_by_slot_order():
    #        0    1    2    3    4    5    6    7
    alive = [1,   0,   1,   1,   0,   1,   0,   1]
    food = [0.9, 0.0, 0.3, 0.8, 0.0, 0.7, 0.0, 0.5]            # 0.5 is not above the threshold; 0.3 is poor
    parents, free = M.match(alive, food, 0.5)
    assert parents.tolist() == [0, 3, 5] and free.tolist() == [1, 4, 6]
    x, y, a, f = _world(alive, food)
    nx, ny, na, nf, born = M.births(x, y, a, f, world_seed=3, world_step=0)
    assert born == 3 and na.tolist() == [1] * 8
    assert nf.tolist() == [np.float32(v) for v in (0.45, 0.45, 0.3, 0.4, 0.4, 0.35, 0.35, 0.5)]
    for s in (0, 2, 3, 5, 7):                                   # nobody who was alive moves
        assert nx[s] == x[s] and ny[s] == y[s]


def test_cap_when_free_slots_run_out():
    alive = [1, 1, 0, 1, 1]
    food = [0.9, 0.9, 0.0, 0.9, 0.9]
    parents, free = M.match(alive, food, 0.5)
    assert parents.tolist() == [0] and free.tolist() == [2]    # parents of rank >= #free do not breed …
    *_, nf, born = M.births(*_world(alive, food), world_seed=1, world_step=5)
    assert born == 1 and nf.tolist() == [np.float32(0.45), np.float32(0.9), np.float32(0.45), np.float32(0.9), np.float32(0.9)]   # … and keep their food
    parents, free = M.match([1, 0, 0, 0], [0.9, 0, 0, 0], 0.5)
    assert parents.tolist() == [0] and free.tolist() == [1]    # and the reverse: the first free slots are taken


@pytest.mark.parametrize('alive, food', [([1, 1, 1], [0.9, 0.9, 0.9]),          # no free slot
                                         ([1, 0, 1], [0.5, 0.0, 0.2]),          # no parent
                                         ([0, 0, 0], [0.0, 0.0, 0.0])])         # nobody
def test_nothing_happens_without_a_pair(alive, food):
    x, y, a, f = _world(alive, food)
    nx, ny, na, nf, born = M.births(x, y, a, f, world_seed=9, world_step=2)
    assert born == 0
    assert np.array_equal(nx, x) and np.array_equal(ny, y) and np.array_equal(na, a) and np.array_equal(nf.view(np.uint32), f.view(np.uint32))


def test_a_pair_conserves_food_to_the_bit():
    rs = np.random.RandomState(4)
    n = 4096
    food = rs.uniform(0.5, 40.0, n).astype(np.float32)
    food[::7] = np.float32(0.5) + np.spacing(np.float32(0.5))   # the smallest parent
    alive = np.ones(2 * n, np.uint8)
    alive[n:] = 0
    x, y, a, f = _world(alive, np.concatenate([food, np.zeros(n, np.float32)]))
    *_, nf, born = M.births(x, y, a, f, world_seed=2, world_step=1)
    assert born == n
    assert np.array_equal((nf[:n] + nf[n:]).view(np.uint32), food.view(np.uint32))      # parent + child == before, exactly
    assert np.array_equal(nf[n:], np.float32(0.5) * food)


def test_displacement_is_within_the_spread_and_uses_the_parents_draw():
    parents = np.arange(0, 200000, 3)
    for spread in (0.02, 0.5, 1e-6, 0.0):
        q = M.spread_q(spread)
        ox, oy = M.displacement(11, 7, parents, spread)
        assert ox.min() >= -q and ox.max() < max(q, 1) and oy.min() >= -q and oy.max() < max(q, 1)
        if spread >= 0.02:
            assert ox.min() < -0.99 * q and ox.max() > 0.99 * q and abs(ox.mean()) < 0.02 * q      # it fills the range, about 0
    a = M.displacement(11, 7, parents, 0.02)
    assert not np.array_equal(a[0], M.displacement(11, 8, parents, 0.02)[0])        # the step, the seed and the slot all enter
    assert not np.array_equal(a[0], M.displacement(12, 7, parents, 0.02)[0])
    assert np.array_equal(a[0][1:2], M.displacement(11, 7, parents[1:2], 0.02)[0])
    assert not np.array_equal(a[0], a[1])


def test_limit_clamps_and_wrap_wraps():
    top = 2 ** 32 - 1
    X = np.array([0, 5, top, top - 5, 2 ** 31], dtype=np.uint32)
    off = np.array([-10, -10, 10, 10, -10], dtype=np.int64)
    assert M.place(X, off, M.LIMIT).tolist() == [0, 0, top, top, 2 ** 31 - 10]
    assert M.place(X, off, M.WRAP).tolist() == [2 ** 32 - 10, 2 ** 32 - 5, 9, 4, 2 ** 31 - 10]
    # through the whole pass: parents on the edges, the largest spread
    n = 64
    alive = np.r_[np.ones(n, np.uint8), np.zeros(n, np.uint8)]
    food = np.r_[np.full(n, 0.9, np.float32), np.zeros(n, np.float32)]
    x = np.r_[np.zeros(n // 2, np.uint32), np.full(n // 2, top, np.uint32), np.zeros(n, np.uint32)]
    ox, _ = M.displacement(5, 0, np.arange(n), 0.5)
    lim, *_ = M.births(x, x, alive, food, world_seed=5, world_step=0, born_spread=0.5, boundary=M.LIMIT)
    wrp, *_ = M.births(x, x, alive, food, world_seed=5, world_step=0, born_spread=0.5, boundary=M.WRAP)
    out = (x[:n].astype(np.int64) + ox < 0) | (x[:n].astype(np.int64) + ox > top)
    assert out.any() and (~out).any()
    assert np.all(np.isin(lim[n:][out], [0, top])) and np.array_equal(lim[n:][~out], wrp[n:][~out])
    assert np.array_equal(wrp[n:], ((x[:n].astype(np.int64) + ox) % 2 ** 32).astype(np.uint32))


# ---------------------------------------------------------------- the library's host side
@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


def test_symbols_and_workspace_query(lib):
    so = C.CDLL(lib.LIB_PATH)
    for name in ('die_agent_births', 'die_agent_births_batch', 'die_births_workspace_bytes'):
        assert hasattr(so, name) and name in lib.EXPORTS, name
    assert C.sizeof(lib.Births) == 4 + 4 + 8 + 4 + 4
    q = lib.lib.die_births_workspace_bytes
    for R, stride in ((1, 1), (1, 641), (5, 777), (64, 1 << 16), (3, 10 ** 7)):
        got = q(R, stride)
        assert got % 256 == 0 and got >= R * stride * 4, (R, stride)          # one word per slot: both rank lists share it
        assert got < R * (stride * 4 + 8192), (R, stride)
    assert q(4, 100) < q(4, 300) and q(4, 100) < q(5, 100)
    for bad in ((0, 10), (65, 10), (-1, 10), (4, 0), (4, -3), (1, 1 << 27)):
        assert q(*bad) == -1, bad


FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host


def _births(lib, spread=0.02, boundary=0, threshold=0.5):
    return lib.Births(threshold, boundary, spread, 0, 0)


def test_entry_points_refuse_bad_arguments_before_any_launch(lib):
    L = lib.lib
    N, R = 100, 3
    a = lib.Agents(N, FAKE, FAKE, FAKE, FAKE, None)
    need = L.die_births_workspace_bytes(1, N)
    p = _births(lib)
    call = lambda a=a, p=p, ws=FAKE, n=need: L.die_agent_births(C.byref(a) if a else None, C.byref(p) if p else None, 7, None, ws, n, None)
    assert call(n=need - 1) == -1 and b'workspace too small' in L.die_last_error()
    assert call(n=0) == -1
    assert call(a=None) == -1 and b'null argument' in L.die_last_error()
    assert call(p=None) == -1 and call(ws=None) == -1
    assert call(a=lib.Agents(0, FAKE, FAKE, FAKE, FAKE, None)) == -1
    assert call(a=lib.Agents(N, FAKE, None, FAKE, FAKE, None)) == -1 and b'bad agents' in L.die_last_error()
    assert call(a=lib.Agents(N, FAKE, FAKE, FAKE, FAKE, FAKE)) == -3 and b'slot order' in L.die_last_error()
    assert call(p=_births(lib, boundary=2)) == -3
    assert call(p=_births(lib, spread=0.6)) == -1 and b'born_spread' in L.die_last_error()
    assert call(p=_births(lib, spread=-0.1)) == -1
    assert call(p=_births(lib, threshold=float('nan'))) == -1
    # the batch: replicas out of range, n > stride, a short workspace
    seeds = (C.c_uint64 * R)(1, 2, 3)
    def batch(replicas=R, n=(100, 37, 64), stride=N, ws_bytes=None, seeds=seeds):
        b = lib.Batch(replicas, 0, 0, stride, 0, (C.c_int64 * 64)(*n))
        ws_bytes = L.die_births_workspace_bytes(R, N) if ws_bytes is None else ws_bytes
        return L.die_agent_births_batch(C.byref(a), C.byref(b), C.byref(p), seeds, FAKE, FAKE, ws_bytes, None)
    assert batch(replicas=0) == -1 and batch(replicas=65) == -1 and b'replicas' in L.die_last_error()
    assert batch(n=(100, 101, 64)) == -1 and b'replica 1' in L.die_last_error()
    assert batch(n=(100, 0, 64)) == -1
    assert batch(ws_bytes=L.die_births_workspace_bytes(R, N) - 1) == -1 and b'workspace too small' in L.die_last_error()
    assert batch(ws_bytes=L.die_births_workspace_bytes(1, N)) == -1
    assert batch(stride=0) == -1
    assert batch(seeds=None) == -1


# ---------------------------------------------------------------- the Python layer's refusals that need no device
def test_dynamics_has_the_birth_fields():
    import die_amd as die
    d = die.Dynamics()
    assert d.agents_born is False and d.born_threshold == 0.5 and d.born_spread == 0.02


def test_batched_env_refusals_before_any_device_work(lib):
    import die_amd as die
    from die_amd.batch import BatchedEnv, _MUST_AGREE
    assert 'born_threshold' in _MUST_AGREE and 'born_spread' in _MUST_AGREE and 'agents_born' in _MUST_AGREE
    with pytest.raises(NotImplementedError, match='compat'):
        BatchedEnv((64, 64), die.Dynamics(agents_born=True, compat='reference'), replicas=3, device='cpu')
    with pytest.raises(ValueError, match='born_spread'):
        BatchedEnv((64, 64), die.Dynamics(agents_born=True, born_spread=0.7), replicas=3, device='cpu')
    for field, other in (('born_threshold', 0.7), ('born_spread', 0.05), ('agents_born', False)):
        dyn = [die.Dynamics(agents_die=True, agents_born=True) for _ in range(3)]
        setattr(dyn[2], field, other)
        with pytest.raises(ValueError, match=field):
            BatchedEnv((64, 64), dyn, replicas=3, device='cpu')


def test_decomposed_world_refuses_births(lib):
    import die_amd as die
    from die_amd.dist import DistEnv
    with pytest.raises(NotImplementedError, match='agents_born'):
        DistEnv((256, 256), (2, 2), die.Dynamics(agents_born=True), probe_reach=11, device='cpu')
