"""die_agents_sort (csrc/die_sort.hip) and die_pic_bin / die_pic_bin_momentum (csrc/die_pic.hip) called directly over the case tables
of tests/reorder_model.py; what they write is read back and handed to that module's checkers (tests/test_reorder_cpu.py checks the
model, the checkers' teeth, the tables and the host refusals).  Every comparison is of bit patterns: there is no tolerance here.

    1  the sort at every scan shape — k_sort_scan with per = 4 (one bucket … every scan thread busy), 8 and 64, k_sort_scan_big with a
       ragged last thread and with an odd, padded bucket count —, N = 1 … 257 around the wave and workgroup sizes with 0 … 4 attached
       arrays and both kinds of slot ids, 300 000 agents where there are at least 4096 buckets, exactly one trip of the strided loops
       and a second trip that ends in a partial workgroup and a partial wave
    2  the sort on a decomposed rank's planes (80 x 96 of 256 x 256), three origins per axis, agents over the whole world
    3  the binning at every compiled tile shape, at 1024, 1056 and 16 384 tiles, into either layout, with and without _prev_grad,
       over the alive forms (no flags, all alive, 85 % dead, one dead, one alive) and two crowdings (one tile, an empty row of tiles)
    4  the binning on a decomposed rank's planes (96 x 128 of 512 x 512): the nearest-edge rule for agents outside the planes
    5  two GradientAgents with inertia on one Env: the sort carries the first one's four arrays, the second realigns itself

Every array a call writes lies between two bands of 64 sentinel elements; the sort's workspace is exactly the stated bytes plus a
256-byte tail; the inputs, the layout that is not written, die_pic.dep and the error word must come back unchanged."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from tests import reorder_model as M                                         # noqa: E402
from tests.reorder_model import Geo                                          # noqa: E402
from tests.test_gpu_parity import random_state                               # noqa: E402
from tests.test_reorder_cpu import medium_struct, pic_struct                 # noqa: E402

ERROR_WORD = 0x5EED
LAYOUT_ARRAYS = ('x', 'y', 'agent_food', 'slot', 'heading_hi', 'heading_lo')
TABLES = ('off', 'n', 's', 'inc')


@pytest.fixture(scope='module')
def L():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import die_amd                   # noqa: F401
    from die_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def die(L):
    import die_amd
    return die_amd


# ---------------------------------------------------------------- device buffers
def dev(a):
    """A host array's bits on the device (None stays None)."""
    if a is None:
        return None
    b = M.bits(a)
    return torch.from_numpy(b.view(np.int32) if b.dtype == np.uint32 else b.copy()).cuda()


class Guarded:
    """n elements of `itemsize` bytes between two bands of M.GUARD elements, every byte M.SENTINEL."""

    def __init__(self, n, itemsize=4):
        self.n, self.itemsize = n, itemsize
        self.buf = torch.full(((n + 2 * M.GUARD) * itemsize,), M.SENTINEL, dtype=torch.uint8, device='cuda')
        self.ptr = self.buf.data_ptr() + M.GUARD * itemsize

    def host(self):
        b = self.buf.cpu().numpy()
        return b if self.itemsize == 1 else b.view(np.uint32)

    def untouched(self):
        return bool((self.buf == M.SENTINEL).all())


def same(t, a):
    return np.array_equal(M.bits(t.cpu().numpy()), M.bits(a))


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------- the sort
def run_sort(L, geo, inp):
    N, n_extra = len(inp['x']), len(inp['extra'])
    d = {k: dev(inp[k]) for k in ('x', 'y', 'alive', 'agent_food', 'slot')}
    ext = [dev(e) for e in inp['extra']]
    out = {k: Guarded(N, 1 if k == 'alive' else 4) for k in ('x', 'y', 'alive', 'agent_food', 'slot')}
    out_ext = [Guarded(N) for _ in ext]
    need = int(L.lib.die_sort_workspace_bytes(geo.W, geo.H, N))
    assert need == M.sort_workspace_bytes(geo.W, geo.H, N) > 0
    ws = torch.full((need + 256,), M.SENTINEL, dtype=torch.uint8, device='cuda')      # exactly the stated bytes, then a tail
    m = medium_struct(L, geo)                                                        # extents only: the sort reads no plane
    a_in = L.Agents(N, d['x'].data_ptr(), d['y'].data_ptr(), d['alive'].data_ptr(), d['agent_food'].data_ptr(),
                    None if d['slot'] is None else d['slot'].data_ptr())
    a_out = L.Agents(N, out['x'].ptr, out['y'].ptr, out['alive'].ptr, out['agent_food'].ptr, out['slot'].ptr)
    ein = (C.c_void_p * max(n_extra, 1))(*[t.data_ptr() for t in ext])
    eout = (C.c_void_p * max(n_extra, 1))(*[g.ptr for g in out_ext])
    L.check(L.lib.die_agents_sort(C.byref(m), C.byref(a_in), C.byref(a_out), n_extra, ein, eout, ws.data_ptr(), need, stream()),
            'die_agents_sort')
    torch.cuda.synchronize()
    what = (geo, N, n_extra, inp['slot'] is not None)
    assert bool((ws[need:] == M.SENTINEL).all()), ('the tail behind the workspace was written', what)
    for k, t in d.items():
        assert t is None or same(t, inp[k]), (f'the input {k} changed', what)
    for t, a in zip(ext, inp['extra']):
        assert same(t, a), ('an attached input changed', what)
    host = {k: g.host() for k, g in out.items()}
    host['extra'] = [g.host() for g in out_ext]
    try:
        return M.check_sort(inp, host, geo)
    except AssertionError as e:
        raise AssertionError(f'{what}: {e}') from None


@pytest.mark.parametrize('W,H', [(W, H) for W, H, *_ in M.SORT_SHAPES], ids=str)
def test_sort_around_the_wave_and_workgroup_sizes(L, W, H):
    geo = Geo(W, H)
    for N in M.SMALL_N:
        for n_extra in M.N_EXTRA:
            for foreign in (False, True):
                count = run_sort(L, geo, M.sort_inputs(geo, N, n_extra, foreign))
                assert count.sum() == N and len(count) == M.n_buckets(W, H)


@pytest.mark.parametrize('W,H', [(W, H) for W, H, nb, *_ in M.SORT_SHAPES if nb >= M.SORT_MID_MIN_BUCKETS], ids=str)
def test_sort_fills_the_bucket_table(L, W, H):
    """300 000 agents: at least nine buckets in ten hold agents and at least one holds none (asserted on the model's counts)."""
    geo = Geo(W, H)
    count = run_sort(L, geo, M.sort_inputs(geo, M.MID_N, 0, False))
    assert np.array_equal(count, M.mid_counts(W, H))
    assert (count > 0).mean() >= 0.9 and (count == 0).any()
    run_sort(L, geo, M.sort_inputs(geo, M.MID_N, 4, True))
    run_sort(L, geo, M.sort_inputs(geo, M.MID_N, 1, True))


@pytest.mark.parametrize('N', [M.ONE_TRIP, M.TRIP_PLUS])
@pytest.mark.parametrize('W,H', M.SORT_BIG_SHAPES, ids=str)
def test_sort_full_and_second_trip(L, W, H, N):
    geo = Geo(W, H)
    assert M.trips(N)[0] == (1 if N == M.ONE_TRIP else 2)
    run_sort(L, geo, M.sort_inputs(geo, N, 4, True))
    run_sort(L, geo, M.sort_inputs(geo, N, 0, False))


@pytest.mark.parametrize('geo', M.sort_geos_decomposed(), ids=lambda g: f'ox{g.ox}oy{g.oy}')
def test_sort_on_a_decomposed_ranks_planes(L, geo):
    for N in M.DECOMPOSED_N:
        for n_extra, foreign in ((0, True), (4, True), (2, False)):
            run_sort(L, geo, M.sort_inputs(geo, N, n_extra, foreign))


def test_sorting_the_sorted_output_again(L):
    """The output of one call as the next one's input (the ping-pong Env.sort_agents does): keys already in order, whole waves of one
    group everywhere."""
    geo = Geo(300, 520)
    inp = M.sort_inputs(geo, 70_000, 2, True)
    order = np.argsort(M.sort_key(inp['x'], inp['y'], geo), kind='stable')
    again = dict(x=inp['x'][order], y=inp['y'][order], alive=inp['alive'][order], agent_food=inp['agent_food'][order],
                 slot=inp['slot'][order], extra=[e[order] for e in inp['extra']])
    run_sort(L, geo, again)


# ---------------------------------------------------------------- the binning
_PLANES = {}


def _dep_plane(W, H):
    """die_pic.dep_plane (W * H floats; given instead of the rim lists, never touched by the binning): one per world size."""
    if (W, H) not in _PLANES:
        _PLANES.clear()
        _PLANES[(W, H)] = torch.empty(W * H, dtype=torch.float32, device='cuda')
    return _PLANES[(W, H)]


def run_bin(L, geo, tile, inp, n_alive, into):
    N, NT = len(inp['x']), M.n_tiles(geo.W, geo.H, tile)
    assert NT == L.lib.die_pic_tiles(geo.W, geo.H, *tile)
    M.bin_tables(inp, geo, tile, n_alive)            # (n_alive is the number of alive flags: the dead go to [n_alive, N))
    momentum = inp['prev_gx'] is not None
    names = ('x', 'y', 'alive', 'agent_food', 'slot', 'heading_hi', 'heading_lo', 'prev_gx', 'prev_gy')
    d = {k: dev(inp[k]) for k in names}
    ptr = lambda k: None if d[k] is None else d[k].data_ptr()
    lay = [{k: Guarded(N) for k in LAYOUT_ARRAYS} for _ in range(2)]
    meta = [{k: Guarded(NT) for k in TABLES} for _ in range(2)]
    pg = [{k: Guarded(N) for k in ('prev_gx', 'prev_gy')} if momentum else None for _ in range(2)]
    dep, part, error = Guarded(N), Guarded(4 * NT), torch.full((1,), ERROR_WORD, dtype=torch.int32, device='cuda')
    p = pic_struct(L, tile, N, *[[lay[l][k].ptr for k in LAYOUT_ARRAYS] + [meta[l][k].ptr for k in TABLES] for l in range(2)],
                   dep.ptr, _dep_plane(geo.W, geo.H).data_ptr(), part.ptr, error.data_ptr(), n_alive=n_alive,
                   prev_grad=[(g['prev_gx'].ptr, g['prev_gy'].ptr) if g else (None, None) for g in pg])
    m = medium_struct(L, geo)
    a = L.Agents(N, ptr('x'), ptr('y'), ptr('alive'), ptr('agent_food'), ptr('slot'))
    if momentum:
        rc = L.lib.die_pic_bin_momentum(C.byref(m), C.byref(a), ptr('heading_hi'), ptr('heading_lo'), ptr('prev_gx'), ptr('prev_gy'),
                                        C.byref(p), into, stream())
    else:
        rc = L.lib.die_pic_bin(C.byref(m), C.byref(a), ptr('heading_hi'), ptr('heading_lo'), C.byref(p), into, stream())
    L.check(rc, 'die_pic_bin')
    torch.cuda.synchronize()
    what = (geo, tile, N, n_alive, into, momentum, inp['slot'] is not None)
    assert int(error.item()) == ERROR_WORD, ('the error word changed', what)
    assert dep.untouched(), ('die_pic.dep was written', what)
    for k in names:
        assert d[k] is None or same(d[k], inp[k]), (f'the input {k} changed', what)
    for k, g in list(lay[1 - into].items()) + list((pg[1 - into] or {}).items()):
        assert g.untouched(), (f'{k} of layout {1 - into}, which is not written, changed', what)
    M._check_bands('part_gain', part.host())
    out = {k: g.host() for k, g in lay[into].items()}
    if momentum:
        out.update({k: g.host() for k, g in pg[into].items()})
    try:
        return M.check_bin(inp, out, *[{k: g.host() for k, g in meta[l].items()} for l in range(2)], geo, tile, n_alive)
    except AssertionError as e:
        raise AssertionError(f'{what}: {e}') from None


def _combos(v):
    """Two of the four (into, _prev_grad) combinations, the other two for the next variant."""
    return ((v % 2, True), (1 - v % 2, False))


BIN_IDS = [f'{1 << t[0]}x{1 << t[1]}-{W}x{H}' for t, W, H, *_ in M.BIN_SHAPES]
VARIANT_IDS = [f if c is None else c for f, c in M.BIN_VARIANTS]


@pytest.mark.parametrize('form,crowd', M.BIN_VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize('tile,W,H', [s[:3] for s in M.BIN_SHAPES], ids=BIN_IDS)
def test_bin_around_the_wave_and_workgroup_sizes(L, tile, W, H, form, crowd):
    geo = Geo(W, H)
    for i, N in enumerate(M.SMALL_N):
        for into in (0, 1):
            for momentum in (False, True):
                inp, n_alive = M.bin_inputs(geo, tile, N, form, crowd, (i + into + momentum) % 2 == 1, momentum)
                count = run_bin(L, geo, tile, inp, n_alive, into)
                assert count.sum() == (n_alive if 0 < n_alive < N else N)


@pytest.mark.parametrize('form,crowd', M.BIN_VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize('tile,W,H', [s[:3] for s in M.BIN_SHAPES], ids=BIN_IDS)
def test_bin_300_000_slots(L, tile, W, H, form, crowd):
    geo, v = Geo(W, H), M.BIN_VARIANTS.index((form, crowd))
    for into, momentum in _combos(v):
        inp, n_alive = M.bin_inputs(geo, tile, M.MID_N, form, crowd, bool(into), momentum)
        count = run_bin(L, geo, tile, inp, n_alive, into)
        if crowd == 'one_tile':
            assert (count > 0).sum() == 1
        if crowd == 'empty_row':
            nty = H >> tile[1]
            assert count[nty:2 * nty].sum() == 0 and count[:nty].sum() > 0 and count[2 * nty:3 * nty].sum() > 0


@pytest.mark.parametrize('tile,W,H', [s[:3] for s in M.BIN_SHAPES], ids=BIN_IDS)
def test_bin_exactly_one_trip(L, tile, W, H):
    geo = Geo(W, H)
    for v, (form, crowd) in enumerate((('dead_85', None), ('alive_null', None))):
        into, momentum = _combos(v)[0]
        inp, n_alive = M.bin_inputs(geo, tile, M.ONE_TRIP, form, crowd, True, momentum)
        run_bin(L, geo, tile, inp, n_alive, into)


@pytest.mark.parametrize('form,crowd', M.BIN_VARIANTS, ids=VARIANT_IDS)
def test_bin_second_trip(L, form, crowd):
    (W, H), tile = M.BIN_TRIP_PLUS_SHAPE, (4, 5)
    geo, v = Geo(W, H), M.BIN_VARIANTS.index((form, crowd))
    assert M.bin_scan_per(W, H, tile) == 2 and M.trips(M.TRIP_PLUS) == (2, 37)
    for into, momentum in _combos(v + 1):
        inp, n_alive = M.bin_inputs(geo, tile, M.TRIP_PLUS, form, crowd, not momentum, momentum)
        run_bin(L, geo, tile, inp, n_alive, into)


@pytest.mark.parametrize('geo', M.bin_geos_decomposed(), ids=lambda g: f'ox{g.ox}oy{g.oy}')
def test_bin_on_a_decomposed_ranks_planes(L, geo):
    tile = M.BIN_PLANE_TILE
    for i, N in enumerate(M.DECOMPOSED_N):
        for v, form in enumerate(('alive_null', 'dead_85', 'one_alive')):
            for into, momentum in _combos(i + v):
                inp, n_alive = M.bin_inputs(geo, tile, N, form, None, True, momentum)
                run_bin(L, geo, tile, inp, n_alive, into)
    inp, _ = M.bin_inputs(geo, tile, 5000, 'alive_null', None, True, False)
    up = np.mod(M.cells(inp['x'], geo.gW) - geo.ox, geo.gW)
    assert (up >= geo.W).mean() > 0.5                      # most agents stand outside the planes: the nearest-edge rule decides


# ---------------------------------------------------------------- through Env: an agent the sort leaves behind
def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_two_agents_with_inertia_follow_the_sort(die):
    """Two GradientAgents with inertia on one world hold eight per-slot arrays; sort_agents carries four (the first agent's), the
    second agent realigns itself in _align_to on its next forward.  Same run with and without the re-sort, bit for bit."""
    W = H = 96
    medium, agents = random_state(W, H, 3000, 2400, np.random.RandomState(21), collide=0.2)
    kw = dict(scale=1.53 / (W - 1), sense_offset=10.2 / (W - 1), inertia=0.3, noise_scale=0.01)
    runs = []
    for sort_every in (2, 0):
        env = die.Env.from_numpy(medium, agents, sort_every=sort_every)
        first, second = die.GradientAgent(max_agents=3000, seed=5, **kw), die.GradientAgent(max_agents=3000, seed=6, **kw)
        obs = env._get_current_obs
        seen, carried = [], []
        for _ in range(10):
            act = first.forward(obs)
            seen.append(second.forward(obs).to_numpy())            # (read: the second agent's forward runs now, in this order)
            carried.append((first._order is env.agents.slot, second._order is env.agents.slot))
            obs, *_ = env.step(act)
        assert (env.agents.slot is not None) == (sort_every > 0)
        if sort_every:                                             # the sort moved the first agent's state, never the second's
            assert first._order is env.agents.slot and second._order is not env.agents.slot
            assert all(a and b for a, b in carried)                # … which had realigned itself by the time it acted
        runs.append([first.direction_rads_numpy(), first.prev_grad_numpy(), second.direction_rads_numpy(), second.prev_grad_numpy(),
                     env.agents.to_numpy(), env.medium.to_numpy(), np.stack(seen), env.medium.owner_slots().cpu().numpy()])
    for k, (a, b) in enumerate(zip(*runs)):
        assert a.shape == b.shape and np.array_equal(_bits64(a), _bits64(b)), f'array {k} differs between sort_every = 2 and 0'
