"""The cases of tests/binned_lattice_cases.py, without a GPU: every case is built and its witnesses — computed from the oracle alone —
are asserted, so that a later edit to a builder cannot turn a GPU case (tests/test_gpu_binned_lattice.py) vacuous unnoticed; and the
launch form each case expects is the one the library's own host functions predict (die_pic_two_launch, die_pic_step_bound).  No
kernel is launched here."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import binned_lattice_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_AGENTS = 20              # agents that must attain a bound (on one side of one tile / across one kind of border)


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib.lib


def ids(specs):
    return [s['id'] + ('-' + s['side'] if 'side' in s else '') for s in specs]


def frac(v):
    return v - np.floor(v)


def long_sides(W, H):
    """Indices into the margin witnesses' sides (x low, x high, y low, y high) of the world's longer axis: a length spans its full
    number of cells there."""
    return ([0, 1] if W >= H else []) + ([2, 3] if H >= W else [])


def check_form(lib, case):
    """The expected form is the library's: die_pic_two_launch on the step scale the host derives (scale · die_pic_step_bound)."""
    W, H = case.medium.shape[1:]
    bound = lib.die_pic_step_bound(float(case.kw.get('inertia', 0.0)), float(case.kw.get('noise_scale', 0.0)))
    assert bound == 1.0                                      # no momentum anywhere in the lattice: the action is scale × a unit vector
    scale = float(np.float32(case.kw['scale']) * np.float32(bound))
    two = lib.die_pic_two_launch(max(W, H), case.tile[0], case.tile[1], scale, float(case.dyn['diffuse_sigma']), 0)
    assert two in (0, 1) and (two == 1) == (case.form == 'two launches'), (two, case.form)
    # … and the step is one the tiles take at all (the limit pick_tile and die_pic_forward_env_step share)
    assert L.reach_f32(case.kw['scale'], max(W, H)) <= min(1 << case.tile[0], 1 << case.tile[1]) - 1


@pytest.mark.parametrize('spec', L.margin_specs() + [s for s in L.special_specs() + L.thread_specs() if s['build'] is L.margin_case],
                         ids=lambda s: s['id'])
def test_margin_cases_attain_the_chem_margin(lib, spec):
    """On every side of the world's longer axis (all four in the square world) at least 20 agents of one tile have a gradient tap at
    the farthest attainable cell beyond the tile's border — floor(probe) + 2 = P_raw for every probe with a fractional part, one
    less for an integer probe (the bound is a supremum there) — and no agent of the population has a tap further out than P_raw."""
    case = L.build(spec)
    w, probe = case.witnesses, spec['args']['probe']
    W, H = case.medium.shape[1:]
    V = 8 if case.f16 else 4
    check_form(lib, case)
    assert case.form == 'two launches'
    assert w['p_raw'] in (int(np.floor(probe)) + 2, int(np.floor(probe)) + 1)     # (+ 1: the float32 product of an integer probe fell below it)
    attain = int(np.floor(probe + L.EDGE + 0.5)) + 1
    assert max(w['max_excess']) <= w['p_raw'], w
    for s in long_sides(W, H):
        assert w['max_excess'][s] == attain and w['at_max'][s] >= MIN_AGENTS, (s, attain, w)
    if frac(probe) >= 0.05:
        assert attain == w['p_raw'] and all(w['at_bound'][s] >= MIN_AGENTS for s in long_sides(W, H)), w
    if abs(frac(probe) - 0.999) < 1e-9:                      # the tight cases: no slack from rounding P up to whole vectors
        assert w['p_raw'] % V == 0 and w['p_raw'] <= L.PIC_MAX_MARGIN, w
    if frac(probe) == 0.5:                                   # one cell fewer in the bound would leave P at P_raw − 1, inside a staged window
        assert (w['p_raw'] - 1) % V == 0 and w['p_raw'] < L.PIC_MAX_MARGIN, w
    if probe == 23.2:
        assert w['p_raw'] == 25 > L.PIC_MAX_MARGIN            # the unstaged instantiation
    assert 1500 <= case.agents.shape[1] <= 30000
    if spec['args'].get('square'):
        assert W == H and long_sides(W, H) == [0, 1, 2, 3]


def check_reach(case, reach, rows_only=False):
    w = case.witnesses
    fl = w['floor_reach']
    seam = int(np.floor(reach - L.SEAM + 0.5)) + 1            # from 0.015 cell inside the world's end: floor(reach) + 2 iff frac(reach) >= 0.515
    inner = int(np.floor(reach + L.EDGE + 0.5))                # from 0.45 cell outside the cell's centre: floor(reach) + 1 iff frac(reach) >= 0.05
    for axis in ('rows',) if rows_only else ('rows', 'cols'):
        a = w[axis]
        assert a['max_interior'] == inner <= fl + 1, (axis, inner, w)
        if inner == fl + 1:
            assert a['interior_at_bound'] >= MIN_AGENTS, (axis, w)
        assert a['max_seam'] == seam <= fl + 2, (axis, seam, w)
        if seam == fl + 2:
            assert a['seam_at_bound'] >= MIN_AGENTS, (axis, w)
    return w


@pytest.mark.parametrize('spec', L.reach_specs() + [s for s in L.special_specs() if s['build'] is L.reach_case], ids=lambda s: s['id'])
def test_reach_cases_attain_the_food_margin(lib, spec):
    """Rows and columns: at least 20 agents land floor(reach) + 1 cells from their old tile across an interior border, and —
    whenever the step's fractional part lets an agent 0.015 cell inside the world's end get there — at least 20 land
    floor(reach) + 2 cells away across the world's seam; nobody lands further."""
    case = L.build(spec)
    check_form(lib, case)
    assert case.form == 'two launches'                        # floor(reach) + 2 + 2 <= 32: the rule allows it for every step of the family
    reach = spec['args']['reach']
    check_reach(case, reach)
    if frac(reach) >= 0.515:
        assert case.witnesses['rows']['max_seam'] == case.witnesses['floor_reach'] + 2


@pytest.mark.parametrize('spec', L.radius_specs(), ids=lambda s: s['id'])
def test_radius_cases_straddle_the_rim(lib, spec):
    """After the oracle's move: agents within R cells of the border shared with each of the eight neighbours; agents exactly R cells
    inside each border that stayed on their tile (not listed) and agents on the last listed cell; rim lists that hold their tile's
    agents, or (overflow cases) a tile with more listed agents than die_pic_rim_cap."""
    case = L.build(spec)
    w = case.witnesses
    check_form(lib, case)
    assert case.form == 'two launches' and w['R'] == L.radius(spec['args']['sigma']) and 1 <= w['R'] <= 4
    assert min(w['near'].values()) >= 1, w
    assert min(w['just_inside_unlisted'].values()) >= 1 and min(w['last_listed'].values()) >= 1, w
    cap = int(lib.die_pic_rim_cap(*case.tile))
    if spec['args'].get('overflow'):
        assert w['max_listed'] > cap, w
        assert w['R'] in (1, 4)
    else:                                                     # some field kernel reads a list that holds all of its tile's agents …
        assert w['min_listed'] <= cap, w
        if 'density' in spec['args']:                         # … and in the thinned 32×64 / R = 4 worlds all nine do
            assert w['max_listed'] <= cap, w


def test_radius_cases_cover_every_instantiation_of_the_field_kernel():
    seen = {(s['args']['tile'], s['args']['f16'], L.radius(s['args']['sigma'])) for s in L.radius_specs()}
    assert seen == {(t, f, r) for t in L.WORLDS for f in (False, True) for r in (1, 2, 3, 4)}
    assert [L.radius(s) for s in L.SIGMAS] == [1, 2, 2, 3, 3, 4, 4]
    assert [L.radius(s['args']['sigma']) for s in L.outside_specs()] == [0, 5]


@pytest.mark.parametrize('spec', L.rule_specs() + [s for s in L.thread_specs() if s['build'] is L.reach_case],
                         ids=ids(L.rule_specs() + [s for s in L.thread_specs() if s['build'] is L.reach_case]))
def test_rule_cases_sit_on_the_two_launch_rule(lib, spec):
    """The rule floor(reach) + 2 + R <= TX at equality, from the library (die_pic_two_launch) and from the oracle's landing cells: on
    the two-launch side the agents that cross the seam land floor(reach) + 2 = TX − R rows away, exactly R cells inside the far
    border of the tile they walk onto (the last cell that is not in its rim); one more cell of reach (three_far) puts them INSIDE that
    rim — where a tile two away would need their deposits — and the library takes the three-launch form."""
    case = L.build(spec)
    check_form(lib, case)
    TX = 1 << case.tile[0]
    assert TX == min(TX, 1 << case.tile[1])
    Rr = L.radius(case.dyn['diffuse_sigma'])
    reach, side = spec['args']['reach'], spec.get('side', 'limit')
    w = check_reach(case, reach, rows_only=True)['rows']
    fl = case.witnesses['floor_reach']
    assert w['max_seam'] <= TX                                # nobody leaves the neighbouring tile
    if side == 'two':
        assert case.form == 'two launches' and fl + 2 + Rr == TX
        assert w['max_seam'] == TX - Rr and w['seam_at_bound'] >= MIN_AGENTS and w['nearest_far_border'] == Rr, w
    elif side == 'three':
        assert case.form == 'three launches' and fl + 1 + Rr == TX and w['nearest_far_border'] == Rr, w
    elif side == 'three_far':
        assert case.form == 'three launches' and fl + 1 + Rr == TX
        assert w['max_seam'] == TX - Rr + 1 and w['seam_at_bound'] >= MIN_AGENTS and w['nearest_far_border'] == Rr - 1, w
    else:
        assert case.form == 'three launches' and reach == TX - 1 and w['max_seam'] == TX and w['nearest_far_border'] == 0, w


@pytest.mark.parametrize('spec', L.outside_specs(), ids=lambda s: s['id'])
def test_radii_without_a_field_kernel_are_not_two_launch(lib, spec):
    case = L.build(spec)
    check_form(lib, case)
    assert case.form == 'three launches' and not 1 <= case.witnesses['R'] <= 4


def test_specialised_points_are_recognised():
    """The predicate the GPU tests use to tell which cases the agent kernel's specialised instantiations take."""
    points = (((6, 6), False), ((5, 7), True))                # (only these tile shapes / dtypes can match: the others are not built again here)
    hits = [s['id'] for s in L.lattice_specs() if (s['args']['tile'], s['args']['f16']) in points and not s['args'].get('threads')
            and s['args'].get('agent', 'physarum') == 'physarum' and L.special_point(L.build(s))]
    assert all(L.special_point(L.build(s)) for s in L.special_specs())
    assert 4 <= len(hits) <= 16 and any('margin' in h for h in hits) and any('reach' in h for h in hits) and any('radius' in h for h in hits), hits


def test_host_and_library_agree_on_the_longest_step(lib):
    """reach <= min(TX, TY) − 1 is decided twice: by the host (Env picks the tile-binned step, die_amd/pic.py pick_tile) and by the
    library (die_pic_forward_env_step refuses longer steps).  Both now take the reach in float32 (pic.reach_cells); in float64 a step of
    exactly 31 cells on a 384-cell axis came out as 31.0000003 and Env quietly took the classic step.

    No library call is made here: the library exports no host function for its reach, so this test compares pic.reach_cells with a
    restatement of the library's float32 product (binned_lattice_cases.reach_f32) and with pick_tile.  That the library itself TAKES
    the step at the limit is shown on the GPU by the `rule-*-limit` cases of tests/test_gpu_binned_lattice.py (31 cells on 384×384,
    15 on 96×96: die_pic_forward_env_step runs, Env bins)."""
    from die_amd.pic import pick_tile, reach_cells
    for tile, n in (((5, 7), 384), ((4, 5), 96), ((6, 6), 192), ((5, 6), 192)):
        T = min(1 << tile[0], 1 << tile[1])
        for cells in (T - 1, T - 1 + 0.01, T - 1 - 0.01):
            agent = SimpleNamespace(_scale=cells / (n - 1), _inertia=0.0, _noise_scale=0.0)
            r = reach_cells(agent, n)
            assert r == L.reach_f32(cells / (n - 1), n)       # the library's arithmetic: float32(scale) · float32(n − 1), rounded to float32
            assert (pick_tile(n, n, r, shapes=(tile,)) == tile) == (r <= T - 1)
            if cells != T - 1:
                assert (r <= T - 1) == (cells < T - 1)
    assert float(np.float32(31 / 383)) * 383 > 31 and reach_cells(SimpleNamespace(_scale=31 / 383, _inertia=0.0, _noise_scale=0.0), 384) == 31.0
