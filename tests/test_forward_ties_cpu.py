"""The forward tie cases (tests/forward_tie_cases.py), CPU side: the builder against the oracle alone — every decision class is present,
the thresholds are straddled by ulp-neighbours (and hit bit-exactly wherever float64 can hit them), the +1 / -1 sign pair tells
undetermined slots from determined ones, the agents stand on their cells, the margins M are small against their thresholds, and a
float64 restatement of the device's axis-aligned branch (renorm_rad, renorm_rad_fast, four comparisons with isclose_bound constants)
agrees with the oracle on every slot of groups 1 and 5 — so a mismatch on the GPU accuses the kernel, not the design or the cases.
No kernel is launched.

What float64 can hit.  delta = renormalize_radians(heading - drads) passes through (x - pi) + pi and lives on the grid of pi's ulp
(4.4e-16), while x_turn (0.03 .. 0.08) has an ulp of 6.9e-18: |delta| == x_turn is reachable only where x_turn = 0.  sense_rad is hit
exactly at 90, 45 and 180 degrees (every axis direction) and at 120 degrees for two of the four; 60 degrees never.  In every case
two headings one step of that grid apart (or one ulp of their own, where that is the larger) decide differently, which is the tie the
device has to put on the same side as numpy."""
import math
import os

import numpy as np
import pytest

from oracle import cpu_ref as R
from tests import forward_tie_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = (0.0, math.pi, math.pi / 2, -math.pi / 2)


@pytest.fixture(scope='module', autouse=True)
def built():
    """q32 (die_amd.device_array) imports the package, which loads the library."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()


def tie_worlds(pset, dtype='f32'):
    return [G.world_of(1, pset, dtype, part) for part in range(G.n_parts(1, pset, dtype))]


def test_constants_are_the_oracles():
    for p in G.PARAM_SETS:
        c, ref = G.Consts(p), R.RefPhysarumAgent(1, init_noise=np.ones((2, 1)), **G.Consts(p).kw())
        assert (c.turn_rad, c.sense_rad, c.rtol) == (ref._turn_radians, ref._sense_radians, ref._rtol)
        # x_turn is the last double np.isclose accepts
        assert np.isclose(0, c.x_turn, rtol=1e-2, atol=c.atol) and not np.isclose(0, np.nextafter(c.x_turn, 1), rtol=1e-2, atol=c.atol)
        assert np.isclose(0, c.x_grad, rtol=1e-5) and not np.isclose(0, np.nextafter(c.x_grad, 1), rtol=1e-5)
    assert G.Consts(G.PARAM_SETS[4]).x_turn == 0.0 and G.Consts(G.PARAM_SETS[3]).sense_rad == math.pi


def test_block_centres_land_on_their_cells_and_fields_are_exact():
    for dtype in ('f32', 'f16'):
        for pset in range(len(G.PARAM_SETS)):
            for w in tie_worlds(pset, dtype):
                assert np.array_equal(R.cell(w.agents[0], w.W), w.cx) and np.array_equal(R.cell(w.agents[1], w.H), w.cy)
                assert w.W <= 256 and w.H <= 192
                # the stored ramps are the exact ones: drads is one of the four constants (or 0 / pi from signed zeros)
                assert np.isin(w.drads, AXES).all() and w.axis.all()
                i = np.arange(G.B) - 1.0
                f = w.fields
                exact = f[:, 3, None, None] + f[:, 2, None, None] * (f[:, 0, None, None] * i[None, :, None] + f[:, 1, None, None] * i[None, None, :])
                chem = w.medium[2].reshape(w.W // G.B, G.B, w.H // G.B, G.B).transpose(0, 2, 1, 3).reshape(w.N, G.B, G.B)
                assert np.array_equal(chem, exact), dtype
    # the angle(-+0 -+0j) quirk is in the sample: sub-clip (-, -) is pi, every other sub-clip ramp and the flat block 0
    w = tie_worlds(0)[0]
    sub = w.fields[:, 3] == 2.0 ** -8
    neg = sub & (w.fields[:, 0] < 0) & (w.fields[:, 1] < 0)
    assert neg.sum() > 100 and (w.drads[neg] == math.pi).all() and (w.drads[sub & ~neg] == 0).all() and (sub & ~neg).sum() > 700
    assert np.signbit(w.g[0][neg]).all() and np.signbit(w.g[1][neg]).all()


def test_every_decision_class_is_present():
    count = {}
    for pset, p in enumerate(G.PARAM_SETS):
        c = G.Consts(p)
        for w in tie_worlds(pset):
            _, ug, ut, un = G.decisions(c, w.drads[:w.n], w.headings[:w.n])
            code = 4 * ug.astype(int) + 2 * ut.astype(int) + un.astype(int)
            for k, n in zip(*np.unique(code, return_counts=True)):
                key = (int(k) >> 2, (int(k) >> 1) & 1, int(k) & 1)
                count[key] = count.get(key, 0) + int(n)
    print('group 1 decision classes (und_grad, und_turn, unseen):', count)
    # und_turn and unseen exclude each other (x_turn < sense_rad): six classes are reachable
    assert set(count) == {(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 0)}
    assert min(count.values()) >= 100, count


def _axis_ramp(w, dr):
    return (w.drads == dr) & (w.fields[:, 2] == 1) & (w.fields[:, 3] == 1)


def test_thresholds_are_straddled_by_ulp_neighbours_and_hit_exactly_where_float64_can():
    exact = {}
    for pset, p in enumerate(G.PARAM_SETS):
        c = G.Consts(p)
        th = {'x_turn': (c.x_turn, 2)}
        if c.sense_rad < math.pi:
            th['sense'] = (c.sense_rad, 3)
        for name, (theta, which) in th.items():
            for dr in AXES:
                hs = np.unique(np.concatenate([w.headings[_axis_ramp(w, dr)] for w in tie_worlds(pset)]))
                dec = G.decisions(c, dr, hs)
                delta, flag = np.abs(dec[0]), dec[which]
                pair = (hs[1:] - hs[:-1] <= G.GRID) & (flag[:-1] != flag[1:])
                near = np.minimum(np.abs(delta[:-1] - theta), np.abs(delta[1:] - theta)) < 1e-15
                assert (pair & near).any(), f'no ulp-neighbours decide differently at {name} of set {p}, drads {dr}'
                exact[pset, name, dr] = int((delta == theta).sum())
    print('bit-exact |delta| == threshold per (set, threshold, drads):', exact)
    for dr in AXES:
        for pset in (0, 2):
            assert exact[pset, 'sense', dr] > 0                      # 90 and 45 degrees
        assert exact[4, 'x_turn', dr] > 0                            # x_turn = 0: delta == 0
    # sense_angle = 180: |delta| == pi exactly, where delta's sign decides right / left
    c = G.Consts(G.PARAM_SETS[3])
    for dr in AXES:
        hs = np.concatenate([w.headings[_axis_ramp(w, dr)] for w in tie_worlds(3)])
        assert (np.abs(G.decisions(c, dr, hs)[0]) == math.pi).any()


def test_sign_pair_separates_undetermined_from_determined():
    for pset, p in enumerate(G.PARAM_SETS):
        c = G.Consts(p)
        for part, w in enumerate(tie_worlds(pset)):
            kw = tuple(sorted(w.kw(c).items()))
            plus, minus = (G.expected((1, pset, 'f32', part, True, 'physarum'), 'physarum', s, kw) for s in (1, -1))
            moved = G.heading_error(plus['heading'], minus['heading']) > 0.1
            assert np.array_equal(moved, plus['und']) and np.array_equal(plus['und'], minus['und'])
            # ... and the oracle's own flags are the lines `decisions` restates
            _, ug, ut, un = G.decisions(c, w.drads, w.headings)
            assert np.array_equal(~(ug | ut), plus['mask']) and np.array_equal(ug | ut | un, plus['und'])
            dep = plus['action'][2]
            assert np.allclose(dep, 4.0 * G.FOOD * np.where(plus['mask'], 1.0, 0.1), rtol=1e-15)


def test_margins_follow_from_the_derivation():
    for pset in G.GENERIC_SETS + G.OUTSIDE_SETS:
        c = G.Consts(G.PARAM_SETS[pset])
        for hmax in (G.PI, G.HMAX_OUTSIDE):
            M = c.margins(hmax)
            print(f'set {G.PARAM_SETS[pset]} hmax {hmax:.3f}:', {k: f'{v:.3e}' for k, v in M.items()})
            assert M['x_turn'] < c.x_turn / 256 and M['sense'] < c.sense_rad / 256          # the linearisation E / |sin theta| holds
            assert M['x_turn'] == 2 * (2.0 ** -24 * hmax + 6 * 2.0 ** -23 / math.sin(c.x_turn))
    # one ulp of c near 1 is 1e-6 rad at the default x_turn: no 3e-7 there, and no 2e-5 for the default set either
    M = G.Consts(G.PARAM_SETS[0]).margins()
    assert 2e-5 < M['x_turn'] < 1e-4 and M['sense'] < 2e-5 and M['pi'] < 2e-5


def test_generic_cases_sit_at_their_margins():
    for pset in G.GENERIC_SETS:
        c = G.Consts(G.PARAM_SETS[pset])
        M = c.margins()
        n_safe = n_close = 0
        for part in range(G.n_parts(3, pset)):
            w = G.world_of(3, pset, 'f32', part)
            gen = ~w.axis
            assert gen[:w.n].all()
            safe = G.safe_slots(w, c)
            n_safe += int((safe & gen).sum())
            n_close += int((~safe).sum())
            tm = G.threshold_margins(c, w.drads, w.headings)
            for name, _ in G.thresholds_of(c):
                # headings were placed f M off: the margin the oracle sees is that, up to float64 rounding of a few pi
                got = tm[name][:w.n]
                assert (np.min(np.abs(got[:, None] / M[name] - np.array(G.MARGIN_FACTORS)[None, :]), axis=1) < 1e-6).mean() > 0.4
        assert n_safe > 2000 and n_close > 2000, (n_safe, n_close)
    # the x_grad test: drads on either side of x_grad, at and below the margin
    w = G.world_of(3, 0, 'f32', G.n_parts(3, 0) - 1)
    small = (w.fields[:, 3] == 0) & (w.fields[:, 2] > 0)
    und = np.isclose(0, w.drads[small], rtol=1e-5)
    assert small.sum() >= 50 and 10 < und.sum() < small.sum() - 10


def test_magnitude_cases_and_their_drop_count():
    total = drops = 0
    for kind in ('physarum', 'gradient'):
        for normalized in (True, False):
            w = G.world_of(4, 0, 'f32', 0, normalized, kind)
            assert (w.W, w.H) == (128, 96) and w.n == len(G.AMPLITUDES) * (G.N_PHI + 1)
            chem = w.medium[2]
            assert np.array_equal(chem, chem.astype(np.float32).astype(np.float64))
            assert 0 < np.abs(chem[chem != 0]).min() < 2.0 ** -126 and chem.max() > 2.0 ** 126
            kw = w.kw(G.Consts(G.PARAM_SETS[0]) if kind == 'physarum' else None, scale=1.0, **({} if kind == 'physarum' else dict(inertia=0.0, noise_scale=0.0)))
            exp = G.expect(w, kind, kw, 1)
            assert np.isfinite(exp['action']).all() and np.isfinite(exp['heading']).all()
            d = G.group4_drops(w, exp)
            total, drops = total + w.N, drops + int(d.sum())
            flat = w.fields[:, 2] == 0
            if kind == 'gradient':
                assert (exp['action'][:2, flat] == 0).all()
    print(f'group 4: {drops} of {total} cases dropped')
    assert drops <= G.DROP_CAP * total
    assert drops == 0


def test_renorm_forms_are_numpys_bit_for_bit():
    rs = np.random.RandomState(1)
    args = np.concatenate([rs.uniform(-8 * math.pi, 8 * math.pi, 60000), [h for k in range(-16, 17) for h in G.ulps(k * math.pi / 2)],
                           [0.0, -0.0, math.pi, -math.pi, 3 * math.pi, -3 * math.pi, 2.5 * math.pi, -2.5 * math.pi]])
    want = R.renormalize_radians(args)
    for f in (G.renorm_rad, G.renorm_rad_fast):
        got = np.array([f(float(a)) for a in args])
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), f.__name__
    assert ((want >= -math.pi) & (want <= math.pi)).all()                  # (numpy's own rounding reaches -pi itself)


def _restated_equals_oracle(w, c, key):
    kw = tuple(sorted(w.kw(c).items()))
    n = 0
    for sign in (1, -1):
        exp = G.expected(key, 'physarum', sign, kw)
        for k in np.nonzero(w.axis)[0]:
            ug, ut, un, h2 = G.axis_branch(c, float(w.g[0][k]), float(w.g[1][k]), float(w.headings[k]), sign)
            assert (not (ug or ut)) == exp['mask'][k] and (ug or ut or un) == exp['und'][k], (key, k, w.headings[k], w.drads[k])
            assert G.heading_error(h2, exp['heading'][k]) < 1e-9, (key, k)
            n += 1
    return n


def test_restated_axis_branch_agrees_with_the_oracle_on_groups_1_and_5():
    n = 0
    for pset, p in enumerate(G.PARAM_SETS):
        for part, w in enumerate(tie_worlds(pset)):
            n += _restated_equals_oracle(w, G.Consts(p), (1, pset, 'f32', part, True, 'physarum'))
    assert n > 20000
    m = 0
    for pset in G.OUTSIDE_SETS:
        for part in range(G.n_parts(5, pset)):
            w = G.world_of(5, pset, 'f32', part)
            assert np.abs(w.headings).max() > 7.9 * math.pi
            m += _restated_equals_oracle(w, G.Consts(G.PARAM_SETS[pset]), (5, pset, 'f32', part, True, 'physarum'))
    assert m > 5000


def test_edge_agents_stand_on_the_first_and_last_coordinates():
    w = tie_worlds(0)[0]
    agents, headings, n = G.edge_agents(w)
    from die_amd.device_array import to_q32
    X, Y = to_q32(agents[0, :n]), to_q32(agents[1, :n])
    assert {0, 1, 2 ** 32 - 1} <= set(X.tolist()) and {0, 1, 2 ** 32 - 1} <= set(Y.tolist()) and n == 120
    assert set(R.cell(agents[0, :n], w.W)) >= {0, w.W - 1} and set(R.cell(agents[1, :n], w.H)) >= {0, w.H - 1}
    assert ((headings > -math.pi) & (headings <= math.pi)).all()
    # the probe of the binned path: X + off as a 32-bit sum whose carry / borrow clamps (die_common.h die_cell_off) is die_cell of the
    # 33-bit sum for every edge agent, and WITHOUT the carry it is another cell on each of the four sides — the set can fail
    so = 10.2 / (max(w.W, w.H) - 1)
    for P, n_cells, trig in ((X, w.W, np.cos), (Y, w.H, np.sin)):
        P = P.astype(np.int64)
        off = np.rint(np.float32(so) * trig(headings[:n]).astype(np.float32) * np.float32(2.0 ** 32)).astype(np.int64)
        cell_u = lambda v: ((v * (n_cells - 1) + (1 << 31)) >> 32)
        full = np.where(P + off < 0, 0, np.where(P + off >= 1 << 32, n_cells - 1, cell_u((P + off) % (1 << 32))))
        lo = (P + off) % (1 << 32)
        out = np.where(off >= 0, lo < P, lo > P)
        with_carry = np.where(out, np.where(off >= 0, n_cells - 1, 0), cell_u(lo))
        assert np.array_equal(with_carry, full)
        wrong = cell_u(lo) != full
        assert (wrong & (off > 0)).sum() >= 8 and (wrong & (off < 0)).sum() >= 8
