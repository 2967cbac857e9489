"""The Gradient / Physarum forward pass at exact ties, at a derived margin off its thresholds, at chem magnitudes from the denormals to
2^126 and at headings outside (-pi, pi] (tests/forward_tie_cases.py has the worlds, the oracle's expectations and the derivation of the
margins M; tests/test_forward_ties_cpu.py holds a float64 restatement of the device's axis-aligned branch against them).

    1  exact ties on axis-aligned, flat and sub-clip gradients, five parameter sets, fp32 and fp16 fields, turn signs all +1 and all -1:
       die_gradient_forward and the fused die_forward_env_step give the same bits and ZERO slots differ from the oracle
    2  the same worlds through one Env.step, tile-binned (die_pic_forward_env_step, FwdTileMem) against classic, 'wrap' and 'limit':
       headings, actions handed back and agents bit for bit; and agents on X, Y in {0, 1, 2^32 - 1} probing outward
    3  generic directions: every slot at least M off every threshold agrees; closer slots are recorded (printed as the module ends)
    4  chem amplitudes 2^-148 .. 2^126, grad_clip = 0, both agent kinds, normalised and not (die_normalize2)
    5  headings in +-8 pi through set_state (renorm_rad's general form, die_sincos beyond its range)

Every world is at most 256 x 192 and sees one forward or one step.

Measured on an MI355X (group 3: slots placed M / 64, M / 16, M / 8, M / 4 and M / 2 off a threshold; M comes from the derivation, not from
these figures, and every slot from M on is asserted):

    set (turn, sense, tolerance)   threshold            M          largest margin of a slot that differed   all agree from
    (30, 90, 0.1)                  x_turn = 0.0529      2.743e-5   1.715e-6                                  3.43e-6 = 0.125 M
                                   sense = 90 deg       1.805e-6   1.128e-7                                  2.26e-7 = 0.125 M
                                   drads at x_grad      1.431e-14  3.02e-16                                  5.86e-16 = 0.041 M
    (35, 120, 0.05)                x_turn = 0.0309      4.675e-5   2.922e-6                                  5.84e-6 = 0.125 M
                                   sense = 120 deg      2.026e-6   1.266e-7                                  2.53e-7 = 0.125 M
    (22.5, 180, 0.2)               x_turn = 0.0793      1.843e-5   1.152e-6                                  2.30e-6 = 0.125 M
                                   |delta| = pi         1.805e-6   1.128e-7                                  2.26e-7 = 0.125 M

So no decision differed beyond M / 8, and the "3e-7 rad" die_forward.h used to claim did not hold at x_turn (slots 1.7e-6 and 2.9e-6 rad
off it differ).  M(x_turn) of the default set is above 2e-5, so the 1e-4 rule of tests/test_gpu_parity.py keeps its wording.

Group 4 found two defects of the un-normalised PhysarumAgent below 2^-126 (fixed in die_forward.h with this module): the generic branch
decided on the raw gradient, whose products with cos and sin have no bits left there (7 of 52 slots at 2^-148 and 7 of 47 at 2^-140 turned
the wrong way at margins >= M; against the parent's library this module fails in test_chem_magnitudes...[physarum-raw] alone), and the
new heading was the fp32 arctangent of the fp32 action (read in the code: 1e-7 rad off at best, the quantised vector's angle in the
denormals) where the reference keeps d2 — the 1e-9 of group 1 holds there only since the fix.
"""
import math

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import cpu_ref as R                                           # noqa: E402
from tests import forward_tie_cases as G                                  # noqa: E402

RECORD = {}            # (set, threshold) -> [M, largest margin of a slot that differed, margins tested below M]


@pytest.fixture(scope='module')
def die():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import die_amd
    yield die_amd
    for (pset, name), (M, worst, tested) in sorted(RECORD.items()):
        if not tested:                                                   # (no slot of this set lies closer than M to that threshold)
            continue
        above = [m for m in tested if m > 1.01 * worst]                   # (margins of one factor differ in their last bits)
        agree = min(above) if above else M
        print(f'forward ties, device: set {G.PARAM_SETS[pset]} {name}: M {M:.3e}, largest margin of a differing slot {worst:.3e}, '
              f'smallest margin from which all agree {agree:.3e} = {agree / M:.3f} M')


def _dt(dtype):
    return {'f32': torch.float32, 'f16': torch.float16}[dtype]


def make_env(die, w, dyn=None, pic=False, agents=None, medium=None):
    env = die.Env.from_numpy(w.medium if medium is None else medium, w.agents if agents is None else agents, dyn, sort_every=0, pic=pic,
                             field_dtype=_dt(w.dtype))
    if pic:
        env._pic_tile = (4, 5)                                           # 16 x 32-cell tiles (worlds this small take the classic step by default)
    return env


def make_agent(die, w, kind, kw, sign, headings=None):
    cls = die.PhysarumAgent if kind == 'physarum' else die.GradientAgent
    ag = cls(max_agents=w.N, seed=1, **kw)
    ag.set_state(w.headings if headings is None else headings)
    if sign is not None:
        ag.set_turn_signs(np.full(w.N, sign))
    return ag


def forward_direct(die, w, kind, kw, sign):
    """die_gradient_forward: (action (3, N) float64, headings)."""
    env, ag = make_env(die, w), make_agent(die, w, kind, kw, sign)
    ag.lazy = False
    act = ag.forward(env._get_current_obs).to_numpy()
    return act, ag.direction_rads_numpy()


def forward_in_step(die, w, kind, kw, sign, pic=False, dyn=None, agents=None, medium=None, headings=None):
    """env.step(agent.forward(obs)): forward inside die_forward_env_step (pic: die_pic_forward_env_step)."""
    env, ag = make_env(die, w, dyn, pic, agents, medium), make_agent(die, w, kind, kw, sign, headings)
    act = ag.forward(env._get_current_obs)
    env.step(act)
    if pic:
        assert env._pic is not None and env._pic.held[0] is env.agents.x, 'the tile-binned path did not run'
    return act.to_numpy(), ag.direction_rads_numpy(), env.agents.to_numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return np.array_equal(a.view(np.int64), b.view(np.int64))


def describe(w, bad, got_heading, exp, limit=8):
    k = np.nonzero(bad)[0][:limit]
    return [dict(slot=int(i), field=w.fields[i].tolist(), heading=float(w.headings[i]).hex(), drads=float(w.drads[i]),
                 got=float(got_heading[i]), want=float(exp['heading'][i])) for i in k]


# ---------------------------------------------------------------- 1. exact ties
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
@pytest.mark.parametrize('pset', range(len(G.PARAM_SETS)), ids=lambda i: '-'.join(str(v) for v in G.PARAM_SETS[i]))
def test_exact_ties_on_axis_aligned_gradients(die, pset, dtype):
    consts = G.Consts(G.PARAM_SETS[pset])
    for part in range(G.n_parts(1, pset, dtype)):
        w = G.world_of(1, pset, dtype, part)
        kw = w.kw(consts)
        moved = []
        for sign in (1, -1):
            exp = G.expected((1, pset, dtype, part, True, 'physarum'), 'physarum', sign, tuple(sorted(kw.items())))
            act, hd = forward_direct(die, w, 'physarum', kw, sign)
            ok = G.slots_agree(w, act, hd, exp, kw['scale'])
            print(f'ties {G.PARAM_SETS[pset]} {dtype} part {part} sign {sign:+d}: {int((~ok).sum())} of {w.N} slots differ')
            assert ok.all(), describe(w, ~ok, hd, exp)
            # the deposit shows the mask itself
            assert np.array_equal(act[2] < 0.5, ~exp['mask'])
            act2, hd2, _ = forward_in_step(die, w, 'physarum', kw, sign)
            assert same_bits(act, act2) and same_bits(hd, hd2), 'die_gradient_forward and the fused step differ'
            moved.append(hd)
        # the sign pair: 'undetermined' is the set of slots whose heading follows the forced sign
        assert np.array_equal(G.heading_error(moved[0], moved[1]) > 0.1, exp['und'])


# ---------------------------------------------------------------- 2. the binned path
@pytest.mark.parametrize('boundary', ['wrap', 'limit'])
@pytest.mark.parametrize('pset,dtype', [(0, 'f32'), (0, 'f16'), (1, 'f32'), (2, 'f32'), (3, 'f32'), (4, 'f32')])
def test_tile_binned_step_on_the_tie_worlds(die, pset, dtype, boundary):
    consts = G.Consts(G.PARAM_SETS[pset])
    for part in range(G.n_parts(1, pset, dtype)):
        w = G.world_of(1, pset, dtype, part)
        kw = w.kw(consts)
        for sign in (1, -1):
            outs = [forward_in_step(die, w, 'physarum', kw, sign, pic=pic, dyn=die.Dynamics(boundary=die.BoundaryCondition(boundary)))
                    for pic in (True, False)]
            for name, a, b in zip(('actions', 'headings', 'agents'), outs[0], outs[1]):
                assert same_bits(a, b), (name, part, sign)
            exp = G.expected((1, pset, dtype, part, True, 'physarum'), 'physarum', sign, tuple(sorted(kw.items())))
            ok = G.slots_agree(w, outs[0][0], outs[0][1], exp, kw['scale'])
            assert ok.all(), describe(w, ~ok, outs[0][1], exp)


@pytest.mark.parametrize('boundary', ['wrap', 'limit'])
@pytest.mark.parametrize('dtype', ['f32', 'f16'])
def test_tile_binned_step_with_agents_on_the_first_and_last_coordinates(die, dtype, boundary):
    w = G.world_of(1, 0, dtype, 0)
    agents, headings, n = G.edge_agents(w)
    medium = w.medium.copy()
    medium[0] = 0
    medium[0][R.cell(agents[0], w.W), R.cell(agents[1], w.H)] = 1
    reach = 10.2                                                         # cells: a staged margin of 12 (fp32) / 16 (fp16), below PIC_MAX_MARGIN
    kw = w.kw(G.Consts(G.PARAM_SETS[0]), sense_offset=reach / (max(w.W, w.H) - 1))
    # the probes do leave the world on all four sides
    off = np.stack(R.polar2xy(kw['sense_offset'], headings[:n]))
    assert ((agents[0, :n] + off[0]).min() < 0 and (agents[0, :n] + off[0]).max() > 1 and (agents[1, :n] + off[1]).min() < 0
            and (agents[1, :n] + off[1]).max() > 1)
    for sign in (1, -1):
        outs = [forward_in_step(die, w, 'physarum', kw, sign, pic=pic, dyn=die.Dynamics(boundary=die.BoundaryCondition(boundary)),
                                agents=agents, medium=medium, headings=headings) for pic in (True, False)]
        for name, a, b in zip(('actions', 'headings', 'agents'), outs[0], outs[1]):
            assert same_bits(a, b), (name, sign)
        assert np.isfinite(outs[0][0]).all()
        # the deposit still shows food and mask alone, wherever the probe went
        assert np.isin(np.round(outs[0][0][2], 6), (0.1, 1.0)).all()


# ---------------------------------------------------------------- 3. generic directions
def _note(pset, consts, M, tm, differ, asserted):
    """Record the slots closer than M to a threshold: the largest margin among those that differ, per nearest threshold."""
    names = [n for n, _ in G.thresholds_of(consts)] + ['x_grad']
    rel = np.stack([tm[n] / M[n] if M[n] > 0 else np.full(len(differ), np.inf) for n in names])
    nearest = np.argmin(rel, axis=0)
    for i, name in enumerate(names):
        sel = (nearest == i) & ~asserted
        rec = RECORD.setdefault((pset, name), [M[name], 0.0, set()])
        rec[2].update(tm[name][sel].tolist())
        if (sel & differ).any():
            rec[1] = max(rec[1], float(tm[name][sel & differ].max()))


@pytest.mark.parametrize('pset', G.GENERIC_SETS, ids=lambda i: '-'.join(str(v) for v in G.PARAM_SETS[i]))
def test_generic_directions_agree_from_the_derived_margin_on(die, pset):
    consts = G.Consts(G.PARAM_SETS[pset])
    M = consts.margins()
    for part in range(G.n_parts(3, pset)):
        w = G.world_of(3, pset, 'f32', part)
        kw = w.kw(consts)
        safe = G.safe_slots(w, consts)
        tm = G.threshold_margins(consts, w.drads, w.headings)
        for sign in (1, -1):
            exp = G.expected((3, pset, 'f32', part, True, 'physarum'), 'physarum', sign, tuple(sorted(kw.items())))
            act, hd = forward_direct(die, w, 'physarum', kw, sign)
            ok = G.slots_agree(w, act, hd, exp, kw['scale'])
            _note(pset, consts, M, tm, ~ok, safe)
            print(f'generic {G.PARAM_SETS[pset]} part {part} sign {sign:+d}: {int((~ok & safe).sum())} of {int(safe.sum())} slots at '
                  f'm >= M differ, {int((~ok & ~safe).sum())} of {int((~safe).sum())} closer ones')
            assert (ok | ~safe).all(), describe(w, ~ok & safe, hd, exp)


# ---------------------------------------------------------------- 4. magnitudes
@pytest.mark.parametrize('normalized', [True, False], ids=['normalised', 'raw'])
@pytest.mark.parametrize('kind', ['physarum', 'gradient'])
def test_chem_magnitudes_from_the_denormals_to_2_126(die, kind, normalized):
    consts = G.Consts(G.PARAM_SETS[0])
    w = G.world_of(4, 0, 'f32', 0, normalized, kind)
    kw = w.kw(consts, scale=1.0) if kind == 'physarum' else w.kw(None, scale=1.0, inertia=0.0, noise_scale=0.0)
    safe = G.safe_slots(w, consts) if kind == 'physarum' else np.ones(w.N, dtype=bool)
    amp = w.fields[:, 2]
    for sign in (1, -1):
        exp = G.expected((4, 0, 'f32', 0, normalized, kind), kind, sign, tuple(sorted(kw.items())))
        keep = ~G.group4_drops(w, exp)
        assert keep.all()                                               # (tests/test_forward_ties_cpu.py: nothing is dropped at scale 1)
        act, hd = forward_direct(die, w, kind, kw, sign)
        assert np.isfinite(act).all() and np.isfinite(hd).all(), 'NaN or Inf'
        want = exp['action']
        # GradientAgent: the action IS the (normalised) gradient — RTOL and one denormal step.  PhysarumAgent: it is |u| (cos, sin) of the
        # new heading rounded to fp32, so group 1's 4e-7 * scale (the angle's rounding at a zero crossing) applies times |u|
        atol = G.DENORM * kw['scale'] + (4e-7 * kw['scale'] * (1.0 if normalized else w.norm) if kind == 'physarum' else 0.0)
        err = np.abs(act[:2] - want[:2]) - (G.RTOL * np.abs(want[:2]) + atol)
        for a in G.AMPLITUDES:
            sel = (amp == a) & keep & safe
            print(f'magnitudes {kind} {"normalised" if normalized else "raw"} sign {sign:+d} a = 2^{int(math.log2(a))}: '
                  f'{int((err[:, sel] > 0).any(axis=0).sum())} of {int(sel.sum())} slots out of tolerance, worst excess {err[:, sel].max():.3e}')
        zero = (want[0] == 0) & (want[1] == 0)
        assert zero.sum() >= len(G.AMPLITUDES) or kind == 'physarum'
        assert (act[:2, zero] == 0).all() and not np.signbit(act[:2, zero]).any(), 'a flat block must give (+0, +0) * scale'
        assert (err[:, keep & safe] <= 0).all(), 'dx, dy'
        if kind == 'physarum':
            ok = G.slots_agree(w, act, hd, exp, kw['scale'], atol_xy=atol)
            assert (ok | ~safe).all(), describe(w, ~ok & safe, hd, exp)
        elif normalized:                                                # get_radians of the fp32 vector: an fp32 arctangent, a few ulp of pi
            assert (G.heading_error(hd, exp['heading']) < 1e-6).all()


# ---------------------------------------------------------------- 5. headings outside (-pi, pi]
@pytest.mark.parametrize('pset', G.OUTSIDE_SETS, ids=lambda i: '-'.join(str(v) for v in G.PARAM_SETS[i]))
def test_headings_outside_the_principal_range(die, pset):
    consts = G.Consts(G.PARAM_SETS[pset])
    for part in range(G.n_parts(5, pset)):
        w = G.world_of(5, pset, 'f32', part)
        kw = w.kw(consts)
        safe = G.safe_slots(w, consts, G.HMAX_OUTSIDE)
        assert safe[w.axis].all() and safe.mean() > 0.9
        for sign in (1, -1):
            exp = G.expected((5, pset, 'f32', part, True, 'physarum'), 'physarum', sign, tuple(sorted(kw.items())))
            act, hd = forward_direct(die, w, 'physarum', kw, sign)
            assert ((hd > -math.pi - 1e-12) & (hd <= math.pi)).all()
            ok = G.slots_agree(w, act, hd, exp, kw['scale'])
            print(f'outside {G.PARAM_SETS[pset]} part {part} sign {sign:+d}: {int((~ok & safe).sum())} of {int(safe.sum())} asserted slots '
                  f'differ ({int((~ok & w.axis).sum())} of them axis-aligned), {int((~ok & ~safe).sum())} of {int((~safe).sum())} closer ones')
            assert (ok | ~safe).all(), describe(w, ~ok & safe, hd, exp)
            act2, hd2, _ = forward_in_step(die, w, 'physarum', kw, sign)
            assert same_bits(act, act2) and same_bits(hd, hd2), 'die_gradient_forward and the fused step differ'
