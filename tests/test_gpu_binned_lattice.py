"""The tile-binned step (die_amd/csrc/die_pic.hip: agent kernel k_pic_forward_move, field kernel k_pic_resolve_diffuse) against the
float64 oracle over the lattice of its host-derived bounds — chem margin, food margin, gaussian radius, two-launch rule — with
agents placed where each bound is attained (tests/binned_lattice_cases.py; the witnesses are asserted without a GPU in
tests/test_binned_lattice_cpu.py).  Every case runs through tests/test_gpu_parity.py::_binned_steps_against_the_oracle: three
teacher-forced steps, its tolerances and its strict rule for forward mismatches, unchanged.  An out-of-window LDS read, a food cell
taken from the wrong row, an agent missing from a rim list or a two-launch step that should have been three launches give a wrong
probe, reward or chem value there — not a fault.

After the run every case asserts the form that ran (the library chooses: the step's state is created with rim lists AND may
allocate the deposit plane), an error word of 0, and that the agent kernel's specialised instantiations were launched exactly where
their parameter points are (die_pic_k1_specialised_launches)."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import cpu_ref as R                                              # noqa: E402
from tests import binned_lattice_cases as L                                  # noqa: E402
from tests.test_gpu_parity import RTOL, _binned_steps_against_the_oracle, applied, ref_dyn      # noqa: E402

STEPS = 3


@pytest.fixture(scope='module')
def die():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import die_amd
    return die_amd


@pytest.fixture(params=[False, True], ids=['specialised', 'DIE_PIC_K1_GENERIC=1'])
def generic(request, monkeypatch):
    monkeypatch.setenv('DIE_PIC_K1_GENERIC', '1' if request.param else '0')
    return request.param


def ids(specs):
    return [s['id'] + ('-' + s['side'] if 'side' in s else '') for s in specs]


def dynamics(die, case):
    return die.Dynamics(boundary=die.BoundaryCondition(case.dyn['boundary']), diffuse_sigma=case.dyn['diffuse_sigma'])


def run_case(die, case, special_launches):
    """The case against the oracle; then the form that ran, the error word and the specialised launches (`special_launches`: how many
    of the STEPS agent-kernel launches must have been a specialised instantiation's)."""
    from die_amd import _lib

    def library_chooses(step, env, agent, when):
        # (_binned_steps_against_the_oracle creates the env with rim lists only for 'two launches': here the step's state always has
        # them, and the library's rule — not the test — sends a step to the three-launch form)
        if when == 'before' and step == 0:
            env._pic_fused = True

    before = int(_lib.lib.die_pic_k1_specialised_launches())
    env = _binned_steps_against_the_oracle(die, case.medium, case.agents, dynamics(die, case), case.tile, case.agent, case.kw, STEPS, f16=case.f16,
                                           form=case.form, dir0=case.dir0, k1_threads=case.threads, callback=library_chooses)
    pic = env._pic
    assert pic.fused and pic.rim is not None
    two = pic._two_launch(env, pic.agent)
    assert two == (case.form == 'two launches'), f'the library chose {"two" if two else "three"} launches, the rule says {case.form}'
    assert (pic._dep_plane is not None) == (not two)
    assert int(pic.error[0].item()) == 0, 'the step set its error word'
    env.check()
    moved = int(_lib.lib.die_pic_k1_specialised_launches()) - before
    assert moved == special_launches, f'{moved} launches of a specialised agent kernel, expected {special_launches}'
    return case, env


LATTICE = L.lattice_specs()


@pytest.mark.parametrize('spec', LATTICE, ids=ids(LATTICE))
def test_lattice_case_vs_oracle(die, spec, monkeypatch):
    """Margin, reach, radius and rule families and the other workgroup sizes (tests/binned_lattice_cases.py).  The cases that sit on a
    parameter point of a specialised instantiation run the GENERIC one here (DIE_PIC_K1_GENERIC=1: the instantiation every other
    point of the lattice takes); nowhere does the counter of specialised launches move."""
    case = L.build(spec)
    monkeypatch.setenv('DIE_PIC_K1_GENERIC', '1' if L.special_point(case) else '0')
    run_case(die, case, 0)


SPECIAL = L.special_specs()


@pytest.mark.parametrize('spec', SPECIAL, ids=ids(SPECIAL))
def test_specialised_points_at_the_tightest_placement(die, spec, generic):
    """The two specialised instantiations (fp32 64×64 tiles / chem margin 12, fp16 32×128 tiles / chem margin 16; food margin 3 rows) with
    a probe whose taps reach the last staged cell and a step that lands on the last staged food row — and the generic instantiation at
    the same points.  Without DIE_PIC_K1_GENERIC every launch is a specialised one: the host's bounds still select it."""
    case = L.build(spec)
    assert L.special_point(case)
    run_case(die, case, 0 if generic else STEPS)


OUTSIDE = L.outside_specs()


@pytest.mark.parametrize('spec', OUTSIDE, ids=ids(OUTSIDE))
def test_radii_without_a_field_kernel_take_the_classic_step(die, spec):
    """σ = 0.12 (R = 0) and σ = 1.125 (R = 5) are NOT three-launch cases of the binned step: its field kernels exist for R = 1..4 (the
    three-launch form's sweep included), die_pic_two_launch says 0 and Env.step does not bin.  R = 5 takes the classic step — with the
    same result against the oracle, teacher-forced as above: coordinates and the agents channel exact, fields and agent_food within
    1e-5 relative.

    KNOWN LIBRARY LIMITATION, not wanted behaviour: R = 0 (σ < 0.125, a gaussian of one tap — an identity diffusion that the
    reference and the oracle take) the library has nowhere; die_diffuse_decay refuses it ("empty kernel") for every step path.  The
    test pins only that the refusal is an error by name and not a silently wrong step; when the library learns R = 0 this branch is to
    become an oracle comparison like the R = 5 one."""
    from die_amd import _lib
    case = L.build(spec)
    N = case.agents.shape[1]
    env = die.Env.from_numpy(case.medium, case.agents, dynamics(die, case), sort_every=0)
    env._pic_tile = case.tile
    rd = ref_dyn(env.dynamics)
    for f in ('rate_feed', 'rate_decay_chem', 'diffuse_sigma'):
        setattr(rd, f, float(np.float32(getattr(rd, f))))
    dev = die.PhysarumAgent(max_agents=N, seed=3, **case.kw)
    dev.set_state(case.dir0)
    obs = env._get_current_obs
    if case.witnesses['R'] == 0:
        with pytest.raises(_lib.DieError, match='empty kernel'):
            env.step(dev.forward(obs))
        assert env._pic is None
        return
    for step in range(STEPS):
        renv = R.RefEnv(env.medium.to_numpy(), env.agents.to_numpy(), rd)
        action = dev.forward(obs)
        obs, reward, _, _, info = env.step(action)
        assert env._pic is None, 'the tile-binned step ran with a gaussian radius it has no field kernel for'
        _, want_reward, _, _, want_info = renv.step(applied(action.to_numpy()))
        ga, gm = env.agents.to_numpy(), env.medium.to_numpy()
        assert np.array_equal(ga[:3], renv.agents[:3]), f'step {step}: coordinates / alive'
        assert np.array_equal(gm[0], renv.medium[0]), f'step {step}: agents channel'
        assert np.allclose(ga[3], renv.agents[3], rtol=RTOL, atol=1e-7), f'step {step}: agent_food'
        assert np.allclose(gm[1], renv.medium[1], rtol=RTOL, atol=1e-7), f'step {step}: food'
        assert np.allclose(gm[2], renv.medium[2], rtol=RTOL, atol=1e-7), f'step {step}: chem'
        assert info['num_agents'] == want_info['num_agents']
        assert abs(reward - want_reward) <= RTOL * np.abs(renv.last_gained).sum() + 1e-9, f'step {step}: reward'
