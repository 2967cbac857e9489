"""The differentiable Env.step, CPU side: the float64 oracle of the GPU tests (tests/field_step_adjoint_model.py) agrees with the
project's explicit diffusion and with finite differences on every case, a plain fp32 evaluation of every case stays a tenth of
the GPU ceiling from it, the two entry points are exported under the unchanged ABI version and refuse bad arguments on the host
(fake pointers: a launch would have failed), and the Python refusals raise before anything is touched.  No kernel is launched."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import cpu_ref as R
from tests import dropout_model as D
from tests import field_step_adjoint_model as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('die_deposit_cells', 'die_env_step_backward')
FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host
ARG, UNSUPPORTED = -1, -3
GPU_TOL = 1e-4                       # tests/test_gpu_field_step_grad.py test 5 (the ceiling of tests/test_gpu_nca_grad.py)
ALL = [(name, W, H, T) for name in sorted(F.CASES) for W, H, T in F.SHAPES]


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


# ---- the model's diffusion is the project's
@pytest.mark.parametrize('W,H,sigma', [(5, 6, 0.5), (24, 68, 0.8), (3, 4, 0.8), (9, 7, 1.2)])
def test_model_diffusion_is_the_explicit_reference(W, H, sigma):
    rs = np.random.RandomState(W * H)
    chem = rs.rand(W, H)
    got = F.diffuse_decay(torch.as_tensor(chem), sigma, 0.1).numpy()
    want = R.diffuse_decay_explicit(chem, float(np.float32(sigma)), float(np.float32(0.1)))
    assert np.abs(got - want).max() <= 1e-14
    assert np.allclose(F.taps(sigma), R.gaussian_weights(float(np.float32(sigma))), rtol=1e-15, atol=0)
    # and one step adds the winners' deposits first: cell 7 gets 2.5, cell 0 nothing from the loser (-1)
    dep = torch.tensor([2.5, 4.0, -1.0], dtype=torch.float64)
    got = F.step_chem(torch.as_tensor(chem), dep, [7, -1, 3], sigma, 0.1).numpy()
    plus = chem.copy().reshape(-1)
    plus[7] += 2.5
    plus[3] -= 1.0
    assert np.abs(got - R.diffuse_decay_explicit(plus.reshape(W, H), float(np.float32(sigma)), float(np.float32(0.1)))).max() <= 1e-14


def test_winner_rule_is_the_last_alive_slot_in_slot_order():
    cx, cy = np.array([1, 1, 1, 2, 2, 0]), np.array([3, 3, 3, 0, 0, 0])
    alive = np.array([1, 1, 0, 0, 1, 0])
    assert F.deposit_cells(cx, cy, alive, None, 10).tolist() == [-1, 13, -1, -1, 20, -1]
    assert F.deposit_cells(cx, cy, alive, [9, 4, 11, 2, 0, 1], 10).tolist() == [13, -1, -1, -1, 20, -1]
    # the reference's fancy-index assignment says the same (core/env.py:211: the last alive index written stays)
    owner = np.full((3, 10), -1)
    idx = np.flatnonzero(alive)
    owner[cx[idx], cy[idx]] = idx
    assert owner[1, 3] == 1 and owner[2, 0] == 4


# ---- the model against finite differences, every case
@functools.lru_cache(maxsize=None)
def _inputs(name, W, H, T):
    c = F.CASES[name]
    masks = None
    if 'p' in c:
        masks = [D.mask(c['seed'], t, W, H, c['p']).astype(np.float64) for t in range(T + 1)]
    chem0, frames, cells = F.synthetic_frames(name, W, H, T, masks)
    cvec, u = F.loss_vectors(name, W, H, frames[0]['cx'].size)
    kw = dict(boundary=c['boundary'], chem0=chem0, frames=frames, cells=cells, c=cvec, u=u, sigma=c['sigma'],
              with_agent_channel=c.get('with_agent_channel', True))
    return F.weights_of(name, W, H), kw


@functools.lru_cache(maxsize=None)
def _f64(name, W, H, T):
    weights, kw = _inputs(name, W, H, T)
    return F.rollout(weights, leaf_chem=True, **kw)


@pytest.mark.parametrize('name,W,H,T', ALL)
def test_model_gradients_agree_with_finite_differences(name, W, H, T):
    weights, kw = _inputs(name, W, H, T)
    ref = _f64(name, W, H, T)
    assert [g.shape for g in ref['grads']] == [w.shape for w in weights]
    assert any(int((cl >= 0).sum()) for cl in kw['cells']) and all(np.abs(g).max() > 0 for g in ref['grads'])
    rs = np.random.RandomState(T)
    eps = 1e-6
    # directional derivatives: one random direction per layer and one over the initial chem plane (every weight enters each of them)
    for li in range(len(weights) + 1):
        if li < len(weights):
            v = rs.standard_normal(weights[li].shape)
            move = lambda s: dict(weights=[w + s * v if i == li else w for i, w in enumerate(weights)])
            want = float((ref['grads'][li] * v).sum())
        else:
            v = rs.standard_normal(kw['chem0'].shape)
            move = lambda s: dict(weights=weights, chem0=kw['chem0'] + s * v)
            want = float((ref['grad_chem0'] * v).sum())
        val = []
        for s in (eps, -eps):
            k = dict(kw)
            k.update(move(s))
            val.append(F.rollout(k.pop('weights'), **k)['loss'])
        fd = (val[0] - val[1]) / (2 * eps)
        # central differences: eps^2 * f''' / 6 truncation (~1e-12 |f'''|) plus 2^-53 * |loss| / eps rounding (~1e-8 at |loss| ~ 100)
        assert abs(fd - want) <= 1e-6 * max(abs(want), 1.0), (li, fd, want)


@pytest.mark.parametrize('name,W,H,T', ALL)
def test_plain_fp32_evaluation_stays_a_tenth_of_the_gpu_ceiling(name, W, H, T):
    weights, kw = _inputs(name, W, H, T)
    ref = _f64(name, W, H, T)
    f32 = F.rollout(weights, dtype=torch.float32, **kw)
    err = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(f32['grads'], ref['grads'])]
    print(f'field_step {name} {W}x{H} T={T}: fp32 torch', ' '.join(f'{e:.3e}' for e in err), f'(of max|grad_f64|; ceiling {GPU_TOL / 10:.0e})')
    assert all(e <= GPU_TOL / 10 for e in err), err


def test_the_deposit_path_matters():
    """Without the path through the field (winners' cells all -1) the gradient is another one: the tests above see the new ground."""
    name, W, H, T = 'two_layers', 24, 68, 3
    weights, kw = _inputs(name, W, H, T)
    ref = _f64(name, W, H, T)
    cut = dict(kw, cells=[np.full_like(cl, -1) for cl in kw['cells']])
    other = F.rollout(weights, **cut)
    assert max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(other['grads'], ref['grads'])) > 100 * GPU_TOL


# ---- the library's new symbols
def test_new_symbols_exported_under_abi_24(lib):
    so = C.CDLL(lib.LIB_PATH)
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    for name in NEW:
        assert hasattr(so, name) and name in lib.EXPORTS, name


def _cells(lib, *, null=None, W=24, H=40, epoch=2, N=10, owner=FAKE, gW=0, null_array=None):
    L = lib
    m = L.Medium(W, H, L.DIE_F32, epoch, owner, FAKE, FAKE, FAKE + 8, gW, gW, 0, 0, 0, 0, 0, 0, None)
    ag = L.Agents(N, None if null_array == 'x' else FAKE, FAKE + 4096, None if null_array == 'alive' else FAKE + 8192, None, None)
    a = dict(m=C.byref(m), ag=C.byref(ag), out=FAKE + 65536)
    if null:
        a[null] = None
    return L.lib.die_deposit_cells(a['m'], a['ag'], a['out'], None)


def _bwd(lib, *, W=24, H=40, sigma=0.8, decay=0.1, N=10, null=None, alias=None):
    a = dict(g=FAKE, cells=FAKE + 65536, gc=FAKE + 2 * 65536, gd=FAKE + 3 * 65536)
    if null:
        a[null] = None
    if alias == 'plane':
        a['gc'] = a['g']
    elif alias:
        a['gd'] = a[alias]
    return lib.lib.die_env_step_backward(W, H, a['g'], sigma, decay, N, a['cells'], a['gc'], a['gd'], None)


@pytest.mark.parametrize('case, call, kw, status, needle', [
    ('cells: null medium', _cells, dict(null='m'), ARG, b'null argument'),
    ('cells: null agents', _cells, dict(null='ag'), ARG, b'null argument'),
    ('cells: null output', _cells, dict(null='out'), ARG, b'null argument'),
    ('cells: empty field', _cells, dict(W=0), ARG, b'bad size'),
    ('cells: epoch 0', _cells, dict(epoch=0), ARG, b'bad epoch'),
    ('cells: epoch 32', _cells, dict(epoch=32), ARG, b'bad epoch'),
    ('cells: no claim plane', _cells, dict(owner=None), ARG, b'null claim plane'),
    ('cells: negative count', _cells, dict(N=-1), ARG, b'bad slot count'),
    ('cells: more slots than a claim word names', _cells, dict(N=1 << 27), ARG, b'bad slot count'),
    ('cells: null coordinates', _cells, dict(null_array='x'), ARG, b'bad arrays'),
    ('cells: null alive flags', _cells, dict(null_array='alive'), ARG, b'bad arrays'),
    ('cells: a decomposed medium', _cells, dict(gW=64), UNSUPPORTED, b'decomposed'),
    ('cells: 2^32 cells', _cells, dict(W=1 << 16, H=1 << 16), UNSUPPORTED, b'int32 cell index'),
    ('backward: null incoming gradient', _bwd, dict(null='g'), ARG, b'null argument'),
    ('backward: null grad_chem', _bwd, dict(null='gc'), ARG, b'null argument'),
    ('backward: empty field', _bwd, dict(H=0), ARG, b'bad size'),
    ('backward: negative field', _bwd, dict(W=-3), ARG, b'bad size'),
    ('backward: in place', _bwd, dict(alias='plane'), ARG, b'in-place grad_chem'),
    ('backward: sigma 0', _bwd, dict(sigma=0.0), ARG, b'sigma must be positive'),
    ('backward: sigma nan', _bwd, dict(sigma=float('nan')), ARG, b'sigma must be positive'),
    ('backward: an empty kernel', _bwd, dict(sigma=0.1), ARG, b'empty kernel'),
    ('backward: radius 9', _bwd, dict(sigma=2.2), UNSUPPORTED, b'radius'),
    ('backward: decay nan', _bwd, dict(decay=float('nan')), ARG, b'decay'),
    ('backward: negative count', _bwd, dict(N=-1), ARG, b'bad entry count'),
    ('backward: entries without cells', _bwd, dict(null='cells'), ARG, b'null cells'),
    ('backward: grad_deposit is grad_chem', _bwd, dict(alias='gc'), ARG, b'in-place grad_deposit'),
    ('backward: grad_deposit is the incoming gradient', _bwd, dict(alias='g'), ARG, b'in-place grad_deposit'),
    ('backward: grad_deposit is the cells', _bwd, dict(alias='cells'), ARG, b'in-place grad_deposit'),
    ('backward: 2^32 cells', _bwd, dict(W=1 << 16, H=1 << 16), UNSUPPORTED, b'int32 cell index'),
])
def test_bad_arguments_refused_before_launch(lib, case, call, kw, status, needle):
    assert call(lib, **kw) == status, (case, lib.lib.die_last_error())
    assert needle in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


def test_no_entries_launch_nothing_in_die_deposit_cells(lib):
    assert _cells(lib, N=0, null_array='x') == 0         # fake pointers again: a launch would have failed


# ---- the Python refusals, on host objects (Env's constructors need a GPU; an Env around host arrays is put together by hand)
def _host_env(dynamics=None, dtype=torch.float32, N=5):
    import die_amd as die
    from die_amd.device_array import DeviceAgents, DeviceMedium
    env = die.Env.__new__(die.Env)
    env.dynamics = dynamics or die.Dynamics()
    env.device = torch.device('cpu')
    env.medium = DeviceMedium((8, 12), 'cpu', dtype)
    env.agents = DeviceAgents(N, 'cpu')
    return env


@pytest.mark.parametrize('what, kw', [
    ('fp16 fields', dict(dtype=torch.float16)),
    ('a non-periodic gaussian', dict(dynamics=dict(diffuse_mode='reflect'))),
    ('the sense mask', dict(dynamics=dict(apply_sense_mask=True))),
    ('the frozen indexer', dict(dynamics=dict(agents_die=True, compat='reference'))),
    ('a decomposed medium', dict(world=(16, 24, 0, 0))),
])
def test_python_refusals_raise_before_anything_is_touched(lib, what, kw):
    import die_amd as die
    kw = dict(kw)
    world = kw.pop('world', None)
    if 'dynamics' in kw:
        kw['dynamics'] = die.Dynamics(**kw['dynamics'])
    env = _host_env(**kw)
    env.medium.world = world
    epoch = env.medium.epoch
    action = torch.zeros((3, 5), dtype=torch.float32)
    with pytest.raises(NotImplementedError, match='differentiable_step'):
        env.differentiable_step(action)
    with pytest.raises(NotImplementedError, match='differentiable_chem'):
        env.differentiable_chem()
    assert env.medium.chem_node is None and env.medium.epoch == epoch


@pytest.mark.parametrize('action', [torch.zeros((3, 4)), torch.zeros((2, 5)), torch.zeros((3, 5), dtype=torch.float64), torch.zeros(15),
                                    np.zeros((3, 5), dtype=np.float32), torch.zeros((3, 5), device='meta')])
def test_a_wrong_action_is_refused(lib, action):
    env = _host_env()
    with pytest.raises(NotImplementedError, match='action must be'):
        env.differentiable_step(action)
    assert env.medium.chem_node is None and env.medium.epoch == 1


def test_agents_die_intended_and_a_chem_node_on_the_host(lib):
    import die_amd as die
    env = _host_env(dynamics=die.Dynamics(agents_die=True))
    env._check_differentiable('differentiable_step')                  # allowed: the lifecycle does not enter the chem adjoint
    node = env.differentiable_chem()
    assert node is env.differentiable_chem() and not node.requires_grad and node.is_leaf and node.dtype == torch.float32
    assert node.data_ptr() != env.medium.chem.data_ptr() and torch.equal(node, env.medium.chem)
    env.medium.upload_channel('chem1', np.ones((8, 12)))
    assert env.medium.chem_node is None
