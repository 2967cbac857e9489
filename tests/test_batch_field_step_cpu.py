"""The action-driven batched step and the batched step adjoint, CPU side: the five entry points are declared, exported and bound under
the unchanged ABI version; each refuses its bad arguments on the host, naming itself, before any launch (fake pointers: a launch
would have failed); the Python refusals leave a batch as it was; and the float64 model of the batched rollout
(tests/field_step_batch_model.py) is R stand-alone model rollouts, summed per candidate when a candidate has several worlds.
No kernel is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import field_step_adjoint_model as F
from tests import field_step_batch_model as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('die_env_step_batch', 'die_env_step_batch_rows', 'die_deposit_cells_batch', 'die_env_step_backward_batch',
       'die_nca_backward_batch_inputs')
FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host
ARG, UNSUPPORTED = -1, -3
R, N, W, H = 4, 10, 24, 40


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


def test_new_symbols_declared_exported_and_bound_under_abi_24(lib):
    so = C.CDLL(lib.LIB_PATH)
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'die_hip.h')).read(), flags=re.S)
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24 and '#define DIE_ABI_VERSION 24' in header
    for name in NEW:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert hasattr(so, name) and name in lib.EXPORTS, name
        assert getattr(lib.lib, name).restype is C.c_int and getattr(lib.lib, name).argtypes, name


# ---- the library's refusals ---------------------------------------------------------------------------------------------------
def _batch(lib, replicas=R, plane_stride=None, agent_stride=N, n=None, W=W, H=H):
    return lib.Batch(replicas, 0, W * H if plane_stride is None else plane_stride, agent_stride, 1,
                     (C.c_int64 * 64)(*(([N] * 64) if n is None else n)))


def _dyn(lib, sigma=0.8, agents_die=0, mode=0, staged=0):
    return lib.Dynamics(0.1, 0.025, sigma, lib.DIE_BOUNDARY_WRAP, lib.DIE_COST_LINEAR, 0.02, 0.01, 1, agents_die, 0, mode, staged)


def _rows_host(lib, radius=3, n=R):
    rows = (lib.DynamicsRow * 64)()
    for r in range(n):
        rows[r].radius, rows[r].keep, rows[r].rate_feed = radius, 0.9, 0.1
    return rows


def _step(lib, *, rows=False, null=None, act_null=None, ws_bytes=None, H=H, sigma=0.8, gW=0, epoch=2, slot=None, null_rows=None, radius=3,
          agents_die=0, **bk):
    L = lib
    m = L.Medium(W, H, L.DIE_F32, epoch, FAKE, FAKE, FAKE, FAKE + 8, gW, gW, 0, 0, 0, 0, 0, 0, None)
    a = L.Agents(N, FAKE, FAKE, FAKE, FAKE, slot)
    act = L.Action(N, FAKE, FAKE, FAKE)
    if act_null:
        setattr(act, act_null, None)
    d, b = _dyn(L, sigma, agents_die), _batch(L, H=H, **bk)
    args = dict(m=C.byref(m), a=C.byref(a), act=C.byref(act), d=C.byref(d), b=C.byref(b), results=FAKE, ws=FAKE)
    if null:
        args[null] = None
    ws_bytes = L.lib.die_batch_lifecycle_workspace_bytes(R, N) if ws_bytes is None else ws_bytes
    front = (args['m'], args['a'], args['act'], args['d'], args['b'], args['results'], args['ws'], ws_bytes)
    if not rows:
        return L.lib.die_env_step_batch(*front, None)
    dev, host = (None if null_rows == 'rows' else FAKE), (None if null_rows == 'rows_host' else _rows_host(L, radius))
    return L.lib.die_env_step_batch_rows(*front, dev, host, None)


def _step_rows(lib, **kw):
    return _step(lib, rows=True, **kw)


def _cells(lib, *, null=None, H=H, epoch=2, owner=FAKE, gW=0, null_array=None, slot=None, agents=N, **bk):
    L = lib
    m = L.Medium(W, H, L.DIE_F32, epoch, owner, FAKE, FAKE, FAKE + 8, gW, gW, 0, 0, 0, 0, 0, 0, None)
    ag = L.Agents(agents, None if null_array == 'x' else FAKE, FAKE + 4096, None if null_array == 'alive' else FAKE + 8192, None, slot)
    b = _batch(L, H=H, **bk)
    a = dict(m=C.byref(m), ag=C.byref(ag), b=C.byref(b), out=FAKE + 65536)
    if null:
        a[null] = None
    return L.lib.die_deposit_cells_batch(a['m'], a['ag'], a['b'], a['out'], None)


def _bwd(lib, *, H=H, Wd=W, sigma=0.8, decay=0.1, null=None, alias=None, tables=None, radius=3, shift=0, **bk):
    L = lib
    span = 1 << 22                                       # far more than R planes of W x H floats
    a = dict(g=FAKE, cells=FAKE + span, gc=FAKE + 2 * span + shift, gd=FAKE + 3 * span)
    b = _batch(L, W=Wd, H=H, **bk)
    bref = C.byref(b)
    if null == 'b':
        bref = None
    elif null:
        a[null] = None
    if alias == 'plane':
        a['gc'] = a['g']
    elif alias == 'plane_overlap':
        a['gc'] = a['g'] + 4 * W * H                     # replica 1's plane of the incoming gradient
    elif alias:
        a['gd'] = a[alias]
    dev, host = {None: (None, None), 'both': (FAKE + 4 * span, _rows_host(L, radius)), 'device': (FAKE + 4 * span, None),
                 'host': (None, _rows_host(L, radius))}[tables]
    return L.lib.die_env_step_backward_batch(Wd, H, bref, a['g'], sigma, decay, dev, host, a['cells'], a['gc'], a['gd'], None)


def _inputs(lib, *, null=None, grad_in=FAKE + (1 << 24), stride=3 * W * H, alias=None, replicas=R, H=H, ws_short=False):
    L = lib
    m = L.Medium(W, H, L.DIE_F32, 2, FAKE, FAKE + (1 << 16), FAKE + (2 << 16), None, 0, 0, 0, 0, 0, 0, 0, 0, None)
    b = _batch(L, replicas=replicas, H=H)
    layers = (L.NcaLayer * 2)(L.NcaLayer(3, 3, 3, 0, FAKE + (3 << 16), 162), L.NcaLayer(3, 3, 3, 0, FAKE + (3 << 16) + 324, 162))
    nca = L.NcaBatch(2, 0, 1, 2, layers, (C.c_float * 3)(0.01, 0.01, 2.0), 0, None, 0)
    need = L.lib.die_nca_backward_batch_workspace_bytes(W, H, min(max(replicas, 1), 64), 2)
    a = dict(store=FAKE + (4 << 16), g=FAKE + (1 << 22), grad=FAKE + (2 << 22), ws=FAKE + (3 << 22), grad_in=grad_in)
    if null:
        a[null] = None
    if alias:
        a['grad_in'] = a[alias] if alias in a else {'chem': FAKE + (2 << 16), 'weights': FAKE + (3 << 16)}[alias]
    return L.lib.die_nca_backward_batch_inputs(C.byref(m), C.byref(b), C.byref(nca), a['store'], a['g'], 3 * W * H, a['grad'], 162, None, a['ws'],
                                               need - 1 if ws_short else need, a['grad_in'], stride, None)


STEP_CASES = [(f'{who.__name__}: {case}', who, kw, status, needle) for who in (_step, _step_rows) for case, kw, status, needle in [
    ('null medium', dict(null='m'), ARG, b'null argument'),
    ('null agents', dict(null='a'), ARG, b'null argument'),
    ('null action', dict(null='act'), ARG, b'null argument'),
    ('null dynamics', dict(null='d'), ARG, b'null argument'),
    ('null batch', dict(null='b'), ARG, b'null argument'),
    ('null results', dict(null='results'), ARG, b'null argument'),
    ('null workspace', dict(null='ws'), ARG, b'null argument'),
    ('no replica', dict(replicas=0), ARG, b'replicas'),
    ('65 replicas', dict(replicas=65), ARG, b'replicas'),
    ('workspace too small', dict(ws_bytes=100), ARG, b'workspace too small'),
    ('no stash for dead slots', dict(agents_die=1, ws_bytes=4 * 3 * 8192 * 8), ARG, b'workspace too small for dead slots'),
    ('planes overlap', dict(plane_stride=W * H - 1), ARG, b'strides smaller than a replica'),
    ('agent rows overlap', dict(agent_stride=N - 1), ARG, b'strides smaller than a replica'),
    ('H % 4', dict(H=42), UNSUPPORTED, b'H % 4 == 0'),
    ('radius 5', dict(sigma=1.2), UNSUPPORTED, b'radius 1..4'),
    ('a decomposed medium', dict(gW=64), ARG, b'single-tile'),
    ('null dx', dict(act_null='dx'), ARG, b'null action arrays'),
    ('null deposit', dict(act_null='deposit'), ARG, b'null action arrays'),
    ('sorted agents', dict(slot=FAKE), ARG, b'slot order'),
    ('epoch 0', dict(epoch=0), ARG, b'bad medium'),
    ('a replica without agents', dict(n=[N, 0, N, N] + [0] * 60), ARG, b'replica 1 has 0 agents'),
    ('a replica beyond its row', dict(n=[N, N, N + 1, N] + [0] * 60), ARG, b'replica 2 has 11 agents'),
]] + [
    ('_step_rows: no device table', _step_rows, dict(null_rows='rows'), ARG, b'null dynamics rows'),
    ('_step_rows: no host table', _step_rows, dict(null_rows='rows_host'), ARG, b'null host copy'),
    ('_step_rows: a row of radius 5', _step_rows, dict(radius=5), ARG, b'radius 5, outside 1..4'),
]

OTHER_CASES = [
    ('cells: null medium', _cells, dict(null='m'), ARG, b'null argument'),
    ('cells: null agents', _cells, dict(null='ag'), ARG, b'null argument'),
    ('cells: null batch', _cells, dict(null='b'), ARG, b'null argument'),
    ('cells: null output', _cells, dict(null='out'), ARG, b'null argument'),
    ('cells: epoch 0', _cells, dict(epoch=0), ARG, b'bad epoch'),
    ('cells: epoch 32', _cells, dict(epoch=32), ARG, b'bad epoch'),
    ('cells: no claim plane', _cells, dict(owner=None), ARG, b'null claim plane'),
    ('cells: null coordinates', _cells, dict(null_array='x'), ARG, b'bad arrays'),
    ('cells: null alive flags', _cells, dict(null_array='alive'), ARG, b'bad arrays'),
    ('cells: sorted agents', _cells, dict(slot=FAKE), ARG, b'slot order'),
    ('cells: a decomposed medium', _cells, dict(gW=64), UNSUPPORTED, b'decomposed'),
    ('cells: no replica', _cells, dict(replicas=0), ARG, b'replicas'),
    ('cells: 65 replicas', _cells, dict(replicas=65), ARG, b'replicas'),
    ('cells: planes overlap', _cells, dict(plane_stride=W * H - 1), ARG, b'strides smaller than a replica'),
    ('cells: agent rows overlap', _cells, dict(agents=N + 1), ARG, b'strides smaller than a replica'),
    ('cells: no agent row', _cells, dict(agent_stride=0, n=[0] * 64, agents=0), ARG, b'bad agent stride'),
    ('cells: a replica beyond its row', _cells, dict(n=[N, N + 1] + [0] * 62), ARG, b'replica 1 has 11 agents'),
    ('cells: a negative count', _cells, dict(n=[N, N, -1] + [0] * 61), ARG, b'replica 2 has -1 agents'),
    ('backward: null incoming gradient', _bwd, dict(null='g'), ARG, b'null argument'),
    ('backward: null grad_chem', _bwd, dict(null='gc'), ARG, b'null argument'),
    ('backward: null batch', _bwd, dict(null='b'), ARG, b'null argument'),
    ('backward: empty field', _bwd, dict(Wd=0), ARG, b'bad size'),
    ('backward: no replica', _bwd, dict(replicas=0), ARG, b'replicas'),
    ('backward: 65 replicas', _bwd, dict(replicas=65), ARG, b'replicas'),
    ('backward: planes overlap', _bwd, dict(plane_stride=W * H - 4), ARG, b'strides smaller than a replica'),
    ('backward: in place', _bwd, dict(alias='plane'), ARG, b'in-place grad_chem'),
    ('backward: grad_chem is another replica\'s incoming plane', _bwd, dict(alias='plane_overlap'), ARG, b'in-place grad_chem'),
    ('backward: H % 4', _bwd, dict(H=42), UNSUPPORTED, b'H % 4 == 0'),
    ('backward: radius 5', _bwd, dict(sigma=1.2), UNSUPPORTED, b'radius 5'),
    ('backward: an empty kernel', _bwd, dict(sigma=0.1), UNSUPPORTED, b'radius 0'),
    ('backward: sigma 0', _bwd, dict(sigma=0.0), ARG, b'sigma must be positive'),
    ('backward: sigma nan', _bwd, dict(sigma=float('nan')), ARG, b'sigma must be positive'),
    ('backward: decay nan', _bwd, dict(decay=float('nan')), ARG, b'decay'),
    ('backward: the device table alone', _bwd, dict(tables='device'), ARG, b'one dynamics table without the other'),
    ('backward: the host table alone', _bwd, dict(tables='host'), ARG, b'one dynamics table without the other'),
    ('backward: a row of radius 5', _bwd, dict(tables='both', radius=5), UNSUPPORTED, b'radius 5, outside 1..4'),
    ('backward: misaligned planes', _bwd, dict(shift=4), ARG, b'16-byte aligned'),
    ('backward: a plane stride off the alignment', _bwd, dict(plane_stride=W * H + 2), ARG, b'16-byte aligned'),
    ('backward: entries without cells', _bwd, dict(null='cells'), ARG, b'null cells'),
    ('backward: a replica beyond its row', _bwd, dict(n=[N + 1] + [0] * 63), ARG, b'replica 0 has 11 agents'),
    ('backward: grad_deposit is grad_chem', _bwd, dict(alias='gc'), ARG, b'in-place grad_deposit'),
    ('backward: grad_deposit is the incoming gradient', _bwd, dict(alias='g'), ARG, b'in-place grad_deposit'),
    ('backward: grad_deposit is the cells', _bwd, dict(alias='cells'), ARG, b'in-place grad_deposit'),
    ('backward: 2^32 cells', _bwd, dict(Wd=1 << 16, H=1 << 16, plane_stride=1 << 32), UNSUPPORTED, b'int32 cell index'),
    ('inputs: null grad_in', _inputs, dict(null='grad_in'), ARG, b'null argument'),
    ('inputs: null store', _inputs, dict(null='store'), ARG, b'null argument'),
    ('inputs: null workspace', _inputs, dict(null='ws'), ARG, b'null argument'),
    ('inputs: 65 replicas', _inputs, dict(replicas=65), ARG, b'replicas'),
    ('inputs: workspace too small', _inputs, dict(ws_short=True), ARG, b'workspace too small'),
    ('inputs: a stride below the input planes', _inputs, dict(stride=3 * W * H - 4), ARG, b'grad_in_stride'),
    ('inputs: a stride off the alignment', _inputs, dict(stride=3 * W * H + 2), ARG, b'16-byte aligned'),
    ('inputs: misaligned grad_in', _inputs, dict(grad_in=FAKE + (1 << 24) + 4), ARG, b'16-byte aligned'),
    ('inputs: grad_in is the weight gradient', _inputs, dict(alias='grad'), ARG, b'grad_in aliases'),
    ('inputs: grad_in is the incoming gradient', _inputs, dict(alias='g'), ARG, b'grad_in aliases'),
    ('inputs: grad_in is the stored planes', _inputs, dict(alias='store'), ARG, b'grad_in aliases'),
    ('inputs: grad_in is the workspace', _inputs, dict(alias='ws'), ARG, b'grad_in aliases'),
    ('inputs: grad_in is the chem planes', _inputs, dict(alias='chem'), ARG, b'grad_in aliases'),
    ('inputs: grad_in is the weights', _inputs, dict(alias='weights'), ARG, b'grad_in aliases'),
]


@pytest.mark.parametrize('case, call, kw, status, needle', STEP_CASES + OTHER_CASES, ids=[c[0] for c in STEP_CASES + OTHER_CASES])
def test_bad_arguments_refused_before_launch(lib, case, call, kw, status, needle):
    assert call(lib, **kw) == status, (case, lib.lib.die_last_error())
    err = lib.lib.die_last_error()
    assert needle in err, (case, err)
    name = {_step: b'die_env_step_batch:', _step_rows: b'die_env_step_batch_rows:', _cells: b'die_deposit_cells_batch:',
            _bwd: b'die_env_step_backward_batch:', _inputs: b'die_nca_backward_batch_inputs:'}[call]
    assert err.startswith(name), (case, err)


# ---- the Python refusals, on a host batch (BatchedEnv's constructor needs a GPU; one around host tensors is put together by hand)
def _host_batch(dtype=torch.float32, per_replica=False):
    import die_amd as die
    from die_amd.batch import BatchedEnv
    env = BatchedEnv.__new__(BatchedEnv)
    env.dynamics, env._dyn, env._flow_mask, env._rows, env._rows_host = die.Dynamics(), None, None, None, None
    env.R, env.W, env.H, env.Nmax, env.n, env.dtype, env.device = 3, 8, 12, 5, [5, 4, 3], dtype, torch.device('cpu')
    env.per_replica, env._fixed, env.epoch, env._steps, env.chem_node = per_replica, None, 7, 11, None
    env.chem = torch.rand((3, 8, 12)).to(dtype)
    return env


def _untouched(env, node=None):
    return env.epoch == 7 and env._steps == 11 and env.chem_node is node


@pytest.mark.parametrize('action', [torch.zeros((3, 3, 4)), torch.zeros((2, 3, 5)), torch.zeros((3, 3, 5), dtype=torch.float64), torch.zeros(45),
                                    np.zeros((3, 3, 5), dtype=np.float32), torch.zeros((3, 3, 5), device='meta'), None])
def test_a_wrong_action_is_refused_with_the_expected_shape(lib, action):
    env = _host_batch()
    node = env.differentiable_chem()
    for call in (env.step_action, env.differentiable_step):
        with pytest.raises(ValueError, match=r'\(3, 3, 5\) float32'):
            call(action)
    with pytest.raises(ValueError, match=r'contiguous \(3, 3, 5\)'):
        env.step_action(torch.zeros((3, 5, 3)).transpose(1, 2))
    assert _untouched(env, node)


def test_differentiable_refusals_leave_the_batch_as_it_was(lib):
    action = torch.zeros((3, 3, 5))
    env = _host_batch(dtype=torch.float16)
    for call, args in ((env.differentiable_step, (action,)), (env.differentiable_chem, ())):
        with pytest.raises(NotImplementedError, match='fp32 fields only'):
            call(*args)
    assert _untouched(env)
    env = _host_batch(per_replica=True)
    for call, args in ((env.differentiable_step, (action,)), (env.differentiable_chem, ())):
        with pytest.raises(NotImplementedError, match=r'envs\[r\].*stand-alone Env.differentiable_step'):
            call(*args)
    with pytest.raises(NotImplementedError, match='per_replica'):
        env.medium_tensor()
    assert _untouched(env)


def test_a_host_operator_is_refused_before_the_step(lib):
    env = _host_batch()
    node = env.differentiable_chem()
    env.dynamics.op_food_flow = lambda food: food * 0.5
    for call in (env.step_action, env.differentiable_step):
        with pytest.raises(NotImplementedError, match='food-flow operator'):
            call(torch.zeros((3, 3, 5)))
    assert _untouched(env, node)


def test_the_chem_node_on_the_host(lib):
    env = _host_batch()
    node = env.differentiable_chem()
    assert node is env.differentiable_chem() is env.chem_node and not node.requires_grad and node.is_leaf and node.dtype == torch.float32
    assert node.shape == (3, 8, 12) and node.data_ptr() != env.chem.data_ptr() and torch.equal(node, env.chem)
    env._initial, env._flow_k0, env._state = (torch.zeros(1), env.chem, env.chem), None, torch.zeros(1)
    env.reset()                                           # every form of reset drops the node
    assert env.chem_node is None and env._steps == 0 and env.epoch == 1


# ---- the float64 model of the batched rollout ---------------------------------------------------------------------------------
BATCH_CASES = [name for name in sorted(F.CASES) if 'sort_every' not in F.CASES[name] and 'p' not in F.CASES[name]]


def _alone(name, weights, chem0, frames, cells, c, u, sigma, decay=F.DECAY):
    k = F.CASES[name]
    return F.rollout(weights, k['boundary'], chem0, frames, cells, c, u, sigma, decay, with_agent_channel=k.get('with_agent_channel', True))


@pytest.mark.parametrize('name', BATCH_CASES)
@pytest.mark.parametrize('T', [1, 3])
def test_batched_model_is_the_stand_alone_model_replica_by_replica(name, T):
    Wm, Hm, Rm = 24, 68, 3
    k = F.CASES[name]
    weights, chem0, frames, cells, c, u = B.synthetic_batch(name, Wm, Hm, T, Rm)
    assert len({f[0]['cx'].size for f in frames}) == Rm                 # replicas of different sizes
    sigma, decay = [k['sigma'], 0.5, 0.8], [0.1, 0.025, 0.06]            # per-replica Dynamics: both radii
    got = B.rollout(weights, k['boundary'], chem0, frames, cells, c, u, sigma, decay, with_agent_channel=k.get('with_agent_channel', True))
    for r in range(Rm):
        want = _alone(name, weights[r], chem0[r], frames[r], cells[r], c[r], u[r], sigma[r], decay[r])
        assert got['loss'][r] == want['loss']
        assert np.array_equal(got['chem'][r], want['chem']) and np.array_equal(got['action'][r], want['action'])
        for a, b in zip(got['grads'][r], want['grads']):
            assert np.array_equal(a, b), r


def test_batched_model_sums_a_candidates_worlds():
    name, Wm, Hm, T, Cn, E = 'two_layers', 24, 68, 2, 2, 3
    k = F.CASES[name]
    weights, chem0, frames, cells, c, u = B.synthetic_batch(name, Wm, Hm, T, Cn * E, episodes=E)
    assert len(weights) == Cn
    got = B.rollout(weights, k['boundary'], chem0, frames, cells, c, u, k['sigma'], episodes=E)
    for cand in range(Cn):
        alone = [_alone(name, weights[cand], chem0[r], frames[r], cells[r], c[r], u[r], k['sigma']) for r in range(cand * E, cand * E + E)]
        for li, g in enumerate(got['grads'][cand]):
            want = sum(a['grads'][li] for a in alone)
            # float64 sums in another order: a few ulps of the largest term
            assert np.abs(g - want).max() <= 1e-13 * max(np.abs(a['grads'][li]).max() for a in alone), (cand, li)
            assert np.abs(g - alone[0]['grads'][li]).max() > 1e-3 * np.abs(g).max()      # … and it IS a sum, not one world's
    assert np.array_equal(got['loss'], [a for cand in range(Cn) for a in
                                        [_alone(name, weights[cand], chem0[r], frames[r], cells[r], c[r], u[r], k['sigma'])['loss']
                                         for r in range(cand * E, cand * E + E)]])
