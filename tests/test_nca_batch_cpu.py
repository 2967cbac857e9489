"""BatchedNeuralAutomataAgent / die_nca_env_step_batch, CPU side: the library exports the entry point and its scratch query,
the structs match their header field lists, bad arguments are refused on the host before any launch, and the (R, P)
parameter rows round-trip against torch's parameters_to_vector.  No kernel is launched here."""
import ctypes as C
import os

import pytest
import torch
from torch.nn.utils import parameters_to_vector

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


def test_entry_point_and_scratch_query_exported(lib):
    so = C.CDLL(lib.LIB_PATH)
    assert hasattr(so, 'die_nca_env_step_batch') and hasattr(so, 'die_nca_batch_scratch_bytes')
    assert 'die_nca_env_step_batch' in lib.EXPORTS and 'die_nca_batch_scratch_bytes' in lib.EXPORTS
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    q = lib.lib.die_nca_batch_scratch_bytes
    # [set][replica][4][W][H] fp32: two ping-pong sets from two layers on, one for a single layer
    assert q(96, 96, 16, 2) == 2 * 16 * 4 * 96 * 96 * 4
    assert q(96, 96, 16, 3) == q(96, 96, 16, 2)
    assert q(64, 48, 5, 1) == 5 * 4 * 64 * 48 * 4
    for bad in ((0, 8, 1, 1), (8, 0, 1, 1), (8, 8, 0, 1), (8, 8, 65, 1), (8, 8, 1, 0), (8, 8, 1, lib.NCA_MAX_LAYERS + 1)):
        assert q(*bad) == -1, bad


def test_struct_sizes_follow_header(lib):
    # die_nca_layer: k, cin, cout, reserved (4 x i32), weights pointer, weight_stride i64
    assert C.sizeof(lib.NcaLayer) == 4 * 4 + 8 + 8
    # die_nca_batch: n_layers, padding_mode, with_agent_channel, sense_epoch, layers pointer, coef[3] + reserved, scratch, scratch_bytes
    assert C.sizeof(lib.NcaBatch) == 4 * 4 + 8 + 3 * 4 + 4 + 8 + 8
    assert C.sizeof(lib.Batch) == 8 + 8 + 8 + 8 + 64 * 8                 # reused unchanged


FAKE = 1 << 20                       # never dereferenced: every call below is refused on the host


def _call(lib, *, layers=((3, 3, 3), (3, 3, 3)), replicas=4, scratch_bytes=None, null=None, W=96, H=96, sense_epoch=1, epoch=2):
    L = lib
    m = L.Medium(W, H, L.DIE_F32, epoch, FAKE, FAKE, FAKE, FAKE + 8, 0, 0, 0, 0, 0, 0, 0, 0, None)
    a = L.Agents(10, FAKE, FAKE, FAKE, FAKE, None)
    arr = (L.NcaLayer * len(layers))(*[L.NcaLayer(k, cin, cout, 0, FAKE, cout * cin * k * k) for k, cin, cout in layers])
    need = L.lib.die_nca_batch_scratch_bytes(W, H, replicas, len(layers)) if 1 <= replicas <= 64 else 1 << 30
    nca = L.NcaBatch(len(layers), 0, 1, sense_epoch, arr, (C.c_float * 3)(0.01, 0.01, 2.0), 0, FAKE,
                     need if scratch_bytes is None else scratch_bytes)
    d = L.Dynamics(0.1, 0.025, 0.8, 0, 0, 0.02, 0.01, 1, 0, 0, 0, 0)
    b = L.Batch(replicas, 0, W * H, 10, 1, (C.c_int64 * 64)(*([10] * 64)))
    ws_bytes = 64 * L.lib.die_batch_workspace_bytes(1)
    args = dict(m=C.byref(m), a=C.byref(a), nca=C.byref(nca), act=None, d=C.byref(d), b=C.byref(b), results=FAKE, ws=FAKE)
    if null:
        args[null] = None
    return L.lib.die_nca_env_step_batch(args['m'], args['a'], args['nca'], args['act'], args['d'], args['b'], args['results'],
                                        args['ws'], ws_bytes, None)


@pytest.mark.parametrize('case, kw, needle', [
    ('null medium', dict(null='m'), b'null argument'),
    ('null stack', dict(null='nca'), b'null argument'),
    ('null results', dict(null='results'), b'null argument'),
    ('null workspace', dict(null='ws'), b'null argument'),
    ('even kernel', dict(layers=((4, 3, 3),)), b'kernel size 4'),
    ('kernel above 7', dict(layers=((9, 3, 3),)), b'kernel size 9'),
    ('five channels', dict(layers=((3, 3, 5), (3, 5, 3))), b'channels'),
    ('no replica', dict(replicas=0), b'replicas'),
    ('65 replicas', dict(replicas=65), b'replicas'),
    ('scratch too small', dict(scratch_bytes=1024), b'scratch too small'),
    ('last layer not 3 planes', dict(layers=((3, 3, 2),)), b'last layer'),
    ('claims not one epoch after sensing', dict(sense_epoch=3, epoch=3), b'epoch'),
])
def test_bad_arguments_refused_before_launch(lib, case, kw, needle):
    assert _call(lib, **kw) == -1, case
    assert needle in lib.lib.die_last_error(), (case, lib.lib.die_last_error())


def test_epoch_wrap_is_accepted_by_the_check_order(lib):
    """Sensing at the last epoch tag and claiming at tag 1 is the wrap, not an error: the call then fails later, on the
    (deliberately) too small scratch — proof that the epoch rule let it through."""
    assert _call(lib, sense_epoch=lib.OWNER_EPOCH_MAX, epoch=1, scratch_bytes=8) == -1
    assert b'scratch too small' in lib.lib.die_last_error()


@pytest.mark.parametrize('kernel_sizes, with_agents', [((3, 3), True), ((3,), True), ((5, 3, 1), False)])
def test_parameter_rows_round_trip(lib, kernel_sizes, with_agents):
    from die_amd import NeuralAutomataAgent
    from die_amd.batch import BatchedNeuralAutomataAgent as B
    torch.manual_seed(0)
    agents = [NeuralAutomataAgent(scale=0.01, deposit=2.0, with_agent_channel=with_agents, kernel_sizes=kernel_sizes) for _ in range(3)]
    for ag in agents:
        ag.model.init_weights()
    rows = B.pack(agents)
    nobs, L = (3 if with_agents else 2), len(kernel_sizes)
    assert rows.shape == (3, sum(k * k * nobs * (nobs if i < L - 1 else 3) for i, k in enumerate(kernel_sizes)))
    for r, ag in enumerate(agents):
        assert torch.equal(rows[r], parameters_to_vector(ag.model.parameters()).detach())
        back = B.unpack(agents[0], rows[r])
        assert back is not ag and back.init_params == ag.init_params
        for p, q in zip(back.model.parameters(), ag.model.parameters()):
            assert torch.equal(p, q)
        assert torch.equal(parameters_to_vector(back.model.parameters()), rows[r])
    rng = torch.get_rng_state()
    B.unpack(agents[0], rows[0])
    assert torch.equal(rng, torch.get_rng_state())                    # the throw-away initial weights draw from a forked RNG
