"""Wide NeuralAutomataAgent stacks (ConvolutionModel(hidden_channels=C, hidden_activation=...)), CPU side: the float64 model of
tests/nca_wide_model.py against torch's fp32 evaluation of the new module, the defaults unchanged, save / load, the refusals, and
the three new entry points under the unchanged ABI version.  No kernel is launched here."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch
from torch.nn.utils import parameters_to_vector

from tests import nca_wide_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('die_conv2d_wide', 'die_nca_wide_batch_scratch_bytes', 'die_nca_wide_env_step_batch')
STACKS = [(3, 3), (3, 1, 3), (5, 3), (3, 5, 3)]
WIDTHS = [5, 16, 17, 32]


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location('die_build', os.path.join(ROOT, 'die_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    from die_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def evo(lib):
    from die_amd.agent import evo
    return evo


# ---------------------------------------------------------------------------------------------------- 1. model against torch
@pytest.mark.parametrize('boundary', ['circular', 'zeros', 'reflect', 'replicate'])
@pytest.mark.parametrize('activation', [None, 'tanh', 'relu'])
@pytest.mark.parametrize('W,H', [(12, 8), (30, 50), (96, 96)])
def test_model_is_torchs_fp32_forward(evo, W, H, activation, boundary):
    """Tolerance 1e-5 absolute, the project's parity tolerance (tests/test_gpu_parity.py).  Torch's fp32 error against float64,
    measured over this table (every field, stack, width, activation and boundary): at most 6.8e-7."""
    rs = np.random.RandomState(W * 31 + H)
    x = rs.rand(3, W, H).astype(np.float32)                       # inputs in [0, 1)
    worst = 0.0
    for sizes in STACKS:
        for width in WIDTHS:
            torch.manual_seed(width * 7 + len(sizes))
            model = evo.ConvolutionModel(kernel_sizes=sizes, boundary=boundary, hidden_channels=width, hidden_activation=activation)
            model.init_weights()                                  # Xavier
            convs = model.conv_layers()
            assert [tuple(k.weight.shape[:2]) for k in convs] == \
                [(width, 3)] + [(width, width)] * (len(sizes) - 2) + [(3, width)]
            with torch.no_grad():
                got = model.eval()(torch.from_numpy(x)[None])[0].numpy()
            want = M.sense(x, [k.weight.detach().numpy() for k in convs], activation, boundary)
            err = float(np.abs(got - want).max())
            worst = max(worst, err)
            assert err <= 1e-5, (sizes, width, err)
    print(f'{W}x{H} {activation} {boundary}: torch fp32 against the float64 model: {worst:.2e}')


def test_model_pads_as_torch_pads():
    """np.pad's four modes are torch's four padding modes (asymmetric data, so that a mirrored or shifted pad shows)."""
    rs = np.random.RandomState(1)
    x = rs.rand(2, 7, 9)
    w = rs.rand(3, 2, 5, 5)
    for boundary in M.NP_PAD:
        conv = torch.nn.Conv2d(2, 3, 5, padding='same', padding_mode=boundary, bias=False, dtype=torch.float64)
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(w))
            want = conv(torch.from_numpy(x)[None])[0].numpy()
        assert np.allclose(M.conv(x, w, boundary), want, rtol=0, atol=1e-12), boundary


# ---------------------------------------------------------------------------------------------------- 2. defaults unchanged
def test_defaults_are_todays_module(evo):
    model = evo.ConvolutionModel()
    assert list(model.state_dict()) == ['kernels.0.weight']
    assert [type(m).__name__ for m in model.kernels] == ['Conv2d', 'Tanh']
    assert sorted(model._init_params) == ['boundary', 'kernel_sizes', 'num_act_channels', 'num_obs_channels', 'p_agent_dropout',
                                          'requires_grad']
    assert parameters_to_vector(model.parameters()).numel() == 3 * 3 * 9 and not model.wide
    ag = evo.NeuralAutomataAgent(kernel_sizes=[3, 3])
    assert list(ag.model.state_dict()) == ['kernels.0.weight', 'kernels.1.weight']
    assert [type(m).__name__ for m in ag.model.kernels] == ['Conv2d', 'Conv2d', 'Tanh']
    assert sorted(ag.init_params) == ['deposit', 'model_kwargs', 'scale', 'with_agent_channel']
    assert ag.init_params['model_kwargs'] == {'kernel_sizes': [3, 3]}
    assert parameters_to_vector(ag.model.parameters()).numel() == 2 * 81 and not ag.model.wide
    # None given in so many words is the default too: nothing new in the saved arguments
    ag = evo.NeuralAutomataAgent(kernel_sizes=[3, 3], hidden_channels=None, hidden_activation=None)
    assert ag.init_params['model_kwargs'] == {'kernel_sizes': [3, 3]} and not ag.model.wide


def test_wide_module_layout(evo):
    ag = evo.NeuralAutomataAgent(kernel_sizes=[3, 3, 3], hidden_channels=16, hidden_activation='relu', with_agent_channel=False)
    assert [type(m).__name__ for m in ag.model.kernels] == ['Conv2d', 'ReLU', 'Conv2d', 'ReLU', 'Conv2d', 'Tanh']
    assert [tuple(k.weight.shape) for k in ag.model.conv_layers()] == [(16, 2, 3, 3), (16, 16, 3, 3), (3, 16, 3, 3)]
    assert ag.model.wide and ag.init_params['model_kwargs'] == dict(kernel_sizes=[3, 3, 3], hidden_channels=16, hidden_activation='relu')
    ag = evo.NeuralAutomataAgent(kernel_sizes=[3, 3, 3], hidden_channels=16)
    assert parameters_to_vector(ag.model.parameters()).numel() == 3168              # 3 -> 16 -> 16 -> 3, 3 x 3 kernels
    assert list(ag.model.state_dict()) == ['kernels.0.weight', 'kernels.1.weight', 'kernels.2.weight']
    only_act = evo.ConvolutionModel(kernel_sizes=(3, 3), hidden_activation='tanh')  # an activation alone is a wide stack of width 3
    assert only_act.wide and [tuple(k.weight.shape[:2]) for k in only_act.conv_layers()] == [(3, 3), (3, 3)]


# ---------------------------------------------------------------------------------------------------- 3. save / load
def test_save_then_load_restores_a_wide_agent(evo):
    torch.manual_seed(3)
    ag = evo.NeuralAutomataAgent(scale=0.02, deposit=1.5, kernel_sizes=[3, 1, 3], hidden_channels=17, hidden_activation='tanh')
    ag.model.init_weights()
    buf = io.BytesIO()
    ag.save(buf)
    buf.seek(0)
    back = evo.NeuralAutomataAgent.load(buf)
    assert back.model.hidden_channels == 17 and back.model.hidden_activation == 'tanh' and back.action_coefs == ag.action_coefs
    assert [type(m).__name__ for m in back.model.kernels] == [type(m).__name__ for m in ag.model.kernels]
    for p, q in zip(back.model.parameters(), ag.model.parameters()):
        assert torch.equal(p, q)
    assert back.init_params == ag.init_params


# ---------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals(evo):
    for bad in (0, 33, -1, 2.5, True):
        with pytest.raises(ValueError, match='hidden_channels'):
            evo.ConvolutionModel(kernel_sizes=(3, 3), hidden_channels=bad)
    for bad in ('gelu', 'none', 1):
        with pytest.raises(ValueError, match='hidden_activation'):
            evo.ConvolutionModel(kernel_sizes=(3, 3), hidden_activation=bad)
    with pytest.raises(ValueError, match='two layers'):
        evo.ConvolutionModel(kernel_sizes=(3,), hidden_channels=8)
    with pytest.raises(ValueError, match='two layers'):
        evo.NeuralAutomataAgent(kernel_sizes=[5], hidden_channels=8)
    for kw in (dict(hidden_channels=8), dict(hidden_activation='relu')):
        with pytest.raises(NotImplementedError, match='kernel size 7'):
            evo.NeuralAutomataAgent(kernel_sizes=[7, 3], **kw)
    evo.NeuralAutomataAgent(kernel_sizes=[7, 3])                  # (the narrow stack keeps its 7)


# ---------------------------------------------------------------------------------------------------- 5. ABI
def test_new_symbols_declared_exported_and_bound_under_abi_24(lib):
    header = open(os.path.join(ROOT, 'include', 'die_hip.h')).read()
    so = C.CDLL(lib.LIB_PATH)
    assert lib.ABI_VERSION == 24 and lib.lib.die_abi_version() == 24
    assert re.search(r'#define\s+DIE_ABI_VERSION\s+24\b', header)
    for name in NEW:
        assert re.search(r'\b(int|int64_t)\s+' + name + r'\(', header), name
        assert hasattr(so, name) and name in lib.EXPORTS and getattr(lib.lib, name).argtypes is not None, name
    # the structs the new calls take are the existing ones: die_nca_layer {4 x int32, pointer, int64}, die_nca_batch
    # {4 x int32, pointer, 3 x float, int32, pointer, int64}, die_conv_plane {pointer, 2 x int32}, die_nca_dropout
    assert C.sizeof(lib.NcaLayer) == 16 + 8 + 8 and C.sizeof(lib.NcaBatch) == 16 + 8 + 12 + 4 + 8 + 8
    assert C.sizeof(lib.ConvPlane) == 16 and C.sizeof(lib.NcaDropout) == 32
    assert lib.NcaLayer.reserved.offset == 12                     # the word die_nca_wide_env_step_batch reads as the activation
    m = re.search(r'DIE_NCA_ACT_NONE = (\d), DIE_NCA_ACT_TANH = (\d), DIE_NCA_ACT_RELU = (\d)', header)
    assert m and [int(g) for g in m.groups()] == [lib.NCA_ACTIVATIONS[k] for k in (None, 'tanh', 'relu')]
    assert lib.NCA_WIDE_MAX_CHANNELS == 32 and lib.NCA_WIDE_KERNEL_SIZES == (1, 3, 5)


def test_wide_scratch_bytes(lib):
    f = lib.lib.die_nca_wide_batch_scratch_bytes
    assert f(96, 96, 16, 3, 16) == 2 * 16 * 16 * 96 * 96 * 4
    assert f(30, 50, 4, 2, 32) == 2 * 4 * 32 * 30 * 50 * 4
    assert f(30, 50, 4, 1, 3) == 1 * 4 * 3 * 30 * 50 * 4          # one layer: one set
    assert f(12, 8, 64, 8, 1) == 2 * 64 * 12 * 8 * 4
    for bad in ((0, 8, 1, 2, 4), (8, 0, 1, 2, 4), (8, 8, 0, 2, 4), (8, 8, 65, 2, 4), (8, 8, 1, 0, 4), (8, 8, 1, 9, 4),
                (8, 8, 1, 2, 0), (8, 8, 1, 2, 33)):
        assert f(*bad) == -1, bad
