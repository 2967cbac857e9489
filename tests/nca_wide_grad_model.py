"""TEST INFRASTRUCTURE ONLY: a float64 numpy model of one WIDE layer's adjoint, as include/die_hip.h states it for
die_conv2d_wide_backward, and the list of cases the tests run (tests/test_nca_wide_grad_cpu.py for the model itself and the fp32
yardstick of every case, tests/test_gpu_nca_wide_grad.py on the device).  The layer and its adjoint are
tests/conv_adjoint_model.py's, which is generic in the channel count; what is added here is the epilogue's adjoint

    g_z = g * mask * act'(t),   act'(t) = 1 - t^2 (tanh), t > 0 ? 1 : 0 (relu: torch's convention, from the stored output), 1 (none)

with t = act(z) an INPUT of the model: the tests hand it the fp32 forward output of the case they check (the device's on the device,
the fp32 evaluation's on the CPU), so relu's kink cannot split the model and what it is compared with.  The mask is
tests/dropout_model.mask, the project's twin of die_rng.h."""
import zlib

import numpy as np

from tests.conv_adjoint_model import SHAPES, _padded, conv, conv_backward, occupancy  # noqa: F401  (re-exported for the tests)
from tests import conv_adjoint_model as A
from tests import dropout_model as M

KS = (1, 3, 5)
MODES = ('circular', 'zeros')
# the chunk-of-4 edge, the 16 / 17 block edge, and a stack's first and last layers
PAIRS = ((1, 1), (3, 16), (16, 3), (4, 5), (5, 4), (17, 16), (16, 17), (32, 32))
ACTIVATIONS = (None, 'tanh', 'relu')
# activation x mask, crossed over these only
X_SHAPES = ((2, 3), (17, 66), (33, 130))
X_PAIRS = ((3, 16), (17, 16), (32, 32))
X_KS = (3, 5)
DROP_P, DROP_STEP = 0.25, 3

# Cases drawn again, as tests/conv_adjoint_model.REDRAWN does and for its reason: an array of ONE element (the single weight
# gradient of a 1 -> 1, k = 1 layer) that happens to cancel makes "error over max|.|" meaningless, and a plain fp32 evaluation of
# the first draw missed the 1e-5 yardstick there.  Other inputs, not another ceiling.
REDRAWN = dict(A.REDRAWN)


def case_inputs(k: int, mode: str, cin: int, cout: int, W: int, H: int):
    """tests/conv_adjoint_model.case_inputs (the same seeds, the same draws) with this module's REDRAWN on top."""
    draw = REDRAWN.get((k, mode, cin, cout, W, H), 0)
    if draw == A.REDRAWN.get((k, mode, cin, cout, W, H), 0):
        return A.case_inputs(k, mode, cin, cout, W, H)
    seed = zlib.crc32(f'{k} {mode} {cin} {cout} {W} {H}'.encode() + f' draw {draw}'.encode())
    rs = np.random.RandomState(seed)
    return dict(seed=seed,
                x=rs.rand(cin, W, H).astype(np.float32),
                w=rs.uniform(-0.5, 0.5, (cout, cin, k, k)).astype(np.float32),
                g=rs.standard_normal((cout, W, H)).astype(np.float32))


def layer_cases(k: int, mode: str):
    """(cin, cout, W, H, activation, masked) of every case at kernel size k and padding `mode`: every pair on every shape plain,
    and the activation x mask cross over X_SHAPES x X_PAIRS at k in X_KS."""
    out = [(cin, cout, W, H, None, False) for W, H in SHAPES for cin, cout in PAIRS]
    if k in X_KS:
        out += [(cin, cout, W, H, act, masked) for W, H in X_SHAPES for cin, cout in X_PAIRS for act in ACTIVATIONS
                for masked in (False, True) if act is not None or masked]
    return out


def act_forward(z, activation):
    z = np.asarray(z)
    return z if activation is None else np.tanh(z) if activation == 'tanh' else np.maximum(z, 0)


def act_derivative(t, activation) -> np.ndarray:
    """act'(z) from t = act(z), float64."""
    t = np.asarray(t, dtype=np.float64)
    if activation is None:
        return np.ones_like(t)
    if activation == 'tanh':
        return 1.0 - t * t
    if activation == 'relu':
        return (t > 0).astype(np.float64)
    raise ValueError(activation)


def case_mask(c, W: int, H: int, masked: bool):
    """The (W, H) float32 mask of a masked case (key: the case's seed; DROP_STEP, DROP_P), or None."""
    return M.mask(c['seed'], DROP_STEP, W, H, DROP_P) if masked else None


def layer_backward(x, w, g, t, activation=None, mask=None, mode: str = 'circular'):
    """(grad_w, grad_in) of <act(conv(x, w)) * mask, g>, float64, with t = act(conv(x, w)) given (None: activation None)."""
    g = np.asarray(g, dtype=np.float64)
    gz = g if mask is None else g * np.asarray(mask, dtype=np.float64)[None]
    if activation is not None:
        gz = gz * act_derivative(t, activation)
    return conv_backward(x, w, gz, mode)


# ------------------------------------------------------------------------------------------------- whole stacks (forward_device)
# (hidden_channels, kernel_sizes, hidden_activation, seed) of the stacks ConvolutionModel.forward_device is checked on, each on
# STACK_FIELDS.  The relu stack's weights and planes are drawn on binary grids (weights in sixteenths, the field planes in quarters,
# the claim plane 0 / 1), so that every hidden pre-activation is a small multiple of 2^-10, computed EXACTLY in fp32 and in float64
# alike: it is either exactly zero — where relu' is 0 in torch's convention and in the kernel's — or at least 2^-10 away from the
# kink, far more than 1e-4 of the largest (tests/test_nca_wide_grad_cpu.py asserts it).  The kink cannot hide a failure.
STACKS = ((8, (3, 3), 'tanh', 801), (16, (3, 5, 3), 'relu', 1601), (32, (1, 3), None, 3201))
STACK_FIELDS = ((17, 66), (40, 136))
STACK_DROP = (0.25, 77)                                          # (p, dropout_seed) of the masked evaluations, at dropout_step 0 and 1


def stack_case(width: int, kernel_sizes, activation, seed: int, W: int, H: int):
    """(planes (3, W, H) float32: occupancy, food, chem; weights: one float32 (cout, cin, k, k) array per layer; the gradient at
    the stack's output (3, W, H) float32)."""
    from tests import nca_wide_model as NW
    rs = np.random.RandomState(seed + 7 * W + H)
    occ = (rs.rand(W, H) < 0.3).astype(np.float32)
    fields = rs.rand(2, W, H).astype(np.float32)
    weights = NW.stack_weights(rs, kernel_sizes, width)
    if activation == 'relu':
        fields = (np.floor(fields * 4) / 4).astype(np.float32)
        weights = [(np.round(w * 16) / 16).astype(np.float32) for w in weights]
    g = rs.standard_normal((3, W, H)).astype(np.float32)
    return np.concatenate([occ[None], fields]), weights, g


def stack_pre_activations(planes, weights, activation, mode: str = 'circular'):
    """The float64 pre-activation z of every layer (the last one's included), hidden activations applied between them."""
    out, z = [], np.asarray(planes, dtype=np.float64)
    for li, w in enumerate(weights):
        z = conv(z, w, mode)
        out.append(z)
        if li < len(weights) - 1:
            z = act_forward(z, activation)
    return out
