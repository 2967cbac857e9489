"""A float64 numpy model of a wide NeuralAutomataAgent stack (ConvolutionModel(hidden_channels=C, hidden_activation=...)), written
from the definition and from nothing of the device code: every layer is a bias-free 'same'-padded cross-correlation over
(channel, x, y) planes under one of torch's four padding modes (np.pad), every layer but the last is followed by the hidden
activation, the last by tanh; an agent's action is the three output planes at its cell times (scale, scale, deposit).

Checked against torch's own fp32 Conv2d stack in tests/test_nca_wide_cpu.py; the yardstick of tests/test_gpu_nca_wide.py."""
from typing import Optional, Sequence

import numpy as np

from oracle.cpu_ref import cell

NP_PAD = {'circular': 'wrap', 'zeros': 'constant', 'reflect': 'reflect', 'replicate': 'edge'}      # torch padding_mode -> np.pad mode
ACTIVATIONS = {None: lambda z: z, 'tanh': np.tanh, 'relu': lambda z: np.maximum(z, 0.0)}


def conv(x: np.ndarray, w: np.ndarray, boundary: str = 'circular') -> np.ndarray:
    """(cin, W, H), (cout, cin, k, k) -> (cout, W, H): out[o, x, y] = sum_i sum_a sum_b w[o, i, a, b] * pad(in)[i, x + a, y + b]."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    cout, cin, k, k2 = w.shape
    assert k == k2 and k % 2 == 1 and x.shape[0] == cin, (w.shape, x.shape)
    r, (W, H) = k // 2, x.shape[1:]
    xp = np.pad(x, ((0, 0), (r, r), (r, r)), mode=NP_PAD[boundary])
    out = np.zeros((cout, W, H))
    for a in range(k):
        for b in range(k):
            out += np.einsum('oi,ixy->oxy', w[:, :, a, b], xp[:, a:a + W, b:b + H])
    return out


def sense(planes: np.ndarray, weights: Sequence[np.ndarray], hidden_activation: Optional[str] = None, boundary: str = 'circular',
          mask: Optional[np.ndarray] = None) -> np.ndarray:
    """The stack over (cin, W, H) input planes -> (3, W, H); `mask`: an optional (W, H) dropout mask on the outputs."""
    z = np.asarray(planes, dtype=np.float64)
    for li, w in enumerate(weights):
        z = conv(z, w, boundary)
        z = np.tanh(z) if li == len(weights) - 1 else ACTIVATIONS[hidden_activation](z)
    return z if mask is None else z * mask


def read_out(sense_planes: np.ndarray, x, y, scale: float, deposit: float) -> np.ndarray:
    """(3, N): the planes at every slot's cell times (scale, scale, deposit)."""
    W, H = sense_planes.shape[1:]
    return sense_planes[:, cell(x, W), cell(y, H)] * np.array([scale, scale, deposit])[:, None]


def xavier(rs: np.random.RandomState, cout: int, cin: int, k: int) -> np.ndarray:
    """torch.nn.init.xavier_uniform_ of a (cout, cin, k, k) weight, as float32 values."""
    bound = np.sqrt(6.0 / ((cin + cout) * k * k))
    return rs.uniform(-bound, bound, (cout, cin, k, k)).astype(np.float32)


def stack_weights(rs: np.random.RandomState, kernel_sizes: Sequence[int], width: int, cin: int = 3, cout: int = 3):
    """Xavier weights of the layers cin -> width -> ... -> width -> cout."""
    chans = [cin] + [width] * (len(kernel_sizes) - 1) + [cout]
    return [xavier(rs, chans[i + 1], chans[i], k) for i, k in enumerate(kernel_sizes)]
