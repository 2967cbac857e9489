"""The oracle of the differentiable NeuralAutomataAgent (tests/test_nca_grad_cpu.py, tests/test_gpu_nca_grad.py): a plain torch
restatement of what the device computes — bias-free `nn.Conv2d` layers with padding='same' and the padding mode, tanh, the optional
cell mask supplied as a tensor, indexing at given integer cells, times the action coefficients — differentiated by torch's own
autograd.  float64 by default; the same code in float32 is the yardstick for how far a correct fp32 evaluation strays.

The cells are not computed here: callers take them from the project's host twin of die_cell (oracle.cpu_ref.cell), and hand the
claim plane over as a 0/1 plane."""
from typing import Optional, Sequence

import numpy as np
import torch
from torch import nn


def layers(weights: Sequence[np.ndarray], padding_mode: str, dtype=torch.float64):
    """One bias-free 'same'-padded Conv2d per (cout, cin, k, k) array, holding that array."""
    out = []
    for w in weights:
        cout, cin, k, k2 = w.shape
        assert k == k2
        conv = nn.Conv2d(cin, cout, k, padding='same', padding_mode=padding_mode, bias=False, dtype=dtype)
        with torch.no_grad():
            conv.weight.copy_(torch.as_tensor(np.asarray(w), dtype=dtype))
        out.append(conv)
    return out


def sense(convs, planes: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(cin, W, H) → (3, W, H): the layers with nothing between them, tanh, times the (W, H) mask if there is one."""
    z = planes[None]
    for conv in convs:
        z = conv(z)
    s = torch.tanh(z[0])
    return s if mask is None else s * mask


def action(convs, planes: torch.Tensor, cx, cy, coefs, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(3, N): row c is sense[c, cx, cy] · coefs[c] for every slot."""
    s = sense(convs, planes, mask)
    cx, cy = torch.as_tensor(np.asarray(cx), dtype=torch.int64), torch.as_tensor(np.asarray(cy), dtype=torch.int64)
    return s[:, cx, cy] * torch.as_tensor(coefs, dtype=s.dtype)[:, None]


def gradients(weights: Sequence[np.ndarray], padding_mode: str, planes: np.ndarray, cx, cy, coefs, grad_action: np.ndarray,
              mask: Optional[np.ndarray] = None, dtype=torch.float64):
    """(action, [d<action, grad_action> / d weight of every layer]) as numpy float64 arrays, evaluated in `dtype`."""
    convs = layers(weights, padding_mode, dtype)
    m = None if mask is None else torch.as_tensor(np.asarray(mask), dtype=dtype)
    act = action(convs, torch.as_tensor(np.asarray(planes), dtype=dtype), cx, cy, coefs, m)
    (act * torch.as_tensor(np.asarray(grad_action), dtype=dtype)).sum().backward()
    return act.detach().to(torch.float64).numpy(), [c.weight.grad.to(torch.float64).numpy() for c in convs]
