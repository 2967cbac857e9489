"""TEST INFRASTRUCTURE ONLY: the float64 reference of the conv adjoints at many tiles (tests/test_gpu_grad_midsize.py) and the list of
its cases.  The numpy models of tests/conv_adjoint_model.py and tests/nca_wide_grad_model.py take seconds to minutes on
514 x 512 x 32 channels, so the linear part — (grad_w, grad_in) of <conv(x, w), g_z> — is torch's float64 conv2d autograd on the
CPU here; the epilogue's adjoint g_z = g * mask * act'(t) stays the model's (nca_wide_grad_model.act_derivative), with t the fp32
forward output of whoever is being checked, so relu's kink cannot split the two.  tests/test_grad_midsize_cpu.py holds this
reference to the numpy models at their own small shapes, and shows how far a plain fp32 evaluation of every case strays."""
import numpy as np
import torch

from tests import dropout_model as D
from tests import nca_wide_grad_model as G
from tests.grad_midsize_shapes import CONV_FIELDS

DROP_P, DROP_STEP = G.DROP_P, G.DROP_STEP

# die_conv2d_wide_backward.  'first_layer' reads the claim plane and the fp16 fields of an Env of that size on the device; on the
# CPU its planes are made up in the same kinds (0 / 1, fp16 values).
WIDE_CASES = {
    '32->32 k3 tanh mask circular': dict(k=3, mode='circular', cin=32, cout=32, field='many_tiles', act='tanh', masked=True),
    '17->16 k5 relu zeros ragged': dict(k=5, mode='zeros', cin=17, cout=16, field='ragged', act='relu', masked=False),
    'first layer 3->16 k3': dict(k=3, mode='circular', cin=3, cout=16, field='many_tiles', act=None, masked=False, first_layer=True),
}
# die_conv2d_backward (1..4 channels, k up to 7; its activation is the stack's last tanh)
NARROW_CASES = {
    '4->4 k7 ragged grad_in': dict(k=7, mode='circular', cin=4, cout=4, field='ragged', act=None, masked=False),
    '3->3 k3 tanh mask': dict(k=3, mode='circular', cin=3, cout=3, field='many_tiles', act='tanh', masked=True),
}


def case_inputs(c):
    """dict(seed, x, w, g) of a case: tests/nca_wide_grad_model.case_inputs at the case's field (x uniform in [0, 1), w in +-0.5, g
    standard normal, all float32).  A first layer's x is a 0 / 1 plane and two planes of fp16 values."""
    W, H = CONV_FIELDS[c['field']]
    out = G.case_inputs(c['k'], c['mode'], c['cin'], c['cout'], W, H)
    if c.get('first_layer'):
        x = out['x'].astype(np.float16).astype(np.float32)
        x[0] = out['x'][0] < 0.3
        out = dict(out, x=x)
    return out


def case_mask(c, inputs):
    W, H = CONV_FIELDS[c['field']]
    return D.mask(inputs['seed'], DROP_STEP, W, H, DROP_P) if c['masked'] else None


def conv_adjoint(x, w, gz, mode, dtype=torch.float64):
    """(z = conv(x, w), grad_w, grad_in of <z, gz>) by torch autograd in `dtype`; z in `dtype`, the gradients widened to float64."""
    r = w.shape[-1] // 2
    xt = torch.as_tensor(np.asarray(x), dtype=dtype).clone().requires_grad_(True)
    wt = torch.as_tensor(np.asarray(w), dtype=dtype).clone().requires_grad_(True)
    xp = torch.nn.functional.pad(xt[None], (r, r, r, r), mode='circular' if mode == 'circular' else 'constant') if r else xt[None]
    z = torch.nn.functional.conv2d(xp, wt)[0]
    (z * torch.as_tensor(np.asarray(gz), dtype=dtype)).sum().backward()
    return z.detach().numpy(), wt.grad.to(torch.float64).numpy(), xt.grad.to(torch.float64).numpy()


def upstream(g, t, activation, mask, dtype=np.float64):
    """g_z = g * mask * act'(t) in `dtype` (the float64 model's epilogue adjoint; in float32 what a plain fp32 evaluation forms)."""
    gz = np.asarray(g, dtype=dtype)
    if mask is not None:
        gz = gz * np.asarray(mask, dtype=dtype)[None]
    if activation is not None:
        gz = gz * G.act_derivative(t, activation).astype(dtype) if dtype == np.float64 else \
            gz * (1 - np.asarray(t, dtype=dtype) ** 2 if activation == 'tanh' else (np.asarray(t) > 0).astype(dtype))
    return gz


def reference(x, w, g, t, activation, mask, mode):
    """(z, grad_w, grad_in) in float64 of <act(conv(x, w)) * mask, g> with t = act(conv(x, w)) GIVEN (None where there is no
    activation): nca_wide_grad_model.layer_backward with torch doing the two correlations."""
    return conv_adjoint(x, w, upstream(g, t, activation, mask), mode)


def fp32_evaluation(x, w, g, activation, mask, mode):
    """A plain fp32 evaluation of the same: (t float32 or None, grad_w, grad_in).  torch's fp32 conv on the CPU, nothing of ours."""
    t = None
    if activation is not None:
        t = G.act_forward(conv_adjoint(x, w, np.zeros_like(g), mode, torch.float32)[0], activation).astype(np.float32)
    _, gw, gi = conv_adjoint(x, w, upstream(g, t, activation, mask, np.float32), mode, torch.float32)
    return t, gw, gi
