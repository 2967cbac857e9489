"""TEST INFRASTRUCTURE ONLY: a float64 numpy model of a wide stack's adjoint for R replicas and E episodes per candidate, as
include/die_hip.h states it for die_nca_wide_backward_batch, the byte formulas of that call and of
die_nca_wide_sense_batch_store, and the population cases both test files run (tests/test_nca_wide_grad_batch_cpu.py for the model
itself and the fp32 yardstick, tests/test_gpu_nca_wide_grad_batch.py on the device).

Composed from what is already here: the layer and its forward are tests/nca_wide_model.py's, a layer's adjoint with t = act(z) as an
input is tests/nca_wide_grad_model.layer_backward, the pre-activations come from its stack_pre_activations, and the fold is
tests/nca_grad_batch_model.py's order — a candidate's E replicas outermost, rounded ONCE (here: float64 sums, never rounded).

    t_l = act_l(conv(t_{l-1}, w_l)),  t_{-1} = the planes,  act_l = the hidden activation, tanh for the last layer
    g_L = the gradient at the sense planes;  (grad_w_l, g_{l-1}) = layer_backward(t_{l-1}, w_l, g_l, t_l, act_l, mask on the last)
    row c = sum over e of the flat gradients of replica c * E + e,  flat = the layers' grad_w in parameters_to_vector order
"""
import numpy as np

from tests import nca_grad_batch_model as B
from tests import nca_wide_grad_model as G
from tests import nca_wide_model as NW

TOL = 1e-4                            # the project's ceiling: of max|ref| per layer block
YARDSTICK = 1e-5                      # what a plain fp32 evaluation has to stay under for that ceiling to stand
DROP_P = 0.25
# the smallest that cross the 16 x 64 tile's edges in both axes with H % 4 == 0; the first case also one cell past either edge and
# past two tiles each way
FIELDS = ((24, 72), (20, 136), (17, 68), (33, 132))

# width, kernel sizes, hidden activation, replicas; E episodes, boundary, the agent channel, fp16 fields, dropout (seed, stride),
# fixed slots, per-replica Dynamics.  `field`: index into FIELDS (the first case runs on all four).
CASES = {
    'tanh 8': dict(width=8, sizes=(3, 3), act='tanh', R=3),
    'tanh 8 on 20 x 136': dict(width=8, sizes=(3, 3), act='tanh', R=3, field=1),
    'tanh 8 on 17 x 68': dict(width=8, sizes=(3, 3), act='tanh', R=3, field=2),
    'tanh 8 on 33 x 132': dict(width=8, sizes=(3, 3), act='tanh', R=3, field=3),
    'relu 16 16': dict(width=16, sizes=(3, 5, 3), act='relu', R=2, field=1),
    'none 32 zeros': dict(width=32, sizes=(1, 3), act=None, R=2, boundary='zeros'),
    'tanh 17': dict(width=17, sizes=(3, 3), act='tanh', R=2),
    'tanh 17 zeros': dict(width=17, sizes=(3, 3), act='tanh', R=2, boundary='zeros'),
    'no agent channel': dict(width=8, sizes=(3, 3), act='tanh', R=2, with_agent_channel=False),
    'fp16 fields': dict(width=8, sizes=(3, 3), act='tanh', R=2, f16=True),
    'dropout stride 0': dict(width=8, sizes=(3, 3), act='tanh', R=3, seed=7, stride=0),
    'dropout stride 1': dict(width=8, sizes=(3, 3), act='tanh', R=3, seed=7, stride=1),
    'dropout stride 1 zeros': dict(width=8, sizes=(3, 3), act='tanh', R=3, seed=7, stride=1, boundary='zeros'),
    'fixed slots': dict(width=8, sizes=(3, 3), act='tanh', R=2, fixed=True),
    'per-replica dynamics': dict(width=8, sizes=(3, 3), act='tanh', R=3, rows=True),
    'two episodes': dict(width=8, sizes=(3, 3), act='tanh', R=4, E=2),
    'one candidate': dict(width=8, sizes=(3, 3), act='tanh', R=3, E=3),
}
# Cases whose made-up CPU inputs were drawn again because a plain fp32 evaluation of the first draw missed YARDSTICK (other inputs,
# never another ceiling): none so far.
REDRAWN = {}


def field_of(case) -> tuple:
    return FIELDS[case.get('field', 0)]


def channels(case) -> list:
    """[cin_0, cout_0 = cin_1, ..., 3]."""
    return [3 if case.get('with_agent_channel', True) else 2] + [case['width']] * (len(case['sizes']) - 1) + [3]


def layer_shapes(case) -> list:
    """(k, cin, cout) of every layer."""
    ch = channels(case)
    return [(k, ch[i], ch[i + 1]) for i, k in enumerate(case['sizes'])]


def row_length(case) -> int:
    return sum(cout * cin * k * k for k, cin, cout in layer_shapes(case))


# ---- the byte formulas ------------------------------------------------------------------------------------------------------
def store_bytes(W: int, H: int, replicas: int, n_layers: int, max_channels: int) -> int:
    """die_nca_wide_sense_batch_store_bytes: [L][R][Cmax][W][H] fp32."""
    if W < 1 or H < 1 or not 1 <= replicas <= 64 or not 1 <= n_layers <= 8 or not 1 <= max_channels <= 32 or -(-W // B.TX) > 65535:
        return -1
    return 4 * n_layers * replicas * max_channels * W * H


def workspace_bytes(W: int, H: int, replicas: int, layers) -> int:
    """die_nca_wide_backward_batch_workspace_bytes for layers (k, cin, cout): the partial rows of the layer with the most weights,
    and min(L - 1, 2) sets of [R][Cmax][W][H] planes for the gradient travelling down the stack."""
    L = len(layers)
    if W < 1 or H < 1 or not 1 <= replicas <= 64 or not 1 <= L <= 8 or -(-W // B.TX) > 65535:
        return -1
    if any(k not in (1, 3, 5) or not 1 <= cin <= 32 or not 1 <= cout <= 32 for k, cin, cout in layers) or layers[-1][2] != 3:
        return -1
    row = max(cout * cin * k * k for k, cin, cout in layers)
    cmax = max(cout for _, _, cout in layers)
    return 4 * (replicas * B.tiles(W, H) * row + min(L - 1, 2) * replicas * cmax * W * H)


def sense(planes, weights, activation, mode: str = 'circular', mask=None) -> np.ndarray:
    """The stack's (3, W, H) output, float64: tests/nca_wide_model.sense."""
    return NW.sense(planes, weights, activation, mode, mask)


# ---- the adjoint -------------------------------------------------------------------------------------------------------------
def stack_outputs(planes, weights, activation, mode: str = 'circular') -> list:
    """t_l = act_l(z_l) of every layer, float64 (the last layer's is tanh, unmasked)."""
    zs = G.stack_pre_activations(planes, weights, activation, mode)
    return [G.act_forward(z, activation) for z in zs[:-1]] + [np.tanh(zs[-1])]


def stack_backward(planes, weights, g, activation, mode: str = 'circular', mask=None, ts=None):
    """(grad_w per layer, grad_in at the planes) of <stack(planes) * mask, g>, float64.  `ts`: forward outputs to take act' from
    instead of the model's own (a caller that compares with an fp32 evaluation hands in THAT evaluation's outputs, so that relu's
    kink cannot split the two); the layers' inputs are the model's own float64 values either way."""
    own = stack_outputs(planes, weights, activation, mode)
    ts = own if ts is None else ts
    L = len(weights)
    grads, cur = [None] * L, np.asarray(g, dtype=np.float64)
    for l in range(L - 1, -1, -1):
        x = np.asarray(planes, dtype=np.float64) if l == 0 else own[l - 1]
        last = l == L - 1
        grads[l], cur = G.layer_backward(x, weights[l], cur, ts[l], 'tanh' if last else activation, mask if last else None, mode)
    return grads, cur


def flat(grads) -> np.ndarray:
    """The layers' gradients in parameters_to_vector order."""
    return np.concatenate([np.asarray(w).ravel() for w in grads])


def population_backward(planes, weights, g, activation, mode: str = 'circular', masks=None, episodes: int = 1, ts=None):
    """planes[r], g[r], masks[r] (or None) per replica, weights[c] per candidate -> ((C, P) float64: row c the sum over candidate
    c's E worlds, episode e = 0 .. E - 1 in order; grad_in[r] at replica r's planes)."""
    R = len(planes)
    assert R % episodes == 0 and len(weights) == R // episodes
    rows, gins = [], []
    for c in range(R // episodes):
        total = None
        for e in range(episodes):
            r = c * episodes + e
            grads, gin = stack_backward(planes[r], weights[c], g[r], activation, mode, None if masks is None else masks[r],
                                        None if ts is None else ts[r])
            total = flat(grads) if total is None else total + flat(grads)
            gins.append(gin)
        rows.append(total)
    return np.stack(rows), gins


def blocks(case, row) -> list:
    """A flat (P,) row cut into the layers' blocks."""
    out, off = [], 0
    for k, cin, cout in layer_shapes(case):
        out.append(np.asarray(row)[off:off + cout * cin * k * k])
        off += cout * cin * k * k
    return out


# ---- made-up inputs for the CPU checks (the device tests read theirs from stepped worlds) ------------------------------------------
def cpu_inputs(name: str):
    """(planes[r] (cin, W, H) float32, weights[c]: one float32 (cout, cin, k, k) per layer, uniform in +-0.5, g[r] (3, W, H) float32,
    masks[r] or None)."""
    from tests import dropout_model as D
    case = CASES[name]
    W, H = field_of(case)
    R, E = case['R'], case.get('E', 1)
    rs = np.random.RandomState(1000 + sorted(CASES).index(name) + 7919 * REDRAWN.get(name, 0))
    cin = channels(case)[0]
    planes = []
    for r in range(R):
        fields = rs.rand(2, W, H).astype(np.float32)
        if case.get('f16'):
            fields = fields.astype(np.float16).astype(np.float32)
        occ = (rs.rand(1, W, H) < 0.3).astype(np.float32)
        planes.append(np.concatenate([occ, fields])[3 - cin:])
    weights = [[rs.uniform(-0.5, 0.5, (cout, ci, k, k)).astype(np.float32) for k, ci, cout in layer_shapes(case)] for _ in range(R // E)]
    g = [rs.standard_normal((3, W, H)).astype(np.float32) for _ in range(R)]
    masks = [D.mask(case['seed'] + r * case['stride'], 2, W, H, DROP_P) for r in range(R)] if 'seed' in case else None
    return planes, weights, g, masks


# ---- the unrolled step: the stack model in front of tests/field_step_adjoint_model.py's field step --------------------------------
def torch_stack(weights, activation, mode: str, dtype):
    """The stack as a torch nn.Sequential of bias-free 'same'-padded Conv2d layers (checked against this module's numpy adjoint
    in tests/test_nca_wide_grad_batch_cpu.py, which builds the same thing)."""
    import torch
    from torch import nn
    stack = nn.Sequential()
    for li, w in enumerate(weights):
        conv = nn.Conv2d(w.shape[1], w.shape[0], w.shape[2], padding='same', padding_mode=mode, bias=False).to(dtype)
        with torch.no_grad():
            conv.weight.copy_(torch.as_tensor(np.asarray(w), dtype=dtype))
        stack.append(conv)
        last = li == len(weights) - 1
        if last or activation is not None:
            stack.append(nn.Tanh() if last or activation == 'tanh' else nn.ReLU())
    return stack


def rollout(weights, activation, mode: str, chem0, frames, cells, c, sigma: float, decay: float, coefs, with_agent_channel: bool = True,
            dtype=None):
    """One world, T = len(cells) unrolled steps with the positions frozen (tests/field_step_adjoint_model.rollout with a wide stack
    and no action term): frames[t] = dict(occ, food (W, H), cx, cy (N,)) as action t was sensed, cells[t] the winners' cells,
        deposit_t = coefs[2] * stack(occ_t, food_t, chem_t)[2, cx_t, cy_t],  chem_{t+1} = step_chem(chem_t, deposit_t, cells_t),
    loss = <c, chem_T>.  Returns (flat gradient in parameters_to_vector order, chem_T), float64 numpy."""
    import torch
    from tests import field_step_adjoint_model as F
    dtype = torch.float64 if dtype is None else dtype
    stack = torch_stack(weights, activation, mode, dtype)
    as_t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    chem = as_t(chem0)
    for t, won in enumerate(cells):
        f = frames[t]
        planes = torch.stack(([as_t(f['occ'])] if with_agent_channel else []) + [as_t(f['food']), chem])
        sense = stack(planes[None])[0]
        deposit = sense[2, torch.as_tensor(f['cx'], dtype=torch.int64), torch.as_tensor(f['cy'], dtype=torch.int64)] * float(coefs[2])
        chem = F.step_chem(chem, deposit, won, sigma, decay)
    (as_t(c) * chem).sum().backward()
    grads = [m.weight.grad.to(torch.float64).numpy() for m in stack if hasattr(m, 'weight')]
    return flat(grads), chem.detach().to(torch.float64).numpy()
