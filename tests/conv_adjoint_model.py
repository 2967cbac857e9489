"""TEST INFRASTRUCTURE ONLY: a plain numpy model of one NeuralAutomataAgent layer and its adjoint, as include/die_hip.h states them
for die_conv2d / die_conv2d_dropout / die_conv2d_backward / die_gather_scale / die_gather_scale_backward, and the list of cases
the direct entry-point tests run (tests/test_gpu_conv_abi.py on the device, tests/test_conv_adjoint_model_cpu.py for the model
itself and for the fp32 yardstick of every one of those cases).  float64 unless a dtype is given; no torch.

    conv             out[o, x, y] = sum_i sum_a sum_b w[o, i, a, b] * xp[i, x + a, y + b],  xp = x padded by r = k // 2 per side
    conv_backward    grad_w[o, i, a, b] = sum_xy g[o, x, y] * xp[i, x + a, y + b];  the gradient of the PADDED array, gp[i, x + a,
                     y + b] += w[o, i, a, b] * g[o, x, y], folded back onto the field by the padding's adjoint: 'zeros' keeps the
                     middle, 'circular' adds every padded cell onto the cell it was copied from (indices mod W, mod H — also when
                     the radius exceeds the field and a cell was copied several times)
    tanh_mask_adjoint, gather, gather_backward   the tanh / dropout epilogue's adjoint and the per-slot read-out with its scatter

Cells and masks are not computed here: oracle.cpu_ref.cell and tests/dropout_model.mask are the project's twins of those."""
import zlib

import numpy as np

from oracle import cpu_ref as R

FWD_MODES = ('circular', 'zeros', 'reflect', 'replicate')
BWD_MODES = ('circular', 'zeros')
KS = (1, 3, 5, 7)
PAIRS = tuple((cin, cout) for cin in (1, 2, 3, 4) for cout in (1, 2, 3, 4))
# the smallest fields that reach each edge of the kernels' 16 x 64 tile, and four smaller than the largest radius
SHAPES = ((16, 64),      # exactly one tile
          (17, 66),      # one row and two columns past a tile; H % 4 != 0
          (20, 68),      # partial tiles with H % 4 == 0
          (33, 130),     # 3 x 3 tiles: the interior tile's halo is all neighbours
          (1, 1), (2, 3), (3, 2), (5, 4))


WORLD_OCC = (np.random.RandomState(20240).rand(33, 130) < 0.3).astype(np.float64)


def reflect_ok(W: int, H: int, k: int) -> bool:
    """'reflect' padding of r cells needs a field larger than r along both axes (torch and die_conv2d refuse it otherwise)."""
    return k // 2 < W and k // 2 < H


def shapes_for(mode: str, k: int):
    return tuple(s for s in SHAPES if mode != 'reflect' or reflect_ok(*s, k))


def occupancy(W: int, H: int) -> np.ndarray:
    """The 0 / 1 plane a claim-plane input of a (W, H) case reads: the first W * H cells of WORLD_OCC, the occupancy of the one
    small world the device tests upload (its claim words are consecutive in memory, so any prefix of them is a plane)."""
    return WORLD_OCC.ravel()[:W * H].reshape(W, H).copy()


# Cases drawn again (the draw's number goes into the seed).  Errors are measured against max|.| of an array, and an array of ONE
# element that happens to cancel (the single output of a 1 x 1 field, the single weight gradient of a 1 -> 1, k = 1 layer over
# 1 122 normal terms) makes that measure meaningless: a plain fp32 evaluation of the first draw missed the 1e-5 yardstick of
# tests/test_conv_adjoint_model_cpu.py there (1.2e-5, 1.7e-5), so the case gets other inputs, not another ceiling.
REDRAWN = {(5, 'circular', 3, 1, 1, 1): 1, (1, 'circular', 1, 1, 17, 66): 1}


def case_inputs(k: int, mode: str, cin: int, cout: int, W: int, H: int):
    """The inputs of one case, as float32 arrays (what the device is given): fields uniform in [0, 1), weights uniform in
    +-0.5, a standard-normal gradient at the outputs."""
    draw = REDRAWN.get((k, mode, cin, cout, W, H), 0)
    seed = zlib.crc32(f'{k} {mode} {cin} {cout} {W} {H}'.encode() + (f' draw {draw}'.encode() if draw else b''))
    rs = np.random.RandomState(seed)
    return dict(seed=seed,
                x=rs.rand(cin, W, H).astype(np.float32),
                w=rs.uniform(-0.5, 0.5, (cout, cin, k, k)).astype(np.float32),
                g=rs.standard_normal((cout, W, H)).astype(np.float32))


# --------------------------------------------------------------------------------------------------------- the layer
def _padded(x: np.ndarray, r: int, mode: str) -> np.ndarray:
    """(cin, W + 2r, H + 2r).  'circular' is written out as indices mod W / mod H, so that a radius beyond the field wraps as
    often as it takes; the other modes are numpy's."""
    if r == 0:
        return x
    if mode == 'circular':
        W, H = x.shape[1:]
        ix, iy = (np.arange(W + 2 * r) - r) % W, (np.arange(H + 2 * r) - r) % H
        return x[:, ix[:, None], iy[None, :]]
    return np.pad(x, ((0, 0), (r, r), (r, r)), mode=R._NP_PAD[mode])


def conv(x, w, mode: str = 'circular') -> np.ndarray:
    """One bias-free 'same'-padded layer in float64: the project's oracle."""
    return R.conv2d_same(np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64), mode)


def conv_taps(x, w, mode: str = 'circular', dtype=np.float64) -> np.ndarray:
    """The same layer tap by tap, every operation in `dtype` (float32: how far a plain fp32 evaluation strays)."""
    x, w = np.asarray(x, dtype=dtype), np.asarray(w, dtype=dtype)
    cout, cin, k, _ = w.shape
    W, H = x.shape[1:]
    xp = _padded(x, k // 2, mode)
    out = np.zeros((cout, W, H), dtype=dtype)
    for a in range(k):
        for b in range(k):
            out += np.tensordot(w[:, :, a, b], xp[:, a:a + W, b:b + H], axes=1).astype(dtype)
    return out


def conv_backward(x, w, g, mode: str = 'circular', dtype=np.float64):
    """(grad_w, grad_in) of <conv(x, w), g> for 'circular' and 'zeros', every operation in `dtype`."""
    assert mode in BWD_MODES, mode
    x, w, g = np.asarray(x, dtype=dtype), np.asarray(w, dtype=dtype), np.asarray(g, dtype=dtype)
    cout, cin, k, _ = w.shape
    r = k // 2
    W, H = x.shape[1:]
    xp = _padded(x, r, mode)
    gp = np.zeros((cin, W + 2 * r, H + 2 * r), dtype=dtype)
    grad_w = np.zeros_like(w)
    gflat = g.reshape(cout, W * H)
    for a in range(k):
        for b in range(k):
            grad_w[:, :, a, b] = gflat @ np.ascontiguousarray(xp[:, a:a + W, b:b + H]).reshape(cin, W * H).T
            gp[:, a:a + W, b:b + H] += (w[:, :, a, b].T @ gflat).reshape(cin, W, H)
    if mode == 'zeros':
        return grad_w, np.ascontiguousarray(gp[:, r:r + W, r:r + H])
    grad_in = np.zeros((cin, W, H), dtype=dtype)
    ix, iy = (np.arange(W + 2 * r) - r) % W, (np.arange(H + 2 * r) - r) % H
    np.add.at(grad_in, (slice(None), ix[:, None], iy[None, :]), gp)
    return grad_w, grad_in


def tanh_mask_adjoint(grad_out, t, mask=None) -> np.ndarray:
    """The gradient at z of s = tanh(z) * mask, from the gradient at s and t = tanh(z): grad_out * mask * (1 - t * t)."""
    grad_out, t = np.asarray(grad_out, dtype=np.float64), np.asarray(t, dtype=np.float64)
    m = 1.0 if mask is None else np.asarray(mask, dtype=np.float64)
    return grad_out * m * (1.0 - t * t)


# --------------------------------------------------------------------------------------------------------- the read-out
def gather(planes, cx, cy, coefs) -> np.ndarray:
    """(3, N): action[c, n] = planes[c][cx[n], cy[n]] * coefs[c]."""
    planes = np.asarray(planes)
    return planes[:, cx, cy] * np.asarray(coefs, dtype=planes.dtype)[:, None]


def gather_backward(cx, cy, grad_action, coefs, W: int, H: int) -> np.ndarray:
    """(3, W, H): grad_planes[c][cx[n], cy[n]] += grad_action[c, n] * coefs[c] for every slot; every other cell is 0."""
    grad_action = np.asarray(grad_action, dtype=np.float64)
    out = np.zeros((3, W, H))
    for c in range(3):
        np.add.at(out[c], (cx, cy), grad_action[c] * float(coefs[c]))
    return out


def gather_case():
    """The read-out's adjoint case: a (17, 66) field with one slot on every cell and one more on each corner, given by the
    coordinates 0.0 and 1.0 themselves.  (W, H, x, y, planes (3, W, H) float32, grad_action (3, N) float32, coefs)."""
    W, H = 17, 66
    rs = np.random.RandomState(1766)
    cx, cy = np.divmod(np.arange(W * H), H)
    x = np.concatenate([cx / (W - 1), [0.0, 0.0, 1.0, 1.0]])
    y = np.concatenate([cy / (H - 1), [0.0, 1.0, 0.0, 1.0]])
    return W, H, x, y, rs.standard_normal((3, W, H)).astype(np.float32), rs.standard_normal((3, x.size)).astype(np.float32), (0.1, 0.1, 2.0)
