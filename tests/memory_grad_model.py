"""The model of the memory channels' adjoints (include/die_hip.h die_memory_cells / die_memory_planes_backward /
die_gather_memory_backward; NeuralAutomataAgent.recurrent_action), used by tests/test_memory_grad_cpu.py and
tests/test_gpu_memory_grad.py.

The record, from the stock channel's winners (tests/stock_plane_model.py) and the memory model's cell indexing
(tests/memory_model.py), everything by SLOT ID:

    cell[id] = ix * H + iy  if the slot is alive                          else -1
    win[id]  = cell[id]     if the slot is the winner of its cell         else -1          (dead slots, losers of a shared cell)

The two maps and their adjoints, as plain loops over the record (float64 unless told otherwise):

    expand          P[j][win[id]]  = mem[j][id]        (win[id] >= 0; every other cell 0)
    expand_adjoint  gm[j][id]      = gp[j][win[id]]    (win[id] >= 0; else 0)
    gather          mem[j][id]     = S[j][cell[id]]    (cell[id] >= 0; else 0)
    gather_adjoint  gp[j][cell[id]] += gm[j][id]       (cell[id] >= 0; ascending slot id)

And `unroll`, the recurrent T-step loop in torch (index ops, `torch.nn.functional.conv2d` with circular or zero padding, the cell
mask given as data): what `recurrent_action` chained through `memory_next` computes, with the records, the slots' cells, the planes
the world supplies and the masks taken as given CONSTANTS.  float64 by default; the same code in float32 is the yardstick for how
far a correct fp32 evaluation strays."""
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from tests import dropout_model
from tests import stock_plane_model as S


# ---- the record -------------------------------------------------------------------------------------------------------------
def record(W: int, H: int, x, y, alive):
    """(cell, win), int32 (N,) each.  x, y: uint32 coordinate words; all per slot, in SLOT order."""
    alive = np.asarray(alive) > 0
    ix, iy = S.cell(x, W), S.cell(y, H)
    _, winner = S.stock_winners(W, H, x, y, alive)
    c = ix * H + iy
    cell = np.where(alive, c, -1).astype(np.int32)
    win = np.where(alive & (winner[ix, iy] == np.arange(len(ix))), c, -1).astype(np.int32)
    return cell, win


def record_of(W: int, H: int, agents: np.ndarray):
    """`record` for a (4, N) agents array as `to_numpy()` returns it (x, y as fractions of the unit square, slot order)."""
    return record(W, H, S.q32_words(agents[0]), S.q32_words(agents[1]), agents[2] > 0)


# ---- the two maps and their adjoints: plain loops ----------------------------------------------------------------------------
def expand(W: int, H: int, win, mem, dtype=np.float64) -> np.ndarray:
    mem = np.asarray(mem, dtype=dtype)
    out = np.zeros((mem.shape[0], W * H), dtype=dtype)
    for j in range(mem.shape[0]):
        for i, c in enumerate(win):
            if 0 <= c < W * H:
                out[j, c] = mem[j, i]
    return out.reshape(-1, W, H)


def expand_adjoint(W: int, H: int, win, grad_planes, dtype=np.float64) -> np.ndarray:
    gp = np.asarray(grad_planes, dtype=dtype).reshape(len(grad_planes), W * H)
    out = np.zeros((gp.shape[0], len(win)), dtype=dtype)
    for j in range(gp.shape[0]):
        for i, c in enumerate(win):
            if 0 <= c < W * H:
                out[j, i] = gp[j, c]
    return out


def gather(W: int, H: int, cell, planes, dtype=np.float64) -> np.ndarray:
    return expand_adjoint(W, H, cell, planes, dtype)                       # the same index-only gather, by `cell`


def gather_adjoint(W: int, H: int, cell, grad_memory, dtype=np.float64) -> np.ndarray:
    gm = np.asarray(grad_memory, dtype=dtype)
    out = np.zeros((gm.shape[0], W * H), dtype=dtype)
    for j in range(gm.shape[0]):
        for i, c in enumerate(cell):                                       # ascending slot id (fp32: two addends commute)
            if 0 <= c < W * H:
                out[j, c] = dtype(out[j, c] + gm[j, i])
    return out.reshape(-1, W, H)


# ---- the recurrent loop ------------------------------------------------------------------------------------------------------
def conv_stack(weights: Sequence[torch.Tensor], boundary: str, hidden_activation: Optional[str], planes: torch.Tensor,
               mask: Optional[torch.Tensor]) -> torch.Tensor:
    """(cin, W, H) -> (cout, W, H): bias-free 'same' convolutions, the hidden activation between them, tanh and the (W, H) mask
    after the last."""
    z = planes[None]
    for li, w in enumerate(weights):
        r = w.shape[-1] // 2
        if boundary == 'circular' and r:
            z = F.pad(z, (r, r, r, r), mode='circular')
            z = F.conv2d(z, w)
        else:
            assert boundary in ('circular', 'zeros')
            z = F.conv2d(z, w, padding=r)
        if li < len(weights) - 1 and hidden_activation is not None:
            z = torch.tanh(z) if hidden_activation == 'tanh' else torch.relu(z)
    s = torch.tanh(z[0])
    return s if mask is None else s * mask


def _idx(a) -> torch.Tensor:
    return torch.as_tensor(np.asarray(a).astype(np.int64))


def t_expand(W: int, H: int, win, mem: torch.Tensor) -> torch.Tensor:
    win = _idx(win)
    won = win >= 0
    return torch.zeros((mem.shape[0], W * H), dtype=mem.dtype).index_copy(1, win[won], mem[:, won]).reshape(-1, W, H)


def t_gather(cell, planes: torch.Tensor) -> torch.Tensor:
    cell = _idx(cell)
    live = cell >= 0
    flat = planes.reshape(planes.shape[0], -1)
    return torch.zeros((planes.shape[0], cell.numel()), dtype=planes.dtype).index_copy(1, torch.nonzero(live)[:, 0], flat[:, cell[live]])


def unroll(weights: Sequence[torch.Tensor], boundary: str, hidden_activation: Optional[str], frames, records, mem0: torch.Tensor, coefs,
           with_agent_channel: bool = True, chem0: Optional[torch.Tensor] = None, world=None, detach_at: Sequence[int] = ()):
    """T = len(records) rounds of the recurrent forward.  frames[t]: dict food (W, H), chem (W, H) unless the chem is threaded,
    occ (W, H) with the agents channel, cx, cy (N,) — the slots' cells in the ARRAY order of round t's action — and optionally
    mask (W, H); records[t] = (cell, win) by slot id; `weights`, `mem0`: torch tensors (leaves where a gradient is wanted), whose
    dtype the loop runs in.  `world` = dict(cells=[T arrays as die_deposit_cells writes them], sigma, decay) threads the chem plane
    from `chem0` through tests/field_step_adjoint_model.step_chem between the rounds; without it every round reads frames[t]['chem'].
    `detach_at`: rounds whose incoming memory is detached.  Returns dict(actions [T x (3, N)], memories [T + 1 x (M, N)],
    expanded [T x (M, W, H)], sense [T x (3 + M, W, H)], chem (the last plane if threaded))."""
    dtype = mem0.dtype
    as_t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    W, H = np.asarray(frames[0]['food']).shape
    mem, chem = mem0, chem0
    out = dict(actions=[], memories=[mem0], expanded=[], sense=[])
    for t, (cell, win) in enumerate(records):
        f = frames[t]
        mem_in = mem.detach() if t in detach_at else mem
        P = t_expand(W, H, win, mem_in)
        field = ([as_t(f['occ'])] if with_agent_channel else []) + [as_t(f['food']), chem if world is not None else as_t(f['chem'])]
        planes = torch.cat([torch.stack(field), P])
        s = conv_stack(weights, boundary, hidden_activation, planes, as_t(f['mask']) if f.get('mask') is not None else None)
        action = s[:3][:, _idx(f['cx']), _idx(f['cy'])] * torch.as_tensor(coefs, dtype=dtype)[:, None]
        mem = t_gather(cell, s[3:])
        for name, v in (('actions', action), ('memories', mem), ('expanded', P), ('sense', s)):
            out[name].append(v)
        if world is not None:
            from tests import field_step_adjoint_model as FS
            chem = FS.step_chem(chem, action[2], world['cells'][t], world['sigma'], world['decay'])
    out['chem'] = chem
    return out


def mask_of(seed: int, step: int, W: int, H: int, p: float) -> np.ndarray:
    """The counter-based mask of NeuralAutomataAgent(dropout_seed=seed) at `dropout_step` = step (tests/dropout_model.py)."""
    return dropout_model.mask(seed, step, W, H, p)


def rel_err(got, ref) -> float:
    """max|got - ref| / max|ref| of one array (0 / 0 = 0)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    top = np.abs(ref).max() if ref.size else 0.0
    err = np.abs(got - ref).max() if ref.size else 0.0
    return 0.0 if err == 0.0 else float(err / top) if top > 0 else float('inf')


# ---- the crafted world both test files share ---------------------------------------------------------------------------------
CRAFTED = (6, 5)


def crafted_world():
    """6 x 5, 12 slots: slots 1, 4, 9 alive on cell (2, 3) (9 wins), slots 0, 7 alive on cell (4, 1) (7 wins), slot 5 dead on the
    crowded cell, slot 2 dead alone, the rest alive on cells of their own.  Returns (medium (3, W, H), agents (4, N)) in slot
    order, coordinates a cell's own label."""
    W, H = CRAFTED
    cx = np.array([4, 2, 0, 1, 2, 2, 5, 4, 3, 2, 0, 5])
    cy = np.array([1, 3, 0, 1, 3, 3, 4, 1, 2, 3, 4, 0])
    alive = np.ones(12, dtype=bool)
    alive[[5, 2]] = False
    rs = np.random.RandomState(1234)
    occ = np.zeros((W, H))
    occ[cx[alive], cy[alive]] = 1.0
    medium = np.stack([occ, rs.rand(W, H), rs.rand(W, H)])
    agents = np.stack([cx / (W - 1), cy / (H - 1), alive.astype(np.float64), np.ones(12)])
    return medium, agents


def label_words(c, n: int) -> np.ndarray:
    """The coordinate words of cells' own labels c / (n - 1), as an upload stores them (1.0 saturates to 2^32 - 1)."""
    return np.array([min(2 ** 32 - 1, (int(v) << 32) // (n - 1)) for v in np.asarray(c)], dtype=np.uint32)


def synthetic_rounds(W: int, H: int, N: int, T: int, rs: np.random.RandomState, crowd: bool = True, p: float = 0.0, seed: int = 0):
    """A made-up trajectory for the CPU checks: T rounds of frames and records (slot order = array order), slots hopping between the
    rounds, a tenth of them dead, and with `crowd` three alive slots on one cell and two on another in every round."""
    alive = rs.permutation(N) >= max(N // 10, 1)
    frames, records = [], []
    for t in range(T):
        cells = rs.choice(W * H, N, replace=False)
        if crowd:
            a = np.flatnonzero(alive)
            cells[a[1]] = cells[a[2]] = cells[a[0]]
            cells[a[4]] = cells[a[3]]
        cx, cy = cells // H, cells % H
        occ = np.zeros((W, H))
        occ[cx[alive], cy[alive]] = 1.0
        x, y = label_words(cx, W), label_words(cy, H)
        frames.append(dict(occ=occ, food=rs.rand(W, H), chem=rs.rand(W, H), cx=cx, cy=cy,
                           mask=mask_of(seed, t, W, H, p) if p > 0 else None))
        records.append(record(W, H, x, y, alive))
    return frames, records
