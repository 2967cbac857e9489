"""The oracle of the differentiable Env.step (tests/test_field_step_adjoint_cpu.py, tests/test_gpu_field_step_grad.py): a plain torch
restatement of one unrolled rollout with the positions FROZEN, differentiated by torch's own autograd.  float64 by default; the
same code in float32 is the yardstick for how far a correct fp32 evaluation strays.

    for t = 0 .. T-1:   action_t = coef * (tanh(conv stack(planes_t)) * mask_t)[:, cx_t, cy_t]          (tests/nca_grad_model.py)
                        chem_{t+1} = (1 - decay) * G(chem_t with chem[cells_t[n]] += action_t[2, n] where cells_t[n] >= 0)
    action_T = the same read-out on planes_T                           loss = <c, chem_T> + <u, action_T>

planes_t = (occ_t, food_t, chem_t): the 'agents' plane, the food plane, the slots' cells (cx_t, cy_t, array order of that moment) and
the winners' cells (cells_t, array order of step t's action) are DATA — callers record them from the device, or make them up with
`synthetic_frames`; only chem_t is computed here.  G is the separable periodic gaussian with the library's taps (scipy's
_gaussian_kernel1d of the fp32 sigma, radius int(4 sigma + .5)), axis 0 then axis 1.

Also here: the winners' rule on the host (`deposit_cells`: the LAST alive slot in slot-id order owns a cell, core/env.py:204-215)
and the case list both test files share."""
from typing import Optional, Sequence

import numpy as np
import torch

from tests import nca_grad_model as G

COEFS = (0.1, 0.1, 2.0)              # NeuralAutomataAgent(scale=0.1, deposit=2.0)
DECAY = 0.1

# Test 5's cases (and the CPU file's): every one on 24 x 68 — one row and four columns past the conv's 16 x 64 tile, H % 4 == 0 so the
# diffusion takes the row sweep — at T = 1, 2, 3, and on 96 x 96 at T = 3.  sigma 0.8 is radius 3, sigma 0.5 radius 2.
CASES = {
    'two_layers': dict(sizes=(3, 3), boundary='circular', sigma=0.8),
    'one_5x5_zeros': dict(sizes=(5,), boundary='zeros', sigma=0.5),
    'no_agent_channel': dict(sizes=(3, 3), boundary='circular', sigma=0.8, with_agent_channel=False),
    'dropout': dict(sizes=(3, 3), boundary='circular', sigma=0.8, p=0.25, seed=7),
    'sort_every_1': dict(sizes=(3, 3), boundary='circular', sigma=0.8, sort_every=1),
    'collisions': dict(sizes=(3, 3), boundary='circular', sigma=0.8, collisions=True),
}
SHAPES = [(24, 68, 1), (24, 68, 2), (24, 68, 3), (96, 96, 3)]            # (W, H, T)


def taps(sigma: float) -> np.ndarray:
    """gaussian_taps of die_env.hip in float64: the library takes sigma as an fp32 number."""
    s = float(np.float32(sigma))
    r = int(4.0 * s + 0.5)
    w = np.exp(-0.5 / (s * s) * np.arange(-r, r + 1, dtype=np.float64) ** 2)
    return w / w.sum()


def diffuse_decay(chem: torch.Tensor, sigma: float, decay: float) -> torch.Tensor:
    """(1 - decay) * G(chem): out[i] = sum_k w[k] * in[i + k] along axis 0, then along axis 1, indices modulo the extent."""
    w = taps(sigma)
    r = len(w) // 2
    out = chem
    for axis in (0, 1):
        out = sum(float(w[k + r]) * torch.roll(out, -k, dims=axis) for k in range(-r, r + 1))
    return out * (1.0 - float(np.float32(decay)))


def step_chem(chem: torch.Tensor, deposit: torch.Tensor, cells, sigma: float, decay: float) -> torch.Tensor:
    """One step of the chem plane: the winners' deposits added at their cells (each cell has at most one winner), then the sweep."""
    cells = torch.as_tensor(np.asarray(cells), dtype=torch.int64)
    won = cells >= 0
    assert torch.unique(cells[won]).numel() == int(won.sum())
    flat = chem.reshape(-1).index_add(0, cells[won], deposit[won])
    return diffuse_decay(flat.reshape(chem.shape), sigma, decay)


def deposit_cells(cx, cy, alive, slot, H: int) -> np.ndarray:
    """int32 (N,): entry n's cell cx * H + cy if it is alive and no alive entry with a larger slot id stands there, else -1."""
    cx, cy, alive = np.asarray(cx, dtype=np.int64), np.asarray(cy, dtype=np.int64), np.asarray(alive) > 0
    slot = np.arange(cx.size) if slot is None else np.asarray(slot, dtype=np.int64)
    cell = cx * H + cy
    best = {}
    for n in np.flatnonzero(alive):
        if slot[n] > best.get(cell[n], (-1, -1))[0]:
            best[cell[n]] = (slot[n], n)
    out = np.full(cx.size, -1, dtype=np.int32)
    for c, (_, n) in best.items():
        out[n] = c
    return out


def rollout(weights: Sequence[np.ndarray], boundary: str, chem0: np.ndarray, frames, cells, c: np.ndarray, u: np.ndarray, sigma: float,
            decay: float = DECAY, coefs=COEFS, with_agent_channel: bool = True, dtype=torch.float64, leaf_chem: bool = False):
    """frames: T + 1 dicts occ, food (W, H), cx, cy (N,) and optionally mask (W, H) — the world as action t was sensed; cells: T arrays.
    Returns dict(loss, grads=[d loss / d weight per layer], chem=chem_T, action=action_T, grad_chem0 if leaf_chem) as numpy float64."""
    T = len(cells)
    assert len(frames) == T + 1
    convs = G.layers(weights, boundary, dtype)
    as_t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    chem = as_t(chem0).requires_grad_(leaf_chem)
    chem_in = chem

    def act(t):
        f = frames[t]
        planes = torch.stack(([as_t(f['occ'])] if with_agent_channel else []) + [as_t(f['food']), chem])
        m = as_t(f['mask']) if f.get('mask') is not None else None
        return G.action(convs, planes, f['cx'], f['cy'], coefs, m)

    for t in range(T):
        chem = step_chem(chem, act(t)[2], cells[t], sigma, decay)
    action = act(T)
    loss = (as_t(c) * chem).sum() + (as_t(u) * action).sum()
    loss.backward()
    f64 = lambda x: x.detach().to(torch.float64).numpy()
    out = dict(loss=float(loss.detach()), grads=[f64(k.weight.grad) for k in convs], chem=f64(chem), action=f64(action))
    if leaf_chem:
        out['grad_chem0'] = f64(chem_in.grad)
    return out


# ---- inputs both files share -----------------------------------------------------------------------------------------------
def _rs(name: str, W: int, H: int, salt: int = 0) -> np.random.RandomState:
    return np.random.RandomState((sorted(CASES).index(name) * 1009 + W * 31 + H + salt * 7919) % (2 ** 31))


def weights_of(name: str, W: int, H: int):
    """The layers' weights of a case, uniform in +-0.5 (the scale at which tests/test_gpu_nca_grad.py holds its ceiling)."""
    c = CASES[name]
    cin = 3 if c.get('with_agent_channel', True) else 2
    rs = _rs(name, W, H, 1)
    return [rs.uniform(-0.5, 0.5, (3 if i == len(c['sizes']) - 1 else cin, cin, k, k)) for i, k in enumerate(c['sizes'])]


def collision_world(W: int, H: int, rs: np.random.RandomState):
    """Test 2's world: three alive slots on one cell, a dead slot on an occupied cell, a dead slot alone, the rest alive on cells
    of their own.  Returns (medium (3, W, H), agents (4, N))."""
    N = W * H // 9
    cells = rs.choice(W * H, N, replace=False)
    cx, cy = cells // H, cells % H
    alive = np.ones(N, dtype=bool)
    cx[[3, 7]], cy[[3, 7]] = cx[11], cy[11]          # slots 3, 7, 11 share a cell: 11 wins
    alive[5] = False
    cx[5], cy[5] = cx[2], cy[2]                      # a dead slot where slot 2 stands
    alive[6] = False                                 # a dead slot alone
    return _world_arrays(W, H, cx, cy, alive, rs)


def plain_world(W: int, H: int, rs: np.random.RandomState):
    """N = W * H // 7 slots, a fifth of them dead, the alive ones on cells of their own."""
    N = W * H // 7
    alive = rs.permutation(N) >= N // 5
    cells = rs.choice(W * H, N, replace=False)
    return _world_arrays(W, H, cells // H, cells % H, alive, rs)


def _world_arrays(W, H, cx, cy, alive, rs):
    occ = np.zeros((W, H))
    occ[cx[alive], cy[alive]] = 1.0
    medium = np.stack([occ, rs.rand(W, H), rs.rand(W, H)])
    agents = np.stack([cx / (W - 1), cy / (H - 1), alive.astype(np.float64), np.ones(cx.size)])      # a cell's own label
    return medium, agents


def world_of(name: str, W: int, H: int):
    rs = _rs(name, W, H, 2)
    return collision_world(W, H, rs) if CASES[name].get('collisions') else plain_world(W, H, rs)


def loss_vectors(name: str, W: int, H: int, N: int):
    """(c (W, H), u (3, N)): standard normal, fixed per case."""
    rs = _rs(name, W, H, 3)
    return rs.standard_normal((W, H)), rs.standard_normal((3, N))


def synthetic_frames(name: str, W: int, H: int, T: int, masks=None):
    """A made-up trajectory for the CPU checks (no device): the case's world, every slot hopping by up to two cells per step (so cells
    get shared and won), a random permutation of the array order per step when the case re-sorts, food decaying under the alive.
    Returns (chem0, frames, cells) as `rollout` takes them."""
    medium, agents = world_of(name, W, H)
    rs = _rs(name, W, H, 4)
    N = agents.shape[1]
    cx, cy = np.rint(agents[0] * (W - 1)).astype(np.int64), np.rint(agents[1] * (H - 1)).astype(np.int64)
    alive, slot, food = agents[2] > 0, np.arange(N), medium[1].copy()
    frames, cells = [], []
    for t in range(T + 1):
        occ = np.zeros((W, H))
        occ[cx[alive], cy[alive]] = 1.0
        frames.append(dict(occ=occ, food=food.copy(), cx=cx.copy(), cy=cy.copy(), mask=None if masks is None else masks[t]))
        if t == T:
            break
        cx, cy = (cx + rs.randint(-2, 3, N)) % W, (cy + rs.randint(-2, 3, N)) % H
        cells.append(deposit_cells(cx, cy, alive, slot, H))
        food = food * np.where(np.isin(np.arange(W * H), cells[-1][cells[-1] >= 0]).reshape(W, H), 0.9, 1.0)
        if CASES[name].get('sort_every'):
            perm = rs.permutation(N)
            cx, cy, alive, slot = cx[perm], cy[perm], alive[perm], slot[perm]
    return medium[2], frames, cells
