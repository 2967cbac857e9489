"""TEST INFRASTRUCTURE ONLY: the exact lattice and the case tables of the wide layer's domain sweep (tests/test_nca_wide_domain_cpu.py
for the method itself, tests/test_gpu_nca_wide_domain.py on the device).

The method.  Inputs are small integers and weights small integers times ONE power of two, 2^-s.  Every product w * x is then an integer
times 2^-s, and so is every partial sum of one output, in whatever order the terms are added; as long as sum |w| |x| stays below
2^24 * 2^-s every one of them is a float32, so an fp32 accumulation in ANY order gives the float64 value, bit for bit.  The device is
then held to the model's value itself, not to a tolerance, and a kernel that later sums in another order still passes.  The same
holds for relu (a comparison), for a dropout mask at p = 0.5 (keep = 2) and for both adjoint sums with activation none or relu.

The layer is tests/nca_wide_model.conv (conv_model below is the same sum by matrix products, held to it by the CPU tests), the mask
tests/dropout_model.mask, the claim and stock words tests/stock_plane_model.encode.
`conv_loops` states include/die_hip.h's formula a second time, tap by tap with the four paddings written out as index rules, for the
fields torch's conv2d does not take ('reflect' excepted, nothing here pads with np.pad)."""
import functools
import zlib

import numpy as np

from tests import nca_wide_model as M
from tests import stock_plane_model as S

MODES = ('circular', 'zeros', 'reflect', 'replicate')
KS = (1, 3, 5)
CIN = (1, 2, 3, 4, 5, 8, 13, 16, 17, 31, 32)                      # the chunk-of-4 edges
COUT = (1, 3, 15, 16, 17, 31, 32)                                 # the 16-channel block edge, NB = 1 / 2
CROSS_FIELD = (17, 66)                                            # one past a tile on each axis, H % 4 = 2
PAIRS = ((1, 1), (3, 16), (16, 3), (5, 17), (32, 32))
FIELD_GROUPS = (
    ('below_radius', ((1, 1), (1, 7), (7, 1), (2, 3), (3, 2))),
    ('below_tile_vec', ((5, 4),)),                                # 16-byte stores on a field below a tile
    ('exact_tile', ((16, 64),)),
    ('tile_edges', ((15, 63), (17, 65))),                         # one cell short of a tile, one past it
    ('partial_vec', ((20, 68),)),
    ('three_tiles', ((33, 130),)),                                # three tile columns, three tile rows
)
FIELDS = tuple(f for _, fs in FIELD_GROUPS for f in fs)
X_MAX, W_MAX, G_MAX, STOCK_MAX = 3, 7, 3, 3
Z_LIMIT = 4.0                                                     # max |z| stays below it: tanh off saturation
EXACT = float(2 ** 24)                                            # integers below it are float32 values
EPOCH = 5                                                         # the epoch the claim and stock planes are read at
DROP_P, DROP_STEP = 0.5, 3                                        # keep = 2: a masked value is a doubled or a zeroed one


def reflect_ok(W: int, H: int, k: int) -> bool:
    """'reflect' padding of k / 2 cells needs a field larger than that on both axes (the header's rule, and torch's)."""
    return k // 2 < W and k // 2 < H


def modes_for(W: int, H: int, k: int):
    return tuple(m for m in MODES if m != 'reflect' or reflect_ok(W, H, k))


def cross_cases(k: int, mode: str):
    """(cin, cout, k, W, H) of the pair cross at kernel size k (every CIN x COUT pair on CROSS_FIELD; `mode` only filters 'reflect')."""
    W, H = CROSS_FIELD
    return [(cin, cout, k, W, H) for cin in CIN for cout in COUT] if mode in modes_for(W, H, k) else []


def field_cases(group: str, mode: str):
    """(cin, cout, k, W, H) of PAIRS x KS on every field of one group of FIELD_GROUPS, 'reflect' only where the header allows it."""
    fields = dict(FIELD_GROUPS)[group]
    return [(cin, cout, k, W, H) for W, H in fields for k in KS if mode in modes_for(W, H, k) for cin, cout in PAIRS]


def case_seed(*key) -> int:
    return zlib.crc32(' '.join(str(v) for v in key).encode())


# ------------------------------------------------------------------------------------------------------------ the formula, as loops
def pad_index(v: np.ndarray, n: int, mode: str) -> np.ndarray:
    """The cell that stands in for coordinate v of an axis of n cells, -1 for "reads as zero": 'circular' wraps, 'zeros' pads with 0,
    'reflect' mirrors without repeating the edge cell, 'replicate' repeats it (torch.nn.functional.pad)."""
    v = np.asarray(v, dtype=np.int64)
    inside = (v >= 0) & (v < n)
    if mode == 'circular':
        out = v % n
    elif mode == 'zeros':
        out = np.full_like(v, -1)
    elif mode == 'replicate':
        out = np.clip(v, 0, n - 1)
    elif mode == 'reflect':
        if n == 1:
            out = np.zeros_like(v)
        else:
            q = v % (2 * (n - 1))
            out = np.where(q < n, q, 2 * (n - 1) - q)
    else:
        raise ValueError(mode)
    return np.where(inside, v, out)


def padded(x: np.ndarray, r: int, mode: str) -> np.ndarray:
    """(cin, W + 2r, H + 2r): the field with r cells of `mode` around it, by pad_index."""
    W, H = x.shape[1:]
    ix, iy = pad_index(np.arange(-r, W + r), W, mode), pad_index(np.arange(-r, H + r), H, mode)
    out = x[:, np.maximum(ix, 0)[:, None], np.maximum(iy, 0)[None, :]].copy()
    out[:, ix < 0, :] = 0
    out[:, :, iy < 0] = 0
    return out


def conv_loops(x, w, mode: str) -> np.ndarray:
    """out[o, x, y] = sum_i sum_a sum_b w[o, i, a, b] * in[i, pad(x + a - r), pad(y + b - r)] in float64, one term at a time."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    cout, cin, k, _ = w.shape
    W, H = x.shape[1:]
    xp = padded(x, k // 2, mode)
    out = np.zeros((cout, W, H))
    for o in range(cout):
        for i in range(cin):
            for a in range(k):
                for b in range(k):
                    out[o] += w[o, i, a, b] * xp[i, a:a + W, b:b + H]
    return out


def conv_model(x, w, mode: str) -> np.ndarray:
    """The same sum in float64 with one matrix product per tap: what the generators below call, a few hundred times faster than the
    loops and than tests/nca_wide_model.conv's einsum.  On the lattice all three are sums of the same integers and agree bit for bit
    (tests/test_nca_wide_domain_cpu.py holds them together on every case of both tables)."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    cout, cin, k, _ = w.shape
    W, H = x.shape[1:]
    xp = padded(x, k // 2, mode)
    out = np.zeros((cout, W * H))
    for a in range(k):
        for b in range(k):
            out += w[:, :, a, b] @ xp[:, a:a + W, b:b + H].reshape(cin, W * H)
    return out.reshape(cout, W, H)


def conv_fp32(x, w, mode: str, reverse: bool = False) -> np.ndarray:
    """The layer accumulated in float32, one rounded product added at a time, in k_conv_wide's order — (chunk of 4 input channels,
    a, b, channel in the chunk) — or in exactly the reverse order."""
    x, w = np.asarray(x, dtype=np.float32), np.asarray(w, dtype=np.float32)
    cout, cin, k, _ = w.shape
    W, H = x.shape[1:]
    xp = padded(x, k // 2, mode)
    order = [(c0 + j, a, b) for c0 in range(0, cin, 4) for a in range(k) for b in range(k) for j in range(min(4, cin - c0))]
    acc = np.zeros((cout, W, H), dtype=np.float32)
    for c, a, b in (reversed(order) if reverse else order):
        acc = acc + w[:, c, a, b][:, None, None] * xp[c, a:a + W, b:b + H][None]
        assert acc.dtype == np.float32
    return acc


# ------------------------------------------------------------------------------------------------------------ the lattice
def _nonzero_ints(rs, top: int, shape) -> np.ndarray:
    """Integers in -top .. top, none zero."""
    v = rs.randint(1, top + 1, size=shape)
    return np.where(rs.rand(*shape) < 0.5, -v, v).astype(np.int64)


def scale_for(peak: float) -> int:
    """The smallest s >= 0 with peak * 2^-s < Z_LIMIT."""
    s = 0
    while peak * 2.0 ** -s >= Z_LIMIT:
        s += 1
    return s


def lattice_case(seed: int, cin: int, cout: int, k: int, W: int, H: int) -> dict:
    """One layer's inputs on the lattice and its float64 model under every padding the shape allows:
        x  (cin, W, H) float32, integers in -3 .. 3         g  (cout, W, H) float32, integers in -3 .. 3
        w  (cout, cin, k, k) float32, integers in -7 .. 7 (none zero) times 2^-s, s the smallest s >= 0 that keeps max |z| < 4
        z  {mode: (cout, W, H) float32}: the float64 model's value, which IS a float32 (asserted)
    Asserted here, as the method's precondition: sum |w| |x| of every output, and both adjoint sums with a p = 0.5 mask, stay below
    2^24 in units of 2^-s, so no order of summation can round."""
    rs = np.random.RandomState(seed)
    xi = rs.randint(-X_MAX, X_MAX + 1, size=(cin, W, H)).astype(np.int64)
    wi = _nonzero_ints(rs, W_MAX, (cout, cin, k, k))
    gi = rs.randint(-G_MAX, G_MAX + 1, size=(cout, W, H)).astype(np.int64)
    modes = modes_for(W, H, k)
    zi = {m: conv_model(xi, wi, m) for m in modes}
    s = scale_for(max(np.abs(z).max() for z in zi.values()))
    # the precondition.  Forward: every output sums cin * k * k terms |w| |x| under any padding, |x| <= its maximum
    assert np.abs(xi).max() * np.abs(wi).sum(axis=(1, 2, 3)).max() < EXACT, (cin, cout, k, W, H)
    # adjoint: grad_w sums W * H terms |g_z| |x| with |g_z| <= keep * |g|; grad_in sums cout * k * k terms |w| |g_z| (a cell of a
    # field below the radius takes several wraps of ONE tap each, never more terms than that)
    keep = 1.0 / (1.0 - DROP_P)
    assert keep * np.abs(gi).reshape(cout, -1).sum(axis=1).max() * np.abs(xi).max() < EXACT
    assert keep * np.abs(gi).max() * np.abs(wi).sum(axis=(0, 2, 3)).max() < EXACT
    w = (wi * 2.0 ** -s).astype(np.float32)
    assert np.array_equal(w.astype(np.float64) * 2.0 ** s, wi)
    z = {}
    for m in modes:
        z64 = zi[m] * 2.0 ** -s
        z[m] = z64.astype(np.float32)
        assert np.array_equal(z[m].astype(np.float64), z64) and np.abs(z64).max() < Z_LIMIT
    return dict(seed=seed, s=s, x=xi.astype(np.float32), w=w, g=gi.astype(np.float32), z=z, modes=modes)


@functools.lru_cache(maxsize=None)
def case(cin: int, cout: int, k: int, W: int, H: int) -> dict:
    """lattice_case of a table row, drawn once per process (the arrays are shared: nobody writes to them)."""
    c = lattice_case(case_seed(cin, cout, k, W, H), cin, cout, k, W, H)
    for a in (c['x'], c['w'], c['g'], *c['z'].values()):
        a.setflags(write=False)
    return c


# ------------------------------------------------------------------------------------------------------------ plane kinds
F32, F16, AGENTS, STOCK = 0, 1, 2, 3                              # die_plane_kind
KIND_CASES = {6: (F32, F16, AGENTS, F32, F16, STOCK),              # a claim plane inside chunk 0, fp16 and the stock plane in chunk 1
              9: (F32, F16, F32, F32, F16, F16, F32, AGENTS, STOCK)}   # the claim plane at index 7, the stock plane alone in chunk 2
KIND_FIELDS = ((17, 66), (2, 3))
KIND_KS = (3, 5)
KIND_COUT = 17


def claim_words(rs, values: np.ndarray, stock: bool) -> np.ndarray:
    """uint64 words that read as `values` at EPOCH: an occupied cell carries EPOCH, a slot id and — a stock plane — its value as the
    payload (a claim plane: any payload, it reads as 1); of the unoccupied cells a third carry a word of EPOCH - 1 with a payload
    that is not zero, which must read as 0, the others the word 0."""
    values = np.asarray(values, dtype=np.float32)
    occupied = values != 0
    slots = rs.randint(0, S.SLOT_MASK, size=values.shape)
    live = S.encode(EPOCH, slots, values if stock else rs.randint(1, 4, size=values.shape).astype(np.float32))
    stale = S.encode(EPOCH - 1, slots, np.full(values.shape, 3.0, dtype=np.float32))
    return np.where(occupied, live, np.where(rs.rand(*values.shape) < 1 / 3, stale, np.uint64(0))).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def kind_case(cin: int, k: int, W: int, H: int) -> dict:
    """lattice_case of cin -> KIND_COUT with the planes of KIND_CASES[cin]: a claim plane holds 0 / 1, a stock plane 0 (unoccupied:
    about half the cells) or a payload in 1 .. 3, and `words[c]` are the uint64 words of such a plane."""
    kinds = KIND_CASES[cin]
    seed = case_seed('kinds', cin, k, W, H)
    rs = np.random.RandomState(seed)
    c = lattice_case(seed, cin, KIND_COUT, k, W, H)
    x, words = c['x'].copy(), {}
    for i, kind in enumerate(kinds):
        if kind == AGENTS:
            x[i] = rs.rand(W, H) < 0.3
        elif kind == STOCK:
            x[i] = np.where(rs.rand(W, H) < 0.5, 0, rs.randint(1, STOCK_MAX + 1, size=(W, H)))
        if kind in (AGENTS, STOCK):
            words[i] = claim_words(rs, x[i], kind == STOCK)
            occ, _, bits, _ = S.decode(words[i], EPOCH)
            assert np.array_equal(np.where(occ, bits.view(np.float32) if kind == STOCK else 1.0, 0.0), x[i])
            assert (~occ & (words[i] != 0)).sum() > 0 or W * H < 12       # stale words are present
    # |x| only shrank (0 / 1 planes, payloads within X_MAX): the scale and the precondition of the draw above still hold, z is new
    wi = c['w'].astype(np.float64) * 2.0 ** c['s']
    z = {}
    for m in c['modes']:
        z64 = conv_model(x, wi, m) * 2.0 ** -c['s']
        assert np.abs(x).max() <= X_MAX
        z[m] = z64.astype(np.float32)
        assert np.array_equal(z[m].astype(np.float64), z64)
    return dict(c, x=x, z=z, kinds=kinds, words=words)


# ------------------------------------------------------------------------------------------------------------ the batched stack
STACK_LAYERS = ((3, 17, 'relu'), (1, 16, None), (5, 3, 'tanh'))   # (k, cout, activation): obs -> 17 -> 16 -> 3
STACK_FIELDS = ((17, 66), (20, 68))
STACK_R = 6
STACK_EPISODES = (1, 2, 3)
STACK_WEIGHT_GAP = 5                                              # floats between two replicas' blocks of a layer
STACK_PLANE_GAPS = (0, 8, 6)                                      # plane_stride = W * H + gap
STACK_CMAX = 17
STACK_SEED_STRIDES = (0, 1)


@functools.lru_cache(maxsize=None)
def stack_case(W: int, H: int, agents: bool, mode: str, R: int = STACK_R) -> dict:
    """R replicas' observation planes and R candidates' weights for the STACK_LAYERS stack, on the lattice:
        planes   (R, cin0, W, H) float32, cin0 = 2 + agents: [0 / 1 occupancy,] two fields of integers in -3 .. 3 (fp16 holds them)
        weights  [layer] (R, cout, cin, k, k) float32: integers in -7 .. 7, none zero, times 2^-s_l, s_l the smallest s >= 0 that
                 keeps that layer's max |z| below 4 over every (replica, candidate) pair the episode counts form
    Layer 0's z is an integer times 2^-s_0 and relu keeps it; layer 1's an integer times 2^-(s_0 + s_1); layer 2's pre-activation an
    integer times 2^-(s_0 + s_1 + s_2).  Each layer's sum of magnitudes is asserted below 2^24 of its unit, so all three are exact
    in fp32 in any order, and only the last layer's tanh rounds."""
    rs = np.random.RandomState(case_seed('stack', W, H, agents, mode, R))
    cin0 = 2 + int(agents)
    planes = rs.randint(-X_MAX, X_MAX + 1, size=(R, cin0, W, H)).astype(np.float64)
    if agents:
        planes[:, 0] = rs.rand(R, W, H) < 0.3
    pairs = sorted({(r, r // E) for E in STACK_EPISODES if R % E == 0 for r in range(R)})
    ints, scales, unit = [], [], 0
    t = {p: planes[p[0]] for p in pairs}
    cin = cin0
    for k, cout, act in STACK_LAYERS:
        wi = _nonzero_ints(rs, W_MAX, (R, cout, cin, k, k))
        zi = {p: conv_model(t[p], wi[p[1]], mode) for p in pairs}     # in units of 2^-unit
        for p in pairs:
            assert np.abs(t[p]).max() * np.abs(wi[p[1]]).sum(axis=(1, 2, 3)).max() * 2.0 ** unit < EXACT, (k, cout, p)
        s = scale_for(max(np.abs(z).max() for z in zi.values()))
        unit += s
        t = {p: M.ACTIVATIONS[None if act == 'tanh' else act](zi[p] * 2.0 ** -s) for p in pairs}
        ints.append(wi)
        scales.append(s)
        cin = cout
    weights = [(wi * 2.0 ** -s).astype(np.float32) for wi, s in zip(ints, scales)]
    for w, wi, s in zip(weights, ints, scales):
        assert np.array_equal(w.astype(np.float64) * 2.0 ** s, wi)
    return dict(planes=planes.astype(np.float32), weights=weights, scales=scales, pairs=pairs, cin0=cin0)


def stack_model(c: dict, r: int, row: int, mode: str):
    """[t_0, t_1, z_2] of replica r under candidate `row`, float64: the two hidden layers' outputs and the last layer's
    pre-activation."""
    out, t = [], c['planes'][r].astype(np.float64)
    for (k, cout, act), w in zip(STACK_LAYERS, c['weights']):
        z = conv_model(t, w[row], mode)
        t = z if act == 'tanh' else M.ACTIVATIONS[act](z)
        out.append(t)
    return out


# ------------------------------------------------------------------------------------------------------------ random real values
RANDOM_FIELD = (33, 130)
RANDOM_TOL = 1e-5                                                 # of max(1, max |f64|): the conv layers' bound (LABBOOK §17)


@functools.lru_cache(maxsize=None)
def random_case(cin: int, cout: int, k: int) -> dict:
    """Real-valued inputs on RANDOM_FIELD: x in +-[0.25, 1), Xavier weights; z {mode: float64 model}."""
    W, H = RANDOM_FIELD
    rs = np.random.RandomState(case_seed('random', cin, cout, k))
    x = (rs.uniform(0.25, 1.0, (cin, W, H)) * np.where(rs.rand(cin, W, H) < 0.5, -1, 1)).astype(np.float32)
    w = M.xavier(rs, cout, cin, k)
    return dict(x=x, w=w, z={m: conv_model(x, w, m) for m in MODES})


def ulps(got: np.ndarray, want64: np.ndarray) -> float:
    """The largest distance of float32 `got` from the float64 `want64`, in units of the float32 spacing at `want64`."""
    want64 = np.asarray(want64, dtype=np.float64)
    spacing = np.spacing(np.maximum(np.abs(want64), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    return float((np.abs(np.asarray(got, dtype=np.float64) - want64) / spacing).max())
