"""The wide MFMA conv layer (die_nca_wide.hip: k_conv_wide) over its argument domain on the GPU, exactly: die_conv2d_wide,
die_nca_wide_sense_batch_store and die_conv2d_wide_backward through ctypes on the lattice of tests/nca_wide_domain_cases.py, where
every product and partial sum is a float32 in any order of summation, so the device must give the float64 model's value BIT FOR BIT
(compared by value: -0 is 0).  tests/test_nca_wide_domain_cpu.py shows that the method holds and that the model is torch's.

1. die_conv2d_wide, activation none: the model, over every CIN x COUT pair x k x padding on 17 x 66 and five pairs on eleven fields.
2. the epilogues against the device's own z of the same case: relu exactly, tanh within 1e-5 (test_gpu_nca_wide.py's ATOL, taken
   over; the worst distance is printed in fp32 ulps), the p = 0.5 mask exactly, p = 1 all zeros.
3. fp16, claim and stock planes past the first chunk of 4 input channels, stale claim words of the epoch before.
4. out_stride W * H, + 8, + 3 and an `out` 4 bytes off 16-byte alignment where H % 4 == 0.
5. die_nca_wide_sense_batch_store on a [2 or 3] -> 17 -> 16 -> 3 stack: episodes, weight and plane strides with gaps, fp16 fields,
   the agents channel, the masked launch, 64 replicas — against the model and against die_conv2d_wide chained by hand.
6. both adjoint sums of die_conv2d_wide_backward with activation none and relu, with and without a mask and grad_in.
7. random real values at 33 x 130 within 1e-5 * max(1, max |f64|), so that rounding stays in view.

Every output is prefilled with NaN between two 64-float NaN bands: the bands and the gaps between planes must stay NaN, every cell
the call owns must lose its NaN.  A test enqueues all its launches and synchronises once before it reads anything back."""
import ctypes as C

import numpy as np
import pytest
import torch

from die_amd import _lib as L
from die_amd.device_array import stream_ptr
from tests import dropout_model as D
from tests import nca_wide_domain_cases as K
from tests import nca_wide_grad_model as G

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
TAIL = 64                                                         # NaN floats before and behind every output
ATOL = 1e-5                                                       # tests/test_gpu_nca_wide.py's, for tanh
GROUPS = [name for name, _ in K.FIELD_GROUPS]
ACT = L.NCA_ACTIVATIONS
NAN = float('nan')


class Planes:
    """`cout` output planes `stride` floats apart inside a NaN buffer, TAIL floats of it before the first and behind the last;
    `shift` floats move the first plane off the buffer's alignment."""

    def __init__(self, cout, cells, stride=None, shift=0):
        self.cout, self.cells, self.stride, self.shift = cout, cells, cells if stride is None else stride, shift
        self.n = (cout - 1) * self.stride + cells
        self.buf = torch.full((TAIL + shift + self.n + TAIL,), NAN, dtype=torch.float32, device=DEV)
        self.ptr = self.buf.data_ptr() + 4 * (TAIL + shift)
        assert self.buf.data_ptr() % 16 == 0

    def host(self, what):
        """(cout, cells) float32: the planes; asserts that the bands and the gaps are NaN still and that no cell of a plane is."""
        h = self.buf.cpu().numpy()
        first = TAIL + self.shift
        assert np.isnan(h[:first]).all() and np.isnan(h[first + self.n:]).all(), f'{what}: written outside the planes'
        body = np.full(self.cout * self.stride, np.nan, dtype=np.float32)
        body[:self.n] = h[first:first + self.n]
        body = body.reshape(self.cout, self.stride)
        assert np.isnan(body[:, self.cells:]).all(), f'{what}: written between the planes'
        left = int(np.isnan(body[:, :self.cells]).sum())
        assert left == 0, f'{what}: {left} cells were never written'
        return body[:, :self.cells]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # (a copy: the cases' arrays are read-only)


def _inputs(x, kinds=None, words=None):
    """(tensors kept alive, die_conv_plane array) of a (cin, W, H) float32 array; `kinds`: the die_plane_kind of every plane (fp16
    planes are rounded — exactly, on the lattice —, claim and stock planes are `words`)."""
    kinds = (K.F32,) * len(x) if kinds is None else kinds
    keep = []
    for i, kind in enumerate(kinds):
        if kind == K.F32:
            keep.append(_dev(x[i].astype(np.float32)))
        elif kind == K.F16:
            assert np.array_equal(x[i].astype(np.float16).astype(np.float32), x[i])
            keep.append(_dev(x[i].astype(np.float16)))
        else:
            keep.append(_dev(words[i].view(np.int64)))
    return keep, (L.ConvPlane * len(x))(*[L.ConvPlane(t.data_ptr(), kind, 0) for t, kind in zip(keep, kinds)])


def _conv(W, H, arr, cin, cout, k, w_dev, act, mode, out, drop=None):
    L.check(L.lib.die_conv2d_wide(W, H, cin, arr, K.EPOCH, cout, out.ptr, out.stride, k, w_dev.data_ptr(), ACT[act], L.PAD_MODES[mode],
                                  None if drop is None else C.byref(drop), stream_ptr(DEV)), 'die_conv2d_wide')
    return out


def _launch_acts(cases, mode, acts):
    """Every case under every activation of `acts`, enqueued: [(case, {act: Planes}, kept tensors)]."""
    jobs = []
    for cin, cout, k, W, H in cases:
        c = K.case(cin, cout, k, W, H)
        keep, arr = _inputs(c['x'])
        w_dev = _dev(c['w'])
        outs = {act: _conv(W, H, arr, cin, cout, k, w_dev, act, mode, Planes(cout, W * H)) for act in acts}
        jobs.append(((cin, cout, k, W, H), outs, (keep, arr, w_dev)))
    return jobs


# ------------------------------------------------------------------------------------------------ 1. activation none, exactly
def _check_exact(cases, mode):
    jobs = _launch_acts(cases, mode, (None,))
    torch.cuda.synchronize()
    assert jobs
    for key, outs, _ in jobs:
        cin, cout, k, W, H = key
        got = outs[None].host(f'{key} {mode}').reshape(cout, W, H)
        want = K.case(*key)['z'][mode]
        bad = got != want
        assert not bad.any(), (f'{key} {mode}: {int(bad.sum())} of {bad.size} outputs differ from the model, the first at (o, x, y) = '
                               f'{tuple(int(v) for v in np.argwhere(bad)[0])}: {got[bad][0]!r} for {want[bad][0]!r}')
    return len(jobs)


@pytest.mark.parametrize('mode', K.MODES)
@pytest.mark.parametrize('k', K.KS)
def test_conv2d_wide_is_the_model_bit_for_bit_on_every_channel_pair(k, mode):
    assert _check_exact(K.cross_cases(k, mode), mode) == len(K.CIN) * len(K.COUT)


@pytest.mark.parametrize('mode', K.MODES)
@pytest.mark.parametrize('group', GROUPS)
def test_conv2d_wide_is_the_model_bit_for_bit_on_every_field(group, mode):
    _check_exact(K.field_cases(group, mode), mode)


# ------------------------------------------------------------------------------------------------ 2. the epilogues
def _check_epilogues(cases, mode):
    jobs = _launch_acts(cases, mode, (None, 'relu', 'tanh'))
    torch.cuda.synchronize()
    worst_ulps = worst_abs = 0.0
    for key, outs, _ in jobs:
        z = outs[None].host(f'{key} {mode} none')
        relu = outs['relu'].host(f'{key} {mode} relu')
        tanh = outs['tanh'].host(f'{key} {mode} tanh')
        assert np.array_equal(relu, np.where(z > 0, z, np.float32(0))), (key, mode, 'relu')
        want = np.tanh(z.astype(np.float64))
        worst_abs = max(worst_abs, float(np.abs(tanh - want).max()))
        worst_ulps = max(worst_ulps, K.ulps(tanh, want))
    print(f'tanh epilogue {mode}, {len(jobs)} cases: worst {worst_abs:.2e} from np.tanh(float64(z)) (ceiling {ATOL:.0e}), {worst_ulps:.2f} fp32 ulps')
    assert worst_abs <= ATOL
    return worst_ulps


@pytest.mark.parametrize('mode', K.MODES)
@pytest.mark.parametrize('k', K.KS)
def test_relu_is_exact_and_tanh_is_within_the_ceiling_on_every_channel_pair(k, mode):
    _check_epilogues(K.cross_cases(k, mode), mode)


@pytest.mark.parametrize('mode', K.MODES)
@pytest.mark.parametrize('group', GROUPS)
def test_relu_is_exact_and_tanh_is_within_the_ceiling_on_every_field(group, mode):
    _check_epilogues(K.field_cases(group, mode), mode)


@pytest.mark.parametrize('mode', ['circular', 'replicate'])
@pytest.mark.parametrize('cin', [5, 32])
def test_masked_planes_are_the_unmasked_planes_times_the_models_mask(cin, mode):
    """cout = 17 (two channel blocks, the second one ragged) on every field: H % 4 == 0 draws one Philox block per four cells,
    any other H draws cell by cell.  p = 0.5: the product is a doubling or a zero, exact.  p = 1: zeros."""
    cout, jobs = 17, []
    for W, H in K.FIELDS:
        for k in K.KS:
            c = K.case(cin, cout, k, W, H)
            keep, arr = _inputs(c['x'])
            w_dev = _dev(c['w'])
            seed = c['seed'] + 2 ** 40
            for act in (None, 'relu', 'tanh'):
                plain = _conv(W, H, arr, cin, cout, k, w_dev, act, mode, Planes(cout, W * H))
                half = _conv(W, H, arr, cin, cout, k, w_dev, act, mode, Planes(cout, W * H), L.nca_dropout(K.DROP_P, seed, 7, K.DROP_STEP))
                one = _conv(W, H, arr, cin, cout, k, w_dev, act, mode, Planes(cout, W * H), L.nca_dropout(1.0, seed, 0, K.DROP_STEP))
                jobs.append(((W, H, k, act), seed, plain, half, one, (keep, arr, w_dev)))
    torch.cuda.synchronize()
    assert {H % 4 == 0 for _, H in K.FIELDS} == {True, False}
    for (W, H, k, act), seed, plain, half, one, _ in jobs:
        where = f'{cin} -> {cout} k = {k} {W} x {H} {act} {mode}'
        t = plain.host(where).reshape(cout, W, H)
        mask = D.mask(seed, K.DROP_STEP, W, H, K.DROP_P)
        assert set(np.unique(mask)) <= {0.0, 2.0}
        assert np.array_equal(half.host(where + ' p = 0.5').reshape(cout, W, H), t * mask[None]), where
        assert (one.host(where + ' p = 1') == 0).all(), where
        if act is None:
            assert np.array_equal(t, K.case(cin, cout, k, W, H)['z'][mode])


# ------------------------------------------------------------------------------------------------ 3. plane kinds past chunk 0
@pytest.mark.parametrize('mode', K.MODES)
@pytest.mark.parametrize('cin', sorted(K.KIND_CASES))
def test_fp16_claim_and_stock_planes_past_the_first_chunk_read_as_their_values(cin, mode):
    jobs = []
    for W, H in K.KIND_FIELDS:
        for k in K.KIND_KS:
            if mode not in K.modes_for(W, H, k):
                continue
            c = K.kind_case(cin, k, W, H)
            keep, arr = _inputs(c['x'], c['kinds'], c['words'])
            w_dev = _dev(c['w'])
            jobs.append(((W, H, k), c, _conv(W, H, arr, cin, K.KIND_COUT, k, w_dev, None, mode, Planes(K.KIND_COUT, W * H)), (keep, w_dev)))
    torch.cuda.synchronize()
    assert len(jobs) >= 3
    for (W, H, k), c, out, _ in jobs:
        got = out.host(f'kinds {c["kinds"]} k = {k} {W} x {H} {mode}').reshape(K.KIND_COUT, W, H)
        assert np.array_equal(got, c['z'][mode]), (cin, k, W, H, mode, int((got != c['z'][mode]).sum()))


# ------------------------------------------------------------------------------------------------ 4. strides and alignment
@pytest.mark.parametrize('mode', K.MODES)
def test_plane_strides_and_an_unaligned_out_where_the_stores_are_16_bytes(mode):
    """H % 4 == 0.  out_stride W * H and + 8 keep the 16-byte stores, + 3 and an `out` 4 bytes off do not: the same values either
    way, and nothing written between or around the planes."""
    jobs = []
    for W, H in ((20, 68), (16, 64), (5, 4)):
        for cin, cout in ((3, 16), (5, 17), (32, 32)):
            for k in K.KS:
                c = K.case(cin, cout, k, W, H)
                keep, arr = _inputs(c['x'])
                w_dev = _dev(c['w'])
                for gap, shift in ((0, 0), (8, 0), (3, 0), (0, 1), (8, 1)):
                    out = _conv(W, H, arr, cin, cout, k, w_dev, None, mode, Planes(cout, W * H, W * H + gap, shift))
                    assert (out.ptr % 16 == 0) == (shift == 0)
                    jobs.append(((cin, cout, k, W, H, gap, shift), out, (keep, arr, w_dev)))
    torch.cuda.synchronize()
    for key, out, _ in jobs:
        cin, cout, k, W, H = key[:5]
        assert np.array_equal(out.host(f'{key} {mode}').reshape(cout, W, H), K.case(cin, cout, k, W, H)['z'][mode]), (key, mode)


# ------------------------------------------------------------------------------------------------ 5. the batched store call
class Stack:
    """One stack_case on the device: R replicas' planes `plane_stride` elements apart (claim words, fp32 or fp16 fields, NaN or stale
    words in the gaps) and every layer's R weight blocks STACK_WEIGHT_GAP floats apart (NaN in the gaps)."""

    def __init__(self, W, H, agents, mode, f16, gap, R=K.STACK_R):
        self.c = c = K.stack_case(W, H, agents, mode, R)
        self.W, self.H, self.R, self.agents, self.mode, self.f16 = W, H, R, agents, mode, f16
        self.cells = cells = W * H
        self.ps = ps = cells + gap
        rs = np.random.RandomState(K.case_seed('stack words', W, H, R))
        fields = np.full((2, R * ps), np.nan, dtype=np.float16 if f16 else np.float32)
        owner = K.claim_words(rs, np.zeros(R * ps), False)        # the gaps: unoccupied, a third of them stale
        for r in range(R):
            for q in range(2):
                fields[q, r * ps:r * ps + cells] = c['planes'][r, int(agents) + q].ravel()
            if agents:
                owner[r * ps:r * ps + cells] = K.claim_words(rs, c['planes'][r, 0], False).ravel()
        self.food, self.chem, self.owner = _dev(fields[0]), _dev(fields[1]), _dev(owner.view(np.int64))
        self.medium = L.Medium(W, H, L.DIE_F16 if f16 else L.DIE_F32, K.EPOCH, self.owner.data_ptr() if agents else None, self.food.data_ptr(),
                               self.chem.data_ptr(), None, 0, 0, 0, 0, 0, 0, 0, 0, None)
        self.batch = L.Batch(R, 0, ps, 1, 1, (C.c_int64 * 64)(*([0] * 64)))
        self.w_dev, self.w_stride = [], []
        for w in c['weights']:
            nw = w[0].size
            rows = np.full((R, nw + K.STACK_WEIGHT_GAP), np.nan, dtype=np.float32)
            rows[:, :nw] = w.reshape(R, nw)
            self.w_dev.append(_dev(rows))
            self.w_stride.append(nw + K.STACK_WEIGHT_GAP)

    def nca(self, E):
        cin, layers = self.c['cin0'], []
        for (k, cout, act), w, stride in zip(K.STACK_LAYERS, self.w_dev, self.w_stride):
            layers.append(L.NcaLayer(k, cin, cout, ACT[act], w.data_ptr(), stride))
            cin = cout
        self._layers = (L.NcaLayer * len(layers))(*layers)
        return L.NcaBatch(len(layers), L.PAD_MODES[self.mode], int(self.agents), K.EPOCH, self._layers, (C.c_float * 3)(0.1, 0.1, 2.0),
                          0 if E == 1 else E, None, 0)

    def store(self, E, drop):
        """die_nca_wide_sense_batch_store into guarded storage: (store, masked or None), each R * Cmax planes per layer."""
        nl, R, cells = len(K.STACK_LAYERS), self.R, self.cells
        need = L.lib.die_nca_wide_sense_batch_store_bytes(self.W, self.H, R, nl, K.STACK_CMAX)
        assert need == nl * R * K.STACK_CMAX * cells * 4
        store = Planes(nl * R * K.STACK_CMAX, cells)
        masked = Planes(R * K.STACK_CMAX, cells) if drop is not None else None
        nca = self.nca(E)
        L.check(L.lib.die_nca_wide_sense_batch_store(C.byref(self.medium), C.byref(self.batch), C.byref(nca), store.ptr, need,
                                                     None if masked is None else masked.ptr, None if drop is None else C.byref(drop),
                                                     stream_ptr(DEV)), 'die_nca_wide_sense_batch_store')
        return store, masked

    def by_hand(self, r, row):
        """The three layers of replica r under candidate `row` as stand-alone die_conv2d_wide launches, each reading the one before."""
        fk, esize = (K.F16, 2) if self.f16 else (K.F32, 4)
        planes = [L.ConvPlane(self.owner.data_ptr() + 8 * r * self.ps, K.AGENTS, 0)] if self.agents else []
        planes += [L.ConvPlane(t.data_ptr() + esize * r * self.ps, fk, 0) for t in (self.food, self.chem)]
        cin, outs = self.c['cin0'], []
        for (k, cout, act), w, stride in zip(K.STACK_LAYERS, self.w_dev, self.w_stride):
            arr = (L.ConvPlane * cin)(*planes)
            out = Planes(cout, self.cells)
            L.check(L.lib.die_conv2d_wide(self.W, self.H, cin, arr, K.EPOCH, cout, out.ptr, self.cells, k, w.data_ptr() + 4 * row * stride,
                                          ACT[act], L.PAD_MODES[self.mode], None, stream_ptr(DEV)), 'die_conv2d_wide')
            outs.append(out)
            planes, cin = [L.ConvPlane(out.ptr + 4 * o * self.cells, K.F32, 0) for o in range(cout)], cout
        return outs


def _layers_of(store, masked, R):
    """store -> [layer][replica] (cout, cells) arrays (channels past cout asserted NaN), masked -> [replica] (3, cells)."""
    nl = len(K.STACK_LAYERS)
    h = store.buf.cpu().numpy()
    assert np.isnan(h[:TAIL]).all() and np.isnan(h[TAIL + store.n:]).all(), 'written outside the store'
    st = h[TAIL:TAIL + store.n].reshape(nl, R, K.STACK_CMAX, -1)
    for l, (_, cout, _) in enumerate(K.STACK_LAYERS):
        assert not np.isnan(st[l, :, :cout]).any() and np.isnan(st[l, :, cout:]).all(), f'layer {l}: its cout planes and no others'
    ms = None
    if masked is not None:
        m = masked.buf.cpu().numpy()
        assert np.isnan(m[:TAIL]).all() and np.isnan(m[TAIL + masked.n:]).all(), 'written outside the masked planes'
        ms = m[TAIL:TAIL + masked.n].reshape(R, K.STACK_CMAX, -1)
        assert not np.isnan(ms[:, :3]).any() and np.isnan(ms[:, 3:]).all()
    return [[st[l, r, :cout] for r in range(R)] for l, (_, cout, _) in enumerate(K.STACK_LAYERS)], ms


def _check_stack(stacks, runs, R):
    """runs: (stack, E, seed stride or None, store, masked); the chains by hand are launched here, once per (replica, candidate)."""
    base = stacks[0]
    W, H, mode, c = base.W, base.H, base.mode, base.c
    hand = {p: base.by_hand(*p) for p in c['pairs']}
    torch.cuda.synchronize()
    model = {p: K.stack_model(c, *p, mode) for p in c['pairs']}
    hand = {p: [o.host(f'by hand {p} layer {l}') for l, o in enumerate(outs)] for p, outs in hand.items()}
    worst_abs = worst_ulps = 0.0
    for st, E, stride, store, masked in runs:
        layers, ms = _layers_of(store, masked, R)
        for r in range(R):
            p, where = (r, r // E), f'{W} x {H} {mode} E = {E} plane_stride {st.ps} replica {r}'
            for l in range(3):
                assert np.array_equal(layers[l][r], hand[p][l]), f'{where}: layer {l} is not the stand-alone launch'
            for l in range(2):
                assert np.array_equal(layers[l][r].astype(np.float64), model[p][l].reshape(len(layers[l][r]), -1)), f'{where}: layer {l} is not the model'
            want = np.tanh(model[p][2]).reshape(3, -1)
            worst_abs = max(worst_abs, float(np.abs(layers[2][r] - want).max()))
            worst_ulps = max(worst_ulps, K.ulps(layers[2][r], want))
            if stride is not None:
                mask = D.mask(STACK_SEED + r * stride, K.DROP_STEP, W, H, K.DROP_P).ravel()
                assert np.array_equal(ms[r, :3], layers[2][r] * mask[None]), f'{where}: masked planes, seed stride {stride}'
    assert worst_abs <= ATOL, worst_abs
    return worst_abs, worst_ulps


STACK_SEED = 2 ** 41 + 12345


@pytest.mark.parametrize('mode', K.MODES)
@pytest.mark.parametrize('f16', [False, True], ids=['fp32', 'fp16'])
@pytest.mark.parametrize('agents', [True, False], ids=['agents', 'fields_only'])
@pytest.mark.parametrize('W,H', K.STACK_FIELDS)
def test_sense_batch_store_is_the_model_and_the_stand_alone_launches(W, H, agents, f16, mode):
    """R = 6 x episodes 1, 2, 3 x plane_stride W * H, + 8, + 6 x (no mask, seed stride 0, seed stride 1)."""
    R = K.STACK_R
    stacks = [Stack(W, H, agents, mode, f16, gap) for gap in K.STACK_PLANE_GAPS]
    runs = []
    for st in stacks:
        for E in K.STACK_EPISODES:
            for stride in (None, *K.STACK_SEED_STRIDES):
                drop = None if stride is None else L.nca_dropout(K.DROP_P, STACK_SEED, stride, K.DROP_STEP)
                runs.append((st, E, stride, *st.store(E, drop)))
    worst_abs, worst_ulps = _check_stack(stacks, runs, R)
    print(f'store {W} x {H} {"agents" if agents else "fields"} {"fp16" if f16 else "fp32"} {mode}: {len(runs)} calls; last layer {worst_abs:.2e} from '
          f'tanh of the model (ceiling {ATOL:.0e}), {worst_ulps:.2f} fp32 ulps')


def test_sense_batch_store_with_64_replicas():
    """The last index of gridDim.z and of die_batch.n[64], on 5 x 4 (16-byte stores, a field below the k = 5 layer's tile and
    barely above its radius)."""
    R, W, H = 64, 5, 4
    st = Stack(W, H, True, 'circular', False, 6, R)
    runs = [(st, E, 1, *st.store(E, L.nca_dropout(K.DROP_P, STACK_SEED, 1, K.DROP_STEP))) for E in (1, 2)]
    _check_stack([st], runs, R)


# ------------------------------------------------------------------------------------------------ 6. the adjoint sums, exactly
def _adjoint_cases(k, mode):
    """(cin, cout, W, H, activation, masked, grad_in wanted): tests/nca_wide_grad_model.layer_cases without tanh, and activation x
    mask x grad_in crossed over its X_SHAPES x X_PAIRS at every k."""
    plain = [c for c in G.layer_cases(k, mode) if c[4] != 'tanh']
    cross = [(cin, cout, W, H, act, masked) for W, H in G.X_SHAPES for cin, cout in G.X_PAIRS for act in (None, 'relu') for masked in (False, True)]
    return [(*c, True) for c in dict.fromkeys(plain + cross)] + [(*c, False) for c in cross]


@pytest.mark.parametrize('mode', G.MODES)
@pytest.mark.parametrize('k', G.KS)
def test_backward_sums_are_the_model_bit_for_bit(k, mode):
    jobs = []
    for cin, cout, W, H, act, masked, want_gin in _adjoint_cases(k, mode):
        c = K.case(cin, cout, k, W, H)
        keep, arr = _inputs(c['x'])
        w_dev, g_dev = _dev(c['w']), _dev(c['g'])
        t = _conv(W, H, arr, cin, cout, k, w_dev, act, mode, Planes(cout, W * H))
        drop = L.nca_dropout(K.DROP_P, c['seed'], 0, K.DROP_STEP) if masked else None
        nw = cout * cin * k * k
        need = L.lib.die_conv2d_wide_backward_workspace_bytes(W, H, cin, cout, k)
        assert need == -(-W // 16) * -(-H // 64) * nw * 4
        gw, ws, gin = Planes(1, nw), Planes(1, need // 4), Planes(1, cin * W * H) if want_gin else None
        L.check(L.lib.die_conv2d_wide_backward(W, H, cin, arr, K.EPOCH, cout, g_dev.data_ptr(), W * H, t.ptr, W * H, k, w_dev.data_ptr(), ACT[act],
                                               L.PAD_MODES[mode], None if drop is None else C.byref(drop), gw.ptr, None if gin is None else gin.ptr,
                                               W * H, ws.ptr, need, stream_ptr(DEV)), 'die_conv2d_wide_backward')
        jobs.append(((cin, cout, W, H, act, masked, want_gin), c, t, gw, gin, ws, (keep, arr, w_dev, g_dev)))
    torch.cuda.synchronize()
    assert len(jobs) >= 100
    for key, c, t, gw, gin, ws, _ in jobs:
        cin, cout, W, H, act, masked, want_gin = key
        where = f'k = {k} {mode} {key}'
        ws.host(where + ': workspace')                             # exactly the stated bytes: all written, nothing behind them
        t = t.host(where + ': forward').reshape(cout, W, H)
        assert np.array_equal(t, G.act_forward(c['z'][mode], act)), where + ': forward'
        mask = D.mask(c['seed'], K.DROP_STEP, W, H, K.DROP_P) if masked else None
        want_w, want_in = G.layer_backward(c['x'], c['w'], c['g'], t, act, mask, mode)
        got_w = gw.host(where + ': grad_weights').reshape(cout, cin, k, k)
        assert np.array_equal(got_w.astype(np.float64), want_w), (where, 'grad_weights', int((got_w != want_w).sum()))
        if want_gin:
            got_in = gin.host(where + ': grad_in').reshape(cin, W, H)
            assert np.array_equal(got_in.astype(np.float64), want_in), (where, 'grad_in', int((got_in != want_in).sum()))


# ------------------------------------------------------------------------------------------------ 7. random real values
def test_random_real_values_stay_within_the_layer_bound():
    """The five pairs x k x padding at 33 x 130, x in +-[0.25, 1), Xavier weights: |device - float64| <= 1e-5 * max(1, max |f64|)."""
    W, H = K.RANDOM_FIELD
    jobs = []
    for cin, cout in K.PAIRS:
        for k in K.KS:
            c = K.random_case(cin, cout, k)
            keep, arr = _inputs(c['x'])
            w_dev = _dev(c['w'])
            for mode in K.MODES:
                jobs.append(((cin, cout, k, mode), c, _conv(W, H, arr, cin, cout, k, w_dev, None, mode, Planes(cout, W * H)), (keep, w_dev)))
    torch.cuda.synchronize()
    assert len(jobs) == 60
    worst = 0.0
    for key, c, out, _ in jobs:
        want = c['z'][key[3]]
        ratio = float(np.abs(out.host(str(key)).reshape(want.shape) - want).max() / (K.RANDOM_TOL * max(1.0, np.abs(want).max())))
        worst = max(worst, ratio)
        print(f'random {key}: error / bound {ratio:.3f}')
    print(f'random real values, 60 cases: worst error / bound {worst:.3f}')
    assert worst <= 1.0
