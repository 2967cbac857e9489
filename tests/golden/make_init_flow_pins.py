"""Generates tests/golden/init_flow_pins.json — one SHA-256 per case over the raw bytes of every array that the
world-building entry points (initialisation, headings, food flows, the NeuralAutomataAgent read-out; stand-alone and
batched) write for fixed inputs, recorded on an MI355X at the commit named in the file.

The stand-alone and the batched kernels of these entry points call the same device bodies; the existing tests compare one
family against the other (both are code under change when a body is edited) or against the float64 oracle (within
tolerances).  This file pins the bits themselves: tests/test_gpu_init_flow_pins.py imports CASES from here, recomputes
every digest and compares.

Run (needs the GPU; only when a change of values is intended):  python tests/golden/make_init_flow_pins.py
"""
import ctypes as C
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, 'init_flow_pins.json')
DEV = 'cuda:0'
U64 = 0xFFFFFFFFFFFFFFFF


def _imports():
    import torch
    from die_amd import _lib
    from die_amd.data_init import food_spec_from_seed
    from die_amd.device_array import _ptr, stream_ptr, to_q32
    return torch, _lib, food_spec_from_seed, _ptr, stream_ptr, to_q32


def _fdt(L, torch, half):
    return (L.DIE_F16, torch.float16) if half else (L.DIE_F32, torch.float32)


def _host(torch, *tensors):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


class _World:
    """Planes and agent arrays of R replicas (R = 1: a stand-alone world, or a tile of one when `tile` is given)."""

    def __init__(self, W, H, half, N, R=1, tile=None):
        torch, L, _, _ptr, _, _ = _imports()
        self.fdt, dt = _fdt(L, torch, half)
        self.W, self.H, self.N, self.R = W, H, N, R
        self.owner = torch.zeros((R, W, H), dtype=torch.int64, device=DEV)
        self.food = torch.full((R, W, H), -1, dtype=dt, device=DEV)
        self.chem = torch.full((R, W, H), -1, dtype=dt, device=DEV)
        self.x = torch.full((R, N), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        self.y = torch.full((R, N), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        self.alive = torch.full((R, N), 7, dtype=torch.uint8, device=DEV)
        self.agent_food = torch.full((R, N), -1, dtype=torch.float32, device=DEV)
        self.counts = torch.zeros((R, 2), dtype=torch.int64, device=DEV)
        g = tile or (0, 0, 0, 0)
        self.m = L.Medium(W, H, self.fdt, 1, _ptr(self.owner), _ptr(self.food), _ptr(self.chem), None, *g, 0, 0, 0, 0, None)
        self.a = L.Agents(N, _ptr(self.x), _ptr(self.y), _ptr(self.alive), _ptr(self.agent_food), None)

    def arrays(self):
        torch = _imports()[0]
        return _host(torch, self.owner, self.food, self.chem, self.x, self.y, self.alive, self.agent_food, self.counts)


# (gW, gH, ox, oy) of the decomposed tile: 64x56 planes at offset (-8, -8) of a 96x80 world; its interior is [8, 56) x [8, 48)
TILE = (96, 80, -8, -8)


def init_stand_alone(W, H, half, N, food='perlin', tile=None, seed=1234, ratio=0.15):
    def run():
        torch, L, food_spec, _ptr, stream_ptr, _ = _imports()
        spec = food_spec(seed, scale=0.5, perlin_octaves=8 if food == 'perlin' else 0, threshold=1.0)
        if N == 'half':                                     # half as many slots as seeded agents: the clip and total[1] == 1
            w = _World(W, H, half, 1)
            L.check(L.lib.die_init_medium(C.byref(w.m), ratio, seed, C.byref(spec), stream_ptr(DEV)), 'die_init_medium')
            w = _World(W, H, half, int(w.owner.ne(0).sum().item()) // 2)
        else:
            w = _World(W, H, half, N, tile=tile)
        L.check(L.lib.die_init_medium(C.byref(w.m), ratio, seed, C.byref(spec), stream_ptr(DEV)), 'die_init_medium')
        if tile:
            mask = torch.zeros((1, W, H), dtype=torch.bool, device=DEV)
            mask[:, 8:56, 8:48] = True
            w.owner.mul_(mask)
        ws = torch.empty(L.lib.die_workspace_bytes(W, H, w.N), dtype=torch.uint8, device=DEV)
        L.check(L.lib.die_init_agents(C.byref(w.m), C.byref(w.a), seed, _ptr(w.counts), _ptr(ws), ws.numel(), stream_ptr(DEV)),
                'die_init_agents')
        arrays = w.arrays()
        assert int(arrays[-1][0, 1]) == (1 if N == 'half' else 0), arrays[-1]
        return arrays
    return run


def init_batch(W, H, half, how, clip=False, R=3, seed=1234, ratio=0.15):
    """how: ('stride', s) for die_init_batch, ('seeds', [...]) for die_init_batch_seeds.  clip: replica 1 gets half its seeded
    count of slots and the call is made twice on the same counts."""
    def run():
        torch, L, food_spec, _ptr, stream_ptr, _ = _imports()
        N = W * H
        w = _World(W, H, half, N, R=R)
        n = [N] * R
        ws = torch.empty(L.lib.die_init_batch_workspace_bytes(W, H, R), dtype=torch.uint8, device=DEV)

        def call():
            b = L.Batch(R, 0, W * H, N, 1, (C.c_int64 * 64)(*n))
            if how[0] == 'stride':
                spec = food_spec(seed, scale=0.5, perlin_octaves=8, threshold=1.0)
                L.check(L.lib.die_init_batch(C.byref(w.m), C.byref(w.a), C.byref(b), ratio, seed, how[1], C.byref(spec), _ptr(w.counts),
                                             _ptr(ws), ws.numel(), stream_ptr(DEV)), 'die_init_batch')
            else:
                spec = food_spec(how[1][0], scale=0.5, perlin_octaves=8, threshold=1.0)
                L.check(L.lib.die_init_batch_seeds(C.byref(w.m), C.byref(w.a), C.byref(b), ratio, (C.c_uint64 * R)(*how[1]), R,
                                                   C.byref(spec), _ptr(w.counts), _ptr(ws), ws.numel(), stream_ptr(DEV)),
                        'die_init_batch_seeds')
        call()
        if clip:
            torch.cuda.synchronize()
            seeded = w.counts[:, 0].tolist()
            assert w.counts[:, 1].tolist() == [0] * R, w.counts
            n[1] = seeded[1] // 2
            call()
            call()
            torch.cuda.synchronize()
            assert w.counts[:, 1].tolist() == [0, 1] + [0] * (R - 2) and w.counts[1, 0].item() == n[1], w.counts
        return w.arrays()
    return run


def heading(N, turn, with_prev, seed=7):
    def run():
        torch, L, _, _ptr, stream_ptr, _ = _imports()
        hi = torch.full((N,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        lo, pg = hi.clone(), torch.full((2, N), -1, dtype=torch.float32, device=DEV)
        L.check(L.lib.die_init_heading(_ptr(hi), _ptr(lo), _ptr(pg[0]) if with_prev else None, _ptr(pg[1]) if with_prev else None, N,
                                       turn, seed, stream_ptr(DEV)), 'die_init_heading')
        return _host(torch, hi, lo, pg)
    return run


def heading_batch(n=(20000, 7, 300), turns=(30.0, 45.0, 7.5), seed=7):
    def run():
        torch, L, _, _ptr, stream_ptr, _ = _imports()
        R, stride = len(n), max(n)
        rows = (L.PhysarumRow * R)()
        for r, deg in enumerate(turns):
            rows[r].turn_radians = math.radians(deg)
        table = torch.from_numpy(np.frombuffer(bytes(rows), dtype=np.uint8).copy()).to(DEV)
        hi = torch.full((R, stride), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        lo = hi.clone()
        b = L.Batch(R, 0, 0, stride, 1, (C.c_int64 * 64)(*n))
        L.check(L.lib.die_physarum_heading_batch(_ptr(hi), _ptr(lo), C.byref(b), _ptr(table), seed, stream_ptr(DEV)),
                'die_physarum_heading_batch')
        return _host(torch, hi, lo)
    return run


def _plane(torch, R, W, H, dt):
    return torch.from_numpy(np.random.RandomState(3).rand(R, W, H)).to(device=DEV, dtype=dt)


def flow_stand_alone(kind, W, H, half, t, tile=None):
    def run():
        torch, L, _, _ptr, stream_ptr, _ = _imports()
        fdt, dt = _fdt(L, torch, half)
        food = _plane(torch, 1, W, H, dt)
        m = L.Medium(W, H, fdt, 1, None, _ptr(food), None, None, *(tile or (0, 0, 0, 0)), 0, 0, 0, 0, None)
        if kind == 'wave':
            L.check(L.lib.die_food_flow_wave(C.byref(m), t, 0.5, 0.5, stream_ptr(DEV)), 'die_food_flow_wave')
        else:
            L.check(L.lib.die_food_flow_perlin(C.byref(m), t, 8, 0.5, 0.5, 11, stream_ptr(DEV)), 'die_food_flow_perlin')
        return _host(torch, food)
    return run


def flow_batch(kind, half, R, mask=None, W=96, H=80, t=0.37):
    def run():
        torch, L, _, _ptr, stream_ptr, _ = _imports()
        fdt, dt = _fdt(L, torch, half)
        food = _plane(torch, R, W, H, dt)
        m = L.Medium(W, H, fdt, 1, None, _ptr(food), None, None, 0, 0, 0, 0, 0, 0, 0, 0, None)
        b = L.Batch(R, 0, W * H, 1, 1, (C.c_int64 * 64)(*([1] * R)))
        flow, octaves = (L.DIE_FLOW_WAVE, 0) if kind == 'wave' else (L.DIE_FLOW_PERLIN, 8)
        if mask is None:
            L.check(L.lib.die_food_flow_batch(C.byref(m), C.byref(b), flow, t, 0.5, 0.5, octaves, 11, stream_ptr(DEV)), 'die_food_flow_batch')
        else:
            L.check(L.lib.die_food_flow_batch_masked(C.byref(m), C.byref(b), flow, t, 0.5, 0.5, octaves, 11, mask, stream_ptr(DEV)),
                    'die_food_flow_batch_masked')
        return _host(torch, food)
    return run


def _distinct_slots(rs, W, H, R, N):
    """(R, N) Q0.32 words of slots standing on distinct cells of each replica (the adjoint's float atomics then add one term per
    cell: no order to depend on)."""
    _, _, _, _, _, to_q32 = _imports()
    cells = np.stack([rs.permutation(W * H)[:N] for _ in range(R)])
    x = to_q32((cells // H + 0.5) / W).view(np.int32)
    y = to_q32((cells % H + 0.5) / H).view(np.int32)
    return x, y


COEFS = (0.5, 0.25, 2.0)


def read_out(batched, backward, W=96, H=80, N=500, n=(500, 7, 300)):
    def run():
        torch, L, _, _ptr, stream_ptr, _ = _imports()
        rs = np.random.RandomState(5)
        R = len(n) if batched else 1
        x, y = (torch.from_numpy(v).to(DEV) for v in _distinct_slots(rs, W, H, R, N))
        planes = torch.from_numpy(rs.randn(R, 3, W, H).astype(np.float32)).to(DEV)       # forward: the sense planes; backward: cleared by the call, then one term added per cell
        act = torch.from_numpy(rs.randn(3, R, N).astype(np.float32)).to(DEV)             # forward: overwritten; backward: the gradient
        m = L.Medium(W, H, L.DIE_F32, 1, None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, None)
        a = L.Agents(N, _ptr(x), _ptr(y), None, None, None)
        u = L.Action(N, act[0].data_ptr(), act[1].data_ptr(), act[2].data_ptr())
        coefs, s = (C.c_float * 3)(*COEFS), stream_ptr(DEV)
        if batched:
            b = L.Batch(R, 0, W * H, N, 1, (C.c_int64 * 64)(*n))
            if backward:
                L.check(L.lib.die_gather_scale_backward_batch(C.byref(m), C.byref(a), C.byref(b), C.byref(u), coefs, _ptr(planes), 3 * W * H, s),
                        'die_gather_scale_backward_batch')
            else:
                L.check(L.lib.die_gather_scale_batch(C.byref(m), C.byref(a), C.byref(b), _ptr(planes), 3 * W * H, coefs, C.byref(u), s),
                        'die_gather_scale_batch')
        else:
            ptrs = (C.c_void_p * 3)(*[planes[0, q].data_ptr() for q in range(3)])
            if backward:
                L.check(L.lib.die_gather_scale_backward(C.byref(m), C.byref(a), C.byref(u), coefs, ptrs, s), 'die_gather_scale_backward')
            else:
                L.check(L.lib.die_gather_scale(C.byref(m), C.byref(a), ptrs, coefs, C.byref(u), s), 'die_gather_scale')
        return _host(torch, planes, act)
    return run


def _cases():
    out = {}
    for half in (False, True):
        p = 'f16' if half else 'f32'
        for W, H in ((16, 12), (96, 80), (1040, 1028)):
            out[f'init {W}x{H} {p}'] = init_stand_alone(W, H, half, W * H)
        out[f'init 96x80 {p} clipped'] = init_stand_alone(96, 80, half, 'half')
        out[f'init 96x80 {p} wave-mix food'] = init_stand_alone(96, 80, half, 96 * 80, food='waves')
        out[f'init tile 64x56 of 96x80 {p}'] = init_stand_alone(64, 56, half, 64 * 56, tile=TILE)
        for W, H in ((96, 80), (1040, 1028)):
            for how in (('stride', 0), ('stride', 1), ('seeds', [5, 5, 9])):
                out[f'init_batch {W}x{H} {p} {how[0]} {how[1]}'] = init_batch(W, H, half, how)
        for how in (('stride', 1), ('seeds', [5, 5, 9])):
            out[f'init_batch 96x80 {p} {how[0]} {how[1]} replica 1 clipped, twice'] = init_batch(96, 80, half, how, clip=True)
        for kind in ('wave', 'perlin'):
            for W, H in ((40, 64), (37, 91)):
                for t in (0.0, 0.37):
                    out[f'flow {kind} {W}x{H} {p} t={t}'] = flow_stand_alone(kind, W, H, half, t)
            out[f'flow {kind} tile 64x56 of 96x80 {p}'] = flow_stand_alone(kind, 64, 56, half, 0.37, tile=TILE)
            for R, part in ((3, 0b101), (17, 0b1_0000_0000_0000_0101)):
                out[f'flow_batch {kind} {p} R={R}'] = flow_batch(kind, half, R)
                out[f'flow_batch_masked {kind} {p} R={R} full'] = flow_batch(kind, half, R, mask=(1 << R) - 1)
                out[f'flow_batch_masked {kind} {p} R={R} mask {part:#b}'] = flow_batch(kind, half, R, mask=part)
    for turn in (math.radians(30), 0.0):
        for with_prev in (True, False):
            out[f'heading turn={turn:.4f} prev={with_prev}'] = heading(20000, turn, with_prev)
    out['heading_batch'] = heading_batch()
    for batched in (False, True):
        for backward in (False, True):
            out[f'read_out batched={batched} backward={backward}'] = read_out(batched, backward)
    return out


CASES = _cases()


def digest(arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    commit = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip() or \
        os.environ.get('DIE_PINS_COMMIT', 'unknown')
    pins = {name: digest(run()) for name, run in CASES.items()}
    with open(OUT, 'w') as f:
        json.dump({'commit': commit, 'pins': pins}, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', OUT, len(pins), 'cases at', commit)


if __name__ == '__main__':
    main()
