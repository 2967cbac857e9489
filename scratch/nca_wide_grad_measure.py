"""Times of one wide layer's forward and adjoint (LABBOOK §27), by device events: warm-up, then the median of single timed calls.

    python scratch/nca_wide_grad_measure.py [--reps 40] [--warmup 10] [--profile]

Per configuration: die_conv2d_wide (tanh), die_conv2d_wide_backward without grad_in (weight-gradient kernel + fold) and with it
(+ the input-gradient kernel), and torch's own circular pad + conv2d + tanh forward and autograd backward on the same tensors.
`--profile`: no events, 20 calls of each of ours per configuration, for a `rocprofv3 --kernel-trace --stats` run of its own."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from die_amd import functional as F          # noqa: E402

CONFIGS = [(size, cin, cout, k) for size in (96, 1024) for cin, cout, k in ((3, 16, 3), (16, 16, 3), (32, 32, 3), (32, 32, 5))]
DEV = 'cuda:0'


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--reps', type=int, default=40)
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--profile', action='store_true')
    args = p.parse_args()
    torch.manual_seed(0)
    for size, cin, cout, k in CONFIGS:
        x = torch.rand((cin, size, size), device=DEV)
        w = (torch.rand((cout, cin, k, k), device=DEV) - 0.5) / (cin * k * k) ** 0.5
        g = torch.randn((cout, size, size), device=DEV)
        act, pad = 1, 0
        t = F._launch_forward(x, w, act, pad, None)
        ours = dict(fwd=lambda: F._launch_forward(x, w, act, pad, None),
                    bwd_w=lambda: F._launch_backward(x, w, g, t, act, pad, None, False),
                    bwd_w_in=lambda: F._launch_backward(x, w, g, t, act, pad, None, True))
        if args.profile:
            for fn in ours.values():
                for _ in range(20):
                    fn()
            torch.cuda.synchronize()
            continue
        r = k // 2
        xt, wt = x.clone().requires_grad_(True), w.clone().requires_grad_(True)

        def torch_fwd():
            xp = torch.nn.functional.pad(xt[None], (r, r, r, r), mode='circular') if r else xt[None]
            return torch.tanh(torch.nn.functional.conv2d(xp, wt))[0]

        y = torch_fwd()
        res = {n: timed(fn, args.reps, args.warmup) for n, fn in ours.items()}
        res['torch_fwd'] = timed(torch_fwd, args.reps, args.warmup)
        res['torch_bwd_w_in'] = timed(lambda: torch.autograd.grad(y, (wt, xt), g, retain_graph=True), args.reps, args.warmup)
        res['torch_bwd_w'] = timed(lambda: torch.autograd.grad(y, (wt,), g, retain_graph=True), args.reps, args.warmup)
        gemm = 2.0 * cin * cout * k * k * size * size
        res.update(size=size, cin=cin, cout=cout, k=k, gemm_gflop=gemm / 1e9,
                   fwd_tflops=gemm / res['fwd'] / 1e6, bwd_w_tflops=gemm / res['bwd_w'] / 1e6,
                   bwd_w_in_tflops=2 * gemm / res['bwd_w_in'] / 1e6)
        print(json.dumps({n: (round(v, 2) if isinstance(v, float) else v) for n, v in res.items()}), flush=True)


if __name__ == '__main__':
    main()
