"""The measurements of LABBOOK §26 (wide NeuralAutomataAgent stacks).  One configuration per process, so that a
`rocprofv3 --kernel-trace --stats` run of it attributes every kernel to that configuration:

    python scratch/nca_wide_measure.py wide    --width 16 --stack 3,3     # R populations' steps: k_conv_wide<K, NB> per layer
    python scratch/nca_wide_measure.py grouped --width 16 --stack 3,3     # the yardstick: torch's grouped conv2d, groups = R
    python scratch/nca_wide_measure.py narrow                             # the default 3-channel stack, the same steps

`wide` / `narrow` step a BatchedEnv of R replicas of size x size; `grouped` evaluates the same R models on the same planes with
F.pad(mode='circular') + F.conv2d(groups=R) + the activation per layer.  Each prints the device-event time per step (or per
evaluation) of the timed window and the flop and bytes one evaluation of the stack needs, from the shapes."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import die_amd as die                                                      # noqa: E402
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent           # noqa: E402

REFERENCE_DYNAMICS = dict(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8)


def stack_cost(sizes, width, cells, R):
    """(flop, HBM bytes) of one evaluation of the stack for R replicas: 2 MAC flop, every layer reads its inputs and writes its
    outputs once, fp32."""
    chans = [3] + [width] * (len(sizes) - 1) + [3]
    flop = sum(2 * chans[i] * chans[i + 1] * k * k for i, k in enumerate(sizes)) * cells * R
    byts = sum(4 * (chans[i] + chans[i + 1]) for i in range(len(sizes))) * cells * R
    return flop, byts


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3                               # microseconds per call


def main():
    p = argparse.ArgumentParser()
    p.add_argument('mode', choices=('wide', 'narrow', 'grouped'))
    p.add_argument('--width', type=int, default=16)
    p.add_argument('--stack', default='3,3')
    p.add_argument('--activation', default='tanh')
    p.add_argument('--replicas', type=int, default=16)
    p.add_argument('--size', type=int, default=96)
    p.add_argument('--iters', type=int, default=300)
    p.add_argument('--warmup', type=int, default=20)
    args = p.parse_args()
    sizes = [int(k) for k in args.stack.split(',')]
    R, S = args.replicas, args.size
    torch.manual_seed(0)
    kw = {} if args.mode == 'narrow' else dict(hidden_channels=args.width, hidden_activation=None if args.activation == 'none' else args.activation)
    template = die.NeuralAutomataAgent(kernel_sizes=sizes, scale=0.01, deposit=2.0, **kw)
    template.model.init_weights()
    benv = BatchedEnv((S, S), die.Dynamics(init_agent_ratio=0.15, **REFERENCE_DYNAMICS), replicas=R, seed=1)
    pop = BatchedNeuralAutomataAgent(benv, template)
    pop.parameters.normal_(0, 0.1)
    flop, byts = stack_cost(sizes, 3 if args.mode == 'narrow' else args.width, S * S, R)
    tag = f'{args.mode} width {3 if args.mode == "narrow" else args.width} stack {tuple(sizes)} R {R} {S}x{S}'
    if args.mode in ('wide', 'narrow'):
        us = timed(lambda: benv.step(pop), args.warmup, args.iters)
        print(f'{tag}: {us:.1f} us per step of {R} replicas (device events, the whole step); the stack alone needs '
              f'{flop / 1e6:.1f} Mflop and {byts / 1e6:.2f} MB', flush=True)
        return
    # the yardstick: the same R models on the same planes through torch's grouped convolution
    layers = template.model.conv_layers()
    ws, off = [], 0
    for k in layers:
        n = k.weight.numel()
        cout, cin, kk, _ = k.weight.shape
        ws.append(pop.parameters[:, off:off + n].reshape(R * cout, cin, kk, kk).contiguous())
        off += n
    occ = (((benv.owner >> (32 + 27)) & 31) == benv.epoch).to(torch.float32)
    x = torch.stack([occ, benv.food, benv.chem], dim=1).reshape(1, R * 3, S, S).contiguous()
    act = {'tanh': torch.tanh, 'relu': torch.relu, 'none': lambda z: z}[args.activation]

    def evaluate():
        z = x
        for li, w in enumerate(ws):
            r = w.shape[-1] // 2
            if r:
                z = F.pad(z, (r, r, r, r), mode='circular')
            z = F.conv2d(z, w, groups=R)
            z = torch.tanh(z) if li == len(ws) - 1 else act(z)
        return z

    with torch.no_grad():
        us = timed(evaluate, args.warmup, args.iters)
        want = evaluate().reshape(R, 3, S, S)
    benv.step(pop)                                                         # (its sensing read the planes `x` was built from)
    diff = max(float((torch.from_numpy(pop.render(r)).to(want.device) - want[r].permute(1, 2, 0)).abs().max()) for r in range(R))
    print(f'{tag}: {us:.1f} us per evaluation of {R} models (device events); {flop / 1e6:.1f} Mflop, {byts / 1e6:.2f} MB; '
          f'largest difference from the population\'s own sense planes {diff:.2e}', flush=True)


if __name__ == '__main__':
    main()
