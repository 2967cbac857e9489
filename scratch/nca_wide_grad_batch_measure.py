"""Forward + backward of a population of wide stacks (LABBOOK §28), by device events: warm-up, then the median of single timed calls.

    python scratch/nca_wide_grad_batch_measure.py [--replicas 16] [--size 96] [--width 16] [--reps 40] [--warmup 10] [--profile WHICH]

Two ways to the same 16 gradients of a 3 -> 16 -> 16 -> 3, k = 3, tanh stack on 16 worlds:
  batched   BatchedNeuralAutomataAgent.forward_device + backward: L launches forward, 3 L - 1 backward for all worlds;
  loop      the worlds one at a time through the stand-alone ConvolutionModel.forward_device + backward (models on the device).
The upstream gradient on the sense planes is a fixed standard normal tensor; the loss is <sense, g> either way.
`--profile batched|loop`: no events, 20 calls of that form, for a `rocprofv3 --kernel-trace --stats` run of its own."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import die_amd as die                                            # noqa: E402
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent   # noqa: E402

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
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--replicas', type=int, default=16)
    p.add_argument('--size', type=int, default=96)
    p.add_argument('--width', type=int, default=16)
    p.add_argument('--reps', type=int, default=40)
    p.add_argument('--warmup', type=int, default=10)
    p.add_argument('--profile', choices=('batched', 'loop'))
    args = p.parse_args()
    R, S = args.replicas, args.size
    benv = BatchedEnv((S, S), die.Dynamics(food_infinite=True), replicas=R, seed=0, device=DEV)
    torch.manual_seed(0)
    template = die.NeuralAutomataAgent(kernel_sizes=(3, 3, 3), hidden_channels=args.width, hidden_activation='tanh', scale=0.1, deposit=2.0)
    P = sum(k.weight.numel() for k in template.model.conv_layers())
    pop = BatchedNeuralAutomataAgent(benv, template, torch.rand((R, P)) - 0.5)
    benv.run(pop, 2)
    g = torch.randn((R, 3, S, S), device=DEV)
    planes = benv.medium_tensor().clone()
    param = pop.parameters.detach().clone().requires_grad_()
    models = [pop.replica_agent(r).model.to(DEV) for r in range(R)]

    def batched():
        param.grad = None
        (pop.forward_device(param) * g).sum().backward()

    def loop():
        for r in range(R):
            models[r].zero_grad(set_to_none=True)
            (models[r].forward_device(planes[r]) * g[r]).sum().backward()

    batched()
    loop()
    torch.cuda.synchronize()
    same = all(torch.equal(param.grad[r], torch.nn.utils.parameters_to_vector([q.grad for q in models[r].parameters()])) for r in range(R))
    print(f'{R} worlds of {S} x {S}, 3 -> {args.width} -> {args.width} -> 3, k = 3, tanh, P = {P}: the two forms give the same bits: {same}')
    if args.profile:
        fn = batched if args.profile == 'batched' else loop
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        return
    tb, tl = timed(batched, args.reps, args.warmup), timed(loop, args.reps, args.warmup)
    tb2, tl2 = timed(batched, args.reps, args.warmup), timed(loop, args.reps, args.warmup)      # and again, alternating
    for name, t in (('batched', tb), ('loop', tl), ('batched again', tb2), ('loop again', tl2)):
        print(f'{name:14s} median {t[0]:9.1f} us  (min {t[1]:.1f}, max {t[2]:.1f}; {args.reps} calls after {args.warmup} warm-up)')
    print(f'loop / batched: {tl[0] / tb[0]:.2f} and {tl2[0] / tb2[0]:.2f}')


if __name__ == '__main__':
    main()
