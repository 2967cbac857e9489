"""Backpropagation through the medium for a population: C students with signal channels trained on R = C·E batched worlds in ONE
optimiser step — `examples/recurrent_agent.py --signal-channels K` for `BatchedNeuralAutomataAgent`.

The worlds, the teacher and the loss are those of `recurrent_agent.py --replicas`: a `BatchedPhysarumAgent`, whose heading is
state, drives a `BatchedEnv` and hands out its actions as targets; every optimiser step is one episode — the worlds reset, `--warm`
steps of the teacher alone, then a window of `--unroll T` steps.  The students are `NeuralAutomataAgent(signal_channels=K,
memory_channels=M)` (M may be 0): on each of the T observations they compute `signalling_action(signals, memory)`, the fields and
the memories blank at the window's start and `signals_next` / `memory_next` handed from step to step, so that `loss.backward()`
runs through the field's update of every step (ONE die_signal_step_backward_batch launch for all K·R planes), the stack
(die_nca_wide_backward_batch_signal) and the memory, for all R worlds at once; the gradient is (C, P), one row a student.
`--detach-every` cuts the field's and the memory's gradient every so many steps inside a window.  `--time` prints optimiser steps
and world-steps per second.

    python examples/signalling_population.py --size 96 --replicas 16 --students 16 --signal-channels 2 --memory-channels 2 --unroll 8
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from recurrent_agent import DEPOSIT, SCALE, make_student                                  # noqa: E402
from die_amd import Dynamics                                                              # noqa: E402
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent, BatchedPhysarumAgent    # noqa: E402


def check_arguments(replicas, students, signal_channels, memory_channels):
    """(students, episodes), or SystemExit with the option to change."""
    students = replicas if students is None else students
    if replicas < 1:
        raise SystemExit('--replicas at least 1')
    if students < 1 or replicas % students:
        raise SystemExit(f'--students {students} must divide --replicas {replicas}')
    if not 1 <= signal_channels <= 8:
        raise SystemExit('--signal-channels 1..8 (students without a signal field: examples/recurrent_agent.py --replicas)')
    if not 0 <= memory_channels <= 8:
        raise SystemExit('--memory-channels 0..8')
    return students, replicas // students


def train(size, signal_channels, memory_channels, unroll, detach_every, steps, lr=1e-2, seed=0, hidden_channels=8, warm=4, replicas=4,
          students=None, log=print, timed=False):
    """`steps` Adam steps on R = `replicas` worlds at once, `students` candidates (default R) of E = R / students worlds each.  The
    loss is the sum over the students of their mean squared error against the teacher's (dx, dy), so that every student's row of the
    (C, P) gradient is its own.  Returns (the BatchedNeuralAutomataAgent, the list of mean losses per student)."""
    students, episodes = check_arguments(replicas, students, signal_channels, memory_channels)
    env = BatchedEnv((size, size), Dynamics(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8), replicas=replicas, seed=seed)
    template = make_student(memory_channels, hidden_channels, seed, signal_channels)
    rows = []
    for _ in range(students):                                     # different initialisations side by side
        template.model.init_weights()
        rows.append(torch.nn.utils.parameters_to_vector(template.model.parameters()).detach().clone())
    pop = BatchedNeuralAutomataAgent(env, template, torch.stack(rows), episodes)
    pop.parameters.requires_grad_()
    opt = torch.optim.Adam([pop.parameters], lr=lr)
    target = torch.zeros((3, env.R, env.Nmax), device=env.device)
    exists = torch.zeros((env.R, env.Nmax), dtype=torch.bool, device=env.device)
    for r in range(env.R):
        exists[r, :env.n[r]] = True
    tag = f'K={signal_channels} M={memory_channels} R={replicas} C={students}'
    losses, t0 = [], None
    warmup = max(1, steps // 10)
    for it in range(steps):
        if timed and it == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        env.reset()
        teacher = BatchedPhysarumAgent(env, scale=SCALE, deposit=DEPOSIT, seed=seed)
        for _ in range(warm):
            env.step(teacher)
        pop.reset_state()
        signals, memory, loss = None, None, 0.
        for t in range(unroll):
            if t and detach_every and t % detach_every == 0:
                signals, memory = signals.detach(), None if memory is None else memory.detach()
            got, signals, memory = pop.signalling_action(signals, memory)      # the students look at the worlds the teacher is about to act on
            live = (exists & (env.alive > 0)).reshape(students, -1)
            env.step(teacher, action=target)                      # its actions on those worlds: the targets
            err = (((got[:2] - target[:2]) / SCALE) ** 2).sum(0).reshape(students, -1)
            loss = loss + ((err * live).sum(1) / (2 * live.sum(1).clamp(min=1))).sum()
        loss = loss / unroll
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()) / students)
        if it % 10 == 0 or it == steps - 1:
            log(f'{tag} step {it:5d}: mean loss per student {losses[-1]:.6f}')
    if t0 is not None and steps > warmup:
        torch.cuda.synchronize()
        rate = (steps - warmup) / (time.perf_counter() - t0)
        log(f'{tag}, T={unroll}: {rate:.2f} optimiser steps/s over {steps - warmup} steps ({rate * replicas * unroll:.0f} world-steps/s)')
    return pop, losses


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--size', type=int, default=96)
    p.add_argument('--replicas', type=int, default=4, metavar='R', help='batched worlds')
    p.add_argument('--students', type=int, default=None, metavar='C', help='C students of R / C worlds each (default R)')
    p.add_argument('--signal-channels', type=int, default=2, metavar='K', help='planes of the signal field the agents write and read, 1..8')
    p.add_argument('--memory-channels', type=int, default=2, metavar='M', help='values every agent carries between steps, 0..8')
    p.add_argument('--unroll', type=int, default=8, metavar='T', help='env steps per optimiser step')
    p.add_argument('--detach-every', type=int, default=0, metavar='K', help="cut the field's and the memory's gradient every K steps of a window "
                                                                            '(0: never)')
    p.add_argument('--steps', type=int, default=200, help='optimiser steps')
    p.add_argument('--warm', type=int, default=4, help='steps the teacher takes alone before every window')
    p.add_argument('--hidden-channels', type=int, default=8)
    p.add_argument('--lr', type=float, default=1e-2)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--time', action='store_true', help='print optimiser steps and world-steps per second')
    args = p.parse_args(argv)
    if args.unroll < 1 or args.steps < 1 or args.detach_every < 0:
        raise SystemExit('--unroll and --steps are at least 1, --detach-every at least 0')
    args.students, _ = check_arguments(args.replicas, args.students, args.signal_channels, args.memory_channels)
    return args


def main(argv=None):
    a = parse(argv)
    _, losses = train(a.size, a.signal_channels, a.memory_channels, a.unroll, a.detach_every, a.steps, a.lr, a.seed, a.hidden_channels, a.warm,
                      a.replicas, a.students, timed=a.time)
    print(f'final mean loss per student, {a.signal_channels} signal and {a.memory_channels} memory channels on {a.replicas} worlds: '
          f'{losses[-1]:.6f}')


if __name__ == '__main__':
    main()
