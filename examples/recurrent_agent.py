"""Backpropagation through time for a NeuralAutomataAgent with memory channels: a recurrent student fitted to a teacher that a
memoryless policy cannot express.

The teacher is a `GradientAgent` with `inertia > 0` and no noise: its heading is a blend of the chem gradient it senses now and
the heading it had a step ago, so its action is a function of the observation AND of its own past.  The teacher drives the world.
Every optimiser step is one episode: the world is reset to its seed, a fresh teacher takes `--warm` steps alone (trails to follow),
then comes a window of `--unroll T` env steps in which the student — `NeuralAutomataAgent(memory_channels=M)`, a wide stack, its
memory blank at the window's start — computes `recurrent_action(obs, memory)` on each of the T observations, handing `memory_next`
of one step to the next, so that `loss.backward()` runs through the read-out into the memory (die_gather_memory_backward), the
stack (die_conv2d_wide_backward) and the expand onto the field (die_memory_planes_backward) of every step of the window;
`--detach-every K` cuts the memory's gradient every K steps inside a window (K = 1: no gradient through memory at all).  The loss
is the mean squared error of (dx, dy) against the teacher's over the alive agents and the window's steps, in units of scale².

`--signal-channels K` gives the student a signal field of K planes as well (`NeuralAutomataAgent(signal_channels=K)`, with or
without memory): every step is then `signalling_action(obs, signals, memory)`, the field blank at the window's start and
`signals_next` handed from step to step, so that `loss.backward()` also runs through the field's update of every step
(die_signal_step_backward: what an agent wrote is read, diffused and decayed, by whoever comes by later in the window);
`--detach-every` cuts the field's gradient with the memory's.  Stand-alone only: with `--replicas` it is refused — populations with
signal channels are trained by examples/signalling_population.py.

`--memory-channels 0` trains the same stack without memory through `model.forward_device` and `functional.gather_scale`: the
baseline.  With M > 0 the baseline is trained as well, on a world seeded alike, and both final losses are printed — side by side,
with no claim about which is smaller.  `--time` prints optimiser steps per second.

`--replicas R [--students C]` runs the window loop on a `BatchedEnv` of R worlds instead: the teacher is a `BatchedPhysarumAgent`
— its heading is state, so a memoryless student cannot express it either — which hands out its targets through
`step(..., action=target)`, and C students (E = R / C worlds each; default C = R) are trained in ONE optimiser step through
`BatchedNeuralAutomataAgent.recurrent_action`: one launch per kernel for all R worlds, a (C, P) gradient.  The stand-alone path
above is untouched by it.

    python examples/recurrent_agent.py --size 96 --memory-channels 2 --unroll 8 --steps 200
    python examples/recurrent_agent.py --size 96 --memory-channels 2 --unroll 8 --steps 200 --replicas 16 --students 16
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from die_amd import Dynamics, Env, GradientAgent, NeuralAutomataAgent, functional          # noqa: E402
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent, BatchedPhysarumAgent   # noqa: E402

SCALE, DEPOSIT = 0.01, 2.0


def make_student(memory_channels, hidden_channels=8, seed=0, signal_channels=0):
    torch.manual_seed(seed)
    student = NeuralAutomataAgent(kernel_sizes=[3, 3], scale=SCALE, deposit=DEPOSIT, hidden_channels=hidden_channels, hidden_activation='tanh',
                                  memory_channels=memory_channels, signal_channels=signal_channels)
    student.model.init_weights()
    return student


def student_step(student, obs, state):
    """One step of the student on `obs`: ((3, N) action with a `grad_fn`, the state to hand on).  `state` = (signals, memory): the
    field and the memory of the step before, each None at a window's start and where the student has no such channels."""
    signals, memory = state
    if student.signal_channels:
        action, signals, memory = student.signalling_action(obs, signals, memory)
        return action, (signals, memory)
    if student.memory_channels:
        action, memory = student.recurrent_action(obs, memory)
        return action, (None, memory)
    medium = obs[1]
    medium.sensed()
    planes = torch.stack([medium.sel(c).float() for c in student.obs_channels])
    return functional.gather_scale(student.model.forward_device(planes), obs, student.action_coefs), (None, None)


def window_loss(student, teacher, env, obs, state, unroll, detach_every):
    """`unroll` env steps driven by the teacher, the student unrolled beside it: (loss, the observation after the window, the
    state — (signals, memory) — after the window)."""
    loss = 0.
    for t in range(unroll):
        if detach_every and t % detach_every == 0:
            state = tuple(None if v is None else v.detach() for v in state)
        agents = obs[0]
        action = teacher.forward(obs)
        target = action.data[:2, :agents.N]
        alive = agents.alive[:agents.N] > 0
        got, state = student_step(student, obs, state)
        loss = loss + (((got[:2] - target) / SCALE)[:, alive] ** 2).mean()
        obs = env.step(action)[0]
    return loss / unroll, obs, state


def train(size, memory_channels, unroll, detach_every, steps, lr=1e-2, seed=0, inertia=0.9, hidden_channels=8, warm=4, log=print, timed=False,
          signal_channels=0):
    """`steps` Adam steps, each on one episode: the world reset to its seed, a fresh teacher, `warm` steps of the teacher alone (so that
    there are trails to follow), then the window of `unroll` steps with the student beside it, its memory (and its signal field, with
    `signal_channels` > 0) blank at the window's start.
    Returns (the student, the list of episode losses)."""
    env = Env((size, size), Dynamics(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8), seed=seed)
    student = make_student(memory_channels, hidden_channels, seed, signal_channels)
    opt = torch.optim.Adam(student.model.parameters(), lr=lr)
    tag = f'M={memory_channels}' + (f' K={signal_channels}' if signal_channels else '')
    losses, t0 = [], None
    warmup = max(1, steps // 10)
    for it in range(steps):
        if timed and it == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        obs = env.reset(seed=seed)[0]
        teacher = GradientAgent(max_agents=env.agents.capacity, scale=SCALE, deposit=DEPOSIT, inertia=inertia, noise_scale=0., seed=seed)
        teacher.lazy = False                                      # its action is the target: computed now, not inside the step
        for _ in range(warm):
            obs = env.step(teacher.forward(obs))[0]
        student.reset_memory()
        student.reset_signals()
        loss, obs, _ = window_loss(student, teacher, env, obs, (None, None), unroll, detach_every)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if it % 10 == 0 or it == steps - 1:
            log(f'{tag} step {it:5d}: loss {losses[-1]:.6f}')
    if t0 is not None and steps > warmup:
        torch.cuda.synchronize()
        log(f'{tag}, T={unroll}: {(steps - warmup) / (time.perf_counter() - t0):.2f} optimiser steps/s over {steps - warmup} steps')
    return student, losses


def train_batched(size, memory_channels, unroll, detach_every, steps, lr=1e-2, seed=0, hidden_channels=8, warm=4, replicas=4, students=None,
                  log=print, timed=False):
    """`train` on R = `replicas` worlds at once: `students` candidates (default R) of E = R / students worlds each, one Adam step per
    episode for all of them.  Every episode: the worlds reset, a fresh BatchedPhysarumAgent takes `warm` steps alone, then the window
    of `unroll` steps — the students look at the worlds through `recurrent_action`, handing `memory_next` on, the teacher steps them
    and leaves its actions in `target`.  The loss is the sum over the students of their mean squared error, so that every student's
    row of the (C, P) gradient is its own.  Returns (the BatchedNeuralAutomataAgent, the list of episode losses)."""
    students = replicas if students is None else students
    if memory_channels < 1:
        raise SystemExit('--replicas trains students with memory: --memory-channels at least 1')
    if students < 1 or replicas % students:
        raise SystemExit(f'--students {students} must divide --replicas {replicas}')
    env = BatchedEnv((size, size), Dynamics(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8), replicas=replicas, seed=seed)
    template = make_student(memory_channels, hidden_channels, seed)
    rows = []
    for _ in range(students):                                     # different initialisations side by side
        template.model.init_weights()
        rows.append(torch.nn.utils.parameters_to_vector(template.model.parameters()).detach().clone())
    pop = BatchedNeuralAutomataAgent(env, template, torch.stack(rows), replicas // students)
    pop.parameters.requires_grad_()
    opt = torch.optim.Adam([pop.parameters], lr=lr)
    target = torch.zeros((3, env.R, env.Nmax), device=env.device)
    exists = torch.zeros((env.R, env.Nmax), dtype=torch.bool, device=env.device)
    for r in range(env.R):
        exists[r, :env.n[r]] = True
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
        pop.reset_memory()
        memory, loss = None, 0.
        for t in range(unroll):
            if memory is not None and detach_every and t % detach_every == 0:
                memory = memory.detach()
            got, memory = pop.recurrent_action(memory)            # the students look at the worlds the teacher is about to act on
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
            log(f'M={memory_channels} R={replicas} C={students} step {it:5d}: mean loss per student {losses[-1]:.6f}')
    if t0 is not None and steps > warmup:
        torch.cuda.synchronize()
        rate = (steps - warmup) / (time.perf_counter() - t0)
        log(f'M={memory_channels}, T={unroll}, R={replicas}, C={students}: {rate:.2f} optimiser steps/s over {steps - warmup} steps '
            f'({rate * replicas * unroll:.0f} world-steps/s)')
    return pop, losses


def main():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--size', type=int, default=96)
    p.add_argument('--memory-channels', type=int, default=2, metavar='M', help='values every agent carries between steps, 1..8; 0: the '
                                                                                'memoryless baseline alone')
    p.add_argument('--signal-channels', type=int, default=0, metavar='K', help='planes of the signal field the agents write and read, 1..8 '
                                                                               '(0: none); stand-alone only')
    p.add_argument('--unroll', type=int, default=8, metavar='T', help='env steps per optimiser step')
    p.add_argument('--detach-every', type=int, default=0, metavar='K', help="cut the memory's gradient every K steps of a window (0: never)")
    p.add_argument('--steps', type=int, default=200, help='optimiser steps')
    p.add_argument('--warm', type=int, default=4, help="steps the teacher takes alone before every window")
    p.add_argument('--hidden-channels', type=int, default=8)
    p.add_argument('--inertia', type=float, default=0.9, help="the teacher's")
    p.add_argument('--lr', type=float, default=1e-2)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--time', action='store_true', help='print optimiser steps per second')
    p.add_argument('--replicas', type=int, default=0, metavar='R', help='train on R batched worlds (0: the stand-alone path)')
    p.add_argument('--students', type=int, default=None, metavar='C', help='with --replicas: C students of R / C worlds each (default R)')
    args = p.parse_args()
    if args.unroll < 1 or args.steps < 1 or args.detach_every < 0:
        raise SystemExit('--unroll and --steps are at least 1, --detach-every at least 0')
    if args.replicas and args.signal_channels:
        raise SystemExit('--signal-channels trains a stand-alone student here; populations with signal channels: examples/signalling_population.py')
    if args.replicas:
        _, losses = train_batched(args.size, args.memory_channels, args.unroll, args.detach_every, args.steps, args.lr, args.seed,
                                  args.hidden_channels, args.warm, args.replicas, args.students, timed=args.time)
        print(f'final mean loss per student, {args.memory_channels} memory channels on {args.replicas} worlds: {losses[-1]:.6f}')
        return
    final = {}
    for M, K in dict.fromkeys(((args.memory_channels, args.signal_channels), (args.memory_channels, 0), (0, 0))):
        _, losses = train(args.size, M, args.unroll, args.detach_every, args.steps, args.lr, args.seed, args.inertia, args.hidden_channels,
                          args.warm, timed=args.time, signal_channels=K)
        final[M, K] = losses[-1]
    for (M, K), loss in final.items():
        name = ' and '.join(([f'{M} memory channels'] if M else []) + ([f'{K} signal channels'] if K else [])) or 'memoryless baseline'
        print(f'final loss, {name}: {loss:.6f}')


if __name__ == '__main__':
    main()
