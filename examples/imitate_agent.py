"""Fit a NeuralAutomataAgent to a hand-written agent by imitation, on the device: the gradient-based counterpart of
examples/learning_agents.py, and a way to give its searchers a warm start (`learning_agents.py --init-from FILE`).

    python examples/imitate_agent.py [--size 96] [--steps 300] [--lr 0.01] [--dynamics st-perlin-wide] [--seed 0]
                                     [--out saved_models/imitated_agent.pt] [--replicas R [--students C]] [--time]
                                     [--hidden-channels C] [--hidden-activation {tanh,relu,none}]

The teacher is a GradientAgent without noise and without momentum; it steps the world.  Every step the student — the searchers'
architecture, kernel_sizes=[3, 3] — looks at the same observation through `differentiable_action` (one forward launch per layer
and the read-out), the loss is the mean squared error of its (dx, dy) against the teacher's over the alive slots, in units of
scale², and `loss.backward()` runs the adjoint kernels (die_conv2d_backward per layer, die_gather_scale_backward): one forward
plus one backward per world step, nothing of the field leaves the device.  Adam updates the 162 weights; the loss is printed
every 10 steps and the agent is saved with `save()`.

`--hidden-channels C --hidden-activation A` make the student a wide stack, 3 -> C -> 3 with A after the first layer.  It is fitted
through `model.forward_device(planes)` on the observation's float32 planes — one `die_amd.functional.conv2d_wide` per layer, whose
backward is die_conv2d_wide_backward (the MFMA adjoint kernels) — and `functional.gather_scale`, the same read-out; the student's
own `differentiable_action` refuses a wide stack.  With `--replicas` the wide students go through
`BatchedNeuralAutomataAgent.forward_device` (die_nca_wide_backward_batch: the same kernels with the replica in blockIdx.z, L
launches forward and 3 L - 1 backward whatever R is) and `functional.gather_scale_batch`.

`--replicas R` (with `--students C`, R = C·E; default C = R) is the batched form: R worlds in one BatchedEnv seeded seed … seed + R − 1,
the teacher a BatchedPhysarumAgent that steps them and hands its actions out through `step(..., action=target)`, the students one
BatchedNeuralAutomataAgent whose (C, P) matrix is the Adam leaf — student c learns from its E worlds at once (C = 1: minibatch
imitation of one model over R worlds).  Every optimiser step is L + 1 launches forward and 1 + 2 L backward whatever R is
(`BatchedNeuralAutomataAgent.differentiable_action`).  `--out` then saves student 0.  `--time` prints optimiser steps per second
(forward + backward + Adam + the teacher's step, after a warm-up tenth of the run, ending in a device synchronise).
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from die_amd import Env, GradientAgent, NeuralAutomataAgent, functional          # noqa: E402
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent, BatchedPhysarumAgent    # noqa: E402
from population_eval import AGENT_KW, DYNAMICS, add_wide_arguments, make_dynamics, wide_keywords        # noqa: E402


def student_action(student, obs):
    """(3, N) with a `grad_fn`: a narrow student's own differentiable_action; a wide one through the model's forward_device on the
    observation's planes and the read-out."""
    if not student.model.wide:
        return student.differentiable_action(obs)
    medium = obs[1]
    medium.sensed()
    planes = torch.stack([medium.sel(c).float() for c in student.obs_channels])
    return functional.gather_scale(student.model.forward_device(planes), obs, student.action_coefs)


def imitate(size, steps, lr, dynamics, seed, log=print, clock=None, wide_kw=None):
    torch.manual_seed(seed)
    env = Env((size, size), make_dynamics(dynamics, size), seed=seed)
    scale = AGENT_KW['scale']
    teacher = GradientAgent(max_agents=env.agents.capacity, scale=scale, deposit=AGENT_KW['deposit'], inertia=0., noise_scale=0., seed=seed)
    teacher.lazy = False                                          # its action is the target: computed now, not inside the step
    student = NeuralAutomataAgent(**AGENT_KW, **(wide_kw or {}))
    student.model.init_weights()
    opt = torch.optim.Adam(student.model.parameters(), lr=lr)
    obs = env._get_current_obs
    for t in range(steps):
        if clock is not None:
            clock.tick(t)
        agents = obs[0]
        action = teacher.forward(obs)
        target = action.data[:2, :agents.N]
        alive = agents.alive[:agents.N] > 0
        got = student_action(student, obs)
        loss = (((got[:2] - target) / scale)[:, alive] ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        if t % 10 == 0 or t == steps - 1:
            log(f'step {t:5d}: loss {float(loss.detach()):.6f}')
        obs = env.step(action)[0]
    if clock is not None:
        clock.report(print, 'imitation, one world')
    return student


class _Clock:
    """Optimiser steps per second over the steps after `warmup`, each end of the window a device synchronise."""

    def __init__(self, steps, enabled):
        self.warmup, self.steps, self.enabled, self.t0 = max(1, steps // 10), steps, enabled and steps >= 2, None

    def tick(self, t):
        if self.enabled and t == self.warmup:
            torch.cuda.synchronize()
            self.t0 = time.perf_counter()

    def report(self, log, what):
        if self.enabled and self.t0 is not None:
            torch.cuda.synchronize()
            n = self.steps - self.warmup
            log(f'{what}: {n / (time.perf_counter() - self.t0):.1f} optimiser steps/s over {n} steps')


def imitate_batched(size, steps, lr, dynamics, seed, replicas, students, log=print, clock=None, wide_kw=None):
    """R worlds, C students, E = R / C worlds per student; returns the BatchedNeuralAutomataAgent.  `wide_kw`: the students are
    wide stacks, fitted through `forward_device` and `functional.gather_scale_batch`."""
    if replicas % students:
        raise SystemExit(f'--students {students} must divide --replicas {replicas}')
    torch.manual_seed(seed)
    env = BatchedEnv((size, size), make_dynamics(dynamics, size), replicas=replicas, seed=seed)
    scale = AGENT_KW['scale']
    teacher = BatchedPhysarumAgent(env, scale=scale, deposit=AGENT_KW['deposit'], seed=seed)
    template = NeuralAutomataAgent(**AGENT_KW, **(wide_kw or {}))
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
    for t in range(steps):
        if clock is not None:
            clock.tick(t)
        # the students look at the worlds the teacher is about to act on
        got = functional.gather_scale_batch(pop.forward_device(), pop) if template.model.wide else pop.differentiable_action()
        live = exists & (env.alive > 0)
        env.step(teacher, action=target)                          # its actions on those worlds: the targets
        loss = (((got[:2] - target[:2]) / scale)[:, live] ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        if t % 10 == 0 or t == steps - 1:
            log(f'step {t:5d}: loss {float(loss.detach()):.6f}')
    return pop


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--size', type=int, default=96)
    p.add_argument('--steps', type=int, default=300)
    p.add_argument('--lr', type=float, default=0.01)
    p.add_argument('--dynamics', choices=DYNAMICS, default='st-perlin-wide')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--out', default=os.path.join('saved_models', 'imitated_agent.pt'))
    p.add_argument('--replicas', type=int, default=0, help='R worlds in one BatchedEnv (0: the single-world form)')
    p.add_argument('--students', type=int, default=0, help='C students, R = C x E (default: one per replica)')
    p.add_argument('--time', action='store_true', help='print optimiser steps per second')
    add_wide_arguments(p)
    args = p.parse_args()
    if args.replicas:
        clock = _Clock(args.steps, args.time)
        quiet = (lambda *a: None) if args.time else print         # (a loss print reads the device: not inside a timed window)
        pop = imitate_batched(args.size, args.steps, args.lr, args.dynamics, args.seed, args.replicas, args.students or args.replicas,
                              log=quiet, clock=clock, wide_kw=wide_keywords(args))
        clock.report(print, f'batched imitation, {args.replicas} worlds, {args.students or args.replicas} students')
        student = pop.candidate(0)
    else:
        if args.students:
            raise SystemExit('--students needs --replicas')
        student = imitate(args.size, args.steps, args.lr, args.dynamics, args.seed, log=(lambda *a: None) if args.time else print,
                          clock=_Clock(args.steps, args.time), wide_kw=wide_keywords(args))
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    student.save(args.out)
    print(f'Saving the agent to: {args.out}')


if __name__ == '__main__':
    main()
