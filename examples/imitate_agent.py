"""Fit a NeuralAutomataAgent to a hand-written agent by imitation, on the device: the gradient-based counterpart of
examples/learning_agents.py, and a way to give its searchers a warm start (`learning_agents.py --init-from FILE`).

    python examples/imitate_agent.py [--size 96] [--steps 300] [--lr 0.01] [--dynamics st-perlin-wide] [--seed 0]
                                     [--out saved_models/imitated_agent.pt]

The teacher is a GradientAgent without noise and without momentum; it steps the world.  Every step the student — the searchers'
architecture, kernel_sizes=[3, 3] — looks at the same observation through `differentiable_action` (one forward launch per layer
and the read-out), the loss is the mean squared error of its (dx, dy) against the teacher's over the alive slots, in units of
scale², and `loss.backward()` runs the adjoint kernels (die_conv2d_backward per layer, die_gather_scale_backward): one forward
plus one backward per world step, nothing of the field leaves the device.  Adam updates the 162 weights; the loss is printed
every 10 steps and the agent is saved with `save()`.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from die_amd import Env, GradientAgent, NeuralAutomataAgent          # noqa: E402
from population_eval import AGENT_KW, DYNAMICS, make_dynamics        # noqa: E402


def imitate(size, steps, lr, dynamics, seed, log=print):
    torch.manual_seed(seed)
    env = Env((size, size), make_dynamics(dynamics, size), seed=seed)
    scale = AGENT_KW['scale']
    teacher = GradientAgent(max_agents=env.agents.capacity, scale=scale, deposit=AGENT_KW['deposit'], inertia=0., noise_scale=0., seed=seed)
    teacher.lazy = False                                          # its action is the target: computed now, not inside the step
    student = NeuralAutomataAgent(**AGENT_KW)
    student.model.init_weights()
    opt = torch.optim.Adam(student.model.parameters(), lr=lr)
    obs = env._get_current_obs
    for t in range(steps):
        agents = obs[0]
        action = teacher.forward(obs)
        target = action.data[:2, :agents.N]
        alive = agents.alive[:agents.N] > 0
        got = student.differentiable_action(obs)
        loss = (((got[:2] - target) / scale)[:, alive] ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        if t % 10 == 0 or t == steps - 1:
            log(f'step {t:5d}: loss {float(loss.detach()):.6f}')
        obs = env.step(action)[0]
    return student


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--size', type=int, default=96)
    p.add_argument('--steps', type=int, default=300)
    p.add_argument('--lr', type=float, default=0.01)
    p.add_argument('--dynamics', choices=DYNAMICS, default='st-perlin-wide')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--out', default=os.path.join('saved_models', 'imitated_agent.pt'))
    args = p.parse_args()
    student = imitate(args.size, args.steps, args.lr, args.dynamics, args.seed)
    os.makedirs(os.path.dirname(args.out) or '.', exist_ok=True)
    student.save(args.out)
    print(f'Saving the agent to: {args.out}')


if __name__ == '__main__':
    main()
