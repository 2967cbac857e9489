"""Physarum parameter maps and searches on batched replicas (die_amd.batch.BatchedPhysarumPopulation): up to 64 PhysarumAgent
parameter sets stepped together on copies of one seeded world, one launch pair per step for all of them.

    python examples/physarum_search.py --sweep sense_angle=22.5:112.5:8 sense_offset=0.01:0.08:8 [--agents-die]
    python examples/physarum_search.py --searcher pgpe|cmaes [--generations 40] [--out best.json]
    ... [--size 96] [--iters 30] [--replicas 10] [--episodes 1] [--seed 0] [--time]

--sweep NAME=LO:HI:N ... lays a grid over the named constructor arguments (the others at PhysarumAgent's defaults; at most 64
cells) and prints, per cell, the mean reward per step and the agents alive at the end (they only fall with --agents-die).
--searcher tunes the six parameters from the default ParameterSpace with the device-resident PGPE or separable CMA-ES (no host
read inside a generation) and saves the best candidate's constructor arguments as JSON.
--episodes E (search mode): every one of the --replicas candidates is scored on E worlds (seeds seed … seed + E − 1, the same E
for every candidate) in the same launches, its fitness their mean; replicas·E may not exceed 64.
--time: sweep mode prints candidate-steps/s of the batch against the same candidates stepped one at a time (a stand-alone Env +
PhysarumAgent each); search mode prints generations/s.
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from die_amd import CMAES, PGPE, Dynamics, Env                                         # noqa: E402
from die_amd.batch import PARAMETER_NAMES, PHYSARUM_DEFAULTS, BatchedEnv, BatchedPhysarumPopulation, episode_seeds   # noqa: E402


def sweep_rows(specs):
    """(rows (n, 6) float32, axes [(name, values)]) of a grid over the named parameters."""
    axes = []
    for spec in specs:
        name, rng = spec.split('=')
        lo, hi, n = rng.split(':')
        if name not in PARAMETER_NAMES:
            raise SystemExit(f'--sweep {name}: one of {PARAMETER_NAMES}')
        axes.append((name, np.linspace(float(lo), float(hi), int(n))))
    cells = list(itertools.product(*[v for _, v in axes]))
    if not 1 <= len(cells) <= 64:
        raise SystemExit(f'--sweep: {len(cells)} cells, at most 64 replicas')
    rows = np.tile(np.float32(PHYSARUM_DEFAULTS), (len(cells), 1))
    for i, cell in enumerate(cells):
        for (name, _), v in zip(axes, cell):
            rows[i, PARAMETER_NAMES.index(name)] = v
    return rows, axes


def one_at_a_time(pop, size, dynamics, seed, iters):
    """The same candidates through the stand-alone API: (rewards (iters, R), seconds)."""
    envs = [Env((size, size), dynamics(), seed=seed, max_agents='alive') for _ in range(pop.R)]
    agents = [pop.candidate(r) for r in range(pop.R)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rewards = np.zeros((iters, pop.R))
    for r, (env, ag) in enumerate(zip(envs, agents)):
        obs = env._get_current_obs
        for i in range(iters):
            obs, rewards[i, r], _, _, _ = env.step(ag.forward(obs))
    torch.cuda.synchronize()
    return rewards, time.perf_counter() - t0


def run_sweep(args, dynamics):
    rows, axes = sweep_rows(args.sweep)
    R = rows.shape[0]
    benv = BatchedEnv((args.size, args.size), dynamics(), replicas=R, seeds=[args.seed] * R)
    pop = BatchedPhysarumPopulation(benv, rows, seed=args.seed)
    benv.run(pop, 2)                                    # (first launches)
    benv.reset()
    pop.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = benv.run(pop, args.iters)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rewards, alive = BatchedEnv.read_results(res)
    print(' '.join(f'{name:>14}' for name, _ in axes) + f' {"reward/step":>14} {"alive":>8}')
    for r in range(R):
        print(' '.join(f'{rows[r, PARAMETER_NAMES.index(name)]:14.5g}' for name, _ in axes) + f' {rewards[:, r].mean():14.6f} {alive[-1, r]:8d}')
    if args.time:
        want, dt1 = one_at_a_time(pop, args.size, dynamics, args.seed, args.iters)
        assert np.array_equal(want, rewards), 'the batch and the stand-alone runs disagree'
        n = R * args.iters
        print(f'batched: {n / dt:.0f} candidate-steps/s; one at a time: {n / dt1:.0f} candidate-steps/s ({dt1 / dt:.1f}x)')


def run_search(args, dynamics):
    R, E = args.replicas, args.episodes               # R candidates on R·E replicas
    benv = BatchedEnv((args.size, args.size), dynamics(), replicas=R * E, seeds=episode_seeds(args.seed, R, E))
    pop = BatchedPhysarumPopulation(benv, parameters=torch.full((R, 6), 0.5), seed=args.seed, episodes=E)
    center = torch.tensor(pop.space.encode(PHYSARUM_DEFAULTS))          # start at the reference's defaults
    if args.searcher == 'pgpe':
        s = PGPE(R, center_init=center, stdev_init=0.1, center_learning_rate=0.05, stdev_learning_rate=0.1,
                 optimizer_config=dict(max_speed=0.1, momentum=0.9), seed=args.seed, device=benv.device)
    else:
        s = CMAES(R, center_init=center, stdev_init=0.15, seed=args.seed, device=benv.device)
    s.for_population(pop, args.iters)
    s.run(1)                                            # (first launches)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.run(args.generations)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    h = s.history()
    for g in range(0, s.iter, max(1, s.iter // 10)):
        print(f'generation {g:4d}: mean {h[g, 0]:10.5f}  max {h[g, 1]:10.5f}  median {h[g, 3]:10.5f}')
    best = s.best_agent()
    keep = PARAMETER_NAMES + ('normalized_grad', 'grad_clip')
    out = {k: v for k, v in best.init_params.items() if k in keep}
    print(f'best fitness {s.status["best_eval"]:.5f}: {out}')
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    if args.time:
        print(f'{args.generations / dt:.1f} generations/s ({R} candidates x {E} episodes x {args.iters} steps, {args.size}x{args.size})')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--sweep', nargs='+', metavar='NAME=LO:HI:N')
    ap.add_argument('--searcher', choices=('pgpe', 'cmaes'))
    ap.add_argument('--size', type=int, default=96)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--replicas', type=int, default=10)
    ap.add_argument('--episodes', type=int, default=1, help='search mode: worlds per candidate and generation (replicas x episodes <= 64)')
    ap.add_argument('--generations', type=int, default=40)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--agents-die', action='store_true')
    ap.add_argument('--time', action='store_true')
    ap.add_argument('--out', default='physarum_best.json')
    args = ap.parse_args()
    if (args.sweep is None) == (args.searcher is None):
        ap.error('one of --sweep and --searcher')
    if args.episodes < 1 or args.replicas * args.episodes > 64 or (args.sweep and args.episodes != 1):
        ap.error(f'--episodes {args.episodes}: at least 1, {args.replicas} replicas x episodes at most 64, and search mode only')
    dynamics = lambda: Dynamics(agents_die=args.agents_die)
    if args.sweep:
        run_sweep(args, dynamics)
    else:
        run_search(args, dynamics)


if __name__ == '__main__':
    main()
