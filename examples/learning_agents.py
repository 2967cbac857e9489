"""The reference's examples/learning_agents.py (`run_experiment` / `run_agent`) on this library: a population of
NeuralAutomataAgent candidates trained by PGPE (popsize 10, radius_init 1.5, ClipUp with max_speed 0.1 and momentum 0.9,
center_learning_rate 0.05, stdev_learning_rate 0.1, the centre drawn in initial_bounds (-0.5, 0.5)), every generation one
chain of launches on the GPU: sample into the population's parameter matrix, reset the batched worlds, `epoch_iters` batched
steps, update (die_amd.search.PGPE).  `--searcher cmaes` trains with the reference's other, commented-out searcher instead:
separable CMA-ES with stdev_init 0.1 and popsize 10 (die_amd.search.CMAES), the same chain of launches.

    python examples/learning_agents.py [--searcher pgpe|cmaes] [--dynamics st-perlin-wide] [--size 96] [--generations 100]
                                       [--epoch-iters 30] [--agents-die] [--agents-born] [--max-agents alive|full|tight|N]
                                       [--reseed S] [--reseed-stride 0] [--episodes 1] [--out saved_models/agent.pt] [--time]
                                       [--dropout P] [--dropout-seed S] [--dropout-stride K] [--init-from FILE]
                                       [--stock-channel] [--memory-channels M [--memory-inherit blank|copy [--memory-mutation A]]]
                                       [--signal-channels K [--signal-sigma S --signal-decay D --signal-deposit G]]

--init-from FILE starts the search from a saved agent (e.g. the one examples/imitate_agent.py fits by gradient descent): its
`parameters_to_vector` becomes the searcher's `center_init` instead of a centre drawn in initial_bounds.  A file whose agent
observes another number of channels than this run's (saved without --stock-channel, searched with it, or the other way round)
is refused with a message naming both counts.

--stock-channel trains agents that sense their own food stock (NeuralAutomataAgent(with_stock_channel=True)): a fourth observation
channel holding, on every cell, the `agent_food` of the agent standing there, built on the device by one more launch per batched
step.  With --agents-die / --agents-born that is the quantity that decides whether an agent dies or breeds.

--memory-channels M (1..8) trains recurrent agents (NeuralAutomataAgent(memory_channels=M)): every agent carries M values from one
step to the next, read by the stack as M more observation planes and written as M more output planes.  The stack is then a wide
stack (--hidden-channels defaults to the observation's width), every generation starts from blank memory, and --agents-born
needs --memory-inherit {blank,copy} [--memory-mutation A] beside it: what a newborn's memory holds — blank, its parent's, or its
parent's plus uniform noise of half-width A (NeuralAutomataAgent(memory_inherit=..., memory_mutation=A)).  Without
a rule the combination stays refused (a newborn would inherit a dead agent's memory).

--signal-channels K (1..8) trains agents that signal (NeuralAutomataAgent(signal_channels=K)): a field of K planes the stack reads as
K more observation channels and writes through K more output planes at the cells the agents stand on; it diffuses (--signal-sigma),
decays (--signal-decay) and is read by whoever comes by; --signal-deposit scales the emission.  A wide stack, two more launches per
batched step, every generation from a blank field; signalling is free of action cost.  With --agents-born it is fine as long as
--memory-channels is 0.  K = 0, 1, 2, 4 varies the medium's capacity for message passing under one searcher.

--dropout P trains the agent with the reference's `p_agent_dropout=P` (its learning_agents.py carries 0.25): in every batched step
replica r's sense planes are multiplied by the counter-based dropout mask of key --dropout-seed + r·--dropout-stride (default
stride 1: every replica its own mask; 0: one mask for all, common random numbers across candidates), evaluated inside the last conv
launch.  The mask counter runs on from generation to generation, so every generation sees new masks, and a run is reproducible.

--dynamics takes one of the reference's three worlds or a comma list of them (e.g. st-perlin,st-perlin-wide,dyn-pred): every candidate
is then scored under EVERY listed dynamics each generation, in the same launches (BatchedEnv(dynamics=[...]): per-replica Dynamics;
episode e lives under dynamics e mod len).  The list implies --episodes len(list) unless --episodes is given (then a multiple of it);
the fitness is the mean over the episodes, and the mean of `episode_fitness` under each dynamics is printed with the history.

--agents-die trains under the death pressure (Dynamics(agents_die=True)); --agents-born adds births (Dynamics(agents_born=True):
after a step's deaths the agents with more than 0.5 food breed into dead slots, three more launches per batched step), so that a
candidate is rewarded for thriving and not only for not starving.

--reseed S gives every generation a new world: generation g resets the batch to the world of seed S + g·popsize, seeded on the
device (BatchedEnv.reset(seed=...), five launches, no host read); with --reseed-stride 0 (default) every candidate of a
generation shares that world, with 1 each gets its own.  It needs a fixed slot layout (--max-agents; 'tight' when not given).

--episodes E scores every candidate on E worlds per generation, its fitness their mean (evotorch's num_episodes): popsize·E
batched replicas (at most 64) stepped by the same launches, one more launch per generation for the fold.  Without --reseed the E
worlds are those of seeds seed … seed + E − 1 every generation; with it generation g takes the worlds of S + g·popsize·E + e
(+ --reseed-stride·c·E for candidate c), seeded on the device from the list (BatchedEnv.reset(seeds=...)).

Deliberate differences from the reference: without --reseed every generation starts the R worlds from the same
seeded state, and with it from a new one each generation, where the reference's run_epoch keeps stepping one env from candidate
to candidate, so that its candidates see the states their predecessors left; no MLflow; and the noise is Philox's, so runs are
reproducible here and not bit-equal to evotorch's.  --time runs G generations of this loop — on the 'alive' layout, on the
fixed layout, and on the fixed layout reseeding every generation — against the same population driven from the host (a fresh
BatchedEnv per generation, host noise, fitness read back, plain Gaussian ES on the host: what examples/population_eval.py
--generations does) and prints generations/s for each.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from die_amd import CMAES, PGPE, Env, NeuralAutomataAgent            # noqa: E402
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent, episode_seeds   # noqa: E402
from population_eval import (DYNAMICS, add_wide_arguments, batch_dynamics, dropout_keywords, dynamics_names, evaluate_population, lifecycle, make_dynamics,   # noqa: E402
                             make_population, make_template, per_dynamics_means, resolve_episodes, run_epoch, slots, wide_keywords)

RADIUS_INIT = 1.5
MAX_SPEED = RADIUS_INIT / 15.              # the reference's rule of thumb
SEARCH_KW = dict(radius_init=RADIUS_INIT, center_learning_rate=MAX_SPEED / 2., stdev_learning_rate=0.1, optimizer='clipup',
                 optimizer_config=dict(max_speed=MAX_SPEED, momentum=0.9))
CMAES_KW = dict(stdev_init=0.1, separable=True)        # the reference's commented-out CMAES(problem, stdev_init=0.1, popsize=10, ...)
SEARCHERS = ('pgpe', 'cmaes')


def make_search(size, choice, popsize, epoch_iters, seed, searcher='pgpe', agents_die=False, max_agents='alive', reseed=None,
                reseed_stride=0, episodes=1, drop_kw=None, dropout=0., center_init=None, wide_kw=None):
    torch.manual_seed(seed)
    template = make_template(dropout, wide_kw)
    benv = BatchedEnv((size, size), batch_dynamics(choice, size, agents_die, popsize, episodes), replicas=popsize * episodes,
                      seeds=episode_seeds(seed, popsize, episodes), max_agents=max_agents)
    pop = BatchedNeuralAutomataAgent(benv, template, episodes=episodes, **(drop_kw or {}))
    if searcher == 'cmaes':
        search = CMAES(popsize, pop.P, seed=seed, center_init=center_init, **CMAES_KW)
    else:
        search = PGPE(popsize, pop.P, seed=seed, center_init=center_init, **SEARCH_KW)
    return search.for_population(pop, epoch_iters, reseed=reseed, reseed_stride=reseed_stride), pop


def init_from_mismatch(loaded, template, file):
    """The message that refuses an --init-from agent observing another number of channels than this run's template; None if they agree."""
    have, want = loaded.obs_channels, template.obs_channels
    if len(have) == len(want):
        return None
    return (f'--init-from {file}: the saved agent observes {len(have)} channels ({", ".join(have)}), this run\'s agents observe '
            f'{len(want)} ({", ".join(want)}): its weights do not fit' +
            (' (run with --stock-channel)' if 'agent_food' in have else ' (run without --stock-channel)' if 'agent_food' in want else ''))


def host_generation(size, choice, template, mean, sigma, lr, iters, seed, agents_die=False, drop_kw=None):
    """One generation driven from the host (population_eval.py --generations): rebuild, evaluate, read back, update."""
    R = 10
    half = torch.randn((R // 2, mean.numel()))
    noise = torch.cat([half, -half])
    fit = evaluate_population(*make_population(size, template, mean + sigma * noise, seed, choice, agents_die, drop_kw=drop_kw), iters)
    f = torch.tensor(fit, dtype=torch.float32)
    f = (f - f.mean()) / (f.std() + 1e-8)
    return mean + lr / (noise.shape[0] * sigma) * (noise.T @ f)


def time_device_loop(args, G, max_agents, reseed):
    searcher, pop = make_search(args.size, args.dynamics, 10, args.epoch_iters, args.seed, args.searcher, args.agents_die, max_agents,
                                reseed, args.reseed_stride, args.episodes, args.drop_kw, args.dropout, wide_kw=args.wide_kw)
    searcher.run(2)                                               # warm-up: first launches, allocations
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    searcher.run(G)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if reseed is not None:
        pop.env.check()                                           # no world seeded more agents than the slots hold
    return searcher, pop, dt


def time_loops(args, N):
    G = args.generations
    fixed = N if N != 'alive' else slots('tight', args.size, args.dynamics, args.agents_die)
    reseed = args.reseed if args.reseed is not None else args.seed + 1
    searcher, pop, t_dev = time_device_loop(args, G, 'alive', None)
    _, _, t_fixed = time_device_loop(args, G, fixed, None)
    _, _, t_reseed = time_device_loop(args, G, fixed, reseed)
    E = args.episodes
    if E > 1:                                                     # (the host-driven loop has no episodes: the device loops only)
        name = type(searcher).__name__ + '.run):'
        for what, t, n in ((f'device loop ({name:15s}', t_dev, 'alive'), ('  fixed slots:             ', t_fixed, fixed),
                           ('  fixed slots, reseeding:  ', t_reseed, f'{fixed}, reseed stride {args.reseed_stride}')):
            print(f'{what}{G / t:9.1f} generations/s  ({t / G * 1e3:.3f} ms per generation, {10 * E * G / t:9.1f} candidate-evaluations/s)  '
                  f'max_agents={n}')
        print(f'({G} generations of 10 candidates x {E} episodes x {args.size}^2, {args.epoch_iters} steps, {args.dynamics})', flush=True)
        return
    template = pop.template
    mean = pop.parameters[0].cpu()
    for _ in range(2):
        mean = host_generation(args.size, args.dynamics, template, mean, 0.1, 0.05, args.epoch_iters, args.seed, args.agents_die, args.drop_kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(G):
        mean = host_generation(args.size, args.dynamics, template, mean, 0.1, 0.05, args.epoch_iters, args.seed, args.agents_die, args.drop_kw)
    torch.cuda.synchronize()
    t_host = time.perf_counter() - t0
    name = type(searcher).__name__ + '.run):'
    print(f'device loop ({name:15s}{G / t_dev:9.1f} generations/s  ({t_dev / G * 1e3:.3f} ms per generation)  max_agents=alive')
    print(f'  fixed slots:             {G / t_fixed:9.1f} generations/s  ({t_fixed / G * 1e3:.3f} ms per generation)  max_agents={fixed}')
    print(f'  fixed slots, reseeding:  {G / t_reseed:9.1f} generations/s  ({t_reseed / G * 1e3:.3f} ms per generation)  '
          f'max_agents={fixed}, reseed stride {args.reseed_stride}')
    print(f'host-driven loop (rebuild): {G / t_host:9.1f} generations/s  ({t_host / G * 1e3:.3f} ms per generation)')
    print(f'speed-up: {t_host / t_dev:.2f}x  ({G} generations of 10 x {args.size}^2, {args.epoch_iters} steps, {args.dynamics})', flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--searcher', choices=SEARCHERS, default='pgpe', help='PGPE (the reference\'s) or separable CMA-ES')
    p.add_argument('--dynamics', default='st-perlin-wide', help=f'one of {", ".join(DYNAMICS)}, or a comma list: every candidate on each')
    p.add_argument('--size', type=int, default=96)
    p.add_argument('--popsize', type=int, default=10)
    p.add_argument('--generations', type=int, default=100, help='epochs of the reference: search generations')
    p.add_argument('--epoch-iters', type=int, default=30, help='steps per evaluation')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--out', default=None, help='agent file for pop_best (default: saved_models/neuralautomataagent_<searcher>_<G>x<T>.pt)')
    p.add_argument('--time', action='store_true')
    p.add_argument('--agents-die', action='store_true', help='Dynamics(agents_die=True): starved agents die, fitness feels it')
    p.add_argument('--agents-born', action='store_true', help='Dynamics(agents_born=True): well-fed agents breed into dead slots')
    p.add_argument('--max-agents', default=None, help="slots per replica: 'alive' (default without --reseed), 'full' (W·H), "
                                                      "'tight' (default with --reseed) or a number")
    p.add_argument('--reseed', type=int, default=None, help='a new world every generation: seed S + g·popsize (device-seeded)')
    p.add_argument('--reseed-stride', type=int, default=0, help='0: one world per generation; 1: one per candidate and generation')
    p.add_argument('--episodes', type=int, default=None, help='worlds per candidate and generation (popsize x episodes <= 64); default 1, '
                                                               'or the length of a --dynamics list (then a multiple of it)')
    p.add_argument('--dropout', type=float, default=0., help='p_agent_dropout of the trained agent (0: none; the reference: 0.25)')
    p.add_argument('--dropout-seed', type=int, default=0, help='key of the dropout masks: replica r uses seed + r·stride')
    p.add_argument('--dropout-stride', type=int, default=1, help='0: every replica the same mask; 1: every replica its own')
    p.add_argument('--init-from', default=None, metavar='FILE', help='a saved NeuralAutomataAgent whose weights are the search\'s first centre')
    add_wide_arguments(p)
    args = p.parse_args()
    args.wide_kw = wide_keywords(args)
    if not 0 <= args.memory_channels <= 8 or (args.memory_channels and args.agents_born and args.memory_inherit is None):
        p.error('--memory-channels in 0..8, and together with --agents-born only with --memory-inherit blank|copy (without a rule a '
                'newborn would inherit a dead agent\'s memory)')
    if args.memory_inherit is not None and not args.memory_channels:
        p.error('--memory-inherit needs --memory-channels M')
    if not 0 <= args.signal_channels <= 8:
        p.error('--signal-channels in 0..8')
    args.agents_die = lifecycle(args.agents_die, args.agents_born)      # (what the helpers hand to make_dynamics)
    if not 0. <= args.dropout <= 1. or args.dropout_stride < 0:
        p.error('--dropout in [0, 1], --dropout-stride >= 0')
    args.drop_kw = dropout_keywords(args.dropout, args.dropout_seed, args.dropout_stride)
    try:
        names = dynamics_names(args.dynamics)
        args.episodes = resolve_episodes(names, args.episodes) if len(names) > 1 else (1 if args.episodes is None else args.episodes)
    except ValueError as err:
        p.error(str(err))
    if args.episodes < 1 or (10 if args.time else args.popsize) * args.episodes > 64:
        p.error(f'--episodes {args.episodes}: at least 1, and popsize x episodes at most 64 replicas')
    N = slots(args.max_agents or ('tight' if args.reseed is not None else 'alive'), args.size, args.dynamics, args.agents_die)
    if args.reseed is not None and N == 'alive':
        sys.exit("--reseed needs a fixed slot layout: --max-agents full, tight or a number")
    if args.time:
        time_loops(args, N)
        return
    center_init = None
    if args.init_from is not None:
        loaded = NeuralAutomataAgent.load(args.init_from)
        mismatch = init_from_mismatch(loaded, make_template(args.dropout, args.wide_kw), args.init_from)
        if mismatch:
            sys.exit(mismatch)
        center_init = torch.nn.utils.parameters_to_vector(loaded.model.parameters()).detach()
        print(f'Starting from {args.init_from} ({center_init.numel()} parameters)')
    searcher, pop = make_search(args.size, args.dynamics, args.popsize, args.epoch_iters, args.seed, args.searcher, args.agents_die, N,
                                args.reseed, args.reseed_stride, args.episodes, args.drop_kw, args.dropout, center_init, args.wide_kw)
    print(f'Network has {pop.P} parameters; {args.popsize} candidates' + (f' x {args.episodes} episodes' if args.episodes > 1 else '') +
          f' on {args.size}x{args.size} {args.dynamics}, '
          f'{args.epoch_iters} steps each, max_agents={N}' + ('' if args.reseed is None else
          f', new worlds every generation (seed {args.reseed} + g·{args.popsize * args.episodes}, stride {args.reseed_stride})') +
          (f', dropout {args.dropout} (seed {args.dropout_seed}, stride {args.dropout_stride})' if args.drop_kw else ''), flush=True)
    t0 = time.perf_counter()
    per_episode = []                                              # a list of dynamics: every generation's (C, E) sums, kept on the device
    if len(names) > 1:
        for _ in range(args.generations):
            searcher.step()
            per_episode.append(searcher.episode_fitness.clone())
    else:
        searcher.run(args.generations)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    pop.env.check()
    col = '|grad|' if args.searcher == 'pgpe' else 'sigma'
    for g, (mean, best, worst, median, col4, sd) in enumerate(searcher.history().tolist()):
        under = '' if not per_episode else '  ' + '  '.join(f'{q} {v:.4f}' for q, v in per_dynamics_means(args.dynamics, per_episode[g].cpu()))
        print(f'generation {g:4d}: mean {mean:10.4f}  median {median:10.4f}  best {best:10.4f}  worst {worst:10.4f}  '
              f'{col} {col4:.4f}  stdev {sd:.5f}{under}')
    st = searcher.status
    print(f'{args.generations} generations in {dt:.2f} s; best eval {st["best_eval"]:.4f}, last pop_best {st["pop_best_eval"]:.4f}')
    out = args.out or os.path.join('saved_models', f'neuralautomataagent_{args.searcher}_{args.generations}x{args.epoch_iters}.pt')
    os.makedirs(os.path.dirname(out) or '.', exist_ok=True)
    solution = searcher.pop_best_agent()
    solution.save(out)
    if args.drop_kw:
        solution.dropout_seed = args.dropout_seed                 # the replay below under the counter-based masks too
    print(f'Saving the agent to: {out}')
    # replay pop_best in its own world (the reference replays for epoch_iters * 100 steps with a plotter; here epoch_iters)
    env = Env((args.size, args.size), make_dynamics(names[0], args.size, args.agents_die), seed=args.seed, max_agents='alive')   # (a list: its first)
    reward = run_epoch(env, solution.to(torch.device('cuda')), args.epoch_iters)
    print(f'Final reward of the pop_best solution over {args.epoch_iters} steps: {reward:.4f}  (its generation: {st["pop_best_eval"]:.4f})')


if __name__ == '__main__':
    main()
