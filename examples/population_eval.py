"""The evaluation half of the reference's examples/learning_agents.py (`run_epoch`, lines 20-38) for a whole population at
once: R NeuralAutomataAgent candidates, each scored by the sum of its rewards over `epoch_iters` steps of its own world,
all R worlds stepped together by die_amd.batch (L + 2 launches per step for an L-layer model, L + 3 with a food flow).

    python examples/population_eval.py [--replicas 10] [--size 96] [--iters 50] [--dynamics st-perlin-wide] [--generations 0] [--agents-die] [--agents-born]
                                       [--max-agents alive|full|tight|N] [--reseed S] [--episodes 1] [--compare]
                                       [--dropout P] [--dropout-seed S] [--dropout-stride K] [--stock-channel] [--memory-channels M [--memory-inherit blank|copy [--memory-mutation A]]]
                                       [--signal-channels K [--signal-sigma S --signal-decay D --signal-deposit G]]

--stock-channel gives the candidates a fourth observation channel, `'agent_food'`: on every cell the stock of the agent standing
there (NeuralAutomataAgent(with_stock_channel=True)), built on the device by one more launch per batched step — what lets a policy
tell a starving agent from a well-fed one under --agents-die / --agents-born.

--memory-channels M (1..8) gives every agent M values it carries from one step to the next (NeuralAutomataAgent(memory_channels=M)):
the stack becomes a wide stack that reads them as M more observation planes and writes them as M more output planes (three more
launches per batched step).  Every evaluation and every search generation starts from blank memory.  With --agents-born it needs
--memory-inherit {blank,copy} [--memory-mutation A]: what a newborn's memory holds (NeuralAutomataAgent(memory_inherit=...,
memory_mutation=A): blank, its parent's, or its parent's plus uniform noise of half-width A; one more launch per batched step, two
in the first step after a birth pass is asked for its record).

--signal-channels K (1..8) gives the agents a field of K planes they write and read (NeuralAutomataAgent(signal_channels=K)): the
stack, a wide stack, reads the planes as K more observation channels and emits into them through K more output planes at the
cells the agents stand on; the field then diffuses (--signal-sigma, default 0.5) and decays (--signal-decay, default 0.1), two
more launches per batched step.  --signal-deposit scales the emission.  Every evaluation and every search generation starts from
a blank field.  K = 0, 1, 2, 4 varies the medium's capacity for message passing.

--dynamics picks one of the reference's three worlds (learning_agents.py `dynamics_choice`): 'st-perlin', 'st-perlin-wide' or
'dyn-pred', where the food flows in running waves (WaveSequence.get_flow_operator, one more launch per batched step).
A comma list (e.g. st-perlin,st-perlin-wide,dyn-pred) scores every candidate under EVERY listed dynamics in the same launches
(BatchedEnv(dynamics=[...]): per-replica Dynamics): it implies --episodes len(list) unless --episodes is given, which must then be a
multiple of it (episode e lives under dynamics e mod len), and the mean score under each dynamics is printed.
--agents-die adds the death pressure (Dynamics(agents_die=True): starved agents are zeroed; one more launch per batched step).
--agents-born adds births (Dynamics(agents_born=True): after a step's deaths the agents with more than 0.5 food breed into dead
slots, in slot order; three more launches per batched step).  Colonies can only grow where there are dead slots: use it with
--agents-die or a --max-agents layout other than 'alive'.
--max-agents picks the replicas' slot layout: 'alive' (K_r slots, the seeded agents), 'full' (W·H, the reference's default),
'tight' (the expected count plus six standard deviations) or a number; every layout but 'alive' runs the dead-slot pass.
--reseed S (with --generations, a fixed layout): generation g evaluates on the world of seed S + g, seeded on the device by
BatchedEnv.reset(seed=...) in the one batch built up front, instead of a batch rebuilt on the host.

--episodes E scores every candidate on E worlds (seeds seed … seed + E − 1, the same E for every candidate) in the same launches
— replicas·E batched replicas, at most 64 — and prints the mean and the spread of its E sums.

--dropout P gives the candidates the reference's `p_agent_dropout=P` (its learning_agents.py trains with 0.25) in training mode:
replica r's sense planes are multiplied by the counter-based mask of key --dropout-seed + r·--dropout-stride (stride 0: one mask
for every replica), new at every step, inside the last conv launch.

--generations G runs a plain Gaussian evolution strategy (antithetic samples, normalised fitness) on the mean parameter
vector — the training loop itself (evotorch's PGPE, MLflow) stays out of scope.  --compare times the same population one
candidate at a time through `Env` + `NeuralAutomataAgent` (what a direct port of run_epoch does; every world with a flow
operator of its own), checks that both give the same fitness, and prints candidate-steps/s for both.
"""
import argparse
import math
import os
import sys
import time

import torch
from torch.nn.utils import parameters_to_vector

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from die_amd import Dynamics, Env, NeuralAutomataAgent, WaveSequence    # noqa: E402
from die_amd.batch import BatchedEnv, BatchedNeuralAutomataAgent, episode_dynamics, episode_seeds   # noqa: E402

AGENT_KW = dict(kernel_sizes=[3, 3], scale=0.01, deposit=2.0)           # learning_agents.py
DYNAMICS = ('st-perlin', 'st-perlin-wide', 'dyn-pred')


def make_dynamics(choice, size, agents_die=False):
    """learning_agents.py's `dynamics_choice[choice]`, with a fresh flow operator (its time counter at 0) for 'dyn-pred';
    `agents_die`: starved agents die (the reference's 'not dying' pressure) — True / False, or `lifecycle(...)`'s dict of the
    lifecycle fields when births are on too (every helper below hands it through to here)."""
    life = dict(agents_die) if isinstance(agents_die, dict) else dict(agents_die=bool(agents_die))
    if choice == 'st-perlin':
        return Dynamics(food_infinite=True, **life)
    if choice == 'st-perlin-wide':
        return Dynamics(food_infinite=True, rate_decay_chem=0.025, diffuse_sigma=.8, **life)
    return Dynamics(food_infinite=False, op_food_flow=WaveSequence((size, size), dt=0.01).get_flow_operator(scale=0.5, decay=0.5), **life)


def lifecycle(agents_die, agents_born):
    """--agents-die / --agents-born as the `agents_die` argument of the helpers here: the plain flag without births."""
    return dict(agents_die=bool(agents_die), agents_born=True) if agents_born else bool(agents_die)


def dynamics_names(spec):
    """--dynamics: one name or a comma list of names -> the list, every name checked."""
    names = [q.strip() for q in spec.split(',')]
    for q in names:
        if q not in DYNAMICS:
            raise ValueError(f'--dynamics {q!r}: one of {", ".join(DYNAMICS)} (or a comma list of them)')
    return names


def resolve_episodes(names, episodes):
    """--episodes for a --dynamics list of L names: L when not given (None), else a multiple of L."""
    if episodes is None:
        return len(names)
    if episodes < 1 or episodes % len(names):
        raise ValueError(f'--episodes {episodes}: a multiple of the {len(names)} dynamics of --dynamics')
    return episodes


def batch_dynamics(choice, size, agents_die, candidates, episodes):
    """BatchedEnv's `dynamics` for --dynamics `choice`: the one Dynamics of a single name; for a list of L names the C·E per-replica
    Dynamics in candidate-major order, episode e under dynamics e mod L ('dyn-pred' entries share ONE flow operator)."""
    names = dynamics_names(choice)
    if len(names) == 1:
        return make_dynamics(names[0], size, agents_die)
    made = {q: make_dynamics(q, size, agents_die) for q in set(names)}
    return episode_dynamics([made[names[e % len(names)]] for e in range(episodes)], candidates)


def per_dynamics_means(choice, episode_sums):
    """(name, mean over candidates and that name's episodes) for a (C, E) nested list / tensor of per-episode sums."""
    names = dynamics_names(choice)
    rows = [list(map(float, row)) for row in episode_sums]
    out = []
    for j, q in enumerate(names):
        vals = [row[e] for row in rows for e in range(j, len(row), len(names))]
        out.append((q, sum(vals) / len(vals)))
    return out


def slots(spec, size, choice, agents_die=False):
    """BatchedEnv max_agents of a --max-agents value: 'alive', 'full' (None: W·H), 'tight' or a number.  'tight' is the expected
    number of seeded agents plus six standard deviations, a bound every seed of the example's worlds stays under."""
    if spec == 'alive':
        return 'alive'
    if spec == 'full':
        return None
    if spec == 'tight':
        p, cells = make_dynamics(dynamics_names(choice)[0], size, agents_die).init_agent_ratio, size * size
        return math.ceil(p * cells + 6.0 * math.sqrt(p * (1.0 - p) * cells))
    return int(spec)


def make_template(dropout=0., wide_kw=None):
    """The candidates' architecture; `dropout` > 0: with the reference's p_agent_dropout (the model stays in training mode);
    `wide_kw`: wide_keywords' hidden_channels / hidden_activation (none: the reference's 3-channel linear stack)."""
    return NeuralAutomataAgent(**AGENT_KW, **(dict(p_agent_dropout=dropout) if dropout > 0 else {}), **(wide_kw or {}))


def add_wide_arguments(p):
    p.add_argument('--hidden-channels', type=int, default=None, metavar='C', help='width of the hidden layers, 1..32 (default: the '
                                                                                  'observation\'s 3 channels, the narrow kernels)')
    p.add_argument('--hidden-activation', choices=('tanh', 'relu', 'none'), default='none', help='activation after every layer but the last')
    p.add_argument('--stock-channel', action='store_true', help="the candidates sense their own food stock: a last observation channel "
                                                                "'agent_food' (with_stock_channel=True; one more launch per batched step)")
    p.add_argument('--memory-channels', type=int, default=0, metavar='M', help='values every agent carries between steps, 1..8 (memory_channels=M: '
                                                                               'a wide stack, three more launches per batched step; with '
                                                                               '--agents-born it needs --memory-inherit)')
    p.add_argument('--memory-inherit', choices=('blank', 'copy'), default=None, help="what a newborn's memory holds under --agents-born: "
                                                                                      "blank, or a copy of its parent's (memory_inherit=...)")
    p.add_argument('--memory-mutation', type=float, default=0.0, metavar='A', help="with --memory-inherit copy: uniform noise of half-width A "
                                                                                   "added to the parent's values (memory_mutation=A)")
    p.add_argument('--signal-channels', type=int, default=0, metavar='K', help='planes of a field the agents write and read, 1..8 '
                                                                               '(signal_channels=K: a wide stack, two more launches per batched step)')
    p.add_argument('--signal-sigma', type=float, default=None, metavar='S', help="the signal field's gaussian sigma (default 0.5; radius int(4 S + .5) in 1..8)")
    p.add_argument('--signal-decay', type=float, default=None, metavar='D', help="the signal field's decay per step, in [0, 1] (default 0.1)")
    p.add_argument('--signal-deposit', type=float, default=None, metavar='G', help='what an emission of 1 adds to a cell (default 1.0)')


def wide_keywords(args):
    """NeuralAutomataAgent's keywords for --hidden-channels C --hidden-activation A --stock-channel --memory-channels M
    --signal-channels K with its three constants (none when none is given; the constants only beside K > 0)."""
    kw = {}
    if getattr(args, 'stock_channel', False):
        kw['with_stock_channel'] = True
    if getattr(args, 'memory_channels', 0):
        kw['memory_channels'] = args.memory_channels
    if getattr(args, 'memory_inherit', None) is not None:
        kw.update(memory_inherit=args.memory_inherit, memory_mutation=args.memory_mutation)
    if getattr(args, 'signal_channels', 0):
        kw['signal_channels'] = args.signal_channels
        for name in ('signal_sigma', 'signal_decay', 'signal_deposit'):
            if getattr(args, name, None) is not None:
                kw[name] = getattr(args, name)
    if args.hidden_channels is not None:
        kw['hidden_channels'] = args.hidden_channels
    if args.hidden_activation != 'none':
        kw['hidden_activation'] = args.hidden_activation
    return kw


def dropout_keywords(dropout, seed, stride):
    """BatchedNeuralAutomataAgent's keywords for --dropout P --dropout-seed S --dropout-stride K (none for P = 0)."""
    return dict(dropout_seed=seed, dropout_seed_stride=stride) if dropout > 0 else {}


def make_population(size, template, rows, seed, choice, agents_die=False, max_agents='alive', episodes=1, drop_kw=None):
    C = rows.shape[0]                                  # every candidate starts on the same world (with episodes: the same E worlds)
    benv = BatchedEnv((size, size), batch_dynamics(choice, size, agents_die, C, episodes), replicas=C * episodes,
                      seeds=episode_seeds(seed, C, episodes), max_agents=max_agents)
    return benv, BatchedNeuralAutomataAgent(benv, template, rows, episodes=episodes, **(drop_kw or {}))


def evaluate_population(benv, pop, iters):
    """Fitness of every replica: the sum of its world's rewards over `iters` steps (run_epoch for all of them)."""
    rewards, _ = BatchedEnv.read_results(benv.run(pop, iters))
    return [sum(rewards[:, r].tolist()) for r in range(benv.R)]        # (summed in step order, like run_epoch)


def candidate_fitness(sums, episodes):
    """Per-replica sums -> per-candidate means over its E worlds, added in episode order (the searchers' fold)."""
    return [sum(sums[c * episodes:(c + 1) * episodes], 0.0) / episodes for c in range(len(sums) // episodes)]


def run_epoch(env, agent, iters):
    """run_epoch of the reference, one candidate."""
    obs, epoch_reward = env._get_current_obs, 0.
    for _ in range(iters):
        obs, reward, _, _, _ = env.step(agent.forward(obs))
        epoch_reward += reward
    return epoch_reward


def one_at_a_time_worlds(size, R, seed, choice, agents_die=False, max_agents='alive', episodes=1):
    names = dynamics_names(choice)                   # replica c·E + e lives under dynamics e mod L, with a flow operator of its own
    return [Env((size, size), make_dynamics(names[(r % episodes) % len(names)], size, agents_die), seed=q, max_agents=max_agents)
            for r, q in enumerate(episode_seeds(seed, R, episodes))]


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--replicas', type=int, default=10)
    p.add_argument('--size', type=int, default=96)
    p.add_argument('--iters', type=int, default=50, help='epoch_iters: steps per evaluation')
    p.add_argument('--dynamics', default='st-perlin-wide', help=f'one of {", ".join(DYNAMICS)}, or a comma list: every candidate on each')
    p.add_argument('--generations', type=int, default=0)
    p.add_argument('--sigma', type=float, default=0.1)
    p.add_argument('--lr', type=float, default=0.05)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--compare', action='store_true')
    p.add_argument('--agents-die', action='store_true', help='Dynamics(agents_die=True): starved agents die')
    p.add_argument('--agents-born', action='store_true', help='Dynamics(agents_born=True): well-fed agents breed into dead slots')
    p.add_argument('--max-agents', default='alive', help="slots per replica: 'alive', 'full' (W·H), 'tight' or a number")
    p.add_argument('--reseed', type=int, default=None, help='--generations on the device-seeded world of seed S + g (fixed layout)')
    p.add_argument('--episodes', type=int, default=None, help='worlds per candidate (replicas x episodes <= 64); default 1, or the '
                                                               'length of a --dynamics list (then a multiple of it)')
    p.add_argument('--dropout', type=float, default=0., help='p_agent_dropout of the candidates (0: none), masked on the device')
    p.add_argument('--dropout-seed', type=int, default=0, help='key of the dropout masks: replica r uses seed + r·stride')
    p.add_argument('--dropout-stride', type=int, default=1, help='0: every replica the same mask; 1: every replica its own')
    add_wide_arguments(p)
    args = p.parse_args()
    if not 0. <= args.dropout <= 1. or args.dropout_stride < 0:
        p.error('--dropout in [0, 1], --dropout-stride >= 0')
    drop_kw = dropout_keywords(args.dropout, args.dropout_seed, args.dropout_stride)
    try:
        names = dynamics_names(args.dynamics)
        args.episodes = resolve_episodes(names, args.episodes) if len(names) > 1 else (1 if args.episodes is None else args.episodes)
    except ValueError as err:
        p.error(str(err))
    R, E = args.replicas, args.episodes
    pressures = (' with agents_die' if args.agents_die else '') + (' with agents_born' if args.agents_born else '')
    args.agents_die = lifecycle(args.agents_die, args.agents_born)
    if E < 1 or R * E > 64:
        p.error(f'--episodes {E}: at least 1, and {R} replicas x episodes at most 64')
    N = slots(args.max_agents, args.size, args.dynamics, args.agents_die)
    if args.reseed is not None and N == 'alive':
        sys.exit("--reseed needs a fixed slot layout: --max-agents full, tight or a number")
    if args.memory_channels and args.agents_born and args.memory_inherit is None:
        p.error('--memory-channels with --agents-born needs --memory-inherit blank|copy (what a newborn\'s memory holds)')
    torch.manual_seed(args.seed)
    try:
        template = make_template(args.dropout, wide_keywords(args))
    except ValueError as err:
        p.error(str(err))
    cands = []
    for _ in range(R):
        template.model.init_weights()
        cands.append(parameters_to_vector(template.model.parameters()).detach().clone())
    rows = torch.stack(cands)
    print(f'{R} candidates of {rows.shape[1]} parameters' + (f' on {E} worlds each' if E > 1 else '') +
          f', {args.size}x{args.size}, {args.iters} steps each, {args.dynamics}'
          f'{pressures}, max_agents={N}' +
          (f', dropout {args.dropout} (seed {args.dropout_seed}, stride {args.dropout_stride})' if drop_kw else ''), flush=True)

    benv, pop = make_population(args.size, template, rows, args.seed, args.dynamics, args.agents_die, N, E, drop_kw)
    sums = evaluate_population(benv, pop, args.iters)
    fitness = candidate_fitness(sums, E)
    for r, f in enumerate(fitness):
        worlds = sums[r * E:(r + 1) * E]
        print(f'candidate {r:2d}: fitness {f:.6f}' + (f'  (its {E} worlds: {min(worlds):.6f} … {max(worlds):.6f})' if E > 1 else ''))
    if len(names) > 1:
        print('mean score under each dynamics: ' + ', '.join(f'{q} {v:.6f}' for q, v in
                                                              per_dynamics_means(args.dynamics, [sums[c * E:(c + 1) * E] for c in range(R)])))
    best = max(range(R), key=lambda r: fitness[r])
    print(f'best: candidate {best} ({fitness[best]:.6f}); pop.candidate({best}).save(...) keeps it', flush=True)

    if args.compare:
        # only the stepping is timed (the worlds are built before); warm-up of both paths first
        dev = torch.device('cuda')
        agents = [pop.replica_agent(r).to(dev) for r in range(R * E)]        # replica r is stepped by its candidate's agent (and its own mask key)
        evaluate_population(*make_population(args.size, template, rows, args.seed, args.dynamics, args.agents_die, N, E, drop_kw), 2)
        run_epoch(one_at_a_time_worlds(args.size, 1, args.seed, args.dynamics, args.agents_die, N)[0], agents[0], 2)
        agents[0].dropout_step = 0                                           # (the warm-up advanced its mask counter)
        agents[0].reset_memory()                                             # (… and left its memory, with --memory-channels)
        agents[0].reset_signals()                                            # (… and its field, with --signal-channels)
        benv, pop = make_population(args.size, template, rows, args.seed, args.dynamics, args.agents_die, N, E, drop_kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batched = evaluate_population(benv, pop, args.iters)
        t_batch = time.perf_counter() - t0
        worlds = one_at_a_time_worlds(args.size, R, args.seed, args.dynamics, args.agents_die, N, E)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        alone = [run_epoch(env, ag, args.iters) for env, ag in zip(worlds, agents)]
        torch.cuda.synchronize()
        t_alone = time.perf_counter() - t0
        cs = R * E * args.iters
        print(f'batched:       {cs / t_batch:12.0f} candidate-steps/s  ({t_batch * 1e3:.2f} ms)')
        print(f'one at a time: {cs / t_alone:12.0f} candidate-steps/s  ({t_alone * 1e3:.2f} ms)')
        print(f'speed-up: {t_alone / t_batch:.2f}x   same fitness: {batched == alone}', flush=True)
        if batched != alone:
            sys.exit('the batched fitness differs from the one-at-a-time fitness')

    if args.generations and R < 2:
        sys.exit('--generations needs at least 2 replicas (antithetic pairs)')
    mean = rows.mean(dim=0)
    for g in range(args.generations):
        half = torch.randn((R // 2, mean.numel()))
        noise = torch.cat([half, -half])                                    # antithetic pairs
        samples = mean + args.sigma * noise
        if args.reseed is not None:                                         # the one batch, a new world seeded on the device
            pop.set_parameters(samples)
            if E == 1:
                benv.reset(seed=args.reseed + g, seed_stride=0)
            else:                                                           # E new worlds, the same for every candidate
                benv.reset(seeds=episode_seeds(args.reseed + g * E, R, E))
            if pop.memory is not None:                                      # --memory-channels: a new world starts from blank memory
                pop.reset_memory()
            pop.reset_signals()                                             # --signal-channels: … and from a blank field
            fit = candidate_fitness(evaluate_population(benv, pop, args.iters), E)
        else:
            gen_benv, gen_pop = make_population(args.size, template, samples, args.seed + 1 + g * E, args.dynamics, args.agents_die, N, E, drop_kw)
            gen_pop.dropout_step = g * args.iters                           # (a fresh population: new masks every generation all the same)
            fit = candidate_fitness(evaluate_population(gen_benv, gen_pop, args.iters), E)
        f = torch.tensor(fit, dtype=torch.float32)
        f = (f - f.mean()) / (f.std() + 1e-8)
        mean = mean + args.lr / (noise.shape[0] * args.sigma) * (noise.T @ f)
        print(f'generation {g}: mean fitness {sum(fit) / len(fit):.6f}  best {max(fit):.6f}', flush=True)


if __name__ == '__main__':
    main()
