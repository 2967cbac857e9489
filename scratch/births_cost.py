"""Cost of the birth pass per search generation (LABBOOK §29): examples/learning_agents.py's device loop at its README shape (10 x 96^2,
30 steps, PGPE, agents_die), with and without agents_born, in one process, interleaved pairs.

    python scratch/births_cost.py            # ms per generation, both layouts
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scratch/births_cost.py prof    # the born loop alone"""
import os, sys, time, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
sys.path.insert(0, ROOT)
from learning_agents import make_search
from population_eval import lifecycle, slots

G = 40
def build(born, max_agents):
    s, pop = make_search(96, 'st-perlin-wide', 10, 30, 0, 'pgpe', lifecycle(True, born), max_agents)
    s.run(3)
    torch.cuda.synchronize()
    return s, pop

def timed(s):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.run(G)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / G * 1e3

if len(sys.argv) > 1 and sys.argv[1] == 'prof':
    s, pop = build(True, 'alive')
    s.run(G)
    torch.cuda.synchronize()
    sys.exit(0)

for layout in ('alive', slots('tight', 96, 'st-perlin-wide', True)):
    off, _ = build(False, layout)
    on, pop = build(True, layout)
    a, b = [], []
    for i in range(9):
        a.append(timed(off)); b.append(timed(on))
    _, alive = pop.env.read_results(pop.env.run(pop, 30))
    print(f'max_agents={layout}: ms per generation (30 steps x 10 replicas), 9 interleaved pairs of {G} generations')
    print('  agents_die           :', ' '.join(f'{v:.3f}' for v in a), ' median', f'{statistics.median(a):.3f}')
    print('  agents_die+agents_born:', ' '.join(f'{v:.3f}' for v in b), ' median', f'{statistics.median(b):.3f}')
    print(f'  difference of medians {statistics.median(b) - statistics.median(a):.3f} ms = {(statistics.median(b) - statistics.median(a)) / 30 * 1e3:.2f} us per step'
          f'; alive at the end of a 30-step run: {alive[-1].tolist()} of n={pop.env.n}', flush=True)
