"""Cost of memory channels per search generation (LABBOOK §32): examples/learning_agents.py's device loop at its README shape (10 x 96^2,
30 steps, PGPE, agents_die) on the wide 3 -> 16 -> 3 tanh stack, with and without memory_channels=2 (then 5 -> 16 -> 5), in one
process, interleaved pairs.

    python scratch/memory_cost.py            # ms per generation
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scratch/memory_cost.py prof    # the memory loop alone"""
import os, sys, time, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
sys.path.insert(0, ROOT)
from learning_agents import make_search
from population_eval import lifecycle

G = 40
WIDE = dict(hidden_channels=16, hidden_activation='tanh')
def build(memory):
    kw = dict(WIDE, **(dict(memory_channels=memory) if memory else {}))
    s, pop = make_search(96, 'st-perlin-wide', 10, 30, 0, 'pgpe', lifecycle(True, False), 'alive', wide_kw=kw)
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
    s, pop = build(2)
    s.run(G)
    torch.cuda.synchronize()
    sys.exit(0)

off, plain = build(0)
on, pop = build(2)
a, b = [], []
for i in range(9):
    a.append(timed(off)); b.append(timed(on))
ma, mb = statistics.median(a), statistics.median(b)
print(f'wide 16 tanh: ms per generation (30 steps x 10 replicas, P = {plain.P} -> {pop.P} with 2 memory channels), 9 interleaved pairs of {G} generations')
print('  agents_die                     :', ' '.join(f'{v:.3f}' for v in a), ' median', f'{ma:.3f}', f' = {1e3 / ma:.1f} generations/s')
print('  agents_die + 2 memory channels :', ' '.join(f'{v:.3f}' for v in b), ' median', f'{mb:.3f}', f' = {1e3 / mb:.1f} generations/s')
print(f'  difference of medians {mb - ma:.3f} ms = {(mb - ma) / 30 * 1e3:.2f} us per step; n = {pop.env.n}', flush=True)
