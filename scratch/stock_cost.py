"""Cost of the stock channel per search generation (LABBOOK §30): examples/learning_agents.py's device loop at its README shape (10 x 96^2,
30 steps, PGPE, agents_die), with and without with_stock_channel, in one process, interleaved pairs.

    python scratch/stock_cost.py            # ms per generation, narrow and wide (3 -> 16 -> 3) stacks
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scratch/stock_cost.py prof    # the stock loop alone"""
import os, sys, time, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
sys.path.insert(0, ROOT)
from learning_agents import make_search
from population_eval import lifecycle

G = 40
def build(stock, wide_kw):
    kw = dict(wide_kw, **(dict(with_stock_channel=True) if stock else {}))
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
    s, pop = build(True, {})
    s.run(G)
    torch.cuda.synchronize()
    sys.exit(0)

for name, wide_kw in (('narrow (3, 3)', {}), ('wide 16 tanh', dict(hidden_channels=16, hidden_activation='tanh'))):
    off, _ = build(False, wide_kw)
    on, pop = build(True, wide_kw)
    a, b = [], []
    for i in range(9):
        a.append(timed(off)); b.append(timed(on))
    print(f'{name}: ms per generation (30 steps x 10 replicas, P = {pop.P} with the channel), 9 interleaved pairs of {G} generations')
    print('  agents_die                :', ' '.join(f'{v:.3f}' for v in a), ' median', f'{statistics.median(a):.3f}')
    print('  agents_die + stock channel:', ' '.join(f'{v:.3f}' for v in b), ' median', f'{statistics.median(b):.3f}')
    print(f'  difference of medians {statistics.median(b) - statistics.median(a):.3f} ms = {(statistics.median(b) - statistics.median(a)) / 30 * 1e3:.2f} us per step'
          f'; n = {pop.env.n}', flush=True)
