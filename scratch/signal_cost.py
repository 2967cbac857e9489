"""Cost of signal channels (LABBOOK §41).

    python scratch/signal_cost.py            # ms per search generation: examples/learning_agents.py's device loop at its README shape
                                             # (10 x 96^2, 30 steps, PGPE, agents_die) on the wide 3 -> 16 -> 3 tanh stack, with and without
                                             # signal_channels=2 (then 5 -> 16 -> 5), one process, interleaved pairs
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scratch/signal_cost.py prof    # the signal loop alone
    python scratch/signal_cost.py bw         # 1 x 2048^2, K = 2: die_signal_step against die_diffuse_decay on the same planes, bytes/s"""
import ctypes as C
import os, sys, time, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
sys.path.insert(0, ROOT)

G = 40
WIDE = dict(hidden_channels=16, hidden_activation='tanh')


def build(signals):
    from learning_agents import make_search
    from population_eval import lifecycle
    kw = dict(WIDE, **(dict(signal_channels=signals) if signals else {}))
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


def bandwidth(W=2048, H=2048, K=2, sigma=0.5, decay=0.1, reps=50):
    from die_amd import _lib
    from die_amd.device_array import stream_ptr
    dev = torch.device('cuda')
    cells = W * H
    field = torch.randn((K, W, H), device=dev) * (torch.rand((K, W, H), device=dev) < 0.6)
    out = torch.empty_like(field)
    emission = torch.tanh(torch.randn((K, W, H), device=dev) * 2)
    # a standing plane with about 15 % of the cells occupied at epoch 5 (slot id 1, payload 0)
    word = ((5 << _lib.OWNER_EPOCH_SHIFT) | 2) << 32
    standing = torch.where(torch.rand((W, H), device=dev) < 0.15, torch.tensor(word, dtype=torch.int64, device=dev),
                           torch.zeros((), dtype=torch.int64, device=dev)).contiguous()
    m = _lib.Medium(W, H, _lib.DIE_F32, 5, None, None, None, None, 0, 0, 0, 0, 0, 0, 0, 0, None)
    sp = stream_ptr(dev)

    def signal():
        _lib.check(_lib.lib.die_signal_step(C.byref(m), standing.data_ptr(), 5, K, emission.data_ptr(), cells, field.data_ptr(), out.data_ptr(),
                                            cells, 1.0, sigma, decay, sp), 'die_signal_step')

    def plain():
        for k in range(K):
            _lib.check(_lib.lib.die_diffuse_decay(field[k].data_ptr(), out[k].data_ptr(), W, H, _lib.DIE_F32, sigma, decay, sp), 'die_diffuse_decay')

    def ms(fn):
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    rows = []
    for _ in range(5):                                       # interleaved
        rows.append((ms(signal), ms(plain)))
    ts, tp = statistics.median(r[0] for r in rows), statistics.median(r[1] for r in rows)
    # bytes a call must move: the field in and out (8 per cell and channel); the signal step also its emission (4) and the words (8)
    bs, bp = K * cells * (4 + 4 + 4 + 8), K * cells * (4 + 4)
    print(f'{W} x {H}, K = {K}, sigma {sigma}: die_signal_step {ts * 1e3:.1f} us a call ({K} planes in one launch), {bs / ts / 1e9:.2f} TB/s of '
          f'{bs / 1e6:.1f} MB (field in + out, emission, standing words read once per channel)')
    print(f'   die_diffuse_decay on the same planes, {K} launches: {tp * 1e3:.1f} us, {bp / tp / 1e9:.2f} TB/s of {bp / 1e6:.1f} MB (field in + out)')
    print('   pairs (signal, plain) ms:', ' '.join(f'({a:.4f}, {b:.4f})' for a, b in rows), flush=True)


if len(sys.argv) > 1 and sys.argv[1] == 'prof':
    s, pop = build(2)
    s.run(G)
    torch.cuda.synchronize()
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == 'bw':
    bandwidth()
    sys.exit(0)

off, plain = build(0)
on, pop = build(2)
a, b = [], []
for i in range(9):
    a.append(timed(off)); b.append(timed(on))
ma, mb = statistics.median(a), statistics.median(b)
print(f'wide 16 tanh: ms per generation (30 steps x 10 replicas, P = {plain.P} -> {pop.P} with 2 signal channels), 9 interleaved pairs of {G} generations')
print('  agents_die                     :', ' '.join(f'{v:.3f}' for v in a), ' median', f'{ma:.3f}', f' = {1e3 / ma:.1f} generations/s')
print('  agents_die + 2 signal channels :', ' '.join(f'{v:.3f}' for v in b), ' median', f'{mb:.3f}', f' = {1e3 / mb:.1f} generations/s')
print(f'  difference of medians {mb - ma:.3f} ms = {(mb - ma) / 30 * 1e3:.2f} us per step; n = {pop.env.n}', flush=True)
