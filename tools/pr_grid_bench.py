"""Times a grid of pr-learn settings (dlco_pr_grid_*) at the reference's shape: F = 5120 pooling regions, N rows, one
window of 100 000 iterations (the reference's LogStep) per launch, for G = 1, 8, 64, 256, 768 settings and each number
of settings per workgroup the library offers (1, 2, 4 - 4 only up to F = 5120; "auto" = the library's rule).  Prints
aggregate setting-iterations/s, microseconds per iteration per setting, and one LogStep's validation + statistics time at
G = 256.  Usage: pr_grid_bench.py [N] [iters] [F]"""
import importlib, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
dlco = importlib.import_module("opencv-dlco_amd")

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
F = int(sys.argv[3]) if len(sys.argv) > 3 else 5120
rng = np.random.default_rng(0)
L = (np.arange(N) % 2 == 0).astype(np.uint8)
D = rng.random((N, F), dtype=np.float32)
D[L == 1, :512] *= 0.5
src = dlco.PrContext(F, N, mu=0.025, gamma=0.10)
src.set_data(D, L)
del D


def settings(G):
    mus = np.linspace(0.005, 0.05, G).astype(np.float32)
    gammas = np.tile(np.array([0.1, 0.25, 0.5, 1.0], np.float32), (G + 3) // 4)[:G]
    return mus, gammas


solo_rate = None
for G in (1, 8, 64, 256, 768):
    mus, gammas = settings(G)
    for c in (0, 1, 2, 4) if F <= 5120 else (0, 1, 2):
        g = dlco.PrGrid(src, mus, gammas)
        g.set_group(c)
        used = g.group()
        g.steps(1000)                                   # warm-up launch
        g.state()
        t0 = time.perf_counter()
        g.steps(iters)
        g.state()
        dt = time.perf_counter() - t0
        g.close()
        agg = G * iters / dt
        if G == 1 and c == 0:
            solo_rate = agg
        print(f"F = {F}  G = {G:4d}  C = {used} ({'auto' if c == 0 else 'set'}): {iters} iterations in {dt:.3f} s = {agg / 1e6:8.2f} M setting-it/s "
              f"({1e6 * dt / iters / G:.4f} us per iteration per setting, {agg / solo_rate:.1f}x G = 1)", flush=True)

G = 256
mus, gammas = settings(G)
g = dlco.PrGrid(src, mus, gammas)
g.steps(iters)
g.state()
P = rng.integers(0, 6, (8 * F, 3)).astype(np.float32)
g.validate()
t0 = time.perf_counter()
v = g.validate()
t1 = time.perf_counter()
s = g.stats(P)
t2 = time.perf_counter()
print(f"LogStep at G = {G}: validate {1e3 * (t1 - t0):.1f} ms (20 % split of {N} rows, all settings), "
      f"stats of all {G} settings {1e3 * (t2 - t1):.1f} ms (all {N} rows); nnz(w) {int(v['nnz'].min())} .. {int(v['nnz'].max())}, "
      f"Dim {int(s['dim'].min())} .. {int(s['dim'].max())}")
g.close()
src.close()
