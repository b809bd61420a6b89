"""Times the two kHomTrain instantiations of the matcher's tile loops that no mode of tools/match_bench.py launches: the float
STORE form beyond one chunk (cross_sqdists_guided, 4096 x 4096, r = 200, h_side 1) and the byte batch form beyond one chunk
(match_pairs_guided_u8_device, 9 images of 2048 rows, all 72 ordered pairs, r = 200, h_side 1), on the geometry of match_bench's
--guided.  One warm-up, five timed calls each; kernel time from last_kernel_ms.  An argument names another tree whose package
is loaded instead of this one's (a parent commit's build, to compare against)."""
import importlib, os, sys, time
sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
dlco = importlib.import_module("opencv-dlco_amd")

ctx = dlco.DescContext()
rng = np.random.default_rng(0)
nq = nt = 4096
r = 200
S = 8.0 * nt ** 0.5
H = np.array([[0.98, -0.05, 0.03 * S], [0.04, 1.02, -0.02 * S], [0.02 / S, -0.01 / S, 1.0]])
Q = rng.normal(0, 0.25, (nq, r)).astype(np.float32)
T = rng.normal(0, 0.25, (nt, r)).astype(np.float32)
qxy = (rng.random((nq, 2)) * S).astype(np.float32)
txy = (rng.random((nt, 2)) * S).astype(np.float32)
ms, wall = [], []
for k in range(6):
    t0 = time.perf_counter()
    out = ctx.cross_sqdists_guided(Q, qxy, T, txy, H, 12.0, 1)
    wall.append(1e3 * (time.perf_counter() - t0))
    ms.append(ctx.last_kernel_ms())
print("cross_sqdists_guided %d x %d r %d h_side 1: kernels %s ms, wall %s ms, finite %.2f %%" % (
    nq, nt, r, " ".join("%.3f" % v for v in ms[1:]), " ".join("%.1f" % v for v in wall[1:]), 100 * float(np.isfinite(out).mean())), flush=True)

sizes = [2048] * 9
seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
pairs = np.array([(a, b) for a in range(9) for b in range(9) if a != b], np.int32)
rows = int(dlco.match_pairs_rows(seg, pairs)[-1])
gen = torch.Generator(device="cuda:0").manual_seed(0)
X = torch.empty((int(seg[-1]), r), dtype=torch.float32, device="cuda:0").normal_(0, 0.25, generator=gen)
S = 8.0 * 2048 ** 0.5
xy = torch.rand((int(seg[-1]), 2), device="cuda:0", generator=gen) * S
H = np.array([[0.98, -0.05, 0.03 * S], [0.04, 1.02, -0.02 * S], [0.02 / S, -0.01 / S, 1.0]])
M = np.stack([H @ np.array([[1.0, 0.0, 2.0 * np.cos(p)], [0.0, 1.0, 2.0 * np.sin(p)], [0.0, 0.0, 1.0]]) for p in range(len(pairs))])
lo = X.min(0).values
ld = (r + 15) // 16 * 16
Xu = torch.zeros((len(X), ld), dtype=torch.uint8, device="cuda:0")
Xu[:, :r] = ((X - lo) * (255.0 / float((X.max(0).values - lo).max()))).round().clamp(0, 255).to(torch.uint8)
oi = torch.empty((rows, 2), dtype=torch.int32, device="cuda:0")
od = torch.empty((rows, 2), dtype=torch.int32, device="cuda:0")
torch.cuda.synchronize()
ms = []
for k in range(6):
    ctx.match_pairs_guided_u8_device(Xu.data_ptr(), xy.data_ptr(), seg, pairs, r, M, oi.data_ptr(), od.data_ptr(), 12.0, 1, ld=ld, ldxy=2)
    ms.append(ctx.last_kernel_ms())
print("match_pairs_guided_u8 9 x 2048 rows, 72 pairs, r %d h_side 1: kernels %s ms, two admitted rows for %.1f %%" % (
    r, " ".join("%.3f" % v for v in ms[1:]), 100 * float((oi[:, 1] >= 0).float().mean())), flush=True)
ctx.close()
