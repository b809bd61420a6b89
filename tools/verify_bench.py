"""Times the verify kernels (dlco_desc_verify_hypotheses, through last_kernel_ms: HIP events around the hypothesis, scoring and
selection kernels) at (m, n_hyp) = (2 000, 2 048), (20 000, 4 096) and (100 000, 4 096) on a planted homography with half the
matches outliers, and dlco_desc_verify_homography (the same plus the mask kernel of the best model and of every refit round).
Beside each: the instruction floor of the scoring loop, 19 m n_hyp fp64 vector operations at the chip's rate without fused
multiply-add (256 CUs x 64 lanes a clock x 2.4 GHz = 39.3e12 operations a second: half the 78.6 TFLOPS the fp64 vector
peak counts with FMA), and a float64 torch evaluation of the same counts on the same GPU, in chunks of hypotheses that keep
its temporaries near 256 MB, timed by torch's events.  torch may contract a multiply and an add, so its counts are compared
and the number that differ is printed, not asserted.  One process, three warm-up calls per shape, then `reps` timed calls, the
median.  No gate: it prints what it measured."""
import importlib, os, sys
import numpy as np
import torch                                                # before libdlco.so: one HIP runtime per process, torch's first
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
dlco = importlib.import_module("opencv-dlco_amd")

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
OPS_PER_SECOND = 256 * 64 * 2.4e9
H_TRUE = np.array([[0.92, -0.11, 140.0], [0.08, 1.05, -60.0], [1.5e-5, -1.0e-5, 1.0]])


def planted(m, rng):
    src = rng.uniform((0, 0), (4000, 3000), (m, 2))
    p = np.c_[src, np.ones(m)] @ H_TRUE.T
    dst = p[:, :2] / p[:, 2:] + rng.normal(0, 0.5, (m, 2))
    out = rng.permutation(m)[:m // 2]
    dst[out] = rng.uniform((0, 0), (4000, 3000), (len(out), 2))
    return src.astype(np.float32), dst.astype(np.float32)


def torch_counts(H_all, src, dst, t2):
    """count [n_hyp] of H_all [n_hyp, 9] by the rule's formula in float64 tensors; returns (counts, milliseconds)"""
    dev = torch.device("cuda")
    H = torch.from_numpy(H_all.reshape(-1, 9)).to(dev)
    x, y, u, v = (torch.from_numpy(a.astype(np.float64)).to(dev) for a in (src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]))
    chunk = max(1, (1 << 25) // len(x))
    out = torch.empty(len(H), dtype=torch.int64, device=dev)

    def run():
        for h0 in range(0, len(H), chunk):
            h = H[h0:h0 + chunk, :, None]
            X = (h[:, 0] * x + h[:, 1] * y) + h[:, 2]
            Y = (h[:, 3] * x + h[:, 4] * y) + h[:, 5]
            W = (h[:, 6] * x + h[:, 7] * y) + h[:, 8]
            ex, ey = X - u * W, Y - v * W
            out[h0:h0 + chunk] = ((W > 0) & (ex * ex + ey * ey <= t2 * (W * W))).sum(dim=1)

    for _ in range(2):
        run()
    ms = []
    for _ in range(max(3, reps // 3)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out.cpu().numpy(), float(np.median(ms))


ctx = dlco.DescContext()
rng = np.random.default_rng(0)
print(f"{reps} timed calls per row, medians; floor = 19 m n_hyp / {OPS_PER_SECOND:.3g} fp64 operations a second")
print("| m | n_hyp | verify_hypotheses kernels | instruction floor | torch float64 | verify_homography kernels (refine 2) | inliers |")
print("|---|---|---|---|---|---|---|")
for m, n_hyp in ((2000, 2048), (20000, 4096), (100000, 4096)):
    src, dst = planted(m, rng)
    for _ in range(3):
        H_all, count = ctx.verify_hypotheses(src, dst, 3.0, n_hyp, 0)
    ms = []
    for _ in range(reps):
        ctx.verify_hypotheses(src, dst, 3.0, n_hyp, 0)
        ms.append(ctx.last_kernel_ms())
    full = []
    for _ in range(reps):
        H, mask, best = ctx.verify_homography(src, dst, 3.0, n_hyp, 0, 2)
        full.append(ctx.last_kernel_ms())
    floor_ms = 1e3 * 19.0 * m * n_hyp / OPS_PER_SECOND
    tc, t_ms = torch_counts(H_all, src, dst, 9.0)
    print(f"| {m} | {n_hyp} | {np.median(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) | {floor_ms:.3f} ms | {t_ms:.2f} ms, {int((tc != count).sum())} counts differ "
          f"| {np.median(full):.3f} ms | {int(mask.sum())} of {m}, hypothesis {best} |")
ctx.close()
