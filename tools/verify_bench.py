"""Times the verify kernels (dlco_desc_verify_hypotheses, through last_kernel_ms: HIP events around the hypothesis, scoring and
selection kernels) at (m, n_hyp) = (2 000, 2 048), (20 000, 4 096) and (100 000, 4 096) on a planted homography with half the
matches outliers, and dlco_desc_verify_homography (the same plus the mask kernel of the best model and of every refit round).
Beside each: the instruction floor of the scoring loop, 19 m n_hyp fp64 vector operations at the chip's rate without fused
multiply-add (256 CUs x 64 lanes a clock x 2.4 GHz = 39.3e12 operations a second: half the 78.6 TFLOPS the fp64 vector
peak counts with FMA), and a float64 torch evaluation of the same counts on the same GPU, in chunks of hypotheses that keep
its temporaries near 256 MB, timed by torch's events.  torch may contract a multiply and an add, so its counts are compared
and the number that differ is printed, not asserted.  One process, three warm-up calls per shape, then `reps` timed calls, the
median.  No gate: it prints what it measured.

    verify_bench.py [reps] --fundamental
times dlco_desc_verify_fundamental_hypotheses / dlco_desc_verify_fundamental instead, at the same three shapes on a planted
two-camera scene (points with depth, a turned camera moved sideways, 0.3 pixels of noise) with half the matches outliers, at a
threshold of 1 pixel.  The floor counts the 33 fp64 operations of the Sampson test per pair (epipolar_rules.hpp, kOpsPerPair).
Here torch's counts must agree with the library's: the run ends with an error when they do not.

    verify_bench.py --pairs [--fundamental]
times one dlco_desc_verify_pairs_homography (_fundamental) call over many match lists against a Python loop of the single
calls on the same lists in the same process: 72 pairs x 2 000 matches x 2 048 hypotheses and 1 056 pairs x 500 matches x 1 024
hypotheses, refine 2, the same planted scenes.  One warm-up each, then three rounds that alternate batch and loop; per side the
best round and the range, for the kernels (last_kernel_ms, summed over the loop's calls) and for the wall clock around the
Python call(s).  The answers of the two sides are compared for equality, and the run ends with an error when they differ; the
last line says whether the batch's slowest wall time is below the loop's fastest on every workload.

    verify_bench.py --pairs --device [--fundamental]
times dlco_desc_verify_pairs_homography_device (_fundamental_device), whose refit rounds run on the device, on lists already in
device memory against dlco_desc_verify_pairs_homography (_fundamental), whose refit is formed on the host, on the same lists in
host memory: the two workloads above, refine 2.  Both sides are the library's C calls on arrays prepared beforehand, so neither
wall time holds the packing of Python lists.  One warm-up each, then three rounds that alternate the two; per side the best round
and the range, kernels (last_kernel_ms) and wall.  Matrices, masks (read back from device memory after the timing), counts and
best hypotheses of the two sides must be the same bytes, or the run ends with an error; the last line says whether the device
form's slowest wall time is below the host form's fastest on every workload."""
import importlib, os, sys, time
import numpy as np
import torch                                                # before libdlco.so: one HIP runtime per process, torch's first
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
dlco = importlib.import_module("opencv-dlco_amd")

FUNDAMENTAL = "--fundamental" in sys.argv[1:]
PAIRS = "--pairs" in sys.argv[1:]
DEVICE = "--device" in sys.argv[1:]
args = [a for a in sys.argv[1:] if a not in ("--fundamental", "--pairs", "--device")]
reps = int(args[0]) if args else 15
OPS_PER_PAIR, THRESHOLD = (33.0, 1.0) if FUNDAMENTAL else (19.0, 3.0)
OPS_PER_SECOND = 256 * 64 * 2.4e9
H_TRUE = np.array([[0.92, -0.11, 140.0], [0.08, 1.05, -60.0], [1.5e-5, -1.0e-5, 1.0]])


def planted(m, rng):
    src = rng.uniform((0, 0), (4000, 3000), (m, 2))
    p = np.c_[src, np.ones(m)] @ H_TRUE.T
    dst = p[:, :2] / p[:, 2:] + rng.normal(0, 0.5, (m, 2))
    out = rng.permutation(m)[:m // 2]
    dst[out] = rng.uniform((0, 0), (4000, 3000), (len(out), 2))
    return src.astype(np.float32), dst.astype(np.float32)


def two_cameras(m, rng):
    P = np.c_[rng.uniform(-2.0, 2.0, m), rng.uniform(-1.5, 1.5, m), rng.uniform(4.0, 8.0, m)]
    cy, sy, cx, sx = np.cos(0.1), np.sin(0.1), np.cos(0.03), np.sin(0.03)
    R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Q = P @ R.T + np.array([-0.5, 0.02, 0.05])
    src, dst = 800.0 * P[:, :2] / P[:, 2:] + (512, 384), 800.0 * Q[:, :2] / Q[:, 2:] + (512, 384) + rng.normal(0, 0.3, (m, 2))
    out = rng.permutation(m)[:m // 2]
    dst[out] = rng.uniform((0, 0), (1024, 768), (len(out), 2))
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
            if FUNDAMENTAL:
                l0 = (h[:, 0] * x + h[:, 1] * y) + h[:, 2]
                l1 = (h[:, 3] * x + h[:, 4] * y) + h[:, 5]
                l2 = (h[:, 6] * x + h[:, 7] * y) + h[:, 8]
                e = (u * l0 + v * l1) + l2
                m0 = (h[:, 0] * u + h[:, 3] * v) + h[:, 6]
                m1 = (h[:, 1] * u + h[:, 4] * v) + h[:, 7]
                S = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
                out[h0:h0 + chunk] = ((S > 0) & (e * e <= t2 * S)).sum(dim=1)
                continue
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


def pairs_bench():
    ctx = dlco.DescContext()
    single, batch = (ctx.verify_fundamental, ctx.verify_pairs_fundamental) if FUNDAMENTAL else (ctx.verify_homography, ctx.verify_pairs_homography)
    name = "fundamental" if FUNDAMENTAL else "homography"
    print(f"verify_pairs_{name} against a loop of verify_{name}: best of 3 alternating rounds (min .. max), threshold {THRESHOLD}, refine 2")
    print("| pairs | m | n_hyp | batch kernels | loop kernels | batch wall | loop wall | wall ratio | inliers |")
    print("|---|---|---|---|---|---|---|---|---|")
    faster = True
    for P, m, n_hyp in ((72, 2000, 2048), (1056, 500, 1024)):
        rng = np.random.default_rng(P)
        lists = [(two_cameras if FUNDAMENTAL else planted)(m, rng) for _ in range(P)]

        def run_batch():
            t0 = time.perf_counter()
            out = batch(lists, THRESHOLD, n_hyp, 0, 2)
            return out, 1e3 * (time.perf_counter() - t0), ctx.last_kernel_ms()

        def run_loop():
            out, kernels = [], 0.0
            t0 = time.perf_counter()
            for src, dst in lists:
                out.append(single(src, dst, THRESHOLD, n_hyp, 0, 2))
                kernels += ctx.last_kernel_ms()
            return out, 1e3 * (time.perf_counter() - t0), kernels

        got, want = run_batch()[0], run_loop()[0]              # the warm-up of each side, and the comparison
        for p, (g, w) in enumerate(zip(got, want)):
            if not (np.array_equal(g[0].view(np.uint64), w[0].view(np.uint64)) and np.array_equal(g[1], w[1]) and g[2] == w[2]):
                sys.exit(f"verify_bench: pair {p} of the batch differs from the single call")
        b, l = [], []
        for _ in range(3):
            b.append(run_batch()[1:])
            l.append(run_loop()[1:])
        (bw, bk), (lw, lk) = (np.array(x).T for x in (b, l))
        row = lambda a: f"{a.min():.3f} ms ({a.min():.3f} .. {a.max():.3f})"
        print(f"| {P} | {m} | {n_hyp} | {row(bk)} | {row(lk)} | {row(bw)} | {row(lw)} | {lw.min() / bw.min():.1f}x | {sum(int(g[1].sum()) for g in got)} of {P * m} |")
        faster = faster and bw.max() < lw.min()
    print("the batch's slowest wall time is below the loop's fastest on every workload" if faster else "the batch did NOT beat the loop by more than the spread")
    ctx.close()


def device_bench():
    import ctypes as C
    ctx = dlco.DescContext()
    name = "fundamental" if FUNDAMENTAL else "homography"
    host_call = getattr(ctx.L, f"dlco_desc_verify_pairs_{name}")
    dev_call = getattr(ctx.L, f"dlco_desc_verify_pairs_{name}_device")
    ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    print(f"verify_pairs_{name}_device on lists in device memory against verify_pairs_{name} on the same lists in host memory: "
          f"best of 3 alternating rounds (min .. max), threshold {THRESHOLD}, refine 2")
    print("| pairs | m | n_hyp | device kernels | host kernels | device wall | host wall | wall ratio | inliers |")
    print("|---|---|---|---|---|---|---|---|---|")
    faster = True
    for P, m, n_hyp in ((72, 2000, 2048), (1056, 500, 1024)):
        rng = np.random.default_rng(P)
        lists = [(two_cameras if FUNDAMENTAL else planted)(m, rng) for _ in range(P)]
        src, dst = (np.ascontiguousarray(np.concatenate([l[k] for l in lists])) for k in (0, 1))
        moff = (np.arange(P + 1) * m).astype(np.int64)
        tsrc, tdst = torch.from_numpy(src).to("cuda"), torch.from_numpy(dst).to("cuda")
        tmask = torch.zeros(P * m, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        out = {side: (np.zeros((P, 9)), np.zeros(P * m, np.uint8), np.zeros(P, np.int64), np.zeros(P, np.int32)) for side in ("device", "host")}

        def run(side):
            M, mask, n, best = out[side]
            a, b, k = (tsrc.data_ptr(), tdst.data_ptr(), tmask.data_ptr()) if side == "device" else (ptr(src, C.c_float), ptr(dst, C.c_float), ptr(mask, C.c_uint8))
            t0 = time.perf_counter()
            rc = (dev_call if side == "device" else host_call)(ctx.h, a, b, ptr(moff, C.c_int64), P, THRESHOLD, n_hyp, 0, 2, ptr(M, C.c_double), k,
                                                               ptr(n, C.c_int64), ptr(best, C.c_int32))
            wall = 1e3 * (time.perf_counter() - t0)
            if rc != 0:
                sys.exit(f"verify_bench: the {side} form failed: {ctx.L.dlco_desc_last_error(ctx.h).decode()}")
            return wall, ctx.last_kernel_ms()

        def compare():
            (Md, _, nd, bd), (Mh, kh, nh, bh) = out["device"], out["host"]
            if not (Md.tobytes() == Mh.tobytes() and tmask.cpu().numpy().tobytes() == kh.tobytes() and nd.tobytes() == nh.tobytes() and bd.tobytes() == bh.tobytes()):
                sys.exit("verify_bench: the device form's answer differs from the host form's")

        run("device"), run("host")                             # the warm-up of each side, and the comparison
        compare()
        d, h = [], []
        for _ in range(3):
            d.append(run("device"))
            h.append(run("host"))
        compare()
        (dw, dk), (hw, hk) = (np.array(x).T for x in (d, h))
        row = lambda a: f"{a.min():.3f} ms ({a.min():.3f} .. {a.max():.3f})"
        print(f"| {P} | {m} | {n_hyp} | {row(dk)} | {row(hk)} | {row(dw)} | {row(hw)} | {hw.min() / dw.min():.1f}x | {int(out['host'][2].sum())} of {P * m} |")
        faster = faster and dw.max() < hw.min()
    print("the device form's slowest wall time is below the host form's fastest on every workload" if faster
          else "the device form did NOT beat the host form by more than the spread")
    ctx.close()


if PAIRS:
    device_bench() if DEVICE else pairs_bench()
    sys.exit(0)

ctx = dlco.DescContext()
rng = np.random.default_rng(0)
hypotheses, model = (ctx.verify_fundamental_hypotheses, ctx.verify_fundamental) if FUNDAMENTAL else (ctx.verify_hypotheses, ctx.verify_homography)
names = ("verify_fundamental_hypotheses", "verify_fundamental") if FUNDAMENTAL else ("verify_hypotheses", "verify_homography")
print(f"{reps} timed calls per row, medians; floor = {OPS_PER_PAIR:.0f} m n_hyp / {OPS_PER_SECOND:.3g} fp64 operations a second")
print(f"| m | n_hyp | {names[0]} kernels | instruction floor | torch float64 | {names[1]} kernels (refine 2) | inliers |")
print("|---|---|---|---|---|---|---|")
for m, n_hyp in ((2000, 2048), (20000, 4096), (100000, 4096)):
    src, dst = (two_cameras if FUNDAMENTAL else planted)(m, rng)
    for _ in range(3):
        H_all, count = hypotheses(src, dst, THRESHOLD, n_hyp, 0)
    ms = []
    for _ in range(reps):
        hypotheses(src, dst, THRESHOLD, n_hyp, 0)
        ms.append(ctx.last_kernel_ms())
    full = []
    for _ in range(reps):
        H, mask, best = model(src, dst, THRESHOLD, n_hyp, 0, 2)
        full.append(ctx.last_kernel_ms())
    floor_ms = 1e3 * OPS_PER_PAIR * m * n_hyp / OPS_PER_SECOND
    tc, t_ms = torch_counts(H_all, src, dst, THRESHOLD * THRESHOLD)
    print(f"| {m} | {n_hyp} | {np.median(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) | {floor_ms:.3f} ms | {t_ms:.2f} ms, {int((tc != count).sum())} counts differ "
          f"| {np.median(full):.3f} ms | {int(mask.sum())} of {m}, hypothesis {best} |")
    if FUNDAMENTAL and (tc != count).any():
        sys.exit(f"verify_bench: {int((tc != count).sum())} of torch's counts differ from the library's at m = {m}")
ctx.close()
