"""Times the orientation kernel (dlco_desc_orient, through last_orient_ms: HIP events around the kernel alone) for 100 000
keypoints on keypoint_bench.py's synthetic 4096 x 3072 image, at the scales s = 1, 2, 4, 8 and 26 (sizes 7.5 s: the detector's
sizes 9 .. 195 give s = 1 .. 26), the keypoints uniformly inside the image so that nearly every sample is used.  Per scale: the
median kernel time of repeated calls, the time per keypoint, and the entries of S a keypoint's footprint holds,
(14 s + 2)^2, against the 109 x 16 corners it reads.  Then detect_oriented at a threshold that yields about 100 000
keypoints: the scales a detection really has, and the kernel's share of the call.  One process, three warm-up calls per
shape, then `reps` timed calls.  No gate: it prints what it measured."""
import importlib, os, sys
import numpy as np
import torch                                                # before libdlco.so: one HIP runtime per process, torch's first
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
dlco = importlib.import_module("opencv-dlco_amd")

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
n = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
W, H = 4096, 3072
rng = np.random.default_rng(0)
img = rng.integers(0, 256, (H, W), dtype=np.uint8)
ctx = dlco.DescContext()
ctx.set_image(img)


def med(v):
    return float(np.median(v))


print(f"image {W} x {H}, {n} keypoints per call, {reps} timed calls per row")
for s in (1, 2, 4, 8, 26):
    kp = np.empty((n, 4), np.float32)
    kp[:, 0], kp[:, 1] = rng.uniform(7 * s, W - 1 - 7 * s, n), rng.uniform(7 * s, H - 1 - 7 * s, n)
    kp[:, 2], kp[:, 3] = 7.5 * s, -1
    for _ in range(3):
        ang, vec, st = ctx.orient(kp)
    ms = []
    for _ in range(reps):
        ctx.orient(kp)
        ms.append(ctx.last_orient_ms())
    print(f"    s = {s:3d}: kernel {med(ms):8.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) = {1e3 * med(ms) / n:7.4f} us per keypoint; "
          f"footprint {(14 * s + 2) ** 2:6d} entries of S, {109 * 16} corners read; {int((st == 2).sum())} with all samples, "
          f"{int((ang >= 0).sum())} with an angle")

# a detection's own keypoints: the threshold by bisection on the 3-octave count, as tools/detect_bench.py does
lo, hi = 1, 1 << 38
while lo < hi:
    mid = (lo + hi) // 2
    if ctx.detect(3, mid, 1)[2] > n:
        lo = mid + 1
    else:
        hi = mid
for _ in range(3):
    kp, resp, n_found = ctx.detect_oriented(3, lo, 1 << 22)
o_ms, total = [], []
for _ in range(reps):
    ctx.detect_oriented(3, lo, 1 << 22)
    o_ms.append(ctx.last_orient_ms())
    total.append(ctx.last_kernel_ms())
scales = np.clip(np.floor(kp[:, 2].astype(np.float64) / 7.5 + 0.5), 1, 128).astype(int)
print(f"detect_oriented, 3 octaves, threshold {lo}: {len(kp)} keypoints, s = 1 .. {scales.max()} (median {int(np.median(scales))}); orientation "
      f"kernel {med(o_ms):.3f} ms = {1e3 * med(o_ms) / max(len(kp), 1):.4f} us per keypoint, {100 * med(o_ms) / med(total):.1f} % of the call's "
      f"{med(total):.3f} ms of kernels (S cached)")
ctx.close()
