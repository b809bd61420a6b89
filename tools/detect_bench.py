"""Times the detector (dlco_desc_detect) by stage on keypoint_bench.py's synthetic 4096 x 3072 image, at 1 to 4 octaves and a
threshold that yields about 100 000 keypoints (found here by bisection on the 3-octave count).  Per stage (integral image,
responses and extrema of every octave, selection): the median kernel time of repeated calls (HIP events, through
detect_stage_ms / last_kernel_ms), the bytes the stage has to move and what those bytes cost at the rate a float4 copy
reaches on an MI355X's HBM (6.29 TB/s of the 8.0 TB/s on the data sheet).  "Must move" is the least any implementation
moves (the image in and S out; S in once per octave; the survivors in and the kept rows out), not what these kernels move.
Then the detector's time as a share of describe_keypoints on the keypoints it found: the comparison DESIGN 3b uses for the sampling kernel.  One process, three warm-up calls per shape, then `reps` timed calls; the
integral image is timed by setting the image anew before every call.  No gate: it prints what it measured."""
import importlib, os, sys
import numpy as np
import torch                                                # before libdlco.so: one HIP runtime per process, torch's first
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
dlco = importlib.import_module("opencv-dlco_amd")

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
target = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
W, H, nsel, r = 4096, 3072, 68, 64
HBM = 6.29e12
rng = np.random.default_rng(0)
img = rng.integers(0, 256, (H, W), dtype=np.uint8)
ctx = dlco.DescContext()
ctx.set_filters((rng.random((nsel, 4096)) < 0.05).astype(np.float32) * rng.random((nsel, 4096)).astype(np.float32) * 0.01)
ctx.set_projection((rng.standard_normal((r, nsel * 8)) / np.sqrt(nsel * 8)).astype(np.float32))
ctx.set_image(img)

# the threshold: the count falls as it rises
lo, hi = 1, 1 << 38
while lo < hi:
    mid = (lo + hi) // 2
    if ctx.detect(3, mid, 1)[2] > target:
        lo = mid + 1
    else:
        hi = mid
thr = lo
print(f"image {W} x {H}; threshold {thr} gives {ctx.detect(3, thr, 1)[2]} keypoints at 3 octaves, threshold 1 gives {ctx.detect(3, 1, 1)[2]}")


def grid(extent, o):
    m = (3 * (2 ** (o + 1) * 4 + 1) - 1) // 2
    return max(0, (extent - 1 - 2 * m) // 2 ** o + 1) if extent - 1 - 2 * m >= 0 else 0


S_bytes = 4 * (H + 1) * ((W + 4) // 4 * 4)
# integral image: the image in, S out (the kernels here move more: S is written by the row pass, read by the column sums, read
# and written by the column scan)
must = {"integral": W * H + S_bytes}
for o in range(4):
    # an octave reads the entries of S its filters touch at least once; a step above 1 still touches every 64-byte line
    must[f"octave {o}"] = S_bytes if grid(W, o) >= 3 and grid(H, o) >= 3 else 0


def med(v):
    return float(np.median(v))


for n_oct in (1, 2, 3, 4):
    for cap in (target, 1 << 22):
        for _ in range(3):
            ctx.detect(n_oct, thr, cap)
        rows, total, with_s = [], [], []
        for _ in range(reps):
            kp, resp, n_found = ctx.detect(n_oct, thr, cap)
            rows.append(ctx.detect_stage_ms())
            total.append(ctx.last_kernel_ms())
        for _ in range(reps):
            ctx.set_image(img)
            ctx.detect(n_oct, thr, cap)
            with_s.append(ctx.detect_stage_ms()["integral"])
        # selection: position and response of every survivor in, the kept rows in and out (the radix sorts move more)
        must["selection"] = n_found * 16 + len(kp) * (16 + 16 + 8)
        stage = {"integral": med(with_s), "selection": med([x["selection"] for x in rows])}
        for o in range(n_oct):
            stage[f"octave {o}"] = med([x["octaves"][o] for x in rows])
        print(f"{n_oct} octaves, max_keypoints {cap}: {n_found} found, {len(kp)} returned; kernels {med(total):.3f} ms with S cached "
              f"(min {min(total):.3f}, max {max(total):.3f}), {med(total) + stage['integral']:.3f} ms with the integral image")
        for name in ["integral"] + [f"octave {o}" for o in range(n_oct)] + ["selection"]:
            ms, b = stage[name], must[name]
            print(f"    {name:10s} {ms:8.3f} ms   must move {b / 1e6:8.1f} MB = {1e3 * b / HBM:6.3f} ms at 6.29 TB/s "
                  f"({100 * (1e3 * b / HBM) / ms if ms > 0 else 0:5.1f} % of that rate)")
    if n_oct == 3:
        kp, resp, n_found = ctx.detect(3, thr, 1 << 22)
        table = torch.empty((len(kp), r), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.describe_keypoints_device(kp[:2048], table.data_ptr())
        ms = []
        for _ in range(3):
            st = ctx.describe_keypoints_device(kp, table.data_ptr())
            ms.append(ctx.last_kernel_ms())
        det = med(total) + stage["integral"]
        print(f"    describe_keypoints of these {len(kp)} keypoints ({int((st == 2).sum())} wholly inside, scale factor 6.25): kernels "
              f"{med(ms):.2f} ms; the detector ({det:.3f} ms with the integral image) is {100 * det / med(ms):.2f} % of it")
ctx.close()
