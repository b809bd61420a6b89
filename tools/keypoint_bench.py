"""Times the front of the describe chain: the sampling kernel that cuts 64 x 64 patches out of an image in HBM, and
describe_keypoints (sampling + transform + pooling + projection, 16 bytes per keypoint on the way up) against describe on the
same patches ready on the host (4 KiB per patch on the way up).  A synthetic 4096 x 3072 image, 100 000 keypoints with
uniform centres and angles, at s = 0.4, 1, 2 and 5 source pixels per patch pixel (s <= 2 is staged in LDS, s = 5 gathers from
global memory).  Kernel times are HIP events through last_kernel_ms, wall times a host clock around the whole call; one
process, one warm-up call per shape, two timed repeats each, the smaller one reported.  No gate: it prints what it measured."""
import importlib, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
dlco = importlib.import_module("opencv-dlco_amd")
import torch

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
W, H, nsel, r = 4096, 3072, 68, 64
rng = np.random.default_rng(0)
img = rng.integers(0, 256, (H, W), dtype=np.uint8)
ctx = dlco.DescContext()
ctx.set_filters((rng.random((nsel, 4096)) < 0.05).astype(np.float32) * rng.random((nsel, 4096)).astype(np.float32) * 0.01)
ctx.set_projection((rng.standard_normal((r, nsel * 8)) / np.sqrt(nsel * 8)).astype(np.float32))
ctx.set_image(img)
table = torch.empty((n, r), dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()


def timed(fn):
    """(wall ms, kernel ms) of the faster of two calls"""
    out = []
    for _ in range(2):
        t0 = time.perf_counter()
        fn()
        out.append((1e3 * (time.perf_counter() - t0), ctx.last_kernel_ms()))
    return min(out)


for s in (0.4, 1.0, 2.0, 5.0):
    kp = np.stack([rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n), np.full(n, 64 * s), rng.uniform(0, 360, n)], axis=1).astype(np.float32)
    patches, status = ctx.extract_patches(kp[:2048], scale_factor=1.0)
    ctx.describe_keypoints_device(kp[:2048], table.data_ptr(), scale_factor=1.0)
    ctx.describe_device(patches, table.data_ptr())
    held = {}
    ex_wall, ex_ms = timed(lambda: held.update(p=ctx.extract_patches(kp, scale_factor=1.0)))
    patches, status = held["p"]
    kp_wall, kp_ms = timed(lambda: ctx.describe_keypoints_device(kp, table.data_ptr(), scale_factor=1.0))
    pt_wall, pt_ms = timed(lambda: ctx.describe_device(patches, table.data_ptr()))
    print(f"s {s}: {n} keypoints ({int((status == 2).sum())} wholly inside): sampling {1e3 * ex_ms / n:.3f} us/patch "
          f"(extract_patches wall {ex_wall:.1f} ms incl. {n * 4096 / 1e6:.0f} MB to the host); "
          f"describe_keypoints kernels {kp_ms:.2f} ms = {1e3 * kp_ms / n:.3f} us/patch, wall {kp_wall:.1f} ms; "
          f"describe on host patches kernels {pt_ms:.2f} ms = {1e3 * pt_ms / n:.3f} us/patch, wall {pt_wall:.1f} ms; "
          f"sampling is {100 * ex_ms / pt_ms:.1f} % of the rest of the chain")
ctx.close()
