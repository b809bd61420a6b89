"""Times the learnt descriptor (describe = transform + pooling + projection by W) against compute (transform + pooling, the
baseline) on resident patches, and pair_stats on a raw pair set: HIP events through last_kernel_ms, one process, one warm-up
call per shape, two timed repeats each.  Prints one line per shape with microseconds per patch and the share the projection
adds, beside the share of the flops (r / 4096)."""
import importlib, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
dlco = importlib.import_module("opencv-dlco_amd")
import torch

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
n_pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
rng = np.random.default_rng(0)
patches = rng.integers(0, 256, (n, 64, 64)).astype(np.uint8)
ctx = dlco.DescContext()
for nsel, r in ((68, 64), (1024, 128)):
    F = nsel * 8
    flt = (rng.random((nsel, 4096)) < 0.05).astype(np.float32) * rng.random((nsel, 4096)).astype(np.float32) * 0.01
    W = (rng.standard_normal((r, F)) / np.sqrt(F)).astype(np.float32)
    ctx.set_filters(flt)
    ctx.set_projection(W)
    table = torch.empty((n, F), dtype=torch.float32, device="cuda:0")
    proj = torch.empty((n, r), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.compute_device(patches[:2048], table.data_ptr())
    ctx.describe_device(patches[:2048], proj.data_ptr())
    comp, desc = [], []
    for _ in range(2):
        ctx.compute_device(patches, table.data_ptr())
        comp.append(ctx.last_kernel_ms())
        ctx.describe_device(patches, proj.data_ptr())
        desc.append(ctx.last_kernel_ms())
    c, d = min(comp), min(desc)
    print(f"nsel {nsel} r {r}, {n} patches: compute {1e3*c/n:.3f} us/patch (repeats {comp[0]:.2f} {comp[1]:.2f} ms), "
          f"describe {1e3*d/n:.3f} us/patch (repeats {desc[0]:.2f} {desc[1]:.2f} ms): +{100*(d/c-1):.2f} % "
          f"against {100*r/4096:.2f} % of the flops")
    if nsel == 68:
        pairs = np.stack([rng.integers(0, n, n_pairs), rng.integers(0, 50, n_pairs), rng.integers(0, n, n_pairs), rng.integers(0, 50, n_pairs)], 1).astype(np.int32)
        ctx.pair_stats(patches[:2048], pairs % np.array([2048, 1 << 30, 2048, 1 << 30], np.int32))
        walls = []
        for _ in range(2):
            t0 = time.time()
            dim, f95, auc = ctx.pair_stats(patches, pairs)
            walls.append(time.time() - t0)
        print(f"pair_stats: {n} patches, {n_pairs} pairs at nsel {nsel} r {r}: kernels (describe + pair distances) {ctx.last_kernel_ms():.2f} ms, "
              f"wall incl. upload, sort and scans {1e3*walls[0]:.1f} {1e3*walls[1]:.1f} ms; dim {dim} fpr95 {f95:.4f} auc {auc:.4f}")
    del table, proj
ctx.close()
