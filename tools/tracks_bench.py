"""Times the two ways from verified match lists in HBM to multi-view tracks in HBM, on the two sets of the README: a, nine
images of 2048 rows, all 72 ordered pairs; b, 33 images of 512 rows, all 1056.  The images see synthetic world points, twice as
many as an image has rows, each image a random half of them in an order of its own: a pair's list holds four in five of the
points both see, a twentieth as many wrong matches, and a mask that keeps nine in ten of the true ones and a share `wrong` of
the wrong ones: 0.02, a verification that works, and 0.3, one that lets so much through that on set b nearly all keypoints hang
together in one component, the hardest case for the union-find.  The world points are the ground truth: a track is pure when
all its keypoints are one point.
  (A) download of matches (8 bytes a match) and mask (1 byte), the host union-find of csrc/track_rules.hpp (tracks_host,
      compiled with g++ -O2 for this run), upload of toff and obs: the caller's route without build_tracks_device.
  (B) build_tracks_device on the lists where they lie; only n_tracks and counts cross.
Per route the wall clock around it; for B also the kernels (last_kernel_ms).  One warm-up of both, then `rounds` (default 5)
rounds that alternate A and B; per figure the best round and the range.  The outputs of the two routes are compared for
equality and the run ends with an error when they differ.  No gate: it prints what it measured.

    tracks_bench.py [rounds]"""
import ctypes as C, importlib, os, subprocess, sys, tempfile, time
import numpy as np
import torch                                                # before libdlco.so: one HIP runtime per process, torch's first
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
dlco = importlib.import_module("opencv-dlco_amd")

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
i32p, i64p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)


def host_rule():
    """track_rules::tracks_host behind the C surface of the tests' shim"""
    out = os.path.join(tempfile.mkdtemp(prefix="tracks_bench_"), "libtrackrules.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, os.path.join(ROOT, "tests", "shim", "track_rules_shim.cpp")])
    L = C.CDLL(out)
    L.shim_track_build.argtypes = [i64p, C.c_int32, i32p, C.c_int64, i64p, i32p, u8p, C.c_int32, C.c_int32, i64p, i32p, i32p, i32p, i64p]
    L.shim_track_build.restype = C.c_int64
    return L


def lists(sizes, seed, wrong):
    rng = np.random.default_rng(seed)
    n_img, n = len(sizes), sizes[0]
    world = [rng.permutation(2 * n)[:s] for s in sizes]
    pairs = np.array([(a, b) for a in range(n_img) for b in range(n_img) if a != b], np.int32)
    ms, ks, moff = [], [], [0]
    for a, b in pairs:
        _, ia, ib = np.intersect1d(world[a], world[b], return_indices=True)
        sel = rng.random(len(ia)) < 0.8
        m = np.stack([ia[sel], ib[sel]], 1)
        k = rng.random(len(m)) < 0.9
        nw = len(ia) // 20
        m = np.concatenate([m, np.stack([rng.integers(0, sizes[a], nw), rng.integers(0, sizes[b], nw)], 1)])
        k = np.concatenate([k, rng.random(nw) < wrong])
        o = np.argsort(m[:, 0], kind="stable")
        ms.append(m[o].astype(np.int32)); ks.append(k[o].astype(np.uint8)); moff.append(moff[-1] + len(m))
    return pairs, np.array(moff, np.int64), np.ascontiguousarray(np.concatenate(ms)), np.ascontiguousarray(np.concatenate(ks)), np.concatenate(world)


def bench(ctx, L, name, sizes, wrong, unique=1):
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pairs, moff, m_h, k_h, world = lists(sizes, 5, wrong)
    N, M, P = int(seg[-1]), int(moff[-1]), len(pairs)
    p = lambda a, t: a.ctypes.data_as(t)
    dev = lambda n, t: torch.empty((n,), dtype=t, device="cuda:0")
    m, k = torch.from_numpy(m_h).to("cuda:0"), torch.from_numpy(k_h).to("cuda:0")
    toff, obs, track_of = dev(N // 2 + 1, torch.int64), dev(N, torch.int32), dev(N, torch.int32)
    toff_a, obs_a = dev(N // 2 + 1, torch.int64), dev(N, torch.int32)
    md, kd = np.empty((M, 2), np.int32), np.empty(M, np.uint8)
    toff_h, obs_h, track_of_h, counts_h = np.empty(N // 2 + 1, np.int64), np.empty(N, np.int32), np.empty(N, np.int32), np.empty(3, np.int64)
    torch.cuda.synchronize()

    def route_a():
        t0 = time.perf_counter()
        torch.from_numpy(md).copy_(m)
        torch.from_numpy(kd).copy_(k)
        T = L.shim_track_build(p(seg, i64p), len(sizes), p(pairs, i32p), P, p(moff, i64p), p(md, i32p), p(kd, u8p), 2, unique, p(toff_h, i64p), p(obs_h, i32p),
                               p(track_of_h, i32p), None, p(counts_h, i64p))
        K = int(toff_h[T])
        toff_a[:T + 1].copy_(torch.from_numpy(toff_h[:T + 1]))
        obs_a[:K].copy_(torch.from_numpy(obs_h[:K]))
        torch.cuda.synchronize()
        return (T, counts_h.copy()), 1e3 * (time.perf_counter() - t0), 9 * M + 8 * (T + 1) + 4 * K

    def route_b():
        t0 = time.perf_counter()
        T, counts = ctx.build_tracks_device(m.data_ptr(), moff, seg, pairs, toff.data_ptr(), obs.data_ptr(), track_of.data_ptr(), keep_ptr=k.data_ptr(),
                                            min_len=2, unique=bool(unique))
        t1 = time.perf_counter()
        return (T, counts), 1e3 * (t1 - t0), 32 + 24 * P + 8 * len(seg), ctx.last_kernel_ms()

    a, b = route_a(), route_b()
    T = a[0][0]
    K = int(toff_h[T])
    same = T == b[0][0] and a[0][1].tolist() == b[0][1].tolist() and toff.cpu().numpy()[:T + 1].tobytes() == toff_h[:T + 1].tobytes() and \
        obs.cpu().numpy()[:K].tobytes() == obs_h[:K].tobytes() and track_of.cpu().numpy().tobytes() == track_of_h.tobytes() and \
        toff_a.cpu().numpy()[:T + 1].tobytes() == toff_h[:T + 1].tobytes()
    if not same:
        sys.exit(f"tracks_bench: the two routes differ on set {name}, wrong {wrong}")
    w = world[obs_h[:K]]
    pure = sum(1 for t in range(T) if (w[toff_h[t]:toff_h[t + 1]] == w[toff_h[t]]).all())
    ra, rb = [], []
    for _ in range(rounds):
        ra.append(route_a()[1:])
        rb.append(route_b()[1:])
    col = lambda rows, i: np.array([r[i] for r in rows])
    fmt = lambda v: f"{v.min():.3f} ({v.min():.3f} .. {v.max():.3f})"
    c = a[0][1]
    head = f"| {name} | {wrong} | {P} | {N} | {M} | {T} ({pure} pure) | {K} | {c[0]} / {c[1]} / {c[2]} |"
    print(f"{head} A | - | {fmt(col(ra, 0))} | {ra[0][1]} |", flush=True)
    print(f"{head} B | {fmt(col(rb, 2))} | {fmt(col(rb, 0))} | {rb[0][1]} |", flush=True)


print(f"tracks_bench: min_len 2, unique 1, best of {rounds} alternating rounds (min .. max), milliseconds")
print("| set | wrong | pairs | N | M | tracks | observations | counts | route | kernels | wall | bytes moved |")
print("|---|---|---|---|---|---|---|---|---|---|---|---|")
ctx, L = dlco.DescContext(), host_rule()
for name, sizes in (("a", [2048] * 9), ("b", [512] * 33)):
    for wrong in (0.02, 0.3):
        bench(ctx, L, name, sizes, wrong)
ctx.close()
