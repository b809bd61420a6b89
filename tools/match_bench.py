"""Times dlco_desc_match_device on tables resident in HBM: HIP events through last_kernel_ms (norms, tile loop and the merge of
the slices), one process, one warm-up call per shape, two timed repeats.  Prints one line per shape with milliseconds per
call, the floor 2 nq nt r / 78.6 TFLOP/s (the f64 MFMA peak DESIGN prices desc_pool_kernel against) and their ratio, and, as
the thing a user would write without this call, the time of a chunked float64 torch Q @ T.T + topk(2) on the same tables
(torch events, same warm-up and repeats).

With --u8 the same tables are quantised to bytes (one scale, per-dimension offsets fitted on both, as dlco_desc_quant_fit
does) and dlco_desc_match_u8_device is timed the same way; the line shows the float call's time of the same shape from the
same run beside it, the int8 MFMA floor 2 nq nt r / 5.0 POP/s (twice the dense BF16 peak of 2.5 PF) and the share of it.

With --guided the rows get keypoints, uniform in a square of side 8 sqrt(nt) (one per 64 px^2), a mild homography and radius
12 (about seven admitted train rows a query), and dlco_desc_match_guided_device is timed for both h_side beside the plain
call: one warm-up each, then three rounds that alternate plain, h_side 0, h_side 1.  The line shows the three times, the
guided calls' ratio to the plain one and their share of the f64 MFMA floor, and how many queries found two admitted rows.

With --guided-epipolar the same keypoints get, beside that homography H, the fundamental matrix F = [e']x H with the epipole
e' = (3 S, 0.4 S, 1), S the side of the square, divided by its largest magnitude, and the threshold 2 of the tests:
dlco_desc_match_guided_epipolar_device is timed for both f_side beside the plain call and the homography-guided call of the
same run, one warm-up each, then three rounds that alternate the five calls.  The line shows the five times with their rounds,
the epipolar calls' ratio to the plain call and to the homography-guided call of the same side, and how many queries found two
admitted rows.

With --pairs (and --u8 for the byte line) the batched call is measured instead: dlco_desc_match_pairs_device on a set of images
in one table in HBM against a loop of dlco_desc_match_device calls over the same pairs on the same sub-tables, the thing the
batch replaces.  The sets: a, 9 images of 2048 rows, all 72 ordered pairs (also at r = 64); b, 33 x 512 rows, all 1056; c,
4 x 8192 rows, all 12; d, 20 images of 500 .. 8000 rows (seeded), all 380; r = 128 unless said.  One warm-up of both, then
three rounds that alternate the batch and the loop in one process.  For each the kernel time (last_kernel_ms, summed over the
loop's calls) and the wall time from sync to sync; the figure is the best of the three rounds, the loop's spread its largest
minus its smallest round.  The line adds the floor 2 sum(nq nt) r / 78.6 TFLOP/s (5.0 POP/s with --u8), the batch's share of
it, and whether the two routes returned the same bytes.

With --pairs --guided (--pairs --guided-epipolar) the guided batch is measured: dlco_desc_match_pairs_guided_device (_epipolar)
on sets a and b at r = 128 against a loop of dlco_desc_match_guided_device (_epipolar) calls over the same pairs, with the plain
batch of the same run beside both.  The keypoints are those of --guided, uniform in a square of side 8 sqrt(n) per image; every
pair has a matrix of its own, the mild homography of --guided (the F of --guided-epipolar) behind a shift of up to 2 px that
depends on the pair; radius 12, threshold 2; both sides.  One warm-up of the three, a check that the batch and the loop returned
the same bytes (the tool stops if they did not), then three rounds that alternate them.  The line shows kernels and wall of
each with their rounds, loop / batch, guided batch / plain batch, and the gate: the batch's slowest round below the loop's
fastest.

With --u8 --guided (--u8 --guided-epipolar) the byte line's guided call is measured: dlco_desc_match_guided_u8_device
(_epipolar_u8_device) on the geometry of --guided (--guided-epipolar) and the float tables quantised with one fitted scale, as
--u8 does.  One process alternates the plain byte call, the byte guided call of both sides and the float guided call of both
sides on the same shape: one warm-up each, three rounds, kernel time from last_kernel_ms.  The line shows the best round of
each with the three rounds' range (largest minus smallest), byte guided / plain byte and float guided / byte guided, and how
many queries found two admitted rows.  With --u8 --pairs --guided (--u8 --pairs --guided-epipolar) the same five calls are
the batches dlco_desc_match_pairs_u8_device, dlco_desc_match_pairs_guided_u8_device (_epipolar_u8_device) and the float guided
batch on the sets a (72 pairs) and b (1056 pairs) of --pairs --guided, with a matrix of its own per pair."""
import importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
dlco = importlib.import_module("opencv-dlco_amd")

PEAK = 78.6e12
PEAK_I8 = 5.0e15
U8 = "--u8" in sys.argv
if U8:
    sys.argv.remove("--u8")
GUIDED = "--guided" in sys.argv
if GUIDED:
    sys.argv.remove("--guided")
EPI = "--guided-epipolar" in sys.argv
if EPI:
    sys.argv.remove("--guided-epipolar")
PAIRS = "--pairs" in sys.argv
if PAIRS:
    sys.argv.remove("--pairs")
SHAPES = [(2048, 2048, 64), (8192, 8192, 64), (8192, 8192, 128), (100000, 100000, 128)]
if len(sys.argv) > 1:
    SHAPES = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]]


def torch_route(Q, T, chunk=8192):
    """Nearest two by a float64 product, a chunk of queries at a time so that the nq x nt matrix never exists whole."""
    T64 = T.double()
    tn = (T64 * T64).sum(1)
    idx, d = [], []
    for i0 in range(0, Q.shape[0], chunk):
        q = Q[i0:i0 + chunk].double()
        D = ((q * q).sum(1)[:, None] + tn[None, :] - 2.0 * (q @ T64.T)).clamp_(min=0)
        v, j = torch.topk(D, min(2, T.shape[0]), dim=1, largest=False)
        idx.append(j)
        d.append(v.float())
    return torch.cat(idx), torch.cat(d)


def pairs_bench():
    import time
    import numpy as np
    rng = np.random.default_rng(4)
    sets = [("a", [2048] * 9, 128), ("a", [2048] * 9, 64), ("b", [512] * 33, 128), ("c", [8192] * 4, 128),
            ("d", [int(v) for v in rng.integers(500, 8001, 20)], 128)]
    ctx = dlco.DescContext()
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    peak, unit = (PEAK_I8, "int8") if U8 else (PEAK, "f64")
    for name, sizes, r in sets:
        n_img = len(sizes)
        seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        pairs = np.array([(a, b) for a in range(n_img) for b in range(n_img) if a != b], np.int32)
        row0 = dlco.match_pairs_rows(seg, pairs)
        X = torch.empty((int(seg[-1]), r), dtype=torch.float32, device="cuda:0").normal_(0, 0.25, generator=gen)
        if U8:
            lo = X.min(0).values
            X = ((X - lo) * (255.0 / float((X.max(0).values - lo).max()))).round().clamp(0, 255).to(torch.uint8)
        esz, ddt = X.element_size(), (torch.int32 if U8 else torch.float32)
        out = [(torch.empty((int(row0[-1]), 2), dtype=torch.int32, device="cuda:0"), torch.empty((int(row0[-1]), 2), dtype=ddt, device="cuda:0"))
               for _ in range(2)]
        torch.cuda.synchronize()
        one = ctx.match_u8_device if U8 else ctx.match_device
        many = ctx.match_pairs_u8_device if U8 else ctx.match_pairs_device

        def batch():
            many(X.data_ptr(), seg, pairs, r, out[0][0].data_ptr(), out[0][1].data_ptr(), ld=r)
            return ctx.last_kernel_ms()

        def loop():
            ms = 0.0
            for p, (a, b) in enumerate(pairs):
                one(X.data_ptr() + int(seg[a]) * r * esz, sizes[a], X.data_ptr() + int(seg[b]) * r * esz, sizes[b], r,
                    out[1][0].data_ptr() + int(row0[p]) * 8, out[1][1].data_ptr() + int(row0[p]) * 8)
                ms += ctx.last_kernel_ms()
            return ms

        def timed(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ms = f()
            torch.cuda.synchronize()
            return ms, 1e3 * (time.perf_counter() - t0)

        batch()
        loop()
        same = bool(torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32)))
        rounds = [(timed(batch), timed(loop)) for _ in range(3)]
        bk, bw = min(x[0][0] for x in rounds), min(x[0][1] for x in rounds)
        lk, lw = [x[1][0] for x in rounds], [x[1][1] for x in rounds]
        floor = 1e3 * 2.0 * float(sum(sizes[a] * sizes[b] for a, b in pairs)) * r / peak
        sl = ctx.match_pairs_slices(seg, pairs, u8=U8)
        fmt = lambda m: " ".join("%.3f" % v for v in m)
        print(f"match_pairs{'_u8' if U8 else ''} set {name}: {n_img} images of {min(sizes)}..{max(sizes)} rows, {len(pairs)} pairs, r {r}, slices "
              f"{int(sl.min())}..{int(sl.max())}: batch kernels {bk:.3f} ms (rounds {fmt(x[0][0] for x in rounds)}), wall {bw:.3f} ms (rounds "
              f"{fmt(x[0][1] for x in rounds)}); loop kernels {min(lk):.3f} ms (rounds {fmt(lk)}, spread {max(lk) - min(lk):.3f}), wall {min(lw):.3f} ms "
              f"(rounds {fmt(lw)}, spread {max(lw) - min(lw):.3f}); loop / batch kernels {min(lk) / bk:.2f}, wall {min(lw) / bw:.2f}; {unit} MFMA floor "
              f"{floor:.3f} ms, share of the floor: batch {floor / bk:.3f}, loop {floor / min(lk):.3f}; same bytes: {same}; batch not slower within the "
              f"loop's spread: kernels {bk <= min(lk) + (max(lk) - min(lk))}, wall {bw <= min(lw) + (max(lw) - min(lw))}", flush=True)
        del X, out
    ctx.close()


def pairs_guided_bench():
    import time
    import numpy as np
    sets = [("a", [2048] * 9, 128), ("b", [512] * 33, 128)]
    ctx = dlco.DescContext()
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    name_of = "match_pairs_guided_epipolar" if EPI else "match_pairs_guided"
    for name, sizes, r in sets:
        n_img, n = len(sizes), sizes[0]
        seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        pairs = np.array([(a, b) for a in range(n_img) for b in range(n_img) if a != b], np.int32)
        row0 = dlco.match_pairs_rows(seg, pairs)
        X = torch.empty((int(seg[-1]), r), dtype=torch.float32, device="cuda:0").normal_(0, 0.25, generator=gen)
        S = 8.0 * n ** 0.5
        xy = torch.rand((int(seg[-1]), 2), device="cuda:0", generator=gen) * S
        H = np.array([[0.98, -0.05, 0.03 * S], [0.04, 1.02, -0.02 * S], [0.02 / S, -0.01 / S, 1.0]])
        M = []
        for p in range(len(pairs)):                        # a matrix per pair: the model behind a small shift of the source image
            m = H @ np.array([[1.0, 0.0, 2.0 * np.cos(p)], [0.0, 1.0, 2.0 * np.sin(p)], [0.0, 0.0, 1.0]])
            if EPI:
                m = np.array([[0.0, -1.0, 0.4 * S], [1.0, 0.0, -3.0 * S], [-0.4 * S, 3.0 * S, 0.0]]) @ m
                m = m / np.abs(m).max()
            M.append(m)
        M = np.stack(M)
        t = 2.0 if EPI else 12.0
        out = [(torch.empty((int(row0[-1]), 2), dtype=torch.int32, device="cuda:0"), torch.empty((int(row0[-1]), 2), dtype=torch.float32, device="cuda:0"))
               for _ in range(3)]
        torch.cuda.synchronize()
        many = ctx.match_pairs_guided_epipolar_device if EPI else ctx.match_pairs_guided_device
        one = ctx.match_guided_epipolar_device if EPI else ctx.match_guided_device
        for side in (0, 1):
            def batch():
                many(X.data_ptr(), xy.data_ptr(), seg, pairs, r, M, out[0][0].data_ptr(), out[0][1].data_ptr(), t, side, ld=r, ldxy=2)
                return ctx.last_kernel_ms()

            def loop():
                ms = 0.0
                for p, (a, b) in enumerate(pairs):
                    one(X.data_ptr() + int(seg[a]) * r * 4, xy.data_ptr() + int(seg[a]) * 8, sizes[a], X.data_ptr() + int(seg[b]) * r * 4,
                        xy.data_ptr() + int(seg[b]) * 8, sizes[b], r, M[p], out[1][0].data_ptr() + int(row0[p]) * 8, out[1][1].data_ptr() + int(row0[p]) * 8,
                        t, side)
                    ms += ctx.last_kernel_ms()
                return ms

            def plain():
                ctx.match_pairs_device(X.data_ptr(), seg, pairs, r, out[2][0].data_ptr(), out[2][1].data_ptr(), ld=r)
                return ctx.last_kernel_ms()

            def timed(f):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ms = f()
                torch.cuda.synchronize()
                return ms, 1e3 * (time.perf_counter() - t0)

            batch(), loop(), plain()
            torch.cuda.synchronize()
            same = bool(torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32)))
            if not same:
                sys.exit(f"{name_of} set {name} side {side}: the batch and the loop of single calls returned different bytes")
            two = 100 * float((out[0][0][:, 1] >= 0).float().mean())
            rounds = [(timed(batch), timed(loop), timed(plain)) for _ in range(3)]
            col = lambda k, w: [x[k][w] for x in rounds]
            fmt = lambda m: " ".join("%.3f" % v for v in m)
            bk, bw, lk, lw, pk, pw = col(0, 0), col(0, 1), col(1, 0), col(1, 1), col(2, 0), col(2, 1)
            print(f"{name_of} set {name}: {n_img} images of {n} rows, {len(pairs)} pairs, r {r}, side {side}: batch kernels {min(bk):.3f} ms (rounds "
                  f"{fmt(bk)}), wall {min(bw):.3f} ms (rounds {fmt(bw)}); loop kernels {min(lk):.3f} ms (rounds {fmt(lk)}), wall {min(lw):.3f} ms (rounds "
                  f"{fmt(lw)}); plain batch kernels {min(pk):.3f} ms (rounds {fmt(pk)}), wall {min(pw):.3f} ms (rounds {fmt(pw)}); loop / batch kernels "
                  f"{min(lk) / min(bk):.2f}, wall {min(lw) / min(bw):.2f}; guided batch / plain batch kernels {min(bk) / min(pk):.3f}; same bytes: {same}; "
                  f"two admitted rows for {two:.1f} % of the queries; the batch's slowest round below the loop's fastest: kernels {max(bk) < min(lk)}, "
                  f"wall {max(bw) < min(lw)}", flush=True)
        del X, xy, out
    ctx.close()


def quantised(X, lo, scale, r):
    """the float rows as bytes at a pitch of whole 16-byte pieces: one scale, per-dimension offsets"""
    ld = (r + 15) // 16 * 16
    B = torch.zeros((len(X), ld), dtype=torch.uint8, device="cuda:0")
    B[:, :r] = ((X - lo) * scale).round().clamp(0, 255).to(torch.uint8)
    return B, ld


def rounds_line(names, calls, ctx):
    """one warm-up of every call, then three rounds that alternate them: (best [k], range [k], text)"""
    for f in calls:
        f()
    ms3 = [[] for _ in calls]
    for _ in range(3):
        for k, f in enumerate(calls):
            f()
            ms3[k].append(ctx.last_kernel_ms())
    best, rng = [min(m) for m in ms3], [max(m) - min(m) for m in ms3]
    text = ", ".join("%s %.3f ms (rounds %s, range %.3f)" % (n, b, " ".join("%.3f" % v for v in m), g) for n, b, m, g in zip(names, best, ms3, rng))
    return best, rng, text


def u8_guided_bench():
    import numpy as np
    ctx = dlco.DescContext()
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    what = "match_guided_epipolar_u8" if EPI else "match_guided_u8"
    for nq, nt, r in SHAPES:
        T = torch.empty((nt, r), dtype=torch.float32, device="cuda:0").normal_(0, 0.25, generator=gen)
        Q = torch.empty((nq, r), dtype=torch.float32, device="cuda:0").normal_(0, 0.25, generator=gen)
        Q[: nq // 2] = T[torch.randint(0, nt, (nq // 2,), device="cuda:0", generator=gen)] + 0.02 * torch.randn((nq // 2, r), device="cuda:0", generator=gen)
        S = 8.0 * nt ** 0.5
        M = np.array([[0.98, -0.05, 0.03 * S], [0.04, 1.02, -0.02 * S], [0.02 / S, -0.01 / S, 1.0]])
        if EPI:
            M = np.array([[0.0, -1.0, 0.4 * S], [1.0, 0.0, -3.0 * S], [-0.4 * S, 3.0 * S, 0.0]]) @ M
            M = M / np.abs(M).max()
        t = 2.0 if EPI else 12.0
        txy = torch.rand((nt, 2), device="cuda:0", generator=gen) * S
        qxy = torch.rand((nq, 2), device="cuda:0", generator=gen) * S
        lo = torch.minimum(Q.min(0).values, T.min(0).values)
        scale = 255.0 / float(torch.maximum(Q.max(0).values, T.max(0).values).sub(lo).max())
        (Qu, ld), (Tu, _) = quantised(Q, lo, scale, r), quantised(T, lo, scale, r)
        oi = [torch.empty((nq, 2), dtype=torch.int32, device="cuda:0") for _ in range(5)]
        od = [torch.empty((nq, 2), dtype=torch.int32, device="cuda:0") for _ in range(3)] + [torch.empty((nq, 2), dtype=torch.float32, device="cuda:0") for _ in range(2)]
        torch.cuda.synchronize()
        g8 = ctx.match_guided_epipolar_u8_device if EPI else ctx.match_guided_u8_device
        gf = ctx.match_guided_epipolar_device if EPI else ctx.match_guided_device
        calls = [lambda: ctx.match_u8_device(Qu.data_ptr(), nq, Tu.data_ptr(), nt, r, oi[0].data_ptr(), od[0].data_ptr(), ldq=ld, ldt=ld)]
        calls += [lambda h=h: g8(Qu.data_ptr(), qxy.data_ptr(), nq, Tu.data_ptr(), txy.data_ptr(), nt, r, M, oi[1 + h].data_ptr(), od[1 + h].data_ptr(), t, h,
                                 ldq=ld, ldt=ld) for h in (0, 1)]
        calls += [lambda h=h: gf(Q.data_ptr(), qxy.data_ptr(), nq, T.data_ptr(), txy.data_ptr(), nt, r, M, oi[3 + h].data_ptr(), od[3 + h].data_ptr(), t, h)
                  for h in (0, 1)]
        best, _, text = rounds_line(["plain byte", "byte guided side 0", "byte guided side 1", "float guided side 0", "float guided side 1"], calls, ctx)
        two = [100 * float((oi[k][:, 1] >= 0).float().mean()) for k in (1, 2)]
        print(f"{what} {nq} x {nt} r {r}: {text}; byte guided / plain byte {best[1] / best[0]:.3f} and {best[2] / best[0]:.3f}; float guided / byte guided "
              f"{best[3] / best[1]:.3f} and {best[4] / best[2]:.3f}; two admitted rows for {two[0]:.1f} % and {two[1]:.1f} % of the queries", flush=True)
        del T, Q, Qu, Tu, txy, qxy, oi, od
    ctx.close()


def pairs_u8_guided_bench():
    import numpy as np
    sets = [("a", [2048] * 9, 128), ("b", [512] * 33, 128)]
    ctx = dlco.DescContext()
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    what = "match_pairs_guided_epipolar_u8" if EPI else "match_pairs_guided_u8"
    for name, sizes, r in sets:
        n_img, n = len(sizes), sizes[0]
        seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        pairs = np.array([(a, b) for a in range(n_img) for b in range(n_img) if a != b], np.int32)
        rows = int(dlco.match_pairs_rows(seg, pairs)[-1])
        X = torch.empty((int(seg[-1]), r), dtype=torch.float32, device="cuda:0").normal_(0, 0.25, generator=gen)
        S = 8.0 * n ** 0.5
        xy = torch.rand((int(seg[-1]), 2), device="cuda:0", generator=gen) * S
        H = np.array([[0.98, -0.05, 0.03 * S], [0.04, 1.02, -0.02 * S], [0.02 / S, -0.01 / S, 1.0]])
        M = []
        for p in range(len(pairs)):                        # a matrix per pair: the model behind a small shift of the source image
            m = H @ np.array([[1.0, 0.0, 2.0 * np.cos(p)], [0.0, 1.0, 2.0 * np.sin(p)], [0.0, 0.0, 1.0]])
            if EPI:
                m = np.array([[0.0, -1.0, 0.4 * S], [1.0, 0.0, -3.0 * S], [-0.4 * S, 3.0 * S, 0.0]]) @ m
                m = m / np.abs(m).max()
            M.append(m)
        M = np.stack(M)
        t = 2.0 if EPI else 12.0
        lo = X.min(0).values
        Xu, ld = quantised(X, lo, 255.0 / float((X.max(0).values - lo).max()), r)
        oi = [torch.empty((rows, 2), dtype=torch.int32, device="cuda:0") for _ in range(5)]
        od = [torch.empty((rows, 2), dtype=torch.int32, device="cuda:0") for _ in range(3)] + [torch.empty((rows, 2), dtype=torch.float32, device="cuda:0") for _ in range(2)]
        torch.cuda.synchronize()
        g8 = ctx.match_pairs_guided_epipolar_u8_device if EPI else ctx.match_pairs_guided_u8_device
        gf = ctx.match_pairs_guided_epipolar_device if EPI else ctx.match_pairs_guided_device
        calls = [lambda: ctx.match_pairs_u8_device(Xu.data_ptr(), seg, pairs, r, oi[0].data_ptr(), od[0].data_ptr(), ld=ld)]
        calls += [lambda h=h: g8(Xu.data_ptr(), xy.data_ptr(), seg, pairs, r, M, oi[1 + h].data_ptr(), od[1 + h].data_ptr(), t, h, ld=ld, ldxy=2) for h in (0, 1)]
        calls += [lambda h=h: gf(X.data_ptr(), xy.data_ptr(), seg, pairs, r, M, oi[3 + h].data_ptr(), od[3 + h].data_ptr(), t, h, ld=r, ldxy=2) for h in (0, 1)]
        best, _, text = rounds_line(["plain byte batch", "byte guided batch side 0", "byte guided batch side 1", "float guided batch side 0",
                                     "float guided batch side 1"], calls, ctx)
        two = [100 * float((oi[k][:, 1] >= 0).float().mean()) for k in (1, 2)]
        print(f"{what} set {name}: {n_img} images of {n} rows, {len(pairs)} pairs, r {r}: {text}; byte guided / plain byte {best[1] / best[0]:.3f} and "
              f"{best[2] / best[0]:.3f}; float guided / byte guided {best[3] / best[1]:.3f} and {best[4] / best[2]:.3f}; two admitted rows for {two[0]:.1f} % "
              f"and {two[1]:.1f} % of the queries", flush=True)
        del X, Xu, xy, oi, od
    ctx.close()


if U8 and (GUIDED or EPI):
    if PAIRS:
        pairs_u8_guided_bench()
    else:
        u8_guided_bench()
    sys.exit(0)

if PAIRS:
    if GUIDED or EPI:
        pairs_guided_bench()
    else:
        pairs_bench()
    sys.exit(0)

ctx = dlco.DescContext()
gen = torch.Generator(device="cuda:0").manual_seed(0)
for nq, nt, r in SHAPES:
    T = torch.empty((nt, r), dtype=torch.float32, device="cuda:0").normal_(0, 0.25, generator=gen)
    Q = torch.empty((nq, r), dtype=torch.float32, device="cuda:0").normal_(0, 0.25, generator=gen)
    Q[: nq // 2] = T[torch.randint(0, nt, (nq // 2,), device="cuda:0", generator=gen)] + 0.02 * torch.randn((nq // 2, r), device="cuda:0", generator=gen)
    idx = torch.empty((nq, 2), dtype=torch.int32, device="cuda:0")
    d = torch.empty((nq, 2), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    call = lambda: ctx.match_device(Q.data_ptr(), nq, T.data_ptr(), nt, r, idx.data_ptr(), d.data_ptr())
    if GUIDED or EPI:
        import numpy as np
        S = 8.0 * nt ** 0.5
        H = np.array([[0.98, -0.05, 0.03 * S], [0.04, 1.02, -0.02 * S], [0.02 / S, -0.01 / S, 1.0]])
        txy = torch.rand((nt, 2), device="cuda:0", generator=gen) * S
        qxy = torch.rand((nq, 2), device="cuda:0", generator=gen) * S
        gi = [torch.empty((nq, 2), dtype=torch.int32, device="cuda:0") for _ in range(2)]
        gd = [torch.empty((nq, 2), dtype=torch.float32, device="cuda:0") for _ in range(2)]
        torch.cuda.synchronize()
        calls = [call] + [lambda h=h: ctx.match_guided_device(Q.data_ptr(), qxy.data_ptr(), nq, T.data_ptr(), txy.data_ptr(), nt, r, H, gi[h].data_ptr(),
                                                              gd[h].data_ptr(), radius=12.0, h_side=h) for h in (0, 1)]
        if EPI:
            F = np.array([[0.0, -1.0, 0.4 * S], [1.0, 0.0, -3.0 * S], [-0.4 * S, 3.0 * S, 0.0]]) @ H
            F = F / np.abs(F).max()
            ei = [torch.empty((nq, 2), dtype=torch.int32, device="cuda:0") for _ in range(2)]
            ed = [torch.empty((nq, 2), dtype=torch.float32, device="cuda:0") for _ in range(2)]
            torch.cuda.synchronize()
            calls += [lambda h=h: ctx.match_guided_epipolar_device(Q.data_ptr(), qxy.data_ptr(), nq, T.data_ptr(), txy.data_ptr(), nt, r, F, ei[h].data_ptr(),
                                                                   ed[h].data_ptr(), threshold=2.0, f_side=h) for h in (0, 1)]
        for f in calls:
            f()
        ms3 = [[] for _ in calls]
        for _ in range(3):
            for k, f in enumerate(calls):
                f()
                ms3[k].append(ctx.last_kernel_ms())
        best, floor = [min(m) for m in ms3], 1e3 * 2.0 * nq * nt * r / PEAK
        two = [100 * float((g[:, 1] >= 0).float().mean()) for g in gi]
        fmt = lambda m: " ".join("%.3f" % v for v in m)
        if EPI:
            two_e = [100 * float((g[:, 1] >= 0).float().mean()) for g in ei]
            print(f"match_guided_epipolar {nq} x {nt} r {r}: plain {best[0]:.3f} ms (rounds {fmt(ms3[0])}), homography h_side 0 {best[1]:.3f} ms (rounds "
                  f"{fmt(ms3[1])}), h_side 1 {best[2]:.3f} ms (rounds {fmt(ms3[2])}), epipolar f_side 0 {best[3]:.3f} ms (rounds {fmt(ms3[3])}), f_side 1 "
                  f"{best[4]:.3f} ms (rounds {fmt(ms3[4])}); epipolar / plain {best[3] / best[0]:.3f} and {best[4] / best[0]:.3f}, homography / plain "
                  f"{best[1] / best[0]:.3f} and {best[2] / best[0]:.3f}, epipolar / homography {best[3] / best[1]:.3f} and {best[4] / best[2]:.3f}; f64 MFMA "
                  f"floor {floor:.3f} ms; two admitted rows for {two_e[0]:.1f} % and {two_e[1]:.1f} % of the queries (homography: {two[0]:.1f} % and "
                  f"{two[1]:.1f} %)", flush=True)
            del T, Q, idx, d, txy, qxy, gi, gd, ei, ed
            continue
        print(f"match_guided {nq} x {nt} r {r}: plain {best[0]:.3f} ms (rounds {fmt(ms3[0])}), h_side 0 {best[1]:.3f} ms (rounds {fmt(ms3[1])}), "
              f"h_side 1 {best[2]:.3f} ms (rounds {fmt(ms3[2])}); guided / plain {best[1] / best[0]:.3f} and {best[2] / best[0]:.3f}; f64 MFMA floor "
              f"{floor:.3f} ms, share of the floor: plain {floor / best[0]:.3f}, guided {floor / best[1]:.3f} and {floor / best[2]:.3f}; two admitted rows "
              f"for {two[0]:.1f} % and {two[1]:.1f} % of the queries", flush=True)
        del T, Q, idx, d, txy, qxy, gi, gd
        continue
    call()
    ms = []
    for _ in range(2):
        call()
        ms.append(ctx.last_kernel_ms())
    if U8:
        lo = torch.minimum(Q.min(0).values, T.min(0).values)
        scale = 255.0 / float(torch.maximum(Q.max(0).values, T.max(0).values).sub(lo).max())
        ld = (r + 15) // 16 * 16
        Qu, Tu = (torch.zeros((len(X), ld), dtype=torch.uint8, device="cuda:0") for X in (Q, T))
        Qu[:, :r], Tu[:, :r] = (((X - lo) * scale).round().clamp(0, 255).to(torch.uint8) for X in (Q, T))
        iu, du = torch.empty((nq, 2), dtype=torch.int32, device="cuda:0"), torch.empty((nq, 2), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        call8 = lambda: ctx.match_u8_device(Qu.data_ptr(), nq, Tu.data_ptr(), nt, r, iu.data_ptr(), du.data_ptr(), ldq=ld, ldt=ld)
        call8()
        ms8 = []
        for _ in range(2):
            call8()
            ms8.append(ctx.last_kernel_ms())
        agree = float((iu[:, 0] == idx[:, 0]).float().mean())
        best8, best, floor8 = min(ms8), min(ms), 1e3 * 2.0 * nq * nt * r / PEAK_I8
        print(f"match_u8 {nq} x {nt} r {r}: {best8:.3f} ms per call (repeats {ms8[0]:.3f} {ms8[1]:.3f}), int8 MFMA floor {floor8:.3f} ms, "
              f"share of the floor {floor8 / best8:.3f}; float call {best:.3f} ms (repeats {ms[0]:.3f} {ms[1]:.3f}), {best / best8:.2f} x the "
              f"byte call; nearest index agrees with the float call for {100 * agree:.3f} % of the queries", flush=True)
        del T, Q, idx, d, Qu, Tu, iu, du
        continue
    torch_route(Q, T)
    tms = []
    for _ in range(2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ti, td = torch_route(Q, T)
        e1.record()
        torch.cuda.synchronize()
        tms.append(e0.elapsed_time(e1))
    agree = float((ti[:, 0] == idx[:, 0].long()).float().mean())
    best, floor = min(ms), 1e3 * 2.0 * nq * nt * r / PEAK
    print(f"match {nq} x {nt} r {r}: {best:.3f} ms per call (repeats {ms[0]:.3f} {ms[1]:.3f}), f64 MFMA floor {floor:.3f} ms, "
          f"share of the floor {floor / best:.3f}; torch float64 matmul + topk {min(tms):.3f} ms (repeats {tms[0]:.3f} {tms[1]:.3f}), "
          f"{min(tms) / best:.2f} x the fused call; nearest index agrees for {100 * agree:.3f} % of the queries", flush=True)
    del T, Q, idx, d
ctx.close()
