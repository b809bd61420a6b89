"""Times the two ways from a table in HBM to the match lists of verify_pairs, on the two sets of the README: a, nine images of
2048 rows, all 72 ordered pairs; b, 33 images of 512 rows, all 1056; r = 128, float and byte line, ratio 0.8, without and with
the mutual check (the reverse pairs are in the same batch).
  (A) match_pairs_device, download of idx + sqdist (16 bytes a row), the rule on the host, a host gather of the coordinates.
      The host rule is numpy over the whole batch at once, no loop over pairs; the host is taken to hold the coordinates.
  (B) match_pairs_device, select_pairs_device, download of moff and of the M entries of the four lists (28 bytes a match).
Per route: the kernels (last_kernel_ms after each library call, summed), the wall clock around the whole route and around the
part behind the match call, which is the part that differs, and the bytes moved between host and device behind the match call.
One warm-up of both, then `rounds` (default 5) rounds that alternate A and B; per figure the best round and the range.  The
lists of the two routes are compared for equality and the run ends with an error when they differ.  No gate: it prints what
it measured.

    select_bench.py [rounds]"""
import importlib, os, sys, time
import numpy as np
import torch                                                # before libdlco.so: one HIP runtime per process, torch's first
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
dlco = importlib.import_module("opencv-dlco_amd")

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
RATIO, R_DIM = 0.8, 128


def host_rule(idx, d, pair_of_row, i_of_row, nt_of_pair, back_row0, ratio):
    """the rule of csrc/select_rules.hpp over all rows at once: the kept rows, ascending"""
    j = idx[:, 0]
    keep = (j >= 0) & (j < nt_of_pair[pair_of_row])
    f = float(np.float32(ratio))
    keep &= (idx[:, 1] == -1) | (d[:, 0].astype(np.float64) < f * f * d[:, 1].astype(np.float64))
    if back_row0 is not None:
        keep &= idx[back_row0[pair_of_row] + np.where(keep, j, 0), 0] == i_of_row
    return np.flatnonzero(keep)


def bench(ctx, name, sizes, u8, mutual):
    n_img = len(sizes)
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pairs = np.array([(a, b) for a in range(n_img) for b in range(n_img) if a != b], np.int32)
    P = len(pairs)
    number = {(int(a), int(b)): p for p, (a, b) in enumerate(pairs)}
    row0 = dlco.match_pairs_rows(seg, pairs)
    R = int(row0[-1])
    back_row0 = np.array([row0[number[(int(b), int(a))]] for a, b in pairs], np.int64) if mutual else None
    pair_of_row = np.repeat(np.arange(P), np.diff(row0))
    i_of_row = np.arange(R) - row0[pair_of_row]
    nt_of_pair = np.diff(seg)[pairs[:, 1]]
    gen = torch.Generator(device="cuda:0").manual_seed(0)
    # images that see one scene: half of an image's rows are noisy views of rows of a shared base, in an order of its own,
    # the rest is clutter, so that the ratio test and the mutual check keep a share of the rows as they do on real images
    n = sizes[0]
    assert all(s == n for s in sizes)
    base = torch.empty((n, R_DIM), dtype=torch.float32, device="cuda:0").normal_(0, 0.25, generator=gen)
    X = torch.empty((int(seg[-1]), R_DIM), dtype=torch.float32, device="cuda:0").normal_(0, 0.25, generator=gen)
    for s in range(n_img):
        order = torch.randperm(n, generator=gen, device="cuda:0")
        view = base[order[:n // 2]] + torch.empty((n // 2, R_DIM), dtype=torch.float32, device="cuda:0").normal_(0, 0.05, generator=gen)
        X[int(seg[s]):int(seg[s]) + n // 2] = view
    if u8:
        lo = X.min(0).values
        X = ((X - lo) * (255.0 / float((X.max(0).values - lo).max()))).round().clamp(0, 255).to(torch.uint8)
    xy_host = np.random.default_rng(1).uniform(0, 4000, (int(seg[-1]), 2)).astype(np.float32)
    xy = torch.from_numpy(xy_host).to("cuda:0")
    ddt, ndt = (torch.int32, np.int32) if u8 else (torch.float32, np.float32)
    dev = lambda shape, t: torch.empty(shape, dtype=t, device="cuda:0")
    idx, d = dev((R, 2), torch.int32), dev((R, 2), ddt)
    m, dd, src, dst = dev((R, 2), torch.int32), dev((R,), ddt), dev((R, 2), torch.float32), dev((R, 2), torch.float32)
    idx_h, d_h = np.empty((R, 2), np.int32), np.empty((R, 2), ndt)
    lists_h = [np.empty((R, 2), np.int32), np.empty(R, ndt), np.empty((R, 2), np.float32), np.empty((R, 2), np.float32)]
    match = ctx.match_pairs_u8_device if u8 else ctx.match_pairs_device
    select = ctx.select_pairs_u8_device if u8 else ctx.select_pairs_device
    copy = lambda host, t, n: host[:n].copy_(t[:n]) if n else None
    torch.cuda.synchronize()

    def route_a():
        t0 = time.perf_counter()
        match(X.data_ptr(), seg, pairs, R_DIM, idx.data_ptr(), d.data_ptr(), ld=R_DIM)
        kernels, t1 = ctx.last_kernel_ms(), time.perf_counter()
        copy(torch.from_numpy(idx_h), idx, R)
        copy(torch.from_numpy(d_h), d, R)
        g = host_rule(idx_h, d_h, pair_of_row, i_of_row, nt_of_pair, back_row0, RATIO)
        p = pair_of_row[g]
        moff = np.concatenate([[0], np.cumsum(np.bincount(p, minlength=P))]).astype(np.int64)
        out = [np.stack([i_of_row[g], idx_h[g, 0]], 1).astype(np.int32), d_h[g, 0], xy_host[seg[pairs[p, 0]] + i_of_row[g]],
               xy_host[seg[pairs[p, 1]] + idx_h[g, 0]]]
        t2 = time.perf_counter()
        return [moff] + out, kernels, 1e3 * (t2 - t0), 1e3 * (t2 - t1), 16 * R

    def route_b():
        t0 = time.perf_counter()
        match(X.data_ptr(), seg, pairs, R_DIM, idx.data_ptr(), d.data_ptr(), ld=R_DIM)
        kernels, t1 = ctx.last_kernel_ms(), time.perf_counter()
        moff = select(idx.data_ptr(), d.data_ptr(), seg, pairs, m.data_ptr(), dd.data_ptr(), ratio=RATIO, back_idx_ptr=idx.data_ptr() if mutual else None,
                      back_row0=back_row0, n_back_rows=R if mutual else 0, xy_ptr=xy.data_ptr(), ldxy=2, src_ptr=src.data_ptr(), dst_ptr=dst.data_ptr())
        kernels += ctx.last_kernel_ms()
        select_ms, M = ctx.last_kernel_ms(), int(moff[-1])
        for host, t in zip(lists_h, (m, dd, src, dst)):
            copy(torch.from_numpy(host), t, M)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return [moff] + [a[:M] for a in lists_h], kernels, 1e3 * (t2 - t0), 1e3 * (t2 - t1), 8 * (P + 1) + 28 * M + 40 * P, select_ms

    a, b = route_a(), route_b()
    for k, (x, y) in enumerate(zip(a[0], b[0])):
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            sys.exit(f"select_bench: list {k} of the two routes differs on set {name}")
    M = int(a[0][0][-1])
    ra, rb = [], []
    for _ in range(rounds):
        ra.append(route_a()[1:])
        rb.append(route_b()[1:])
    col = lambda rows, k: np.array([r[k] for r in rows])
    fmt = lambda v: f"{v.min():.3f} ({v.min():.3f} .. {v.max():.3f})"
    line = "u8" if u8 else "float"
    for tag, rows in (("A", ra), ("B", rb)):
        extra = f" of which select {fmt(col(rows, 4))}" if tag == "B" else ""
        print(f"| {name} | {line} | {'yes' if mutual else 'no'} | {P} | {R} | {M} | {tag} | {fmt(col(rows, 0))}{extra} | {fmt(col(rows, 1))} | {fmt(col(rows, 2))} | "
              f"{rows[0][3]} |", flush=True)
    del X


print(f"select_bench: r {R_DIM}, ratio {RATIO}, best of {rounds} alternating rounds (min .. max), milliseconds")
print("| set | line | mutual | pairs | R | M | route | kernels | wall, whole route | wall behind the match call | bytes moved behind the match call |")
print("|---|---|---|---|---|---|---|---|---|---|---|")
ctx = dlco.DescContext()
for name, sizes in (("a", [2048] * 9), ("b", [512] * 33)):
    for u8 in (False, True):
        for mutual in (False, True):
            bench(ctx, name, sizes, u8, mutual)
ctx.close()
