"""The match-selection surface (dlco_desc_select_pairs and its forms, the DescContext methods) on a machine without a GPU: the
C ABI is declared, exported and bound with the stated signatures, and every argument check answers before the handle is used,
with no output touched."""
import ctypes as C
import re
import subprocess

import numpy as np

FUNCS = ["dlco_desc_select_pairs", "dlco_desc_select_pairs_device", "dlco_desc_select_pairs_u8", "dlco_desc_select_pairs_u8_device"]
METHODS = ["select_pairs", "select_pairs_u8", "select_pairs_device", "select_pairs_u8_device"]
f32p, i32p, i64p = (C.POINTER(t) for t in (C.c_float, C.c_int32, C.c_int64))
# phrases of include/dlco.h that earlier ABI tests look for: the header still carries every one of them
OLD_PHRASES = ("guided forms of the batch", "a batched distance matrix", "seg / pairs in device memory", "a batched verify",
               "after a match_pairs call, float or _u8, every kernel of the call",
               "Out of scope of this call: a device-memory form (the match list is filtered on the host)",
               "Out of scope: a device-memory form; seeds or thresholds per pair; a choice between H and F.",
               "In scope since: a batched verify, dlco_desc_verify_pairs_* below; guided forms of the batch, dlco_desc_match_pairs_guided* below.",
               "In scope since: an epipolar predicate for guided matching, dlco_desc_match_guided_epipolar above.",
               "of the best models and the mask launch of every lockstep refit round")
NEW_PHRASES = ("In scope since: the step from idx / sqdist to the match list of dlco_desc_verify_pairs_* (ratio test, mutual check, "
               "compaction) on the device, dlco_desc_select_pairs* below.",
               "In scope since: filtering the match list on the device, dlco_desc_select_pairs* below",
               "after a select_pairs call, float or _u8, its kernels",
               "a device-memory form of dlco_desc_verify_pairs_*", "single-pair entry points: a batch of one pair is the single call",
               "the tools, which keep their host rule", "csrc/select_rules.hpp states the rule")


def test_functions_are_declared_exported_and_bound(dlco):
    declared = set(dlco.exported_symbols())
    nm = subprocess.run(["nm", "-D", "--defined-only", dlco.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    L = dlco.load()
    for f in FUNCS:
        assert f in declared, f + " is not declared in include/dlco.h"
        assert f in exported, f + " is not exported by libdlco.so"
        assert getattr(L, f).argtypes is not None, f + " has no ctypes signature"
    for m in METHODS:
        assert callable(getattr(dlco.DescContext, m, None)), "DescContext." + m
    vp, i64, i32, fl = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    assert L.dlco_desc_select_pairs.argtypes == [vp, i64p, i32, i32p, i64, i32p, f32p, fl, i32p, i64p, i64, f32p, i64p, i32p, f32p, f32p, f32p]
    assert L.dlco_desc_select_pairs_u8.argtypes == [vp, i64p, i32, i32p, i64, i32p, i32p, fl, i32p, i64p, i64, f32p, i64p, i32p, i32p, f32p, f32p]
    for f in (L.dlco_desc_select_pairs_device, L.dlco_desc_select_pairs_u8_device):
        assert f.argtypes == [vp, i64p, i32, i32p, i64, vp, vp, fl, vp, i64p, i64, vp, i64, i64p, vp, vp, vp, vp]
    # the header states the same parameter lists
    text = re.sub(r"/\*.*?\*/", " ", open(dlco.HEADER_PATH).read(), flags=re.S)
    params = lambda name: [" ".join(p.split()) for p in re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")]
    head = ["dlco_desc_ctx *ctx", "const int64_t *seg", "int32_t n_img", "const int32_t *pairs", "int64_t n_pairs"]
    back = ["const int64_t *back_row0", "int64_t n_back_rows"]
    for name, dist, where in (("dlco_desc_select_pairs", "float", "host"), ("dlco_desc_select_pairs_device", "float", "dev"),
                              ("dlco_desc_select_pairs_u8", "int32_t", "host"), ("dlco_desc_select_pairs_u8_device", "int32_t", "dev")):
        w = lambda s: s % where
        assert params(name) == head + [w("const int32_t *idx_%s"), "const " + dist + w(" *sqdist_%s"), "float ratio", w("const int32_t *back_idx_%s")] + back + \
            [w("const float *xy_%s")] + (["int64_t ldxy"] if where == "dev" else []) + \
            ["int64_t *moff", w("int32_t *matches_%s"), dist + w(" *dist_%s"), w("float *src_xy_%s"), w("float *dst_xy_%s")], name
    raw = " ".join(l.strip().lstrip("*").strip() for l in open(dlco.HEADER_PATH).read().splitlines())
    raw = " ".join(raw.split())
    for words in OLD_PHRASES + NEW_PHRASES:
        assert " ".join(words.split()) in raw, words


def test_calls_reject_bad_arguments_without_a_device(dlco):
    L = dlco.load()
    E = dlco.ERR_INVALID
    seg, pairs = np.array([0, 3, 3, 10], np.int64), np.array([[0, 2], [2, 0], [1, 2]], np.int32)       # R = 10, nt_b = 7, 3, 7
    idx, d, d8 = np.zeros((10, 2), np.int32), np.ones((10, 2), np.float32), np.ones((10, 2), np.int32)
    brow0, xy = np.array([3, 0, -1], np.int64), np.zeros((10, 4), np.float32)
    moff, m, dd, dd8 = np.full(4, -5, np.int64), np.full((10, 2), -5, np.int32), np.full(10, -5, np.float32), np.full(10, -5, np.int32)
    src, dst = np.full((10, 2), -5, np.float32), np.full((10, 2), -5, np.float32)
    p = lambda a, t: a.ctypes.data_as(t)
    v = lambda a: C.c_void_p(a.ctypes.data)
    K = ("seg", "n_img", "pairs", "n_pairs", "idx", "d", "ratio", "back", "brow0", "nback", "xy")
    OUT = ("moff", "m", "dd", "src", "dst")
    plain = dict(seg=p(seg, i64p), n_img=3, pairs=p(pairs, i32p), n_pairs=3, ratio=0.8, back=None, brow0=None, nback=0, xy=None, ldxy=2,
                 moff=p(moff, i64p), src=None, dst=None)
    arg = lambda good, kw, keys: [{**good, **kw}[k] for k in keys]
    gh = {**plain, "idx": p(idx, i32p), "d": p(d, f32p), "m": p(m, i32p), "dd": p(dd, f32p)}
    gh8 = {**plain, "idx": p(idx, i32p), "d": p(d8, i32p), "m": p(m, i32p), "dd": p(dd8, i32p)}
    gd = {**plain, "idx": v(idx), "d": v(d), "m": v(m), "dd": v(dd)}
    gd8 = {**plain, "idx": v(idx), "d": v(d8), "m": v(m), "dd": v(dd8)}
    host = lambda h, **kw: L.dlco_desc_select_pairs(h, *arg(gh, kw, K + OUT))
    host8 = lambda h, **kw: L.dlco_desc_select_pairs_u8(h, *arg(gh8, kw, K + OUT))
    dev = lambda h, **kw: L.dlco_desc_select_pairs_device(h, *arg(gd, kw, K + ("ldxy",) + OUT))
    dev8 = lambda h, **kw: L.dlco_desc_select_pairs_u8_device(h, *arg(gd8, kw, K + ("ldxy",) + OUT))
    hosts, devs = (host, host8), (dev, dev8)
    for f in hosts + devs:
        assert f(None) == E                                # a null handle: invalid before anything touches a device
    # the arguments are looked at before the handle is used: a handle that is never dereferenced stands in for one
    h = C.c_void_p(idx.ctypes.data)
    keep = []                                              # the arrays behind the pointers stay alive
    def segs(a):
        keep.append(np.array(a, np.int64))
        return dict(seg=p(keep[-1], i64p), n_img=len(a) - 1)
    def prs(a):
        keep.append(np.array(a, np.int32))
        return dict(pairs=p(keep[-1], i32p), n_pairs=len(a))
    def rows(a, n, where):
        keep.append(np.array(a, np.int64))
        return dict(back=p(idx, i32p) if where == "host" else v(idx), brow0=p(keep[-1], i64p), nback=n)
    for where, fs in (("host", hosts), ("dev", devs)):
        P = (lambda a, t: p(a, t)) if where == "host" else (lambda a, t: v(a))
        coords = dict(xy=P(xy, f32p), src=P(src, f32p), dst=P(dst, f32p))
        bad = [dict(seg=None), dict(pairs=None), dict(idx=None), dict(d=None), dict(moff=None), dict(m=None), dict(dd=None),
               # the seg / pairs errors of match_pairs
               dict(n_img=0), dict(n_img=-1), dict(n_pairs=0), dict(n_pairs=-3), segs([1, 3, 3, 10]), segs([0, 3, 2, 10]), segs([0, 0, 0, 0]),
               segs([0, 3, 3 + 2 ** 31, 4 + 2 ** 31]), prs([[0, 3], [2, 0], [1, 2]]), prs([[0, 2], [-1, 0], [1, 2]]), prs([[0, 2], [2, 0], [1, 2 ** 20]]),
               # R >= 2^31: three query images of 2^30 rows
               {**segs([0, 2 ** 30, 2 ** 30 + 1]), **prs([[0, 1], [0, 1], [0, 0]])},
               # the ratio: NaN, negative, above 1
               dict(ratio=float("nan")), dict(ratio=-0.5), dict(ratio=float(np.nextafter(np.float32(1), np.float32(2)))), dict(ratio=float("inf")),
               # the reverse table: without back_row0, a row below -1, rows that end beyond n_back_rows, a negative row count
               {**rows([3, 0, -1], 10, where), "brow0": None}, rows([3, 0, -2], 10, where), rows([4, 0, -1], 10, where), rows([3, 8, -1], 10, where),
               rows([3, 0, 4], 10, where), rows([3, 0, -1], 9, where), rows([3, 0, -1], -1, where), rows([2 ** 62, 0, -1], 10, where),
               # coordinates: lists without the table, or only one of the two
               dict(src=coords["src"]), dict(dst=coords["dst"]), dict(src=coords["src"], dst=coords["dst"]), {**coords, "src": None},
               {**coords, "dst": None}]
        if where == "dev":
            bad += [{**coords, "ldxy": 1}, {**coords, "ldxy": 0}, {**coords, "ldxy": -2}]
        for kw in bad:
            for f in fs:
                assert f(h, **kw) == E, (where, kw)
    assert (moff == -5).all() and (m == -5).all() and (dd == -5).all() and (dd8 == -5).all() and (src == -5).all() and (dst == -5).all()
    assert not idx.any() and (d == 1).all() and (d8 == 1).all() and not xy.any() and brow0.tolist() == [3, 0, -1]
