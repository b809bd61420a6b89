"""The guided surface of the byte line (the ten dlco_desc_*guided*_u8 calls and their DescContext methods) on a machine without
a GPU: the C ABI is declared, exported and bound with the stated signatures, the header's parameter lists equal the ctypes
ones, the argument checks that need no device (the bad-argument table of tests/test_guided_abi.py and of the byte calls, on a
handle that is never dereferenced), and the batch planner under the byte matcher's slicing with a Guide, through
tests/shim/match_batch_guided_shim.cpp."""
import ctypes as C
import inspect
import re
import subprocess

import numpy as np
import pytest

from test_match_batch_guided_rules import FORMS, gplan, guided, random_sets, same_plan       # noqa: F401 (guided is a fixture)

SINGLE = ["dlco_desc_match_guided_u8", "dlco_desc_match_guided_epipolar_u8"]
DEVICE = ["dlco_desc_match_guided_u8_device", "dlco_desc_match_guided_epipolar_u8_device"]
CROSS = ["dlco_desc_cross_sqdists_guided_u8", "dlco_desc_cross_sqdists_guided_epipolar_u8"]
PAIRS = ["dlco_desc_match_pairs_guided_u8", "dlco_desc_match_pairs_guided_epipolar_u8"]
PAIRS_DEVICE = ["dlco_desc_match_pairs_guided_u8_device", "dlco_desc_match_pairs_guided_epipolar_u8_device"]
FUNCS = SINGLE + DEVICE + CROSS + PAIRS + PAIRS_DEVICE
u8p, f32p, f64p, i32p, i64p = (C.POINTER(t) for t in (C.c_uint8, C.c_float, C.c_double, C.c_int32, C.c_int64))
CTYPE = {"dlco_desc_ctx *": C.c_void_p, "const uint8_t *": u8p, "const float *": f32p, "const double *": f64p, "const int64_t *": i64p,
         "const int32_t *": i32p, "int32_t *": i32p, "int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}


def header_params(dlco, name):
    text = re.sub(r"/\*.*?\*/", " ", open(dlco.HEADER_PATH).read(), flags=re.S)
    return [" ".join(p.split()) for p in re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")]


def test_the_ten_functions_are_declared_exported_and_bound(dlco):
    assert len(FUNCS) == 10
    declared = set(dlco.exported_symbols())
    nm = subprocess.run(["nm", "-D", "--defined-only", dlco.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in nm.splitlines() if l.strip())
    L = dlco.load()
    for f in FUNCS:
        assert f in declared, f + " is not declared in include/dlco.h"
        assert f in exported, f + " is not exported by libdlco.so"
        assert getattr(L, f).argtypes is not None, f + " has no ctypes signature"
        assert callable(getattr(dlco.DescContext, f[len("dlco_desc_"):], None)), "DescContext." + f[len("dlco_desc_"):]
    vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    for f in SINGLE:
        assert getattr(L, f).argtypes == [vp, u8p, f32p, i64, u8p, f32p, i64, i32, f64p, f32, i32, i32p, i32p]
    for f in DEVICE:
        assert getattr(L, f).argtypes == [vp, vp, i64, vp, i64, i64, vp, i64, vp, i64, i64, i32, f64p, f32, i32, vp, vp]
    for f in CROSS:
        assert getattr(L, f).argtypes == [vp, u8p, f32p, i64, u8p, f32p, i64, i32, f64p, f32, i32, i32p]
    for f in PAIRS:
        assert getattr(L, f).argtypes == [vp, u8p, f32p, i64p, i32, i32p, i64, i32, f64p, f32, i32, i32p, i32p]
    for f in PAIRS_DEVICE:
        assert getattr(L, f).argtypes == [vp, vp, i64, vp, i64, i64p, i32, i32p, i64, i32, f64p, f32, i32, vp, vp]


def test_the_header_states_the_float_calls_parameter_lists_on_bytes(dlco):
    """every byte call is its float counterpart argument for argument: uint8_t tables, int32_t distances; and the header's
    types are the ctypes ones (a device pointer is bound as void *)"""
    L = dlco.load()
    for f in FUNCS:
        float_name = f.replace("_u8", "")
        got, want = header_params(dlco, f), header_params(dlco, float_name)
        assert len(got) == len(want), f
        for g, w in zip(got, want):
            w = re.sub(r"\bconst float \*(query|train|table)_(host|dev)\b", lambda m: "const uint8_t *%s_%s" % (m.group(1), "u8" if m.group(2) == "host" else "dev"), w)
            w = re.sub(r"\bfloat \*(sqdist_host|sqdist_dev|out_host)\b", r"int32_t *\1", w)
            assert g == w, (f, g, w)
        types = getattr(L, f).argtypes
        assert len(types) == len(got)
        for p, t in zip(got, types):
            decl = p[:p.rindex("*") + 1] if "*" in p else p.rsplit(" ", 1)[0]
            assert t is C.c_void_p or t is CTYPE[decl], (f, p, t)
    for m, defaults in (("match_guided_u8", [("radius", 6.0), ("h_side", 0)]), ("cross_sqdists_guided_u8", [("radius", 6.0), ("h_side", 0)]),
                        ("match_guided_epipolar_u8", [("threshold", 3.0), ("f_side", 0)]), ("cross_sqdists_guided_epipolar_u8", [("threshold", 3.0), ("f_side", 0)]),
                        ("match_pairs_guided_u8", [("radius", 6.0), ("h_side", 0)]), ("match_pairs_guided_epipolar_u8", [("threshold", 3.0), ("f_side", 0)])):
        got, ref = (inspect.signature(getattr(dlco.DescContext, n)) for n in (m, m.replace("_u8", "")))
        assert [(p.name, p.default) for p in got.parameters.values()] == [(p.name, p.default) for p in ref.parameters.values()], m
        assert [(p.name, p.default) for p in got.parameters.values()][-2:] == defaults
    for m in ("match_guided_u8_device", "match_guided_epipolar_u8_device", "match_pairs_guided_u8_device", "match_pairs_guided_epipolar_u8_device"):
        got, ref = (inspect.signature(getattr(dlco.DescContext, n)) for n in (m, m.replace("_u8", "")))
        assert [(p.name, p.default) for p in got.parameters.values()] == [(p.name, p.default) for p in ref.parameters.values()], m
        assert got.parameters["ldxy" if "pairs" in m else "ldxy_q"].default == 2
    raw = " ".join(open(dlco.HEADER_PATH).read().split())
    for words in ("there is no dlco_desc_match_u8_guided", "In scope since: the byte line", "with INT32_MAX where P fails",
                  "the guided _u8 calls, single or pairs, likewise: norms, record kernels, tile loop, merge"):
        assert words in raw, words


@pytest.mark.parametrize("model", [0, 1])
def test_single_calls_reject_bad_arguments_without_a_device(dlco, model):
    L = dlco.load()
    E = dlco.ERR_INVALID
    Q, T = np.zeros((3, 16), np.uint8), np.zeros((5, 16), np.uint8)
    qxy, txy, H = np.zeros((3, 4), np.float32), np.zeros((5, 4), np.float32), np.eye(3).reshape(9).copy()
    idx, d, X = np.full((3, 2), -5, np.int32), np.full((3, 2), -5, np.int32), np.full((3, 5), -5, np.int32)
    p = lambda a, t: a.ctypes.data_as(t)
    good = dict(q=p(Q, u8p), qxy=p(qxy, f32p), nq=3, t=p(T, u8p), txy=p(txy, f32p), nt=5, r=8, H=p(H, f64p), radius=6.0, h_side=0, idx=p(idx, i32p),
                d=p(d, i32p), X=p(X, i32p))
    f_host, f_dev, f_cross = (getattr(L, names[model]) for names in (SINGLE, DEVICE, CROSS))
    host = lambda h, **kw: f_host(h, *[{**good, **kw}[k] for k in ("q", "qxy", "nq", "t", "txy", "nt", "r", "H", "radius", "h_side", "idx", "d")])
    cross = lambda h, **kw: f_cross(h, *[{**good, **kw}[k] for k in ("q", "qxy", "nq", "t", "txy", "nt", "r", "H", "radius", "h_side", "X")])
    vq, vt, vqx, vtx, vi, vd = (C.c_void_p(a.ctypes.data) for a in (Q, T, qxy, txy, idx, d))
    assert Q.ctypes.data % 16 == 0 and T.ctypes.data % 16 == 0
    dgood = dict(q=vq, ldq=16, qxy=vqx, ldxq=4, nq=3, t=vt, ldt=16, txy=vtx, ldxt=4, nt=5, r=8, H=p(H, f64p), radius=6.0, h_side=0, idx=vi, d=vd)
    device = lambda h, **kw: f_dev(h, *[{**dgood, **kw}[k] for k in ("q", "ldq", "qxy", "ldxq", "nq", "t", "ldt", "txy", "ldxt", "nt", "r", "H", "radius",
                                                                     "h_side", "idx", "d")])
    assert host(None) == E and cross(None) == E and device(None) == E       # a null handle: invalid before anything touches a device
    # the arguments are looked at before the handle is used: a handle that is never dereferenced stands in for one
    h = C.c_void_p(Q.ctypes.data)
    H_nan, H_inf = H.copy(), H.copy()
    H_nan[4], H_inf[8] = np.nan, np.inf
    common = [dict(q=None), dict(t=None), dict(qxy=None), dict(txy=None), dict(H=None), dict(H=p(H_nan, f64p)), dict(H=p(H_inf, f64p)), dict(radius=0.0),
              dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(h_side=2), dict(h_side=-1), dict(nq=0), dict(nt=0), dict(nt=2 ** 31),
              dict(r=0), dict(r=1025)]
    for kw in common:
        assert host(h, **kw) == E, kw
        assert cross(h, **kw) == E, kw
        assert device(h, **kw) == E, kw
    for kw in (dict(idx=None), dict(d=None)):
        assert host(h, **kw) == E and device(h, **kw) == E, kw
    assert cross(h, X=None) == E and cross(h, nq=2 ** 20, nt=2 ** 20) == E                                # the matrix's own limit
    # the device form: coordinate pitches and alignment as the float guided call, table pitches and alignment as the byte call
    for kw in (dict(ldxq=1), dict(ldxt=1), dict(ldxq=0), dict(ldxt=-4), dict(ldq=12), dict(ldt=20), dict(ldq=8), dict(ldt=4), dict(ldq=0, r=16), dict(r=17),
               dict(qxy=C.c_void_p(qxy.ctypes.data + 2)), dict(txy=C.c_void_p(txy.ctypes.data + 1)), dict(q=C.c_void_p(Q.ctypes.data + 4)),
               dict(t=C.c_void_p(T.ctypes.data + 8))):
        assert device(h, **kw) == E, kw
    assert (idx == -5).all() and (d == -5).all() and (X == -5).all()
    assert not Q.any() and not T.any() and not qxy.any() and not txy.any() and np.array_equal(H, np.eye(3).reshape(9))


@pytest.mark.parametrize("model", [0, 1])
def test_pair_calls_reject_bad_arguments_without_a_device(dlco, model):
    L = dlco.load()
    E = dlco.ERR_INVALID
    table, xy = np.zeros((8, 16), np.uint8), np.zeros((8, 4), np.float32)
    seg, pairs, M = np.array([0, 3, 8], np.int64), np.array([[0, 1], [1, 0]], np.int32), np.tile(np.eye(3).reshape(9), (2, 1)).copy()
    idx, d = np.full((8, 2), -5, np.int32), np.full((8, 2), -5, np.int32)
    p = lambda a, t: a.ctypes.data_as(t)
    good = dict(t=p(table, u8p), xy=p(xy, f32p), seg=p(seg, i64p), n_img=2, pairs=p(pairs, i32p), n_pairs=2, r=8, M=p(M, f64p), radius=6.0, side=0,
                idx=p(idx, i32p), d=p(d, i32p))
    f_host, f_dev = getattr(L, PAIRS[model]), getattr(L, PAIRS_DEVICE[model])
    host = lambda h, **kw: f_host(h, *[{**good, **kw}[k] for k in ("t", "xy", "seg", "n_img", "pairs", "n_pairs", "r", "M", "radius", "side", "idx", "d")])
    dgood = {**good, **dict(t=C.c_void_p(table.ctypes.data), ld=16, xy=C.c_void_p(xy.ctypes.data), ldxy=4, idx=C.c_void_p(idx.ctypes.data),
                            d=C.c_void_p(d.ctypes.data))}
    device = lambda h, **kw: f_dev(h, *[{**dgood, **kw}[k] for k in ("t", "ld", "xy", "ldxy", "seg", "n_img", "pairs", "n_pairs", "r", "M", "radius", "side",
                                                                     "idx", "d")])
    assert host(None) == E and device(None) == E
    h = C.c_void_p(table.ctypes.data)
    M_nan = M.copy()
    M_nan[1, 7] = np.nan                                   # an entry of the second pair's matrix
    bad_seg, bad_pairs = np.array([1, 3, 8], np.int64), np.array([[0, 2], [1, 0]], np.int32)
    for kw in (dict(t=None), dict(xy=None), dict(seg=None), dict(pairs=None), dict(M=None), dict(idx=None), dict(d=None), dict(M=p(M_nan, f64p)),
               dict(radius=0.0), dict(radius=-2.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(side=2), dict(side=-1), dict(r=0), dict(r=1025),
               dict(n_img=0), dict(n_pairs=0), dict(seg=p(bad_seg, i64p)), dict(pairs=p(bad_pairs, i32p))):
        assert host(h, **kw) == E, kw
        assert device(h, **kw) == E, kw
    for kw in (dict(ld=12), dict(ld=8, r=9), dict(ld=-16), dict(ld=24), dict(t=C.c_void_p(table.ctypes.data + 4)), dict(ldxy=1), dict(ldxy=0), dict(ldxy=-4),
               dict(xy=C.c_void_p(xy.ctypes.data + 2))):
        assert device(h, **kw) == E, kw
    assert (idx == -5).all() and (d == -5).all() and not table.any() and not xy.any()


@pytest.mark.parametrize("both,side", FORMS)
def test_the_planner_under_the_byte_slicing_with_a_guide(guided, both, side):
    """match_slicing::kU8 (256 queries a block) with a Guide: the entries, fills and slices of the byte line's plain plan wherever
    the record limit closes no launch early, and record rows of every entry disjoint and inside the launch's rec_rows"""
    rng = np.random.default_rng(11 + 2 * both + side)
    large = 0
    for seg, pairs in random_sets(120):
        n = np.diff(seg)
        plain = gplan(guided, "u8", seg, pairs, 256)
        assert len(plain["o"]["rec0"]) == 0 and plain["max_rec_rows"] == 0
        assert same_plan(gplan(guided, "u8", seg, pairs, 256, dict(both=both, side=side, no_model=np.zeros(len(pairs), np.uint8))), plain)
        flags = (rng.random(len(pairs)) < 0.2).astype(np.uint8)
        pl = gplan(guided, "u8", seg, pairs, 256, dict(both=both, side=side, no_model=flags, rec_limit=900, launch_rows=1024))
        e, l, o = pl["e"], pl["l"], pl["o"]
        assert np.array_equal(e["qblocks"], -(-e["nq"] // 256))                                   # the byte line's query block
        nq_p, nt_p = n[pairs[:, 0]], n[pairs[:, 1]]
        assert np.array_equal(np.isin(np.arange(len(pairs)), e["pair"]), (nq_p > 0) & (nt_p > 0) & (flags == 0))
        assert len(o["rec0"]) == len(e["nq"])
        assert np.array_equal(o["nqrec"], e["nq"] if both or side == 0 else 0 * e["nq"])
        assert np.array_equal(o["ntrec"], e["nt"] if both or side == 1 else 0 * e["nt"])
        rows = o["nqrec"] + o["ntrec"]
        for k in range(len(l["e0"])):
            s_ = slice(int(l["e0"][k]), int(l["e0"][k] + l["n"][k]))
            assert np.array_equal(o["rec0"][s_], np.concatenate([[0], np.cumsum(rows[s_])])[:-1])    # disjoint, in order
            assert (o["rec0"][s_] + rows[s_] <= l["rec_rows"][k]).all() and rows[s_].sum() == l["rec_rows"][k] <= pl["max_rec_rows"]
            assert l["rec_rows"][k] <= 900 or l["n"][k] == 1
            large += l["rec_rows"][k] > 450
        tiles = -(-e["nt"] // 128)
        assert ((e["slices"] - 1) * e["tps"] < tiles).all() and (e["slices"] * e["tps"] >= tiles).all()          # no slice is empty
    assert large > 0
