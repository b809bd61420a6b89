"""The track-building surface (dlco_desc_build_tracks, dlco_desc_build_tracks_device, the DescContext methods) on a machine
without a GPU: the C ABI is declared, exported and bound with the stated signatures, and every argument check answers before
the handle is used, with no output touched."""
import ctypes as C
import re
import subprocess

import numpy as np

FUNCS = ["dlco_desc_build_tracks", "dlco_desc_build_tracks_device"]
METHODS = ["build_tracks", "build_tracks_device"]
i32p, i64p, u8p = (C.POINTER(t) for t in (C.c_int32, C.c_int64, C.c_uint8))
NEW_PHRASES = ("csrc/track_rules.hpp states the rule", "a conflicting component is dropped whole",
               "*n_tracks = counts[0] - counts[1] - counts[2]", "only n_tracks and counts cross to the host",
               "entries beyond those used are not touched", "min_len < 2, unique not 0 or 1")


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
    assert dlco.Tracks._fields == ("toff", "obs", "track_of", "label", "counts", "seg")
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    assert L.dlco_desc_build_tracks.argtypes == [vp, i64p, i32, i32p, i64, i64p, i32p, u8p, i32, i32, i64p, i64p, i32p, i32p, i32p, i64p]
    assert L.dlco_desc_build_tracks_device.argtypes == [vp, i64p, i32, i32p, i64, i64p, vp, vp, i32, i32, i64p, vp, vp, vp, vp, i64p]
    # the header states the same parameter lists
    text = re.sub(r"/\*.*?\*/", " ", open(dlco.HEADER_PATH).read(), flags=re.S)
    params = lambda name: [" ".join(p.split()) for p in re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")]
    for name, where in (("dlco_desc_build_tracks", "host"), ("dlco_desc_build_tracks_device", "dev")):
        w = lambda s: s % where
        assert params(name) == ["dlco_desc_ctx *ctx", "const int64_t *seg", "int32_t n_img", "const int32_t *pairs", "int64_t n_pairs", "const int64_t *moff",
                                w("const int32_t *matches_%s"), w("const uint8_t *keep_%s"), "int32_t min_len", "int32_t unique", "int64_t *n_tracks",
                                w("int64_t *toff_%s"), w("int32_t *obs_%s"), w("int32_t *track_of_%s"), w("int32_t *label_%s"), "int64_t counts[3]"], name
    raw = " ".join(l.strip().lstrip("*").strip() for l in open(dlco.HEADER_PATH).read().splitlines())
    raw = " ".join(raw.split())
    for words in NEW_PHRASES:
        assert " ".join(words.split()) in raw, words


def test_calls_reject_bad_arguments_without_a_device(dlco):
    L = dlco.load()
    E = dlco.ERR_INVALID
    seg, pairs = np.array([0, 3, 3, 10], np.int64), np.array([[0, 2], [2, 0], [1, 2]], np.int32)       # N = 10
    moff, m, keep = np.array([0, 2, 4, 4], np.int64), np.array([[0, 1], [1, 2], [3, 0], [4, 1]], np.int32), np.ones(4, np.uint8)
    nt, toff, obs = np.full(1, -5, np.int64), np.full(6, -5, np.int64), np.full(10, -5, np.int32)
    track_of, label, counts = np.full(10, -5, np.int32), np.full(10, -5, np.int32), np.full(3, -5, np.int64)
    p = lambda a, t: a.ctypes.data_as(t)
    v = lambda a: C.c_void_p(a.ctypes.data)
    K = ("seg", "n_img", "pairs", "n_pairs", "moff", "m", "keep", "min_len", "unique", "nt", "toff", "obs", "track_of", "label", "counts")
    plain = dict(seg=p(seg, i64p), n_img=3, pairs=p(pairs, i32p), n_pairs=3, moff=p(moff, i64p), min_len=2, unique=1, nt=p(nt, i64p), counts=p(counts, i64p))
    gh = {**plain, "m": p(m, i32p), "keep": p(keep, u8p), "toff": p(toff, i64p), "obs": p(obs, i32p), "track_of": p(track_of, i32p), "label": p(label, i32p)}
    gd = {**plain, "m": v(m), "keep": v(keep), "toff": v(toff), "obs": v(obs), "track_of": v(track_of), "label": v(label)}
    arg = lambda good, kw: [{**good, **kw}[k] for k in K]
    host = lambda h, **kw: L.dlco_desc_build_tracks(h, *arg(gh, kw))
    dev = lambda h, **kw: L.dlco_desc_build_tracks_device(h, *arg(gd, kw))
    for f in (host, dev):
        assert f(None) == E                                # a null handle: invalid before anything touches a device
    # the arguments are looked at before the handle is used: a handle that is never dereferenced stands in for one
    h = C.c_void_p(m.ctypes.data)
    alive = []                                             # the arrays behind the pointers stay alive
    def segs(a):
        alive.append(np.array(a, np.int64))
        return dict(seg=p(alive[-1], i64p), n_img=len(a) - 1)
    def prs(a):
        alive.append(np.array(a, np.int32))
        return dict(pairs=p(alive[-1], i32p), n_pairs=len(a))
    def moffs(a):
        alive.append(np.array(a, np.int64))
        return dict(moff=p(alive[-1], i64p))
    bad = [dict(seg=None), dict(pairs=None), dict(moff=None), dict(m=None), dict(nt=None), dict(toff=None), dict(obs=None), dict(track_of=None),
           dict(counts=None),
           # the seg / pairs errors of match_pairs
           dict(n_img=0), dict(n_img=-1), dict(n_pairs=0), dict(n_pairs=-3), segs([1, 3, 3, 10]), segs([0, 3, 2, 10]),
           segs([0, 3, 3 + 2 ** 31, 4 + 2 ** 31]), prs([[0, 3], [2, 0], [1, 2]]), prs([[0, 2], [-1, 0], [1, 2]]), prs([[0, 2], [2, 0], [1, 2 ** 20]]),
           # N >= 2^31: images below 2^31 rows each
           segs([0, 2 ** 30, 2 ** 31, 2 ** 31 + 5]),
           # moff: a first entry other than 0, a decrease, M >= 2^31
           moffs([1, 2, 4, 4]), moffs([0, 2, 1, 4]), moffs([0, 2, 4, -1]), moffs([0, 2, 4, 2 ** 31]), moffs([-1, 2, 4, 4]),
           # the settings
           dict(min_len=1), dict(min_len=0), dict(min_len=-2), dict(unique=2), dict(unique=-1)]
    for kw in bad:
        for f in (host, dev):
            assert f(h, **kw) == E, kw
    assert (nt == -5).all() and (toff == -5).all() and (obs == -5).all() and (track_of == -5).all() and (label == -5).all() and (counts == -5).all()
    assert moff.tolist() == [0, 2, 4, 4] and m.tolist() == [[0, 1], [1, 2], [3, 0], [4, 1]] and (keep == 1).all()
