// track_rules.hpp — which keypoints of many images are one scene point (dlco_desc_build_tracks*): the verified matches of many
// ordered pairs are the edges of one graph over the rows of the batch's segmented table, its connected components are the
// tracks.  The rule stated once for the kernels (kernels_tracks.hip), the host side of the call (dlco_desc_api.cpp), the
// benchmark's host route (tools/tracks_bench.py) and the CPU tests (tests/shim/track_rules_shim.cpp,
// tests/shim/track_rules_asan_main.cpp).  Plain C++: no HIP header, no device, no I/O.
//
//   nodes   the rows of the table: N = seg[n_img], row i of image a is node g = seg[a] + i; image_of recovers a from g.
//   edges   match m of pair p = (a, b), moff[p] <= m < moff[p + 1], matches[m] = (i, j), is the edge (seg[a] + i, seg[b] + j).
//           It is skipped, not an error, when keep != NULL && keep[m] == 0, or when i or j lies outside its image; the range
//           is decided before anything is indexed with i or j (the `range` clause of select_rules.hpp).  Duplicate edges, both
//           directions of a pair and edges with equal ends are harmless.
//   label   label[g] is the smallest node id of g's connected component.
//   track   a component of at least min_len nodes (min_len >= 2) and, when unique != 0, with no two nodes in one image; a
//           conflicting component is dropped whole.
//   counts  counts[0] components of at least 2 nodes, counts[1] those of fewer than min_len nodes, counts[2] those of at least
//           min_len nodes dropped for a conflict; n_tracks = counts[0] - counts[1] - counts[2].
//   order   tracks ascend in label; inside a track nodes ascend in id, so images ascend as well.  toff [n_tracks + 1] int64,
//           toff[0] = 0; obs [toff[n_tracks]] int32 node ids; track_of [N] int32, the node's track or -1; label [N] int32.  A
//           component has at least min_len >= 2 nodes, so N / 2 + 1 entries of toff and N of obs always suffice.
// Everything is an integer or a comparison: no result depends on the order of the matches, on scheduling or on the run.
//
// The union-find.  parent [N] starts as parent[g] = g.  hook(u, v) below is the step of one edge, written over two operations:
// load(x), which returns parent[x] or an older value of it, and amin(x, v), an atomic parent[x] = min(parent[x], v) that
// returns the value it found.
//   invariant    every write to parent is such a minimum, so a slot only ever decreases and parent[x] <= x always holds; a
//                slot x is only ever given nodes that were already connected to x by the edges hooked so far.
//   termination  find_root walks x -> parent[x] < x, strictly descending, so it ends.  A retry of hook continues with
//                (old, lo), both below hi, so the larger end strictly decreases and the retries end.  No loop waits for
//                another lane.
//   stale reads  a stale load(x) returns an earlier value of parent[x]: an older, larger ancestor of x in the same component.
//                The walk from it still descends inside the component and ends at a node that was a root when it was read.
//                Should hi have ceased to be a root meanwhile, amin tells: it returns old != hi, and the edge (old, lo) is
//                hooked in its place; should lo have ceased to be one, parent[hi] = lo still joins the two components, which
//                is all the edge asks.  So stale reads cost steps, never a result.
//   result       when every edge has been hooked, the nodes with parent[x] == x are the smallest nodes of the components:
//                nothing smaller in its component could ever be written over parent[m] of the smallest node m, and every
//                other root was linked below by the hook that met it.  label[g] = find_root(g).
// Run sequentially with plain loads and a plain minimum, the very same function is the host rule and the CPU tests'.
//
// The kernels group the nodes by a stable sort on label, cut the N sorted nodes into blocks of kBlockNodes, one workgroup
// each, and scan the block counts in one workgroup per counted quantity, kScanChunk counts per step with a carry.  Matches
// are hooked one per lane in workgroups of kBlockNodes lanes as well.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define TRACK_RULES_HD __host__ __device__
#else
#define TRACK_RULES_HD
#endif

namespace track_rules {

constexpr int kBlockNodes = 256;                           // sorted nodes (and matches) a workgroup owns: four waves, a ballot word each
constexpr int kScanChunk = 1024;                           // block counts the scan handles per step: one per lane of its workgroup
constexpr int kCounted = 5;                                // quantities counted per block: kept nodes, kept heads, counts[0 .. 2]

// One pair as the hook kernel reads it (24 bytes): its first match, the first nodes of its two images and their rows
struct Pair {
    int64_t m0;
    int32_t a0, na, b0, nb;
};
static_assert(sizeof(Pair) == 24, "the kernels read pairs of 24 bytes");

TRACK_RULES_HD inline bool in_range(int32_t i, int32_t n) { return i >= 0 && i < n; }

// the edge of match (i, j) of pair pr: false when it is skipped, decided before anything is indexed with i or j
TRACK_RULES_HD inline bool edge_of(const Pair &pr, int32_t i, int32_t j, int32_t *u, int32_t *v)
{
    if (!in_range(i, pr.na) || !in_range(j, pr.nb)) return false;
    *u = pr.a0 + i;
    *v = pr.b0 + j;
    return true;
}

// the last p in [lo, hi] with pairs[p].m0 <= m: empty pairs repeat a value, and the match belongs to the last of them.
// pairs[lo].m0 <= m is the caller's to keep
TRACK_RULES_HD inline int64_t pair_of_match(const Pair *pairs, int64_t lo, int64_t hi, int64_t m)
{
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (pairs[mid].m0 <= m) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the image of node g, 0 <= g < seg[n_img]: the last a in [0, n_img) with seg[a] <= g (empty images repeat a value)
TRACK_RULES_HD inline int32_t image_of(const int64_t *seg, int32_t n_img, int64_t g)
{
    int32_t lo = 0, hi = n_img - 1;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (seg[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <typename Load>
TRACK_RULES_HD inline int32_t find_root(int32_t x, Load &&load)
{
    for (;;) {
        const int32_t p = load(x);
        if (p == x) return x;
        x = p;                                             // p < x: the walk descends
    }
}

// the step of one edge; see the head of the file for load and amin
template <typename Load, typename AtomicMin>
TRACK_RULES_HD inline void hook(int32_t u, int32_t v, Load &&load, AtomicMin &&amin)
{
    for (;;) {
        u = find_root(u, load);
        v = find_root(v, load);
        if (u == v) return;
        const int32_t hi = u > v ? u : v, lo = u > v ? v : u;
        const int32_t old = amin(hi, lo);
        if (old == hi) return;                             // hi was a root and now hangs below lo
        u = old;                                           // hi had a parent already: that one and lo are to be joined
        v = lo;
    }
}

TRACK_RULES_HD inline int64_t blocks(int64_t n) { return (n + kBlockNodes - 1) / kBlockNodes; }

// is a component of sz nodes, with or without two nodes in one image, a track?
TRACK_RULES_HD inline bool is_track(int64_t sz, bool conflict, int32_t min_len, int32_t unique) { return sz >= min_len && !(unique && conflict); }

// what dlco_desc_build_tracks* check beyond seg / pairs (dlco_desc_match_pairs' checks, a table of no rows allowed)
inline bool moff_ok(const int64_t *moff, int64_t n_pairs)
{
    if (!moff || moff[0] != 0) return false;
    for (int64_t p = 0; p < n_pairs; p++)
        if (moff[p + 1] < moff[p]) return false;
    return moff[n_pairs] < ((int64_t)1 << 31);
}
inline bool settings_ok(int32_t min_len, int32_t unique) { return min_len >= 2 && (unique == 0 || unique == 1); }

// the pairs of a call as the hook kernel reads them, [n_pairs]; seg / pairs valid, every image below 2^31 rows and N < 2^31
inline void pair_records(const int64_t *seg, const int32_t *pairs, int64_t n_pairs, const int64_t *moff, std::vector<Pair> &out)
{
    out.resize((size_t)n_pairs);
    for (int64_t p = 0; p < n_pairs; p++) {
        const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
        out[(size_t)p] = Pair{moff[p], (int32_t)seg[a], (int32_t)(seg[a + 1] - seg[a]), (int32_t)seg[b], (int32_t)(seg[b + 1] - seg[b])};
    }
}

// label [N] of the components: every match hooked in the order order[0 .. M) (null: ascending), by the function the kernel runs
inline void labels_host(const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs, const int64_t *moff, const int32_t *matches,
                        const uint8_t *keep, const int64_t *order, int32_t *label)
{
    const int64_t N = seg[n_img], M = moff[n_pairs];
    std::vector<Pair> rec;
    pair_records(seg, pairs, n_pairs, moff, rec);
    std::vector<int32_t> parent((size_t)N);
    for (int64_t g = 0; g < N; g++) parent[(size_t)g] = (int32_t)g;
    auto load = [&](int32_t x) { return parent[(size_t)x]; };
    auto amin = [&](int32_t x, int32_t v) {
        const int32_t old = parent[(size_t)x];
        if (v < old) parent[(size_t)x] = v;
        return old;
    };
    for (int64_t k = 0; k < M; k++) {
        const int64_t m = order ? order[k] : k;
        if (keep && keep[m] == 0) continue;
        const Pair &pr = rec[(size_t)pair_of_match(rec.data(), 0, n_pairs - 1, m)];
        int32_t u, v;
        if (edge_of(pr, matches[2 * m], matches[2 * m + 1], &u, &v)) hook(u, v, load, amin);
    }
    for (int64_t g = 0; g < N; g++) label[g] = find_root((int32_t)g, load);
}

// The whole call on the host.  toff [N / 2 + 1], obs [N], track_of [N], label [N] or null, counts [3]; returns n_tracks.  The
// entries of toff and obs beyond those used are not touched.  For the CPU tests and the benchmark's host route: the library's
// path is the kernels.
inline int64_t tracks_host(const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs, const int64_t *moff, const int32_t *matches,
                           const uint8_t *keep, int32_t min_len, int32_t unique, int64_t *toff, int32_t *obs, int32_t *track_of, int32_t *label,
                           int64_t counts[3])
{
    const int64_t N = seg[n_img];
    std::vector<int32_t> own;
    if (!label) { own.resize((size_t)N); label = own.data(); }
    labels_host(seg, n_img, pairs, n_pairs, moff, matches, keep, nullptr, label);
    // per component, at its label: the size, the image of the node seen last and the conflict; nodes come in ascending id, so
    // two nodes of one image in a component follow one another among that component's nodes
    std::vector<int32_t> size((size_t)N, 0), last_img((size_t)N, -1), slot((size_t)N, -1);
    std::vector<uint8_t> conflict((size_t)N, 0);
    for (int64_t g = 0; g < N; g++) {
        const int32_t l = label[g], a = image_of(seg, n_img, g);
        size[(size_t)l]++;
        if (last_img[(size_t)l] == a) conflict[(size_t)l] = 1;
        last_img[(size_t)l] = a;
    }
    counts[0] = counts[1] = counts[2] = 0;
    int64_t n_tracks = 0, n_obs = 0;
    toff[0] = 0;
    for (int64_t l = 0; l < N; l++) {                      // labels ascending: a component is met at its smallest node
        const int64_t sz = size[(size_t)l];
        if (sz < 2) continue;
        counts[0]++;
        if (sz < min_len) counts[1]++;
        else if (unique && conflict[(size_t)l]) counts[2]++;
        if (!is_track(sz, conflict[(size_t)l] != 0, min_len, unique)) continue;
        slot[(size_t)l] = (int32_t)n_tracks;
        n_obs += sz;
        toff[++n_tracks] = n_obs;
    }
    std::vector<int64_t> fill(toff, toff + n_tracks);
    for (int64_t g = 0; g < N; g++) {
        const int32_t t = slot[(size_t)label[g]];
        track_of[g] = t;
        if (t >= 0) obs[fill[(size_t)t]++] = (int32_t)g;
    }
    return n_tracks;
}

}  // namespace track_rules
