// verify_batch.hpp — the plan of a batched verification (dlco_desc_verify_pairs_*): from the offsets of one segmented match
// list, the hypothesis count and the model's sample size, the launches of the call.  The rule stated once for the host path
// (dlco_desc_api.cpp), the kernels (kernels_verify.hip), which read the Entry below as it is uploaded, and the CPU test
// (tests/shim/verify_batch_shim.cpp).  Plain C++: no HIP header, no device, no I/O.
//
// The match lists of all pairs are one list: pair p owns the matches [moff[p], moff[p + 1]), moff[0] = 0, non-decreasing
// (match-pairs' MatchOffsets).  A pair with at least k_sample matches is an Entry; a pair with fewer launches nothing and
// gets the "no model" answer from the host.
//
// A launch is a run of consecutive entries.  Its matches are the contiguous range from its first entry's first match to
// its last entry's end (the short pairs in between ride along), uploaded once; an entry's m0 counts from there.  Device
// results of the entry at position e of its launch live in slot e: M_all [e][n_hyp][9], count [e][n_hyp], the key, M_cur and
// n [e]; the host's results go to slot `pair` of the caller's arrays.  The scoring grid is 1-D: an entry owns
// ceil(n_hyp / kLanes) x ceil(m / kLanes) workgroups from swg0 on, the hypothesis block the faster index; the mask grid
// gives it ceil(m / kLanes) workgroups from mwg0 on when every entry of the launch is scored.
//
// Limits, parameters so that a test can shrink them: a launch holds at most max_hyp hypotheses (entries x n_hyp; M_all is
// 72 bytes each) and at most max_wgs scoring workgroups.  n_hyp <= max_hyp is the caller's to keep (the library: n_hyp <=
// 2^20).  An entry that alone has more than max_wgs scoring workgroups is a launch of its own, and the host walks its
// scoring grid in pieces of max_wgs.  Launches run one after another and share scratch sized by the largest.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace verify_batch {

constexpr int kLanes = 256;                                // hypotheses of a block and matches of a chunk (verify_rules::kScoreChunk)
constexpr int64_t kLaunchHyp = (int64_t)1 << 22;
constexpr int64_t kLaunchWgs = ((int64_t)1 << 31) - 1;

// One pair as the kernels read it (24 bytes)
struct Entry {
    int64_t m0;                        // first match, counted from the launch's first match
    int32_t m;
    int32_t pair;                      // the caller's slot
    int32_t swg0;                      // first workgroup of the scoring grid
    int32_t mwg0;                      // first workgroup of the mask grid over all entries of the launch
};
static_assert(sizeof(Entry) == 24, "the kernels read entries of 24 bytes");

// an entry the mask kernel scores and its first workgroup among those of the list (8 bytes)
struct Active {
    int32_t entry, wg0;
};
static_assert(sizeof(Active) == 8, "the mask kernel reads active entries of 8 bytes");

struct Launch {
    int64_t e0, n;                     // entries [e0, e0 + n)
    int64_t match0, matches;           // the range of the call's match list it uploads
    int64_t hyps;                      // n * n_hyp
    int64_t score_wgs, mask_wgs;
};

struct Plan {
    std::vector<Entry> entries;
    std::vector<Launch> launches;
    std::vector<int32_t> launch_of_pair;   // [n_pairs]: -1, the pair launches nothing
    int64_t max_entries = 0, max_matches = 0, max_hyps = 0;   // of the largest launch each
};

// what dlco_desc_verify_pairs_* check of the offsets before anything else
inline bool offsets_ok(const int64_t *moff, int64_t n_pairs)
{
    if (!moff || n_pairs < 1 || n_pairs >= ((int64_t)1 << 31) || moff[0] != 0) return false;
    for (int64_t p = 0; p < n_pairs; p++)
        if (moff[p + 1] < moff[p] || moff[p + 1] - moff[p] >= ((int64_t)1 << 31)) return false;
    return true;
}

inline int64_t blocks(int64_t n) { return (n + kLanes - 1) / kLanes; }

// moff is valid (offsets_ok), 1 <= n_hyp <= max_hyp, max_wgs >= 1
inline Plan plan(const int64_t *moff, int64_t n_pairs, int32_t n_hyp, int k_sample, int64_t max_hyp = kLaunchHyp, int64_t max_wgs = kLaunchWgs)
{
    Plan pl;
    pl.launch_of_pair.assign((size_t)n_pairs, -1);
    Launch L{0, 0, 0, 0, 0, 0, 0};
    auto close = [&]() {
        if (L.n == 0) return;
        pl.max_entries = std::max(pl.max_entries, L.n);
        pl.max_matches = std::max(pl.max_matches, L.matches);
        pl.max_hyps = std::max(pl.max_hyps, L.hyps);
        pl.launches.push_back(L);
        L = Launch{(int64_t)pl.entries.size(), 0, 0, 0, 0, 0, 0};
    };
    for (int64_t p = 0; p < n_pairs; p++) {
        const int64_t m = moff[p + 1] - moff[p];
        if (m < k_sample) continue;
        const int64_t wgs = blocks(n_hyp) * blocks(m);
        if (L.n > 0 && (L.hyps + n_hyp > max_hyp || L.score_wgs + wgs > max_wgs)) close();
        if (L.n == 0) L.match0 = moff[p];
        pl.entries.push_back(Entry{moff[p] - L.match0, (int32_t)m, (int32_t)p, (int32_t)L.score_wgs, (int32_t)L.mask_wgs});
        pl.launch_of_pair[(size_t)p] = (int32_t)pl.launches.size();
        L.n++;
        L.matches = moff[p + 1] - L.match0;
        L.hyps += n_hyp;
        L.score_wgs += wgs;
        L.mask_wgs += blocks(m);
        if (L.score_wgs > max_wgs) close();                // an entry too large to share a launch
    }
    close();
    return pl;
}

}  // namespace verify_batch
