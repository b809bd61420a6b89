// match_batch.hpp — the plan of a batched match (dlco_desc_match_pairs*): from the segment table of a set of images, a list
// of (query image, train image) pairs and the CU count, the launches of the call.  The rule stated once for the host path
// (dlco_desc_api.cpp), the kernels (kernels_match.hip, kernels_match_u8.hip), which read the Entry below as it is uploaded,
// and the CPU test (tests/shim/match_batch_shim.cpp).  Plain C++: no HIP header, no device, no I/O.
//
// A set of images is one table: image s owns the rows [seg[s], seg[s + 1]).  Pair p = (a, b) owns the output rows
// [row0[p], row0[p + 1]), row0 the running sum of the query images' row counts; they are what a single call with query =
// image a and train = image b returns.
//
// A launch is a 1-D grid over a run of consecutive pairs with at most kLaunchRows query rows (the kernels index a launch's
// queries with an int); a pair with more is cut into row ranges.  Every pair or range is an Entry, whose workgroups are
// (its query blocks) x (its slices), the slice the slower index, numbered from the entry's first workgroup.  The slices of
// an entry are match_slices.hpp's rule on its train image with the query blocks of the WHOLE launch in place of the single
// call's: once the launch has per_cu * n_cu query blocks every entry has one slice and stores its rows directly; with few
// pairs the entries keep their slices, write partials at offsets of their own and a merge launch follows.  The property the
// kernels rely on is the single call's: NO SLICE IS EMPTY.  A pair whose query image is empty owns no rows and has no
// entry; a pair whose train image is empty has no entry either and goes to the fill list (-1 / +inf in both columns).
// Entries keep the order of the pairs: the order of workgroups changes no result, and no other order was measured.
//
// The guided forms (dlco_desc_match_pairs_guided*) give plan() a Guide.  Geometry in a batch belongs to a PAIR, not to an
// image: the same image meets another matrix in every pair it appears in, so the records of guided_rules.hpp /
// guided_epipolar_rules.hpp (32 bytes a row) are per entry.  A launch has one record buffer; entry e owns its rows
// [rec0, rec0 + nqrec + ntrec), first the records of its query rows, then those of its train image.  Under a homography only
// the side H applies to has records (side 0: the entry's queries, side 1: its train image), under a fundamental matrix both
// sides have.  Plan::guide is indexed like Plan::entries; the Entry itself is unchanged.  A launch also closes when its record
// rows would pass Guide::rec_limit, except that it always holds one entry; closing a launch early changes slice counts only,
// and the key is a total order, so no result moves.  The row ranges of a cut pair never share a launch (the first fills one),
// so each range carries its train image's records again.  A pair whose flag in Guide::no_model is set ("no model": the
// all-zero matrix, which admits nothing) has no entry and goes to the fill list like a pair with an empty train image.
#pragma once

#include "match_slices.hpp"

#include <cstdint>
#include <vector>

namespace match_batch {

constexpr int64_t kLaunchRows = (int64_t)1 << 20;

// One pair, or one row range of a pair, as the kernels read it (64 bytes).  Rows are rows of the one table; part0 counts
// partials (16 bytes each) from the start of the partial buffer, slice s of the entry writes at part0 + s * nq.
struct Entry {
    int64_t q0, t0;                    // first query row, first row of the train image
    int64_t out0;                      // first output row
    int64_t part0;                     // slices > 1: offset of its partials
    int32_t nq, nt;
    int32_t tiles_per_slice, slices;
    int32_t wg0;                       // first workgroup of the tile loop's launch
    int32_t mwg0;                      // first workgroup (256 rows each) of the merge launch; slices == 1: it has none
    int32_t qblocks;                   // workgroups per slice
    int32_t pair;
};
static_assert(sizeof(Entry) == 64, "the kernels read entries of 64 bytes");

struct Launch {
    int64_t e0, n;                     // entries [e0, e0 + n)
    int64_t rows;                      // query rows
    int64_t qblocks;                   // query blocks of the launch, the figure the slicing rule took
    int64_t wgs, merge_wgs;            // grid of the tile loop, of the merge (0: nothing to merge)
    int64_t parts;                     // partials written
    int64_t rec_rows;                  // guided: record rows of the launch (0 without a Guide)
};

constexpr int64_t kRecordRows = (int64_t)1 << 22;          // record rows of a launch in the library: 128 MB

// What the guided forms add to the arguments of plan().
struct Guide {
    const uint8_t *no_model = nullptr; // [n_pairs], or null: non-zero sends the pair to the fill list
    bool both_sides = false;           // records on both sides (a fundamental matrix) or on the side the homography applies to
    int side = 0;                      // the homography's side: 0 the queries carry the records, 1 the train image does
    int64_t rec_limit = kRecordRows;
    int64_t launch_rows = kLaunchRows; // query rows of a launch; the library leaves it, the CPU test shrinks both limits
};

// The records of entry e of a launch, as the kernels read them (16 bytes), in record rows of the launch's buffer
struct GuideOff {
    int64_t rec0;                      // its first record row: the queries' records, then the train image's
    int32_t nqrec, ntrec;              // record rows of the queries (0 or nq) and of the train image (0 or nt)
};
static_assert(sizeof(GuideOff) == 16, "the kernels read guide offsets of 16 bytes");

// rows [out0, out0 + n) of a pair with an empty train image; first = rows of the fills before it
struct Fill {
    int64_t out0, n, first;
    int64_t pair;
};
static_assert(sizeof(Fill) == 32, "the fill kernel reads fills of 32 bytes");

struct Plan {
    std::vector<Entry> entries;
    std::vector<Launch> launches;
    std::vector<Fill> fills;
    std::vector<int64_t> row0;         // [n_pairs + 1]
    std::vector<int32_t> slices;       // [n_pairs]: slices of the pair (the most of its ranges); 0: it launches nothing
    int64_t fill_rows = 0;
    int64_t max_parts = 0;             // the largest launch's partials: launches run one after another and share the buffer
    std::vector<GuideOff> guide;       // guided: [entries.size()], else empty
    int64_t max_rec_rows = 0;          // guided: the largest launch's record rows; the launches share that buffer too
};

inline void row_offsets(const int64_t *seg, const int32_t *pairs, int64_t n_pairs, int64_t *row0)
{
    row0[0] = 0;
    for (int64_t p = 0; p < n_pairs; p++) row0[p + 1] = row0[p] + (seg[pairs[2 * p] + 1] - seg[pairs[2 * p]]);
}

// seg and pairs are valid (dlco_desc_match_pairs' checks): every image has fewer than 2^31 rows
inline Plan plan(const match_slicing::Shape &s, const int64_t *seg, const int32_t *pairs, int64_t n_pairs, int n_cu, const Guide *guide = nullptr)
{
    Plan pl;
    pl.row0.resize((size_t)n_pairs + 1);
    pl.slices.assign((size_t)n_pairs, 0);
    row_offsets(seg, pairs, n_pairs, pl.row0.data());

    // close the open launch: its query blocks are known now, so its entries get their slices, workgroups and partials
    const int64_t launch_rows = guide ? guide->launch_rows : kLaunchRows;
    size_t open = 0;
    int64_t open_rows = 0, open_rec = 0;
    auto close = [&]() {
        if (open == pl.entries.size()) return;
        Launch L{(int64_t)open, (int64_t)(pl.entries.size() - open), open_rows, 0, 0, 0, 0, open_rec};
        pl.max_rec_rows = std::max(pl.max_rec_rows, open_rec);
        for (size_t e = open; e < pl.entries.size(); e++) L.qblocks += pl.entries[e].qblocks;
        for (size_t e = open; e < pl.entries.size(); e++) {
            Entry &en = pl.entries[e];
            en.tiles_per_slice = match_slicing::tiles_per_slice_of(s, L.qblocks, en.nt, n_cu);
            en.slices = match_slicing::slices(s, en.nt, en.tiles_per_slice);
            en.wg0 = (int32_t)L.wgs;
            en.mwg0 = (int32_t)L.merge_wgs;
            en.part0 = L.parts;
            L.wgs += (int64_t)en.qblocks * en.slices;
            if (en.slices > 1) {
                L.merge_wgs += (en.nq + 255) / 256;
                L.parts += (int64_t)en.slices * en.nq;
            }
            pl.slices[(size_t)en.pair] = std::max(pl.slices[(size_t)en.pair], en.slices);
        }
        pl.max_parts = std::max(pl.max_parts, L.parts);
        pl.launches.push_back(L);
        open = pl.entries.size();
        open_rows = 0;
        open_rec = 0;
    };

    for (int64_t p = 0; p < n_pairs; p++) {
        const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
        const int64_t nq = seg[a + 1] - seg[a], nt = seg[b + 1] - seg[b];
        if (nq == 0) continue;
        if (nt == 0 || (guide && guide->no_model && guide->no_model[p])) {
            pl.fills.push_back(Fill{pl.row0[(size_t)p], nq, pl.fill_rows, p});
            pl.fill_rows += nq;
            continue;
        }
        for (int64_t r0 = 0; r0 < nq; r0 += launch_rows) {
            const int64_t cnt = std::min(launch_rows, nq - r0);
            if (open_rows + cnt > launch_rows) close();
            if (guide) {
                const bool qrec = guide->both_sides || guide->side == 0, trec = guide->both_sides || guide->side != 0;
                const int64_t rec = (qrec ? cnt : 0) + (trec ? nt : 0);
                if (open_rec + rec > guide->rec_limit) close();          // an empty launch takes the entry whatever its size
                pl.guide.push_back(GuideOff{open_rec, (int32_t)(qrec ? cnt : 0), (int32_t)(trec ? nt : 0)});
                open_rec += rec;
            }
            Entry en{};
            en.q0 = seg[a] + r0;
            en.t0 = seg[b];
            en.out0 = pl.row0[(size_t)p] + r0;
            en.nq = (int32_t)cnt;
            en.nt = (int32_t)nt;
            en.qblocks = (int32_t)((cnt + s.qblock - 1) / s.qblock);
            en.pair = (int32_t)p;
            pl.entries.push_back(en);
            open_rows += cnt;
        }
    }
    close();
    return pl;
}

}  // namespace match_batch
