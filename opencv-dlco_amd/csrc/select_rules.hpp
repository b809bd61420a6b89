// select_rules.hpp — which rows of a batched match answer become matches (dlco_desc_select_pairs*): Lowe's ratio test, the
// mutual check and the order of the compacted list.  The rule stated once for the host path (dlco_desc_api.cpp), the kernels
// (kernels_select.hip) and the CPU tests (tests/shim/select_rules_shim.cpp, and match_rules_shim.cpp / match_rules_u8_shim.cpp
// on one pair).  The tools match and match-pairs hold no copy: they call dlco_desc_select_pairs*.  Plain C++: no HIP header, no
// device, no I/O.
//
// The answer of a match_pairs call, plain or guided, is idx [R][2] / sqdist [R][2]: pair p = (a, b) owns the rows
// [row0[p], row0[p + 1]) (match_batch.hpp), row i of it holds the nearest two rows of image b for row i of image a.  With
// j = idx[i][0], d1 = sqdist[i][0], d2 = sqdist[i][1] and nt_b the rows of image b, row i is a match iff
//   range    0 <= j < nt_b.  Decided before anything at j is read, so that a stray index in a caller's table reads nothing
//            outside a buffer; -1 is "no candidate" (a guided answer, an empty train image).
//   ratio    (when asked for, f in (0, 1])  idx[i][1] == -1, a row without a second neighbour, or
//            (double)d1 < (double)f * (double)f * (double)d2.  f * f is exact in double and the product with d2 is one
//            rounding, the same on every machine; d1 == f^2 d2 is dropped, and so is d1 = d2 = 0.  The distances are float or,
//            on the byte line, int32, which double holds exactly.
//   mutual   (when asked for, per pair)  back_idx[back0 + j][0] == i, back0 the first row of the reverse answer, image b's rows
//            matched against image a; back0 = -1: no mutual check for this pair.
// The list is the stable compaction of the kept rows: pairs in order, rows ascending inside a pair; moff[p] counts the
// matches before pair p's first row.  Everything is an integer or a comparison: no result depends on scheduling.
//
// The kernels cut the R rows into blocks of kBlockRows, one workgroup each; the exclusive scan of the block counts runs in
// one workgroup, kScanChunk counts per step with a carry.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define SELECT_RULES_HD __host__ __device__
#else
#define SELECT_RULES_HD
#endif

namespace select_rules {

constexpr int kBlockRows = 256;                            // rows a workgroup owns: four waves, a ballot word each
constexpr int kScanChunk = 1024;                           // block counts the scan handles per step: one per lane of its workgroup

SELECT_RULES_HD inline bool ratio_keep(float d1, float d2, int32_t idx2, float f)
{
    if (idx2 == -1) return true;
    return (double)d1 < (double)f * (double)f * (double)d2;
}

SELECT_RULES_HD inline bool ratio_keep(int32_t d1, int32_t d2, int32_t idx2, float f)
{
    if (idx2 == -1) return true;
    return (double)d1 < (double)f * (double)f * (double)d2;
}

// back [nt_b][2]: the reverse answer of the pair.  j is in range (in_range)
SELECT_RULES_HD inline bool cross_keep(int64_t i, int32_t j, const int32_t *back) { return back[2 * (int64_t)j] == (int32_t)i; }

SELECT_RULES_HD inline bool in_range(int32_t j, int32_t nt_b) { return j >= 0 && j < nt_b; }

// One pair as the kernels read it (40 bytes): its first output row, the first rows of its two images in the one table (for
// the coordinates), the first row of its reverse answer (-1: no mutual check) and the rows of its train image.
struct Pair {
    int64_t row0, src0, dst0, back0;
    int32_t nt, pad;
};
static_assert(sizeof(Pair) == 40, "the kernels read pairs of 40 bytes");

// The rule for row i of a pair: idx2 / d2 are the row's own two columns, f == 0: no ratio test, back: the whole reverse
// table or null.  Reads back only at back0 + j with j in range.
template <typename Dist>
SELECT_RULES_HD inline bool keep(const Pair &pr, int64_t i, const int32_t idx2[2], const Dist d2[2], float f, const int32_t *back)
{
    const int32_t j = idx2[0];
    if (!in_range(j, pr.nt)) return false;
    if (f != 0.0f && !ratio_keep(d2[0], d2[1], idx2[1], f)) return false;
    if (back && pr.back0 >= 0 && !cross_keep(i, j, back + 2 * pr.back0)) return false;
    return true;
}

// the last p in [lo, hi] with pairs[p].row0 <= g: empty pairs repeat a value, and the row belongs to the last of them.
// pairs[lo].row0 <= g is the caller's to keep
SELECT_RULES_HD inline int64_t pair_of_row(const Pair *pairs, int64_t lo, int64_t hi, int64_t g)
{
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (pairs[mid].row0 <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

SELECT_RULES_HD inline int64_t blocks(int64_t rows) { return (rows + kBlockRows - 1) / kBlockRows; }

// what dlco_desc_select_pairs* check of the reverse table, seg / pairs being valid (dlco_desc_match_pairs' checks): every
// back_row0[p] is -1 or the first of nt_b rows inside [0, n_back_rows)
inline bool back_rows_ok(const int64_t *seg, const int32_t *pairs, int64_t n_pairs, const int64_t *back_row0, int64_t n_back_rows)
{
    if (!back_row0 || n_back_rows < 0) return false;
    for (int64_t p = 0; p < n_pairs; p++) {
        const int32_t b = pairs[2 * p + 1];
        const int64_t nt = seg[b + 1] - seg[b];
        if (back_row0[p] < -1) return false;
        if (back_row0[p] >= 0 && (back_row0[p] > n_back_rows || nt > n_back_rows - back_row0[p])) return false;
    }
    return true;
}

// f == 0 (no ratio test) or f in (0, 1]; a NaN fails
inline bool ratio_ok(float f) { return f >= 0.0f && f <= 1.0f; }

// the pairs of a call as the kernels read them, [n_pairs]; back_row0 may be null (no mutual check); returns R
inline int64_t pair_records(const int64_t *seg, const int32_t *pairs, int64_t n_pairs, const int64_t *back_row0, std::vector<Pair> &out)
{
    out.resize((size_t)n_pairs);
    int64_t row = 0;
    for (int64_t p = 0; p < n_pairs; p++) {
        const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
        out[(size_t)p] = Pair{row, seg[a], seg[b], back_row0 ? back_row0[p] : -1, (int32_t)(seg[b + 1] - seg[b]), 0};
        row += seg[a + 1] - seg[a];
    }
    return row;
}

// The whole call on the host, in the kernels' cut: the flag words and block counts, the scan in chunks with a carry, the
// scatter by block offset + earlier words + the bits below the row.  rec [n_pairs] / R from pair_records; idx, sqdist [R][2];
// back the reverse table or null; xy [.][ldxy] or null; moff [n_pairs + 1]; matches [.][2], dist [.], src_xy, dst_xy [.][2]
// (null without xy) receive the first M = moff[n_pairs] entries.  For the CPU tests: the library's path is the kernels.
template <typename Dist>
inline void select_host(const Pair *rec, int64_t n_pairs, int64_t R, const int32_t *idx, const Dist *sqdist, float f, const int32_t *back,
                        const float *xy, int64_t ldxy, int64_t *moff, int32_t *matches, Dist *dist, float *src_xy, float *dst_xy)
{
    const int64_t nb = blocks(R), nw = (R + 63) / 64;
    std::vector<uint64_t> word((size_t)nw, 0);
    std::vector<int32_t> count((size_t)nb, 0);
    std::vector<int64_t> off((size_t)nb + 1, 0);
    for (int64_t g = 0; g < R; g++) {
        const Pair &pr = rec[pair_of_row(rec, 0, n_pairs - 1, g)];
        if (keep(pr, g - pr.row0, idx + 2 * g, sqdist + 2 * g, f, back)) {
            word[(size_t)(g / 64)] |= (uint64_t)1 << (g % 64);
            count[(size_t)(g / kBlockRows)]++;
        }
    }
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < nb; c0 += kScanChunk) {
        int64_t run = 0;
        for (int64_t k = c0; k < nb && k < c0 + kScanChunk; k++) { off[(size_t)k] = carry + run; run += count[(size_t)k]; }
        carry += run;
    }
    off[(size_t)nb] = carry;
    auto position = [&](int64_t g) {
        int64_t pos = off[(size_t)(g / kBlockRows)];
        for (int64_t w = g / kBlockRows * (kBlockRows / 64); w < g / 64; w++) pos += __builtin_popcountll(word[(size_t)w]);
        return pos + __builtin_popcountll(word[(size_t)(g / 64)] & (((uint64_t)1 << (g % 64)) - 1));
    };
    for (int64_t g = 0; g < R; g++) {
        if (!((word[(size_t)(g / 64)] >> (g % 64)) & 1)) continue;
        const Pair &pr = rec[pair_of_row(rec, 0, n_pairs - 1, g)];
        const int64_t pos = position(g), i = g - pr.row0;
        const int32_t j = idx[2 * g];
        matches[2 * pos] = (int32_t)i;
        matches[2 * pos + 1] = j;
        dist[pos] = sqdist[2 * g];
        if (xy) {
            src_xy[2 * pos] = xy[(pr.src0 + i) * ldxy]; src_xy[2 * pos + 1] = xy[(pr.src0 + i) * ldxy + 1];
            dst_xy[2 * pos] = xy[(pr.dst0 + j) * ldxy]; dst_xy[2 * pos + 1] = xy[(pr.dst0 + j) * ldxy + 1];
        }
    }
    for (int64_t p = 0; p <= n_pairs; p++) {
        const int64_t g = p < n_pairs ? rec[p].row0 : R;
        moff[p] = g == R ? carry : position(g);
    }
}

}  // namespace select_rules
