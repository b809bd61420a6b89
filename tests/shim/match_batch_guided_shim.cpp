// C entry points over the guided arguments of opencv-dlco_amd/csrc/match_batch.hpp for tests/test_match_batch_guided_rules.py:
// the plan of dlco_desc_match_pairs_guided*, with and without a Guide.  Pure host code, no libdlco.so; built by the test.
#include "../../opencv-dlco_amd/csrc/match_batch.hpp"

#include <cstdint>

extern "C" {

int64_t shim_record_rows() { return match_batch::kRecordRows; }

// kind 0: the float matcher, kind 1: the byte matcher.  guided 0: plan() as the plain batch calls it; 1: with a Guide of
// no_model [n_pairs] (or null), both_sides, side, rec_limit and launch_rows (<= 0: the library's)
void *shim_guided_plan(int kind, const int64_t *seg, const int32_t *pairs, int64_t n_pairs, int n_cu, int guided, const uint8_t *no_model,
                       int both_sides, int side, int64_t rec_limit, int64_t launch_rows)
{
    const match_slicing::Shape &s = kind ? match_slicing::kU8 : match_slicing::kFloat;
    if (!guided) return new match_batch::Plan(match_batch::plan(s, seg, pairs, n_pairs, n_cu));
    match_batch::Guide g;
    g.no_model = no_model;
    g.both_sides = both_sides != 0;
    g.side = side;
    if (rec_limit > 0) g.rec_limit = rec_limit;
    if (launch_rows > 0) g.launch_rows = launch_rows;
    return new match_batch::Plan(match_batch::plan(s, seg, pairs, n_pairs, n_cu, &g));
}
void shim_guided_free(void *p) { delete static_cast<match_batch::Plan *>(p); }

// 0: entries, 1: launches, 2: fills, 3: fill rows, 4: the largest launch's partials, 5: guide offsets, 6: the largest launch's record rows
int64_t shim_guided_count(const void *p, int what)
{
    const auto &pl = *static_cast<const match_batch::Plan *>(p);
    switch (what) {
    case 0: return (int64_t)pl.entries.size();
    case 1: return (int64_t)pl.launches.size();
    case 2: return (int64_t)pl.fills.size();
    case 3: return pl.fill_rows;
    case 4: return pl.max_parts;
    case 5: return (int64_t)pl.guide.size();
    default: return pl.max_rec_rows;
    }
}
// [n][12]: q0, t0, out0, part0, nq, nt, tiles_per_slice, slices, wg0, mwg0, qblocks, pair
void shim_guided_entries(const void *p, int64_t *out)
{
    for (const match_batch::Entry &e : static_cast<const match_batch::Plan *>(p)->entries) {
        const int64_t v[12] = {e.q0, e.t0, e.out0, e.part0, e.nq, e.nt, e.tiles_per_slice, e.slices, e.wg0, e.mwg0, e.qblocks, e.pair};
        for (int64_t x : v) *out++ = x;
    }
}
// [n][8]: e0, n, rows, qblocks, wgs, merge_wgs, parts, rec_rows
void shim_guided_launches(const void *p, int64_t *out)
{
    for (const match_batch::Launch &l : static_cast<const match_batch::Plan *>(p)->launches) {
        const int64_t v[8] = {l.e0, l.n, l.rows, l.qblocks, l.wgs, l.merge_wgs, l.parts, l.rec_rows};
        for (int64_t x : v) *out++ = x;
    }
}
// [n][4]: out0, n, first, pair
void shim_guided_fills(const void *p, int64_t *out)
{
    for (const match_batch::Fill &f : static_cast<const match_batch::Plan *>(p)->fills) {
        const int64_t v[4] = {f.out0, f.n, f.first, f.pair};
        for (int64_t x : v) *out++ = x;
    }
}
// [n][3]: rec0, nqrec, ntrec
void shim_guided_offsets(const void *p, int64_t *out)
{
    for (const match_batch::GuideOff &g : static_cast<const match_batch::Plan *>(p)->guide) {
        const int64_t v[3] = {g.rec0, g.nqrec, g.ntrec};
        for (int64_t x : v) *out++ = x;
    }
}
void shim_guided_row0(const void *p, int64_t *out) { for (int64_t x : static_cast<const match_batch::Plan *>(p)->row0) *out++ = x; }
void shim_guided_slices(const void *p, int32_t *out) { for (int32_t x : static_cast<const match_batch::Plan *>(p)->slices) *out++ = x; }

}  // extern "C"
