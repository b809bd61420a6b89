// C entry points over opencv-dlco_amd/csrc/select_rules.hpp for tests/test_select_rules.py: pure host code, no libdlco.so.
#include "../../opencv-dlco_amd/csrc/select_rules.hpp"

namespace sr = select_rules;

namespace {
template <typename Dist>
int64_t run(const int64_t *seg, const int32_t *pairs, int64_t n_pairs, const int32_t *idx, const Dist *sqdist, float f, const int32_t *back,
            const int64_t *back_row0, const float *xy, int64_t ldxy, int64_t *moff, int32_t *matches, Dist *dist, float *src_xy, float *dst_xy)
{
    std::vector<sr::Pair> rec;
    const int64_t R = sr::pair_records(seg, pairs, n_pairs, back ? back_row0 : nullptr, rec);
    sr::select_host(rec.data(), n_pairs, R, idx, sqdist, f, back, xy, ldxy, moff, matches, dist, src_xy, dst_xy);
    return R;
}
}  // namespace

extern "C" {

int shim_select_block_rows() { return sr::kBlockRows; }
int shim_select_scan_chunk() { return sr::kScanChunk; }

int shim_select_ratio_keep(float d1, float d2, int32_t idx2, float f) { return sr::ratio_keep(d1, d2, idx2, f) ? 1 : 0; }
int shim_select_ratio_keep_i32(int32_t d1, int32_t d2, int32_t idx2, float f) { return sr::ratio_keep(d1, d2, idx2, f) ? 1 : 0; }
int shim_select_ratio_ok(float f) { return sr::ratio_ok(f) ? 1 : 0; }

// the rule for one row of a pair whose train image has nt rows; back [.][2] is the pair's own reverse table or null
int shim_select_keep(int32_t nt, int64_t i, const int32_t *idx2, const float *d2, float f, const int32_t *back)
{
    const sr::Pair pr{0, 0, 0, back ? 0 : -1, nt, 0};
    return sr::keep(pr, i, idx2, d2, f, back) ? 1 : 0;
}
int shim_select_keep_i32(int32_t nt, int64_t i, const int32_t *idx2, const int32_t *d2, float f, const int32_t *back)
{
    const sr::Pair pr{0, 0, 0, back ? 0 : -1, nt, 0};
    return sr::keep(pr, i, idx2, d2, f, back) ? 1 : 0;
}

int shim_select_back_rows_ok(const int64_t *seg, const int32_t *pairs, int64_t n_pairs, const int64_t *back_row0, int64_t n_back_rows)
{
    return sr::back_rows_ok(seg, pairs, n_pairs, back_row0, n_back_rows) ? 1 : 0;
}

// the pair of row g among the pairs of a call
int64_t shim_select_pair_of_row(const int64_t *seg, const int32_t *pairs, int64_t n_pairs, int64_t g)
{
    std::vector<sr::Pair> rec;
    sr::pair_records(seg, pairs, n_pairs, nullptr, rec);
    return sr::pair_of_row(rec.data(), 0, n_pairs - 1, g);
}

// the whole call on the host (select_rules::select_host); returns R
int64_t shim_select_pairs(const int64_t *seg, const int32_t *pairs, int64_t n_pairs, const int32_t *idx, const float *sqdist, float f,
                          const int32_t *back, const int64_t *back_row0, const float *xy, int64_t ldxy, int64_t *moff, int32_t *matches, float *dist,
                          float *src_xy, float *dst_xy)
{
    return run(seg, pairs, n_pairs, idx, sqdist, f, back, back_row0, xy, ldxy, moff, matches, dist, src_xy, dst_xy);
}
int64_t shim_select_pairs_i32(const int64_t *seg, const int32_t *pairs, int64_t n_pairs, const int32_t *idx, const int32_t *sqdist, float f,
                              const int32_t *back, const int64_t *back_row0, const float *xy, int64_t ldxy, int64_t *moff, int32_t *matches,
                              int32_t *dist, float *src_xy, float *dst_xy)
{
    return run(seg, pairs, n_pairs, idx, sqdist, f, back, back_row0, xy, ldxy, moff, matches, dist, src_xy, dst_xy);
}

}  // extern "C"
