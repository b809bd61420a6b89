// C entry points over opencv-dlco_amd/csrc/select_rules.hpp, the rule of the tools' -ratio / -cross and of
// dlco_desc_select_pairs*, for tests/test_match_rules.py: pure host code, no libdlco.so.
#include "../../opencv-dlco_amd/csrc/select_rules.hpp"

extern "C" {

int shim_match_ratio_keep(float d1, float d2, int32_t idx2, float f) { return select_rules::ratio_keep(d1, d2, idx2, f) ? 1 : 0; }

// one pair of nq queries against nt train rows, back [nt][2] or null; returns m; pairs_out [nq][2] / dists_out [nq] receive
// the first m entries
int64_t shim_match_select(int64_t nq, int32_t nt, const int32_t *nearest, const float *sqdist, int use_ratio, float f, const int32_t *back,
                          int32_t *pairs_out, float *dists_out)
{
    const select_rules::Pair pr{0, 0, 0, back ? 0 : -1, nt, 0};
    int64_t moff[2];
    select_rules::select_host<float>(&pr, 1, nq, nearest, sqdist, use_ratio ? f : 0.0f, back, nullptr, 2, moff, pairs_out, dists_out, nullptr, nullptr);
    return moff[1];
}

}  // extern "C"
