// C entry points over opencv-dlco_amd/cli/match_rules.hpp for tests/test_match_rules.py: pure host code, no libdlco.so.
#include "../../opencv-dlco_amd/cli/match_rules.hpp"

#include <cstring>

extern "C" {

int shim_match_ratio_keep(float d1, float d2, int32_t idx2, float f) { return match_rules::ratio_keep(d1, d2, idx2, f) ? 1 : 0; }

// returns m; pairs_out [nq][2] / dists_out [nq] receive the first m entries
int64_t shim_match_select(int64_t nq, const int32_t *nearest, const float *sqdist, int use_ratio, float f, const int32_t *back,
                          int32_t *pairs_out, float *dists_out)
{
    std::vector<int32_t> pairs;
    std::vector<float> dists;
    match_rules::select(nq, nearest, sqdist, use_ratio != 0, f, back, pairs, dists);
    if (!pairs.empty()) std::memcpy(pairs_out, pairs.data(), pairs.size() * sizeof(int32_t));
    if (!dists.empty()) std::memcpy(dists_out, dists.data(), dists.size() * sizeof(float));
    return (int64_t)dists.size();
}

}  // extern "C"
