// C entry points over the integer overloads of opencv-dlco_amd/cli/match_rules.hpp (the filters of `match -u8`) for
// tests/test_quant_rules.py: pure host code, no libdlco.so.
#include "../../opencv-dlco_amd/cli/match_rules.hpp"

#include <cstring>

extern "C" {

int shim_match_ratio_keep_i32(int32_t d1, int32_t d2, int32_t idx2, float f) { return match_rules::ratio_keep(d1, d2, idx2, f) ? 1 : 0; }

// returns m; pairs_out [nq][2] / dists_out [nq] receive the first m entries
int64_t shim_match_select_i32(int64_t nq, const int32_t *nearest, const int32_t *sqdist, int use_ratio, float f, const int32_t *back,
                              int32_t *pairs_out, int32_t *dists_out)
{
    std::vector<int32_t> pairs, dists;
    match_rules::select(nq, nearest, sqdist, use_ratio != 0, f, back, pairs, dists);
    if (!pairs.empty()) std::memcpy(pairs_out, pairs.data(), pairs.size() * sizeof(int32_t));
    if (!dists.empty()) std::memcpy(dists_out, dists.data(), dists.size() * sizeof(int32_t));
    return (int64_t)dists.size();
}

}  // extern "C"
