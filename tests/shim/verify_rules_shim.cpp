// C entry points over opencv-dlco_amd/csrc/verify_rules.hpp for tests/test_verify_rules.py: pure host code, no libdlco.so.
// Built with -ffp-contract=off.
#include "../../opencv-dlco_amd/csrc/verify_rules.hpp"

namespace vr = verify_rules;

extern "C" {

int shim_verify_score_chunk() { return vr::kScoreChunk; }

uint64_t shim_verify_mix(uint64_t z) { return vr::mix(z); }

// idx [4] of hypothesis h among m matches; returns 1 iff four distinct indices were found
int shim_verify_sample(uint64_t seed, uint32_t h, uint32_t m, int32_t *idx) { return vr::sample(seed, h, m, idx) ? 1 : 0; }

// H [9] from four matches, pts [4][4] = (x, y, u, v) as doubles; returns validity
int shim_verify_model(const double *pts, double *H)
{
    double sx[4], sy[4], dx[4], dy[4];
    for (int i = 0; i < 4; i++) { sx[i] = pts[4 * i]; sy[i] = pts[4 * i + 1]; dx[i] = pts[4 * i + 2]; dy[i] = pts[4 * i + 3]; }
    return vr::model(sx, sy, dx, dy, H) ? 1 : 0;
}

// H_all [n_hyp][9], idx_all [n_hyp][4], valid [n_hyp]
void shim_verify_hypotheses(const float *src, const float *dst, int64_t m, int32_t n_hyp, uint64_t seed, double *H_all, int32_t *idx_all,
                            uint8_t *valid)
{
    vr::all_hypotheses(src, dst, m, n_hyp, seed, H_all, idx_all, valid);
}

// count [n_hyp] of H_all
void shim_verify_counts(const float *src, const float *dst, int64_t m, float threshold, const double *H_all, int32_t n_hyp, int32_t *count)
{
    const double t2 = vr::threshold_sq(threshold);
    for (int32_t h = 0; h < n_hyp; h++) count[h] = (int32_t)vr::count_inliers(H_all + 9 * (int64_t)h, src, dst, m, t2, nullptr);
}

// mask [m] and the count of one H
int64_t shim_verify_mask(const float *src, const float *dst, int64_t m, float threshold, const double *H, uint8_t *mask)
{
    return vr::count_inliers(H, src, dst, m, vr::threshold_sq(threshold), mask);
}

// best hypothesis of count [n_hyp], -1 when every count is 0
int32_t shim_verify_select(const int32_t *count, int32_t n_hyp)
{
    const uint64_t key = vr::select(count, n_hyp);
    return vr::key_count(key) == 0 ? -1 : vr::key_hyp(key);
}

// one refit round on the inliers of mask; returns 1 when the round formed an H'
int shim_verify_refit_round(const float *src, const float *dst, int64_t m, const uint8_t *mask, double *H) { return vr::refit_round(src, dst, m, mask, H) ? 1 : 0; }

// the whole rule: H [9], mask [m], *count, *best_hyp, rounds [refine][9] and *n_rounds; H_all [n_hyp][9], counts [n_hyp] scratch
void shim_verify(const float *src, const float *dst, int64_t m, float threshold, int32_t n_hyp, uint64_t seed, int32_t refine, double *H_all,
                 int32_t *counts, double *H, uint8_t *mask, int64_t *count, int32_t *best_hyp, double *rounds, int32_t *n_rounds)
{
    vr::verify_host(src, dst, m, threshold, n_hyp, seed, refine, H_all, counts, H, mask, count, best_hyp, rounds, n_rounds);
}

}  // extern "C"
