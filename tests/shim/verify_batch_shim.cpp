// C entry points over opencv-dlco_amd/csrc/verify_batch.hpp, and over the whole rule of verify_rules.hpp / epipolar_rules.hpp
// whose refit loop ends a round in verify_rules::refit_step, for tests/test_verify_batch_rules.py: pure host code, no
// libdlco.so.  Built with -ffp-contract=off.
#include "../../opencv-dlco_amd/csrc/verify_batch.hpp"
#include "../../opencv-dlco_amd/csrc/epipolar_rules.hpp"

namespace vb = verify_batch;

extern "C" {

int shim_vbatch_lanes() { return vb::kLanes; }
int64_t shim_vbatch_launch_hyp() { return vb::kLaunchHyp; }
int64_t shim_vbatch_launch_wgs() { return vb::kLaunchWgs; }
int shim_vbatch_sample(int fundamental) { return fundamental ? epipolar_rules::Fundamental::kSample : verify_rules::Homography::kSample; }

int shim_vbatch_offsets_ok(const int64_t *moff, int64_t n_pairs) { return vb::offsets_ok(moff, n_pairs) ? 1 : 0; }

// max_hyp, max_wgs <= 0: the library's limits
void *shim_vbatch_plan(const int64_t *moff, int64_t n_pairs, int32_t n_hyp, int fundamental, int64_t max_hyp, int64_t max_wgs)
{
    return new vb::Plan(vb::plan(moff, n_pairs, n_hyp, shim_vbatch_sample(fundamental), max_hyp > 0 ? max_hyp : vb::kLaunchHyp,
                                 max_wgs > 0 ? max_wgs : vb::kLaunchWgs));
}
void shim_vbatch_free(void *p) { delete static_cast<vb::Plan *>(p); }

// 0: entries, 1: launches, 2 .. 4: the largest launch's entries, matches, hypotheses
int64_t shim_vbatch_count(const void *p, int what)
{
    const auto &pl = *static_cast<const vb::Plan *>(p);
    switch (what) {
    case 0: return (int64_t)pl.entries.size();
    case 1: return (int64_t)pl.launches.size();
    case 2: return pl.max_entries;
    case 3: return pl.max_matches;
    default: return pl.max_hyps;
    }
}
// [n][5]: m0, m, pair, swg0, mwg0
void shim_vbatch_entries(const void *p, int64_t *out)
{
    for (const vb::Entry &e : static_cast<const vb::Plan *>(p)->entries) {
        const int64_t v[5] = {e.m0, e.m, e.pair, e.swg0, e.mwg0};
        for (int64_t x : v) *out++ = x;
    }
}
// [n][7]: e0, n, match0, matches, hyps, score_wgs, mask_wgs
void shim_vbatch_launches(const void *p, int64_t *out)
{
    for (const vb::Launch &l : static_cast<const vb::Plan *>(p)->launches) {
        const int64_t v[7] = {l.e0, l.n, l.match0, l.matches, l.hyps, l.score_wgs, l.mask_wgs};
        for (int64_t x : v) *out++ = x;
    }
}
void shim_vbatch_launch_of_pair(const void *p, int32_t *out) { for (int32_t x : static_cast<const vb::Plan *>(p)->launch_of_pair) *out++ = x; }

// the whole rule of either model, the arguments of shim_verify (tests/shim/verify_rules_shim.cpp)
void shim_vbatch_verify(int fundamental, const float *src, const float *dst, int64_t m, float threshold, int32_t n_hyp, uint64_t seed, int32_t refine,
                        double *M_all, int32_t *counts, double *M, uint8_t *mask, int64_t *count, int32_t *best_hyp, double *rounds, int32_t *n_rounds)
{
    if (fundamental)
        epipolar_rules::verify_host(src, dst, m, threshold, n_hyp, seed, refine, M_all, counts, M, mask, count, best_hyp, rounds, n_rounds);
    else
        verify_rules::verify_host(src, dst, m, threshold, n_hyp, seed, refine, M_all, counts, M, mask, count, best_hyp, rounds, n_rounds);
}

// one round's acceptance: returns 1 when the refit goes on
int shim_vbatch_refit_step(int64_t m, double *M, uint8_t *mask, int64_t *count, const double *Mn, const uint8_t *trial, int64_t c)
{
    return verify_rules::refit_step(m, M, mask, *count, Mn, trial, c) ? 1 : 0;
}

}  // extern "C"
