// Test-only shim: exposes the product's host-side pair indexing (opencv-dlco_amd/csrc/pair_index.hpp,
// header-only, no HIP) through a C ABI so that the CPU test-suite can compare it bit for bit
// with the oracle without a GPU, and the eigen tracker's host rules (csrc/eig_rules.hpp, likewise
// HIP-free) so that it can check what their comments promise.  Built by the tests with g++.
#include "../../opencv-dlco_amd/csrc/eig_rules.hpp"
#include "../../opencv-dlco_amd/csrc/pair_index.hpp"

#include <cstring>

extern "C" {

int shim_build_index(const uint8_t *labels, int N, int32_t *pos, int *n_pos, int *n_pos_trn, int32_t *neg, int *n_neg,
                     int *n_neg_trn)
{
    dlco::PairIndex idx;
    idx.build(labels, N);
    if (!idx.pos.empty()) std::memcpy(pos, idx.pos.data(), idx.pos.size() * sizeof(int32_t));
    if (!idx.neg.empty()) std::memcpy(neg, idx.neg.data(), idx.neg.size() * sizeof(int32_t));
    *n_pos = (int)idx.pos.size(); *n_neg = (int)idx.neg.size();
    *n_pos_trn = idx.n_pos_trn; *n_neg_trn = idx.n_neg_trn;
    return 0;
}

// `steps` batches of B interleaved (iPos, iNeg) draws, src/pj-learn.cpp:310-314
void shim_sample(uint64_t seed, int n_pos_trn, int n_neg_trn, int B, int steps, int32_t *ipos, int32_t *ineg)
{
    dlco::CvRng rng(seed);
    for (int s = 0; s < steps; s++)
        for (int k = 0; k < B; k++) {
            ipos[s * B + k] = rng.uniform(0, n_pos_trn);
            ineg[s * B + k] = rng.uniform(0, n_neg_trn);
        }
}

int shim_split(uint64_t n) { return dlco::PairIndex::split((size_t)n); }

void shim_rda_coeffs(uint32_t B, uint32_t t, float *w_dloss, float *w_dfavg) { dlco::rda_coeffs(B, t, w_dloss, w_dfavg); }

uint32_t shim_rng_next(uint64_t *state)
{
    dlco::CvRng r(*state);
    const uint32_t v = r.next();
    *state = r.state;
    return v;
}

// ---- the eigen tracker's host rules (csrc/eig_rules.hpp) ----
static dlco::eig_rules::Block shim_block(const float *theta, const float *res, int m, int live, int guard, float mu, float cscale,
                                         float tol)
{
    dlco::eig_rules::Block b;
    b.theta = theta; b.res = res; b.m = m; b.live = live; b.guard = guard; b.mu = mu; b.cscale = cscale; b.tol = tol;
    return b;
}

// iout = {filtered, d, n_lock, cheap}, fout = {c0, e0}
void shim_eig_plan_filter(const float *theta, const float *res, int m, int live, int guard, float mu, float cscale, float tol,
                          int n_ritz, int nw, int it, int deg0, float lo_bound, float block_min, float theta_top, int locking,
                          int cheap_ok, float last_crit, int *iout, float *fout)
{
    const dlco::eig_rules::FilterPlan p = dlco::eig_rules::plan_filter(shim_block(theta, res, m, live, guard, mu, cscale, tol), n_ritz, nw, it,
                                                                       deg0, lo_bound, block_min, theta_top, locking != 0, cheap_ok != 0, last_crit);
    iout[0] = p.filtered; iout[1] = p.d; iout[2] = p.n_lock; iout[3] = p.cheap;
    fout[0] = p.c0; fout[1] = p.e0;
}

// returns the number of cuts written to ends (at most m)
int shim_eig_cut_panels(const float *theta, int m, int n_ritz, int filtered, float c0, float e0, int d, int n_lock, int panel_max, int *ends)
{
    dlco::eig_rules::FilterPlan p;
    p.filtered = filtered != 0; p.c0 = c0; p.e0 = e0; p.d = d; p.n_lock = n_lock;
    std::vector<int> v;
    dlco::eig_rules::cut_panels(shim_block(theta, nullptr, m, 0, 0, 0.f, 0.f, 0.f), n_ritz, p, panel_max, v);
    for (size_t i = 0; i < v.size(); i++) ends[i] = v[i];
    return (int)v.size();
}

float shim_eig_lam_cut(const float *theta, int m, int guard, float mu, int all_ritz)
{
    return dlco::eig_rules::jacobi_lam_cut(shim_block(theta, nullptr, m, 0, guard, mu, 0.f, 0.f), all_ritz != 0);
}

// iout = {nw, guards_ok, conv}
void shim_eig_judge(const float *theta, const float *res, int m, int live, int guard, float mu, float cscale, float tol, int it, int *iout,
                    float *crit)
{
    const dlco::eig_rules::Verdict v = dlco::eig_rules::judge(shim_block(theta, res, m, live, guard, mu, cscale, tol), it);
    iout[0] = v.nw; iout[1] = v.guards_ok; iout[2] = v.conv;
    *crit = v.crit;
}

int shim_eig_lower_bound_period(int64_t updates) { return dlco::eig_rules::lower_bound_period(updates); }
float shim_eig_lowered_bound(float lo_bound, float theta_last) { return dlco::eig_rules::lowered_bound(lo_bound, theta_last); }
int shim_eig_reaches_guards(int nw, int m, int guard) { return dlco::eig_rules::reaches_guards(nw, m, guard); }
int shim_eig_growth_rows(int m, int cap, int guard, int nw) { return dlco::eig_rules::growth_rows(m, cap, guard, nw); }
int shim_eig_next_deg0(int deg0, int passes, int conv, float last_crit, float tol) { return dlco::eig_rules::next_deg0(deg0, passes, conv != 0, last_crit, tol); }
int shim_eig_trimmed_rows(int m, int nw, int guard) { return dlco::eig_rules::trimmed_rows(m, nw, guard); }

}
