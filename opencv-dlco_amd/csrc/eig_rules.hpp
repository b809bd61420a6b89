// eig_rules.hpp — the host decisions of the eigen tracker (eig_tracker.cpp): which interval and degree the
// Chebyshev filter takes, which rows it locks, where the orthonormalisation panels are cut, when a block has
// converged, how it grows and how it is trimmed.  Pure arithmetic on the Ritz values and residual norms that
// a pass read back: no HIP, no state, no environment, so the CPU suite tests every rule without a GPU
// (tests/shim/host_logic_shim.cpp).  The tracker keeps no second copy of any of them.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace dlco {
namespace eig_rules {

constexpr float kTolPass1 = 0.85f;     // see judge(): tolerance factor of the first pass ...
constexpr float kTolPass2 = 0.5f;      // ... and of the passes after the first
constexpr float kCheapMargin = 1.6f;   // see plan_filter(): how narrow a miss must be for a pass without products
constexpr double kPanelAmp = 1e5;      // largest filter-amplification ratio inside one orthonormalisation panel

// The block as the last Rayleigh-Ritz step left it: m rows ordered by descending Ritz value theta (of H = -G) with
// residual norms res, of a problem with `live` coordinates; pairs above mu are kept, `guard` rows ride behind them;
// cscale = sqrt(t+1)/gamma scales H to the matrix A whose error `tol` bounds.
struct Block {
    const float *theta = nullptr, *res = nullptr;
    int m = 0, live = 0, guard = 0;
    float mu = 0.f, cscale = 0.f, tol = 0.f;
};

// K slices of a Gram product X * Y^T over K = F columns whose output is `tiles` tiles of the generic GEMM: enough slices
// that 512 workgroups run, none shorter than 64 columns (128 at F = 8192: with 128 slices of 64 the launch is no faster
// and the ordered reduce reads twice as much, 593 -> 608 k on c2; ten slices of 64 at the reference's F = 640, where five
// of 128 measured 2.5 % slower), no more than the slab holds (slab_cap = slab floats / output floats).  split_k is what the
// GEMM is asked for; chunk and slices are what it makes of that (whole 16-column K tiles per slice).  Both the GEMM form
// and the reduction that emits the partials itself (reduce_gram_kernel) slice by this rule; the latter needs whole().
struct GramSlicing {
    int split_k = 1, chunk = 0, slices = 1;
    // every slice is 64 or 128 columns, none is short, and none straddles a 128-column slab
    bool whole(long F) const { return (chunk == 64 || chunk == 128) && (long)chunk * slices == F && F % 128 == 0; }
};
inline GramSlicing gram_slicing(long F, long tiles, long slab_cap)
{
    GramSlicing g;
    const long kslice = std::max(64L, F / 64 / 64 * 64);
    g.split_k = (int)std::max(1L, std::min(std::min((512 + tiles - 1) / tiles, F / kslice), slab_cap));
    g.chunk = (int)std::max(16L, ((F + g.split_k - 1) / g.split_k + 15) / 16 * 16);
    g.slices = F > 0 ? (int)((F + g.chunk - 1) / g.chunk) : 1;
    return g;
}

// How many updates may pass between two refreshes of the lower spectral bound: lambda_max(G) drifts as 1/t
inline int lower_bound_period(int64_t updates)
{
    return updates < 20 ? 1 : (updates < 200 ? 5 : (updates < 400 ? 20 : 50));
}

// A Ritz value below the lower bound moves the bound under it
inline float lowered_bound(float lo_bound, float theta_last)
{
    return theta_last < lo_bound ? theta_last - 0.5f * std::fabs(theta_last) - 1e-12f : lo_bound;
}

struct FilterPlan {
    bool filtered = false;         // the pass filters at all (the other fields mean nothing otherwise)
    float c0 = 0.f, e0 = 1.f;      // centre and half width of the damped interval [a, b]
    int d = 0;                     // degree
    int n_lock = 0;                // leading rows that are locked
    bool cheap = false;            // the degree-1 pass without a product
};

// The filter of pass `it`.  n_ritz: leading rows that are Ritz vectors with a known theta; nw: pairs above mu as of the
// last pass; deg0: starting degree of the step; [lo_bound, block_min]: the interval to damp; cheap_ok: no cheap pass yet
// in this update and Y = Q H is still there; last_crit: the last pass's criterion relative to emax.
inline FilterPlan plan_filter(const Block &b, int n_ritz, int nw, int it, int deg0, float lo_bound, float block_min, float theta_top,
                              bool locking, bool cheap_ok, float last_crit)
{
    FilterPlan p;
    // The filter is only applied to a block of Ritz vectors (theta known): the amplification of
    // each row is then predictable and the panels of the orthonormalisation can follow it.
    if (!(b.m < b.live && n_ritz > 0)) return p;
    p.filtered = true;
    // ---- Chebyshev filter of degree d damping [a, b] of H = -G ---------------------------
    const float a = lo_bound;
    float bb = std::min(block_min, b.mu);
    const float minw = 1e-3f * (std::fabs(a) + std::fabs(b.mu)) + 1e-20f;
    if (bb < a + minw) bb = a + minw;
    const float c0 = 0.5f * (a + bb), e0 = 0.5f * (bb - a);
    int d = std::min(12, deg0 + 2 * it);
    const float xmax = std::max(1.5f, (std::max(theta_top, b.mu) - c0) / e0);
    // keep the top/guard amplification ratio T_d(xmax) below ~1e5: the guard rows survive the
    // cancellation against the amplified rows with ~1e5 * 6e-8 relative noise
    const int dcap = (int)(12.2f / std::acosh(xmax));
    // ---- locking (passes after the first): while theta_top / mu is in the hundreds (the start-up transient) the
    // cap above holds the filter at degree 2-4, and the pairs just above mu - hundreds of them, a dense spectrum -
    // gain a factor ~1.6 per pass: ten passes per step.  The pairs at the top converge in the first pass or two
    // (their amplification is the largest).  Once they have - residuals of the CURRENT matrix, a quarter of the
    // tolerance - they are locked: not filtered, and projected out of every term of the recurrence that runs on
    // the rows below them, so that the cap is set by the largest UNLOCKED Ritz value and the degree can rise.
    // (The locked rows stay in the Rayleigh-Ritz step and in the convergence test.)
    int n_lock = 0, dcap_a = dcap;
    if (locking && it >= 1 && n_ritz == b.m && nw > 0 && b.m > 32 && dcap < d + 4) {
        const float emax_l = b.cscale * (b.theta[0] - b.mu);
        int np = 0;
        while (np < nw && np < b.m - 16 && b.cscale * b.res[np] <= 0.25f * b.tol * emax_l) np++;
        if (np >= 8) {
            const float xa = std::max(1.5f, (std::max(b.theta[np], b.mu) - c0) / e0);
            const int cap_a = (int)(12.2f / std::acosh(xa));
            if (cap_a >= dcap + 2) { n_lock = np; dcap_a = cap_a; }
        }
    }
    if (n_lock > 0) d = std::min(16, d + 4);
    d = std::max(2, std::min(d, dcap_a));
    // A pass that missed the tolerance only narrowly is followed by a degree-1 pass that costs
    // no product at all: Y = Q H is still there from the Rayleigh-Ritz step, and
    // (H - c0) Q / e0 = (Y - c0 Q) / e0 already damps everything below the block by the
    // factor the marginal case needs.
    // (It gains a factor 0.5-0.9 on the criterion, measured, and what it must reach is the tolerance of the passes
    // after the first: only a miss within 1.6x of THAT is worth a pass without products.)
    p.cheap = it >= 1 && cheap_ok && last_crit <= kCheapMargin * kTolPass2 * b.tol;
    if (p.cheap) { d = 1; n_lock = 0; }                      // (once per step: if it is not enough, filter properly)
    p.c0 = c0; p.e0 = e0; p.d = d; p.n_lock = n_lock;
    return p;
}

// Where the orthonormalisation cuts its panels (ends, ascending, the last one m).
// panels: at most panel_max rows, predicted amplification T_d(x_j) within kPanelAmp inside a
// panel.  A Ritz row carries the directions above it only at the level of its own
// residual, so after the filter it is at worst (residual level x amplification ratio)
// parallel to them: CholQR2 resolves that as long as the product stays below ~1e2.
inline void cut_panels(const Block &b, int n_ritz, const FilterPlan &p, int panel_max, std::vector<int> &panel_ends)
{
    panel_ends.clear();
    if (p.filtered) {
        int start = p.n_lock;
        double amp0 = 0.0;
        if (p.n_lock > 0) panel_ends.push_back(p.n_lock);
        for (int j = p.n_lock; j < n_ritz; j++) {
            const double x = std::max(1.0, (double)(b.theta[j] - p.c0) / p.e0);
            const double amp = std::cosh((double)p.d * std::acosh(x));
            if (j == start) amp0 = amp;
            else if (j - start >= panel_max || amp0 > kPanelAmp * amp) { panel_ends.push_back(j); start = j; amp0 = amp; }
        }
        if (n_ritz < b.m) panel_ends.push_back(n_ritz);
    }
    for (int j = n_ritz + 64; j < b.m; j += 64) panel_ends.push_back(j);   // rows without a Ritz value: panels of 64
    panel_ends.push_back(b.m);
}

// Guard directions only have to span: pairs of two columns below the Ritz value of the guard at a
// quarter of the guard depth (known from the last pass; the leading guards above it still count,
// they decide guards_ok) are rotated but do not prolong the Jacobi sweeps.  What this may leave unfinished
// shows up in the residuals, which decide convergence.  all_ritz: every row of the block has a known theta.
inline float jacobi_lam_cut(const Block &b, bool all_ritz)
{
    float lam_cut = -3.0e38f;
    if (all_ritz) {
        int nwp = 0;
        while (nwp < b.m && b.theta[nwp] > b.mu) nwp++;
        const int ig = nwp + std::max(2, b.guard / 4);
        if (ig < b.m) lam_cut = b.theta[ig];
    }
    return lam_cut;
}

struct Verdict {
    int nw = 0;                    // pairs above mu
    float crit = 0.f;              // criterion relative to emax = cscale (theta_0 - mu)
    bool guards_ok = true, conv = false;
};

// Has pass `it` converged?
inline Verdict judge(const Block &b, int it)
{
    const float *theta = b.theta, *res = b.res;
    const int m = b.m;
    const float mu = b.mu, cscale = b.cscale, tol = b.tol;
    Verdict v;
    int nw = 0;
    while (nw < m && theta[nw] > mu) nw++;
    v.nw = nw;
    // What has to be small is the error of A = c * (G - mu)_+, not every Ritz pair by itself.  The
    // Ritz pairs of the block are exact eigenpairs of G + E with E = -sum_i (r_i q_i^T + q_i r_i^T),
    // r_i orthogonal to the block, and the derivative of the matrix function (x - mu)_+ damps the
    // component of E that couples a pair at theta_i > mu with a direction at lambda < mu by the
    // divided difference (theta_i - mu) / (theta_i - lambda) <= (theta_i - mu) / (theta_i - b), b
    // the top of the spectrum outside the converged part of the block (taken at the middle guard):
    // a pair just above the threshold carries almost no weight in A and its residual counts with
    // that weight.  Pairs well above mu keep the weight 1 of the plain residual test.
    float crit = 0.f;
    const float bsep = nw < m ? std::min(mu, theta[nw + (m - nw) / 2]) : mu;
    for (int i = 0; i < nw; i++) {
        float wgt = 1.f;
        const float den = theta[i] - bsep;
        if (den > 0.f) wgt = std::min(1.f, (theta[i] - mu + res[i]) / den);
        crit = std::max(crit, cscale * res[i] * wgt);
    }
    const float emax = nw > 0 ? cscale * (theta[0] - mu) : 0.f;
    v.crit = emax > 0.f ? crit / emax : 0.f;
    // the leading guards must be resolved too, or an eigenvalue just above mu can hide in them: each
    // needs theta + |r| < mu (no eigenvalue of that pair's interval reaches mu), or an interval that
    // reaches above mu by less than the tolerance (what could hide there weighs less than that in A),
    // or a small residual
    const int ng = std::min(m, nw + std::max(2, b.guard / 4));
    const float gtol = tol * std::max(emax, cscale * 1e-3f * std::fabs(mu));
    for (int i = nw; i < ng; i++) {
        const float excess = theta[i] + res[i] - mu;
        const bool below = excess < 0.f || cscale * excess <= gtol;
        const bool small = cscale * res[i] <= gtol;
        v.guards_ok = v.guards_ok && (below || small);
    }
    if (m >= b.live) v.conv = true;                              // dense: Rayleigh-Ritz is exact
    else if (nw == 0) v.conv = v.guards_ok || it >= 6;
    // A step that converges in its first pass inherits Ritz vectors that already met the tolerance, and the measured
    // error of A+ then sits 3-10x below it; one that needed more passes (start-up transient, a growing block) has
    // nothing to lean on and stops right at the tolerance (free runs against ssyevr step by step: up to 1.03e-4 of
    // the 1e-4 gate at eig_tol = 2e-4).  Passes after the first therefore converge to half of it.
    // (And a first pass that stops right AT the tolerance was measured at 0.46 of it in A+ - 9.2e-5 against the 1e-4 gate, in a
    // small free run; at full width the ratio is 0.25-0.29, tools/full_width_crit_vs_error.py - so the first pass is held to
    // 0.85 of it: worst free-run step 7.4e-5, and the rank ~128 workload pays 1.12 instead of 1.11 passes per step.)
    else v.conv = crit <= (it == 0 ? kTolPass1 * tol : kTolPass2 * tol) * emax && v.guards_ok;
    return v;
}

// The positive eigenspace reaches into the guard: the block has to grow (or, at its capacity, cannot certify the rank)
inline bool reaches_guards(int nw, int m, int guard) { return nw > m - std::max(2, guard / 2); }

// Rows a growing block of m rows takes on
inline int growth_rows(int m, int cap, int guard, int nw) { return std::min(cap - m, std::max(guard, nw / 4)); }

// Starting degree for the next step: the cheapest one that has been converging in a single
// filter + Rayleigh-Ritz pass (each extra pass costs a Jacobi and an orthonormalisation).
// tol: the tracker's own tolerance, not the tightened one of a cold update.
inline int next_deg0(int deg0, int passes, bool conv, float last_crit, float tol)
{
    if (passes >= 2) return std::min(10, deg0 + 2);
    if (conv && last_crit < 0.15f * tol) return std::max(2, deg0 - 1);
    return deg0;
}

// Rows the block keeps for the next step
inline int trimmed_rows(int m, int nw, int guard)
{
    // the products pad the block to a multiple of 32 rows: prefer a block that fills its
    // padding exactly, as long as at least half of the guard vectors stay
    int keep = nw + guard;
    const int r32 = (keep / 32) * 32;
    if (r32 >= nw + std::max(4, guard / 2)) keep = r32;
    else if (keep <= 96) {
        // the m x m solvers work on PAIRS of eight-column blocks (kernels_jacobi.hip): 81-96 rows cost eleven block rounds
        // per sweep, 65-80 rows nine.  A small block - where that chain is half the step - that can drop to a multiple of
        // 16 rows and keep three quarters of its guards does (the reference's own shape: rank 55 + 32 guards = 87 rows
        // -> 80; Jacobi 0.117 -> 0.100 ms, 1.005 -> 1.015 passes per step, +3.5 % on ref544).  Not above 96 rows: at rank
        // ~115 the same rule (152 -> 144 rows, 24 guards) cost more passes than it saved rounds (1.16 -> 1.24 per step).
        const int r16 = (keep / 16) * 16;
        if (r16 >= nw + std::max(4, (3 * guard) / 4)) keep = r16;
    }
    return std::max(1, std::min(m, keep));
}

}  // namespace eig_rules
}  // namespace dlco
