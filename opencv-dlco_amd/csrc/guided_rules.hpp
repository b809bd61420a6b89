// guided_rules.hpp — which pairs (query i, train j) a homography admits (dlco_desc_match_guided,
// dlco_desc_cross_sqdists_guided): guided matching looks for the nearest two rows among the train keypoints that a model
// puts within `radius` pixels of the query.  The rule stated once for the host, the matcher's guided epilogue
// (kernels_match.hip) and the CPU tests (tests/shim/guided_rules_shim.cpp).  Plain C++: no HIP header, no device, no I/O.
//
// The predicate is verify_rules::inlier, split in two so that the part that depends on one point alone is formed once per
// point and not once per pair:
//   record(H, x, y, t2)   X = (H00 x + H01 y) + H02, Y and W likewise, exactly as inlier forms them, and
//                         T = W > 0 ? t2 (W W) : -1
//   admits(rec, u, v)     ex = X - u W, ey = Y - v W; ex ex + ey ey <= T
// A sum of two squares is never below 0, so T = -1 stands in for inlier's `W > 0` term (a NaN sum fails the comparison as
// well), and for all inputs, NaN and infinities included, admits(record(H, x, y, t2), u, v) == inlier(H, x, y, u, v, t2).
// t2 = verify_rules::threshold_sq(radius).  Every step is IEEE double + - x, one rounding each, no fused multiply-add and no
// division; the functions switch contraction off themselves (VERIFY_RULES_NO_FMA), and a kernel reaches this arithmetic
// through them only.
//
// The pair predicate P(i, j), with qxy [nq] and txy [nt] the (x, y) of the rows of the two tables:
//   h_side = 0   H maps the query image to the train image:  P = inlier(H, qxy_i, txy_j, t2)
//   h_side = 1   H maps the train image to the query image:  P = inlier(H, txy_j, qxy_i, t2)
// h_side = 1 lets a mutual check swap the tables and keep H: the call with the tables swapped and h_side = 1 sees the
// transpose of the same admissible set.
//
// The guided answer for query i: the first two admitted j under the matcher's key (float distance, train index), i.e. the
// top two of the finite entries of row i of the matrix with +inf where P fails; -1 / +inf where fewer than two are admitted.
#pragma once

#include "verify_rules.hpp"

namespace guided_rules {

// a point on the side H applies to
struct Rec { double X, Y, W, T; };

VERIFY_RULES_HD inline Rec record(const double H[9], double x, double y, double t2)
{
    VERIFY_RULES_NO_FMA
    Rec r;
    r.X = (H[0] * x + H[1] * y) + H[2];
    r.Y = (H[3] * x + H[4] * y) + H[5];
    r.W = (H[6] * x + H[7] * y) + H[8];
    r.T = r.W > 0.0 ? t2 * (r.W * r.W) : -1.0;
    return r;
}

VERIFY_RULES_HD inline bool admits(const Rec &r, double u, double v)
{
    VERIFY_RULES_NO_FMA
    const double ex = r.X - u * r.W, ey = r.Y - v * r.W;
    return ex * ex + ey * ey <= r.T;
}

// P(i, j) for one pair, from the points themselves
inline bool pair_admitted(const double H[9], double t2, int h_side, const float *qxy, const float *txy)
{
    return h_side == 0 ? admits(record(H, (double)qxy[0], (double)qxy[1], t2), (double)txy[0], (double)txy[1])
                       : admits(record(H, (double)txy[0], (double)txy[1], t2), (double)qxy[0], (double)qxy[1]);
}

// The guided top two on the host: dist [nq][nt] the matrix of distances, qxy [nq][2], txy [nt][2];
// idx [nq][2], sqdist [nq][2].  A NaN distance never enters, like in the kernel's strict comparisons.
inline void guided_top2_host(const float *dist, const float *qxy, int64_t nq, const float *txy, int64_t nt, const double H[9], float radius,
                             int h_side, int32_t *idx, float *sqdist)
{
    const double t2 = verify_rules::threshold_sq(radius);
    const float inf = __builtin_inff();
    for (int64_t i = 0; i < nq; i++) {
        float d1 = inf, d2 = inf;
        int32_t j1 = -1, j2 = -1;
        for (int64_t j = 0; j < nt; j++) {
            if (!pair_admitted(H, t2, h_side, qxy + 2 * i, txy + 2 * j)) continue;
            const float f = dist[i * nt + j];
            if (f < d1) { d2 = d1; j2 = j1; d1 = f; j1 = (int32_t)j; }
            else if (f < d2) { d2 = f; j2 = (int32_t)j; }
        }
        idx[2 * i] = j1; idx[2 * i + 1] = j2;
        sqdist[2 * i] = d1; sqdist[2 * i + 1] = d2;
    }
}

}  // namespace guided_rules
