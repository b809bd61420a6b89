// guided_epipolar_rules.hpp — which pairs (query i, train j) a fundamental matrix admits (dlco_desc_match_guided_epipolar,
// dlco_desc_cross_sqdists_guided_epipolar): guided matching looks for the nearest two rows among the train keypoints whose
// Sampson error against the query under F is within `threshold` pixels.  The rule stated once for the host, the matcher's
// epipolar epilogue (kernels_match.hip) and the CPU tests (tests/shim/guided_epipolar_rules_shim.cpp).  Plain C++: no HIP
// header, no device, no I/O.
//
// The predicate is epipolar_rules::inlier, x'^T F x = 0 with x = (x, y, 1) of the image F applies to (src) and x' = (u, v, 1)
// of the other (dst), split so that everything that depends on one point alone is formed once per point:
//   src_record(F, x, y)   l0 = (F0 x + F1 y) + F2, l1 = (F3 x + F4 y) + F5, l2 = (F6 x + F7 y) + F8, L = l0 l0 + l1 l1
//   dst_record(F, u, v)   m0 = (F0 u + F3 v) + F6, m1 = (F1 u + F4 v) + F7, A = m0 m0, B = m1 m1; u and v carried along
//   admits(s, d, t2)      e = (d.u s.l0 + d.v s.l1) + s.l2; S = (s.L + d.A) + d.B; S > 0 && e e <= t2 S
// The same operations as inlier's in the same order, one rounding each, so for all inputs, NaN and infinities included,
// admits(src_record(F, x, y), dst_record(F, u, v), t2) == epipolar_rules::inlier(F, x, y, u, v, t2).  A pair costs 8 fp64
// operations and two comparisons.  t2 = verify_rules::threshold_sq(threshold) stays an argument of the pair: t2 (L + A + B)
// does not distribute in floating point, so it cannot be folded into a record.  No fused multiply-add and no division; the
// functions switch contraction off themselves (VERIFY_RULES_NO_FMA), and a kernel reaches this arithmetic through them only.
//
// The pair predicate P(i, j), with qxy [nq] and txy [nt] the (x, y) of the rows of the two tables:
//   f_side = 0   the query image is src:  P = inlier(F, qxy_i, txy_j, t2); F as verify_fundamental(src = query keypoints,
//                dst = train keypoints) returns it
//   f_side = 1   the train image is src:  P = inlier(F, txy_j, qxy_i, t2)
// f_side = 1 lets a mutual check swap the tables and keep F: the call with the tables swapped and f_side = 1 sees the
// transpose of the same admissible set.
//
// Documented and not detected.  An all-zero F (what verification returns for "no model") is valid and admits nothing: S = 0.
// A point at an epipole of F (l = 0 on the src side, m = 0 on the dst side) admits every point of the other side whose own
// record leaves S > 0: the verdict of the verification's own inlier test.
//
// The guided answer for query i: as guided_rules.hpp, the first two admitted j under the matcher's key.
#pragma once

#include "epipolar_rules.hpp"

namespace guided_epipolar {

struct SrcRec { double l0, l1, l2, L; };                   // a point of the image F applies to
struct DstRec { double u, v, A, B; };                      // a point of the other image

VERIFY_RULES_HD inline SrcRec src_record(const double F[9], double x, double y)
{
    VERIFY_RULES_NO_FMA
    SrcRec s;
    s.l0 = (F[0] * x + F[1] * y) + F[2];
    s.l1 = (F[3] * x + F[4] * y) + F[5];
    s.l2 = (F[6] * x + F[7] * y) + F[8];
    s.L = s.l0 * s.l0 + s.l1 * s.l1;
    return s;
}

VERIFY_RULES_HD inline DstRec dst_record(const double F[9], double u, double v)
{
    VERIFY_RULES_NO_FMA
    DstRec d;
    const double m0 = (F[0] * u + F[3] * v) + F[6];
    const double m1 = (F[1] * u + F[4] * v) + F[7];
    d.u = u; d.v = v;
    d.A = m0 * m0;
    d.B = m1 * m1;
    return d;
}

VERIFY_RULES_HD inline bool admits(const SrcRec &s, const DstRec &d, double t2)
{
    VERIFY_RULES_NO_FMA
    const double e = (d.u * s.l0 + d.v * s.l1) + s.l2;
    const double S = (s.L + d.A) + d.B;
    return S > 0.0 && e * e <= t2 * S;
}

// P(i, j) for one pair, from the points themselves
inline bool pair_admitted(const double F[9], double t2, int f_side, const float *qxy, const float *txy)
{
    return f_side == 0 ? admits(src_record(F, (double)qxy[0], (double)qxy[1]), dst_record(F, (double)txy[0], (double)txy[1]), t2)
                       : admits(src_record(F, (double)txy[0], (double)txy[1]), dst_record(F, (double)qxy[0], (double)qxy[1]), t2);
}

// The guided top two on the host, as guided_rules::guided_top2_host: dist [nq][nt] the matrix of distances, qxy [nq][2],
// txy [nt][2]; idx [nq][2], sqdist [nq][2].  A NaN distance never enters, like in the kernel's strict comparisons.
inline void guided_top2_host(const float *dist, const float *qxy, int64_t nq, const float *txy, int64_t nt, const double F[9], float threshold,
                             int f_side, int32_t *idx, float *sqdist)
{
    const double t2 = verify_rules::threshold_sq(threshold);
    const float inf = __builtin_inff();
    for (int64_t i = 0; i < nq; i++) {
        float d1 = inf, d2 = inf;
        int32_t j1 = -1, j2 = -1;
        for (int64_t j = 0; j < nt; j++) {
            if (!pair_admitted(F, t2, f_side, qxy + 2 * i, txy + 2 * j)) continue;
            const float f = dist[i * nt + j];
            if (f < d1) { d2 = d1; j2 = j1; d1 = f; j1 = (int32_t)j; }
            else if (f < d2) { d2 = f; j2 = (int32_t)j; }
        }
        idx[2 * i] = j1; idx[2 * i + 1] = j2;
        sqdist[2 * i] = d1; sqdist[2 * i + 1] = d2;
    }
}

}  // namespace guided_epipolar
