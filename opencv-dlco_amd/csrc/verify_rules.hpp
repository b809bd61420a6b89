// verify_rules.hpp — how a list of putative matches is verified against a homography (dlco_desc_verify_homography,
// dlco_desc_verify_hypotheses): a deterministic RANSAC.  Hypotheses from four matches each, an inlier count for every
// hypothesis, the best by a total order, and a refit on the inliers.  The rule stated once for the host, the kernels
// (kernels_verify.hip) and the CPU tests (tests/shim/verify_rules_shim.cpp).  Plain C++: no HIP header, no device, no I/O.
//
// This is NOT cv::findHomography, which nothing here can run or pin, and no parity with it is claimed.  It is a rule of
// this library: every step is IEEE double + - x, one rounding each, no fused multiply-add; counts are integers.  Up to
// the first mask there is no division; the refit adds / and sqrt, correctly rounded on the host and on the device alike.  So the host, the kernels and a numpy restatement agree in every bit.  The scalar
// functions below switch contraction off themselves (VERIFY_RULES_NO_FMA); a compiler that does not know the pragma
// builds this header with -ffp-contract=off.
//
// Out of scope: an essential matrix (the fundamental matrix
// is epipolar_rules.hpp); symmetric transfer error; an adaptive hypothesis count.
// In scope since: a device-memory form, dlco_desc_verify_pairs_homography_device, whose refit rounds run in refit_pairs_kernel.
//
// Inputs.  src [m][2] and dst [m][2] float, widened to double; 4 <= m < 2^31.  Expected finite with |x|, |y| <= 2^20;
// nothing is checked: a non-finite coordinate fails every comparison below, so its match is never an inlier and a sample
// that holds it is invalid.
//
// Sampler.  Hypothesis h in 0 .. n_hyp-1, arithmetic mod 2^64, G = 0x9E3779B97F4A7C15:
//   mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
//   s = seed ^ ((h + 1) G); a draw is s += G, j = ((mix(s) >> 32) m) >> 32.  A draw equal to an earlier index of this
//   hypothesis is skipped; the first four distinct indices, in draw order, are the sample; after 16 draws without four the
//   hypothesis is invalid.
//
// Model from four matches, p_i = (x_i, y_i, 1), i = 1 .. 4:
//   cross(u, v) = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0),  dot(u, v) = (u0 v0 + u1 v1) + u2 v2
//   r0 = cross(p2, p3), r1 = cross(p3, p1), r2 = cross(p1, p2); lambda_i = dot(r_i, p4), det = dot(r0, p1): twice the
//   signed areas of the four triples.  a_i = lambda_i p_i (i = 1 .. 3, lambda_{i-1}).  The same on the destination points:
//   b_i, lambda'_i, det'.
//   Valid iff for each of the four pairs (lambda_i, lambda'_i), (det, det') both magnitudes are > 1.0 and the signs agree:
//   no three sample points nearly collinear in either image, orientation preserved.
//   R0 = cross(a2, a3), R1 = cross(a3, a1), R2 = cross(a1, a2): the rows of adj([a1 a2 a3]).
//   H[i][j] = (b1[i] R0[j] + b2[i] R1[j]) + b3[i] R2[j].
//   Scale (normalise): invalid if an entry is not finite or all are 0.  With E the biased exponent field of max |H| and
//   k = 1023 - E, H = (H 2^floor(k/2)) 2^(k - floor(k/2)): two multiplications by powers of two, exact unless an entry
//   turns subnormal, and max |H| lands in [1, 2) (a subnormal maximum, E = 0, stays below 1).
//   Sign: H is negated if w = (H20 x1 + H21 y1) + H22 < 0 at the first sample point.
//   An invalid hypothesis has H all zero.
//
// Inlier test, forward transfer without a division: X = (H00 x + H01 y) + H02, Y and W likewise; ex = X - u W,
// ey = Y - v W; inlier iff W > 0 and ex ex + ey ey <= t2 (W W), t2 = (double)threshold (double)threshold.
//
// Selection.  count[h] = inliers of hypothesis h (0 for an invalid one: W = 0 everywhere).  The best has the largest count,
// ties go to the smallest h: the maximum of the key (count << 32) | (0xFFFFFFFF - h).  A best count of 0: no model.
//
// Refit (refit_round on the host, refit_pairs_kernel on the device from the same functions; a round's acceptance is
// refit_step, step_pairs_kernel on the device; the loop is the library's lockstep one and, in the CPU frame verify_host,
// refit_rounds).  At most `refine` rounds; a round runs on the inliers of the current model in
// ascending match index:
//   Hartley normalisation of each side: centroid c = (sum x / n, sum y / n), d = (sum sqrt(dx dx + dy dy)) / n with
//   dx = x - cx, s = sqrt(2) / d, sums in index order; a normalised point is ((x - cx) s, (y - cy) s).
//   The 8 x 8 normal equations of the DLT with h33 = 1: a1 = (x, y, 1, 0, 0, 0, -(u x), -(u y)),
//   a2 = (0, 0, 0, x, y, 1, -(v x), -(v y)); N[i][j] += a1[i] a1[j] + a2[i] a2[j], r[i] += a1[i] u + a2[i] v.
//   Gaussian elimination with partial pivoting (largest magnitude, lowest row on ties), back-substitution.
//   H' = (Td^-1 Hn) Ts with Td^-1 = [1/sd 0 cxd; 0 1/sd cyd; 0 0 1], Ts = [ss 0 -(ss cxs); 0 ss -(ss cys); 0 0 1], products
//   by the dot rule; then the scale above and the sign from W at the first inlier.
//   Rejected when d is 0 or not finite, a pivot's magnitude is <= 1e-12 max |N|, H' is not finite (or zero), or W is 0 at
//   the first inlier: a rejected round keeps the model and ends the refit.  Otherwise H' is scored against all matches and
//   replaces the model iff its count is >= the current one (if not, the refit ends); if the mask did not change, the refit
//   ends as well.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define VERIFY_RULES_HD __host__ __device__
#else
#define VERIFY_RULES_HD
#endif

#if defined(__clang__)
#define VERIFY_RULES_NO_FMA _Pragma("clang fp contract(off)")
#else
#define VERIFY_RULES_NO_FMA
#endif

namespace verify_rules {

constexpr int kScoreChunk = 256;               // matches a workgroup of the scoring kernel stages in LDS at a time
constexpr int kRefitChunk = 128;               // matches a workgroup of the refit kernel stages in LDS at a time
constexpr int kMaxDraws = 16;
constexpr int32_t kMaxHyp = 1 << 20;
constexpr int32_t kMaxRefine = 8;
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
constexpr double kLargestDouble = 1.7976931348623157e308;
constexpr double kSqrt2 = 1.4142135623730951;  // sqrt(2.0) rounded to double

VERIFY_RULES_HD inline uint64_t mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the sample of hypothesis h among m matches: idx [4], -1 where no index was found; true iff there are four
VERIFY_RULES_HD inline bool sample(uint64_t seed, uint32_t h, uint32_t m, int32_t idx[4])
{
    uint64_t s = seed ^ (((uint64_t)h + 1) * kGolden);
    int n = 0;
    idx[0] = idx[1] = idx[2] = idx[3] = -1;
    for (int d = 0; d < kMaxDraws && n < 4; d++) {
        s += kGolden;
        const int32_t j = (int32_t)(((mix(s) >> 32) * (uint64_t)m) >> 32);
        bool seen = false;
        for (int k = 0; k < 4; k++) seen = seen || (k < n && idx[k] == j);
        if (!seen) {
            for (int k = 0; k < 4; k++)
                if (k == n) idx[k] = j;                    // no dynamic index: idx stays in registers on the device
            n++;
        }
    }
    return n == 4;
}

struct V3 { double x, y, z; };

VERIFY_RULES_HD inline V3 cross(V3 u, V3 v)
{
    VERIFY_RULES_NO_FMA
    return V3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}

VERIFY_RULES_HD inline double dot(V3 u, V3 v)
{
    VERIFY_RULES_NO_FMA
    return (u.x * v.x + u.y * v.y) + u.z * v.z;
}

VERIFY_RULES_HD inline V3 times(double s, V3 p)
{
    VERIFY_RULES_NO_FMA
    return V3{s * p.x, s * p.y, s * p.z};
}

// the projective basis of four points: the columns a_i = lambda_i p_i and the four areas (l[3] = det)
struct Basis { V3 a1, a2, a3; double l[4]; };

VERIFY_RULES_HD inline Basis basis(V3 p1, V3 p2, V3 p3, V3 p4)
{
    const V3 r0 = cross(p2, p3), r1 = cross(p3, p1), r2 = cross(p1, p2);
    Basis b;
    b.l[0] = dot(r0, p4); b.l[1] = dot(r1, p4); b.l[2] = dot(r2, p4); b.l[3] = dot(r0, p1);
    b.a1 = times(b.l[0], p1); b.a2 = times(b.l[1], p2); b.a3 = times(b.l[2], p3);
    return b;
}

// both magnitudes above 1 and the signs agree; false for a NaN
VERIFY_RULES_HD inline bool areas_agree(double a, double b) { return (a > 1.0 && b > 1.0) || (a < -1.0 && b < -1.0); }

VERIFY_RULES_HD inline double pow2(int n)                  // 2^n for n in -1022 .. 1023
{
    const uint64_t bits = (uint64_t)(n + 1023) << 52;
    double d;
    __builtin_memcpy(&d, &bits, sizeof d);
    return d;
}

// the power-of-two scale of H [9]; false: an entry is not finite, or all are zero
VERIFY_RULES_HD inline bool normalise(double H[9])
{
    VERIFY_RULES_NO_FMA
    double mx = 0.0;
    bool finite = true;
    for (int i = 0; i < 9; i++) {
        const double a = __builtin_fabs(H[i]);
        finite = finite && a <= kLargestDouble;
        mx = a > mx ? a : mx;
    }
    if (!finite || !(mx > 0.0)) return false;
    uint64_t bits;
    __builtin_memcpy(&bits, &mx, sizeof bits);
    const int k = 1023 - (int)((bits >> 52) & 0x7FF);
    const int k1 = (k - (k & 1)) / 2, k2 = k - k1;         // floor(k / 2) and the rest, both in -512 .. 512
    const double s1 = pow2(k1), s2 = pow2(k2);
    for (int i = 0; i < 9; i++) H[i] = (H[i] * s1) * s2;
    return true;
}

// W of H at (x, y)
VERIFY_RULES_HD inline double w_at(const double H[9], double x, double y)
{
    VERIFY_RULES_NO_FMA
    return (H[6] * x + H[7] * y) + H[8];
}

// H [9] row-major from the four matches (sx[i], sy[i]) -> (dx[i], dy[i]); false: invalid, H is all zero
VERIFY_RULES_HD inline bool model(const double sx[4], const double sy[4], const double dx[4], const double dy[4], double H[9])
{
    VERIFY_RULES_NO_FMA
    for (int i = 0; i < 9; i++) H[i] = 0.0;
    const Basis A = basis(V3{sx[0], sy[0], 1.0}, V3{sx[1], sy[1], 1.0}, V3{sx[2], sy[2], 1.0}, V3{sx[3], sy[3], 1.0});
    const Basis B = basis(V3{dx[0], dy[0], 1.0}, V3{dx[1], dy[1], 1.0}, V3{dx[2], dy[2], 1.0}, V3{dx[3], dy[3], 1.0});
    bool ok = true;
    for (int i = 0; i < 4; i++) ok = ok && areas_agree(A.l[i], B.l[i]);
    if (!ok) return false;
    const V3 R0 = cross(A.a2, A.a3), R1 = cross(A.a3, A.a1), R2 = cross(A.a1, A.a2);
    const double b1[3] = {B.a1.x, B.a1.y, B.a1.z}, b2[3] = {B.a2.x, B.a2.y, B.a2.z}, b3[3] = {B.a3.x, B.a3.y, B.a3.z};
    const double r0[3] = {R0.x, R0.y, R0.z}, r1[3] = {R1.x, R1.y, R1.z}, r2[3] = {R2.x, R2.y, R2.z};
    double T[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) T[3 * i + j] = (b1[i] * r0[j] + b2[i] * r1[j]) + b3[i] * r2[j];
    if (!normalise(T)) return false;
    const bool flip = w_at(T, sx[0], sy[0]) < 0.0;
    for (int i = 0; i < 9; i++) H[i] = flip ? -T[i] : T[i];
    return true;
}

// hypothesis h of the call: its sample idx [4] and H [9] (all zero when invalid)
VERIFY_RULES_HD inline bool hypothesis(const float *src, const float *dst, uint32_t m, uint64_t seed, uint32_t h, int32_t idx[4], double H[9])
{
    for (int i = 0; i < 9; i++) H[i] = 0.0;
    if (!sample(seed, h, m, idx)) return false;
    double sx[4], sy[4], dx[4], dy[4];
    for (int i = 0; i < 4; i++) {
        sx[i] = (double)src[2 * (int64_t)idx[i]]; sy[i] = (double)src[2 * (int64_t)idx[i] + 1];
        dx[i] = (double)dst[2 * (int64_t)idx[i]]; dy[i] = (double)dst[2 * (int64_t)idx[i] + 1];
    }
    return model(sx, sy, dx, dy, H);
}

VERIFY_RULES_HD inline double threshold_sq(float threshold)
{
    VERIFY_RULES_NO_FMA
    return (double)threshold * (double)threshold;
}

// the match (x, y) -> (u, v) is an inlier of H
VERIFY_RULES_HD inline bool inlier(const double H[9], double x, double y, double u, double v, double t2)
{
    VERIFY_RULES_NO_FMA
    const double X = (H[0] * x + H[1] * y) + H[2];
    const double Y = (H[3] * x + H[4] * y) + H[5];
    const double W = (H[6] * x + H[7] * y) + H[8];
    const double ex = X - u * W, ey = Y - v * W;
    return W > 0.0 && ex * ex + ey * ey <= t2 * (W * W);
}

// the selection key: larger is better
VERIFY_RULES_HD inline uint64_t select_key(int32_t count, uint32_t h) { return ((uint64_t)(uint32_t)count << 32) | (uint64_t)(0xFFFFFFFFu - h); }
VERIFY_RULES_HD inline int32_t key_count(uint64_t key) { return (int32_t)(key >> 32); }
VERIFY_RULES_HD inline int32_t key_hyp(uint64_t key) { return (int32_t)(0xFFFFFFFFu - (uint32_t)key); }

// ---- the rule on the host: what the kernels must reproduce ---------------------------------------------------------------
// the key of the best hypothesis; its count is 0 when there is no model
inline uint64_t select(const int32_t *count, int32_t n_hyp)
{
    uint64_t best = 0;
    for (int32_t h = 0; h < n_hyp; h++) {
        const uint64_t key = select_key(count[h], (uint32_t)h);
        best = key > best ? key : best;
    }
    return best;
}

// ---- the pieces of a refit round that the host below and refit_pairs_kernel (kernels_verify.hip) share: everything but the
// sums, which both walk over the inliers in ascending match index -------------------------------------------------------------
// the distance of (x, y) from the centroid
VERIFY_RULES_HD inline double centred_length(double x, double y, double cx, double cy)
{
    VERIFY_RULES_NO_FMA
    const double dx = x - cx, dy = y - cy;
    return __builtin_sqrt(dx * dx + dy * dy);
}

// Hartley's scale from the mean distance d; false: d is 0 or not finite
VERIFY_RULES_HD inline bool hartley_scale(double d, double &s)
{
    VERIFY_RULES_NO_FMA
    if (!(d > 0.0) || !(d <= kLargestDouble)) return false;
    s = kSqrt2 / d;
    return true;
}

// a coordinate of the normalised point
VERIFY_RULES_HD inline double normalised(double p, double c, double s)
{
    VERIFY_RULES_NO_FMA
    return (p - c) * s;
}

// what a normalised match (x, y) -> (u, v) adds to the DLT's normal equations: a [0, 8) = a1, a [8, 16) = a2, then u and v
constexpr int kDltRow = 18;
VERIFY_RULES_HD inline void dlt_rows(double x, double y, double u, double v, double *a)
{
    VERIFY_RULES_NO_FMA
    a[0] = x; a[1] = y; a[2] = 1.0; a[3] = 0.0; a[4] = 0.0; a[5] = 0.0; a[6] = -(u * x); a[7] = -(u * y);
    a[8] = 0.0; a[9] = 0.0; a[10] = 0.0; a[11] = x; a[12] = y; a[13] = 1.0; a[14] = -(v * x); a[15] = -(v * y);
    a[16] = u; a[17] = v;
}

// one term of N[p][q] (a = a1[p], b = a1[q], c = a2[p], d = a2[q]) or of r[p] (b = u, d = v)
VERIFY_RULES_HD inline double dlt_add(double acc, double a, double b, double c, double d)
{
    VERIFY_RULES_NO_FMA
    return acc + (a * b + c * d);
}

// The sums of a round as refit_pairs_kernel spreads them over lanes: sum l adds, match after match, the product(s) of the
// entries a, b (and c, d) of the match's row.  The homography: l < 64 is N[l / 8][l % 8], l < 72 is r[l - 64] (kDltSums);
// beyond, a sum nobody reads
struct Terms { int a, b, c, d; };
constexpr int kDltSums = 72;
VERIFY_RULES_HD inline Terms dlt_terms(int l)
{
    if (l < 64) return Terms{l >> 3, l & 7, 8 + (l >> 3), 8 + (l & 7)};
    if (l < kDltSums) return Terms{l - 64, 16, 8 + (l - 64), 17};
    return Terms{0, 0, 0, 0};
}
VERIFY_RULES_HD inline double dlt_add(double acc, const double *row, Terms t) { return dlt_add(acc, row[t.a], row[t.b], row[t.c], row[t.d]); }

// h [8] of the summed normal equations N [8][8] (row-major), r [8], both overwritten: Gaussian elimination with partial
// pivoting (largest magnitude, lowest row on ties), back-substitution; false: a pivot at or under 1e-12 max |N|
VERIFY_RULES_HD inline bool dlt_solve(double *N, double *r, double *h)
{
    VERIFY_RULES_NO_FMA
    double nmax = 0.0;
    for (int i = 0; i < 64; i++) nmax = __builtin_fabs(N[i]) > nmax ? __builtin_fabs(N[i]) : nmax;
    const double floor_pivot = 1e-12 * nmax;
    for (int k = 0; k < 8; k++) {
        int piv = k;
        double best = __builtin_fabs(N[8 * k + k]);
        for (int i = k + 1; i < 8; i++)
            if (__builtin_fabs(N[8 * i + k]) > best) { best = __builtin_fabs(N[8 * i + k]); piv = i; }
        if (!(best > floor_pivot)) return false;
        if (piv != k) {
            for (int q = 0; q < 8; q++) { const double t = N[8 * k + q]; N[8 * k + q] = N[8 * piv + q]; N[8 * piv + q] = t; }
            const double t = r[k]; r[k] = r[piv]; r[piv] = t;
        }
        for (int i = k + 1; i < 8; i++) {
            const double f = N[8 * i + k] / N[8 * k + k];
            for (int q = k + 1; q < 8; q++) N[8 * i + q] = N[8 * i + q] - f * N[8 * k + q];
            r[i] = r[i] - f * r[k];
        }
    }
    for (int i = 7; i >= 0; i--) {
        double acc = r[i];
        for (int q = i + 1; q < 8; q++) acc = acc - N[8 * i + q] * h[q];
        h[i] = acc / N[8 * i + i];
    }
    return true;
}

// C = A B of 3 x 3 matrices by the dot rule
VERIFY_RULES_HD inline void mul3(const double A[9], const double B[9], double C[9])
{
    VERIFY_RULES_NO_FMA
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

// H' = (Td^-1 Hn) Ts of the solution h [8] (h33 = 1), scaled; false: not finite or zero
VERIFY_RULES_HD inline bool dlt_denormalise(const double *h, double cxs, double cys, double ss, double cxd, double cyd, double sd, double H_out[9])
{
    VERIFY_RULES_NO_FMA
    const double Hn[9] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], 1.0};
    const double isd = 1.0 / sd;
    const double Tdi[9] = {isd, 0.0, cxd, 0.0, isd, cyd, 0.0, 0.0, 1.0};
    const double Ts[9] = {ss, 0.0, -(ss * cxs), 0.0, ss, -(ss * cys), 0.0, 0.0, 1.0};
    double T[9];
    mul3(Tdi, Hn, T);
    mul3(T, Ts, H_out);
    return normalise(H_out);
}

// the sign of H from W at the first inlier (x, y); false: W is 0
VERIFY_RULES_HD inline bool dlt_sign(double H[9], double x, double y)
{
    const double W = w_at(H, x, y);
    if (W == 0.0) return false;
    if (W < 0.0)
        for (int i = 0; i < 9; i++) H[i] = -H[i];
    return true;
}

// Hartley normalisation of the masked points: centroid and scale; false: the mean distance is 0 or not finite
inline bool hartley(const float *pts, const uint8_t *mask, int64_t m, double &cx, double &cy, double &s)
{
    VERIFY_RULES_NO_FMA
    double sum_x = 0.0, sum_y = 0.0, sum_d = 0.0;
    int64_t n = 0;
    for (int64_t i = 0; i < m; i++)
        if (mask[i]) { sum_x += (double)pts[2 * i]; sum_y += (double)pts[2 * i + 1]; n++; }
    cx = sum_x / (double)n; cy = sum_y / (double)n;
    for (int64_t i = 0; i < m; i++)
        if (mask[i]) sum_d += centred_length((double)pts[2 * i], (double)pts[2 * i + 1], cx, cy);
    return hartley_scale(sum_d / (double)n, s);
}

// one round of the refit on the inliers of mask: H' in H_out; false: rejected, H_out is undefined
inline bool refit_round(const float *src, const float *dst, int64_t m, const uint8_t *mask, double H_out[9])
{
    double cxs, cys, ss, cxd, cyd, sd;
    if (!hartley(src, mask, m, cxs, cys, ss) || !hartley(dst, mask, m, cxd, cyd, sd)) return false;
    double N[64] = {}, r[8] = {}, h[8];
    int64_t first = -1;
    for (int64_t i = 0; i < m; i++) {
        if (!mask[i]) continue;
        if (first < 0) first = i;
        double a[kDltRow];
        dlt_rows(normalised((double)src[2 * i], cxs, ss), normalised((double)src[2 * i + 1], cys, ss), normalised((double)dst[2 * i], cxd, sd),
                 normalised((double)dst[2 * i + 1], cyd, sd), a);
        for (int p = 0; p < 8; p++) {
            for (int q = 0; q < 8; q++) N[8 * p + q] = dlt_add(N[8 * p + q], a[p], a[q], a[8 + p], a[8 + q]);
            r[p] = dlt_add(r[p], a[p], a[16], a[8 + p], a[17]);
        }
    }
    if (!dlt_solve(N, r, h)) return false;
    if (!dlt_denormalise(h, cxs, cys, ss, cxd, cyd, sd, H_out)) return false;
    return dlt_sign(H_out, (double)src[2 * first], (double)src[2 * first + 1]);
}

// The acceptance rule of one round: the model M [9] with (mask [m], count) meets the round's Mn [9], scored as (trial [m], c).
// Mn replaces the model iff c >= count.  Returns whether the refit goes on: not after a rejected round, nor after one that
// left the mask unchanged.  The library's lockstep loop (dlco_desc_api.cpp, every dlco_desc_verify_* call) and the CPU
// frame's loop below both end a round here.
inline bool refit_step(int64_t m, double M[9], uint8_t *mask, int64_t &count, const double Mn[9], const uint8_t *trial, int64_t c)
{
    if (c < count) return false;
    const bool same = std::memcmp(trial, mask, (size_t)m) == 0;
    std::memcpy(M, Mn, 9 * sizeof(double));
    std::memcpy(mask, trial, (size_t)m);
    count = c;
    return !same;
}

// The refit's loop of the CPU frame (verify_host) for a model M [9] with (mask [m], count); the library drops a pair from its
// lockstep loop under the same two conditions.  round(mask, M') forms the model of one round from the inliers of
// mask (false: rejected), score(M', trial mask [m]) -> count of M' over all matches.  rounds [refine][9] (may be NULL) receives
// every M' a round formed; returns their number.
template <typename Round, typename Score>
inline int refit_rounds(int64_t m, int32_t refine, double M[9], uint8_t *mask, int64_t &count, Round &&round, Score &&score, double *rounds)
{
    std::vector<uint8_t> trial((size_t)m);
    int formed = 0;
    for (int32_t k = 0; k < refine; k++) {
        double Mn[9];
        if (!round(mask, Mn)) break;
        if (rounds) std::memcpy(rounds + 9 * formed, Mn, sizeof Mn);
        formed++;
        const int64_t c = score(Mn, trial.data());
        if (!refit_step(m, M, mask, count, Mn, trial.data(), c)) break;
    }
    return formed;
}

// The homography as the frame below and the kernels (kernels_verify.hip) take a model: the sample size and the three
// functions above, nothing of its own.  The fundamental matrix is epipolar_rules::Fundamental.
struct Homography {
    static constexpr int kSample = 4;
    VERIFY_RULES_HD static bool hypothesis(const float *src, const float *dst, uint32_t m, uint64_t seed, uint32_t h, int32_t idx[kSample], double H[9])
    {
        return verify_rules::hypothesis(src, dst, m, seed, h, idx, H);
    }
    VERIFY_RULES_HD static bool inlier(const double H[9], double x, double y, double u, double v, double t2)
    {
        return verify_rules::inlier(H, x, y, u, v, t2);
    }
    static bool refit_round(const float *src, const float *dst, int64_t m, const uint8_t *mask, double H_out[9])
    {
        return verify_rules::refit_round(src, dst, m, mask, H_out);
    }
    // The round as refit_pairs_kernel takes a model (and its walk on the CPU, tests/shim/verify_refit_asan_main.cpp): the doubles
    // of a staged match's row, the sums and their terms, the fewest inliers, and the solve on work = N [64], r [8] summed, h [8]
    // with the centroids, the scales and the first inlier (fx, fy) of src
    static constexpr int kRefitRow = kDltRow, kRefitSums = kDltSums, kRefitWork = 64 + 8 + 8;
    VERIFY_RULES_HD static void refit_row(double x, double y, double u, double v, double *a) { dlt_rows(x, y, u, v, a); }
    VERIFY_RULES_HD static Terms refit_terms(int l) { return dlt_terms(l); }
    VERIFY_RULES_HD static double refit_add(double acc, const double *a, Terms t) { return dlt_add(acc, a, t); }
    VERIFY_RULES_HD static bool refit_few(int) { return false; }
    VERIFY_RULES_HD static bool refit_solve(double *work, double cxs, double cys, double ss, double cxd, double cyd, double sd, double fx, double fy,
                                            double H_out[9])
    {
        return dlt_solve(work, work + 64, work + 72) && dlt_denormalise(work + 72, cxs, cys, ss, cxd, cyd, sd, H_out) && dlt_sign(H_out, fx, fy);
    }
};

// ---- the frame of every model: Model is Homography or epipolar_rules::Fundamental, M its 3 x 3 matrix row-major -----------
// M_all [n_hyp][9]; idx_all [n_hyp][Model::kSample] and valid [n_hyp] may be NULL
template <typename Model>
inline void all_hypotheses(const float *src, const float *dst, int64_t m, int32_t n_hyp, uint64_t seed, double *M_all, int32_t *idx_all,
                           uint8_t *valid)
{
    for (int32_t h = 0; h < n_hyp; h++) {
        int32_t idx[Model::kSample];
        const bool ok = Model::hypothesis(src, dst, (uint32_t)m, seed, (uint32_t)h, idx, M_all + 9 * (int64_t)h);
        if (idx_all) std::memcpy(idx_all + Model::kSample * (int64_t)h, idx, sizeof idx);
        if (valid) valid[h] = ok ? 1 : 0;
    }
}

// the inliers of M among all matches; mask [m] may be NULL
template <typename Model>
inline int64_t count_inliers(const double M[9], const float *src, const float *dst, int64_t m, double t2, uint8_t *mask)
{
    int64_t n = 0;
    for (int64_t i = 0; i < m; i++) {
        const bool in = Model::inlier(M, (double)src[2 * i], (double)src[2 * i + 1], (double)dst[2 * i], (double)dst[2 * i + 1], t2);
        if (mask) mask[i] = in ? 1 : 0;
        n += in ? 1 : 0;
    }
    return n;
}

// The whole rule on the host.  M [9], mask [m], *count, *best_hyp (-1: no model, M and mask zero); M_all [n_hyp][9] and
// counts [n_hyp] scratch of the caller; rounds as for refit_rounds, *n_rounds the number formed (both may be NULL).  The
// refit's score is count_inliers here, the mask kernel in the library, whose loop runs the rounds of many pairs in lockstep.
template <typename Model>
inline void verify_host(const float *src, const float *dst, int64_t m, float threshold, int32_t n_hyp, uint64_t seed, int32_t refine, double *M_all,
                        int32_t *counts, double M[9], uint8_t *mask, int64_t *count, int32_t *best_hyp, double *rounds, int32_t *n_rounds)
{
    const double t2 = threshold_sq(threshold);
    all_hypotheses<Model>(src, dst, m, n_hyp, seed, M_all, nullptr, nullptr);
    for (int32_t h = 0; h < n_hyp; h++) counts[h] = (int32_t)count_inliers<Model>(M_all + 9 * (int64_t)h, src, dst, m, t2, nullptr);
    const uint64_t key = select(counts, n_hyp);
    if (n_rounds) *n_rounds = 0;
    if (key_count(key) == 0) {
        for (int i = 0; i < 9; i++) M[i] = 0.0;
        std::memset(mask, 0, (size_t)m);
        *count = 0; *best_hyp = -1;
        return;
    }
    *best_hyp = key_hyp(key);
    std::memcpy(M, M_all + 9 * (int64_t)*best_hyp, 9 * sizeof(double));
    *count = count_inliers<Model>(M, src, dst, m, t2, mask);
    const int formed = refit_rounds(m, refine, M, mask, *count, [&](const uint8_t *cur, double *Mn) { return Model::refit_round(src, dst, m, cur, Mn); },
                                    [&](const double *Mn, uint8_t *trial) { return count_inliers<Model>(Mn, src, dst, m, t2, trial); }, rounds);
    if (n_rounds) *n_rounds = formed;
}

// the frame with the homography under this namespace's plain names: what the tests' shims call
inline void all_hypotheses(const float *src, const float *dst, int64_t m, int32_t n_hyp, uint64_t seed, double *H_all, int32_t *idx_all,
                           uint8_t *valid)
{
    all_hypotheses<Homography>(src, dst, m, n_hyp, seed, H_all, idx_all, valid);
}
inline int64_t count_inliers(const double H[9], const float *src, const float *dst, int64_t m, double t2, uint8_t *mask)
{
    return count_inliers<Homography>(H, src, dst, m, t2, mask);
}
inline void verify_host(const float *src, const float *dst, int64_t m, float threshold, int32_t n_hyp, uint64_t seed, int32_t refine, double *H_all,
                        int32_t *counts, double H[9], uint8_t *mask, int64_t *count, int32_t *best_hyp, double *rounds, int32_t *n_rounds)
{
    verify_host<Homography>(src, dst, m, threshold, n_hyp, seed, refine, H_all, counts, H, mask, count, best_hyp, rounds, n_rounds);
}

}  // namespace verify_rules
