// epipolar_rules.hpp — how a list of putative matches is verified against a fundamental matrix
// (dlco_desc_verify_fundamental, dlco_desc_verify_fundamental_hypotheses): the deterministic RANSAC of verify_rules.hpp with
// the epipolar model x'^T F x = 0, x = (x, y, 1) from src and x' = (u, v, 1) from dst.  Hypotheses from eight matches each, an
// inlier count for every hypothesis, the best by the same total order, and a refit on the inliers.  The rule stated once for
// the host, the kernels (kernels_verify.hip) and the CPU tests (tests/shim/epipolar_rules_shim.cpp).  Plain C++: no HIP
// header, no device, no I/O.
//
// This is NOT cv::findFundamentalMat, which nothing here can run or pin, and no parity with it is claimed.  It is a rule of
// this library: every step is IEEE double + - x /, one rounding each, no fused multiply-add and no transcendental; counts
// are integers.  The refit adds sqrt, correctly rounded on the host and on the device alike.  So the host, the kernels and a
// numpy restatement agree in every bit.  The functions below switch contraction off themselves (VERIFY_RULES_NO_FMA).
//
// Out of scope: a seven-point solver; an essential matrix; a choice between a homography and F; an
// adaptive hypothesis count.  (The inlier test as the predicate of guided matching: guided_epipolar_rules.hpp.)
// In scope since: a device-memory form, dlco_desc_verify_pairs_fundamental_device, whose refit rounds run in refit_pairs_kernel.
//
// Degeneracy, documented and not detected.  Matches related by a homography (a plane, a camera that only rotates, a shifted
// image) satisfy a three-dimensional family of F.  The pivot floor below makes an exactly degenerate sample invalid; a nearly
// degenerate one yields some F of that family, which all those matches satisfy.
//
// Inputs.  As verify_rules.hpp, with 8 <= m < 2^31.
//
// Sampler.  The counter stream of verify_rules.hpp: s = seed ^ ((h + 1) G), a draw is s += G, j = ((mix(s) >> 32) m) >> 32.
//   The first eight distinct indices, in draw order, are the sample; after 32 draws without eight the hypothesis is invalid.
//
// Local normalisation, per side, of the sample's eight points p_i in sample order (local_norm):
//   c = (((p_0 + p_1) + p_2) + ... + p_7) 0.125 per coordinate, d_i = p_i - c, mx = max |d| over the sixteen numbers; invalid
//   if a |d| is not finite or mx is 0.  With E the biased exponent field of mx, k = 1023 - E, k1 = floor(k / 2), k2 = k - k1:
//   d = (d 2^k1) 2^k2, so mx lands in [1, 2).  The transform is T = [s 0 tx; 0 s ty; 0 0 1], s = 2^k1 2^k2, tx = -(s cx),
//   ty = -(s cy): Ts for src, Td for dst.
//
// Eight-point system (eight_point).  With (x, y) the normalised src and (u, v) the normalised dst point of sample i, row i of
//   the 8 x 9 matrix A is (u x, u y, u, v x, v y, v, x, y, 1); amax = max |A|.  Gaussian elimination with complete pivoting,
//   k = 0 .. 7: the pivot is the entry of largest magnitude among rows k .. 7 and columns k .. 8 in their current positions,
//   scanned row by row, a later entry winning only when strictly larger (ties: lowest row, then lowest column).  Invalid
//   unless |pivot| > 2^-40 amax.  Rows k and the pivot's are swapped, then columns k and the pivot's (in all eight rows);
//   for r = k+1 .. 7: f = A[r][k] / A[k][k], A[r][q] = A[r][q] - f A[k][q] for q = k+1 .. 8.
//   The column left at position 8 is the free unknown: z[8] = 1; for i = 7 .. 0: acc = -A[i][8], acc = acc - A[i][q] z[q] for
//   q = i+1 .. 7 ascending, z[i] = acc / A[i][i].  Fn[j] = z[position of original column j]: Fn row-major.
//   (Complete pivoting, not F33 = 1: a sideways translation has F33 = 0.)
//
// Denormalise, scale, sign (finish).  F = (Td^T Fn) Ts by verify_rules::mul3, then verify_rules::normalise (max |F| in [1, 2);
//   invalid if F is not finite or is zero), then F is negated if the first entry in row-major order whose magnitude equals
//   max |F| is negative.  An invalid hypothesis has F all zero.
//
// Inlier test (inlier), the Sampson error without a division, 33 fp64 operations (kOpsPerPair) and two comparisons:
//   l0 = (F00 x + F01 y) + F02, l1 and l2 likewise with rows 1 and 2      12
//   e = (u l0 + v l1) + l2                                                 4
//   m0 = (F00 u + F10 v) + F20, m1 = (F01 u + F11 v) + F21                 8
//   S = ((l0 l0 + l1 l1) + m0 m0) + m1 m1                                  7
//   inlier iff S > 0 and e e <= t2 S, t2 = verify_rules::threshold_sq      2
//   S > 0 keeps an all-zero F from admitting everything; a NaN fails both comparisons.
//
// Selection.  verify_rules::select_key, unchanged; a best count of 0: no model.
//
// Refit (refit_round on the host, refit_pairs_kernel on the device from the same functions; a round's acceptance is
// verify_rules::refit_step, the loop the library's lockstep one and, in the CPU frame verify_host, verify_rules::refit_rounds).  At most `refine` rounds; a round runs on the
// inliers of the current model in ascending match index and is rejected when there are fewer than 8:
//   verify_rules::hartley on each side; a normalised point is ((x - cx) s, (y - cy) s).
//   N = sum a a^T, 9 x 9, a the row above of the normalised match, N[p][q] = N[p][q] + a[p] a[q] in index order.
//   Fn = the eigenvector of N's smallest eigenvalue by the cyclic Jacobi rule below (ties: lowest index).
//   Rank 2: G = Fn^T Fn by mul3, v = the eigenvector of G's smallest eigenvalue by the same rule, w = Fn v by the dot rule,
//   Fn[i][j] = Fn[i][j] - w[i] v[j]: the nearest rank-2 matrix, without an SVD.
//   F' = (Td^T Fn) Ts with Ts = [ss 0 -(ss cxs); 0 ss -(ss cys); 0 0 1] and Td likewise; then the scale and sign above.
//   Rejected when hartley fails or F' is not finite or is zero: a rejected round keeps the model and ends the refit.  Otherwise
//   F' is scored against all matches and replaces the model iff its count is >= the current one (if not, the refit ends); if the
//   mask did not change, the refit ends as well.
//   With refine = 0 the result is the linear eight-point hypothesis, which need not be singular; after an accepted round it is
//   of rank 2 up to rounding.
//
// Cyclic Jacobi (jacobi) of a symmetric n x n matrix N, V = I at the start.  At most 30 sweeps; a sweep visits the pairs (p, q),
//   p < q, in row-major order, and the iteration ends after a sweep that rotated nothing.  A pair with N[p][q] == 0 is skipped.
//   Otherwise, with a = N[p][q]: theta = (N[q][q] - N[p][p]) / (2 a); t = sgn(theta) / (|theta| + sqrt(theta theta + 1)),
//   sgn(0) = +1; c = 1 / sqrt(t t + 1); s = t c;
//   N[p][p] = N[p][p] - t a; N[q][q] = N[q][q] + t a; N[p][q] = N[q][p] = 0;
//   for r other than p, q, ascending: g = N[r][p], h = N[r][q]; N[r][p] = N[p][r] = c g - s h; N[r][q] = N[q][r] = s g + c h;
//   for r = 0 .. n-1: g = V[r][p], h = V[r][q]; V[r][p] = c g - s h; V[r][q] = s g + c h.
//   Operations are + - x / sqrt, one rounding each.  The eigenvalues are N's diagonal, the eigenvectors V's columns.
#pragma once

#include "verify_rules.hpp"

#if defined(__clang__)
#define EPIPOLAR_RULES_UNROLL _Pragma("unroll")
#else
#define EPIPOLAR_RULES_UNROLL
#endif

namespace epipolar_rules {

namespace vr = verify_rules;

constexpr int kSample = 8;
constexpr int kMaxDraws = 32;
constexpr int kOpsPerPair = 33;                            // fp64 operations of inlier() per (hypothesis, match)
constexpr int kMaxSweeps = 30;
constexpr double kPivotFloor = 9.094947017729282379150390625e-13;  // 2^-40

// the sample of hypothesis h among m matches: idx [8], -1 where no index was found; true iff there are eight
VERIFY_RULES_HD inline bool sample(uint64_t seed, uint32_t h, uint32_t m, int32_t idx[kSample])
{
    uint64_t s = seed ^ (((uint64_t)h + 1) * vr::kGolden);
    int n = 0;
    EPIPOLAR_RULES_UNROLL
    for (int k = 0; k < kSample; k++) idx[k] = -1;
    for (int d = 0; d < kMaxDraws && n < kSample; d++) {
        s += vr::kGolden;
        const int32_t j = (int32_t)(((vr::mix(s) >> 32) * (uint64_t)m) >> 32);
        bool seen = false;
        EPIPOLAR_RULES_UNROLL
        for (int k = 0; k < kSample; k++) seen = seen || (k < n && idx[k] == j);
        if (!seen) {
            EPIPOLAR_RULES_UNROLL
            for (int k = 0; k < kSample; k++)
                if (k == n) idx[k] = j;                    // no dynamic index: idx stays in registers on the device
            n++;
        }
    }
    return n == kSample;
}

// the local normalisation of one side's eight points, in place; T = [s 0 tx; 0 s ty; 0 0 1]; false: invalid
VERIFY_RULES_HD inline bool local_norm(double px[kSample], double py[kSample], double &s, double &tx, double &ty)
{
    VERIFY_RULES_NO_FMA
    double sum_x = px[0], sum_y = py[0];
    EPIPOLAR_RULES_UNROLL
    for (int i = 1; i < kSample; i++) { sum_x = sum_x + px[i]; sum_y = sum_y + py[i]; }
    const double cx = sum_x * 0.125, cy = sum_y * 0.125;
    double mx = 0.0;
    bool finite = true;
    EPIPOLAR_RULES_UNROLL
    for (int i = 0; i < kSample; i++) {
        px[i] = px[i] - cx; py[i] = py[i] - cy;
        const double a = __builtin_fabs(px[i]), b = __builtin_fabs(py[i]);
        finite = finite && a <= vr::kLargestDouble && b <= vr::kLargestDouble;
        mx = a > mx ? a : mx;
        mx = b > mx ? b : mx;
    }
    if (!finite || !(mx > 0.0)) return false;
    uint64_t bits;
    __builtin_memcpy(&bits, &mx, sizeof bits);
    const int k = 1023 - (int)((bits >> 52) & 0x7FF);
    const int k1 = (k - (k & 1)) / 2, k2 = k - k1;
    const double s1 = vr::pow2(k1), s2 = vr::pow2(k2);
    EPIPOLAR_RULES_UNROLL
    for (int i = 0; i < kSample; i++) { px[i] = (px[i] * s1) * s2; py[i] = (py[i] * s1) * s2; }
    s = s1 * s2;
    tx = -(s * cx); ty = -(s * cy);
    return true;
}

// Fn [9] of eight normalised matches (x, y) -> (u, v): the null vector of the 8 x 9 system; false: a pivot under the floor.
// Every index below is a constant once the loops are unrolled and every swap is a select, so that A stays in registers on
// the device.
VERIFY_RULES_HD inline bool eight_point(const double x[kSample], const double y[kSample], const double u[kSample], const double v[kSample],
                                        double Fn[9])
{
    VERIFY_RULES_NO_FMA
    double A[8][9];
    int perm[9];
    double amax = 0.0;
    EPIPOLAR_RULES_UNROLL
    for (int i = 0; i < 8; i++) {
        A[i][0] = u[i] * x[i]; A[i][1] = u[i] * y[i]; A[i][2] = u[i];
        A[i][3] = v[i] * x[i]; A[i][4] = v[i] * y[i]; A[i][5] = v[i];
        A[i][6] = x[i]; A[i][7] = y[i]; A[i][8] = 1.0;
        EPIPOLAR_RULES_UNROLL
        for (int q = 0; q < 9; q++) { const double a = __builtin_fabs(A[i][q]); amax = a > amax ? a : amax; }
    }
    EPIPOLAR_RULES_UNROLL
    for (int q = 0; q < 9; q++) perm[q] = q;
    const double floor_pivot = kPivotFloor * amax;
    EPIPOLAR_RULES_UNROLL
    for (int k = 0; k < 8; k++) {
        double best = __builtin_fabs(A[k][k]);
        int pr = k, pc = k;
        EPIPOLAR_RULES_UNROLL
        for (int r = k; r < 8; r++) {
            EPIPOLAR_RULES_UNROLL
            for (int c = k; c < 9; c++) {
                const double a = __builtin_fabs(A[r][c]);
                const bool better = a > best;
                best = better ? a : best; pr = better ? r : pr; pc = better ? c : pc;
            }
        }
        if (!(best > floor_pivot)) return false;
        EPIPOLAR_RULES_UNROLL
        for (int r = k + 1; r < 8; r++) {
            const bool sw = pr == r;
            EPIPOLAR_RULES_UNROLL
            for (int q = k; q < 9; q++) {
                const double a = A[k][q], b = A[r][q];
                A[k][q] = sw ? b : a; A[r][q] = sw ? a : b;
            }
        }
        EPIPOLAR_RULES_UNROLL
        for (int c = k + 1; c < 9; c++) {
            const bool sw = pc == c;
            EPIPOLAR_RULES_UNROLL
            for (int r = 0; r < 8; r++) {
                const double a = A[r][k], b = A[r][c];
                A[r][k] = sw ? b : a; A[r][c] = sw ? a : b;
            }
            const int a = perm[k], b = perm[c];
            perm[k] = sw ? b : a; perm[c] = sw ? a : b;
        }
        EPIPOLAR_RULES_UNROLL
        for (int r = k + 1; r < 8; r++) {
            const double f = A[r][k] / A[k][k];
            EPIPOLAR_RULES_UNROLL
            for (int q = k + 1; q < 9; q++) A[r][q] = A[r][q] - f * A[k][q];
        }
    }
    double z[9];
    z[8] = 1.0;
    EPIPOLAR_RULES_UNROLL
    for (int i = 7; i >= 0; i--) {
        double acc = -A[i][8];
        EPIPOLAR_RULES_UNROLL
        for (int q = i + 1; q < 8; q++) acc = acc - A[i][q] * z[q];
        z[i] = acc / A[i][i];
    }
    EPIPOLAR_RULES_UNROLL
    for (int j = 0; j < 9; j++) {
        double f = 0.0;
        EPIPOLAR_RULES_UNROLL
        for (int pos = 0; pos < 9; pos++) f = perm[pos] == j ? z[pos] : f;
        Fn[j] = f;
    }
    return true;
}

// F = (Td^T Fn) Ts, scaled and signed, with T = [s 0 tx; 0 s ty; 0 0 1] on each side; false: not finite or zero, F undefined
VERIFY_RULES_HD inline bool finish(const double Fn[9], double ss, double txs, double tys, double sd, double txd, double tyd, double F[9])
{
    VERIFY_RULES_NO_FMA
    const double TdT[9] = {sd, 0.0, 0.0, 0.0, sd, 0.0, txd, tyd, 1.0};
    const double Ts[9] = {ss, 0.0, txs, 0.0, ss, tys, 0.0, 0.0, 1.0};
    double T[9];
    vr::mul3(TdT, Fn, T);
    vr::mul3(T, Ts, F);
    if (!vr::normalise(F)) return false;
    double mx = 0.0;
    EPIPOLAR_RULES_UNROLL
    for (int i = 0; i < 9; i++) { const double a = __builtin_fabs(F[i]); mx = a > mx ? a : mx; }
    bool found = false, flip = false;
    EPIPOLAR_RULES_UNROLL
    for (int i = 0; i < 9; i++) {
        const bool here = !found && __builtin_fabs(F[i]) == mx;
        flip = here ? F[i] < 0.0 : flip;
        found = found || here;
    }
    EPIPOLAR_RULES_UNROLL
    for (int i = 0; i < 9; i++) F[i] = flip ? -F[i] : F[i];
    return true;
}

// F [9] row-major from the eight matches (sx[i], sy[i]) -> (dx[i], dy[i]), which are overwritten; false: invalid, F is all zero
VERIFY_RULES_HD inline bool model(double sx[kSample], double sy[kSample], double dx[kSample], double dy[kSample], double F[9])
{
    EPIPOLAR_RULES_UNROLL
    for (int i = 0; i < 9; i++) F[i] = 0.0;
    double ss, txs, tys, sd, txd, tyd, Fn[9], T[9];
    if (!local_norm(sx, sy, ss, txs, tys) || !local_norm(dx, dy, sd, txd, tyd)) return false;
    if (!eight_point(sx, sy, dx, dy, Fn)) return false;
    if (!finish(Fn, ss, txs, tys, sd, txd, tyd, T)) return false;
    EPIPOLAR_RULES_UNROLL
    for (int i = 0; i < 9; i++) F[i] = T[i];
    return true;
}

// hypothesis h of the call: its sample idx [8] and F [9] (all zero when invalid)
VERIFY_RULES_HD inline bool hypothesis(const float *src, const float *dst, uint32_t m, uint64_t seed, uint32_t h, int32_t idx[kSample], double F[9])
{
    EPIPOLAR_RULES_UNROLL
    for (int i = 0; i < 9; i++) F[i] = 0.0;
    if (!sample(seed, h, m, idx)) return false;
    double sx[kSample], sy[kSample], dx[kSample], dy[kSample];
    EPIPOLAR_RULES_UNROLL
    for (int i = 0; i < kSample; i++) {
        sx[i] = (double)src[2 * (int64_t)idx[i]]; sy[i] = (double)src[2 * (int64_t)idx[i] + 1];
        dx[i] = (double)dst[2 * (int64_t)idx[i]]; dy[i] = (double)dst[2 * (int64_t)idx[i] + 1];
    }
    return model(sx, sy, dx, dy, F);
}

// the match (x, y) -> (u, v) is an inlier of F
VERIFY_RULES_HD inline bool inlier(const double F[9], double x, double y, double u, double v, double t2)
{
    VERIFY_RULES_NO_FMA
    const double l0 = (F[0] * x + F[1] * y) + F[2];
    const double l1 = (F[3] * x + F[4] * y) + F[5];
    const double l2 = (F[6] * x + F[7] * y) + F[8];
    const double e = (u * l0 + v * l1) + l2;
    const double m0 = (F[0] * u + F[3] * v) + F[6];
    const double m1 = (F[1] * u + F[4] * v) + F[7];
    const double S = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
    return S > 0.0 && e * e <= t2 * S;
}

// ---- the pieces of a refit round that the host below and refit_pairs_kernel (kernels_verify.hip) share: everything but the
// sums, which both walk over the inliers in ascending match index.  Whatever is indexed at run time comes through a pointer,
// so that the kernel can keep it in LDS ---------------------------------------------------------------------------------------
// the row a [9] of a normalised match (x, y) -> (u, v)
VERIFY_RULES_HD inline void refit_row(double x, double y, double u, double v, double *a)
{
    VERIFY_RULES_NO_FMA
    a[0] = u * x; a[1] = u * y; a[2] = u; a[3] = v * x; a[4] = v * y; a[5] = v; a[6] = x; a[7] = y; a[8] = 1.0;
}

// one term of N[p][q]: a = a[p], b = a[q]
VERIFY_RULES_HD inline double refit_add(double acc, double a, double b)
{
    VERIFY_RULES_NO_FMA
    return acc + a * b;
}

// the sums of a round as refit_pairs_kernel spreads them over lanes (verify_rules::Terms): l < 81 is N[l / 9][l % 9]
constexpr int kRefitRow = 9, kRefitSums = 81;
VERIFY_RULES_HD inline vr::Terms refit_terms(int l) { return l < kRefitSums ? vr::Terms{l / 9, l % 9, 0, 0} : vr::Terms{0, 0, 0, 0}; }
VERIFY_RULES_HD inline double refit_add(double acc, const double *row, vr::Terms t) { return refit_add(acc, row[t.a], row[t.b]); }

// cyclic Jacobi of the symmetric N [n][n] (row-major, n <= 9): N's diagonal becomes the eigenvalues, V [n][n] the eigenvectors
// in its columns; returns the number of sweeps that rotated
VERIFY_RULES_HD inline int jacobi(double *N, int n, double *V)
{
    VERIFY_RULES_NO_FMA
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) V[n * i + j] = i == j ? 1.0 : 0.0;
    int sweeps = 0;
    for (; sweeps < kMaxSweeps; sweeps++) {
        int rotated = 0;
        for (int p = 0; p < n; p++)
            for (int q = p + 1; q < n; q++) {
                const double a = N[n * p + q];
                if (a == 0.0) continue;
                rotated++;
                const double theta = (N[n * q + q] - N[n * p + p]) / (2.0 * a);
                const double den = __builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0);
                const double t = (theta < 0.0 ? -1.0 : 1.0) / den;
                const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
                N[n * p + p] = N[n * p + p] - t * a;
                N[n * q + q] = N[n * q + q] + t * a;
                N[n * p + q] = N[n * q + p] = 0.0;
                for (int r = 0; r < n; r++) {
                    if (r == p || r == q) continue;
                    const double g = N[n * r + p], h = N[n * r + q];
                    N[n * r + p] = N[n * p + r] = c * g - s * h;
                    N[n * r + q] = N[n * q + r] = s * g + c * h;
                }
                for (int r = 0; r < n; r++) {
                    const double g = V[n * r + p], h = V[n * r + q];
                    V[n * r + p] = c * g - s * h;
                    V[n * r + q] = s * g + c * h;
                }
            }
        if (rotated == 0) break;
    }
    return sweeps;
}

// vec [n] = the eigenvector of the smallest eigenvalue of the symmetric N [n][n], which is overwritten (ties: lowest index);
// V [n][n] is scratch
VERIFY_RULES_HD inline void smallest_eigenvector(double *N, int n, double *V, double *vec)
{
    jacobi(N, n, V);
    int best = 0;
    for (int i = 1; i < n; i++)
        if (N[n * i + i] < N[n * best + best]) best = i;
    for (int j = 0; j < n; j++) vec[j] = V[n * j + best];
}

constexpr int kRefitWork = 21;                             // doubles of refit_solve's w: Fn [9], G [9], v [3]

// F' of the summed N [81], which is overwritten: the smallest eigenvector, the rank-2 step, finish; V [81] and w [kRefitWork]
// are scratch; false: F' is not finite or is zero
VERIFY_RULES_HD inline bool refit_solve(double *N, double *V, double *w, double cxs, double cys, double ss, double cxd, double cyd, double sd,
                                        double F_out[9])
{
    VERIFY_RULES_NO_FMA
    double *Fn = w, *G = w + 9, *v = w + 18;
    double FnT[9], Fr[9];
    smallest_eigenvector(N, 9, V, Fn);
    EPIPOLAR_RULES_UNROLL
    for (int i = 0; i < 3; i++) {
        EPIPOLAR_RULES_UNROLL
        for (int j = 0; j < 3; j++) FnT[3 * i + j] = Fn[3 * j + i];
    }
    EPIPOLAR_RULES_UNROLL
    for (int i = 0; i < 9; i++) Fr[i] = Fn[i];
    vr::mul3(FnT, Fr, G);
    smallest_eigenvector(G, 3, V, v);
    EPIPOLAR_RULES_UNROLL
    for (int i = 0; i < 3; i++) {
        const double d = (Fr[3 * i] * v[0] + Fr[3 * i + 1] * v[1]) + Fr[3 * i + 2] * v[2];
        EPIPOLAR_RULES_UNROLL
        for (int j = 0; j < 3; j++) Fr[3 * i + j] = Fr[3 * i + j] - d * v[j];
    }
    return finish(Fr, ss, -(ss * cxs), -(ss * cys), sd, -(sd * cxd), -(sd * cyd), F_out);
}

// ---- the rule on the host: what the kernels must reproduce ---------------------------------------------------------------
inline void smallest_eigenvector(double *N, int n, double *vec)
{
    double V[81];
    smallest_eigenvector(N, n, V, vec);
}

// one round of the refit on the inliers of mask: F' in F_out; false: rejected, F_out is undefined
inline bool refit_round(const float *src, const float *dst, int64_t m, const uint8_t *mask, double F_out[9])
{
    int64_t n = 0;
    for (int64_t i = 0; i < m; i++) n += mask[i] ? 1 : 0;
    if (n < kSample) return false;
    double cxs, cys, ss, cxd, cyd, sd;
    if (!vr::hartley(src, mask, m, cxs, cys, ss) || !vr::hartley(dst, mask, m, cxd, cyd, sd)) return false;
    double N[81] = {}, V[81], w[kRefitWork];
    for (int64_t i = 0; i < m; i++) {
        if (!mask[i]) continue;
        double a[9];
        refit_row(vr::normalised((double)src[2 * i], cxs, ss), vr::normalised((double)src[2 * i + 1], cys, ss), vr::normalised((double)dst[2 * i], cxd, sd),
                  vr::normalised((double)dst[2 * i + 1], cyd, sd), a);
        for (int p = 0; p < 9; p++)
            for (int q = 0; q < 9; q++) N[9 * p + q] = refit_add(N[9 * p + q], a[p], a[q]);
    }
    return refit_solve(N, V, w, cxs, cys, ss, cxd, cyd, sd, F_out);
}

// The fundamental matrix as the frame of verify_rules.hpp (all_hypotheses, count_inliers, verify_host) and the kernels
// (kernels_verify.hip) take a model: the sample size and the three functions above, nothing of its own.
struct Fundamental {
    static constexpr int kSample = epipolar_rules::kSample;
    VERIFY_RULES_HD static bool hypothesis(const float *src, const float *dst, uint32_t m, uint64_t seed, uint32_t h, int32_t idx[kSample], double F[9])
    {
        return epipolar_rules::hypothesis(src, dst, m, seed, h, idx, F);
    }
    VERIFY_RULES_HD static bool inlier(const double F[9], double x, double y, double u, double v, double t2)
    {
        return epipolar_rules::inlier(F, x, y, u, v, t2);
    }
    static bool refit_round(const float *src, const float *dst, int64_t m, const uint8_t *mask, double F_out[9])
    {
        return epipolar_rules::refit_round(src, dst, m, mask, F_out);
    }
    // the round as refit_pairs_kernel takes a model (verify_rules::Homography says what each is): work = N [81] summed, V [81], w
    static constexpr int kRefitRow = epipolar_rules::kRefitRow, kRefitSums = epipolar_rules::kRefitSums, kRefitWork = 81 + 81 + epipolar_rules::kRefitWork;
    VERIFY_RULES_HD static void refit_row(double x, double y, double u, double v, double *a) { epipolar_rules::refit_row(x, y, u, v, a); }
    VERIFY_RULES_HD static vr::Terms refit_terms(int l) { return epipolar_rules::refit_terms(l); }
    VERIFY_RULES_HD static double refit_add(double acc, const double *a, vr::Terms t) { return epipolar_rules::refit_add(acc, a, t); }
    VERIFY_RULES_HD static bool refit_few(int n) { return n < kSample; }
    VERIFY_RULES_HD static bool refit_solve(double *work, double cxs, double cys, double ss, double cxd, double cyd, double sd, double, double,
                                            double F_out[9])
    {
        return epipolar_rules::refit_solve(work, work + 81, work + 162, cxs, cys, ss, cxd, cyd, sd, F_out);
    }
};

// the frame with the fundamental matrix under this namespace's plain names: what the tests' shims call
inline void all_hypotheses(const float *src, const float *dst, int64_t m, int32_t n_hyp, uint64_t seed, double *F_all, int32_t *idx_all,
                           uint8_t *valid)
{
    vr::all_hypotheses<Fundamental>(src, dst, m, n_hyp, seed, F_all, idx_all, valid);
}
inline int64_t count_inliers(const double F[9], const float *src, const float *dst, int64_t m, double t2, uint8_t *mask)
{
    return vr::count_inliers<Fundamental>(F, src, dst, m, t2, mask);
}
inline void verify_host(const float *src, const float *dst, int64_t m, float threshold, int32_t n_hyp, uint64_t seed, int32_t refine, double *F_all,
                        int32_t *counts, double F[9], uint8_t *mask, int64_t *count, int32_t *best_hyp, double *rounds, int32_t *n_rounds)
{
    vr::verify_host<Fundamental>(src, dst, m, threshold, n_hyp, seed, refine, F_all, counts, F, mask, count, best_hyp, rounds, n_rounds);
}

}  // namespace epipolar_rules
