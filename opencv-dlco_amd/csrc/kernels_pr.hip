// kernels_pr.hip — pr-learn: the pooling-region stage of the pipeline on gfx950.
//
// The reference's loop (src/pr-learn.cpp:302-329) is a strictly sequential stochastic method: one
// (positive, negative) row pair per iteration, a 5120-term dot product whose SIGN decides the update,
// and three element-wise vector updates; iteration t+1 needs the w of iteration t.  There is nothing to
// batch, so the whole window of iterations between two log steps (100 000 in the reference) runs inside
// ONE launch of one workgroup: w and dfAvg live in registers (20 floats per thread at F = 5120), the two
// rows of the next iteration are prefetched while the current one is reduced, and an iteration costs one
// workgroup barrier.  Arithmetic follows the reference operation for operation (double accumulation of
// the dot product like cv::gemm, the float scale factors of the MatExpr / scaleAdd calls, products and
// sums NOT fused), so the trajectory is the oracle's, bit for bit, as long as no dot product lands
// within one double-rounding of a float boundary.
//
// A grid of (mu, gamma) settings (pr_grid_steps_kernel) batches what the reference runs as separate
// pr-learn processes: the settings are independent chains on the same sampled rows, so a workgroup
// applies each fetched row pair to several of them, with the per-iteration functions of the solo kernel.
#include "dlco_internal.hpp"

namespace dlco {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int PT = 256;           // threads of the sequential kernel
constexpr int PW = PT / 64;

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The per-iteration arithmetic of src/pr-learn.cpp:312-329, shared by the solo and the grid kernel so that
// the two cannot drift apart.  Thread tid owns the 16-byte chunks c = tid + PT * u of w, dfAvg and the row
// difference d (zero past F).  Products and sums are NOT fused (the pragma holds inside each function).

// this thread's share of w . d, accumulated in double chunk by chunk, element by element (gemm in double, :319)
template <int CH>
__device__ __forceinline__ double pr_partial_dot(const f32x4 (&w)[CH], const f32x4 (&d)[CH])
{
#pragma clang fp contract(off)
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < CH; u++)
#pragma unroll
        for (int e = 0; e < 4; e++) acc += (double)w[u][e] * (double)d[u][e];
    return acc;
}

// the dot product: the PW wave sums in wave order
__device__ __forceinline__ double pr_sum_parts(const double *part)
{
#pragma clang fp contract(off)
    double tot = 0.0;
#pragma unroll
    for (int q = 0; q < PW; q++) tot += part[q];
    return tot;
}

// dual average and soft threshold of iteration t given the dot product tot (:322-329); returns f
template <int CH>
__device__ __forceinline__ float pr_update(f32x4 (&w)[CH], f32x4 (&df)[CH], const f32x4 (&d)[CH], double tot, unsigned t, float mu,
                                           float gamma)
{
#pragma clang fp contract(off)
    const float f = (float)tot;
    const float sa = (float)((double)t * (1.0 / ((double)t + 1.0)));            // :322
    const float al = (float)(1.0 / ((double)t + 1.0));                           // :325
    const double a = -sqrt((double)t + 1.0) / (double)gamma;                     // :328
    const float fa = (float)a, fb = (float)((double)mu * a);
    const bool upd = f > -1.0f;                                                  // :324
#pragma unroll
    for (int u = 0; u < CH; u++)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            float v = df[u][e] * sa;
            if (upd) { const float p = d[u][e] * al; v = p + v; }
            df[u][e] = v;
            const float q = v * fa;
            const float r = q + fb;
            w[u][e] = r > 0.0f ? r : 0.0f;                                       // :329
        }
    return f;
}

// CH = 16-byte chunks of w per thread (F <= 1024 * CH)
template <int CH>
__global__ __launch_bounds__(PT) void pr_steps_kernel(const float *D, long ld, const int32_t *pos_rows, const int32_t *neg_rows,
                                                      unsigned n, unsigned t0, float mu, float gamma, int F, float *w_io,
                                                      float *df_io, float *last_f)
{
#pragma clang fp contract(off)
    __shared__ double part[2][PW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = F >> 2;
    f32x4 w[CH], df[CH], xp[CH], xn[CH];
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < CH; u++) {
        const int c = tid + PT * u;
        w[u] = c < nch ? reinterpret_cast<const f32x4 *>(w_io)[c] : z4;
        df[u] = c < nch ? reinterpret_cast<const f32x4 *>(df_io)[c] : z4;
    }
    auto fetch = [&](unsigned s) {
        const f32x4 *rp = reinterpret_cast<const f32x4 *>(D + (long)pos_rows[s] * ld);
        const f32x4 *rn = reinterpret_cast<const f32x4 *>(D + (long)neg_rows[s] * ld);
#pragma unroll
        for (int u = 0; u < CH; u++) {
            const int c = tid + PT * u;
            xp[u] = c < nch ? rp[c] : z4;
            xn[u] = c < nch ? rn[c] : z4;
        }
    };
    if (n > 0) fetch(0);
    float f = 0.f;
    for (unsigned s = 0; s < n; s++) {
        f32x4 d[CH];
#pragma unroll
        for (int u = 0; u < CH; u++) d[u] = xp[u] - xn[u];                      // subtract(), :312-314
        double acc = pr_partial_dot<CH>(w, d);
        if (s + 1 < n) fetch(s + 1);                           // the next iteration's rows travel meanwhile
        acc = wave_sum_f64(acc);
        if (lane == 0) part[s & 1][wave] = acc;
        __syncthreads();
        f = pr_update<CH>(w, df, d, pr_sum_parts(part[s & 1]), t0 + s, mu, gamma);
    }
#pragma unroll
    for (int u = 0; u < CH; u++) {
        const int c = tid + PT * u;
        if (c < nch) {
            reinterpret_cast<f32x4 *>(w_io)[c] = w[u];
            reinterpret_cast<f32x4 *>(df_io)[c] = df[u];
        }
    }
    if (tid == 0 && last_f) *last_f = f;
}

// A grid of G independent settings (mu[k], gamma[k]) on the same sampled rows: workgroup b runs settings
// b*C .. b*C+C-1.  The row pair of iteration s is fetched once per workgroup and applied to all C
// settings, whose w and dfAvg stay in registers; one barrier per iteration for all of them.  Per setting
// the arithmetic is pr_steps_kernel's (same thread-to-column map, same functions).  w / dfAvg are [G][ldw]
// (ldw >= F, a multiple of 4); settings past G in the last workgroup run on zeros and are never stored.
template <int CH, int C>
__global__ __launch_bounds__(PT) void pr_grid_steps_kernel(const float *D, long ld, const int32_t *pos_rows, const int32_t *neg_rows,
                                                           unsigned n, unsigned t0, const float *mu, const float *gamma, int G, int F,
                                                           long ldw, float *w_io, float *df_io)
{
#pragma clang fp contract(off)
    __shared__ double part[2][C][PW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = F >> 2, g0 = blockIdx.x * C;
    f32x4 w[C][CH], df[C][CH], xp[CH], xn[CH];
    float mu_k[C], gamma_k[C];
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < C; k++) {
        const bool live = g0 + k < G;
        const f32x4 *wk = reinterpret_cast<const f32x4 *>(w_io + (long)(g0 + k) * ldw);
        const f32x4 *dk = reinterpret_cast<const f32x4 *>(df_io + (long)(g0 + k) * ldw);
        mu_k[k] = live ? mu[g0 + k] : 0.f;
        gamma_k[k] = live ? gamma[g0 + k] : 1.f;
#pragma unroll
        for (int u = 0; u < CH; u++) {
            const int c = tid + PT * u;
            w[k][u] = live && c < nch ? wk[c] : z4;
            df[k][u] = live && c < nch ? dk[c] : z4;
        }
    }
    auto fetch = [&](unsigned s) {
        const f32x4 *rp = reinterpret_cast<const f32x4 *>(D + (long)pos_rows[s] * ld);
        const f32x4 *rn = reinterpret_cast<const f32x4 *>(D + (long)neg_rows[s] * ld);
#pragma unroll
        for (int u = 0; u < CH; u++) {
            const int c = tid + PT * u;
            xp[u] = c < nch ? rp[c] : z4;
            xn[u] = c < nch ? rn[c] : z4;
        }
    };
    if (n > 0) fetch(0);
    for (unsigned s = 0; s < n; s++) {
        f32x4 d[CH];
#pragma unroll
        for (int u = 0; u < CH; u++) d[u] = xp[u] - xn[u];
        double acc[C];
#pragma unroll
        for (int k = 0; k < C; k++) acc[k] = pr_partial_dot<CH>(w[k], d);
        if (s + 1 < n) fetch(s + 1);
#pragma unroll
        for (int k = 0; k < C; k++) {
            acc[k] = wave_sum_f64(acc[k]);
            if (lane == 0) part[s & 1][k][wave] = acc[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < C; k++) pr_update<CH>(w[k], df[k], d, pr_sum_parts(part[s & 1][k]), t0 + s, mu_k[k], gamma_k[k]);
    }
#pragma unroll
    for (int k = 0; k < C; k++) {
        if (g0 + k >= G) continue;
        f32x4 *wk = reinterpret_cast<f32x4 *>(w_io + (long)(g0 + k) * ldw);
        f32x4 *dk = reinterpret_cast<f32x4 *>(df_io + (long)(g0 + k) * ldw);
#pragma unroll
        for (int u = 0; u < CH; u++) {
            const int c = tid + PT * u;
            if (c < nch) {
                wk[c] = w[k][u];
                dk[c] = df[k][u];
            }
        }
    }
}

// One lane's term of the row . w products below: 4 columns, the expression of both gemv kernels.
__device__ __forceinline__ double gemv_term_f64(const f32x4 a, const f32x4 b)
{
    return (double)a[0] * b[0] + (double)a[1] * b[1] + (double)a[2] * b[2] + (double)a[3] * b[3];
}
__device__ __forceinline__ float gemv_term_f32(const f32x4 a, const f32x4 b)
{
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
}

// out[i] = w . D[row(i)]; one wave per row.  DOUBLE = accumulate in double (cv::gemm on the CPU,
// src/misc.cpp:226), else in float (cuda::gemm, src/pr-learn.cpp:343-344: order unspecified).
template <bool DOUBLE>
__global__ __launch_bounds__(256) void pr_gemv_kernel(const float *D, long ld, const int32_t *ids, int n, const float *w, int F, float *out)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const f32x4 *x = reinterpret_cast<const f32x4 *>(D + (long)(ids ? ids[row] : row) * ld);
    const f32x4 *w4 = reinterpret_cast<const f32x4 *>(w);
    if (DOUBLE) {
        double s = 0.0;
        for (int c = lane; c < F / 4; c += 64) s += gemv_term_f64(x[c], w4[c]);
        s = wave_sum_f64(s);
        if (lane == 0) out[row] = (float)s;
    } else {
        float s = 0.f;
        for (int c = lane; c < F / 4; c += 64) s += gemv_term_f32(x[c], w4[c]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) out[row] = s;
    }
}

// pr_gemv_kernel for several weight vectors at once: the wave keeps its row in registers (RC 16-byte
// chunks per lane, F <= 256 * RC) and takes it through the vectors W + sel[k] * ldw, k < nsel (sel NULL:
// k), writing out[k * ldo + i].  Each row is read once for all of them; per vector the lane order and the
// reduction are pr_gemv_kernel's, so every distance is bit-identical to a single-vector launch.
template <bool DOUBLE, int RC>
__global__ __launch_bounds__(256) void pr_gemv_multi_kernel(const float *D, long ld, const int32_t *ids, int n, const float *W, long ldw,
                                                            const int32_t *sel, int nsel, int F, float *out, long ldo)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const int nch = F / 4;
    const f32x4 *x = reinterpret_cast<const f32x4 *>(D + (long)(ids ? ids[row] : row) * ld);
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 xr[RC];
#pragma unroll
    for (int j = 0; j < RC; j++) xr[j] = lane + 64 * j < nch ? x[lane + 64 * j] : z4;
    for (int k = 0; k < nsel; k++) {
        const f32x4 *w4 = reinterpret_cast<const f32x4 *>(W + (long)(sel ? sel[k] : k) * ldw);
        if (DOUBLE) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < RC; j++)
                if (lane + 64 * j < nch) s += gemv_term_f64(xr[j], w4[lane + 64 * j]);
            s = wave_sum_f64(s);
            if (lane == 0) out[(long)k * ldo + row] = (float)s;
        } else {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < RC; j++)
                if (lane + 64 * j < nch) s += gemv_term_f32(xr[j], w4[lane + 64 * j]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) out[(long)k * ldo + row] = s;
        }
    }
}

}  // namespace

bool pr_steps(const float *D, long ld, const int32_t *pos_rows, const int32_t *neg_rows, unsigned n, unsigned t0, float mu, float gamma,
              int F, float *w_io, float *df_io, float *last_f, hipStream_t s)
{
    if (F % 4 != 0 || F > 1024 * 8 || ld % 4 != 0) return false;
    const int ch = (F / 4 + PT - 1) / PT;
#define DLCO_PR_LAUNCH(C) hipLaunchKernelGGL(pr_steps_kernel<C>, dim3(1), dim3(PT), 0, s, D, ld, pos_rows, neg_rows, n, t0, mu, gamma, F, w_io, df_io, last_f)
    if (ch <= 1) DLCO_PR_LAUNCH(1);
    else if (ch <= 2) DLCO_PR_LAUNCH(2);
    else if (ch <= 4) DLCO_PR_LAUNCH(4);
    else if (ch <= 5) DLCO_PR_LAUNCH(5);
    else DLCO_PR_LAUNCH(8);
#undef DLCO_PR_LAUNCH
    DLCO_HIP(hipGetLastError());
    return true;
}

// Settings per workgroup: one while every setting gets a CU of its own (a workgroup then
// iterates at the solo rate; C = 1 is 1.4x C = 2 there), two beyond that up to F = 5120 (G = 768 on 256
// CUs: 316 M setting-iterations/s against 249 M for C = 1 and 245 M for C = 4).  At F = 8192 C = 2 holds
// 354 registers per thread, half the waves per SIMD of C = 1, and loses (146 M against 187 M at G = 768).
int pr_grid_group(int G, int F, int cus)
{
    return G > cus && F <= 1024 * 5 ? 2 : 1;
}

bool pr_grid_steps(const float *D, long ld, const int32_t *pos_rows, const int32_t *neg_rows, unsigned n, unsigned t0, const float *mu,
                   const float *gamma, int G, int group, int F, long ldw, float *w_io, float *df_io, hipStream_t s)
{
    if (F % 4 != 0 || F > 1024 * 8 || ld % 4 != 0 || ldw % 4 != 0 || ldw < F || G < 1) return false;
    if (group != 1 && group != 2 && group != 4) return false;
    const int ch = (F / 4 + PT - 1) / PT;
    if (ch > 5 && group == 4) return false;                    // C = 4 at CH = 8 does not fit the register file
    const dim3 grid((unsigned)((G + group - 1) / group));
#define DLCO_PR_GRID_LAUNCH(CH, C) hipLaunchKernelGGL((pr_grid_steps_kernel<CH, C>), grid, dim3(PT), 0, s, D, ld, pos_rows, neg_rows, n, t0, \
                                                      mu, gamma, G, F, ldw, w_io, df_io)
#define DLCO_PR_GRID_C(CH) \
    do { if (group == 1) DLCO_PR_GRID_LAUNCH(CH, 1); else if (group == 2) DLCO_PR_GRID_LAUNCH(CH, 2); else DLCO_PR_GRID_LAUNCH(CH, 4); } while (0)
    if (ch <= 1) DLCO_PR_GRID_C(1);
    else if (ch <= 2) DLCO_PR_GRID_C(2);
    else if (ch <= 4) DLCO_PR_GRID_C(4);
    else if (ch <= 5) DLCO_PR_GRID_C(5);
    else if (group == 1) DLCO_PR_GRID_LAUNCH(8, 1);
    else DLCO_PR_GRID_LAUNCH(8, 2);
#undef DLCO_PR_GRID_C
#undef DLCO_PR_GRID_LAUNCH
    DLCO_HIP(hipGetLastError());
    return true;
}

void pr_gemv_multi(const float *D, long ld, const int32_t *ids, int n, const float *W, long ldw, const int32_t *sel, int nsel, int F,
                   float *out, long ldo, bool in_double, hipStream_t s)
{
    if (n <= 0 || nsel <= 0) return;
    const int rc = (F / 4 + 63) / 64;
    const dim3 grid((unsigned)((n + 3) / 4));
#define DLCO_PR_MULTI(RC)                                                                                                               \
    do {                                                                                                                                \
        if (in_double) hipLaunchKernelGGL((pr_gemv_multi_kernel<true, RC>), grid, dim3(256), 0, s, D, ld, ids, n, W, ldw, sel, nsel, F, out, ldo); \
        else hipLaunchKernelGGL((pr_gemv_multi_kernel<false, RC>), grid, dim3(256), 0, s, D, ld, ids, n, W, ldw, sel, nsel, F, out, ldo);      \
    } while (0)
    if (rc <= 2) DLCO_PR_MULTI(2);
    else if (rc <= 4) DLCO_PR_MULTI(4);
    else if (rc <= 8) DLCO_PR_MULTI(8);
    else if (rc <= 16) DLCO_PR_MULTI(16);
    else if (rc <= 20) DLCO_PR_MULTI(20);
    else DLCO_PR_MULTI(32);
#undef DLCO_PR_MULTI
    DLCO_HIP(hipGetLastError());
}

void pr_gemv(const float *D, long ld, const int32_t *ids, int n, const float *w, int F, float *out, bool in_double, hipStream_t s)
{
    if (n <= 0) return;
    if (in_double) hipLaunchKernelGGL(pr_gemv_kernel<true>, dim3((n + 3) / 4), dim3(256), 0, s, D, ld, ids, n, w, F, out);
    else hipLaunchKernelGGL(pr_gemv_kernel<false>, dim3((n + 3) / 4), dim3(256), 0, s, D, ld, ids, n, w, F, out);
    DLCO_HIP(hipGetLastError());
}

}  // namespace dlco
