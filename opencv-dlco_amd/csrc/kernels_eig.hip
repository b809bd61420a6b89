// kernels_eig.hip — vector kernels and the CholQR building block of the subspace tracker
// (E1/E2 of the pj-learn step, src/pj-learn.cpp:434-490), for gfx950.  The Rayleigh-Ritz
// eigensolver itself is in kernels_jacobi.hip.
#include "dlco_internal.hpp"

#include <type_traits>

namespace dlco {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wsum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void residual_kernel(const float *X, const float *Y, long ld, const float *theta,
                                                       int m, int F, float *res)
{
    __shared__ float part[4];
    const int i = blockIdx.x;
    if (i >= m) return;
    const float th = theta[i];
    float s = 0.f;
    if ((F & 3) == 0 && (ld & 3) == 0) {                  // 16-byte accesses (rows are 16-byte aligned)
        const f32x4 *y4 = reinterpret_cast<const f32x4 *>(Y + (long)i * ld), *x4 = reinterpret_cast<const f32x4 *>(X + (long)i * ld);
        for (int f = threadIdx.x; f < F / 4; f += blockDim.x) {
            const f32x4 d = y4[f] - th * x4[f];
            s += d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
        }
    } else {
        for (int f = threadIdx.x; f < F; f += blockDim.x) {
            const float d = Y[(long)i * ld + f] - th * X[(long)i * ld + f];
            s += d * d;
        }
    }
    s = wsum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) res[i] = sqrtf(part[0] + part[1] + part[2] + part[3]);
}

// rows whose norm is below `min_norm` are zeroed (dependent directions), the rest scaled to unit norm
__global__ __launch_bounds__(256) void row_normalize_kernel(float *X, long ld, int m, int F, float min_norm)
{
    __shared__ float part[4];
    __shared__ float inv;
    const int i = blockIdx.x;
    if (i >= m) return;
    float s = 0.f;
    const bool vec = (F & 3) == 0 && (ld & 3) == 0;       // 16-byte accesses (rows are 16-byte aligned)
    f32x4 *x4 = reinterpret_cast<f32x4 *>(X + (long)i * ld);
    if (vec) {
        for (int f = threadIdx.x; f < F / 4; f += blockDim.x) { const f32x4 v = x4[f]; s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]; }
    } else {
        for (int f = threadIdx.x; f < F; f += blockDim.x) { const float v = X[(long)i * ld + f]; s += v * v; }
    }
    s = wsum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) { const float n2 = part[0] + part[1] + part[2] + part[3]; inv = (n2 > 0.f && n2 >= min_norm * min_norm) ? 1.f / sqrtf(n2) : 0.f; }
    __syncthreads();
    const float sc = inv;
    if (vec) {
        for (int f = threadIdx.x; f < F / 4; f += blockDim.x) x4[f] = x4[f] * sc;
    } else {
        for (int f = threadIdx.x; f < F; f += blockDim.x) X[(long)i * ld + f] *= sc;
    }
}

__global__ __launch_bounds__(256) void symv_kernel(const float *H, long ld, int F, const float *x, float *y)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= F) return;
    float s = 0.f;
    for (int f = lane; f < F; f += 64) s += H[(long)row * ld + f] * x[f];
    s = wsum(s);
    if (lane == 0) y[row] = s;
}

// CholQR building block: Gram matrix M (n <= 160, lower triangle read) -> Linv = L^-1 with M = L L^T, on one workgroup.
//
// Right-looking elimination without pivoting on the augmented matrix [M | I]: step j subtracts (A_ij / A_jj) * row j
// from every row i > j.  The left half turns into the Schur complements (pivot d_j = A_jj at step j), the right half into
// U^-1 of M = U D U^T, and L^-1 = D^-1/2 U^-1.  A row whose pivot drops below rel_thresh * M_jj lies (to fp32 accuracy) in
// the span of the rows before it: it is marked dead, eliminated from nothing, and its row of Linv is zero.  (Round 1's
// kernel did this one pivot per workgroup barrier - ~1.2 us each, 114 us at n = 96; it left the library in round 4.)
// ---- blocked: 32 pivots per workgroup barrier instead of one --------------------------------------------
// The elimination of [M | I] proceeds in blocks of 32 pivots:
//   1. the 32 x 32 diagonal block D goes to LDS and ONE wave eliminates it in registers (lane i = row i of D; the
//      pivot row reaches the other lanes through v_readlane, no barrier inside the 32 steps), which yields the
//      pivots d, the dead flags and the multipliers f_ij of the block's steps.  That wave is the kernel's chain: one
//      wave issues a dependent instruction every 4-5 cycles, so a step costs what its readlane + FMA pairs cost;
//   2. the identity half of [D | I] - the unit lower triangular T = L1^-1 - is not on that chain: its column k joins at
//      step k and needs only the multipliers.  All sixteen waves build it from them, two columns each;
//   3. every thread then applies the block's 32 steps at once to its entries: the block's rows become
//      P = T * rows, the multipliers of the rows below are F = (A[:,K] T^T) / d (the Schur complement
//      is symmetric, so U_KK^-1 = T^T D^-1), and the trailing update is the rank-32 product F * P.
// The matrix stays in registers (thread (ty, tx) holds rows ty + 32 r, columns tx + 32 c of [M | I]); LDS only
// carries the block's rows, columns, multipliers, T, P and F.  Four barriers per block of 32 pivots.  The multipliers
// are a[j] * rcp(d) instead of a[j] / d (CholQR2's second pass absorbs that).  Fast path for M = I + E with
// |E|_F^2 <= 1e-6 (the second pass of CholQR2): M^-1/2 = I - E/2, no elimination.
// Measured (tools/kern_time small, s_memtime stamps of the eliminating wave: profiles/chol_phases_*.txt).  Until the
// eliminating wave shed the identity half it carried both halves - 32 pairs per step whatever the step, 16 000 cycles
// per block, half the kernel at n = 96 - and parked its matrix entries in LDS meanwhile; the products of step 3 read
// LDS four bytes at a time along j.  Now: D alone 10 800 cycles per block, T 3 500, step 3 on 16-byte reads (P and F
// 11 900 -> 5 400 cycles in the first block of n = 96, the trailing update 7 500 -> 5 600 with the wait for the slowest
// wave); 39.7 -> 30.8 us at n = 96, 63.4 -> 48.6 at 128, 94.2 -> 71.9 at 160 (10.0 -> 10.3 at n = 32: one barrier
// more), every entry of Linv through the same FMAs in the same order: the same bits
// (tests/test_chol_probe_gpu.py).  Tried and taken out: D in the lower and the
// identity half in the upper half-wave (the multiplier handed over by v_permlane32_swap) - the same 32 pairs per
// step in two EXEC regions, 18 000 cycles per block instead of 16 000.  Not built: the next block's diagonal
// eliminated beside the trailing update (its wave must first redo the F * P update of the 32 x 32 diagonal block on
// its own, ~2 000 cycles, to hide a trailing update of 3 100 - 5 600 with its wait: DESIGN section 9, item 2).
// NBM = blocks of 32 rows the kernel is built for: 4 (n <= 128) or 5 (n <= 160: the block of the rank ~128 workload in ONE
// orthonormalisation panel instead of two panels with a Gram-Schmidt step between them; 50 registers of matrix per thread).
constexpr int C2_T = 1024;
// LDS images read along the pivot index j are stored j-contiguous with a row stride of C2_LD = 36 floats: a thread
// fetches four consecutive j with one ds_read_b128 (rows stay 16-byte aligned), and the 16 lanes a ds_read_b128 serves
// per cycle - consecutive rows modulo 16 - fall on the 16 distinct 16-byte slots of the bank row (9 * row mod 16).
constexpr int C2_LD = 36;
__host__ __device__ constexpr size_t c2_lds_floats(int nbm)
{
    return (size_t)32 * 33 + 32 * C2_LD + 4 * 32 * nbm * C2_LD + 32 * nbm * 3 + 64;
}

__device__ __forceinline__ float readlane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// TR (developer aid, tools/kern_time): lane 0 of wave 0 - the eliminating wave - stamps s_memtime at the phase boundaries
// of every block into trace[1..]; trace[0] = number of stamps, trace[62], trace[63] = s_memrealtime at both ends.
constexpr int C2_STAMPS = CHOL_INV_STAMPS;
template <int NBM, bool TR = false>
__global__ __launch_bounds__(C2_T) void chol_inv2_kernel(const float *M, long ldm, int n, float rel_thresh, float *Linv, long ldl,
                                                         int *dead, unsigned long long *trace)
{
    int tri = 1;
    auto stamp = [&]() {
        if constexpr (TR) {
            unsigned long long now;
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now) :: "memory");
            __builtin_amdgcn_sched_barrier(0);
            if (threadIdx.x == 0 && tri < C2_STAMPS - 2) trace[tri++] = now;
        }
    };
    if constexpr (TR) { if (threadIdx.x == 0) trace[C2_STAMPS - 2] = __builtin_amdgcn_s_memrealtime(); }
    stamp();
    extern __shared__ __attribute__((aligned(16))) float c2[];
    float (*Dblk)[33] = reinterpret_cast<float (*)[33]>(c2);
    constexpr int NR = 32 * NBM;                               // NR: rows / columns the registers cover
    // Tblk[i][j] = T_ij; Praw / Pbuf[32 c + k][j]: entry (j, k) of column block c of the block's rows before / after T (of
    // M for c > kb, of the identity half for c <= kb: one slot per c serves both); Acol / Fbuf[row][j]: column j of the block
    float (*Tblk)[C2_LD] = reinterpret_cast<float (*)[C2_LD]>(c2 + 32 * 33);
    float (*Praw)[C2_LD] = reinterpret_cast<float (*)[C2_LD]>(c2 + 32 * 33 + 32 * C2_LD);
    float (*Pbuf)[C2_LD] = reinterpret_cast<float (*)[C2_LD]>(c2 + 32 * 33 + 32 * C2_LD + NR * C2_LD);
    float (*Acol)[C2_LD] = reinterpret_cast<float (*)[C2_LD]>(c2 + 32 * 33 + 32 * C2_LD + 2 * NR * C2_LD);
    float (*Fbuf)[C2_LD] = reinterpret_cast<float (*)[C2_LD]>(c2 + 32 * 33 + 32 * C2_LD + 3 * NR * C2_LD);
    float *diag0 = c2 + 32 * 33 + 32 * C2_LD + 4 * NR * C2_LD;
    float *dpiv = diag0 + NR;
    int *deadf = reinterpret_cast<int *>(dpiv + NR);
    float *dinv = dpiv + 2 * NR;                               // [32] of the current block, then scratch [16]
    const int t = threadIdx.x, tx = t & 31, ty = t >> 5;
    const int nb = (n + 31) >> 5;

    // reg[r][c]: row 32r + ty; c < NBM: column 32c + tx of M, c >= NBM: column 32(c-NBM) + tx of the identity
    float reg[NBM][2 * NBM];
#pragma unroll
    for (int r = 0; r < NBM; r++)
#pragma unroll
        for (int c = 0; c < NBM; c++) {
            const int i = 32 * r + ty, k = 32 * c + tx;
            reg[r][c] = (i < n && k < n) ? M[(long)max(i, k) * ldm + min(i, k)] : ((i == k) ? 1.f : 0.f);
            reg[r][NBM + c] = (i == k) ? 1.f : 0.f;
        }
    if (t < NR) { diag0[t] = t < n ? M[(long)t * ldm + t] : 1.f; deadf[t] = 0; dpiv[t] = 1.f; }
    // Fast path (second pass of CholQR2): M = I + E with |E|_F^2 <= 1e-6 -> M^-1/2 = I - E/2 
    {
        float e2 = 0.f;
#pragma unroll
        for (int r = 0; r < NBM; r++)
#pragma unroll
            for (int c = 0; c < NBM; c++) { const float e = reg[r][c] - ((32 * r + ty == 32 * c + tx) ? 1.f : 0.f); e2 += e * e; }
        e2 = wsum(e2);
        if ((t & 63) == 0) dinv[32 + (t >> 6)] = e2;
    }
    __syncthreads();
    {
        float tot = 0.f;
        for (int w = 0; w < C2_T / 64; w++) tot += dinv[32 + w];
        if (tot <= 1e-6f) {                                   // workgroup-uniform (false for NaN)
#pragma unroll
            for (int r = 0; r < NBM; r++)
#pragma unroll
                for (int c = 0; c < NBM; c++) {
                    const int i = 32 * r + ty, k = 32 * c + tx;
                    if (i < n && k < n) Linv[(long)i * ldl + k] = ((i == k) ? 1.5f : 0.f) - 0.5f * reg[r][c];
                }
            if (t < n) dead[t] = 0;
            return;
        }
    }

    // one block of 32 pivots; KB is a compile-time constant so that every index into reg[][] is static
    auto block = [&](auto KBc) {
        constexpr int kb = decltype(KBc)::value;
        if (kb < nb) {                                         // workgroup-uniform
            stamp();
            // ---- 1. the diagonal block of the current Schur complement -------------------------------
            Dblk[ty][tx] = reg[kb][kb];
            __syncthreads();
            stamp();
            // ---- 2a. one wave eliminates D in registers and leaves the multipliers in LDS -----------------------
            // Only the D half of [D | I] is a chain: the pivot of step j needs every step before it.  Lane i holds row i
            // of D (32 registers next to the wave's own matrix entries: nothing to park) and stores its multiplier of
            // step j - zero for i <= j or a dead pivot - over the block it has read: Dblk[j][i].
            if (t < 64) {
                const int i = t & 31;
                float a[32];
#pragma unroll
                for (int k = 0; k < 32; k++) a[k] = Dblk[i][k];
                const float d0_mine = diag0[32 * kb + i];
                float piv_mine = 0.f;
#pragma unroll
                for (int j = 0; j < 32; j++) {
                    const float piv = readlane_f(a[j], j);
                    const float d0 = readlane_f(d0_mine, j);
                    const bool dd = !(piv > rel_thresh * d0) || !(d0 > 0.f);
                    const float rinv = dd ? 0.f : __builtin_amdgcn_rcpf(piv);
                    if (i == j) piv_mine = a[j];
                    const float f = (i > j) ? a[j] * rinv : 0.f;
                    Dblk[j][i] = f;                                  // (both half-waves: the same value to the same word)
#pragma unroll
                    for (int k = j + 1; k < 32; k++) a[k] = __builtin_fmaf(-f, readlane_f(a[k], j), a[k]);
                }
                // what the block leaves for the phases behind it, once per lane instead of once per step: lane j
                // repeats the step's test and reciprocal on its own pivot (the same instructions on the same values)
                const bool dd = !(piv_mine > rel_thresh * d0_mine) || !(d0_mine > 0.f);
                const float rinv = dd ? 0.f : __builtin_amdgcn_rcpf(piv_mine);
                dpiv[32 * kb + i] = piv_mine; deadf[32 * kb + i] = dd ? 1 : 0; dinv[i] = rinv;
            }
            stamp();
            // ---- 3a. the block's rows (columns still needed) and the block's columns of the rows below ---
#pragma unroll
            for (int c = 0; c < NBM; c++) {
                if (c > kb && c < nb) Praw[32 * c + tx][ty] = reg[kb][c];              // M part right of the block
                if (c <= kb) Praw[32 * c + tx][ty] = reg[kb][NBM + c];                // identity part up to the block
            }
#pragma unroll
            for (int r = 0; r < NBM; r++)
                if (r > kb && r < nb) Acol[32 * r + ty][tx] = reg[r][kb];
            __syncthreads();
            stamp();
            // ---- 2b. the identity half, T = L1^-1, by columns on all waves ---------------------------------------
            // Column k of the identity half takes part in the steps j >= k only and in them needs nothing but the
            // multipliers: x_i -= f_ij * x_j, the same FMAs on the same entries as when the eliminating wave carried
            // them along.  Wave w takes columns w and 31 - w (33 readlane + FMA pairs) and lane i row i.
            {
                const int i = t & 31;
                const int k0 = __builtin_amdgcn_readfirstlane(t >> 6), k1 = 31 - k0;
                float f[32];
#pragma unroll
                for (int j = 0; j < 32; j++) f[j] = Dblk[j][i];
                float x0 = (i == k0) ? 1.f : 0.f, x1 = (i == k1) ? 1.f : 0.f;
#pragma unroll
                for (int j = 0; j < 32; j++) {
                    if (j >= k0) x0 = __builtin_fmaf(-f[j], readlane_f(x0, j), x0);
                    if (j >= k1) x1 = __builtin_fmaf(-f[j], readlane_f(x1, j), x1);
                }
                if ((t & 32) == 0) { Tblk[i][k0] = x0; Tblk[i][k1] = x1; }
            }
            __syncthreads();
            stamp();
            // ---- 3b. P = T * rows (this thread's row of the block), F = (A[:,K] T^T) / d --------------------
            // Every accumulator takes its 32 terms in ascending j, one FMA each (spelled out: left to contraction, the
            // products of a four-wide read come out as packed multiplies and separate adds); four j per LDS read.  The
            // loops carry no test of nb: a column or row block beyond it accumulates stale LDS into a value nobody stores.
            {
                constexpr int QUADS_3B = NBM <= 3 ? 4 : 2;        // quads of j in flight (registers: 4 (NBM + 1) each)
                float pacc[NBM];                                  // slot c: M part for c > kb, identity part for c <= kb
#pragma unroll
                for (int c = 0; c < NBM; c++) pacc[c] = 0.f;
#pragma unroll QUADS_3B
                for (int j = 0; j < 32; j += 4) {
                    const f32x4 tj = *reinterpret_cast<const f32x4 *>(&Tblk[ty][j]);   // zero for j > ty
#pragma unroll
                    for (int c = 0; c < NBM; c++) {
                        const f32x4 pj = *reinterpret_cast<const f32x4 *>(&Praw[32 * c + tx][j]);
#pragma unroll
                        for (int e = 0; e < 4; e++) pacc[c] = __builtin_fmaf(tj[e], pj[e], pacc[c]);
                    }
                }
#pragma unroll
                for (int c = 0; c < NBM; c++) {
                    if (c > kb && c < nb) { reg[kb][c] = pacc[c]; Pbuf[32 * c + tx][ty] = pacc[c]; }
                    if (c <= kb) { reg[kb][NBM + c] = pacc[c]; Pbuf[32 * c + tx][ty] = pacc[c]; }
                }
                const float di = dinv[tx];
                float facc[NBM];
#pragma unroll
                for (int r = 0; r < NBM; r++) facc[r] = 0.f;
#pragma unroll QUADS_3B
                for (int l = 0; l < 32; l += 4) {
                    const f32x4 tl = *reinterpret_cast<const f32x4 *>(&Tblk[tx][l]);
#pragma unroll
                    for (int r = 0; r < NBM; r++) {
                        if (r > kb) {
                            const f32x4 al = *reinterpret_cast<const f32x4 *>(&Acol[32 * r + ty][l]);
#pragma unroll
                            for (int e = 0; e < 4; e++) facc[r] = __builtin_fmaf(tl[e], al[e], facc[r]);
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < NBM; r++)
                    if (r > kb && r < nb) Fbuf[32 * r + ty][tx] = facc[r] * di;
            }
            __syncthreads();
            stamp();
            // ---- 4. trailing update of the rows below the block: rank-32 product F * P ---------------------
            if (kb + 1 < nb) {
                const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
                constexpr int QUADS_IN_FLIGHT = NBM <= 3 ? 4 : NBM == 4 ? 2 : 1;          // registers: 4 (2 NBM - kb - 1) per quad of j
#pragma unroll QUADS_IN_FLIGHT
                for (int j = 0; j < 32; j += 4) {
                    f32x4 fr[NBM], pc[NBM];                                          // pc[c]: the slot of column block c
#pragma unroll
                    for (int r = 0; r < NBM; r++) {
                        if (r > kb) { const f32x4 v = *reinterpret_cast<const f32x4 *>(&Fbuf[32 * r + ty][j]); fr[r] = r < nb ? v : zero4; }
                    }
#pragma unroll
                    for (int c = 0; c < NBM; c++) { const f32x4 v = *reinterpret_cast<const f32x4 *>(&Pbuf[32 * c + tx][j]); pc[c] = c < nb ? v : zero4; }
#pragma unroll
                    for (int e = 0; e < 4; e++) {
#pragma unroll
                        for (int r = 0; r < NBM; r++) {
                            if (r > kb) {
#pragma unroll
                                for (int c = 0; c < NBM; c++) {
                                    if (c > kb) reg[r][c] = __builtin_fmaf(-fr[r][e], pc[c][e], reg[r][c]);
                                    if (c <= kb) reg[r][NBM + c] = __builtin_fmaf(-fr[r][e], pc[c][e], reg[r][NBM + c]);
                                }
                            }
                        }
                    }
                }
            }
        }
    };
    block(std::integral_constant<int, 0>{});
    block(std::integral_constant<int, 1>{});
    block(std::integral_constant<int, 2>{});
    if constexpr (NBM > 3) block(std::integral_constant<int, 3>{});
    if constexpr (NBM > 4) block(std::integral_constant<int, NBM - 1>{});
    stamp();
    __syncthreads();
    // Linv = D^-1/2 U^-1 (lower triangular); dead rows and the padding are zero
#pragma unroll
    for (int r = 0; r < NBM; r++) {
        const int i = 32 * r + ty;
        if (i < n) {
            const float sc = deadf[i] ? 0.f : rsqrtf(dpiv[i]);
#pragma unroll
            for (int c = 0; c < NBM; c++) {
                const int k = 32 * c + tx;
                if (k < n) Linv[(long)i * ldl + k] = (k <= i) ? reg[r][NBM + c] * sc : 0.f;
            }
        }
    }
    if (t < n) dead[t] = deadf[t];
    stamp();
    if constexpr (TR) { if (t == 0) { trace[0] = tri - 1; trace[C2_STAMPS - 1] = __builtin_amdgcn_s_memrealtime(); } }
}

}  // namespace

template <int NBM, bool TR>
static void launch_chol_inv2(const float *M, long ldm, int n, float rel_thresh, float *Linv, long ldl, int *dead, unsigned long long *trace,
                             hipStream_t s)
{
    ensure_dynamic_lds(reinterpret_cast<const void *>(chol_inv2_kernel<NBM, TR>), (int)(c2_lds_floats(NBM) * sizeof(float)));
    hipLaunchKernelGGL((chol_inv2_kernel<NBM, TR>), dim3(1), dim3(C2_T), c2_lds_floats(NBM) * sizeof(float), s, M, ldm, n, rel_thresh, Linv,
                       ldl, dead, trace);
}

template <bool TR>
static void chol_inverse_dispatch(const float *M, long ldm, int n, float rel_thresh, float *Linv, long ldl, int *dead,
                                  unsigned long long *trace, hipStream_t s)
{
    DLCO_CHECK(n >= 1 && n <= CHOL_INV_MAX_N, -2, "chol_inverse128: n out of range");
    if (n <= 96) launch_chol_inv2<3, TR>(M, ldm, n, rel_thresh, Linv, ldl, dead, trace, s);      // (the steady-state block: 18 matrix registers per thread instead of 32: 44.2 -> 39.7 us at n = 96)
    else if (n <= 128) launch_chol_inv2<4, TR>(M, ldm, n, rel_thresh, Linv, ldl, dead, trace, s);
    else launch_chol_inv2<5, TR>(M, ldm, n, rel_thresh, Linv, ldl, dead, trace, s);
    DLCO_HIP(hipGetLastError());
}

void chol_inverse128(const float *M, long ldm, int n, float rel_thresh, float *Linv, long ldl, int *dead, hipStream_t s)
{
    chol_inverse_dispatch<false>(M, ldm, n, rel_thresh, Linv, ldl, dead, nullptr, s);
}

void chol_inverse128_stamped(const float *M, long ldm, int n, float rel_thresh, float *Linv, long ldl, int *dead, unsigned long long *trace,
                             hipStream_t s)
{
    chol_inverse_dispatch<true>(M, ldm, n, rel_thresh, Linv, ldl, dead, trace, s);
}

// residual_kernel and the read-back in one launch: the workgroup that finishes LAST (a ticket counter, left at zero
// again) copies the n floats of the block into pinned host memory - the block holds the residuals the other workgroups
// have just written, hence the agent-scope release / acquire pair around the ticket and the agent-scope loads - and
// then raises a sequence number there (system-scope release): the host polls the number instead of paying a stream
// synchronisation for a read-back of a few hundred bytes.  extra_dev: one more word the caller wants back.
// em.W != nullptr: the workgroup of row i also writes that row of W - W[nw-1-i] = sqrt(cscale (theta_i - mu)) * x_i for the nw rows
// with theta > mu (ascending order and scaling of src/pj-learn.cpp:480-487; the arithmetic of emit_w_kernel, bit for bit), the
// rows behind them unscaled in place when em.guards - and the scale into em.wscale: the row is in flight anyway, and the pass that
// turns out to be the last one of an update has then emitted W without a launch of its own (an earlier pass's rows are simply
// written over).
__global__ __launch_bounds__(256) void residual_publish_kernel(const float *X, const float *Y, long ld, const float *theta, int m, int F,
                                                               float *res, unsigned *ticket, const float *src, float *dst_host, int n,
                                                               unsigned *flag_host, unsigned seq, const int *extra_dev, int *extra_host,
                                                               ResidualEmit em)
{
    __shared__ float part[4];
    __shared__ int last;
    __shared__ int cnt[4];
    const int i = blockIdx.x;
    const float th = theta[i];
    float s = 0.f;
    if (em.W && (F & 3) == 0 && (ld & 3) == 0 && (em.ldw & 3) == 0) {
        int c = 0;
        for (int k = threadIdx.x; k < m; k += blockDim.x) c += theta[k] > em.mu ? 1 : 0;
        c = (int)wsum((float)c);                                  // m <= 4096: exact in fp32
        if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = c;
        __syncthreads();
        const int nw = cnt[0] + cnt[1] + cnt[2] + cnt[3];
        const bool mine = i < nw || em.guards;
        const float sc = i < nw ? sqrtf(em.cscale * (th - em.mu)) : 1.0f;
        f32x4 *w4 = reinterpret_cast<f32x4 *>(em.W + (long)(i < nw ? nw - 1 - i : i) * em.ldw);
        if (em.wscale && threadIdx.x == 0) em.wscale[i] = sc;
        const f32x4 *y4 = reinterpret_cast<const f32x4 *>(Y + (long)i * ld), *x4 = reinterpret_cast<const f32x4 *>(X + (long)i * ld);
        for (int f = threadIdx.x; f < F / 4; f += blockDim.x) {
            const f32x4 x = x4[f];
            const f32x4 d = y4[f] - th * x;
            s += d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
            if (mine) { f32x4 v = x; v[0] *= sc; v[1] *= sc; v[2] *= sc; v[3] *= sc; w4[f] = v; }
        }
    } else if ((F & 3) == 0 && (ld & 3) == 0) {
        const f32x4 *y4 = reinterpret_cast<const f32x4 *>(Y + (long)i * ld), *x4 = reinterpret_cast<const f32x4 *>(X + (long)i * ld);
        for (int f = threadIdx.x; f < F / 4; f += blockDim.x) {
            const f32x4 d = y4[f] - th * x4[f];
            s += d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3];
        }
    } else {
        for (int f = threadIdx.x; f < F; f += blockDim.x) {
            const float d = Y[(long)i * ld + f] - th * X[(long)i * ld + f];
            s += d * d;
        }
    }
    s = wsum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_store(res + i, sqrtf(part[0] + part[1] + part[2] + part[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = t == gridDim.x - 1 ? 1 : 0;
        if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    for (int k = threadIdx.x; k < n; k += 256) dst_host[k] = __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (extra_dev && threadIdx.x == 0) *extra_host = __hip_atomic_load(extra_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag_host, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

bool residual_norms_publish(const ResidualPublish &a, hipStream_t s)
{
    DLCO_CHECK(a.m > 0, -2, "residual_norms_publish: empty block");
    ResidualEmit em;
    if (a.emit.W && (a.F & 3) == 0 && (a.ld & 3) == 0 && (a.emit.ldw & 3) == 0 && (reinterpret_cast<uintptr_t>(a.emit.W) & 15) == 0) em = a.emit;
    hipLaunchKernelGGL(residual_publish_kernel, dim3(a.m), dim3(256), 0, s, a.X, a.Y, a.ld, a.theta, a.m, a.F, a.res, a.ticket, a.src,
                       a.dst_host, a.n, a.flag_host, a.seq, a.extra_dev, a.extra_host, em);
    DLCO_HIP(hipGetLastError());
    return em.W != nullptr;
}

void residual_norms(const float *X, const float *Y, long ld, const float *theta, int m, int F, float *res,
                    hipStream_t s)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(residual_kernel, dim3(m), dim3(256), 0, s, X, Y, ld, theta, m, F, res);
    DLCO_HIP(hipGetLastError());
}

void row_normalize(float *X, long ld, int m, int F, float min_norm, hipStream_t s)
{
    if (m <= 0) return;
    hipLaunchKernelGGL(row_normalize_kernel, dim3(m), dim3(256), 0, s, X, ld, m, F, min_norm);
    DLCO_HIP(hipGetLastError());
}

void symv(const float *H, long ld, int F, const float *x, float *y, hipStream_t s)
{
    hipLaunchKernelGGL(symv_kernel, dim3((F + 3) / 4), dim3(256), 0, s, H, ld, F, x, y);
    DLCO_HIP(hipGetLastError());
}

}  // namespace dlco
