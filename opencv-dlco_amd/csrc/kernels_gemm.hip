// kernels_gemm.hip — generic fp32 GEMM on v_mfma_f32_32x32x2_f32 (gfx950).
//
// One templated kernel serves every GEMM-shaped piece of the pj-learn path that is
// not the fused SYRK (kernels_syrk.hip): projection W*X^T, subspace products Q*H,
// Gram / Rayleigh matrices, basis rotations.  64-wide wavefronts, four waves per
// workgroup in a 2x2 arrangement, each wave owning WM x WN tiles of 32x32, LDS tiles
// stored k-major so that both MFMA operand fragments are conflict-free ds_read_b32
// (lane l reads element (l&31) of row k = 2*kk + (l>>5)).  Exact fp32: the MFMA is a
// k-ordered fmaf chain (MI355X guide, "FP32-input MFMA").
#include "dlco_internal.hpp"

namespace dlco {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int BK = 16;
constexpr int PAD = 4;
constexpr int NT = 256;
// K tiles in flight in the 64-wide instantiations (gemm_kernel's DEPTH); 128 x 128 tiles keep one.  Chosen by
// measurement among 2, 4 and 8; a build with -DDLCO_GEMM_DEPTH=n repeats the measurement.
#ifndef DLCO_GEMM_DEPTH
#define DLCO_GEMM_DEPTH 4
#endif
constexpr int RING_DEPTH = DLCO_GEMM_DEPTH;
static_assert(RING_DEPTH == 2 || RING_DEPTH == 4 || RING_DEPTH == 8, "ring depth: 2, 4 or 8");

struct OperandDev {
    const float *p;
    long ld;
    const int32_t *row_ids;
    const float *row_scale;
    int vec_ok;
    const int32_t *row_ids2;      // pair mode: operand row = p[row_ids[x]] - p[row_ids2[x]]
};

// up to 4 consecutive floats starting at src, elements at or beyond `limit - pos` are zero
__device__ __forceinline__ f32x4 load4(const float *src, int pos, int limit, int vec_ok)
{
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec_ok && pos + 3 < limit) {
        v = *reinterpret_cast<const f32x4 *>(src);
    } else {
        v[0] = src[0];
        if (pos + 1 < limit) v[1] = src[1];
        if (pos + 2 < limit) v[2] = src[2];
        if (pos + 3 < limit) v[3] = src[3];
    }
    return v;
}

struct GemmDev {
    int M, N, K;
    OperandDev A, B;
    float *C;
    long ldc;
    float alpha, beta, b1, b2;
    const float *E1, *E2;
    const int *k_dev;
    int k_chunk;      // K range per blockIdx.z
    float *slab;      // != nullptr: write raw partials to slab[z][M][N]
    int upper_only;
    const float *B2;  // != nullptr: a second product with the same A in the same launch, blockIdx.z == 1: C2 = A * B2 (no K split)
    float *C2;
};

// Stage one BK x BT tile of an operand into LDS (k-major image [BK][BT+PAD]).
// KM = memory rows run along K (contiguous along the M/N index), else along M/N.
// A tile at or beyond kend is all zeros and touches no memory.
template <int BT, bool KM>
__device__ __forceinline__ void load_tile(const OperandDev &op, int t0, int tmax, int k0, int kend,
                                          f32x4 (&regs)[BT / 64])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int u = 0; u < BT / 64; u++) {
        const int f = tid + NT * u;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (KM) {
            const int row = f / (BT / 4), c4 = f % (BT / 4);
            const int k = k0 + row, col = t0 + c4 * 4;
            if (k < kend && col < tmax) {
                const long mr = op.row_ids ? (long)op.row_ids[k] : (long)k;
                v = load4(op.p + mr * op.ld + col, col, tmax, op.vec_ok);
                if (op.row_ids2) v -= load4(op.p + (long)op.row_ids2[k] * op.ld + col, col, tmax, op.vec_ok);
                if (op.row_scale) {
                    const float sc = op.row_scale[k];
                    v *= sc;
                }
            }
        } else {
            const int row = f / (BK / 4), kq = f % (BK / 4);
            const int t = t0 + row, k = k0 + kq * 4;
            if (t < tmax && k < kend) {
                const long mr = op.row_ids ? (long)op.row_ids[t] : (long)t;
                v = load4(op.p + mr * op.ld + k, k, kend, op.vec_ok);
                if (op.row_ids2) v -= load4(op.p + (long)op.row_ids2[t] * op.ld + k, k, kend, op.vec_ok);
            }
        }
        regs[u] = v;
    }
}

// ---- plain operands: the loader of the deeper schedules ---------------------------------------------------------
// A load that sits behind a branch, be it a lane's bounds test, cannot be counted by hipcc among the requests in flight:
// the wait for an older tile then becomes a wait for all of them, and every test of load_tile is such a branch.  An
// operand is plain (gemm_f32: plain_operand) when one unconditional 16-byte load per piece, at a clamped address inside
// the operand, and a select afterwards give load_tile's values: 16-byte rows, nothing subtracted or scaled, no row ids
// along K, and the contiguous extent (M or N of a k-major operand, else K) a multiple of 4.

// The part of a row-major operand's addressing that no K tile changes: the memory row of each tile row a thread stages
// (rows beyond tmax: the last one, never used).  A gathered row id fetched inside the K loop would be the youngest
// request in flight; waiting for it drains every tile behind it.
template <int BT>
struct TileRows {
    const float *r[BT / 64];
};

template <int BT, bool KM>
__device__ __forceinline__ void tile_rows(const OperandDev &op, int t0, int tmax, TileRows<BT> &rows)
{
#pragma unroll
    for (int u = 0; u < BT / 64; u++) {
        rows.r[u] = op.p;
        if (KM) continue;
        const int t = min(t0 + (int)(threadIdx.x + NT * u) / (BK / 4), tmax - 1);
        rows.r[u] = op.p + (op.row_ids ? (long)op.row_ids[t] : (long)t) * op.ld;
    }
}

// A plain operand's tile in two steps that together give load_tile's values.  fetch_plain: the loads alone, unconditional,
// at addresses clamped into the operand (K = its whole K extent, a multiple of 4 when !KM).  zero_beyond: the zero fill
// beyond M / N and kend, applied when the tile is copied to LDS, DEPTH - 1 iterations later: next to the load hipcc
// turns the select back into a branch around it.
template <int BT, bool KM>
__device__ __forceinline__ void fetch_plain(const OperandDev &op, const TileRows<BT> &rows, int t0, int tmax, int k0, int kend, int K,
                                            f32x4 (&regs)[BT / 64])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int u = 0; u < BT / 64; u++) {
        const int f = tid + NT * u;
        if (KM) {
            const int row = f / (BT / 4), c4 = f % (BT / 4);
            regs[u] = *reinterpret_cast<const f32x4 *>(op.p + (long)min(k0 + row, kend - 1) * op.ld + min(t0 + c4 * 4, tmax - 4));
        } else {
            const int kq = f % (BK / 4);
            regs[u] = *reinterpret_cast<const f32x4 *>(rows.r[u] + min(k0 + kq * 4, K - 4));
        }
    }
}

template <int BT, bool KM>
__device__ __forceinline__ void zero_beyond(int t0, int tmax, int k0, int kend, f32x4 (&regs)[BT / 64])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int u = 0; u < BT / 64; u++) {
        const int f = tid + NT * u;
        int live;                                                 // elements of the piece that are the operand's
        if (KM) {
            const int row = f / (BT / 4), c4 = f % (BT / 4);
            live = (k0 + row < kend && t0 + c4 * 4 < tmax) ? 4 : 0;
        } else {
            const int row = f / (BK / 4), kq = f % (BK / 4);
            live = t0 + row < tmax ? kend - (k0 + kq * 4) : 0;
        }
        regs[u][0] = live > 0 ? regs[u][0] : 0.f;
        regs[u][1] = live > 1 ? regs[u][1] : 0.f;
        regs[u][2] = live > 2 ? regs[u][2] : 0.f;
        regs[u][3] = live > 3 ? regs[u][3] : 0.f;
    }
}

// Copy a fetched tile into its LDS image (k-major [BK][BT+PAD]).
template <int BT, bool KM>
__device__ __forceinline__ void store_tile(float (*lds)[BT + PAD], const f32x4 (&regs)[BT / 64])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int u = 0; u < BT / 64; u++) {
        const int f = tid + NT * u;
        if (KM) {
            const int row = f / (BT / 4), c4 = f % (BT / 4);
            *reinterpret_cast<f32x4 *>(&lds[row][c4 * 4]) = regs[u];
        } else {
            const int row = f / (BK / 4), kq = f % (BK / 4);
            lds[kq * 4 + 0][row] = regs[u][0];
            lds[kq * 4 + 1][row] = regs[u][1];
            lds[kq * 4 + 2][row] = regs[u][2];
            lds[kq * 4 + 3][row] = regs[u][3];
        }
    }
}

// DEPTH = K tiles whose global loads are in flight.  Tile p is multiplied from LDS image p & 1 during iteration p,
// copied there from register set p % DEPTH at the end of iteration p - 1 and requested into that set at the top of
// iteration p - DEPTH (tiles 0 .. DEPTH-1: before the loop), so the copy waits for a request DEPTH - 1 tiles old
// (s_waitcnt vmcnt(n), n > 0) instead of for the youngest one.  DEPTH 1 is the single-tile schedule on load_tile: one
// exposed global-load latency per K tile, which is all a 64-wide launch of 6 - 15 tiles consists of.  DEPTH > 1 needs
// plain operands (fetch_plain).  The loop is unrolled by DEPTH so that every register set has a static name (one
// chosen at run time would live in scratch memory), and a trip has no branch: a request beyond the last tile yields
// zeros, which go to the image nobody reads any more.  The arithmetic does not depend on DEPTH: every accumulator is
// the same k-ordered chain over the same LDS images.
template <int WM, int WN, bool A_KM, bool B_KM, int DEPTH>
__global__ __launch_bounds__(NT) void gemm_kernel(GemmDev g)
{
    constexpr int BM = 64 * WM, BN = 64 * WN;
    __shared__ __attribute__((aligned(16))) float As[2][BK][BM + PAD];
    __shared__ __attribute__((aligned(16))) float Bs[2][BK][BN + PAD];

    const int bi = blockIdx.y, bj = blockIdx.x;
    if (g.upper_only && bj * BN + BN <= bi * BM) return;     // tile entirely below the diagonal
    const int i0 = bi * BM, j0 = bj * BN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    int kz = blockIdx.z;
    if (g.B2) {
        if (kz == 1) { g.B.p = g.B2; g.C = g.C2; }
        kz = 0;
    }
    const int kbeg = kz * g.k_chunk;
    int kend = min(g.K, kbeg + g.k_chunk);
    if (g.k_dev) kend = min(kend, *g.k_dev);

    f32x16 acc[WM][WN];
#pragma unroll
    for (int a = 0; a < WM; a++)
#pragma unroll
        for (int b = 0; b < WN; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;

    const int nk = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0;
    if (nk > 0) {                                            // (the same for the whole workgroup)
    TileRows<BM> rows_a;
    TileRows<BN> rows_b;
    if (DEPTH > 1) {
        tile_rows<BM, A_KM>(g.A, i0, g.M, rows_a);
        tile_rows<BN, B_KM>(g.B, j0, g.N, rows_b);
    }
    struct Slot { f32x4 a[BM / 64], b[BN / 64]; };
    Slot ring[DEPTH];
    // one fixed order of a set's loads, before the loop and inside it
    auto request = [&](int p, Slot &s) {
        if (DEPTH > 1) {
            fetch_plain<BM, A_KM>(g.A, rows_a, i0, g.M, kbeg + p * BK, kend, g.K, s.a);
            fetch_plain<BN, B_KM>(g.B, rows_b, j0, g.N, kbeg + p * BK, kend, g.K, s.b);
        } else {
            load_tile<BM, A_KM>(g.A, i0, g.M, kbeg + p * BK, kend, s.a);
            load_tile<BN, B_KM>(g.B, j0, g.N, kbeg + p * BK, kend, s.b);
        }
    };
    auto commit = [&](int buf, int p, const Slot &s) {       // s holds tile p
        Slot t = s;
        if (DEPTH > 1) {
            zero_beyond<BM, A_KM>(i0, g.M, kbeg + p * BK, kend, t.a);
            zero_beyond<BN, B_KM>(j0, g.N, kbeg + p * BK, kend, t.b);
        }
        store_tile<BM, A_KM>(As[buf], t.a);
        store_tile<BN, B_KM>(Bs[buf], t.b);
    };
    const int lr = lane & 31, lk = lane >> 5;
    auto multiply = [&](int buf) {
#pragma unroll
        for (int kk = 0; kk < BK / 2; kk++) {
            float af[WM], bf[WN];
#pragma unroll
            for (int a = 0; a < WM; a++) af[a] = As[buf][2 * kk + lk][wm * 32 * WM + a * 32 + lr];
#pragma unroll
            for (int b = 0; b < WN; b++) bf[b] = Bs[buf][2 * kk + lk][wn * 32 * WN + b * 32 + lr];
#pragma unroll
            for (int a = 0; a < WM; a++)
#pragma unroll
                for (int b = 0; b < WN; b++)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a], bf[b], acc[a][b], 0, 0, 0);
        }
    };

#pragma unroll
    for (int d = 0; d < DEPTH; d++) request(d, ring[d]);
    commit(0, 0, ring[0]);
    __syncthreads();
    int kt = 0;
    for (; kt + DEPTH <= nk; kt += DEPTH) {
#pragma unroll
        for (int d = 0; d < DEPTH; d++) {
            request(kt + d + DEPTH, ring[d]);
            multiply((kt + d) & 1);
            commit(((kt + d) & 1) ^ 1, kt + d + 1, ring[(d + 1) % DEPTH]);
            __syncthreads();
        }
    }
    // the last nk % DEPTH tiles: everything they need was requested above
#pragma unroll
    for (int d = 0; d + 1 < DEPTH; d++) {
        if (kt + d < nk) {
            multiply((kt + d) & 1);
            commit(((kt + d) & 1) ^ 1, kt + d + 1, ring[d + 1]);
            __syncthreads();
        }
    }
    }

    // epilogue: C/D layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
    const int lc = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int a = 0; a < WM; a++)
#pragma unroll
        for (int b = 0; b < WN; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int i = i0 + wm * 32 * WM + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int j = j0 + wn * 32 * WN + b * 32 + lc;
                if (i >= g.M || j >= g.N) continue;
                if (g.slab) {
                    g.slab[((long)blockIdx.z * g.M + i) * g.N + j] = acc[a][b][r];
                    continue;
                }
                if (g.upper_only && j < i) continue;
                const long idx = (long)i * g.ldc + j;
                float o = g.alpha * acc[a][b][r];
                if (g.beta != 0.f) o += g.beta * g.C[idx];
                if (g.E1) o += g.b1 * g.E1[idx];
                if (g.E2) o += g.b2 * g.E2[idx];
                g.C[idx] = o;
                if (g.upper_only && j > i) g.C[(long)j * g.ldc + i] = o;
            }
}

__global__ void splitk_reduce_kernel(const float *slab, int split, int M, int N, float *C, long ldc, float alpha,
                                     float beta, const float *E1, float b1, const float *E2, float b2)
{
    // 16 lanes (one DPP row) per output element: lane z adds slices z, z+16, ... in order, the 16
    // partial sums are combined by a fixed butterfly, so the result does not depend on timing.
    const long total = (long)M * N;
    const int zl = threadIdx.x & 15;
    for (long e = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 4; e < total; e += ((long)gridDim.x * blockDim.x) >> 4) {
        const int i = (int)(e / N), j = (int)(e % N);
        float s = 0.f;
        for (int z = zl; z < split; z += 16) s += slab[(long)z * total + e];
        s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0xB1, 0xF, 0xF, true));
        s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x4E, 0xF, 0xF, true));
        s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x141, 0xF, 0xF, true));
        s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x140, 0xF, 0xF, true));
        if (zl != 0) continue;
        const long idx = (long)i * ldc + j;
        float o = alpha * s;
        if (beta != 0.f) o += beta * C[idx];
        if (E1) o += b1 * E1[idx];
        if (E2) o += b2 * E2[idx];
        C[idx] = o;
    }
}

// Few slices over a large output (the tracker's split-bf16 products: 4-32 slices of m x F): one
// thread per four consecutive outputs, slices added in order, 16-byte accesses throughout.
__global__ __launch_bounds__(256) void splitk_reduce_wide_kernel(const float *slab, int split, int M, int N, float *C,
                                                                 long ldc, float alpha, float beta, const float *E1,
                                                                 float b1, const float *E2, float b2)
{
    const long total = (long)M * N, q = N >> 2;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < (long)M * q; e += (long)gridDim.x * blockDim.x) {
        const int i = (int)(e / q), j = (int)(e % q) * 4;
        const float *p = slab + (long)i * N + j;
        f32x4 s = *reinterpret_cast<const f32x4 *>(p);
        for (int z = 1; z < split; z++) s += *reinterpret_cast<const f32x4 *>(p + (long)z * total);
        const long idx = (long)i * ldc + j;
        f32x4 o = alpha * s;
        if (beta != 0.f) o += beta * *reinterpret_cast<const f32x4 *>(C + idx);
        if (E1) o += b1 * *reinterpret_cast<const f32x4 *>(E1 + idx);
        if (E2) o += b2 * *reinterpret_cast<const f32x4 *>(E2 + idx);
        *reinterpret_cast<f32x4 *>(C + idx) = o;
    }
}

template <int WM, int WN, int DEPTH>
void launch(const GemmDev &g, bool akm, bool bkm, dim3 grid, hipStream_t s)
{
    if (akm && bkm) hipLaunchKernelGGL((gemm_kernel<WM, WN, true, true, DEPTH>), grid, dim3(NT), 0, s, g);
    else if (akm && !bkm) hipLaunchKernelGGL((gemm_kernel<WM, WN, true, false, DEPTH>), grid, dim3(NT), 0, s, g);
    else if (!akm && bkm) hipLaunchKernelGGL((gemm_kernel<WM, WN, false, true, DEPTH>), grid, dim3(NT), 0, s, g);
    else hipLaunchKernelGGL((gemm_kernel<WM, WN, false, false, DEPTH>), grid, dim3(NT), 0, s, g);
}

// a 64-wide instantiation: RING_DEPTH tiles in flight, or one
template <int WM, int WN>
void launch_small(const GemmDev &g, bool akm, bool bkm, dim3 grid, bool ring, hipStream_t s)
{
    if (ring) launch<WM, WN, RING_DEPTH>(g, akm, bkm, grid, s);
    else launch<WM, WN, 1>(g, akm, bkm, grid, s);
}

inline int vec_ok(const GemmOperand &o) { return (o.ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(o.p) & 15) == 0); }

// fetch_plain's conditions; t = the operand's M or N extent
inline bool plain_operand(const GemmOperand &o, int t, int K)
{
    if (!vec_ok(o) || o.row_ids2 || (o.kmajor && (o.row_scale || o.row_ids))) return false;
    return (o.kmajor ? t : K) % 4 == 0;
}

}  // namespace

size_t gemm_slab_floats(int M, int N, int split_k) { return split_k > 1 ? (size_t)split_k * M * N : 0; }

bool splitk_reduce_is_wide(const float *slab, int split, int M, int N, const float *C, long ldc, const float *E1, const float *E2)
{
    auto al16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    return split <= 32 && (long)M * N >= 65536 && N % 4 == 0 && ldc % 4 == 0 && al16(slab) && al16(C) && (!E1 || al16(E1)) &&
           (!E2 || al16(E2));
}

// C = alpha * sum_z slab[z] + beta*C + b1*E1 + b2*E2 over `split` [M][N] partial slabs (fixed order)
void splitk_reduce_f32(const float *slab, int split, int M, int N, float *C, long ldc, float alpha, float beta,
                       const float *E1, float b1, const float *E2, float b2, hipStream_t s)
{
    const long total = (long)M * N;
    if (splitk_reduce_is_wide(slab, split, M, N, C, ldc, E1, E2)) {
        long blocks = (total / 4 + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(splitk_reduce_wide_kernel, dim3((unsigned)blocks), dim3(256), 0, s, slab, split, M, N, C, ldc, alpha,
                           beta, E1, b1, E2, b2);
        DLCO_HIP(hipGetLastError());
        return;
    }
    long blocks = (total * 16 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, slab, split, M, N, C, ldc, alpha, beta,
                       E1, b1, E2, b2);
    DLCO_HIP(hipGetLastError());
}

int gemm_ring_depth() { return RING_DEPTH; }

void gemm_f32(const GemmArgs &a, hipStream_t s)
{
    if (a.M <= 0 || a.N <= 0) return;
    DLCO_CHECK(a.depth == 0 || a.depth == 1, -2, "gemm_f32: depth is 0 (the library's choice) or 1");
    DLCO_CHECK(a.A.p && a.B.p && a.C, -2, "gemm_f32: null operand");
    DLCO_CHECK(!(a.upper_only && (a.M != a.N || a.split_k > 1)), -2, "gemm_f32: upper_only needs M==N, split_k==1");
    GemmDev g;
    g.M = a.M; g.N = a.N; g.K = a.K;
    g.A = {a.A.p, a.A.ld, a.A.row_ids, a.A.kmajor ? a.A.row_scale : nullptr, vec_ok(a.A), a.A.row_ids2};
    g.B = {a.B.p, a.B.ld, a.B.row_ids, a.B.kmajor ? a.B.row_scale : nullptr, vec_ok(a.B), a.B.row_ids2};
    g.C = a.C; g.ldc = a.ldc;
    g.alpha = a.alpha; g.beta = a.beta; g.E1 = a.E1; g.b1 = a.b1; g.E2 = a.E2; g.b2 = a.b2;
    g.k_dev = a.k_dev;
    g.upper_only = a.upper_only ? 1 : 0;
    int split = a.split_k < 1 ? 1 : a.split_k;
    int chunk = (a.K + split - 1) / split;
    chunk = ((chunk + BK - 1) / BK) * BK;
    if (chunk < BK) chunk = BK;
    split = a.K > 0 ? (a.K + chunk - 1) / chunk : 1;
    g.k_chunk = chunk;
    g.slab = nullptr;
    if (split > 1) {
        DLCO_CHECK(a.slab != nullptr, -2, "gemm_f32: split_k > 1 needs a slab workspace");
        g.slab = a.slab;
    }
    g.B2 = a.B2; g.C2 = a.C2;
    if (a.B2) {
        DLCO_CHECK(a.C2 && split == 1 && !a.upper_only, -2, "gemm_f32: a twin product needs C2 and no K split");
        split = 2;                                                 // grid z = the two products
    }
    // tile choice: the small dimension decides; a launch that would leave most of the 256 CUs
    // without a workgroup takes 64-wide tiles instead (the tracker's m x F x m products)
    bool small_m = a.M <= 64 || a.small_m_tiles, small_n = a.N <= 64 || a.small_n_tiles;
    auto n_wg = [&](bool sm, bool sn) {
        return (long)((a.M + (sm ? 63 : 127)) / (sm ? 64 : 128)) * ((a.N + (sn ? 63 : 127)) / (sn ? 64 : 128)) * split;
    };
    if (!a.upper_only) {
        if (!small_m && n_wg(small_m, small_n) < 256) small_m = true;
        if (!small_n && n_wg(small_m, small_n) < 256) small_n = true;
    }
    // K tiles in flight (gemm_kernel): the ring for 64-wide tiles of plain operands, which is every small product of a
    // training step; one tile, the schedule and loader of before, for everything else and on request
    const bool ring = a.depth != 1 && plain_operand(a.A, a.M, a.K) && plain_operand(a.B, a.N, a.K);
    if (a.depth_used) *a.depth_used = ring && (small_m || small_n) ? RING_DEPTH : 1;
    if (small_m && small_n) {
        dim3 grid((a.N + 63) / 64, (a.M + 63) / 64, split);
        launch_small<1, 1>(g, a.A.kmajor, a.B.kmajor, grid, ring, s);
    } else if (small_m) {
        dim3 grid((a.N + 127) / 128, (a.M + 63) / 64, split);
        launch_small<1, 2>(g, a.A.kmajor, a.B.kmajor, grid, ring, s);
    } else if (small_n) {
        dim3 grid((a.N + 63) / 64, (a.M + 127) / 128, split);
        launch_small<2, 1>(g, a.A.kmajor, a.B.kmajor, grid, ring, s);
    } else {
        dim3 grid((a.N + 127) / 128, (a.M + 127) / 128, split);
        launch<2, 2, 1>(g, a.A.kmajor, a.B.kmajor, grid, s);              // 128 x 128 tiles: one tile in flight
    }
    DLCO_HIP(hipGetLastError());
    if (split > 1 && !a.B2)
        splitk_reduce_f32(a.slab, split, a.M, a.N, a.C, a.ldc, a.alpha, a.beta, a.E1, a.b1, a.E2, a.b2, s);
}

}  // namespace dlco
