// kernels_describe.hip — the learnt descriptor y = W * min(sPRFilters * get_desc(patch), 1) behind the
// pooling product of kernels_desc.hip, and the per-pair distance on such descriptors:
//
//   desc_project_kernel       Y[n][j] = sum_f Desc[n][f] * W[j][f] for a chunk of patches on the f64 matrix
//                             cores: the reference world forms this product with cv::gemm on floats, which
//                             accumulates in double, so the operands are widened when the fragments are read
//                             and the double accumulator is rounded to fp32 once, at the store
//   desc_pair_sqdist_kernel   dist[p] = sum_j (Y[a_p][j] - Y[b_p][j])^2 and Label = (id1 == id2), one wave per
//                             pair: the difference in fp32 (as desc_pair_diff_kernel forms it), squares and
//                             sum in double, rounded once
//
// Both operands of the projection are K-contiguous (Desc [n][F] as desc_pool_kernel stores it, W [r][F]
// row-major as pj-learn writes it).  F = nsel*8 is a multiple of 8, so a row is a whole number of 16-byte
// pieces whatever nsel is; the ragged edges (patches of a short chunk, r not a multiple of the column tile,
// F not a multiple of the staged k chunk) are zero-filled when a tile is staged and masked at the store.
#include "dlco_internal.hpp"

namespace dlco {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

// A workgroup owns 16 patches x 64 rows of W and runs the whole K = F in order: a patch's entry is two chains
// of MFMA accumulations whose order depends on F alone, never on the number of patches in the call, and no
// partial sums meet outside the workgroup.  16 rows is the M of v_mfma_f64_16x16x4: a chunk of 2048 patches
// gives 128 row tiles (x ceil(r/64) column tiles) instead of the 16 a 128-row tile would leave on 256 CUs.
// Eight waves, two per SIMD: wave (g, w) holds the 16 x 16 result of W rows 16w.. over the k of half g (64 wide) of
// every staged 128-wide chunk; the two halves meet once, at the end, through LDS and in the fixed order half 0 + half 1.
// (Four waves - one per SIMD, one dependent MFMA chain each - left the matrix pipe idle during every LDS read and
// barrier: 127 us per 2048-patch chunk at F = 8192, r = 128, where the MFMAs alone need 55.)
constexpr int PM = 16;                 // patches per workgroup
constexpr int PN = 64;                 // rows of W per workgroup (16 per wave)
constexpr int PH = 64;                 // k per wave and staged chunk
constexpr int PK = 2 * PH;             // k per staged chunk
constexpr int PP = PK + 4;             // LDS pitch in floats: 16-byte reads of 16 rows spread over all banks
constexpr int PD = 4;                  // staged chunks in flight per thread (even)
constexpr int PTH = 512;

__global__ __launch_bounds__(PTH) void desc_project_kernel(const float *desc, long desc_ld, int n, const float *W, int r, int F, float *Y,
                                                           long y_ld)
{
    __shared__ float As[2][PM * PP], Bs[2][PN * PP];
    __shared__ double red[4 * 64 * 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, half = tid >> 8;
    const long n0 = (long)blockIdx.x * PM;
    const int j0 = blockIdx.y * PN;
    // loader: thread t stages the 16-byte piece lseg of Desc row lrow and of W rows lrow + 16*u
    const int lrow = tid >> 5, lseg = tid & 31;
    // every load is unconditional and in bounds - a row or a k piece beyond the edge reads row 0 / the row's last piece
    // and is replaced by zeros afterwards - so that no branch sits between a load and its use: with loads under
    // branches the compiler waited for ALL outstanding loads (vmcnt(0)) before every LDS store
    const bool a_in = n0 + lrow < n;
    const float *Ag = desc + (a_in ? n0 + lrow : 0) * desc_ld;
    const float *Bg[4];
    bool b_in[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int j = j0 + lrow + 16 * u;
        b_in[u] = j < r;
        Bg[u] = W + (long)(b_in[u] ? j : 0) * F;
    }
    const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
    // PD chunks are in flight per thread: the slot of chunk c is c % PD
    f32x4 ra[PD], rb[PD][4];
    auto gload = [&](int kc, int slot) {
        const int k = kc * PK + 4 * lseg;                  // F % 4 == 0: a piece is inside the row or beyond it
        const bool k_in = k < F;
        const int kk = k_in ? k : F - 4;
        const f32x4 va = *reinterpret_cast<const f32x4 *>(Ag + kk);
        ra[slot] = (a_in && k_in) ? va : zero4;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const f32x4 vb = *reinterpret_cast<const f32x4 *>(Bg[u] + kk);
            rb[slot][u] = (b_in[u] && k_in) ? vb : zero4;
        }
    };
    auto lstore = [&](int buf, int slot) {
        *reinterpret_cast<f32x4 *>(&As[buf][lrow * PP + 4 * lseg]) = ra[slot];
#pragma unroll
        for (int u = 0; u < 4; u++) *reinterpret_cast<f32x4 *>(&Bs[buf][(lrow + 16 * u) * PP + 4 * lseg]) = rb[slot][u];
    };
    // fragment order of desc_pool_kernel: lane l supplies A[l%16][kq] and B[kq][l%16], kq = l/16; within a 16-wide k
    // chunk lane group g reads k = 4g..4g+3 as one 16-byte LDS read and MFMA step s uses element s of both
    const int li = lane & 15, lg = lane >> 4;
    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
    const int nch = (F + PK - 1) / PK;
    auto mfma_chunk = [&](int buf) {
#pragma unroll
        for (int c = 0; c < PH / 16; c++) {
            const f32x4 fa = *reinterpret_cast<const f32x4 *>(&As[buf][li * PP + PH * half + 16 * c + 4 * lg]);
            const f32x4 fb = *reinterpret_cast<const f32x4 *>(&Bs[buf][(16 * wave + li) * PP + PH * half + 16 * c + 4 * lg]);
#pragma unroll
            for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)fa[s], (double)fb[s], acc, 0, 0, 0);
        }
    };
#pragma unroll
    for (int d = 0; d < PD; d++) gload(d, d);              // a chunk beyond the end loads as zeros
    lstore(0, 0);
    __syncthreads();
    // whole groups of PD chunks: nothing here is conditional, so the compiler can count the loads in flight and wait
    // for the oldest chunk only; a load or an LDS store past the last chunk moves zeros that nothing reads
    const int nfull = nch / PD * PD;
    for (int kc0 = 0; kc0 < nfull; kc0 += PD) {
#pragma unroll
        for (int d = 0; d < PD; d++) {
            const int buf = d & 1;                         // PD is even: chunk kc0 + d sits in LDS buffer d & 1
            gload(kc0 + d + PD, d);                        // slot d went to LDS in the step before
            mfma_chunk(buf);
            lstore(buf ^ 1, (d + 1) % PD);
            __syncthreads();
        }
    }
    // the last nch % PD chunks are in their slots already (conditions uniform over the workgroup)
#pragma unroll
    for (int d = 0; d < PD - 1; d++) {
        if (nfull + d < nch) {
            mfma_chunk(d & 1);
            if (nfull + d + 1 < nch) lstore((d & 1) ^ 1, d + 1);
            __syncthreads();
        }
    }
    // half 1 hands its sums over; the last barrier of the k loop is behind every wave here
    if (half == 1) {
#pragma unroll
        for (int rr = 0; rr < 4; rr++) red[(wave * 4 + rr) * 64 + lane] = acc[rr];
    }
    __syncthreads();
    if (half == 1) return;
#pragma unroll
    for (int rr = 0; rr < 4; rr++) acc[rr] += red[(wave * 4 + rr) * 64 + lane];
    // the f64 16x16x4 result: column = lane & 15 (row of W), row = lane / 16 + 4 * register (patch)
    const int j = j0 + 16 * wave + li;
    if (j < r) {
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const long row = n0 + lg + 4 * rr;
            if (row < n) Y[row * y_ld + j] = (float)acc[rr];
        }
    }
}

constexpr int QTH = 256;               // four pairs per workgroup, one wave each

__global__ __launch_bounds__(QTH) void desc_pair_sqdist_kernel(const float *Y, long ld, int r, const int32_t *pairs, long n_pairs, float *dist,
                                                               uint8_t *label)
{
#pragma clang fp contract(off)
    const long pr = (long)blockIdx.x * (QTH / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pr >= n_pairs) return;
    const int32_t *q = pairs + pr * 4;
    const float *a = Y + (long)q[0] * ld, *b = Y + (long)q[2] * ld;
    double s = 0.0;
    for (int j = lane; j < r; j += 64) {
        const float d = a[j] - b[j];
        s += (double)d * (double)d;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
        dist[pr] = (float)s;
        if (label) label[pr] = (q[1] == q[3]) ? 1 : 0;
    }
}

}  // namespace

// desc: [n][desc_ld] with n*F floats readable, W: [r][F], Y: [n][y_ld]; columns [r, y_ld) of Y are not written
void desc_project(const float *desc, long desc_ld, int n, const float *W, int r, int F, float *Y, long y_ld, hipStream_t s)
{
    if (n <= 0 || r <= 0 || F <= 0) return;
    hipLaunchKernelGGL(desc_project_kernel, dim3((n + PM - 1) / PM, (r + PN - 1) / PN), dim3(PTH), 0, s, desc, desc_ld, n, W, r, F, Y, y_ld);
    DLCO_HIP(hipGetLastError());
}

void desc_pair_sqdist(const float *Y, long ld, int r, const int32_t *pairs, long n_pairs, float *dist, uint8_t *label, hipStream_t s)
{
    if (n_pairs <= 0) return;
    const long per = QTH / 64;
    hipLaunchKernelGGL(desc_pair_sqdist_kernel, dim3((unsigned)((n_pairs + per - 1) / per)), dim3(QTH), 0, s, Y, ld, r, pairs, n_pairs, dist,
                       label);
    DLCO_HIP(hipGetLastError());
}

}  // namespace dlco
