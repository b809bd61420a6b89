// kernels_bf16x2.hip — tracker filter product on the bf16 matrix cores with split operands.
//
//     out[M][F] = alpha * X[M][F] * G[F][F] + b1*E1 + b2*E2          (G symmetric, fp32 in HBM)
//
// The Chebyshev filter of the subspace tracker only has to ENRICH the block (the Rayleigh-Ritz
// step that follows uses the exact fp32 product and the convergence test is on fp32
// residuals), so its products may carry ~1e-5 relative error.  Each fp32 operand is split
// into two bf16 values, x = hi + lo (16 mantissa bits kept), and the product is formed as
// hi*hi + hi*lo + lo*hi with fp32 accumulation on v_mfma_f32_32x32x16_bf16: three bf16 MFMAs
// (3/16 of the fp32-MFMA time) in place of one fp32 pass, which moves the product from
// MFMA-bound to HBM-bound (one read of G).
//   * X is split once per product into fragment-ordered bf16 planes (split_x_kernel), so the
//     A fragments are whole 1-KiB coalesced loads;
//   * G is split on the fly in registers: a lane loads the 8 k-values of its column
//     (32 lanes = one 128-byte row segment per instruction) and packs hi / lo;
//   * one workgroup = 128 output columns x all rows x one K slice; its 8 waves are 4 column
//     tiles x 2 K halves, combined in order through LDS and a slab reduce (deterministic).
// NS = 3 splits every operand three ways, x = hi + mid + lo (24 mantissa bits, i.e. all of an
// fp32), and keeps the six product terms down to 2^-16 (hh, hm, mh, mm, hl, lh): the dropped
// terms are at the level of one fp32 rounding.  Six bf16 MFMAs still cost 3/8 of the fp32
// MFMA pass, so the Rayleigh-Ritz product of the tracker runs at fp32 accuracy from one
// HBM-bound read of G as well.
// The split, the plane layout, the MFMA term order and the LDS geometry of these kernels are in split_bf16_dev.hpp.
#include "dlco_internal.hpp"
#include "split_bf16_dev.hpp"

#include <algorithm>

namespace dlco {

namespace {

constexpr int W8 = 8;             // waves per workgroup
constexpr int T8 = 64 * W8;
constexpr int KS = 4;             // default K split (gridDim.y); the slices are summed in order by splitk_reduce_f32

// one thread per plane entry t = plane_entry(k16, MT, tile, lane)
__global__ __launch_bounds__(256) void split_x_kernel(const float *X, long ldx, int M, int MT, int K, bf16x8 *hi, bf16x8 *lo,
                                                      bf16x8 *lo2)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)(K / 16) * MT * 64;
    if (t >= total) return;
    const int lane = (int)(t & 63);
    const long q = t >> 6;
    const int tile = (int)(q % MT);
    const int k16 = (int)(q / MT);
    const int row = tile * 32 + (lane & 31), k = k16 * 16 + 8 * (lane >> 5);
    bf16x8 h, l, l2;
    if (row < M) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(X + (long)row * ldx + k);
        const f32x4 b = *reinterpret_cast<const f32x4 *>(X + (long)row * ldx + k + 4);
#pragma unroll
        for (int j = 0; j < 8; j++) split_f32<3>(j < 4 ? a[j & 3] : b[j & 3], j, h, l, l2);
    } else {
        h = l = l2 = bf16x8{};
    }
    hi[t] = h;
    lo[t] = l;
    if (lo2) lo2[t] = l2;
}

struct Bf2Dev {
    int M, N, K;
    const bf16x8 *xhi, *xlo, *xlo2;
    const float *G;
    long ldg;
    float *slab;                  // [KS][M][N] raw partial sums
};

template <int MT, int NS>
__global__ __launch_bounds__(T8) void skinny_bf16x2_kernel(Bf2Dev g)
{
    // Workgroup = 128 output columns x one K quarter (blockIdx.y); wave w owns column tile w&3 and
    // K half w>>2 of that quarter.  All four column tiles walk the same X fragments, so the X
    // planes are pulled through L2 once per 128 columns instead of once per 32 (the planes do not
    // stay L2-resident beside the streamed G, and the Infinity Cache rate was the bound).
    __shared__ float red[4 * MT * 16 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 31, lh = lane >> 5;
    const int ct = wave & 3, kh = wave >> 2;
    const int col = blockIdx.x * 128 + ct * 32 + lc;
    const int nsteps = g.K / 16;
    const int per = nsteps / ((int)gridDim.y * 2);        // host guarantees divisibility (and per % 4 == 0)
    const int s0 = (blockIdx.y * 2 + kh) * per, s1 = s0 + per;

    f32x16 acc[MT];
#pragma unroll
    for (int a = 0; a < MT; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[a][r] = 0.f;

    bf16x8 ah[MT], al[MT], ahn[MT], aln[MT];
    bf16x8 am[NS == 3 ? MT : 1], amn[NS == 3 ? MT : 1];        // third plane of X (NS = 3 only)
    // (Reading G[col][k] instead — a lane streaming its own row, legal because G is symmetric —
    // was measured 15 % slower: 32 distinct lines per wave instruction.)
    auto load_g = [&](int s, float (&gv)[8]) {
        const float *p = g.G + ((long)s * 16 + 8 * lh) * g.ldg + col;
#pragma unroll
        for (int j = 0; j < 8; j++) gv[j] = p[(long)j * g.ldg];
    };
    auto load_a = [&](int s, bf16x8 (&h)[MT], bf16x8 (&l)[MT], bf16x8 (&m2)[NS == 3 ? MT : 1]) {
#pragma unroll
        for (int t = 0; t < MT; t++) {
            const long idx = plane_entry((long)s, MT, t, lane);
            h[t] = g.xhi[idx];
            l[t] = g.xlo[idx];
            if (NS == 3) m2[t] = g.xlo2[idx];
        }
    };
    auto compute = [&](const float (&gv)[8], const bf16x8 (&h)[MT], const bf16x8 (&l)[MT], const bf16x8 (&m2)[NS == 3 ? MT : 1]) {
        bf16x8 bh, bl, bl2;
        split_frag<NS>(gv, bh, bl, bl2);
        mfma_split_terms<MT, NS>(h, l, m2, bh, bl, bl2, acc);
    };

    // G fragments run four K steps ahead (HBM latency: ~64 KiB in flight per CU), X fragments two
    // The loop is branch-free (the step count per wave is a multiple of 4, and the prefetch index
    // is clamped at the tail instead of guarded): any branch around a load makes hipcc drain
    // vmcnt(0) at the join, which serialises the whole prefetch.
    float gq[4][8];
    const int last = s1 - 1;
#pragma unroll
    for (int q = 0; q < 4; q++) load_g(s0 + q, gq[q]);
    load_a(s0, ah, al, am);
    load_a(s0 + 1, ahn, aln, amn);
    for (int s = s0; s < s1; s += 4) {
        compute(gq[0], ah, al, am);
        load_g(min(s + 4, last), gq[0]);
        load_a(min(s + 2, last), ah, al, am);
        compute(gq[1], ahn, aln, amn);
        load_g(min(s + 5, last), gq[1]);
        load_a(min(s + 3, last), ahn, aln, amn);
        compute(gq[2], ah, al, am);
        load_g(min(s + 6, last), gq[2]);
        load_a(min(s + 4, last), ah, al, am);
        compute(gq[3], ahn, aln, amn);
        load_g(min(s + 7, last), gq[3]);
        load_a(min(s + 5, last), ahn, aln, amn);
    }

    // ---- the two K halves of a column tile meet in LDS; the raw quarter-sum goes to its slab --------
    if (kh == 1) {
#pragma unroll
        for (int a = 0; a < MT; a++)
#pragma unroll
            for (int r = 0; r < 16; r++) red[((ct * MT + a) * 16 + r) * 64 + lane] = acc[a][r];
    }
    __syncthreads();
    if (kh == 0) {
        float *slab = g.slab + (long)blockIdx.y * g.M * g.N;
#pragma unroll
        for (int a = 0; a < MT; a++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float s = acc[a][r] + red[((ct * MT + a) * 16 + r) * 64 + lane];
                const int i = a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (i < g.M) slab[(long)i * g.N + col] = s;
            }
    }
}

// ---- symmetric G, whole matrix: stream ROWS of G ---------------------------------------------------
// out[:, j] = sum_k X[:, k] G[k][j] = sum_k X[:, k] G[j][k] when G is symmetric: the B operand of output
// column j is ROW j of G, which is contiguous in memory.  A workgroup owns 128 output columns = 128 rows
// of G and one K slice and walks it in chunks of 64 k.
//
// What the kernel above waits for is not G but its X fragments: every wave fetches them itself, two steps
// ahead, from an L2 that the G stream keeps flushing (measured: the same pass with deeper or wider G
// prefetch got slower, 75 -> 87 -> 131 us, whatever the shape of the G accesses; non-temporal G loads
// keep the planes in L2 but are themselves 30 % slower).  So here BOTH operands of a chunk go through
// LDS, and the roles are split by wave (a wave has one in-order counter for its loads):
//   * four LOADER waves keep two chunks in flight in their registers - the 128 x 64 panel of G
//     (32 KiB) and the chunk's slice of the X planes (contiguous: the planes are stored in fragment
//     order) - and copy the chunk that has arrived into one of two LDS images;
//   * eight COMPUTE waves (4 column tiles x 2 halves of the chunk's K steps; two per SIMD, so that one
//     converts / reads LDS while the other's MFMAs run) multiply the image before it: B fragments are
//     32-byte reads of 32 different rows (row stride 68 floats: conflict-free), A fragments whole
//     1-KiB reads; they issue no global load at all.
// One barrier per chunk.  Same MFMA schedule per K step and the same slab reduction as above; a column's
// K order is plain ascending inside the slice.  Deterministic.

template <int MT, int NS>
__global__ __launch_bounds__(SB_T) void skinny_rows_kernel(Bf2Dev g)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    constexpr int ABYTES = sb_abytes(MT, NS);
    constexpr int APLANE = MT * 256;                          // 16-byte entries of one plane's chunk slice
    constexpr int NA = NS * MT;                                // A entries per loader thread and chunk
    float *gb0 = reinterpret_cast<float *>(lds_raw), *gb1 = reinterpret_cast<float *>(lds_raw + SB_GBYTES);
    bf16x8 *ab0 = reinterpret_cast<bf16x8 *>(lds_raw + 2 * SB_GBYTES), *ab1 = reinterpret_cast<bf16x8 *>(lds_raw + 2 * SB_GBYTES + ABYTES);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // Workgroup -> (column tile bx, K slice by).  Workgroups are dealt round-robin to the 8 XCDs, each with
    // its own L2: all workgroups of one XCD are given the SAME K slice (or as few as possible), so that the
    // slice of the X planes they all re-read (planes / ks: ~1 MB) stays in that L2 beside the G stream; with
    // the plain mapping every XCD touches all of the planes (3 - 4.5 MB > its 4 MB L2) and the re-reads,
    // as many bytes as G itself, come from the Infinity Cache.
    int bx = blockIdx.x, by = blockIdx.y;
    {
        const int gx = gridDim.x, ks = gridDim.y;
        if (ks <= 8 && 8 % ks == 0 && (gx * ks) % 8 == 0 && gx % (8 / ks) == 0) {
            const int b = by * gx + bx, xcd = b & 7, w = b >> 3, per = 8 / ks;
            by = xcd / per;
            bx = w * per + xcd % per;
        }
    }
    const int j0 = bx * 128;
    const int kslice = g.K / (int)gridDim.y;                  // host: a multiple of 128
    const int kbeg = by * kslice;
    const int nchunks = kslice / SB_KC;
    const int st0 = kbeg / 16;                                // K step (of 16) of chunk c, step q: st0 + 4c + q

    if (wave >= 8) {
        // ---- loader -----------------------------------------------------------------------------------------
        // G: thread -> 16-byte column c4 of rows row + 16u (u < 8) of the chunk; buffer loads with one per-lane
        // byte offset, the row / chunk displacement is a scalar operand.
        const int lt = tid - 512, grow = lt >> 4, gc4 = lt & 15;
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.G), 0, (int)((long)g.K * g.ldg * (long)sizeof(float)), 0x00020000);
        const long base = (long)(j0 + grow) * g.ldg + kbeg + 4 * gc4;
        const int voff = (int)(base * (long)sizeof(float));
        const int row16 = (int)(16 * g.ldg * (long)sizeof(float));
        const PlaneRsrc rs = make_plane_rsrc<MT, NS>(g.xhi, g.xlo, g.xlo2, g.K);
        struct Stage { f32x4 gq[8]; bf16x8 aq[NA]; };
        Stage s0, s1;
        auto gload = [&](int c, Stage &st) {
            const int soff = c * SB_KC * (int)sizeof(float);
#pragma unroll
            for (int u = 0; u < 8; u++) st.gq[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff + u * row16, 0));
            const int a0 = slice_bytes<MT>(st0 + 4 * c);
#pragma unroll
            for (int v = 0; v < NA; v++) st.aq[v] = load_slice_entry<MT>(rs, a0, lt, v);
        };
        auto gstore = [&](int buf, const Stage &st) {
            float *gb = buf ? gb1 : gb0;
            bf16x8 *ab = buf ? ab1 : ab0;
#pragma unroll
            for (int u = 0; u < 8; u++) *reinterpret_cast<f32x4 *>(gb + (grow + 16 * u) * SB_RS + 4 * gc4) = st.gq[u];
#pragma unroll
            for (int v = 0; v < NA; v++) ab[lt + 256 * v] = st.aq[v];
        };
        // Chunk p is multiplied during iteration p, copied to LDS image p & 1 at the start of iteration
        // p - 1 and requested at iteration p - 3 into register set p & 1 (chunks 0..2: before the loop).
        const int last = nchunks - 1;
        gload(0, s0);
        gload(min(1, last), s1);
        gstore(0, s0);
        __builtin_amdgcn_sched_barrier(0);                     // chunk 2 goes into s0's registers, not a third set hoisted above the copy
        gload(min(2, last), s0);
        __syncthreads();
        // iteration cc: copy chunk cc+1 (waiting in `set`) into image `buf`, request chunk cc+3 into the same registers
        auto full = [&](int buf, Stage &set, int cc) { gstore(buf, set); gload(cc + 3, set); __syncthreads(); };
        auto part = [&](int buf, Stage &set, int cc) {
            if (cc >= nchunks) return;
            if (cc + 1 < nchunks) gstore(buf, set);
            if (cc + 3 < nchunks) gload(cc + 3, set);
            __syncthreads();
        };
        int c = 0;
        // steady state: no branch around a load (after one the compiler can no longer tell which requests
        // are older than the ones it waits for, and drains them all)
        for (; c + 4 < nchunks; c += 2) { full(1, s1, c); full(0, s0, c + 1); }
        // tail (at most four iterations): the same sequence with guards
        part(1, s1, c); part(0, s0, c + 1); part(1, s1, c + 2); part(0, s0, c + 3);
        __syncthreads();                                       // the compute waves' K-half exchange
        return;
    }

    // ---- compute: wave = (32-column tile, half of the chunk's four K steps), operands from LDS only ----------
    const int lc = lane & 31, lh = lane >> 5;
    const int nt = wave & 3, kh = wave >> 2;
    f32x16 acc[MT];
#pragma unroll
    for (int a = 0; a < MT; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[a][r] = 0.f;

    // operands of one K step, read from the LDS images: issued one step ahead of the MFMAs that use them
    // (this wave is alone on its SIMD as far as LDS latency goes)
    auto fetch = [&](const float *gb, const bf16x8 *ab, int q, Frag<MT, NS> &f) {
        const float *p = gb + (nt * 32 + lc) * SB_RS + 16 * q + 8 * lh;
        f.g0 = *reinterpret_cast<const f32x4 *>(p);
        f.g1 = *reinterpret_cast<const f32x4 *>(p + 4);
#pragma unroll
        for (int n = 0; n < NS; n++)
#pragma unroll
            for (int t = 0; t < MT; t++) f.a[n][t] = ab[n * APLANE + plane_entry(q, MT, t, lane)];
    };
    auto multiply = [&](const Frag<MT, NS> &f) {              // a lambda of the kernel: see Frag
        bf16x8 bh, bl, bl2;
        split_frag<NS>(f.g0, f.g1, bh, bl, bl2);
        mfma_split_terms<MT, NS>(f.a[0], f.a[NS >= 2 ? 1 : 0], f.a[NS - 1], bh, bl, bl2, acc);
    };
    Frag<MT, NS> fa;                                          // (the SIMD's other compute wave covers the LDS latency)
    __syncthreads();
    for (int c = 0; c < nchunks; c++) {
        const float *gb = (c & 1) ? gb1 : gb0;
        const bf16x8 *ab = (c & 1) ? ab1 : ab0;
        fetch(gb, ab, 2 * kh, fa);
        multiply(fa);
        fetch(gb, ab, 2 * kh + 1, fa);
        multiply(fa);
        __syncthreads();
    }

    // ---- the two K halves of a column tile meet in LDS; the raw slice sum goes to its slab ------------
    float *red = reinterpret_cast<float *>(lds_raw);          // 4*MT*16*64 floats <= the two G images
    if (kh == 1) {
#pragma unroll
        for (int a = 0; a < MT; a++)
#pragma unroll
            for (int r = 0; r < 16; r++) red[((nt * MT + a) * 16 + r) * 64 + lane] = acc[a][r];
    }
    __syncthreads();
    if (kh == 0) {
        float *slab = g.slab + (long)by * g.M * g.N;
        const int col = j0 + nt * 32 + lc;
#pragma unroll
        for (int a = 0; a < MT; a++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float sum = acc[a][r] + red[((nt * MT + a) * 16 + r) * 64 + lane];
                const int i = a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (i < g.M) slab[(long)i * g.N + col] = sum;
            }
    }
}

// The ordered sum of the K-slice slabs (splitk_reduce_f32's arithmetic: slices added in order, then alpha, E1, E2) that ALSO
// emits the two-way split planes of its result in fragment order: inside the Chebyshev recurrence the output of one filter
// product is the X of the next, so the next product needs no split_x_kernel launch of its own.  One thread per 8 consecutive
// columns of a row: 32-byte slab reads (a wave covers 2 KiB of a row), one 16-byte store per plane.
__global__ __launch_bounds__(256) void reduce_split_kernel(const float *slab, int split, int M, int MT, int N, float *C, long ldc, float alpha,
                                                           const float *E1, float b1, const float *E2, float b2, bf16x8 *hi, bf16x8 *lo)
{
    const long total = (long)M * N, q = N >> 3;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < (long)M * q; e += (long)gridDim.x * blockDim.x) {
        const int i = (int)(e / q), k8 = (int)(e % q), j = k8 * 8;
        const float *p = slab + (long)i * N + j;
        f32x4 s0 = *reinterpret_cast<const f32x4 *>(p), s1 = *reinterpret_cast<const f32x4 *>(p + 4);
        for (int z = 1; z < split; z++) {
            s0 += *reinterpret_cast<const f32x4 *>(p + (long)z * total);
            s1 += *reinterpret_cast<const f32x4 *>(p + (long)z * total + 4);
        }
        const long idx = (long)i * ldc + j;
        f32x4 o0 = alpha * s0, o1 = alpha * s1;
        if (E1) { o0 += b1 * *reinterpret_cast<const f32x4 *>(E1 + idx); o1 += b1 * *reinterpret_cast<const f32x4 *>(E1 + idx + 4); }
        if (E2) { o0 += b2 * *reinterpret_cast<const f32x4 *>(E2 + idx); o1 += b2 * *reinterpret_cast<const f32x4 *>(E2 + idx + 4); }
        *reinterpret_cast<f32x4 *>(C + idx) = o0;
        *reinterpret_cast<f32x4 *>(C + idx + 4) = o1;
        bf16x8 h, l, l2;
        split_frag<2>(o0, o1, h, l, l2);
        const long t = plane_entry_at(MT, i, k8);
        hi[t] = h;
        lo[t] = l;
    }
}

// The same ordered sum that ALSO forms the raw K-slice partials of a Gram product of its result, C * B^T with B = C itself
// (CholQR's first Gram matrix, SELF) or B = a second row block Y (the Rayleigh-Ritz T = Yb * Qo^T): the generic GEMM would
// read C back a few microseconds later for 150 MFLOP, in a launch of its own.  Workgroup = (128-column slab of C, 32-row
// tile ti of C); a slab is one or two whole Gram slices (eig_rules::gram_slicing).
//   * reduce: C = alpha * sum_z slab[z] + b1*E1 + b2*E2 with the operations of the reduce launch this one replaces, spelled
//     out so that no contraction can differ: the wide kernel's ((s0 + s1) + s2) + s3, or with `tree` what
//     splitk_reduce_kernel's butterfly leaves in lane 0 for four slices, ((0 + s0) + (0 + s1)) + ((0 + s2) + (0 + s3)) (the zeros
//     of its idle lanes added afterwards change nothing: that sum is never -0); then one multiply and two fused multiply-adds.
//     SELF reduces the rows of its own tile and of its partner tile (self_partner) and stores its own; otherwise the
//     tile's rows only, and B = Y's columns come from memory.  Both sit in LDS k-major ([column][row], gemm_kernel's image).
//   * Gram: wave = (32-row tile tj of B, slice of the slab): the k-ascending chain from zero of gemm_kernel on the same
//     v_mfma_f32_32x32x2_f32 with the same k pairing, so the partial slab holds the bits gemm_f32 would have written and
//     the ordered reduce of that slab is the unchanged second launch.
// No grid barrier, no atomics: every workgroup writes its own rows of C and its own entries of the Gram slab.
struct ReduceGramDev {
    const float *slab;            // [4][M][F] group sums of skinny_sym_kernel
    int M, F;
    float *C;
    long ldc;                     // also the row stride of E1 / E2
    float alpha;
    const float *E1;
    float b1;
    const float *E2;
    float b2;
    int tree;
    const float *Y;               // !SELF: [M][ldy]
    long ldy;
    float *gram;                  // [F / chunk][M][M]
    int chunk;                    // Gram slice: 64 or 128 columns
};
constexpr int RG_T = 512;
constexpr int RG_SA = 36;         // row stride of the A image (!SELF)
constexpr int rg_sb(int mt) { return mt * 32 + 4; }
constexpr int rg_lds_bytes(int mt, bool self) { return (128 * rg_sb(mt) + (self ? 0 : 128 * RG_SA)) * (int)sizeof(float); }

// SELF: C * C^T is symmetric bit for bit (element (j, i) is the same chain of the same products), so row tile ti forms the
// diagonal tile (ti, ti) and ONE off-diagonal tile (ti, partner) and stores the latter mirrored as well: with three row
// tiles the partners 1, 2, 0 cover all nine tiles, with two tile 0 takes tile 1.  A workgroup then needs the rows of two
// tiles, not of all.  -1: no partner.
template <int MT>
__device__ __forceinline__ int self_partner(int ti)
{
    return MT == 3 ? (ti + 1) % 3 : (MT == 2 && ti == 0 ? 1 : -1);
}

// The Gram phase of a workgroup that holds its operands k-major in LDS (A: the 32 rows of tile ti at As[k * SA + r], B: all
// rows at Bs[k * SB + row], k = column of the 128-column slab at c0): wave = (tile of B, slice of the slab), each the
// k-ascending chain from zero on v_mfma_f32_32x32x2_f32 with gemm_kernel's k pairing; raw partials to gram[slice][M][M].
template <int MT, bool SELF>
__device__ __forceinline__ void gram_tiles(const float *As, int SA, const float *Bs, int SB, int ti, int c0, int chunk, int M, float *gram)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 31, lh = lane >> 5;
    const int nsl = 128 / chunk, ntj = SELF ? (self_partner<MT>(ti) >= 0 ? 2 : 1) : MT;
    if (wave >= ntj * nsl) return;
    const int tj = SELF ? (wave % ntj == 0 ? ti : self_partner<MT>(ti)) : wave % ntj, sl = wave / ntj;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;
    const float *ap = As + (sl * chunk + lh) * SA + lr, *bp = Bs + (sl * chunk + lh) * SB + tj * 32 + lr;
    for (int k0 = 0; k0 < chunk; k0 += 16) {                  // (a slice is whole 16-column K tiles)
        float af[8], bf[8];
#pragma unroll
        for (int kk = 0; kk < 8; kk++) { af[kk] = ap[(k0 + 2 * kk) * SA]; bf[kk] = bp[(k0 + 2 * kk) * SB]; }
#pragma unroll
        for (int kk = 0; kk < 8; kk++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk], bf[kk], acc, 0, 0, 0);
    }
    float *gs = gram + (long)(c0 / chunk + sl) * M * M;
    const int j = tj * 32 + lr;
    const bool mirror = SELF && tj != ti;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int i = ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (i < M && j < M) {
            gs[(long)i * M + j] = acc[r];
            if (mirror) gs[(long)j * M + i] = acc[r];
        }
    }
}

template <int MT, bool SELF>
__global__ __launch_bounds__(RG_T) void reduce_gram_kernel(ReduceGramDev g)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    constexpr int SB = rg_sb(MT), SA = SELF ? SB : RG_SA;
    const int tid = threadIdx.x, ti = blockIdx.y, c0 = blockIdx.x * 128;
    float *Bs = reinterpret_cast<float *>(lds_raw);
    float *As = SELF ? Bs + ti * 32 : Bs + 128 * SB;
    const long total = (long)g.M * g.F;

    // unit f of an image with ROWS rows: 16 bytes of row (f / 4) % ROWS, columns 16 * (f / 4 / ROWS) + 4 * (f % 4).
    // The loads are unconditional at a clamped row (a branch around them would serialise the units); rows >= M become zeros.
    auto reduced = [&](int row, int col, bool store) {
        const int rc = min(row, g.M - 1);
        const float *p = g.slab + (long)rc * g.F + c0 + col;
        const f32x4 s0 = *reinterpret_cast<const f32x4 *>(p), s1 = *reinterpret_cast<const f32x4 *>(p + total);
        const f32x4 s2 = *reinterpret_cast<const f32x4 *>(p + 2 * total), s3 = *reinterpret_cast<const f32x4 *>(p + 3 * total);
        const long idx = (long)rc * g.ldc + c0 + col;
        f32x4 e1 = {0.f, 0.f, 0.f, 0.f}, e2 = {0.f, 0.f, 0.f, 0.f};
        if (g.E1) e1 = *reinterpret_cast<const f32x4 *>(g.E1 + idx);
        if (g.E2) e2 = *reinterpret_cast<const f32x4 *>(g.E2 + idx);
        f32x4 o;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            float s;
            if (g.tree) s = __fadd_rn(__fadd_rn(__fadd_rn(0.f, s0[c]), __fadd_rn(0.f, s1[c])), __fadd_rn(__fadd_rn(0.f, s2[c]), __fadd_rn(0.f, s3[c])));
            else s = __fadd_rn(__fadd_rn(__fadd_rn(s0[c], s1[c]), s2[c]), s3[c]);
            float v = __fmul_rn(g.alpha, s);
            if (g.E1) v = __fmaf_rn(g.b1, e1[c], v);
            if (g.E2) v = __fmaf_rn(g.b2, e2[c], v);
            o[c] = v;
        }
        if (store && row < g.M) *reinterpret_cast<f32x4 *>(g.C + idx) = o;
        if (row >= g.M) o = f32x4{0.f, 0.f, 0.f, 0.f};
        return o;
    };
    auto to_image = [&](float *img, int stride, int r, int col, const f32x4 &v) {
#pragma unroll
        for (int c = 0; c < 4; c++) img[(col + c) * stride + r] = v[c];
    };
    if (SELF) {
        // the rows of the tile itself and of its partner (self_partner): the tiles the workgroup's Gram products need
        const int tp = self_partner<MT>(ti);
#pragma unroll
        for (int t = 0; t < (MT > 1 ? 2 : 1); t++) {
            if (t == 1 && tp < 0) break;
            const int r0 = 32 * (t == 0 ? ti : tp);
#pragma unroll
            for (int it = 0; it < 32 * 32 / RG_T; it++) {
                const int f = tid + RG_T * it, r = r0 + ((f >> 2) & 31), col = 16 * (f >> 7) + 4 * (f & 3);
                to_image(Bs, SB, r, col, reduced(r, col, t == 0));
            }
        }
    } else {
#pragma unroll
        for (int it = 0; it < 32 * 32 / RG_T; it++) {
            const int f = tid + RG_T * it, r = (f >> 2) & 31, col = 16 * (f >> 7) + 4 * (f & 3);
            to_image(As, SA, r, col, reduced(ti * 32 + r, col, true));
        }
#pragma unroll
        for (int it = 0; it < MT * 32 * 32 / RG_T; it++) {
            const int f = tid + RG_T * it, r = (f >> 2) % (MT * 32), col = 16 * ((f >> 2) / (MT * 32)) + 4 * (f & 3);
            f32x4 v = *reinterpret_cast<const f32x4 *>(g.Y + (long)min(r, g.M - 1) * g.ldy + c0 + col);
            if (r >= g.M) v = f32x4{0.f, 0.f, 0.f, 0.f};
            to_image(Bs, SB, r, col, v);
        }
    }
    __syncthreads();
    gram_tiles<MT, SELF>(As, SA, Bs, SB, ti, c0, g.chunk, g.M, g.gram);
}

// CholQR's dst = L^-1 * src by 128-column slabs, feeding what comes next.  Workgroup = (slab, 32-row tile ti of dst); L^-1
// (n <= 96 rows, transposed: the A operand k-major) and the slab of src (the B operand, k-major as it lies in memory) sit
// in LDS; wave = (row tile, 32 columns): gemm_kernel's chain for this product - k ascending from zero over K = n padded with
// zeros to whole 16-wide K tiles, the same MFMA and k pairing, alpha = 1 - so dst has the bits the GEMM launch gave it.
//   TAIL 0 (first pass): the Gram partials of dst for the second pass, as reduce_gram_kernel forms them (SELF: the
//   workgroup also computes the rows of its partner tile, self_partner).
//   TAIL 1 (second pass): the three-way split planes of its rows of dst (split_x_kernel's entries), so the exact product
//   that follows starts with its planes ready.
struct LinvApplyDev {
    const float *Linv;            // [n][ldl]
    long ldl;
    int n, F;
    const float *src;             // [n][ld]
    float *dst;
    long ld;
    float *gram;                  // TAIL 0: [F / chunk][n][n]
    int chunk;
    bf16x8 *hi, *lo, *lo2;        // TAIL 1
};
constexpr int LA_SS = 132;        // row stride of the src image [k][128 columns]
constexpr int LA_SL = 68;         // row stride of the L^-1 image [k][rows of tile ti | rows of its partner]
constexpr int la_lds_bytes(int mt) { return (96 * LA_SS + 96 * LA_SL + 128 * rg_sb(mt)) * (int)sizeof(float); }

template <int MT, int TAIL>
__global__ __launch_bounds__(RG_T) void linv_apply_kernel(LinvApplyDev g)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    constexpr int SB = rg_sb(MT);
    float *Ss = reinterpret_cast<float *>(lds_raw), *Lt = Ss + 96 * LA_SS, *Ds = Lt + 96 * LA_SL;
    const int tid = threadIdx.x, ti = blockIdx.y, c0 = blockIdx.x * 128;
    const int KP = (g.n + 15) / 16 * 16;                      // K as gemm_kernel walks it
    const int tp = TAIL == 0 ? self_partner<MT>(ti) : -1;
    // src: 16 bytes per thread, a row of the slab per 32 threads; rows beyond n are zeros
#pragma unroll
    for (int it = 0; it < 96 * 32 / RG_T; it++) {
        const int f = tid + RG_T * it, k = f >> 5, c4 = f & 31;
        f32x4 v = *reinterpret_cast<const f32x4 *>(g.src + (long)min(k, g.n - 1) * g.ld + c0 + 4 * c4);
        if (k >= g.n) v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (k < KP) *reinterpret_cast<f32x4 *>(Ss + k * LA_SS + 4 * c4) = v;
    }
    // L^-1 transposed: rows of tile ti in columns 0..31 of the image, of the partner in 32..63
#pragma unroll
    for (int it = 0; it < 64 * 96 / RG_T; it++) {
        const int f = tid + RG_T * it, il = f / 96, k = f % 96;
        const int row = 32 * (il < 32 ? ti : max(tp, 0)) + (il & 31);
        float v = g.Linv[(long)min(row, g.n - 1) * g.ldl + min(k, g.n - 1)];
        if (row >= g.n || k >= g.n || (il >= 32 && tp < 0)) v = 0.f;
        if (k < KP) Lt[k * LA_SL + il] = v;
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6, lr = lane & 31, lh = lane >> 5;
    const int t = wave >> 2, jt = wave & 3;
    if (t == 0 || tp >= 0) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.f;
        const float *ap = Lt + lh * LA_SL + t * 32 + lr, *bp = Ss + lh * LA_SS + jt * 32 + lr;
        for (int k0 = 0; k0 < KP; k0 += 16) {
            float af[8], bf[8];
#pragma unroll
            for (int kk = 0; kk < 8; kk++) { af[kk] = ap[(k0 + 2 * kk) * LA_SL]; bf[kk] = bp[(k0 + 2 * kk) * LA_SS]; }
#pragma unroll
            for (int kk = 0; kk < 8; kk++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk], bf[kk], acc, 0, 0, 0);
        }
        const int i0 = 32 * (t == 0 ? ti : tp), col = jt * 32 + lr;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (t == 0 && i < g.n) g.dst[(long)i * g.ld + c0 + col] = acc[r];
            Ds[col * SB + i] = acc[r];                        // (rows beyond n: their row of the L^-1 image is zero)
        }
    }
    __syncthreads();
    if (TAIL == 0) {
        gram_tiles<MT, true>(Ds + ti * 32, SB, Ds, SB, ti, c0, g.chunk, g.n, g.gram);
    } else {
        // one plane entry per thread: row ti * 32 + (tid & 31), the eight columns c8
        const int rr = tid & 31, c8 = tid >> 5;
        bf16x8 h, l, l2;
#pragma unroll
        for (int j = 0; j < 8; j++) split_f32<3>(Ds[(c8 * 8 + j) * SB + ti * 32 + rr], j, h, l, l2);
        const long e = plane_entry_at(MT, ti * 32 + rr, c0 / 8 + c8);
        g.hi[e] = h;
        g.lo[e] = l;
        g.lo2[e] = l2;
    }
}

// ---- symmetric G stored as its packed upper tiles: every tile leaves HBM once ------------------------------------------
// out[:, I] = sum_J X[:, J] G[J][I] over tile blocks; G[J][I] is the stored tile (I, J) read along its rows when I <= J
// ("direct", exactly the chunk of skinny_rows_kernel), or the stored tile (J, I) read along its COLUMNS when J < I
// ("transposed").  Every off-diagonal tile therefore has two users, output blocks I and J, and the Infinity Cache does
// not help (tools/mall_probe.cpp: a table that fits it streams at the HBM rate all the same) - the second read has to
// hit the XCD's own L2.  So the two users of a tile are put on the SAME XCD at the SAME time:
//   * the 64 tile rows are the vectors of Z_2^6; block I meets block I ^ d, d = 0..63.  The 64 differences are dealt to
//     four groups p by their two top bits h_p (01, 10, 11, 00); within group p the blocks are halved by a linear form
//     f_p that vanishes on the group's differences (bit 5, bit 4, bit 5 ^ bit 4, bit 5), so that I and I ^ d always
//     fall into the same half.  XCD x = 2 p + c takes the 32 blocks with f_p(I) = c, one workgroup each (one per CU),
//     and in step s = 0..15 workgroup I works on the tile it shares with I ^ (16 h_p + s): the partner workgroup is on
//     the same XCD and works on the same tile in the same step.  An XCD streams 16 tiles (1 MB) per step, each read
//     twice back to back, and touches the X planes of its own 32 blocks only (1.5 MB, re-read every step: L2-resident).
//   * every output block appears once per group: four partial slabs, summed in order by splitk_reduce_f32 - the same
//     reduction as before; a column's K order is fixed by the schedule.  Deterministic.
// Workgroups are dealt to XCDs round-robin by the hardware (block b -> XCD b % 8; observed, not guaranteed): a wrong guess
// costs the L2 hits (the kernel then moves the full 268 MB again), never correctness.
// Roles, LDS images, MFMA schedule and epilogue are those of skinny_rows_kernel; a transposed chunk is staged as
// [64 k][128 columns] (row stride 132) and its B fragments are eight 4-byte reads of 32 consecutive columns.
constexpr int SYM_TS = 132;                // LDS row stride of a transposed chunk image (floats)
static_assert(SB_KC * SYM_TS * 4 <= SB_GBYTES, "a transposed chunk image must fit the G image");

// Other widths (round 4): nt = K / 128 tile rows are embedded in Z_2^b, 2^b = the next power of two >= max(nt, 4); the same
// pairing runs on 4 * 2^b workgroups, of which those of a block I >= nt leave at once and the others skip partners
// J >= nt (a workgroup's list of real partners sits in LDS).  Below 64 tile rows there are fewer than 256 workgroups and
// the XCD placement is whatever the dispatcher does: the matrix is then at most 34 MB and the pass is short anyway.
struct SymDev {
    int M, K;
    int nt, lb;                   // tile rows K / 128, log2 of the padded tile count (2..6)
    const bf16x8 *xhi, *xlo, *xlo2;
    const float *G;               // packed upper tiles: tile (I, J), I <= J, at (I*nt - I*(I-1)/2 + J - I) * 16384 floats
    float *slab;                  // [4][M][K] raw partial sums
};

// FULL: the tile count is the power of two itself (K = 8192: 64 tile rows) - every partner is real and comes from bit
// arithmetic alone, no list in LDS inside the loop.
template <int MT, int NS, bool FULL>
__global__ __launch_bounds__(SB_T) void skinny_sym_kernel(SymDev g)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    constexpr int ABYTES = sb_abytes(MT, NS);
    constexpr int APLANE = MT * 256;
    constexpr int NA = NS * MT;
    const int NT = g.nt, lb = g.lb;                            // tile rows; 2^lb = padded tile count
    float *gb0 = reinterpret_cast<float *>(lds_raw), *gb1 = reinterpret_cast<float *>(lds_raw + SB_GBYTES);
    bf16x8 *ab0 = reinterpret_cast<bf16x8 *>(lds_raw + 2 * SB_GBYTES), *ab1 = reinterpret_cast<bf16x8 *>(lds_raw + 2 * SB_GBYTES + ABYTES);
    __shared__ int jlist[16];                                  // the real partners of this workgroup, in schedule order
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // workgroup -> (group p, half c, block I): see above (bits 5, 4 there are bits lb-1, lb-2 here)
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int p = xcd >> 1, c = xcd & 1;
    int I;
    if (p == 0 || p == 3) I = (c << (lb - 1)) | slot;
    else {
        const int b5 = slot >> (lb - 2), b4 = p == 1 ? c : (b5 ^ c);
        I = (b5 << (lb - 1)) | (b4 << (lb - 2)) | (slot & ((1 << (lb - 2)) - 1));
    }
    if (I >= NT) return;                                       // a block of the padding: the whole workgroup leaves
    const int dbase = (p == 0 ? 1 : (p == 1 ? 2 : (p == 2 ? 3 : 0))) << (lb - 2);
    int nchunks;                                               // real partner tiles x 2 halves of 64 k
    if (FULL) nchunks = 2 << (lb - 2);
    else {
        const int nslots = 1 << (lb - 2);
        int cnt = 0;
        for (int sl = 0; sl < nslots; sl++) {
            const int J = I ^ (dbase | sl);
            if (J < NT) { if (tid == 0) jlist[cnt] = J; cnt++; }
        }
        nchunks = 2 * cnt;
        __syncthreads();
    }
    if (!FULL && nchunks == 0) {
        // no real partner in this group (only possible beside padding blocks): the group's slab still has to hold zeros
        // for this block's columns, the reduction adds all four
        float *slab = g.slab + (long)p * g.M * g.K;
        for (int e = tid; e < g.M * 128; e += SB_T) slab[(long)(e >> 7) * g.K + I * 128 + (e & 127)] = 0.f;
        return;
    }
    // chunk cc: partner block, orientation, byte offset of the stored tile
    auto partner = [&](int cc) { return FULL ? (I ^ (dbase | (cc >> 1))) : jlist[cc >> 1]; };
    auto tile_bytes = [&](int J) {
        const int a = min(I, J), b = max(I, J);
        return (a * NT - a * (a - 1) / 2 + (b - a)) * (128 * 128 * (int)sizeof(float));
    };

    if (wave >= 8) {
        // ---- loader -----------------------------------------------------------------------------------------
        const int lt = tid - 512;
        // direct chunk: thread -> 16-byte column gc4 of tile rows grow + 16 u; transposed: column c4 of tile rows half*64 + kr + 8 u
        const int voff_d = ((lt >> 4) * 128 + 4 * (lt & 15)) * (int)sizeof(float);
        const int voff_t = ((lt >> 5) * 128 + 4 * (lt & 31)) * (int)sizeof(float);
        const int loff_d = (lt >> 4) * SB_RS + 4 * (lt & 15), loff_t = (lt >> 5) * SYM_TS + 4 * (lt & 31);
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(g.G), 0, (NT * (NT + 1) / 2) * 128 * 128 * (int)sizeof(float), 0x00020000);
        const PlaneRsrc rs = make_plane_rsrc<MT, NS>(g.xhi, g.xlo, g.xlo2, g.K);
        struct Stage { f32x4 gq[8]; bf16x8 aq[NA]; };
        Stage s0, s1;
        // The loads of a chunk are issued in ONE fixed order (G then X planes, fenced against the scheduler): hipcc places
        // its s_waitcnt from a per-register model that is merged conservatively at the loop header, and when the prologue
        // issues a set's loads in another order than the loop body does, the merged state makes a store in the loop wait
        // for the YOUNGEST load in flight (vmcnt(0): the chunk requested one barrier ago) instead of its own (vmcnt(14+)) -
        // the prefetch distance collapses to one chunk (seen in the ISA of round 3's kernel).
        auto gload = [&](int cc, Stage &st) {
            const int J = __builtin_amdgcn_readfirstlane(partner(cc)), half = cc & 1;
            const bool direct = I <= J;
            const int voff = direct ? voff_d : voff_t;
            const int soff = tile_bytes(J) + (direct ? half * 64 : half * 64 * 128) * (int)sizeof(float);
            const int ustep = (direct ? 16 : 8) * 128 * (int)sizeof(float);
            const int a0 = slice_bytes<MT>(J * 8 + half * 4);  // the X planes' slice for block J, this half
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 8; u++) {
                st.gq[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff + u * ustep, 0));
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int v = 0; v < NA; v++) {
                st.aq[v] = load_slice_entry<MT>(rs, a0, lt, v);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        auto gstore = [&](int cc, const Stage &st) {                 // into image cc & 1
            float *gb = (cc & 1) ? gb1 : gb0;
            bf16x8 *ab = (cc & 1) ? ab1 : ab0;
            const bool direct = I <= partner(cc);
            const int loff = direct ? loff_d : loff_t, lstep = direct ? 16 * SB_RS : 8 * SYM_TS;
#pragma unroll
            for (int u = 0; u < 8; u++) *reinterpret_cast<f32x4 *>(gb + loff + u * lstep) = st.gq[u];
#pragma unroll
            for (int v = 0; v < NA; v++) ab[lt + 256 * v] = st.aq[v];
        };
        // chunk q: multiplied in iteration q, copied to image q & 1 at the start of iteration q - 1, requested at iteration
        // q - 3 into register set q & 1 (chunks 0..2 before the loop); no branch around a load in the steady state
        // (nchunks is even and >= 2 here; the prologue is unconditional - chunk 2 is clamped to the last one, a harmless
        // re-load when there are only two - because a branch around a load would again leave the loop header with a
        // merged, conservative wait state)
        gload(0, s0);
        gload(1, s1);
        gstore(0, s0);
        gload(min(2, nchunks - 1), s0);
        __syncthreads();
        int cc = 0;
        for (; cc + 4 < nchunks; cc += 2) {
            gstore(cc + 1, s1); gload(cc + 3, s1); __syncthreads();
            gstore(cc + 2, s0); gload(cc + 4, s0); __syncthreads();
        }
        // tail: iterations cc .. nchunks - 1 (cc = nchunks - 4 when nchunks >= 4, else 0), the same sequence with guards
        // (cc is even here and so is nchunks: iterations in pairs, each with its own register set - a set chosen at run time
        // would put both into scratch memory)
        for (; cc < nchunks; cc += 2) {
            if (cc + 1 < nchunks) gstore(cc + 1, s1);
            if (cc + 3 < nchunks) gload(cc + 3, s1);
            __syncthreads();
            if (cc + 2 < nchunks) gstore(cc + 2, s0);
            if (cc + 4 < nchunks) gload(cc + 4, s0);
            __syncthreads();
        }
        __syncthreads();                                           // the compute waves' K-half exchange
        return;
    }

    // ---- compute: wave = (32-column tile of block I, half of the chunk's four K steps), operands from LDS only ------
    const int lc = lane & 31, lh = lane >> 5;
    const int nt = wave & 3, kh = wave >> 2;
    f32x16 acc[MT];
#pragma unroll
    for (int a = 0; a < MT; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[a][r] = 0.f;

    auto fetch = [&](const float *gb, const bf16x8 *ab, bool direct, int q, Frag<MT, NS> &f) {
        if (direct) {
            const float *pp = gb + (nt * 32 + lc) * SB_RS + 16 * q + 8 * lh;
            f.g0 = *reinterpret_cast<const f32x4 *>(pp);
            f.g1 = *reinterpret_cast<const f32x4 *>(pp + 4);
        } else {
            const float *pp = gb + (16 * q + 8 * lh) * SYM_TS + nt * 32 + lc;
#pragma unroll
            for (int j = 0; j < 4; j++) { f.g0[j] = pp[j * SYM_TS]; f.g1[j] = pp[(4 + j) * SYM_TS]; }
        }
#pragma unroll
        for (int n = 0; n < NS; n++)
#pragma unroll
            for (int t = 0; t < MT; t++) f.a[n][t] = ab[n * APLANE + plane_entry(q, MT, t, lane)];
    };
    // (Two fragment sets per wave - the second K step's reads in flight under the first one's MFMAs - were measured and
    // changed nothing: 59.3 against 59.6 us per pass.  Ablation of this kernel at M = 96, two-way, per pass incl. 10 us of
    // split + reduce: 60 us as is, 61 us without the G loads, 44 us without the compute waves' work, 32 us with neither -
    // the loaders' LDS stores and the compute waves' LDS reads and conversions add up rather than overlap.)
    auto multiply = [&](const Frag<MT, NS> &f) {              // a lambda of the kernel: see Frag
        bf16x8 bh, bl, bl2;
        split_frag<NS>(f.g0, f.g1, bh, bl, bl2);
        mfma_split_terms<MT, NS>(f.a[0], f.a[NS >= 2 ? 1 : 0], f.a[NS - 1], bh, bl, bl2, acc);
    };
    Frag<MT, NS> fa;
    __syncthreads();
    for (int cc = 0; cc < nchunks; cc++) {
        const float *gb = (cc & 1) ? gb1 : gb0;
        const bf16x8 *ab = (cc & 1) ? ab1 : ab0;
        const bool direct = I <= partner(cc);
        fetch(gb, ab, direct, 2 * kh, fa);
        multiply(fa);
        fetch(gb, ab, direct, 2 * kh + 1, fa);
        multiply(fa);
        __syncthreads();
    }

    // ---- the two K halves of a column tile meet in LDS; the raw group sum goes to its slab ---------------------------
    float *red = reinterpret_cast<float *>(lds_raw);
    if (kh == 1) {
#pragma unroll
        for (int a = 0; a < MT; a++)
#pragma unroll
            for (int r = 0; r < 16; r++) red[((nt * MT + a) * 16 + r) * 64 + lane] = acc[a][r];
    }
    __syncthreads();
    if (kh == 0) {
        float *slab = g.slab + (long)p * g.M * g.K;
        const int col = I * 128 + nt * 32 + lc;
#pragma unroll
        for (int a = 0; a < MT; a++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float sum = acc[a][r] + red[((nt * MT + a) * 16 + r) * 64 + lane];
                const int i = a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (i < g.M) slab[(long)i * g.K + col] = sum;
            }
    }
}

template <int MT, int NS>
void launch_sym(const SymDev &g, hipStream_t s)
{
    const size_t lds = sb_lds_bytes(MT, NS);
    if (g.nt == (1 << g.lb)) {
        ensure_dynamic_lds(reinterpret_cast<const void *>(skinny_sym_kernel<MT, NS, true>), (int)lds);
        hipLaunchKernelGGL((skinny_sym_kernel<MT, NS, true>), dim3(4u << g.lb), dim3(SB_T), lds, s, g);
    } else {
        ensure_dynamic_lds(reinterpret_cast<const void *>(skinny_sym_kernel<MT, NS, false>), (int)lds);
        hipLaunchKernelGGL((skinny_sym_kernel<MT, NS, false>), dim3(4u << g.lb), dim3(SB_T), lds, s, g);
    }
}

template <int MT, int NS>
void launch_rows(const Bf2Dev &g, dim3 grid, hipStream_t s)
{
    const size_t lds = sb_lds_bytes(MT, NS);
    ensure_dynamic_lds(reinterpret_cast<const void *>(skinny_rows_kernel<MT, NS>), (int)lds);
    hipLaunchKernelGGL((skinny_rows_kernel<MT, NS>), grid, dim3(SB_T), lds, s, g);
}

template <int MT, bool SELF>
void launch_reduce_gram(const ReduceGramDev &r, hipStream_t s)
{
    constexpr int lds = rg_lds_bytes(MT, SELF);
    ensure_dynamic_lds(reinterpret_cast<const void *>(reduce_gram_kernel<MT, SELF>), lds);
    hipLaunchKernelGGL((reduce_gram_kernel<MT, SELF>), dim3(r.F / 128, MT), dim3(RG_T), lds, s, r);
}

// May the reduction of this symmetric product be the one that also emits the Gram partials the caller asked for?
bool reduce_gram_fits(const SkinnyArgs &a)
{
    auto al16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (!a.gram_slab || a.emit_planes || a.M > 96 || (a.gram_chunk != 64 && a.gram_chunk != 128)) return false;
    if (a.ldc % 4 != 0 || !al16(a.slab) || !al16(a.C) || !al16(a.E1) || !al16(a.E2) || a.C == a.E1 || a.C == a.E2) return false;
    if (a.gram_with && (a.gram_ld % 4 != 0 || !al16(a.gram_with) || a.gram_with == a.C)) return false;
    return true;
}

}  // namespace

void split_planes_bf16(const float *X, long ldx, int M, int K, void *hi, void *lo, void *lo2, hipStream_t s)
{
    const int mt = (M + 31) / 32;
    const long total = (long)(K / 16) * mt * 64;
    hipLaunchKernelGGL(split_x_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, X, ldx, M, mt, K,
                       static_cast<bf16x8 *>(hi), static_cast<bf16x8 *>(lo), static_cast<bf16x8 *>(lo2));
    DLCO_HIP(hipGetLastError());
}

size_t bf16x2_plane_bytes(int M, int K) { return (size_t)((M + 31) / 32) * 32 * K * sizeof(__bf16); }
size_t bf16x2_slab_floats(int M, int N, int ksplit) { return (size_t)(ksplit > 0 ? ksplit : KS) * M * N; }

// Returns false when the shape is not supported (the caller then takes gemm_f32).
bool skinny_product_bf16x2(const SkinnyArgs &a, hipStream_t s)
{
    const int M = a.M, N = a.N, K = a.K;
    const long ldg = a.ldg;
    const float *G = a.G;
    void *plane_lo2 = a.planes.lo2;
    const int mt = (M + 31) / 32;
    const int ks = a.ksplit > 0 ? a.ksplit : KS;
    if (M < 1 || mt > 5 || N % 128 != 0 || K % (16 * ks * 2 * 4) != 0) return false;   // 4 steps per loop trip
    if (a.ldx % 4 != 0 || (reinterpret_cast<uintptr_t>(a.X) & 15) != 0) return false;
    split_planes_bf16(a.X, a.ldx, M, K, a.planes.hi, a.planes.lo, plane_lo2, s);
    Bf2Dev g;
    g.M = M; g.N = N; g.K = K;
    g.xhi = static_cast<const bf16x8 *>(a.planes.hi); g.xlo = static_cast<const bf16x8 *>(a.planes.lo);
    g.xlo2 = static_cast<const bf16x8 *>(plane_lo2);
    g.G = G; g.ldg = ldg; g.slab = a.slab;
    const dim3 grid(N / 128, ks), block(T8);
    // whole symmetric matrix: stream its rows through LDS (skinny_rows_kernel)
    // (four row tiles with the three-way split do not fit the register budget of the split-role kernel)
    if (N == K && K % (128 * ks) == 0 && ldg % 4 == 0 && (reinterpret_cast<uintptr_t>(G) & 15) == 0 &&
        (long)K * ldg * 4 < (1L << 31) && !(mt >= 4 && plane_lo2)) {
        if (plane_lo2) dispatch_mt<4>(mt, [&](auto MT) { launch_rows<MT(), 3>(g, grid, s); });
        else dispatch_mt<5>(mt, [&](auto MT) { launch_rows<MT(), 2>(g, grid, s); });   // 160 rows: blocks of rank ~128 + guards in ONE pass over G
        DLCO_HIP(hipGetLastError());
        splitk_reduce_f32(a.slab, ks, M, N, a.C, a.ldc, a.alpha, 0.f, a.E1, a.b1, a.E2, a.b2, s);
        return true;
    }
    if (mt > 4) return false;                                  // only the row-streaming kernel takes five row tiles
    if (plane_lo2) dispatch_mt<4>(mt, [&](auto MT) { hipLaunchKernelGGL((skinny_bf16x2_kernel<MT(), 3>), grid, block, 0, s, g); });   // three-way split: fp32-level accuracy
    else dispatch_mt<4>(mt, [&](auto MT) { hipLaunchKernelGGL((skinny_bf16x2_kernel<MT(), 2>), grid, block, 0, s, g); });
    DLCO_HIP(hipGetLastError());
    splitk_reduce_f32(a.slab, ks, M, N, a.C, a.ldc, a.alpha, 0.f, a.E1, a.b1, a.E2, a.b2, s);
    return true;
}

// CholQR's dst = Linv * src as the column-slab kernel that also feeds the next launch (linv_apply_kernel); false, and
// nothing launched, where the shape does not fit: the caller then takes gemm_f32.
bool linv_apply_slab(const LinvApplyArgs &a, hipStream_t s)
{
    auto al16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool planes = a.planes.hi != nullptr;
    if (a.n < 1 || a.n > 96 || a.F % 128 != 0 || a.ld % 4 != 0 || !al16(a.src) || !al16(a.dst) || a.src == a.dst) return false;
    if (planes ? (!a.planes.lo || !a.planes.lo2 || a.gram_slab != nullptr) : (!a.gram_slab || (a.gram_chunk != 64 && a.gram_chunk != 128))) return false;
    LinvApplyDev g;
    g.Linv = a.Linv; g.ldl = a.ldl; g.n = a.n; g.F = a.F;
    g.src = a.src; g.dst = a.dst; g.ld = a.ld;
    g.gram = a.gram_slab; g.chunk = a.gram_chunk;
    g.hi = static_cast<bf16x8 *>(a.planes.hi); g.lo = static_cast<bf16x8 *>(a.planes.lo); g.lo2 = static_cast<bf16x8 *>(a.planes.lo2);
    dispatch_mt<3>((a.n + 31) / 32, [&](auto MT) {
        constexpr int lds = la_lds_bytes(MT());
        const dim3 grid(a.F / 128, MT());
        if (planes) {
            ensure_dynamic_lds(reinterpret_cast<const void *>(linv_apply_kernel<MT(), 1>), lds);
            hipLaunchKernelGGL((linv_apply_kernel<MT(), 1>), grid, dim3(RG_T), lds, s, g);
        } else {
            ensure_dynamic_lds(reinterpret_cast<const void *>(linv_apply_kernel<MT(), 0>), lds);
            hipLaunchKernelGGL((linv_apply_kernel<MT(), 0>), grid, dim3(RG_T), lds, s, g);
        }
    });
    DLCO_HIP(hipGetLastError());
    return true;
}

// The reduction of skinny_product_sym alone, in the form that also emits the Gram partials a.gram_slab asks for
// (reduce_gram_kernel); false, and nothing launched, where a does not ask for them or the shape does not fit.
bool reduce_gram_sym(const SkinnyArgs &a, hipStream_t s)
{
    const int M = a.M, F = a.K;
    if (a.N != F || F % 128 != 0 || M < 1 || !reduce_gram_fits(a)) return false;
    ReduceGramDev r;
    r.slab = a.slab; r.M = M; r.F = F;
    r.C = a.C; r.ldc = a.ldc;
    r.alpha = a.alpha; r.E1 = a.E1; r.b1 = a.b1; r.E2 = a.E2; r.b2 = a.b2;
    r.tree = splitk_reduce_is_wide(a.slab, 4, M, F, a.C, a.ldc, a.E1, a.E2) ? 0 : 1;
    r.Y = a.gram_with; r.ldy = a.gram_ld;
    r.gram = a.gram_slab; r.chunk = a.gram_chunk;
    dispatch_mt<3>((M + 31) / 32, [&](auto MT) {
        if (a.gram_with) launch_reduce_gram<MT(), false>(r, s);
        else launch_reduce_gram<MT(), true>(r, s);
    });
    DLCO_HIP(hipGetLastError());
    return true;
}

// The same product for a symmetric G given as its packed upper tiles (see skinny_sym_kernel).
bool skinny_product_sym(const SkinnyArgs &a, hipStream_t s)
{
    const int M = a.M, F = a.K;
    void *plane_hi = a.planes.hi, *plane_lo = a.planes.lo, *plane_lo2 = a.planes.lo2;
    const int mt = (M + 31) / 32;
    const int nt = F / 128;
    if (a.N != F || F % 128 != 0 || nt < 1 || nt > 64 || M < 1 || mt > 5 || (mt >= 4 && plane_lo2)) return false;
    if (a.ldx % 4 != 0 || (reinterpret_cast<uintptr_t>(a.X) & 15) != 0 || (reinterpret_cast<uintptr_t>(a.G) & 15) != 0) return false;
    if (a.emit_planes && plane_lo2) return false;              // the planes a reduction emits are the two-way ones
    if (!a.planes_ready) split_planes_bf16(a.X, a.ldx, M, F, plane_hi, plane_lo, plane_lo2, s);
    SymDev g;
    g.M = M; g.K = F;
    g.nt = nt; g.lb = 2;
    while ((1 << g.lb) < nt) g.lb++;
    g.xhi = static_cast<const bf16x8 *>(plane_hi); g.xlo = static_cast<const bf16x8 *>(plane_lo); g.xlo2 = static_cast<const bf16x8 *>(plane_lo2);
    g.G = a.G; g.slab = a.slab;
    if (plane_lo2) dispatch_mt<3>(mt, [&](auto MT) { launch_sym<MT(), 3>(g, s); });
    else dispatch_mt<5>(mt, [&](auto MT) { launch_sym<MT(), 2>(g, s); });
    DLCO_HIP(hipGetLastError());
    if (a.emit_planes && a.ldc % 4 == 0 && (reinterpret_cast<uintptr_t>(a.C) & 15) == 0) {
        // the product kernel has read the planes of X: they now receive the planes of the result, rows up to 32 mt zeroed by
        // the split of the first product of the chain (rows >= M of a tile are never written here and stay zero)
        const long work = (long)M * (F / 8);
        hipLaunchKernelGGL(reduce_split_kernel, dim3((unsigned)std::min<long>((work + 255) / 256, 4096)), dim3(256), 0, s, a.slab, 4, M, mt, F, a.C, a.ldc,
                           a.alpha, a.E1, a.b1, a.E2, a.b2, static_cast<bf16x8 *>(plane_hi), static_cast<bf16x8 *>(plane_lo));
        DLCO_HIP(hipGetLastError());
    } else if (reduce_gram_sym(a, s)) {
        if (a.gram_done) *a.gram_done = true;
    } else {
        splitk_reduce_f32(a.slab, 4, M, F, a.C, a.ldc, a.alpha, 0.f, a.E1, a.b1, a.E2, a.b2, s);
    }
    return true;
}

}  // namespace dlco
