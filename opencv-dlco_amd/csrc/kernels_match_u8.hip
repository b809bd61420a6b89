// kernels_match_u8.hip — the 8-bit line beside kernels_match.hip: nearest and second-nearest row of one table of byte
// descriptors in another (dlco_desc_match_u8), the whole matrix of the same distances (dlco_desc_cross_sqdists_u8), and the
// kernel that turns a chunk of float descriptor rows into bytes by the rule of quant_rules.hpp (the _u8 forms of describe):
//
//   desc_quantize_kernel    one thread per element: quant_rules::quantize_one
//   match_u8_norms_kernel   |a|^2 of every row in int32, a = u - 128 (the byte with its top bit flipped, read as int8)
//   match_u8_kernel         d(i,j) = |a_q|^2 + |a_t|^2 - 2 a_q.a_t in int32, the dot products on v_mfma_i32_16x16x64_i8;
//                           then either the running top two per query, or (STORE) the matrix itself: one tile loop, two
//                           epilogues, so the matrix and the top two cannot disagree
//   match_u8_merge_kernel   the top two of a query over the S slices of train (the slicing rule: match_slices.hpp)
//   match_u8_kernel<.., BATCH>, match_u8_merge_batch_kernel   the batch forms (dlco_desc_match_pairs_u8, the plan: match_batch.hpp):
//                           many (query image, train image) pairs over one segmented table in one 1-D launch; a workgroup
//                           finds its pair in the uploaded plan and runs the plain form's tile loop
//
// Everything is an integer: differences do not see the shift by 128, |a|^2 <= 1024 * 128^2 = 2^24 and every partial stays
// below 2^26 in magnitude, so d is the exact sum_k (q_ik - t_jk)^2 <= 1024 * 255^2 and nothing depends on an order of
// accumulation.  Candidates are ordered by (d, train index); the slices hold disjoint train rows, so the result does not
// depend on the grouping.
//
// Inside the kernels a candidate is the key 2 a_q.a_t - |a_t|^2 = |a_q|^2 - d, LARGER is nearer: the query's own norm
// is the same for all its candidates and is only subtracted when a result is written, and the key is one shift-and-add
// behind the MFMA.  Keys are above -2^27; the empty slot is (kEmpty = -2^30, index -1) and loses against every real one.
//
// Tables are [n][ld] bytes with ld % 16 == 0 and 16-byte aligned: a row is read in 16-byte pieces up to
// ceil(r / 16) * 16 <= ld, the bytes at and beyond r are replaced by zeros after the flip.  Every load is unconditional
// and in bounds (a row or piece beyond the edge reads a valid one and is replaced by zeros), stores are masked.
#include "dlco_internal.hpp"
#include "match_batch.hpp"
#include "match_slices.hpp"
#include "quant_rules.hpp"

namespace dlco {

typedef int i32x4 __attribute__((ext_vector_type(4)));

namespace {

// The MFMA's M side (A operand, result rows 4 (lane >> 4) + reg) is train, its N side (B operand, result column
// lane & 15) the queries: a lane then holds ONE query per 16-query block and meets that query's train rows in ascending
// order, four per MFMA, so a query block costs a lane one running (best, second) and the columns need no butterfly over
// 16 lanes, only over the four lane groups.  A wave owns 64 queries (four blocks; their B fragments of a 128-byte k chunk
// are 32 VGPRs), four waves own 256 and read every staged tile of train: UT rows x 128 bytes in LDS, two buffers, fetched
// to registers one step ahead of its use.  Both operands are cut into 16-byte pieces by the same rule (lane group g takes
// bytes [16 g, 16 g + 16) of every 64), so whatever order of k the instruction gives those bytes, it is the same on both
// sides.  r <= 128 is one chunk per tile; beyond it (MULTI) the accumulators of all UT / 16 row blocks are kept over the
// chunks of a tile and the query fragments are re-read per chunk: correct, not tuned.
using match_slicing::UQ;                // queries per workgroup: 256 (match_slices.hpp, with the slicing rule)
constexpr int UWQ = 64;                // queries per wave
constexpr int UQB = UWQ / 16;          // 16-query blocks per wave
using match_slicing::UT;                // train rows per staged tile: 128
constexpr int UK = 128;                // bytes of k per staged chunk
constexpr int UP = UK + 16;            // LDS pitch in bytes: the 16-byte reads of 16 rows fall into 16 different bank groups
constexpr int UTH = 256;
constexpr int USUB = UT / 16;
constexpr int kEmpty = -(1 << 30);

struct Top2 { int k1; int j1; int k2; int j2; };

// (key, index) order: larger key (smaller distance) first, equal keys by smaller index
__device__ __forceinline__ bool key_first(int ka, int ja, int kb, int jb) { return ka > kb || (ka == kb && ja < jb); }

// top two of the union of two top-two lists of disjoint candidates
__device__ __forceinline__ Top2 merge2(const Top2 a, const Top2 b)
{
    Top2 o;
    const bool b_first = key_first(b.k1, b.j1, a.k1, a.j1);
    const int wk = b_first ? b.k1 : a.k1, lk = b_first ? a.k1 : b.k1;          // winner / loser of the two firsts
    const int wj = b_first ? b.j1 : a.j1, lj = b_first ? a.j1 : b.j1;
    const int sk = b_first ? b.k2 : a.k2;                                      // the winner's own second
    const int sj = b_first ? b.j2 : a.j2;
    const bool l_second = key_first(lk, lj, sk, sj);
    o.k1 = wk; o.j1 = wj;
    o.k2 = l_second ? lk : sk;
    o.j2 = l_second ? lj : sj;
    return o;
}

// the 16 bytes [k, k + 16) of a row as int8 a = u - 128, with the bytes at and beyond r, or all of them (!ok), zero
__device__ __forceinline__ i32x4 piece(i32x4 v, int k, int r, bool ok)
{
    i32x4 o;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int nv = ok ? r - (k + 4 * e) : 0;                               // bytes of this dword below r
        const unsigned m = nv >= 4 ? 0xffffffffu : (nv <= 0 ? 0u : ((1u << (8 * nv)) - 1u));
        o[e] = (int)(((unsigned)v[e] ^ 0x80808080u) & m);
    }
    return o;
}

// The entry of the plan that workgroup wg of a batched launch belongs to: the last one whose first workgroup (`first`
// picks wg0 or mwg0) is not above wg.  wg is the same for the whole workgroup, so the search is scalar loads and branches.
template <typename First>
__device__ __forceinline__ int batch_entry_of(const match_batch::Entry *__restrict__ ent, int n_ent, int wg, First first)
{
    int lo = 0, hi = n_ent;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first(ent[mid]) <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

// BATCH (dlco_desc_match_pairs_u8; STORE = 0): a 1-D grid over the workgroups of every entry of a launch of the plan
// (match_batch.hpp).  query is the one table [.][ldq] whose segments are the images, qnorm and tneg the norms of all its rows
// in both signs; the workgroup finds its entry and takes from it what the plain form takes from its arguments and its grid:
// the query image's and the train image's first row (tables, norms), nq, nt, tiles_per_slice, the first output row, the
// offset of the entry's partials (part stays null when the entry has one slice), its query block and its slice.  Tiles are
// counted from the slice's first row, which need not be tile-aligned in the table; the rows at and beyond jend belong to
// the next image (or lie beyond the table) and are never read: the loads clamp to jbeg.  The loop below is the plain form's.
template <bool STORE, bool MULTI, bool BATCH = false>
__global__ __launch_bounds__(UTH) void match_u8_kernel(const uint8_t *__restrict__ query, long ldq, int nq, const uint8_t *__restrict__ train,
                                                       long ldt, int nt, int r, const int32_t *__restrict__ qnorm,
                                                       const int32_t *__restrict__ tneg, int tiles_per_slice, int32_t *__restrict__ idx,
                                                       int32_t *__restrict__ sqdist, i32x4 *__restrict__ part, int32_t *__restrict__ out,
                                                       const match_batch::Entry *__restrict__ ent, int n_ent)
{
    unsigned qblk = blockIdx.x, slice = blockIdx.y;
    if constexpr (BATCH) {
        const int wg = (int)blockIdx.x;
        const match_batch::Entry e = ent[batch_entry_of(ent, n_ent, wg, [](const match_batch::Entry &x) { return x.wg0; })];
        const unsigned w = (unsigned)(wg - e.wg0);
        slice = w / (unsigned)e.qblocks;
        qblk = w - slice * (unsigned)e.qblocks;
        train = query + e.t0 * ldq; ldt = ldq; tneg += e.t0;
        query += e.q0 * ldq; qnorm += e.q0;
        nq = e.nq; nt = e.nt; tiles_per_slice = e.tiles_per_slice;
        idx += 2 * e.out0; sqdist += 2 * e.out0;
        part = e.slices > 1 ? part + e.part0 : nullptr;
    }
    __shared__ __attribute__((aligned(16))) uint8_t Bs[2][UT * UP];            // the staged tile, flipped and masked when stored
    __shared__ __attribute__((aligned(16))) int32_t Tn[2][UT];                 // -|a_t|^2 of its rows, kEmpty beyond the slice
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int q0 = qblk * UQ + wave * UWQ;
    const bool wave_on = q0 < nq;                          // uniform over the wave
    const int jbeg = (int)((long)slice * tiles_per_slice * UT);    // this slice of train: [jbeg, jend), never empty (jbeg < nt)
    const int jend = (int)min((long)nt, (long)jbeg + (long)tiles_per_slice * UT);
    const int ntile = (jend - jbeg + UT - 1) / UT;
    const int nch = MULTI ? (r + UK - 1) / UK : 1;
    const int nstep = ntile * nch;
    const int r16 = (r + 15) & ~15;

    // loader: thread t fetches the 16-byte piece lseg of the train rows lrow + 32 u of a tile, and the first UT threads
    // the negated squared norm of one of its rows
    const int lrow = tid >> 3, lseg = tid & 7;
    i32x4 rb[UT / 32];
    int rtn;
    auto gload = [&](int step) {
        step = min(step, nstep - 1);                       // past the end: the last step again, never used
        const int tile = step / nch, kc = step - tile * nch;
        const int k = kc * UK + 16 * lseg;
        const int kk = k < r16 ? k : 0;
        const long jt = (long)jbeg + (long)tile * UT;      // nt may be just below 2^31
#pragma unroll
        for (int u = 0; u < UT / 32; u++) {
            const long j = jt + lrow + 32 * u;
            const bool ok = j < jend;
            const i32x4 v = *reinterpret_cast<const i32x4 *>(train + (ok ? j : (long)jbeg) * ldt + kk);
            rb[u] = piece(v, k, r, ok);
        }
        const long jn = jt + (tid & (UT - 1));
        const int tn = tneg[jn < jend ? jn : (long)jbeg];
        rtn = jn < jend ? tn : kEmpty;
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int u = 0; u < UT / 32; u++) *reinterpret_cast<i32x4 *>(&Bs[buf][(lrow + 32 * u) * UP + 16 * lseg]) = rb[u];
        if (tid < UT) Tn[buf][tid] = rtn;
    };

    // B fragments of one k chunk: lane (li, lg) holds query q0 + 16 qb + li at the bytes 64 c + 16 lg ... + 15 of the chunk
    i32x4 fb[UQB][UK / 64];
    auto bload = [&](int kc) {
#pragma unroll
        for (int qb = 0; qb < UQB; qb++) {
            const int q = q0 + 16 * qb + li;
            const bool ok = q < nq;
            const uint8_t *qrow = query + (long)(ok ? q : 0) * ldq;
#pragma unroll
            for (int c = 0; c < UK / 64; c++) {
                const int k = kc * UK + 64 * c + 16 * lg;
                const i32x4 v = *reinterpret_cast<const i32x4 *>(qrow + (k < r16 ? k : 0));
                fb[qb][c] = piece(v, k, r, ok);
            }
        }
    };
    if (!MULTI) bload(0);

    int qn[UQB];                                           // STORE: |a_q|^2 of the lane's query of every block
    if (STORE) {
#pragma unroll
        for (int qb = 0; qb < UQB; qb++) {
            const int q = q0 + 16 * qb + li;
            qn[qb] = qnorm[q < nq ? q : 0];
        }
    }
    // running (best, second) of the lane's query of every block over the train rows == 4 lg + reg (mod 16).  The index
    // kept in the loop is the wave-uniform count (16-row block of the slice) * 4 + reg, turned into a train row at the
    // end; a lane meets its rows in ascending order, so a strict comparison keeps the smaller index among equal keys.
    int b1[UQB], b2[UQB], c1[UQB], c2[UQB];
#pragma unroll
    for (int qb = 0; qb < UQB; qb++) { b1[qb] = kEmpty; b2[qb] = kEmpty; c1[qb] = -1; c2[qb] = -1; }

    // the four results of one MFMA: query q0 + 16 qb + li against the train rows jt + 16 sub + 4 lg + reg
    auto entries = [&](const i32x4 dot, int qb, const i32x4 tn, int blk, long jrow0) {
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int key = (dot[reg] << 1) + tn[reg];
            if (STORE) {
                const int q = q0 + 16 * qb + li;
                const long j = jrow0 + reg;
                if (q < nq && j < jend) out[(long)q * nt + j] = qn[qb] - key;
            } else {
                const int cnt = blk * 4 + reg;
                const bool first = key > b1[qb], second = key > b2[qb];
                c2[qb] = first ? c1[qb] : (second ? cnt : c2[qb]);
                c1[qb] = first ? cnt : c1[qb];
                b2[qb] = max(b2[qb], min(key, b1[qb]));
                b1[qb] = max(b1[qb], key);
            }
        }
    };
    const i32x4 zacc = i32x4{0, 0, 0, 0};
    i32x4 acc[MULTI ? USUB : 1][MULTI ? UQB : 1];

    gload(0);
    lstore(0);
    __syncthreads();
    for (int step = 0; step < nstep; step++) {
        const int buf = step & 1;
        gload(step + 1);
        if (wave_on) {
            const int tile = step / nch, kc = step - tile * nch;
            if (MULTI) bload(kc);
#pragma unroll
            for (int sub = 0; sub < USUB; sub++) {
                const uint8_t *ap = &Bs[buf][(16 * sub + li) * UP + 16 * lg];
                const i32x4 a0 = *reinterpret_cast<const i32x4 *>(ap), a1 = *reinterpret_cast<const i32x4 *>(ap + 64);
                const i32x4 tn = *reinterpret_cast<const i32x4 *>(&Tn[buf][16 * sub + 4 * lg]);
                const long jrow0 = (long)jbeg + (long)tile * UT + 16 * sub + 4 * lg;
#pragma unroll
                for (int qb = 0; qb < UQB; qb++) {
                    i32x4 d = MULTI ? (kc == 0 ? zacc : acc[MULTI ? sub : 0][MULTI ? qb : 0]) : zacc;
                    d = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, fb[qb][0], d, 0, 0, 0);
                    d = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, fb[qb][1], d, 0, 0, 0);
                    if (MULTI) acc[MULTI ? sub : 0][MULTI ? qb : 0] = d;
                    if (!MULTI || kc == nch - 1) entries(d, qb, tn, tile * USUB + sub, jrow0);
                }
            }
        }
        lstore(buf ^ 1);                                   // every wave left that buffer before the barrier of the step before
        __syncthreads();
    }
    if (STORE || !wave_on) return;
    // the four lane groups of a query hold disjoint train rows: butterfly under the key, every lane ends with the top two
#pragma unroll
    for (int qb = 0; qb < UQB; qb++) {
        Top2 me;
        me.k1 = b1[qb]; me.k2 = b2[qb];
        me.j1 = c1[qb] < 0 ? -1 : jbeg + (c1[qb] >> 2) * 16 + 4 * lg + (c1[qb] & 3);
        me.j2 = c2[qb] < 0 ? -1 : jbeg + (c2[qb] >> 2) * 16 + 4 * lg + (c2[qb] & 3);
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
            Top2 other;
            other.k1 = __shfl_xor(me.k1, o, 64); other.j1 = __shfl_xor(me.j1, o, 64);
            other.k2 = __shfl_xor(me.k2, o, 64); other.j2 = __shfl_xor(me.j2, o, 64);
            me = merge2(me, other);
        }
        const int q = q0 + 16 * qb + li;
        if (lg == 0 && q < nq) {
            if (part) {
                part[(long)slice * nq + q] = i32x4{me.k1, me.j1, me.k2, me.j2};
            } else {
                const int n = qnorm[q];
                idx[2 * (long)q] = me.j1; idx[2 * (long)q + 1] = me.j2;
                sqdist[2 * (long)q] = me.j1 < 0 ? INT_MAX : n - me.k1;
                sqdist[2 * (long)q + 1] = me.j2 < 0 ? INT_MAX : n - me.k2;
            }
        }
    }
}

// the merge of a batched launch: 256 rows of an entry with more than one slice per workgroup, numbered from its mwg0
__global__ __launch_bounds__(256) void match_u8_merge_batch_kernel(const i32x4 *__restrict__ part, const match_batch::Entry *__restrict__ ent,
                                                                   int n_ent, const int32_t *__restrict__ qnorm, int32_t *__restrict__ idx,
                                                                   int32_t *__restrict__ sqdist)
{
    const int wg = (int)blockIdx.x;
    const match_batch::Entry e = ent[batch_entry_of(ent, n_ent, wg, [](const match_batch::Entry &x) { return x.mwg0; })];
    const int row = (wg - e.mwg0) * 256 + threadIdx.x;
    if (row >= e.nq) return;
    const i32x4 *pp = part + e.part0;
    const i32x4 p0 = pp[row];
    Top2 me{p0[0], p0[1], p0[2], p0[3]};
    for (int s = 1; s < e.slices; s++) {
        const i32x4 p = pp[(long)s * e.nq + row];
        me = merge2(me, Top2{p[0], p[1], p[2], p[3]});
    }
    const int n = qnorm[e.q0 + row];
    const long o = 2 * (e.out0 + row);
    idx[o] = me.j1; idx[o + 1] = me.j2;
    sqdist[o] = me.j1 < 0 ? INT_MAX : n - me.k1;
    sqdist[o + 1] = me.j2 < 0 ? INT_MAX : n - me.k2;
}

__global__ __launch_bounds__(256) void match_u8_merge_kernel(const i32x4 *__restrict__ part, int slices, int nq, const int32_t *__restrict__ qnorm,
                                                             int32_t *__restrict__ idx, int32_t *__restrict__ sqdist)
{
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= nq) return;
    const i32x4 p0 = part[row];
    Top2 me{p0[0], p0[1], p0[2], p0[3]};
    for (int s = 1; s < slices; s++) {
        const i32x4 p = part[(long)s * nq + row];
        me = merge2(me, Top2{p[0], p[1], p[2], p[3]});
    }
    const int n = qnorm[row];
    idx[2 * (long)row] = me.j1; idx[2 * (long)row + 1] = me.j2;
    sqdist[2 * (long)row] = me.j1 < 0 ? INT_MAX : n - me.k1;
    sqdist[2 * (long)row + 1] = me.j2 < 0 ? INT_MAX : n - me.k2;
}

constexpr int NTH = 256;               // four rows per workgroup, one wave each

__global__ __launch_bounds__(NTH) void match_u8_norms_kernel(const uint8_t *__restrict__ x, long ld, long n, int r, int negate,
                                                             int32_t *__restrict__ norm)
{
    const long row = (long)blockIdx.x * (NTH / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const uint32_t *p = reinterpret_cast<const uint32_t *>(x + row * ld);
    int s = 0;
    for (int w = lane; 4 * w < r; w += 64) {               // the dword [4 w, 4 w + 4): below ceil(r / 4) * 4 <= ld
        const uint32_t v = p[w];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int a = (int)((v >> (8 * e)) & 255u) - 128;
            s += 4 * w + e < r ? a * a : 0;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) norm[row] = negate ? -s : s;
}

__global__ __launch_bounds__(256) void desc_quantize_kernel(const float *__restrict__ Y, long ldy, int n, int r, float scale,
                                                            const float *__restrict__ offset, uint8_t *__restrict__ out, long ldo)
{
    const int i = blockIdx.x * 256 + threadIdx.x;          // n * r <= 2^21: a chunk of describe
    if (i >= n * r) return;
    const int row = i / r, k = i - row * r;
    out[(long)row * ldo + k] = quant_rules::quantize_one(Y[(long)row * ldy + k], offset[k], scale);
}

}  // namespace

// bytes out [n][ldo] (r written per row, the others left alone) of the float rows Y [n][ldy]; offset [r] in device memory
void desc_quantize_rows(const float *Y, long ldy, int n, int r, float scale, const float *offset, uint8_t *out, long ldo, hipStream_t s)
{
    if (n <= 0 || r <= 0) return;
    hipLaunchKernelGGL(desc_quantize_kernel, dim3((unsigned)(((long)n * r + 255) / 256)), dim3(256), 0, s, Y, ldy, n, r, scale, offset, out, ldo);
    DLCO_HIP(hipGetLastError());
}

// |a|^2 of the rows of x [n][ld], a = u - 128, or its negative (the form the tile loop takes for train)
void match_u8_norms(const uint8_t *x, long ld, long n, int r, bool negate, int32_t *norm, hipStream_t s)
{
    if (n <= 0) return;
    const long per = NTH / 64;
    hipLaunchKernelGGL(match_u8_norms_kernel, dim3((unsigned)((n + per - 1) / per)), dim3(NTH), 0, s, x, ld, n, r, negate ? 1 : 0, norm);
    DLCO_HIP(hipGetLastError());
}

// query [nq][ldq], train [nt][ldt], qnorm = |a_q|^2 and tneg = -|a_t|^2 from match_u8_norms.  out != nullptr: the matrix
// out[nq][nt]; else idx / sqdist [nq][2], through part [slices][nq] (16 bytes each) when tiles_per_slice leaves more than
// one slice.
void match_u8_top2(const uint8_t *query, long ldq, int nq, const uint8_t *train, long ldt, int nt, int r, const int32_t *qnorm,
                   const int32_t *tneg, int tiles_per_slice, int32_t *idx, int32_t *sqdist, void *part, int32_t *out, hipStream_t s)
{
    if (nq <= 0 || nt <= 0) return;
    const int slices = match_slicing::slices(match_slicing::kU8, nt, tiles_per_slice);
    const dim3 grid((unsigned)((nq + UQ - 1) / UQ), (unsigned)slices);
    i32x4 *pp = (!out && slices > 1) ? static_cast<i32x4 *>(part) : nullptr;
    const bool multi = r > UK;
#define DLCO_MATCH_U8_LAUNCH(ST, MU)                                                                                                  \
    hipLaunchKernelGGL((match_u8_kernel<ST, MU>), grid, dim3(UTH), 0, s, query, ldq, nq, train, ldt, nt, r, qnorm, tneg, tiles_per_slice, \
                       idx, sqdist, pp, out, nullptr, 0)
    if (out) { if (multi) DLCO_MATCH_U8_LAUNCH(true, true); else DLCO_MATCH_U8_LAUNCH(true, false); }
    else     { if (multi) DLCO_MATCH_U8_LAUNCH(false, true); else DLCO_MATCH_U8_LAUNCH(false, false); }
#undef DLCO_MATCH_U8_LAUNCH
    DLCO_HIP(hipGetLastError());
    if (pp) {
        hipLaunchKernelGGL(match_u8_merge_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, pp, slices, nq, qnorm, idx, sqdist);
        DLCO_HIP(hipGetLastError());
    }
}

// One launch of a batched match (match_batch.hpp): table [.][ld], qnorm = |a|^2 and tneg = -|a|^2 of all its rows, the launch's
// n_ent entries in device memory, wgs workgroups of the tile loop, merge_wgs of the merge (0: every entry has one slice).
void match_u8_top2_batch(const uint8_t *table, long ld, int r, const int32_t *qnorm, const int32_t *tneg, const match_batch::Entry *ent, int n_ent,
                         long wgs, long merge_wgs, int32_t *idx, int32_t *sqdist, void *part, hipStream_t s)
{
    if (n_ent <= 0 || wgs <= 0) return;
    i32x4 *pp = static_cast<i32x4 *>(part);
    const dim3 grid((unsigned)wgs);
#define DLCO_MATCH_U8_BATCH_LAUNCH(MU)                                                                                                \
    hipLaunchKernelGGL((match_u8_kernel<false, MU, true>), grid, dim3(UTH), 0, s, table, ld, 0, nullptr, 0L, 0, r, qnorm, tneg, 0, idx, sqdist, \
                       pp, nullptr, ent, n_ent)
    if (r > UK) DLCO_MATCH_U8_BATCH_LAUNCH(true); else DLCO_MATCH_U8_BATCH_LAUNCH(false);
#undef DLCO_MATCH_U8_BATCH_LAUNCH
    DLCO_HIP(hipGetLastError());
    if (merge_wgs > 0) {
        hipLaunchKernelGGL(match_u8_merge_batch_kernel, dim3((unsigned)merge_wgs), dim3(256), 0, s, pp, ent, n_ent, qnorm, idx, sqdist);
        DLCO_HIP(hipGetLastError());
    }
}

}  // namespace dlco
