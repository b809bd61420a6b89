// kernels_match_u8.hip — the 8-bit line beside kernels_match.hip: nearest and second-nearest row of one table of byte
// descriptors in another (dlco_desc_match_u8), the whole matrix of the same distances (dlco_desc_cross_sqdists_u8), and the
// kernel that turns a chunk of float descriptor rows into bytes by the rule of quant_rules.hpp (the _u8 forms of describe):
//
//   desc_quantize_kernel    one thread per element: quant_rules::quantize_one
//   match_u8_norms_kernel   |a|^2 of every row in int32, a = u - 128 (the byte with its top bit flipped, read as int8)
//   match_u8_kernel         d(i,j) = |a_q|^2 + |a_t|^2 - 2 a_q.a_t in int32, the dot products on v_mfma_i32_16x16x64_i8;
//                           then either the running top two per query, or (STORE) the matrix itself: one tile loop, two
//                           epilogues, so the matrix and the top two cannot disagree
//   match_u8_kernel<.., GUIDED>   the guided forms (dlco_desc_match_guided_u8, _epipolar_u8 and their kin): the same tile loop with a
//                           third epilogue, on the records the float line's record kernels write
//   match_u8_kernel<.., BATCH>   the batch forms (dlco_desc_match_pairs_u8, the plan: match_batch.hpp): many (query image, train
//                           image) pairs over one segmented table in one 1-D launch; a workgroup finds its pair in the
//                           uploaded plan and runs the plain form's tile loop
//
// What the float line states too is in match_dev.hpp: the guided forms and their dispatch, the geometry a row brings and how it
// moves, the verdict, the top two under a key with the merge over slices (match_merge_kernel; the slicing rule:
// match_slices.hpp), a batched workgroup's entry.
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
#include "match_dev.hpp"
#include "match_slices.hpp"
#include "quant_rules.hpp"

namespace dlco {

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

// the byte line's key: larger key (smaller distance) first, equal keys by smaller index; a partial holds the keys, and a
// result is the query's norm |a_q|^2 = qnorm[qrow] less the key, INT32_MAX for an empty slot
struct ByteKey {
    using Key = int;
    static __device__ __forceinline__ bool first(int ka, int ja, int kb, int jb) { return ka > kb || (ka == kb && ja < jb); }
    static __device__ __forceinline__ i32x4 pack(const Top2<int> t) { return i32x4{t.k1, t.j1, t.k2, t.j2}; }
    static __device__ __forceinline__ Top2<int> unpack(const i32x4 p) { return Top2<int>{p[0], p[1], p[2], p[3]}; }
    static __device__ __forceinline__ void write(const Top2<int> t, long qrow, long row, const int32_t *qnorm, int32_t *idx, int32_t *sqdist)
    {
        const int n = qnorm[qrow];
        idx[2 * row] = t.j1; idx[2 * row + 1] = t.j2;
        sqdist[2 * row] = t.j1 < 0 ? INT_MAX : n - t.k1;
        sqdist[2 * row + 1] = t.j2 < 0 ? INT_MAX : n - t.k2;
    }
};

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

// BATCH (dlco_desc_match_pairs_u8; STORE = 0): a 1-D grid over the workgroups of every entry of a launch of the plan
// (match_batch.hpp).  query is the one table [.][ldq] whose segments are the images, qnorm and tneg the norms of all its rows
// in both signs; the workgroup finds its entry and takes from it what the plain form takes from its arguments and its grid:
// the query image's and the train image's first row (tables, norms), nq, nt, tiles_per_slice, the first output row, the
// offset of the entry's partials (part stays null when the entry has one slice), its query block and its slice.  Tiles are
// counted from the slice's first row, which need not be tile-aligned in the table; the rows at and beyond jend belong to
// the next image (or lie beyond the table) and are never read: the loads clamp to jbeg.  The loop below is the plain form's.
//   A guided form (dlco_desc_match_guided*_u8; GuidedForm, match_dev.hpp): the same tile loop with a third epilogue.  A
// candidate that admits<GUIDED> does not admit takes the key kEmpty before it meets the running top two, and then loses as a
// row beyond the slice does; STORE writes INT32_MAX for it.  The workgroup's queries' geometry is written to LDS once, before
// the loop; a train tile's is staged beside Tn, both buffers, under the same barrier.  Per 16-row block a lane reads the
// geometry of its four train rows once and that of its query of every block, and keeps the sixteen verdicts as a bit mask
// (bit 4 qb + reg: sixteen entries of one row block, the layout of the int8 MFMA's result).  MULTI forms them with the last
// chunk of a tile.  BATCH: bind_entry_guide rebinds records and coordinates to the entry's own.
struct NoGuide {};
template <int GUIDED> struct GuideArg { using type = MatchGuide; };
template <> struct GuideArg<kPlain> { using type = NoGuide; };      // the plain forms keep their arguments

template <bool STORE, bool MULTI, int GUIDED = kPlain, bool BATCH = false>
__global__ __launch_bounds__(UTH) void match_u8_kernel(const uint8_t *__restrict__ query, long ldq, int nq, const uint8_t *__restrict__ train,
                                                       long ldt, int nt, int r, const int32_t *__restrict__ qnorm,
                                                       const int32_t *__restrict__ tneg, int tiles_per_slice, int32_t *__restrict__ idx,
                                                       int32_t *__restrict__ sqdist, i32x4 *__restrict__ part, int32_t *__restrict__ out,
                                                       const match_batch::Entry *__restrict__ ent, int n_ent,
                                                       const typename GuideArg<GUIDED>::type g)
{
    unsigned qblk = blockIdx.x, slice = blockIdx.y;
    const double *grec = nullptr, *gqrec = nullptr;        // GUIDED: the records and the coordinates the loop reads
    const float *gxy = nullptr;
    long gld = 0;
    double gt2 = 0.0;
    if constexpr (GUIDED != kPlain) { grec = g.rec; gqrec = g.qrec; gxy = g.xy; gld = g.ldxy; gt2 = g.t2; }
    if constexpr (BATCH) {
        const int wg = (int)blockIdx.x;
        const int ei = batch_entry_of(ent, n_ent, wg, [](const match_batch::Entry &x) { return x.wg0; });
        const match_batch::Entry e = ent[ei];
        if constexpr (GUIDED != kPlain) bind_entry_guide<GUIDED>(g, e, ei, grec, gqrec, gxy);
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
    constexpr int CW = train_geom_width(GUIDED), QW = query_geom_width(GUIDED);
    __shared__ __attribute__((aligned(16))) double Tg[GUIDED ? 2 : 1][GUIDED ? UT * CW : 1];   // GUIDED: the tile's geometry, staged with it,
    __shared__ __attribute__((aligned(16))) double Qg[GUIDED ? UQ * QW : 1];   // and the workgroup's queries': written once, before the loop
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
    double rg[CW];
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
        geom_fetch<GUIDED>(rg, grec, gxy, gld, jn < jend ? jn : (long)jbeg);   // a row beyond the slice: the slice's first row's, never consulted
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int u = 0; u < UT / 32; u++) *reinterpret_cast<i32x4 *>(&Bs[buf][(lrow + 32 * u) * UP + 16 * lseg]) = rb[u];
        if (tid < UT) {
            Tn[buf][tid] = rtn;
            if constexpr (GUIDED != kPlain) geom_store(&Tg[buf][tid * CW], rg);
        }
    };
    // GUIDED: the geometry of the lane's query of block qb.  The empty asm hides from the compiler that the queries' address
    // does not change over the tile loop: hoisted out of it, the four records would sit in registers for the whole loop.
    auto qgeom = [&](int qb) {
        int qoff = (wave * UWQ + 16 * qb + li) * QW;
        asm volatile("" : "+v"(qoff));
        Geom o{};                                          // not geom_read: through it these reads compile to other LDS instructions
#pragma unroll
        for (int e = 0; e < QW; e += 2) {
            const f64x2 t = *reinterpret_cast<const f64x2 *>(&Qg[qoff + e]);
            o.v[e] = t[0]; o.v[e + 1] = t[1];
        }
        return o;
    };
    // which of the sixteen entries of the 16-row block sub of the staged tile the rule admits: bit 4 qb + reg
    auto admit_mask = [&](int buf, int sub) -> unsigned {
        unsigned m = 0;
        Geom t[4];
#pragma unroll
        for (int reg = 0; reg < 4; reg++) t[reg] = geom_read<CW>(&Tg[buf][(16 * sub + 4 * lg + reg) * CW]);
#pragma unroll
        for (int qb = 0; qb < UQB; qb++) {
            const Geom q = qgeom(qb);
#pragma unroll
            for (int reg = 0; reg < 4; reg++) m |= (admits<GUIDED>(q, t[reg], gt2) ? 1u : 0u) << (4 * qb + reg);
        }
        return m;
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

    // GUIDED: the geometry of the workgroup's queries, a record or (x, y) (query_geom_fill), a thread per query; the
    // barrier before the loop orders it
    if constexpr (GUIDED != kPlain) {
        query_geom_fill<GUIDED>(&Qg[tid * QW], grec, gqrec, gxy, gld, (long)qblk * UQ + tid, nq);
    }
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
    // GUIDED: bit reg of m is the verdict of the entry
    auto entries = [&](const i32x4 dot, int qb, const i32x4 tn, int blk, long jrow0, unsigned m) {
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            int key = (dot[reg] << 1) + tn[reg];
            if (STORE) {
                const int q = q0 + 16 * qb + li;
                const long j = jrow0 + reg;
                int d = qn[qb] - key;
                if constexpr (GUIDED != kPlain) d = ((m >> reg) & 1u) != 0 ? d : INT_MAX;
                if (q < nq && j < jend) out[(long)q * nt + j] = d;
            } else {
                if constexpr (GUIDED != kPlain) key = ((m >> reg) & 1u) != 0 ? key : kEmpty;
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
                unsigned adm = 0;
                if constexpr (GUIDED != kPlain) {
                    if (!MULTI || kc == nch - 1) adm = admit_mask(buf, sub);
                }
#pragma unroll
                for (int qb = 0; qb < UQB; qb++) {
                    i32x4 d = MULTI ? (kc == 0 ? zacc : acc[MULTI ? sub : 0][MULTI ? qb : 0]) : zacc;
                    d = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, fb[qb][0], d, 0, 0, 0);
                    d = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, fb[qb][1], d, 0, 0, 0);
                    if (MULTI) acc[MULTI ? sub : 0][MULTI ? qb : 0] = d;
                    if (!MULTI || kc == nch - 1) entries(d, qb, tn, tile * USUB + sub, jrow0, adm >> (4 * qb));
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
        Top2<int> me;
        me.k1 = b1[qb]; me.k2 = b2[qb];
        me.j1 = c1[qb] < 0 ? -1 : jbeg + (c1[qb] >> 2) * 16 + 4 * lg + (c1[qb] & 3);
        me.j2 = c2[qb] < 0 ? -1 : jbeg + (c2[qb] >> 2) * 16 + 4 * lg + (c2[qb] & 3);
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) me = merge2<ByteKey>(me, shfl_xor_top2(me, o));
        const int q = q0 + 16 * qb + li;
        if (lg == 0 && q < nq) {
            if (part) part[(long)slice * nq + q] = ByteKey::pack(me);
            else ByteKey::write(me, q, q, qnorm, idx, sqdist);
        }
    }
}

// what a launch passes for the guide: the geometry, or nothing at all for the plain forms
template <int GUIDED> typename GuideArg<GUIDED>::type guide_arg(const MatchGuide &g)
{
    if constexpr (GUIDED != kPlain) return g; else return NoGuide{};
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
// one slice.  guide: nullptr, or the geometry of the guided form (dlco_internal.hpp), as match_top2 takes it.
void match_u8_top2(const uint8_t *query, long ldq, int nq, const uint8_t *train, long ldt, int nt, int r, const int32_t *qnorm,
                   const int32_t *tneg, int tiles_per_slice, int32_t *idx, int32_t *sqdist, void *part, int32_t *out, const MatchGuide *guide,
                   hipStream_t s)
{
    if (nq <= 0 || nt <= 0) return;
    const int slices = match_slicing::slices(match_slicing::kU8, nt, tiles_per_slice);
    const dim3 grid((unsigned)((nq + UQ - 1) / UQ), (unsigned)slices);
    i32x4 *pp = (!out && slices > 1) ? static_cast<i32x4 *>(part) : nullptr;
    const MatchGuide g = guide ? *guide : MatchGuide{};
    dispatch_form(guided_form_of(guide), [&](auto form) {
        dispatch_bool(out != nullptr, [&](auto store) {
            dispatch_bool(r > UK, [&](auto multi) {
                hipLaunchKernelGGL((match_u8_kernel<store.value, multi.value, form.value>), grid, dim3(UTH), 0, s, query, ldq, nq, train, ldt, nt, r,
                                   qnorm, tneg, tiles_per_slice, idx, sqdist, pp, out, nullptr, 0, guide_arg<form.value>(g));
            });
        });
    });
    DLCO_HIP(hipGetLastError());
    if (pp) {
        hipLaunchKernelGGL((match_merge_kernel<ByteKey, false, const int32_t, int32_t, int32_t>), dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, pp, slices, nq,
                           qnorm, idx, sqdist);
        DLCO_HIP(hipGetLastError());
    }
}

// One launch of a batched match (match_batch.hpp): table [.][ld], qnorm = |a|^2 and tneg = -|a|^2 of all its rows, the launch's
// n_ent entries in device memory, wgs workgroups of the tile loop, merge_wgs of the merge (0: every entry has one slice).
// guide: nullptr, or the geometry of the guided batch, as match_top2_batch takes it: rec the launch's record buffer, already
// written (match_records_batch), off its entries' record rows, xy / ldxy the coordinates of the whole table.
void match_u8_top2_batch(const uint8_t *table, long ld, int r, const int32_t *qnorm, const int32_t *tneg, const match_batch::Entry *ent, int n_ent,
                         long wgs, long merge_wgs, int32_t *idx, int32_t *sqdist, void *part, const MatchGuide *guide, hipStream_t s)
{
    if (n_ent <= 0 || wgs <= 0) return;
    i32x4 *pp = static_cast<i32x4 *>(part);
    const dim3 grid((unsigned)wgs);
    const MatchGuide g = guide ? *guide : MatchGuide{};
    dispatch_form(guided_form_of(guide), [&](auto form) {
        dispatch_bool(r > UK, [&](auto multi) {
            hipLaunchKernelGGL((match_u8_kernel<false, multi.value, form.value, true>), grid, dim3(UTH), 0, s, table, ld, 0, nullptr, 0L, 0, r, qnorm,
                               tneg, 0, idx, sqdist, pp, nullptr, ent, n_ent, guide_arg<form.value>(g));
        });
    });
    DLCO_HIP(hipGetLastError());
    if (merge_wgs > 0) {
        hipLaunchKernelGGL((match_merge_kernel<ByteKey, true, const int32_t, int32_t, int32_t>), dim3((unsigned)merge_wgs), dim3(256), 0, s, pp, ent, n_ent,
                           qnorm, idx, sqdist);
        DLCO_HIP(hipGetLastError());
    }
}

}  // namespace dlco
