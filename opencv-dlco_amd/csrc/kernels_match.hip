// kernels_match.hip — nearest and second-nearest row of one descriptor table in another (dlco_desc_match) and the
// whole matrix of the same distances (dlco_desc_cross_sqdists):
//
//   match_norms_kernel    |row|^2 of a table in double, one wave per row: lane l sums the elements l, l + 64, ...
//                         in order, then a fixed butterfly; the order depends on r alone
//   match_top2_kernel     d(i,j) = max(0, |q_i|^2 + |t_j|^2 - 2 q_i.t_j) in double with the dot products on
//                         v_mfma_f64_16x16x4_f64 (fp32 operands widened exactly: the queries when their fragments
//                         are read, a train tile when it is stored to LDS), rounded to float once; then either the running top two per query
//                         under the key (float distance, train index), or (STORE) the matrix itself: one tile loop, two
//                         epilogues, so the matrix and the top two cannot disagree
//   match_top2_kernel<.., GUIDED>   the guided forms (dlco_desc_match_guided*, dlco_desc_match_guided_epipolar*; GuidedForm,
//                         match_dev.hpp): the same tile loop with a third epilogue.  A candidate enters the running top two only if
//                         admits<GUIDED> says so, and STORE writes +inf for one that is not admitted; distance, key, merge and
//                         slices are those of the plain form, so a guided answer is the top two of the plain matrix with +inf where
//                         the predicate fails.  A train tile's geometry is staged beside Tn, the workgroup's queries' sits in
//                         LDS, and a lane keeps the verdicts of a pair of column blocks as a bit mask: eight entries of two
//                         column blocks, the layout of the f64 MFMA's result.  MULTI forms a tile's epipolar verdicts before
//                         the A fragments of its last chunk are fetched, one byte per pair of column blocks: beside the
//                         epilogue, with every accumulator live, they cost scratch.
//   match_records_kernel, match_epi_records_kernel, match_records_batch_kernel   the records of the rows of a table under H or F
//                         (record_of, store_record: match_dev.hpp), one lane per row; both lines read them
//   match_top2_kernel<.., BATCH>, match_fill_kernel   the batch forms (dlco_desc_match_pairs*, the plan: match_batch.hpp): many
//                         (query image, train image) pairs over one segmented table in one 1-D launch; a workgroup finds its
//                         pair in the uploaded plan and runs the plain form's tile loop.  Guided: every pair has a matrix of its
//                         own, so a launch forms the records of its entries into one buffer
//
// What the byte line (kernels_match_u8.hip) states too is in match_dev.hpp: the guided forms and their dispatch, the geometry
// a row brings and how it moves, the verdict, the top two under a key with the merge over slices (match_merge_kernel; the
// slicing rule: match_slices.hpp), a batched workgroup's entry.
//
// The key is a total order and the slices hold disjoint train rows, so the result does not depend on the grouping.
// An entry's accumulation is one chain of MFMAs over k in an order fixed by r: it depends neither on where the query
// or the train row sits, nor on nq, nt or the slice count.
//
// Tables are [n][ld] floats with ld % 4 == 0 and 16-byte aligned: a row is read in 16-byte pieces up to
// ceil(r / 4) * 4 <= ld, the elements at and beyond r are replaced by zeros.  Every load is unconditional and in
// bounds (a row or piece beyond the edge reads a valid one and is replaced by zeros), stores are masked.
#include "match_dev.hpp"
#include "match_slices.hpp"

namespace dlco {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

// A wave owns 16 queries (the M of the f64 MFMA) and keeps their A fragments of a whole 128-wide k chunk in registers
// (one float per lane and k-step: 32 VGPRs, which the compiler widens once: 64); eight waves, two per SIMD, own 128
// queries and read every staged tile of train: TN rows x 128 k in LDS as doubles (133 KB: one workgroup per CU), fetched
// to registers one step ahead of its use and widened once, at the LDS store, so that no conversion sits between the MFMAs.  r <= 128 is one chunk per tile (the
// case of every shipped model); beyond it (MULTI) the accumulators of all TN / 16 column blocks are kept over the
// chunks of a tile and the A fragments are re-read per chunk: correct, not tuned.
using match_slicing::MQ;                // queries per workgroup: 128 (match_slices.hpp, with the slicing rule)
using match_slicing::TN;                // train rows per staged tile: 128
constexpr int KC = 128;                // k per staged chunk
constexpr int MP = KC + 2;             // LDS pitch in doubles: the 16-byte reads of 16 rows fall into 16 different bank groups
constexpr int MTH = 512;
constexpr int NSUB = TN / 16;

// the float line's key is the distance itself: smaller distance first, equal distances by smaller index; a partial holds
// the distances' bits
struct FloatKey {
    using Key = float;
    static __device__ __forceinline__ bool first(float da, int ja, float db, int jb) { return da < db || (da == db && ja < jb); }
    static __device__ __forceinline__ i32x4 pack(const Top2<float> t) { return i32x4{__float_as_int(t.k1), t.j1, __float_as_int(t.k2), t.j2}; }
    static __device__ __forceinline__ Top2<float> unpack(const i32x4 p) { return Top2<float>{__int_as_float(p[0]), p[1], __int_as_float(p[2]), p[3]}; }
    static __device__ __forceinline__ void write(const Top2<float> t, long, long row, int32_t *idx, float *sqdist)
    {
        idx[2 * row] = t.j1; idx[2 * row + 1] = t.j2;
        sqdist[2 * row] = t.k1; sqdist[2 * row + 1] = t.k2;
    }
};

// BATCH (dlco_desc_match_pairs; STORE = 0, GUIDED = kPlain): a 1-D grid over the workgroups of every entry of a launch of the plan
// (match_batch.hpp).  query is the one table [.][ldq] whose segments are the images and qnorm the norms of all its rows;
// the workgroup finds its entry and takes from it what the plain form takes from its arguments and its grid: the query
// image's and the train image's first row (tables, norms), nq, nt, tiles_per_slice, the first output row, the offset of the
// entry's partials (part stays null when the entry has one slice), its query block and its slice.  Tiles are counted from
// the slice's first row, which need not be tile-aligned in the table; the rows at and beyond jend belong to the next image
// (or lie beyond the table) and are never read: the loads clamp to jbeg.  The loop below is the plain form's.
//   BATCH with a guided form (dlco_desc_match_pairs_guided*): geometry belongs to the pair, and bind_entry_guide rebinds it.
template <bool STORE, bool MULTI, int GUIDED, bool BATCH = false>
__global__ __launch_bounds__(MTH) void match_top2_kernel(const float *__restrict__ query, long ldq, int nq, const float *__restrict__ train, long ldt,
                                                         int nt, int r, const double *__restrict__ qnorm, const double *__restrict__ tnorm,
                                                         int tiles_per_slice, int32_t *__restrict__ idx, float *__restrict__ sqdist,
                                                         i32x4 *__restrict__ part, float *__restrict__ out, const MatchGuide g,
                                                         const match_batch::Entry *__restrict__ ent, int n_ent)
{
    unsigned qblk = blockIdx.x, slice = blockIdx.y;
    const double *grec = g.rec, *gqrec = g.qrec;           // GUIDED: the records and the coordinates the loop reads
    const float *gxy = g.xy;
    if constexpr (BATCH) {
        const int wg = (int)blockIdx.x;
        const int ei = batch_entry_of(ent, n_ent, wg, [](const match_batch::Entry &x) { return x.wg0; });
        const match_batch::Entry e = ent[ei];
        if constexpr (GUIDED != kPlain) bind_entry_guide<GUIDED>(g, e, ei, grec, gqrec, gxy);
        const unsigned w = (unsigned)(wg - e.wg0);
        slice = w / (unsigned)e.qblocks;
        qblk = w - slice * (unsigned)e.qblocks;
        train = query + e.t0 * ldq; ldt = ldq; tnorm = qnorm + e.t0;
        query += e.q0 * ldq; qnorm += e.q0;
        nq = e.nq; nt = e.nt; tiles_per_slice = e.tiles_per_slice;
        idx += 2 * e.out0; sqdist += 2 * e.out0;
        part = e.slices > 1 ? part + e.part0 : nullptr;
    }
    constexpr int CW = train_geom_width(GUIDED), QW = query_geom_width(GUIDED);
    __shared__ double Bs[TN * MP];                         // the staged tile, widened to double once, when it is stored
    __shared__ double Tn[TN];
    __shared__ __attribute__((aligned(16))) double Tg[GUIDED ? TN * CW : 1];            // GUIDED: the tile's geometry, staged with it,
    __shared__ __attribute__((aligned(16))) double Qg[GUIDED ? MQ * QW : 1];            // and the workgroup's queries': written once, before the loop
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int q0 = qblk * MQ + wave * 16;
    const bool wave_on = q0 < nq;                          // uniform over the wave
    const int jbeg = (int)((long)slice * tiles_per_slice * TN);    // this slice of train: [jbeg, jend), never empty (jbeg < nt)
    const int jend = (int)min((long)nt, (long)jbeg + (long)tiles_per_slice * TN);
    const int ntile = (jend - jbeg + TN - 1) / TN;
    const int nch = MULTI ? (r + KC - 1) / KC : 1;
    const int nstep = ntile * nch;
    const int r4 = (r + 3) & ~3;

    // the piece [k, k + 4) of a row with the elements at and beyond r zeroed
    auto mask_k = [&](f32x4 v, int k, bool row_ok) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; e++) o[e] = (row_ok && k + e < r) ? v[e] : 0.f;
        return o;
    };

    // loader: thread t fetches the 16-byte piece lseg of the train rows lrow + 16 u of a tile, and the first TN
    // threads the squared norm of one of its rows
    const int lrow = tid >> 5, lseg = tid & 31;
    f32x4 rb[NSUB];
    double rtn;
    double rg[CW];
    auto gload = [&](int step) {
        step = min(step, nstep - 1);                       // past the end: the last step again, never used
        const int tile = step / nch, kc = step - tile * nch;
        const int k = kc * KC + 4 * lseg;
        const int kk = k < r4 ? k : 0;
        const long jt = (long)jbeg + (long)tile * TN;      // nt may be just below 2^31
#pragma unroll
        for (int u = 0; u < NSUB; u++) {
            const long j = jt + lrow + 16 * u;
            const bool ok = j < jend;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(train + (ok ? j : (long)jbeg) * ldt + kk);
            rb[u] = mask_k(v, k, ok);
        }
        const long jn = jt + (tid & (TN - 1));
        const long js = jn < jend ? jn : (long)jbeg;
        rtn = tnorm[js];
        geom_fetch<GUIDED>(rg, grec, gxy, g.ldxy, js);
    };
    auto lstore = [&]() {
#pragma unroll
        for (int u = 0; u < NSUB; u++) {
            double *dst = &Bs[(lrow + 16 * u) * MP + 4 * lseg];
            *reinterpret_cast<f64x2 *>(dst) = f64x2{(double)rb[u][0], (double)rb[u][1]};
            *reinterpret_cast<f64x2 *>(dst + 2) = f64x2{(double)rb[u][2], (double)rb[u][3]};
        }
        if (tid < TN) {
            Tn[tid] = rtn;
            if constexpr (GUIDED != kPlain) geom_store(&Tg[tid * CW], rg);
        }
    };

    // A fragments of one k chunk: lane (li, lg) holds query q0 + li at k = 16 c + 4 lg + s, s = element of fa[c]
    const bool q_ok = q0 + li < nq;
    const float *qrow = query + (long)(q_ok ? q0 + li : 0) * ldq;
    f32x4 fa[KC / 16];
    auto aload = [&](int kc) {
#pragma unroll
        for (int c = 0; c < KC / 16; c++) {
            const int k = kc * KC + 16 * c + 4 * lg;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(qrow + (k < r4 ? k : 0));
            fa[c] = mask_k(v, k, q_ok);
        }
    };
    if (!MULTI) aload(0);

    // the lane's four result rows: query q0 + lg + 4 rr
    double qn[4];
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
        const int row = q0 + lg + 4 * rr;
        qn[rr] = qnorm[row < nq ? row : 0];
    }
    // GUIDED: the geometry of the workgroup's queries, a record or (x, y) (query_geom_fill), goes to LDS (the first
    // barrier of the loop below orders it) and is read again for every pair of column blocks: four rows' records held in
    // registers over the loop would put the kernel into scratch
    if constexpr (GUIDED != kPlain) {
        if (tid < MQ) {
            query_geom_fill<GUIDED>(&Qg[tid * QW], grec, gqrec, gxy, g.ldxy, (long)qblk * MQ + tid, nq);
        }
    }
    // GUIDED: which of the eight entries of the column blocks at c0 and c0 + 16 of the staged tile the rule admits, bit e as
    // prev_entry counts them.  One burst of LDS reads and fp64 VALU work per pair of blocks, whose only result that lives
    // on is the mask.  The empty asm hides from the compiler that the queries' address does not change over the tile loop:
    // hoisted out of it, their geometry would sit in registers again.
    auto admit_mask = [&](int c0) -> unsigned {
        unsigned m = 0xffu;
        if constexpr (GUIDED != kPlain) {
            int qoff = (wave * 16 + lg) * QW;
            asm volatile("" : "+v"(qoff));
            const Geom a = geom_read<CW>(&Tg[c0 * CW]), b = geom_read<CW>(&Tg[(c0 + 16) * CW]);
            m = 0;
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const Geom q = geom_read<QW>(&Qg[qoff + 4 * rr * QW]);
                m |= (admits<GUIDED>(q, a, g.t2) ? 1u : 0u) << rr;
                m |= (admits<GUIDED>(q, b, g.t2) ? 1u : 0u) << (4 + rr);
            }
        }
        return m;
    };
    // running (best, second) of the columns == li (mod 16) for each of the four rows; a lane meets its columns in
    // ascending order, so a strict comparison keeps the smaller index among equal distances
    const float inf = __builtin_inff();
    f32x4 bd1 = f32x4{inf, inf, inf, inf}, bd2 = bd1;
    i32x4 bj1 = i32x4{-1, -1, -1, -1}, bj2 = bj1;

    // one entry of a 16 x 16 result: row q0 + lg + 4 rr against train row jl, whose squared norm is tn
    auto entry = [&](double dot, int rr, double tn, long jl, unsigned mask, int e) {
        const bool j_ok = jl < jend;
        const bool adm = GUIDED == kPlain || ((mask >> e) & 1u) != 0;
        const int j = (int)jl;
        double d = __builtin_fma(-2.0, dot, qn[rr] + tn);
        d = __builtin_fmax(d, 0.0);
        const float f = (float)d;
        if (STORE) {
            const int row = q0 + lg + 4 * rr;
            if (j_ok && row < nq) out[(long)row * nt + j] = adm ? f : inf;
        } else {
            const bool in = j_ok && adm;
            const bool first = in && f < bd1[rr], second = in && f < bd2[rr];
            bd2[rr] = first ? bd1[rr] : (second ? f : bd2[rr]);
            bj2[rr] = first ? bj1[rr] : (second ? j : bj2[rr]);
            bd1[rr] = first ? f : bd1[rr];
            bj1[rr] = first ? j : bj1[rr];
        }
    };
    // The finished column blocks of the step before: their epilogue (VALU work) is issued between the MFMAs of the
    // next pair of blocks, one entry per 16-wide k group, so that it runs beside them instead of after them.
    f64x4 p0 = f64x4{0.0, 0.0, 0.0, 0.0}, p1 = p0;
    double ptn0 = 0.0, ptn1 = 0.0;
    unsigned pm = 0;
    long pj = jend;                                        // no block yet: jl >= jend masks every entry
    auto prev_entry = [&](int e) {
        if (e < 4) entry(p0[e], e, ptn0, pj, pm, e);
        else entry(p1[e - 4], e - 4, ptn1, pj + 16, pm, e);
    };
    // the k chunk in LDS against the A fragments, for the column blocks sub and sub + 1: two independent MFMA chains
    // over the nc 16-wide k groups that hold a k below r
    const int nc = MULTI ? KC / 16 : (r + 15) / 16;
    auto mfma_pair = [&](int sub, f64x4 &a0, f64x4 &a1, bool fused) {
        const double *b0 = &Bs[(16 * sub + li) * MP + 4 * lg];
#pragma unroll
        for (int c = 0; c < KC / 16; c++) {
            if (c < nc) {
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const f64x2 f0 = *reinterpret_cast<const f64x2 *>(b0 + 16 * c + 2 * h);
                    const f64x2 f1 = *reinterpret_cast<const f64x2 *>(b0 + 16 * MP + 16 * c + 2 * h);
#pragma unroll
                    for (int s = 0; s < 2; s++) {
                        a0 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)fa[c][2 * h + s], f0[s], a0, 0, 0, 0);
                        a1 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)fa[c][2 * h + s], f1[s], a1, 0, 0, 0);
                    }
                }
            }
            if (fused) prev_entry(c);
        }
    };
    const f64x4 zacc = f64x4{0.0, 0.0, 0.0, 0.0};
    f64x4 acc[MULTI ? NSUB : 2];

    gload(0);
    for (int step = 0; step < nstep; step++) {
        lstore();
        __syncthreads();
        gload(step + 1);
        if (wave_on) {
            if (MULTI) {
                const int tile = step / nch, kc = step - tile * nch;
                // the epipolar forms: the verdicts of the whole tile, a byte per pair of column blocks, before the chunk's A fragments
                // are fetched: between two chunks their registers are free, and 16 doubles of geometry fit without scratch
                unsigned mtile = 0;
                if constexpr (GUIDED >= kEpiQuerySrc) {
                    if (kc == nch - 1) {
#pragma unroll
                        for (int sub = 0; sub < NSUB; sub += 2) mtile |= admit_mask(16 * sub + li) << (4 * sub);
                    }
                    asm volatile("" : "+v"(mtile));           // formed here, not beside the epilogue below
                }
                aload(kc);
#pragma unroll
                for (int sub = 0; sub < NSUB; sub += 2) {
                    if (kc == 0) { acc[sub] = zacc; acc[sub + 1] = zacc; }
                    mfma_pair(sub, acc[sub], acc[sub + 1], false);
                    if (kc == nch - 1) {
                        const long jl = (long)jbeg + (long)tile * TN + 16 * sub + li;
                        const unsigned m = GUIDED >= kEpiQuerySrc ? (mtile >> (4 * sub)) & 0xffu : admit_mask(16 * sub + li);
#pragma unroll
                        for (int rr = 0; rr < 4; rr++) {
                            entry(acc[sub][rr], rr, Tn[16 * sub + li], jl, m, rr);
                            entry(acc[sub + 1][rr], rr, Tn[16 * sub + 16 + li], jl + 16, m, 4 + rr);
                        }
                    }
                }
            } else {
#pragma unroll 1
                for (int sub = 0; sub < NSUB; sub += 2) {
                    acc[0] = zacc; acc[1] = zacc;
                    mfma_pair(sub, acc[0], acc[1], true);
                    p0 = acc[0]; p1 = acc[1];
                    ptn0 = Tn[16 * sub + li]; ptn1 = Tn[16 * sub + 16 + li];
                    pm = admit_mask(16 * sub + li);
                    pj = (long)jbeg + (long)step * TN + 16 * sub + li;
                }
            }
        }
        __syncthreads();
    }
    if (!MULTI && wave_on) {
#pragma unroll
        for (int e = 0; e < 8; e++) prev_entry(e);         // the last pair of blocks
    }
    if (STORE || !wave_on) return;
    // the 16 lanes of a row hold disjoint columns: butterfly under the key, every lane ends with the row's top two
#pragma unroll
    for (int rr = 0; rr < 4; rr++) {
        Top2<float> me{bd1[rr], bj1[rr], bd2[rr], bj2[rr]};
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) me = merge2<FloatKey>(me, shfl_xor_top2(me, o));
        const int row = q0 + lg + 4 * rr;
        if (li == 0 && row < nq) {
            if (part) part[(long)slice * nq + row] = FloatKey::pack(me);
            else FloatKey::write(me, row, row, idx, sqdist);
        }
    }
}

// the rows of the pairs of a batch whose train image is empty: -1 and the line's "no candidate" distance (the bits of +inf
// or INT32_MAX) in both columns; one lane per row, which finds its fill by its number among all fill rows
__global__ __launch_bounds__(256) void match_fill_kernel(const match_batch::Fill *__restrict__ fill, int n_fill, long rows, int32_t none,
                                                         int32_t *__restrict__ idx, int32_t *__restrict__ sqdist)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    int lo = 0, hi = n_fill;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (fill[mid].first <= i) lo = mid; else hi = mid;
    }
    const long o = 2 * (fill[lo].out0 + (i - fill[lo].first));
    idx[o] = -1; idx[o + 1] = -1;
    sqdist[o] = none; sqdist[o + 1] = none;
}

// the records of n rows (x, y) = xy[i * ld], xy[i * ld + 1] under H: rec [n][4] = (X, Y, W, T), one lane per row
struct H9 { double h[9]; };
__global__ __launch_bounds__(256) void match_records_kernel(const float *__restrict__ xy, long ld, long n, const H9 H, double t2,
                                                            double *__restrict__ rec)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    store_record(rec + 4 * i, record_of<kRecHom>(H.h, (double)xy[i * ld], (double)xy[i * ld + 1], t2));
}

// the epipolar records of n rows (x, y) under F: rec [n][4] = the src record (l0, l1, l2, L) of a row of the image F applies to
// (dst_side 0) or the dst record (u, v, A, B) of a row of the other (dst_side 1), one lane per row
__global__ __launch_bounds__(256) void match_epi_records_kernel(const float *__restrict__ xy, long ld, long n, const H9 F, int dst_side,
                                                                double *__restrict__ rec)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = (double)xy[i * ld], y = (double)xy[i * ld + 1];
    store_record(rec + 4 * i, dst_side ? record_of<kRecDst>(F.h, x, y, 0.0) : record_of<kRecSrc>(F.h, x, y, 0.0));
}

// The records of one launch of a guided batch (match_batch.hpp): one lane per record row of the launch, which is also the
// row's place in rec.  The lane finds its entry by its row among the entries' first record rows, as match_fill_kernel finds
// its fill; rows below nqrec are the entry's queries, the others its train image.  M [n_pairs][9] holds every pair's
// matrix and xy the coordinates of the whole table.  EPI: the side F applies to (side 0: the queries) gets src records and
// the other dst records; else every row is on the side H applies to.
template <bool EPI>
__global__ __launch_bounds__(256) void match_records_batch_kernel(const float *__restrict__ xy, long ld, const match_batch::Entry *__restrict__ ent,
                                                                  const match_batch::GuideOff *__restrict__ off, int n_ent, long rows,
                                                                  const double *__restrict__ M, double t2, int side, double *__restrict__ rec)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    int lo = 0, hi = n_ent;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid].rec0 <= i) lo = mid; else hi = mid;
    }
    const long k = i - off[lo].rec0;
    const bool is_query = k < off[lo].nqrec;
    const long row = is_query ? ent[lo].q0 + k : ent[lo].t0 + (k - off[lo].nqrec);
    double h[9];
#pragma unroll
    for (int e = 0; e < 9; e++) h[e] = M[9 * (long)ent[lo].pair + e];
    const double x = (double)xy[row * ld], y = (double)xy[row * ld + 1];
    if constexpr (EPI) store_record(rec + 4 * i, is_query == (side == 0) ? record_of<kRecSrc>(h, x, y, t2) : record_of<kRecDst>(h, x, y, t2));
    else store_record(rec + 4 * i, record_of<kRecHom>(h, x, y, t2));
}

constexpr int NTH = 256;               // four rows per workgroup, one wave each

__global__ __launch_bounds__(NTH) void match_norms_kernel(const float *__restrict__ x, long ld, long n, int r, double *__restrict__ norm)
{
    const long row = (long)blockIdx.x * (NTH / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const float *p = x + row * ld;
    double s = 0.0;
    for (int k = lane; k < r; k += 64) s = __builtin_fma((double)p[k], (double)p[k], s);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) norm[row] = s;
}

}  // namespace

void match_norms(const float *x, long ld, long n, int r, double *norm, hipStream_t s)
{
    if (n <= 0) return;
    const long per = NTH / 64;
    hipLaunchKernelGGL(match_norms_kernel, dim3((unsigned)((n + per - 1) / per)), dim3(NTH), 0, s, x, ld, n, r, norm);
    DLCO_HIP(hipGetLastError());
}

void match_records(const float *xy, long ld, long n, const double H[9], double t2, double *rec, hipStream_t s)
{
    if (n <= 0) return;
    H9 h;
    for (int i = 0; i < 9; i++) h.h[i] = H[i];
    hipLaunchKernelGGL(match_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, xy, ld, n, h, t2, rec);
    DLCO_HIP(hipGetLastError());
}

void match_epi_records(const float *xy, long ld, long n, const double F[9], int dst_side, double *rec, hipStream_t s)
{
    if (n <= 0) return;
    H9 f;
    for (int i = 0; i < 9; i++) f.h[i] = F[i];
    hipLaunchKernelGGL(match_epi_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, xy, ld, n, f, dst_side, rec);
    DLCO_HIP(hipGetLastError());
}

// query [nq][ldq], train [nt][ldt], norms from match_norms.  out != nullptr: the matrix out[nq][nt]; else idx / sqdist
// [nq][2], through part [slices][nq] (16 bytes each) when the tiles_per_slice leaves more than one slice.  guide: nullptr, or
// the geometry of the guided form (dlco_internal.hpp).
void match_top2(const float *query, long ldq, int nq, const float *train, long ldt, int nt, int r, const double *qnorm, const double *tnorm,
                int tiles_per_slice, int32_t *idx, float *sqdist, void *part, float *out, const MatchGuide *guide, hipStream_t s)
{
    if (nq <= 0 || nt <= 0) return;
    const int slices = match_slicing::slices(match_slicing::kFloat, nt, tiles_per_slice);
    const dim3 grid((unsigned)((nq + MQ - 1) / MQ), (unsigned)slices);
    i32x4 *pp = (!out && slices > 1) ? static_cast<i32x4 *>(part) : nullptr;
    const MatchGuide g = guide ? *guide : MatchGuide{};
    dispatch_form(guided_form_of(guide), [&](auto form) {
        dispatch_bool(out != nullptr, [&](auto store) {
            dispatch_bool(r > KC, [&](auto multi) {
                hipLaunchKernelGGL((match_top2_kernel<store.value, multi.value, form.value>), grid, dim3(MTH), 0, s, query, ldq, nq, train, ldt, nt, r,
                                   qnorm, tnorm, tiles_per_slice, idx, sqdist, pp, out, g, nullptr, 0);
            });
        });
    });
    DLCO_HIP(hipGetLastError());
    if (pp) {
        hipLaunchKernelGGL((match_merge_kernel<FloatKey, false, int32_t, float>), dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, pp, slices, nq,
                           idx, sqdist);
        DLCO_HIP(hipGetLastError());
    }
}

// The records of one launch of a guided batch: rows record rows into rec, by the launch's entries and their record rows
void match_records_batch(const float *xy, long ldxy, const match_batch::Entry *ent, const match_batch::GuideOff *off, int n_ent, long rows,
                         const double *M, double t2, int side, int model, double *rec, hipStream_t s)
{
    if (n_ent <= 0 || rows <= 0) return;
    const dim3 grid((unsigned)((rows + 255) / 256));
    if (model == kGuideFundamental)
        hipLaunchKernelGGL(match_records_batch_kernel<true>, grid, dim3(256), 0, s, xy, ldxy, ent, off, n_ent, rows, M, t2, side, rec);
    else
        hipLaunchKernelGGL(match_records_batch_kernel<false>, grid, dim3(256), 0, s, xy, ldxy, ent, off, n_ent, rows, M, t2, side, rec);
    DLCO_HIP(hipGetLastError());
}

// One launch of a batched match (match_batch.hpp): table [.][ld] with its norms, the launch's n_ent entries in device memory,
// wgs workgroups of the tile loop, merge_wgs of the merge (0: every entry has one slice); idx / sqdist are the call's.
// guide: nullptr, or the geometry of the guided batch: rec the launch's record buffer, already written
// (match_records_batch), off its entries' record rows, xy / ldxy the coordinates of the whole table; ent_host / off_host
// are the same entries and record rows in host memory.
//   The homography with records on train (kHomTrain) has no batch form beyond r = 128: with the batch prologue its MULTI loop needs 10
// spilled registers.  Such a launch is served entry by entry with the single call's kernel on the entry's rows, norms,
// records, coordinates and partials, which returns the same bytes: the plan, the norms and the records are still the batch's.
void match_top2_batch(const float *table, long ld, int r, const double *norm, const match_batch::Entry *ent, int n_ent, long wgs, long merge_wgs,
                      int32_t *idx, float *sqdist, void *part, const MatchGuide *guide, const match_batch::Entry *ent_host,
                      const match_batch::GuideOff *off_host, hipStream_t s)
{
    if (n_ent <= 0 || wgs <= 0) return;
    i32x4 *pp = static_cast<i32x4 *>(part);
    const dim3 grid((unsigned)wgs);
    const MatchGuide g = guide ? *guide : MatchGuide{};
    if (guided_form_of(guide) == kHomTrain && r > KC) {
        for (int k = 0; k < n_ent; k++) {
            const match_batch::Entry &e = ent_host[k];
            MatchGuide ge = g;
            ge.rec = g.rec + 4 * (off_host[k].rec0 + off_host[k].nqrec);
            ge.xy = g.xy + e.q0 * g.ldxy;
            ge.off = nullptr;
            match_top2(table + e.q0 * ld, ld, e.nq, table + e.t0 * ld, ld, e.nt, r, norm + e.q0, norm + e.t0, e.tiles_per_slice, idx + 2 * e.out0,
                       sqdist + 2 * e.out0, pp + e.part0, nullptr, &ge, s);
        }
        return;
    }
    dispatch_form(guided_form_of(guide), [&](auto form) {
        dispatch_bool(r > KC, [&](auto multi) {
            if constexpr (!(form.value == kHomTrain && multi.value))   // served above: that form is not instantiated
                hipLaunchKernelGGL((match_top2_kernel<false, multi.value, form.value, true>), grid, dim3(MTH), 0, s, table, ld, 0, nullptr, 0L, 0, r,
                                   norm, nullptr, 0, idx, sqdist, pp, nullptr, g, ent, n_ent);
        });
    });
    DLCO_HIP(hipGetLastError());
    if (merge_wgs > 0) {
        hipLaunchKernelGGL((match_merge_kernel<FloatKey, true, int32_t, float>), dim3((unsigned)merge_wgs), dim3(256), 0, s, pp, ent, n_ent,
                           idx, sqdist);
        DLCO_HIP(hipGetLastError());
    }
}

// rows of pairs with an empty train image, either line: `none` is the bit pattern of the distance that means "no candidate"
void match_fill(const match_batch::Fill *fill, int n_fill, long rows, int32_t none, int32_t *idx, void *sqdist, hipStream_t s)
{
    if (n_fill <= 0 || rows <= 0) return;
    hipLaunchKernelGGL(match_fill_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, fill, n_fill, rows, none, idx,
                       static_cast<int32_t *>(sqdist));
    DLCO_HIP(hipGetLastError());
}

}  // namespace dlco
