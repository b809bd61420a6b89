// match_dev.hpp — what the two lines of the matcher share: the float line (kernels_match.hip, f64 matrix cores) and the byte
// line (kernels_match_u8.hip, int8 matrix cores) each own a tile loop (loaders, LDS layout, MFMA order, epilogue, running top
// two, mask layout) and their norms; everything that must agree between them is stated here, once:
//
//   GuidedForm, guided_form_of, dispatch_form   the five forms of a tile loop, the one place that reads MatchGuide's model and
//                         side for dispatch, and the runtime form as a template argument
//   batch_entry_of, bind_entry_guide   a batched workgroup (match_batch.hpp): its entry, and the entry's geometry
//   train_geom_width, query_geom_width, Geom, geom_fetch, geom_store, geom_read, query_geom_fill   which geometry a train row
//                         and a query bring per form, and how it moves: global -> registers -> LDS -> doubles
//   admits<FORM>          the verdict on a (query, train row) pair: the only caller of guided_rules::admits and
//                         guided_epipolar::admits in the matcher
//   Top2, merge2, shfl_xor_top2, match_merge_kernel<Line, BATCH>   the top two under a line's key, and the merge over slices
//   record_of, store_record   the record of a point under a matrix for a role, as the record kernels write it
//
// A helper is optimised on its own before it is inlined, so one that looks like the text it replaces can still change a
// kernel.  With these, every instantiation of the two tile loops has the instructions it had with its own copy, or (the
// kHomTrain forms beyond one chunk or in a batch) the same ones under other register names, and every other kernel is
// unchanged: tools/kernel_resources.py --compare; DESIGN.md, "Shared pieces of the two matcher lines", also lists what
// stayed in the kernels for that reason.
#pragma once

#include "dlco_internal.hpp"
#include "guided_rules.hpp"
#include "guided_epipolar_rules.hpp"
#include "match_batch.hpp"

namespace dlco {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// ---- the forms of a tile loop ---------------------------------------------------------------------------------------------
// The GUIDED template argument of both tile loops (an int, so a kernel's name does not depend on this header).  A record is
// 32 bytes, four doubles: guided_rules::Rec of a row of the side the homography applies to, or, under a fundamental matrix,
// guided_epipolar::SrcRec of a row of the image F applies to and DstRec of a row of the other.
enum GuidedForm : int {
    kPlain = 0,             // no predicate
    kHomQuery = 1,          // homography, side 0: the queries carry records, a train row brings its (x, y)
    kHomTrain = 2,          // homography, side 1: the train rows carry records, a query brings its (x, y)
    kEpiQuerySrc = 3,       // fundamental, side 0: both carry records, the queries are src
    kEpiTrainSrc = 4,       // fundamental, side 1: both carry records, train is src
};

inline GuidedForm guided_form_of(const MatchGuide *g)
{
    if (!g) return kPlain;
    if (g->model == kGuideHomography) return g->side == 0 ? kHomQuery : kHomTrain;
    return g->side == 0 ? kEpiQuerySrc : kEpiTrainSrc;
}

// Runtime form -> template argument, as dispatch_mt: calls f(std::integral_constant<int, form>); dispatch_bool likewise
template <int FORM = kEpiTrainSrc, typename F>
void dispatch_form(GuidedForm form, F &&f)
{
    if constexpr (FORM > kPlain) {
        if (form < FORM) return dispatch_form<FORM - 1>(form, f);
    }
    f(std::integral_constant<int, FORM>{});
}

template <typename F>
void dispatch_bool(bool b, F &&f)
{
    if (b) f(std::true_type{}); else f(std::false_type{});
}

// ---- the prologue of a batched workgroup ----------------------------------------------------------------------------------
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

// ---- geometry: shape and movement -----------------------------------------------------------------------------------------
// What a guided tile loop reads: rec, the records of the train rows (kHomQuery: of the queries); qrec, the queries' records of
// the epipolar forms; xy, the (x, y) floats of the side without records at a pitch of ldxy.  Single call: MatchGuide's own.
// The guided batch: g.rec is the launch's record buffer, g.off the record rows of every entry (indexed like ent) and g.xy the
// coordinates of the whole table; entry ei = e reads its own records, the queries' first and train's behind them, and the
// coordinates of the rows of the image that brings them.
template <int FORM>
__device__ __forceinline__ void bind_entry_guide(const MatchGuide &g, const match_batch::Entry &e, int ei, const double *&rec, const double *&qrec,
                                                 const float *&xy)
{
    const match_batch::GuideOff o = g.off[ei];
    const double *qr = g.rec + 4 * o.rec0, *tr = qr + 4 * (long)o.nqrec;
    rec = FORM == kHomQuery ? qr : tr;
    qrec = qr;
    xy = g.xy + (FORM == kHomQuery ? e.t0 : e.q0) * g.ldxy;
}

// doubles of geometry a train row brings, (x, y) or a record, and a query
constexpr int train_geom_width(int form) { return form >= kHomTrain ? 4 : 2; }
constexpr int query_geom_width(int form) { return form == kHomQuery || form >= kEpiQuerySrc ? 4 : 2; }

// the geometry of one row in registers: a record, or (x, y) in v[0], v[1]
struct Geom { double v[4]; };

// train row js of the slice -> registers, on its way to LDS beside the row's norm
template <int FORM>
__device__ __forceinline__ void geom_fetch(double (&rg)[train_geom_width(FORM)], const double *rec, const float *xy, long ldxy, long js)
{
    if constexpr (FORM == kHomQuery) {
        const float *p = xy + js * ldxy;
        rg[0] = (double)p[0]; rg[1] = (double)p[1];
    } else if constexpr (FORM != kPlain) {
        const f64x2 a = *reinterpret_cast<const f64x2 *>(rec + 4 * js), b = *reinterpret_cast<const f64x2 *>(rec + 4 * js + 2);
        rg[0] = a[0]; rg[1] = a[1]; rg[2] = b[0]; rg[3] = b[1];
    }
}

// W doubles of geometry, registers -> LDS and LDS -> registers, in 16-byte pieces
template <int W>
__device__ __forceinline__ void geom_store(double *dst, const double (&rg)[W])
{
#pragma unroll
    for (int e = 0; e < W; e += 2) *reinterpret_cast<f64x2 *>(dst + e) = f64x2{rg[e], rg[e + 1]};
}

template <int W>
__device__ __forceinline__ Geom geom_read(const double *src)
{
    Geom o{};
#pragma unroll
    for (int e = 0; e < W; e += 2) {
        const f64x2 t = *reinterpret_cast<const f64x2 *>(src + e);
        o.v[e] = t[0]; o.v[e + 1] = t[1];
    }
    return o;
}

// query `row` of the launch (at and beyond nq: query 0, never consulted) -> dst in LDS, once before the loop: its record
// (kHomQuery: from rec; epipolar: from qrec) or (x, y)
template <int FORM>
__device__ __forceinline__ void query_geom_fill(double *dst, const double *rec, const double *qrec, const float *xy, long ldxy, long row, int nq)
{
    const long rs = row < nq ? row : 0;
    if constexpr (query_geom_width(FORM) == 4) {
        const double *qr = FORM == kHomQuery ? rec : qrec;
        *reinterpret_cast<f64x2 *>(dst) = *reinterpret_cast<const f64x2 *>(qr + 4 * rs);
        *reinterpret_cast<f64x2 *>(dst + 2) = *reinterpret_cast<const f64x2 *>(qr + 4 * rs + 2);
    } else {
        const float *p = xy + rs * ldxy;
        *reinterpret_cast<f64x2 *>(dst) = f64x2{(double)p[0], (double)p[1]};
    }
}

// ---- the verdict ----------------------------------------------------------------------------------------------------------
// on a query and a train row, whichever of the two carries the record (homography) or is src (fundamental)
template <int FORM>
__device__ __forceinline__ bool admits(const Geom &q, const Geom &t, double t2)
{
    if constexpr (FORM == kHomQuery) return guided_rules::admits(guided_rules::Rec{q.v[0], q.v[1], q.v[2], q.v[3]}, t.v[0], t.v[1]);
    else if constexpr (FORM == kHomTrain) return guided_rules::admits(guided_rules::Rec{t.v[0], t.v[1], t.v[2], t.v[3]}, q.v[0], q.v[1]);
    else if constexpr (FORM == kEpiQuerySrc)
        return guided_epipolar::admits(guided_epipolar::SrcRec{q.v[0], q.v[1], q.v[2], q.v[3]},
                                       guided_epipolar::DstRec{t.v[0], t.v[1], t.v[2], t.v[3]}, t2);
    else if constexpr (FORM == kEpiTrainSrc)
        return guided_epipolar::admits(guided_epipolar::SrcRec{t.v[0], t.v[1], t.v[2], t.v[3]},
                                       guided_epipolar::DstRec{q.v[0], q.v[1], q.v[2], q.v[3]}, t2);
    else return true;
}

// ---- the top two under a key ----------------------------------------------------------------------------------------------
// A line (FloatKey, ByteKey: beside the tile loops) states its Key, which of two (key, index) candidates comes first
// (Line::first: a total order, equal keys by smaller index), how a 16-byte partial unpacks (Line::unpack) and how the top two
// of a query become a row of idx / sqdist (Line::write).
template <typename K> struct Top2 { K k1; int j1; K k2; int j2; };

// top two of the union of two top-two lists of disjoint candidates
template <typename Line, typename K = typename Line::Key>
__device__ __forceinline__ Top2<K> merge2(const Top2<K> a, const Top2<K> b)
{
    Top2<K> o;
    const bool b_first = Line::first(b.k1, b.j1, a.k1, a.j1);
    const K wk = b_first ? b.k1 : a.k1, lk = b_first ? a.k1 : b.k1;            // winner / loser of the two firsts
    const int wj = b_first ? b.j1 : a.j1, lj = b_first ? a.j1 : b.j1;
    const K sk = b_first ? b.k2 : a.k2;                                        // the winner's own second
    const int sj = b_first ? b.j2 : a.j2;
    const bool l_second = Line::first(lk, lj, sk, sj);
    o.k1 = wk; o.j1 = wj;
    o.k2 = l_second ? lk : sk;
    o.j2 = l_second ? lj : sj;
    return o;
}

// the top two of the lane o away, for a butterfly under the key
template <typename K>
__device__ __forceinline__ Top2<K> shfl_xor_top2(const Top2<K> me, int o)
{
    return Top2<K>{__shfl_xor(me.k1, o, 64), __shfl_xor(me.j1, o, 64), __shfl_xor(me.k2, o, 64), __shfl_xor(me.j2, o, 64)};
}

namespace {                             // instantiated per translation unit on purpose: every line instantiates its own, with its own Line

// The top two of a query over the slices of train, from part [slices][nq]: one lane per row.  The call's form takes
// (slices, nq); BATCH takes (ent, n_ent) in their place: 256 rows of an entry with more than one slice per workgroup, numbered
// from its mwg0, and part, slices, nq and the rows are the entry's.  out: what Line::write takes, the line's result arrays (with
// the queries' norms before them where a result needs them; BATCH: of the whole table).  Every instantiation has the argument
// list, and so the instructions, of the kernel it replaces.
template <typename Line, bool BATCH, typename... Out>
__global__ __launch_bounds__(256) void match_merge_kernel(const i32x4 *__restrict__ part, const typename std::conditional<BATCH, const match_batch::Entry *, int>::type a,
                                                          const int b, Out *__restrict__... out)
{
    int row = blockIdx.x * 256 + threadIdx.x, slices, nq;
    long q0 = 0, out0 = 0;                                 // the first of the rows among the norms and among the outputs
    if constexpr (BATCH) {
        const int wg = (int)blockIdx.x;
        const match_batch::Entry e = a[batch_entry_of(a, b, wg, [](const match_batch::Entry &x) { return x.mwg0; })];
        row = (wg - e.mwg0) * 256 + threadIdx.x;
        q0 = e.q0; out0 = e.out0;
        part += e.part0; slices = e.slices; nq = e.nq;
    } else {
        slices = a; nq = b;
    }
    if (row >= nq) return;
    Top2<typename Line::Key> me = Line::unpack(part[row]);
    for (int s = 1; s < slices; s++) me = merge2<Line>(me, Line::unpack(part[(long)s * nq + row]));
    Line::write(me, q0 + row, out0 + row, out...);
}

}  // namespace

// ---- records --------------------------------------------------------------------------------------------------------------
// The record of the point (x, y) under the matrix M to rec [4], by the point's role.  kRecHom: M is H, the point is on the side
// H applies to, the record is (X, Y, W, T) with t2.  M is F: kRecSrc, the point's image is the one F applies to, the record is
// (l0, l1, l2, L); kRecDst, it is the other image, the record is (u, v, A, B).  record_of forms it, store_record stores it; a kernel that learns
// the role at run time chooses between two record_of, in the order it always had, and stores once.
enum RecordRole : int { kRecHom, kRecSrc, kRecDst };

struct Rec4 { f64x2 lo, hi; };

template <int ROLE>
__device__ __forceinline__ Rec4 record_of(const double M[9], double x, double y, double t2)
{
    if constexpr (ROLE == kRecSrc) {
        const guided_epipolar::SrcRec s = guided_epipolar::src_record(M, x, y);
        return Rec4{f64x2{s.l0, s.l1}, f64x2{s.l2, s.L}};
    } else if constexpr (ROLE == kRecDst) {
        const guided_epipolar::DstRec d = guided_epipolar::dst_record(M, x, y);
        return Rec4{f64x2{d.u, d.v}, f64x2{d.A, d.B}};
    } else {
        const guided_rules::Rec r = guided_rules::record(M, x, y, t2);
        return Rec4{f64x2{r.X, r.Y}, f64x2{r.W, r.T}};
    }
}

__device__ __forceinline__ void store_record(double *rec, const Rec4 r)
{
    *reinterpret_cast<f64x2 *>(rec) = r.lo;
    *reinterpret_cast<f64x2 *>(rec + 2) = r.hi;
}

}  // namespace dlco
