// dlco_desc_api.cpp — C ABI of descriptor generation (comp-uprjdists): see the
// dlco_desc_* block of include/dlco.h.  Host orchestration and the filter selection of
// SelectPRFilters (src/misc.cpp:78-168, pure host logic); the patch transform, the pooling product and
// the pair differences run in HIP kernels (kernels_desc.hip), the projection by a learnt W and the distances
// of projected descriptors in kernels_describe.hip, the sampling of patches around keypoints in kernels_patch.hip, the
// quantisation of rows to bytes (quant_rules.hpp) and the match of byte tables in kernels_match_u8.hip, the detection of
// keypoints (detect_rules.hpp) in kernels_detect.hip, their orientation (orient_rules.hpp) in kernels_orient.hip, the
// verification of a match list against a homography (verify_rules.hpp) or a fundamental matrix (epipolar_rules.hpp) in
// kernels_verify.hip, the selection of matches from a batched answer (select_rules.hpp) in kernels_select.hip, the tracks
// across the verified matches of many pairs (track_rules.hpp) in kernels_tracks.hip.
// compute() serves every describe call: a PatchSource in, the rows a RowsOut names out.  The float and the byte matcher
// share one host path (match_host, match_device) over a FloatLine / ByteLine.
#include "../../include/dlco.h"

#include "dlco_internal.hpp"
#include "detect_rules.hpp"
#include "guided_rules.hpp"
#include "guided_epipolar_rules.hpp"
#include "orient_rules.hpp"
#include "patch_rules.hpp"
#include "quant_rules.hpp"
#include "verify_rules.hpp"
#include "epipolar_rules.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

using namespace dlco;

namespace {
constexpr int kPix = 64 * 64;
constexpr int kBins = 8;
constexpr int kChunk = 2048;            // patches per launch pair: 256 MB of PatchTrans
}

// The buffers of one matcher (FloatLine, ByteLine below): the uploaded tables of the host forms, the result of a chunk and
// the matrix, part [slices][nq] partial (d1, j1, d2, j2) of 16 bytes each, the norms of the queries and of train; for the
// guided forms of either line the uploaded (x, y) of both tables and rec [n][4], the records of the side the homography
// applies to (guided_rules.hpp): a launch's queries or all of train; for the epipolar guided forms (guided_epipolar_rules.hpp)
// rec holds train's records and qrec a launch's queries'; for the batch forms (dlco_desc_match_pairs*) plan, the uploaded
// entries of every launch and behind them the fill list (match_batch.hpp), train the one table and tnorm / qnorm its norms;
// for the guided batch forms (dlco_desc_match_pairs_guided*) plan holds the guide offsets and the pairs' matrices behind the
// fill list, txy the coordinates of the one table and rec the records of one launch
template <typename Elem, typename Dist, typename Norm>
struct MatchBufs {
    DevBuf<Elem> query, train;
    DevBuf<Dist> sqdist, cross;
    DevBuf<int32_t> idx, part;
    DevBuf<Norm> qnorm, tnorm;
    DevBuf<float> qxy, txy;
    DevBuf<double> rec, qrec;
    DevBuf<uint8_t> plan;
};

struct dlco_desc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    float sigma = 1.4f;
    bool norm = true;
    int ks = 13, qk = 1;
    float inv_step = 0.f, qgamma = 0.f;
    int nsel = 0, nsel_pad = 0;
    DevBuf<float> cf, filt, pt, desc_chunk;
    DevBuf<uint8_t> patches;
    // the learnt projection W [r, proj_F] (pj-learn's output) and the projected rows of one chunk
    int r = 0, proj_F = 0, proj_dim = 0;                   // proj_dim: rows of W with a non-zero entry (src/misc.cpp:269-277)
    DevBuf<float> W, y_chunk;
    // matching (dlco_desc_match*): buffers of their own, so that a match call leaves the scratch of the calls above alone
    int n_cu = 0;
    MatchBufs<float, float, double> m_float;
    // the quantiser of the _u8 forms of describe (quant_rules.hpp): scale, offsets [q_r] on the device; q_r == 0: none
    int q_r = 0;
    float q_scale = 1.f;
    DevBuf<float> q_off;
    DevBuf<uint8_t> u8_chunk;                              // the bytes of one chunk on their way to the host
    // matching byte tables (dlco_desc_match_u8*): again buffers of their own; part under the integer key, tnorm = -|a_t|^2
    MatchBufs<uint8_t, int32_t, int32_t> m_u8;
    // keypoint calls (dlco_desc_set_image* and after): the image, copied (img_own) or the caller's, and a chunk's frames
    const uint8_t *img = nullptr;
    int img_w = 0, img_h = 0;
    long img_pitch = 0;
    DevBuf<uint8_t> img_own;
    DevBuf<patch_rules::Frame> frames;
    // the detector (dlco_desc_detect*): the integral image of the image set (d_S_valid: it is that image's), the survivors of
    // the octaves and the scratch of their selection; d_cap survivors fit, and it only grows
    bool d_S_valid = false;
    DevBuf<uint32_t> d_S, d_seg, d_idx_a, d_idx_b, d_count;
    DevBuf<uint64_t> d_pos, d_key_a, d_key_b;
    DevBuf<int64_t> d_resp, d_resp_out;
    DevBuf<float> d_kp, d_kp_out;
    DevBuf<uint8_t> d_tmp;
    size_t d_cap = 0;
    double d_stage_ms[2 + detect_rules::kMaxOctaves] = {0};  // integral, the octaves, selection
    // orientation (dlco_desc_orient, dlco_desc_detect_oriented): uploaded keypoints, vectors and status of the last call
    DevBuf<float> o_kp;
    DevBuf<int64_t> o_vec;
    DevBuf<uint8_t> o_status;
    double o_ms = 0.0;
    // verification (dlco_desc_verify_*, either model; a single call is a launch of one entry): one launch of
    // verify_batch.hpp's plan, a slot per entry.  The uploaded matches, every hypothesis and its count, the selection key,
    // v_cur, the matrix the mask kernel scores per entry, the trial mask and its count, and v_plan, the uploaded entries and
    // behind them the active list; buffers of their own, like the matchers'.  The refit on the device (the _device forms,
    // verify_pairs_refit_round) adds a round's matrices v_try, its trial mask and count, and the entries' live flags
    DevBuf<float> v_src, v_dst;
    DevBuf<double> v_H, v_cur, v_try;
    DevBuf<int32_t> v_count, v_n, v_ntry;
    DevBuf<uint64_t> v_key;
    DevBuf<uint8_t> v_mask, v_plan, v_trial, v_live;
    // selecting matches (dlco_desc_select_pairs*, select_rules.hpp): the uploaded pairs, the kept rows as bits, the block
    // counts, their exclusive sums and the match offsets; for the host forms the uploaded answer, reverse table and
    // coordinates and the lists on their way down (distances of either line as 4-byte words); buffers of their own
    DevBuf<select_rules::Pair> s_pairs;
    DevBuf<uint64_t> s_word;
    DevBuf<int32_t> s_count, s_idx, s_sqdist, s_back, s_matches, s_dist;
    DevBuf<int64_t> s_off, s_moff;
    DevBuf<float> s_xy, s_src, s_dst;
    // building tracks (dlco_desc_build_tracks*, track_rules.hpp): the uploaded pairs and seg, the union-find's parent, the
    // labels when the caller wants none, the nodes and labels before and after the sort with its workspace, the components'
    // sizes and conflicts, the kept nodes and heads as bits, the block counts, their exclusive sums and the five totals; for the
    // host form the uploaded matches and mask and the outputs on their way down; buffers of their own
    DevBuf<track_rules::Pair> t_pairs;
    DevBuf<int64_t> t_seg, t_off, t_total, t_toff;
    DevBuf<int32_t> t_parent, t_label, t_node, t_slabel, t_snode, t_size, t_count, t_matches, t_obs, t_track_of;
    DevBuf<uint8_t> t_conf, t_tmp, t_keep;
    DevBuf<uint64_t> t_word;
    double last_ms = 0.0;
};

static thread_local std::string g_desc_error;

namespace {

template <typename Fn>
int guarded(dlco_desc_ctx *c, Fn &&fn)
{
    return guarded_call(g_desc_error, c ? &c->err : nullptr, fn);
}

void sync(dlco_desc_ctx *c) { DLCO_HIP(hipStreamSynchronize(c->stream)); }

struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventPair() { DLCO_HIP(hipEventCreate(&e0)); if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); throw Error(DLCO_ERR_HIP, "hipEventCreate failed"); } }
    ~EventPair() { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); }
};

// milliseconds the work that `run` queues on the stream takes there; `after` is queued behind it, outside the timing, and
// the stream has drained on return
template <typename Run, typename After>
float timed_ms(dlco_desc_ctx *c, const EventPair &ev, Run &&run, After &&after)
{
    DLCO_HIP(hipEventRecord(ev.e0, c->stream));
    run();
    DLCO_HIP(hipEventRecord(ev.e1, c->stream));
    after();
    sync(c);
    float ms = 0.f;
    DLCO_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    return ms;
}
template <typename Run>
float timed_ms(dlco_desc_ctx *c, const EventPair &ev, Run &&run) { return timed_ms(c, ev, run, [] {}); }

// Where the patches of a chunk come from: the caller's table on the host, copied up, or the frames of keypoints
// (patch_rules.hpp), for which the sampling kernel writes the chunk's patch buffer from the image in HBM.
struct PatchSource {
    const uint8_t *host = nullptr;                          // [n,64,64]
    const patch_rules::Frame *frames = nullptr;             // [n], on the host
    static PatchSource patches(const uint8_t *host) { PatchSource s; s.host = host; return s; }
    static PatchSource keypoints(const patch_rules::Frame *frames) { PatchSource s; s.frames = frames; return s; }
};

// What a compute call produces: the kind of rows, where they go (the caller's memory on the host or on the device) and
// their pitch in elements of the row type.
enum class Where { Host, Device };
struct RowsOut {
    enum Kind { Pooled, Projected, Bytes } kind;            // F floats; r floats, W * Desc; r bytes, those under the quantiser
    void *dst;
    Where where;
    long ld;
    static RowsOut pooled(float *dst, Where where, long ld) { return {Pooled, dst, where, ld}; }
    static RowsOut projected(float *dst, Where where, long ld) { return {Projected, dst, where, ld}; }
    static RowsOut bytes(uint8_t *dst, Where where, long ld) { return {Bytes, dst, where, ld}; }
};

// The copy that brings chunk [p0, p0 + cnt) of `src` to the device: the patches themselves into c->patches, or the frames
// that sample_chunk turns into them.
void upload_chunk(dlco_desc_ctx *c, const PatchSource &src, int64_t p0, int cnt)
{
    if (src.host)
        DLCO_HIP(hipMemcpyAsync(c->patches.p, src.host + p0 * kPix, (size_t)cnt * kPix, hipMemcpyHostToDevice, c->stream));
    else
        DLCO_HIP(hipMemcpyAsync(c->frames.p, src.frames + p0, (size_t)cnt * sizeof(patch_rules::Frame), hipMemcpyHostToDevice, c->stream));
}

// the sampling kernel on the uploaded frames of a chunk (frames_host: the same cnt frames): c->patches from c->img
void sample_chunk(dlco_desc_ctx *c, const patch_rules::Frame *frames_host, int cnt)
{
    patch_sample(c->img, c->img_w, c->img_h, c->img_pitch, c->frames.p, cnt, c->patches.p,
                 patch_stage_bytes(frames_host, cnt, c->img_w, c->img_h), c->stream);
}

// descriptors of n patches of `src`, as `o` says.  Projected rows are the learnt descriptor W * Desc: the un-projected rows
// of a chunk stay in the library's scratch buffer and the projection kernel follows the pooling product on the same
// stream.  The rows of invalid frames are zeroed behind the last kernel.
//   For bytes the float rows of a chunk stay in the scratch as well, and one elementwise kernel behind the zeroing turns
// them into bytes by the context's quantiser.
void compute(dlco_desc_ctx *c, const PatchSource &src, int64_t n, const RowsOut &o)
{
    const bool project = o.kind != RowsOut::Pooled, to_bytes = o.kind == RowsOut::Bytes, to_dev = o.where == Where::Device;
    const long ld = o.ld;
    DLCO_CHECK(c->nsel > 0, DLCO_ERR_INVALID, "dlco_desc: set the filters first");
    const int F = c->nsel * kBins;
    DLCO_CHECK(!project || (c->r > 0 && c->proj_F == F), DLCO_ERR_INVALID, "dlco_desc: set a projection that fits the filters first");
    const int cols = project ? c->r : F;                   // elements per output row
    DLCO_CHECK(!to_bytes || (c->q_r > 0 && c->q_r == c->r), DLCO_ERR_INVALID, "dlco_desc: set a quantiser that fits the projection first");
    DLCO_CHECK(ld >= cols, DLCO_ERR_INVALID, project ? "dlco_desc: row pitch below the projected size" : "dlco_desc: row pitch below the descriptor size");
    const bool direct = to_dev && !to_bytes;               // the kernels write the caller's float rows themselves
    float *dst = to_bytes ? nullptr : static_cast<float *>(o.dst);
    uint8_t *dst_u8 = to_bytes ? static_cast<uint8_t *>(o.dst) : nullptr;
    DLCO_HIP(hipSetDevice(c->device));
    c->patches.alloc((size_t)kChunk * kPix);
    c->pt.alloc((size_t)kChunk * kBins * kPix);
    if (src.frames) c->frames.alloc((size_t)kChunk);
    if (!direct || project) c->desc_chunk.alloc((size_t)kChunk * F);
    if (!direct && project) c->y_chunk.alloc((size_t)kChunk * cols);
    if (to_bytes && !to_dev) c->u8_chunk.alloc((size_t)kChunk * cols);
    EventPair ev;
    double ms_total = 0.0;
    for (int64_t p0 = 0; p0 < n; p0 += kChunk) {
        const int cnt = (int)std::min<int64_t>(kChunk, n - p0);
        upload_chunk(c, src, p0, cnt);
        float *out = direct ? dst + p0 * ld : (project ? c->y_chunk.p : c->desc_chunk.p);     // the float rows of the chunk
        const long old = direct ? ld : cols;
        ms_total += timed_ms(c, ev, [&] {
            if (src.frames) sample_chunk(c, src.frames + p0, cnt);
            desc_transform(c->patches.p, cnt, c->cf.p, c->ks, c->inv_step, c->norm, c->qk, c->qgamma, c->pt.p, c->stream);
            if (project) {
                desc_pool(c->pt.p, cnt, c->filt.p, c->nsel, c->nsel_pad, c->desc_chunk.p, F, c->stream);
                desc_project(c->desc_chunk.p, F, cnt, c->W.p, c->r, F, out, old, c->stream);
            } else {
                desc_pool(c->pt.p, cnt, c->filt.p, c->nsel, c->nsel_pad, out, old, c->stream);
            }
        }, [&] {
            for (int i = 0; src.frames && i < cnt; i++)
                if (!src.frames[p0 + i].valid) DLCO_HIP(hipMemsetAsync(out + (size_t)i * old, 0, (size_t)cols * sizeof(float), c->stream));
            if (!to_dev && !to_bytes)
                DLCO_HIP(hipMemcpy2DAsync(dst + p0 * ld, (size_t)ld * sizeof(float), out, (size_t)cols * sizeof(float),
                                          (size_t)cols * sizeof(float), (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
        });
        if (to_bytes) {
            uint8_t *bytes = to_dev ? dst_u8 + p0 * ld : c->u8_chunk.p;
            const long bld = to_dev ? ld : cols;
            ms_total += timed_ms(c, ev, [&] { desc_quantize_rows(out, old, cnt, cols, c->q_scale, c->q_off.p, bytes, bld, c->stream); }, [&] {
                if (!to_dev)
                    DLCO_HIP(hipMemcpy2DAsync(dst_u8 + p0 * ld, (size_t)ld, bytes, (size_t)cols, (size_t)cols, (size_t)cnt, hipMemcpyDeviceToHost,
                                              c->stream));
            });
        }
    }
    c->last_ms = ms_total;
}

// ---- matching: the two nearest rows of train for every row of query (kernels_match.hip, kernels_match_u8.hip) --------------
// One host path serves both matchers.  A line (FloatLine, ByteLine) says what differs: the types of an element, a distance
// and a norm, the Shape of the slicing rule, the context's buffers, the kernel wrappers, and the name in the "do not fit"
// message.  Both tile loops have the guided epilogue, so the guided forms (a Geometry, a PairsGeometry) are this path too.
struct FloatLine {
    using Elem = float; using Dist = float; using Norm = double;
    static constexpr match_slicing::Shape shape = match_slicing::kFloat;
    static constexpr const char *name = "dlco_desc_match";
    static MatchBufs<Elem, Dist, Norm> &bufs(dlco_desc_ctx *c) { return c->m_float; }
    static void query_norms(const Elem *x, long ld, long n, int r, Norm *norm, hipStream_t s) { match_norms(x, ld, n, r, norm, s); }
    static void train_norms(const Elem *x, long ld, long n, int r, Norm *norm, hipStream_t s) { match_norms(x, ld, n, r, norm, s); }
    static constexpr auto top2 = match_top2;
    // the batch forms: the norms of a whole table serve both sides; the bits of "no candidate" (+inf)
    static constexpr bool two_norms = false;
    static constexpr int32_t none = 0x7f800000;
    // guide: nullptr, or the geometry of a guided launch, with the launch's entries and record rows in host memory as well
    static void top2_batch(const Elem *table, long ld, int r, const Norm *, const Norm *tnorm, const match_batch::Entry *ent, int n_ent, long wgs,
                           long merge_wgs, int32_t *idx, Dist *sqdist, void *part, const MatchGuide *guide, const match_batch::Entry *ent_host,
                           const match_batch::GuideOff *off_host, hipStream_t s)
    {
        match_top2_batch(table, ld, r, tnorm, ent, n_ent, wgs, merge_wgs, idx, sqdist, part, guide, ent_host, off_host, s);
    }
};
struct ByteLine {
    using Elem = uint8_t; using Dist = int32_t; using Norm = int32_t;
    static constexpr match_slicing::Shape shape = match_slicing::kU8;
    static constexpr const char *name = "dlco_desc_match_u8";
    static MatchBufs<Elem, Dist, Norm> &bufs(dlco_desc_ctx *c) { return c->m_u8; }
    static void query_norms(const Elem *x, long ld, long n, int r, Norm *norm, hipStream_t s) { match_u8_norms(x, ld, n, r, false, norm, s); }
    // negated: the form the tile loop takes for train
    static void train_norms(const Elem *x, long ld, long n, int r, Norm *norm, hipStream_t s) { match_u8_norms(x, ld, n, r, true, norm, s); }
    static constexpr auto top2 = match_u8_top2;
    // the batch forms: a whole table's norms in both signs, a launch each; the bits of "no candidate" (INT32_MAX)
    static constexpr bool two_norms = true;
    static constexpr int32_t none = INT32_MAX;
    static void top2_batch(const Elem *table, long ld, int r, const Norm *qnorm, const Norm *tnorm, const match_batch::Entry *ent, int n_ent,
                           long wgs, long merge_wgs, int32_t *idx, Dist *sqdist, void *part, const MatchGuide *guide, const match_batch::Entry *,
                           const match_batch::GuideOff *, hipStream_t s)
    {
        match_u8_top2_batch(table, ld, r, qnorm, tnorm, ent, n_ent, wgs, merge_wgs, idx, sqdist, part, guide, s);
    }
};

// The geometry of a guided call (guided_rules.hpp), an optional argument of either line's host path: the (x, y) of the
// rows of both tables at pitches in floats (device memory in match_on_device and match_device, host memory with pitch 2 in
// match_host), the model (kGuideHomography: H, guided_rules.hpp; kGuideFundamental: F, guided_epipolar_rules.hpp), its nine
// entries, the squared radius or threshold and the side the model applies to.
struct Geometry {
    const float *qxy; long ldq;
    const float *txy; long ldt;
    const double *H;
    double t2;
    int side;
    int model;
};

constexpr int64_t kMatchRows = (int64_t)1 << 20;           // queries per launch (the kernels index a launch's queries with an int)
constexpr int64_t kRowPitchBytes = 16;                     // the host forms pad uploaded rows to this: the kernels fetch 16-byte pieces
constexpr int64_t kQueryChunkBytes = (int64_t)1 << 28;     // the host forms upload this much of padded query rows at a time

bool match_args_ok(const void *a, const void *b, const void *o1, const void *o2, int64_t nq, int64_t nt, int32_t r)
{
    return a && b && o1 && o2 && r >= 1 && r <= 1024 && nq >= 1 && nt >= 1 && nt < ((int64_t)1 << 31);
}

// device tables in, device results out; adds the kernels' time to *ms.  The line's tnorm holds train's norms already, and
// with a homography of side 1, or a fundamental matrix, its rec train's records (train_norms); geo's tables are device
// memory, and the queries' coordinates move with the rows.
template <typename L>
void match_on_device(dlco_desc_ctx *c, const typename L::Elem *q, long ldq, int64_t nq, const typename L::Elem *t, long ldt, int64_t nt, int r,
                     int32_t *idx, typename L::Dist *sqdist, typename L::Dist *cross, double *ms, const Geometry *geo = nullptr)
{
    auto &b = L::bufs(c);
    EventPair ev;
    for (int64_t q0 = 0; q0 < nq; q0 += kMatchRows) {
        const int cnt = (int)std::min(kMatchRows, nq - q0);
        const int tps = match_slicing::tiles_per_slice(L::shape, cnt, nt, c->n_cu), slices = match_slicing::slices(L::shape, nt, tps);
        b.qnorm.alloc((size_t)cnt);
        if (!cross && slices > 1) b.part.alloc((size_t)slices * cnt * 4);
        const bool epi = geo && geo->model == kGuideFundamental;
        const float *qxy0 = geo ? geo->qxy + q0 * geo->ldq : nullptr;       // the coordinates of the launch's first query
        MatchGuide guide;
        if (epi) {
            b.qrec.alloc((size_t)cnt * 4);
            guide.rec = b.rec.p; guide.qrec = b.qrec.p; guide.side = geo->side; guide.model = kGuideFundamental; guide.t2 = geo->t2;
        } else if (geo && geo->side == 0) {
            b.rec.alloc((size_t)cnt * 4);
            guide.rec = b.rec.p; guide.xy = geo->txy; guide.ldxy = geo->ldt; guide.side = 0;
        } else if (geo) {
            guide.rec = b.rec.p; guide.xy = qxy0; guide.ldxy = geo->ldq; guide.side = 1;
        }
        *ms += timed_ms(c, ev, [&] {
            L::query_norms(q + q0 * ldq, ldq, cnt, r, b.qnorm.p, c->stream);
            if (epi) match_epi_records(qxy0, geo->ldq, cnt, geo->H, geo->side == 0 ? 0 : 1, b.qrec.p, c->stream);   // side 0: the queries are src
            else if (geo && geo->side == 0) match_records(qxy0, geo->ldq, cnt, geo->H, geo->t2, b.rec.p, c->stream);
            L::top2(q + q0 * ldq, ldq, cnt, t, ldt, (int)nt, r, b.qnorm.p, b.tnorm.p, tps, idx ? idx + 2 * q0 : nullptr,
                    sqdist ? sqdist + 2 * q0 : nullptr, b.part.p, cross ? cross + q0 * nt : nullptr, geo ? &guide : nullptr, c->stream);
        });
    }
}

// train's norms, and train's records: with a homography of side 1, or a fundamental matrix (dst records when the queries are src)
template <typename L>
double train_norms(dlco_desc_ctx *c, const typename L::Elem *t, long ldt, int64_t nt, int r, const Geometry *geo = nullptr)
{
    auto &b = L::bufs(c);
    EventPair ev;
    b.tnorm.alloc((size_t)nt);
    const bool epi = geo && geo->model == kGuideFundamental;
    const bool records = geo && (epi || geo->side == 1);
    if (records) b.rec.alloc((size_t)nt * 4);
    return timed_ms(c, ev, [&] {
        L::train_norms(t, ldt, nt, r, b.tnorm.p, c->stream);
        if (epi) match_epi_records(geo->txy, geo->ldt, nt, geo->H, geo->side == 0 ? 1 : 0, b.rec.p, c->stream);
        else if (records) match_records(geo->txy, geo->ldt, nt, geo->H, geo->t2, b.rec.p, c->stream);
    });
}

// the device forms: both tables where the caller has them
template <typename L>
void match_device(dlco_desc_ctx *c, const typename L::Elem *query_dev, long ldq, int64_t nq, const typename L::Elem *train_dev, long ldt,
                  int64_t nt, int r, int32_t *idx_dev, typename L::Dist *sqdist_dev, const Geometry *geo = nullptr)
{
    DLCO_HIP(hipSetDevice(c->device));
    double ms = train_norms<L>(c, train_dev, ldt, nt, r, geo);
    match_on_device<L>(c, query_dev, ldq, nq, train_dev, ldt, nt, r, idx_dev, sqdist_dev, nullptr, &ms, geo);
    c->last_ms = ms;
}

// the host forms: train wholly in HBM, the queries a chunk at a time; cross_host: the matrix instead of the top two; geo:
// the guided form, its tables [n][2] on the host: train's go up with train, a chunk's queries' with the chunk
template <typename L>
void match_host(dlco_desc_ctx *c, const typename L::Elem *query_host, int64_t nq, const typename L::Elem *train_host, int64_t nt, int r,
                int32_t *idx_host, typename L::Dist *sqdist_host, typename L::Dist *cross_host, const Geometry *geo = nullptr)
{
    using Elem = typename L::Elem;
    using Dist = typename L::Dist;
    auto &b = L::bufs(c);
    DLCO_HIP(hipSetDevice(c->device));
    constexpr long per = kRowPitchBytes / sizeof(Elem);
    const long ld = (r + per - 1) / per * per;
    const int64_t qchunk = std::max<int64_t>(1, std::min<int64_t>(nq, kQueryChunkBytes / (ld * (int64_t)sizeof(Elem))));
    try {
        b.train.alloc((size_t)nt * ld);
        b.query.alloc((size_t)qchunk * ld);
        if (cross_host) b.cross.alloc((size_t)qchunk * nt);
        else { b.idx.alloc((size_t)qchunk * 2); b.sqdist.alloc((size_t)qchunk * 2); }
        if (geo) { b.txy.alloc((size_t)nt * 2); b.qxy.alloc((size_t)qchunk * 2); }
    } catch (const Error &e) {
        throw Error(DLCO_ERR_HIP, std::string(L::name) + ": the tables do not fit in device memory: " + e.what());
    }
    // rows of r elements on the host -> rows of pitch ld in dst
    auto upload_rows = [&](Elem *dst, const Elem *src_host, int64_t n) {
        DLCO_HIP(hipMemcpy2DAsync(dst, (size_t)ld * sizeof(Elem), src_host, (size_t)r * sizeof(Elem), (size_t)r * sizeof(Elem), (size_t)n,
                                  hipMemcpyHostToDevice, c->stream));
    };
    upload_rows(b.train.p, train_host, nt);
    Geometry dev_geo{};                                    // the same geometry on the uploaded tables
    if (geo) {
        dev_geo = Geometry{b.qxy.p, 2, b.txy.p, 2, geo->H, geo->t2, geo->side, geo->model};
        DLCO_HIP(hipMemcpyAsync(b.txy.p, geo->txy, (size_t)nt * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    const Geometry *dg = geo ? &dev_geo : nullptr;
    double ms = train_norms<L>(c, b.train.p, ld, nt, r, dg);
    for (int64_t q0 = 0; q0 < nq; q0 += qchunk) {
        const int64_t cnt = std::min(qchunk, nq - q0);
        upload_rows(b.query.p, query_host + q0 * r, cnt);
        if (geo) DLCO_HIP(hipMemcpyAsync(b.qxy.p, geo->qxy + 2 * q0, (size_t)cnt * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        if (cross_host) {
            match_on_device<L>(c, b.query.p, ld, cnt, b.train.p, ld, nt, r, nullptr, nullptr, b.cross.p, &ms, dg);
            DLCO_HIP(hipMemcpyAsync(cross_host + q0 * nt, b.cross.p, (size_t)cnt * nt * sizeof(Dist), hipMemcpyDeviceToHost, c->stream));
        } else {
            match_on_device<L>(c, b.query.p, ld, cnt, b.train.p, ld, nt, r, b.idx.p, b.sqdist.p, nullptr, &ms, dg);
            DLCO_HIP(hipMemcpyAsync(idx_host + 2 * q0, b.idx.p, (size_t)cnt * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            DLCO_HIP(hipMemcpyAsync(sqdist_host + 2 * q0, b.sqdist.p, (size_t)cnt * 2 * sizeof(Dist), hipMemcpyDeviceToHost, c->stream));
        }
        sync(c);
    }
    c->last_ms = ms;
}

// ---- the batch forms (dlco_desc_match_pairs*): many (query image, train image) pairs over one table whose segments are the
// images, by the plan of match_batch.hpp.  The same lines, buffers and norm kernels as above; what differs is that the
// norms of the table are formed once per call and that a launch carries the workgroups of many pairs. ------------------------
bool match_pairs_args_ok(const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs)
{
    if (!seg || !pairs || n_img < 1 || n_pairs < 1 || n_pairs >= ((int64_t)1 << 31) || seg[0] != 0) return false;
    for (int32_t i = 0; i < n_img; i++)
        if (seg[i + 1] < seg[i] || seg[i + 1] - seg[i] >= ((int64_t)1 << 31)) return false;
    if (seg[n_img] < 1) return false;
    for (int64_t p = 0; p < 2 * n_pairs; p++)
        if (pairs[p] < 0 || pairs[p] >= n_img) return false;
    return true;
}

// The geometry of a guided batch (dlco_desc_match_pairs_guided*), an optional argument of either line's batch path: xy, the
// coordinates of the rows of the one table in device memory at a pitch of ldxy floats, M [n_pairs][9] the pairs' matrices on
// the host, and the model, squared radius or threshold and side of every pair.
struct PairsGeometry {
    const float *xy; long ldxy;
    const double *M;
    double t2;
    int side;
    int model;
};

// the plan's Guide of a guided batch: none[p] is set for an all-zero matrix, "no model", which admits nothing
match_batch::Guide pairs_guide(const PairsGeometry &geo, int64_t n_pairs, std::vector<uint8_t> &none)
{
    none.assign((size_t)n_pairs, 0);
    for (int64_t p = 0; p < n_pairs; p++)
        none[(size_t)p] = std::all_of(geo.M + 9 * p, geo.M + 9 * p + 9, [](double v) { return v == 0.0; }) ? 1 : 0;
    match_batch::Guide g;
    g.no_model = none.data();
    g.both_sides = geo.model == kGuideFundamental;
    g.side = geo.side;
    return g;
}

// the table in device memory in, device results out: the norms of every row once, the fill rows, then the launches of the
// plan one after another (they share the partial buffer); returns the kernels' time.  geo: the guided form (pl was planned
// with pairs_guide): the guide offsets and the matrices go up behind the plan, and every launch forms its records first
template <typename L>
double match_pairs_on_device(dlco_desc_ctx *c, const typename L::Elem *table, long ld, const int64_t *seg, int32_t n_img,
                             const match_batch::Plan &pl, int r, int32_t *idx, typename L::Dist *sqdist, const PairsGeometry *geo = nullptr,
                             int64_t n_pairs = 0)
{
    auto &b = L::bufs(c);
    const int64_t n_rows = seg[n_img];
    const size_t ent_bytes = pl.entries.size() * sizeof(match_batch::Entry), fill_bytes = pl.fills.size() * sizeof(match_batch::Fill);
    const size_t off_bytes = geo ? pl.guide.size() * sizeof(match_batch::GuideOff) : 0, mat_bytes = geo ? (size_t)n_pairs * 9 * sizeof(double) : 0;
    b.tnorm.alloc((size_t)n_rows);
    if (L::two_norms) b.qnorm.alloc((size_t)n_rows);
    b.plan.alloc(ent_bytes + fill_bytes + off_bytes + mat_bytes);
    if (pl.max_parts > 0) b.part.alloc((size_t)pl.max_parts * 4);
    if (geo && pl.max_rec_rows > 0) b.rec.alloc((size_t)pl.max_rec_rows * 4);
    if (ent_bytes) DLCO_HIP(hipMemcpyAsync(b.plan.p, pl.entries.data(), ent_bytes, hipMemcpyHostToDevice, c->stream));
    if (fill_bytes) DLCO_HIP(hipMemcpyAsync(b.plan.p + ent_bytes, pl.fills.data(), fill_bytes, hipMemcpyHostToDevice, c->stream));
    if (off_bytes) DLCO_HIP(hipMemcpyAsync(b.plan.p + ent_bytes + fill_bytes, pl.guide.data(), off_bytes, hipMemcpyHostToDevice, c->stream));
    if (mat_bytes) DLCO_HIP(hipMemcpyAsync(b.plan.p + ent_bytes + fill_bytes + off_bytes, geo->M, mat_bytes, hipMemcpyHostToDevice, c->stream));
    const auto *ent = reinterpret_cast<const match_batch::Entry *>(b.plan.p);
    const auto *fill = reinterpret_cast<const match_batch::Fill *>(b.plan.p + ent_bytes);
    const auto *off = reinterpret_cast<const match_batch::GuideOff *>(b.plan.p + ent_bytes + fill_bytes);
    const auto *mat = reinterpret_cast<const double *>(b.plan.p + ent_bytes + fill_bytes + off_bytes);
    EventPair ev;
    return timed_ms(c, ev, [&] {
        L::train_norms(table, ld, n_rows, r, b.tnorm.p, c->stream);
        if (L::two_norms) L::query_norms(table, ld, n_rows, r, b.qnorm.p, c->stream);
        match_fill(fill, (int)pl.fills.size(), pl.fill_rows, L::none, idx, sqdist, c->stream);
        for (const match_batch::Launch &la : pl.launches) {
            MatchGuide g;
            if (geo) {
                g.rec = b.rec.p; g.xy = geo->xy; g.ldxy = geo->ldxy; g.side = geo->side; g.model = geo->model; g.t2 = geo->t2;
                g.off = off + la.e0;
                match_records_batch(geo->xy, geo->ldxy, ent + la.e0, off + la.e0, (int)la.n, la.rec_rows, mat, geo->t2, geo->side, geo->model,
                                    b.rec.p, c->stream);
            }
            L::top2_batch(table, ld, r, b.qnorm.p, b.tnorm.p, ent + la.e0, (int)la.n, la.wgs, la.merge_wgs, idx, sqdist, b.part.p,
                          geo ? &g : nullptr, pl.entries.data() + la.e0, geo ? pl.guide.data() + la.e0 : nullptr, c->stream);
        }
    });
}

// geo: the guided form, its xy in device memory
template <typename L>
void match_pairs_device(dlco_desc_ctx *c, const typename L::Elem *table_dev, long ld, const int64_t *seg, int32_t n_img, const int32_t *pairs,
                        int64_t n_pairs, int r, int32_t *idx_dev, typename L::Dist *sqdist_dev, const PairsGeometry *geo = nullptr)
{
    DLCO_HIP(hipSetDevice(c->device));
    std::vector<uint8_t> none;
    match_batch::Guide guide;
    if (geo) guide = pairs_guide(*geo, n_pairs, none);
    const match_batch::Plan pl = match_batch::plan(L::shape, seg, pairs, n_pairs, c->n_cu, geo ? &guide : nullptr);
    c->last_ms = match_pairs_on_device<L>(c, table_dev, ld, seg, n_img, pl, r, idx_dev, sqdist_dev, geo, n_pairs);
}

// the host form: the table goes up once, padded to the 16-byte row pitch, the outputs of every pair come down once; geo: the
// guided form, its xy [n_rows][2] on the host, which goes up with the table
template <typename L>
void match_pairs_host(dlco_desc_ctx *c, const typename L::Elem *table_host, const int64_t *seg, int32_t n_img, const int32_t *pairs,
                      int64_t n_pairs, int r, int32_t *idx_host, typename L::Dist *sqdist_host, const PairsGeometry *geo = nullptr)
{
    using Elem = typename L::Elem;
    using Dist = typename L::Dist;
    auto &b = L::bufs(c);
    DLCO_HIP(hipSetDevice(c->device));
    constexpr long per = kRowPitchBytes / sizeof(Elem);
    const long ld = (r + per - 1) / per * per;
    const int64_t n_rows = seg[n_img];
    std::vector<uint8_t> none;
    match_batch::Guide guide;
    if (geo) guide = pairs_guide(*geo, n_pairs, none);
    const match_batch::Plan pl = match_batch::plan(L::shape, seg, pairs, n_pairs, c->n_cu, geo ? &guide : nullptr);
    const int64_t out_rows = pl.row0[(size_t)n_pairs];
    try {
        b.train.alloc((size_t)n_rows * ld);
        b.idx.alloc((size_t)out_rows * 2);
        b.sqdist.alloc((size_t)out_rows * 2);
        if (geo) b.txy.alloc((size_t)n_rows * 2);
    } catch (const Error &e) {
        throw Error(DLCO_ERR_HIP, std::string(L::name) + "_pairs: the table and the results do not fit in device memory: " + e.what());
    }
    DLCO_HIP(hipMemcpy2DAsync(b.train.p, (size_t)ld * sizeof(Elem), table_host, (size_t)r * sizeof(Elem), (size_t)r * sizeof(Elem), (size_t)n_rows,
                              hipMemcpyHostToDevice, c->stream));
    PairsGeometry dev_geo{};                               // the same geometry on the uploaded coordinates
    if (geo) {
        dev_geo = PairsGeometry{b.txy.p, 2, geo->M, geo->t2, geo->side, geo->model};
        DLCO_HIP(hipMemcpyAsync(b.txy.p, geo->xy, (size_t)n_rows * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    c->last_ms = match_pairs_on_device<L>(c, b.train.p, ld, seg, n_img, pl, r, b.idx.p, b.sqdist.p, geo ? &dev_geo : nullptr, n_pairs);
    if (out_rows > 0) {
        DLCO_HIP(hipMemcpyAsync(idx_host, b.idx.p, (size_t)out_rows * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        DLCO_HIP(hipMemcpyAsync(sqdist_host, b.sqdist.p, (size_t)out_rows * 2 * sizeof(Dist), hipMemcpyDeviceToHost, c->stream));
    }
    sync(c);
}

// ---- selecting matches (dlco_desc_select_pairs*): from the answer of a match_pairs call to the segmented match list of a
// verify_pairs call, by the rule of select_rules.hpp in kernels_select.hip.  One path over the distance type of the two lines;
// the host forms are the device path between an upload and a download -----------------------------------------------------------
struct SelectArgs {
    const int64_t *seg; int32_t n_img;
    const int32_t *pairs; int64_t n_pairs;
    float ratio;
    const int64_t *back_row0; int64_t n_back_rows;
    int64_t *moff;
};

// xy: ldxy is looked at only with a coordinate table
bool select_args_ok(const SelectArgs &a, const void *idx, const void *sqdist, const void *back, const void *xy, int64_t ldxy, const void *matches,
                    const void *dist, const void *src, const void *dst)
{
    if (!idx || !sqdist || !a.moff || !matches || !dist || !match_pairs_args_ok(a.seg, a.n_img, a.pairs, a.n_pairs)) return false;
    if (!select_rules::ratio_ok(a.ratio)) return false;
    if (back && !select_rules::back_rows_ok(a.seg, a.pairs, a.n_pairs, a.back_row0, a.n_back_rows)) return false;
    if (xy ? (!src || !dst || ldxy < 2) : (src || dst)) return false;
    int64_t rows = 0;                                      // fewer than 2^31 pairs of fewer than 2^31 rows each: no overflow
    for (int64_t p = 0; p < a.n_pairs; p++) rows += a.seg[a.pairs[2 * p] + 1] - a.seg[a.pairs[2 * p]];
    return rows < ((int64_t)1 << 31);
}

// every table in device memory, moff on the host: the kernels, timed, and the download of the offsets behind them
template <typename Dist>
void select_on_device(dlco_desc_ctx *c, const std::vector<select_rules::Pair> &rec, int64_t R, const int32_t *idx, const Dist *sqdist, float f,
                      const int32_t *back, const float *xy, int64_t ldxy, int64_t *moff, int32_t *matches, Dist *dist, float *src, float *dst)
{
    const int64_t P = (int64_t)rec.size();
    if (R == 0) {                                          // every query image is empty: no row, no match, nothing to launch
        std::fill(moff, moff + P + 1, (int64_t)0);
        c->last_ms = 0.0;
        return;
    }
    const int64_t nb = select_rules::blocks(R);
    c->s_pairs.alloc((size_t)P);
    c->s_word.alloc((size_t)nb * (select_rules::kBlockRows / 64));
    c->s_count.alloc((size_t)nb);
    c->s_off.alloc((size_t)nb + 1);
    c->s_moff.alloc((size_t)P + 1);
    DLCO_HIP(hipMemcpyAsync(c->s_pairs.p, rec.data(), (size_t)P * sizeof(select_rules::Pair), hipMemcpyHostToDevice, c->stream));
    EventPair ev;
    c->last_ms = timed_ms(c, ev, [&] {
        select_flag(c->s_pairs.p, P, R, idx, sqdist, f, back, c->s_word.p, c->s_count.p, c->stream);
        select_scan(c->s_count.p, nb, c->s_off.p, c->stream);
        select_scatter(c->s_pairs.p, P, R, idx, sqdist, c->s_word.p, c->s_off.p, xy, ldxy, matches, dist, src, dst, c->stream);
        select_offsets(c->s_pairs.p, P, R, c->s_word.p, c->s_off.p, c->s_moff.p, c->stream);
    }, [&] { DLCO_HIP(hipMemcpyAsync(moff, c->s_moff.p, (size_t)(P + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream)); });
}

template <typename Dist>
int select_pairs_device_call(dlco_desc_ctx *c, const SelectArgs &a, const int32_t *idx_dev, const Dist *sqdist_dev, const int32_t *back_dev,
                             const float *xy_dev, int64_t ldxy, int32_t *matches_dev, Dist *dist_dev, float *src_dev, float *dst_dev)
{
    if (!c || !select_args_ok(a, idx_dev, sqdist_dev, back_dev, xy_dev, ldxy, matches_dev, dist_dev, src_dev, dst_dev)) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_HIP(hipSetDevice(c->device));
        std::vector<select_rules::Pair> rec;
        const int64_t R = select_rules::pair_records(a.seg, a.pairs, a.n_pairs, back_dev ? a.back_row0 : nullptr, rec);
        select_on_device<Dist>(c, rec, R, idx_dev, sqdist_dev, a.ratio, back_dev, xy_dev, ldxy, a.moff, matches_dev, dist_dev, src_dev, dst_dev);
    });
}

// the host form: the answer, the reverse table (unless it is the answer itself) and the coordinates go up once, the first
// M entries of the lists come down
template <typename Dist>
int select_pairs_host_call(dlco_desc_ctx *c, const SelectArgs &a, const int32_t *idx_host, const Dist *sqdist_host, const int32_t *back_host,
                           const float *xy_host, int32_t *matches_host, Dist *dist_host, float *src_host, float *dst_host)
{
    static_assert(sizeof(Dist) == sizeof(int32_t), "distances travel as 4-byte words");
    if (!c || !select_args_ok(a, idx_host, sqdist_host, back_host, xy_host, 2, matches_host, dist_host, src_host, dst_host)) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_HIP(hipSetDevice(c->device));
        std::vector<select_rules::Pair> rec;
        const int64_t R = select_rules::pair_records(a.seg, a.pairs, a.n_pairs, back_host ? a.back_row0 : nullptr, rec);
        const int64_t n_rows = a.seg[a.n_img];
        const bool back_is_idx = back_host == idx_host && a.n_back_rows <= R;
        if (R > 0) {
            try {
                c->s_idx.alloc((size_t)R * 2);
                c->s_sqdist.alloc((size_t)R * 2);
                c->s_matches.alloc((size_t)R * 2);
                c->s_dist.alloc((size_t)R);
                if (back_host && !back_is_idx) c->s_back.alloc((size_t)a.n_back_rows * 2);
                if (xy_host) { c->s_xy.alloc((size_t)n_rows * 2); c->s_src.alloc((size_t)R * 2); c->s_dst.alloc((size_t)R * 2); }
            } catch (const Error &e) {
                throw Error(DLCO_ERR_HIP, std::string("dlco_desc_select_pairs: the tables and the lists do not fit in device memory: ") + e.what());
            }
            DLCO_HIP(hipMemcpyAsync(c->s_idx.p, idx_host, (size_t)R * 2 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            DLCO_HIP(hipMemcpyAsync(c->s_sqdist.p, sqdist_host, (size_t)R * 2 * sizeof(Dist), hipMemcpyHostToDevice, c->stream));
            if (back_host && !back_is_idx && a.n_back_rows > 0)
                DLCO_HIP(hipMemcpyAsync(c->s_back.p, back_host, (size_t)a.n_back_rows * 2 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            if (xy_host) DLCO_HIP(hipMemcpyAsync(c->s_xy.p, xy_host, (size_t)n_rows * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        }
        const int32_t *back_dev = !back_host ? nullptr : back_is_idx ? c->s_idx.p : c->s_back.p;
        Dist *dist_dev = reinterpret_cast<Dist *>(c->s_dist.p);
        select_on_device<Dist>(c, rec, R, c->s_idx.p, reinterpret_cast<const Dist *>(c->s_sqdist.p), a.ratio, back_dev, xy_host ? c->s_xy.p : nullptr, 2,
                               a.moff, c->s_matches.p, dist_dev, c->s_src.p, c->s_dst.p);
        const int64_t M = a.moff[a.n_pairs];
        if (M > 0) {
            DLCO_HIP(hipMemcpyAsync(matches_host, c->s_matches.p, (size_t)M * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            DLCO_HIP(hipMemcpyAsync(dist_host, dist_dev, (size_t)M * sizeof(Dist), hipMemcpyDeviceToHost, c->stream));
            if (xy_host) {
                DLCO_HIP(hipMemcpyAsync(src_host, c->s_src.p, (size_t)M * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
                DLCO_HIP(hipMemcpyAsync(dst_host, c->s_dst.p, (size_t)M * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
            }
            sync(c);
        }
    });
}

// ---- building tracks (dlco_desc_build_tracks*): from the match lists and masks of many pairs to the tracks across all images,
// by the rule of track_rules.hpp in kernels_tracks.hip.  The host form is the device path between an upload and a download ---
struct TracksArgs {
    const int64_t *seg; int32_t n_img;
    const int32_t *pairs; int64_t n_pairs;
    const int64_t *moff;
    int32_t min_len, unique;
    int64_t *n_tracks, *counts;
};

// seg / pairs as dlco_desc_match_pairs checks them, except that a table of no rows is a batch like another here
bool tracks_args_ok(const TracksArgs &a, const void *matches, const void *toff, const void *obs, const void *track_of)
{
    if (!a.seg || !a.pairs || !a.moff || !matches || !a.n_tracks || !a.counts || !toff || !obs || !track_of) return false;
    if (a.n_img >= 1 && a.seg[0] == 0 && a.seg[a.n_img] == 0) {
        for (int32_t i = 0; i < a.n_img; i++)
            if (a.seg[i + 1] != 0) return false;
        if (a.n_pairs < 1 || a.n_pairs >= ((int64_t)1 << 31)) return false;
        for (int64_t p = 0; p < 2 * a.n_pairs; p++)
            if (a.pairs[p] < 0 || a.pairs[p] >= a.n_img) return false;
    } else if (!match_pairs_args_ok(a.seg, a.n_img, a.pairs, a.n_pairs)) {
        return false;
    }
    return a.seg[a.n_img] < ((int64_t)1 << 31) && track_rules::moff_ok(a.moff, a.n_pairs) && track_rules::settings_ok(a.min_len, a.unique);
}

// every list in device memory: the kernels, timed, and the download of the five totals behind them
void tracks_on_device(dlco_desc_ctx *c, const TracksArgs &a, const int32_t *matches, const uint8_t *keep, int64_t *toff, int32_t *obs,
                      int32_t *track_of, int32_t *label)
{
    const int64_t N = a.seg[a.n_img], M = a.moff[a.n_pairs], P = a.n_pairs;
    if (N == 0) {                                          // no node: no track, nothing to launch
        DLCO_HIP(hipMemsetAsync(toff, 0, sizeof(int64_t), c->stream));
        sync(c);
        *a.n_tracks = 0;
        a.counts[0] = a.counts[1] = a.counts[2] = 0;
        c->last_ms = 0.0;
        return;
    }
    std::vector<track_rules::Pair> rec;
    track_rules::pair_records(a.seg, a.pairs, P, a.moff, rec);
    const int64_t nb = track_rules::blocks(N);
    const size_t tmp_bytes = tracks_sort_bytes(N);
    c->t_pairs.alloc((size_t)P);
    c->t_seg.alloc((size_t)a.n_img + 1);
    c->t_parent.alloc((size_t)N);
    if (!label) { c->t_label.alloc((size_t)N); label = c->t_label.p; }
    c->t_node.alloc((size_t)N);
    c->t_slabel.alloc((size_t)N);
    c->t_snode.alloc((size_t)N);
    c->t_size.alloc((size_t)N);
    c->t_conf.alloc((size_t)N);
    c->t_tmp.alloc(std::max<size_t>(tmp_bytes, 1));
    c->t_word.alloc((size_t)nb * 2 * (track_rules::kBlockNodes / 64));
    c->t_count.alloc((size_t)nb * track_rules::kCounted);
    c->t_off.alloc((size_t)(nb + 1) * track_rules::kCounted);
    c->t_total.alloc(track_rules::kCounted);
    DLCO_HIP(hipMemcpyAsync(c->t_pairs.p, rec.data(), (size_t)P * sizeof(track_rules::Pair), hipMemcpyHostToDevice, c->stream));
    DLCO_HIP(hipMemcpyAsync(c->t_seg.p, a.seg, ((size_t)a.n_img + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    int64_t total[track_rules::kCounted] = {0, 0, 0, 0, 0};
    EventPair ev;
    c->last_ms = timed_ms(c, ev, [&] {
        tracks_labels(c->t_pairs.p, P, N, M, matches, keep, c->t_parent.p, c->t_node.p, c->t_conf.p, label, c->stream);
        tracks_group(N, label, c->t_node.p, c->t_seg.p, a.n_img, a.min_len, a.unique, c->t_slabel.p, c->t_snode.p, c->t_size.p, c->t_conf.p, c->t_tmp.p,
                     tmp_bytes, c->t_word.p, c->t_count.p, c->t_off.p, c->t_total.p, toff, obs, track_of, c->stream);
    }, [&] { DLCO_HIP(hipMemcpyAsync(total, c->t_total.p, sizeof(total), hipMemcpyDeviceToHost, c->stream)); });
    *a.n_tracks = total[1];
    a.counts[0] = total[2];
    a.counts[1] = total[3];
    a.counts[2] = total[4];
}

int build_tracks_device_call(dlco_desc_ctx *c, const TracksArgs &a, const int32_t *matches_dev, const uint8_t *keep_dev, int64_t *toff_dev,
                             int32_t *obs_dev, int32_t *track_of_dev, int32_t *label_dev)
{
    if (!c || !tracks_args_ok(a, matches_dev, toff_dev, obs_dev, track_of_dev)) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_HIP(hipSetDevice(c->device));
        tracks_on_device(c, a, matches_dev, keep_dev, toff_dev, obs_dev, track_of_dev, label_dev);
    });
}

// the host form: matches and mask go up once; toff [n_tracks + 1], the observations, track_of and label come down
int build_tracks_host_call(dlco_desc_ctx *c, const TracksArgs &a, const int32_t *matches_host, const uint8_t *keep_host, int64_t *toff_host,
                           int32_t *obs_host, int32_t *track_of_host, int32_t *label_host)
{
    if (!c || !tracks_args_ok(a, matches_host, toff_host, obs_host, track_of_host)) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_HIP(hipSetDevice(c->device));
        const int64_t N = a.seg[a.n_img], M = a.moff[a.n_pairs];
        if (N == 0) {
            *a.n_tracks = 0;
            a.counts[0] = a.counts[1] = a.counts[2] = 0;
            toff_host[0] = 0;
            c->last_ms = 0.0;
            return;
        }
        try {
            c->t_matches.alloc((size_t)std::max<int64_t>(M, 1) * 2);
            if (keep_host) c->t_keep.alloc((size_t)std::max<int64_t>(M, 1));
            c->t_toff.alloc((size_t)N / 2 + 1);
            c->t_obs.alloc((size_t)N);
            c->t_track_of.alloc((size_t)N);
            if (label_host) c->t_label.alloc((size_t)N);
        } catch (const Error &e) {
            throw Error(DLCO_ERR_HIP, std::string("dlco_desc_build_tracks: the lists do not fit in device memory: ") + e.what());
        }
        if (M > 0) {
            DLCO_HIP(hipMemcpyAsync(c->t_matches.p, matches_host, (size_t)M * 2 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            if (keep_host) DLCO_HIP(hipMemcpyAsync(c->t_keep.p, keep_host, (size_t)M, hipMemcpyHostToDevice, c->stream));
        }
        tracks_on_device(c, a, c->t_matches.p, keep_host ? c->t_keep.p : nullptr, c->t_toff.p, c->t_obs.p, c->t_track_of.p, label_host ? c->t_label.p : nullptr);
        const int64_t T = *a.n_tracks;
        DLCO_HIP(hipMemcpyAsync(toff_host, c->t_toff.p, (size_t)(T + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        DLCO_HIP(hipMemcpyAsync(track_of_host, c->t_track_of.p, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (label_host) DLCO_HIP(hipMemcpyAsync(label_host, c->t_label.p, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        sync(c);
        if (toff_host[T] > 0) {
            DLCO_HIP(hipMemcpyAsync(obs_host, c->t_obs.p, (size_t)toff_host[T] * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            sync(c);
        }
    });
}

// ---- verification: a homography (verify_rules.hpp) or a fundamental matrix (epipolar_rules.hpp) between the two sides of
// a match list, both in kernels_verify.hip; one host path over the rule header's Model (verify_rules::Homography,
// epipolar_rules::Fundamental) and over the match lists of many pairs as one segmented list, by the plan of verify_batch.hpp.
// A launch carries the workgroups of many pairs, the selection leaves the winning matrices on the device for the first mask,
// and the refit runs in lockstep: the host forms a round's models, one mask launch scores those of every pair still refining.
// The _device forms (verify_pairs_device_call) read their lists in device memory and run the lockstep rounds in kernels.
// The single calls (dlco_desc_verify_homography and its kin) are this path with one pair, moff = {0, m}: a launch of one
// entry.  Model::kSample matches make a sample -------------------------------------------------------------------------------
using verify_rules::Homography;
using epipolar_rules::Fundamental;
namespace vb = verify_batch;

// what a single call checks of its list before anything else; a list below the sample is invalid there, where the _pairs
// forms answer "no model" for it
template <typename Model>
bool verify_args_ok(const float *src, const float *dst, int64_t m, float threshold, int32_t n_hyp)
{
    return src && dst && m >= Model::kSample && m < ((int64_t)1 << 31) && std::isfinite(threshold) && threshold > 0.0f && n_hyp >= 1 &&
           n_hyp <= verify_rules::kMaxHyp;
}

template <typename Model>
bool verify_pairs_args_ok(const float *src, const float *dst, const int64_t *moff, int64_t n_pairs, float threshold, int32_t n_hyp)
{
    return src && dst && vb::offsets_ok(moff, n_pairs) && std::isfinite(threshold) && threshold > 0.0f && n_hyp >= 1 && n_hyp <= verify_rules::kMaxHyp;
}

// One launch of the plan on the device: its matches, its entries and, behind them, room for an active list.
struct VerifyLaunch {
    const vb::Entry *ent_host;
    const vb::Entry *ent;
    vb::Active *active;
    int64_t n, matches;
};

// the launch's matches and entries to the device, count and n zeroed
VerifyLaunch verify_pairs_upload(dlco_desc_ctx *c, const vb::Plan &pl, const vb::Launch &la, const float *src_host, const float *dst_host, int32_t n_hyp)
{
    const size_t n = (size_t)la.n, ent_bytes = n * sizeof(vb::Entry);
    c->v_src.alloc((size_t)la.matches * 2); c->v_dst.alloc((size_t)la.matches * 2);
    c->v_H.alloc((size_t)la.hyps * 9); c->v_count.alloc((size_t)la.hyps);
    c->v_key.alloc(n); c->v_cur.alloc(n * 9); c->v_n.alloc(n);
    c->v_mask.alloc((size_t)la.matches);
    c->v_plan.alloc(ent_bytes + n * sizeof(vb::Active));
    const vb::Entry *ent_host = pl.entries.data() + la.e0;
    DLCO_HIP(hipMemcpyAsync(c->v_src.p, src_host + 2 * la.match0, (size_t)la.matches * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    DLCO_HIP(hipMemcpyAsync(c->v_dst.p, dst_host + 2 * la.match0, (size_t)la.matches * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    DLCO_HIP(hipMemcpyAsync(c->v_plan.p, ent_host, ent_bytes, hipMemcpyHostToDevice, c->stream));
    DLCO_HIP(hipMemsetAsync(c->v_count.p, 0, (size_t)la.hyps * sizeof(int32_t), c->stream));
    DLCO_HIP(hipMemsetAsync(c->v_n.p, 0, n * sizeof(int32_t), c->stream));
    return VerifyLaunch{ent_host, reinterpret_cast<const vb::Entry *>(c->v_plan.p), reinterpret_cast<vb::Active *>(c->v_plan.p + ent_bytes), la.n, la.matches};
}

// every hypothesis of every pair and its count, to the host; a pair without an entry gets zeros
template <typename Model>
int verify_pairs_hypotheses_call(dlco_desc_ctx *c, const float *src_xy_host, const float *dst_xy_host, const int64_t *moff, int64_t n_pairs,
                                 float threshold, int32_t n_hyp, uint64_t seed, double *M_all_host, int32_t *count_host)
{
    if (!c || !M_all_host || !count_host || !verify_pairs_args_ok<Model>(src_xy_host, dst_xy_host, moff, n_pairs, threshold, n_hyp))
        return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_HIP(hipSetDevice(c->device));
        const double t2 = verify_rules::threshold_sq(threshold);
        const vb::Plan pl = vb::plan(moff, n_pairs, n_hyp, Model::kSample);
        const size_t nh = (size_t)n_hyp;
        for (int64_t p = 0; p < n_pairs; p++) {
            if (pl.launch_of_pair[(size_t)p] >= 0) continue;
            std::memset(M_all_host + (size_t)p * nh * 9, 0, nh * 9 * sizeof(double));
            std::memset(count_host + (size_t)p * nh, 0, nh * sizeof(int32_t));
        }
        EventPair ev;
        double ms = 0.0;
        for (const vb::Launch &la : pl.launches) {
            const VerifyLaunch v = verify_pairs_upload(c, pl, la, src_xy_host, dst_xy_host, n_hyp);
            ms += timed_ms(c, ev, [&] {
                verify_pairs_hypotheses<Model>(c->v_src.p, c->v_dst.p, v.ent, v.n, seed, n_hyp, c->v_H.p, c->stream);
                verify_pairs_score<Model>(c->v_src.p, c->v_dst.p, v.ent, v.n, la.score_wgs, c->v_H.p, n_hyp, t2, c->v_count.p, c->stream);
            }, [&] {
                // entries [e, r) whose pairs are consecutive own one range of the caller's arrays: their slots go straight there
                for (int64_t e = 0, r; e < v.n; e = r) {
                    for (r = e + 1; r < v.n && v.ent_host[r].pair == v.ent_host[r - 1].pair + 1; r++) {}
                    const size_t p = (size_t)v.ent_host[e].pair, run = (size_t)(r - e) * nh;
                    DLCO_HIP(hipMemcpyAsync(M_all_host + p * nh * 9, c->v_H.p + (size_t)e * nh * 9, run * 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
                    DLCO_HIP(hipMemcpyAsync(count_host + p * nh, c->v_count.p + (size_t)e * nh, run * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
                }
            });
        }
        c->last_ms = ms;
    });
}

// the best model of every pair, its mask and the refit in lockstep: in a round the host forms Model::refit_round for every
// pair still refining, on the pair's own slice, one mask launch scores them, and verify_rules::refit_step decides per pair
template <typename Model>
int verify_pairs_model_call(dlco_desc_ctx *c, const float *src_xy_host, const float *dst_xy_host, const int64_t *moff, int64_t n_pairs,
                            float threshold, int32_t n_hyp, uint64_t seed, int32_t refine, double *M_out, uint8_t *inlier_host, int64_t *n_inliers,
                            int32_t *best_hyp)
{
    if (!c || !M_out || !n_inliers || refine < 0 || refine > verify_rules::kMaxRefine ||
        !verify_pairs_args_ok<Model>(src_xy_host, dst_xy_host, moff, n_pairs, threshold, n_hyp))
        return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        namespace vr = verify_rules;
        DLCO_HIP(hipSetDevice(c->device));
        const double t2 = vr::threshold_sq(threshold);
        const vb::Plan pl = vb::plan(moff, n_pairs, n_hyp, Model::kSample);
        // "no model" everywhere; the entries overwrite their slots
        std::memset(M_out, 0, (size_t)n_pairs * 9 * sizeof(double));
        if (inlier_host) std::memset(inlier_host, 0, (size_t)moff[n_pairs]);
        for (int64_t p = 0; p < n_pairs; p++) { n_inliers[p] = 0; if (best_hyp) best_hyp[p] = -1; }
        const size_t ne = (size_t)pl.max_entries;
        std::vector<uint64_t> key(ne);
        std::vector<double> M_try(ne * 9);
        std::vector<int32_t> cnt(ne), live;
        std::vector<uint8_t> cur((size_t)pl.max_matches), trial((size_t)pl.max_matches);
        std::vector<vb::Active> act(ne);
        EventPair ev;
        double ms = 0.0;
        for (const vb::Launch &la : pl.launches) {
            const VerifyLaunch v = verify_pairs_upload(c, pl, la, src_xy_host, dst_xy_host, n_hyp);
            const float *src = src_xy_host + 2 * la.match0, *dst = dst_xy_host + 2 * la.match0;
            for (int64_t e = 0; e < v.n; e++) act[(size_t)e] = vb::Active{(int32_t)e, v.ent_host[e].mwg0};
            DLCO_HIP(hipMemcpyAsync(v.active, act.data(), (size_t)v.n * sizeof(vb::Active), hipMemcpyHostToDevice, c->stream));
            ms += timed_ms(c, ev, [&] {
                verify_pairs_hypotheses<Model>(c->v_src.p, c->v_dst.p, v.ent, v.n, seed, n_hyp, c->v_H.p, c->stream);
                verify_pairs_score<Model>(c->v_src.p, c->v_dst.p, v.ent, v.n, la.score_wgs, c->v_H.p, n_hyp, t2, c->v_count.p, c->stream);
                verify_pairs_select(c->v_count.p, c->v_H.p, v.n, n_hyp, c->v_key.p, c->v_cur.p, c->stream);
                verify_pairs_mask<Model>(c->v_src.p, c->v_dst.p, v.ent, v.active, v.n, la.mask_wgs, c->v_cur.p, t2, c->v_mask.p, c->v_n.p, nullptr, c->stream);
            }, [&] {
                DLCO_HIP(hipMemcpyAsync(key.data(), c->v_key.p, (size_t)v.n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
                DLCO_HIP(hipMemcpyAsync(M_try.data(), c->v_cur.p, (size_t)v.n * 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
                DLCO_HIP(hipMemcpyAsync(cur.data(), c->v_mask.p, (size_t)v.matches, hipMemcpyDeviceToHost, c->stream));
                DLCO_HIP(hipMemcpyAsync(cnt.data(), c->v_n.p, (size_t)v.n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            });
            live.clear();
            for (int64_t e = 0; e < v.n; e++) {
                if (vr::key_count(key[(size_t)e]) == 0) continue;
                const size_t p = (size_t)v.ent_host[e].pair;
                std::memcpy(M_out + 9 * p, M_try.data() + 9 * (size_t)e, 9 * sizeof(double));
                n_inliers[p] = cnt[(size_t)e];
                if (best_hyp) best_hyp[p] = vr::key_hyp(key[(size_t)e]);
                live.push_back((int32_t)e);
            }
            for (int32_t k = 0; k < refine && !live.empty(); k++) {
                int64_t n_act = 0, wgs = 0;
                for (int32_t e : live) {
                    const vb::Entry &en = v.ent_host[e];
                    if (!Model::refit_round(src + 2 * en.m0, dst + 2 * en.m0, en.m, cur.data() + en.m0, M_try.data() + 9 * (size_t)e)) continue;
                    act[(size_t)n_act++] = vb::Active{e, (int32_t)wgs};
                    wgs += vb::blocks(en.m);
                }
                if (n_act == 0) break;
                DLCO_HIP(hipMemcpyAsync(c->v_cur.p, M_try.data(), (size_t)v.n * 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
                DLCO_HIP(hipMemcpyAsync(v.active, act.data(), (size_t)n_act * sizeof(vb::Active), hipMemcpyHostToDevice, c->stream));
                DLCO_HIP(hipMemsetAsync(c->v_n.p, 0, (size_t)v.n * sizeof(int32_t), c->stream));
                ms += timed_ms(c, ev, [&] {
                    verify_pairs_mask<Model>(c->v_src.p, c->v_dst.p, v.ent, v.active, n_act, wgs, c->v_cur.p, t2, c->v_mask.p, c->v_n.p, nullptr, c->stream);
                }, [&] {
                    DLCO_HIP(hipMemcpyAsync(trial.data(), c->v_mask.p, (size_t)v.matches, hipMemcpyDeviceToHost, c->stream));
                    DLCO_HIP(hipMemcpyAsync(cnt.data(), c->v_n.p, (size_t)v.n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
                });
                live.clear();
                for (int64_t a = 0; a < n_act; a++) {
                    const int32_t e = act[(size_t)a].entry;
                    const vb::Entry &en = v.ent_host[e];
                    if (vr::refit_step(en.m, M_out + 9 * (size_t)en.pair, cur.data() + en.m0, n_inliers[en.pair], M_try.data() + 9 * (size_t)e,
                                       trial.data() + en.m0, cnt[(size_t)e]))
                        live.push_back(e);
                }
            }
            if (inlier_host)
                for (int64_t e = 0; e < v.n; e++)
                    std::memcpy(inlier_host + la.match0 + v.ent_host[e].m0, cur.data() + v.ent_host[e].m0, (size_t)v.ent_host[e].m);
        }
        c->last_ms = ms;
    });
}

// The same call on lists in device memory, read in place (8-byte aligned: the kernels read pairs of floats), with the refit
// on the device: per launch of the plan the hypotheses, the scoring, the selection and the first mask, then `refine` rounds of
// refit, mask and step queued without a host sync (an entry that has left the refit only reads its live flag), one download
// of matrices, counts and keys and one sync.  The current mask of an entry lives where it ends up: in inlier_dev, or in
// scratch when that is NULL.
template <typename Model>
int verify_pairs_device_call(dlco_desc_ctx *c, const float *src_xy_dev, const float *dst_xy_dev, const int64_t *moff, int64_t n_pairs, float threshold,
                             int32_t n_hyp, uint64_t seed, int32_t refine, double *M_out, uint8_t *inlier_dev, int64_t *n_inliers, int32_t *best_hyp)
{
    if (!c || !M_out || !n_inliers || refine < 0 || refine > verify_rules::kMaxRefine || (uintptr_t)src_xy_dev % 8 != 0 || (uintptr_t)dst_xy_dev % 8 != 0 ||
        !verify_pairs_args_ok<Model>(src_xy_dev, dst_xy_dev, moff, n_pairs, threshold, n_hyp))
        return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        namespace vr = verify_rules;
        DLCO_HIP(hipSetDevice(c->device));
        const double t2 = vr::threshold_sq(threshold);
        const vb::Plan pl = vb::plan(moff, n_pairs, n_hyp, Model::kSample);
        std::memset(M_out, 0, (size_t)n_pairs * 9 * sizeof(double));
        for (int64_t p = 0; p < n_pairs; p++) { n_inliers[p] = 0; if (best_hyp) best_hyp[p] = -1; }
        if (inlier_dev && moff[n_pairs] > 0) DLCO_HIP(hipMemsetAsync(inlier_dev, 0, (size_t)moff[n_pairs], c->stream));
        const size_t ne = (size_t)pl.max_entries;
        std::vector<uint64_t> key(ne);
        std::vector<double> M(ne * 9);
        std::vector<int32_t> cnt(ne);
        std::vector<vb::Active> act(ne);
        EventPair ev;
        double ms = 0.0;
        for (const vb::Launch &la : pl.launches) {
            const size_t n = (size_t)la.n, ent_bytes = n * sizeof(vb::Entry);
            c->v_H.alloc((size_t)la.hyps * 9); c->v_count.alloc((size_t)la.hyps);
            c->v_key.alloc(n); c->v_cur.alloc(n * 9); c->v_try.alloc(n * 9); c->v_n.alloc(n); c->v_ntry.alloc(n); c->v_live.alloc(n);
            c->v_trial.alloc((size_t)la.matches);
            if (!inlier_dev) c->v_mask.alloc((size_t)la.matches);
            c->v_plan.alloc(ent_bytes + n * sizeof(vb::Active));
            const vb::Entry *ent_host = pl.entries.data() + la.e0;
            const vb::Entry *ent = reinterpret_cast<const vb::Entry *>(c->v_plan.p);
            const vb::Active *active = reinterpret_cast<const vb::Active *>(c->v_plan.p + ent_bytes);
            const float *src = src_xy_dev + 2 * la.match0, *dst = dst_xy_dev + 2 * la.match0;
            uint8_t *mask = inlier_dev ? inlier_dev + la.match0 : c->v_mask.p;
            for (int64_t e = 0; e < la.n; e++) act[(size_t)e] = vb::Active{(int32_t)e, ent_host[e].mwg0};
            DLCO_HIP(hipMemcpyAsync(c->v_plan.p, ent_host, ent_bytes, hipMemcpyHostToDevice, c->stream));
            DLCO_HIP(hipMemcpyAsync(c->v_plan.p + ent_bytes, act.data(), n * sizeof(vb::Active), hipMemcpyHostToDevice, c->stream));
            DLCO_HIP(hipMemsetAsync(c->v_count.p, 0, (size_t)la.hyps * sizeof(int32_t), c->stream));
            DLCO_HIP(hipMemsetAsync(c->v_n.p, 0, n * sizeof(int32_t), c->stream));
            DLCO_HIP(hipMemsetAsync(c->v_ntry.p, 0, n * sizeof(int32_t), c->stream));
            ms += timed_ms(c, ev, [&] {
                verify_pairs_hypotheses<Model>(src, dst, ent, la.n, seed, n_hyp, c->v_H.p, c->stream);
                verify_pairs_score<Model>(src, dst, ent, la.n, la.score_wgs, c->v_H.p, n_hyp, t2, c->v_count.p, c->stream);
                verify_pairs_select(c->v_count.p, c->v_H.p, la.n, n_hyp, c->v_key.p, c->v_cur.p, c->stream);
                verify_pairs_mask<Model>(src, dst, ent, active, la.n, la.mask_wgs, c->v_cur.p, t2, mask, c->v_n.p, nullptr, c->stream);
                if (refine > 0) verify_pairs_live(c->v_key.p, la.n, c->v_live.p, c->stream);
                for (int32_t k = 0; k < refine; k++) {
                    verify_pairs_refit<Model>(src, dst, ent, la.n, mask, c->v_live.p, c->v_try.p, c->stream);
                    verify_pairs_mask<Model>(src, dst, ent, active, la.n, la.mask_wgs, c->v_try.p, t2, c->v_trial.p, c->v_ntry.p, c->v_live.p, c->stream);
                    verify_pairs_step(ent, la.n, c->v_try.p, c->v_trial.p, c->v_ntry.p, c->v_cur.p, mask, c->v_n.p, c->v_live.p, c->stream);
                }
            }, [&] {
                DLCO_HIP(hipMemcpyAsync(key.data(), c->v_key.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
                DLCO_HIP(hipMemcpyAsync(M.data(), c->v_cur.p, n * 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
                DLCO_HIP(hipMemcpyAsync(cnt.data(), c->v_n.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
            });
            for (int64_t e = 0; e < la.n; e++) {
                if (vr::key_count(key[(size_t)e]) == 0) continue;
                const size_t p = (size_t)ent_host[e].pair;
                std::memcpy(M_out + 9 * p, M.data() + 9 * (size_t)e, 9 * sizeof(double));
                n_inliers[p] = cnt[(size_t)e];
                if (best_hyp) best_hyp[p] = vr::key_hyp(key[(size_t)e]);
            }
        }
        if (pl.launches.empty()) sync(c);                   // the memset of the mask
        c->last_ms = ms;
    });
}

// one round of the refit kernel on masks of the caller's: for tests and tools
template <typename Model>
void verify_pairs_refit_round_call(dlco_desc_ctx *c, const float *src_host, const float *dst_host, const int64_t *moff, int64_t n_pairs,
                                   const uint8_t *mask_host, double *M_out, uint8_t *ok)
{
    DLCO_HIP(hipSetDevice(c->device));
    const vb::Plan pl = vb::plan(moff, n_pairs, 1, Model::kSample);
    std::memset(M_out, 0, (size_t)n_pairs * 9 * sizeof(double));
    std::memset(ok, 0, (size_t)n_pairs);
    std::vector<double> M((size_t)pl.max_entries * 9);
    std::vector<uint8_t> live((size_t)pl.max_entries);
    EventPair ev;
    double ms = 0.0;
    for (const vb::Launch &la : pl.launches) {
        const VerifyLaunch v = verify_pairs_upload(c, pl, la, src_host, dst_host, 1);
        const size_t n = (size_t)la.n;
        c->v_try.alloc(n * 9); c->v_live.alloc(n);
        DLCO_HIP(hipMemcpyAsync(c->v_mask.p, mask_host + la.match0, (size_t)la.matches, hipMemcpyHostToDevice, c->stream));
        DLCO_HIP(hipMemsetAsync(c->v_live.p, 1, n, c->stream));
        ms += timed_ms(c, ev, [&] { verify_pairs_refit<Model>(c->v_src.p, c->v_dst.p, v.ent, v.n, c->v_mask.p, c->v_live.p, c->v_try.p, c->stream); }, [&] {
            DLCO_HIP(hipMemcpyAsync(M.data(), c->v_try.p, n * 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            DLCO_HIP(hipMemcpyAsync(live.data(), c->v_live.p, n, hipMemcpyDeviceToHost, c->stream));
        });
        for (size_t e = 0; e < n; e++) {
            const size_t p = (size_t)v.ent_host[e].pair;
            ok[p] = live[e];
            std::memcpy(M_out + 9 * p, M.data() + 9 * e, 9 * sizeof(double));
        }
    }
    c->last_ms = ms;
}
}  // namespace

extern "C" {

const char *dlco_desc_last_error(const dlco_desc_ctx *c) { return c ? c->err.c_str() : g_desc_error.c_str(); }

int dlco_desc_create(dlco_desc_ctx **out, float init_sigma, int32_t n_angle_bins, int32_t norm, int32_t device)
{
    if (!out) return DLCO_ERR_INVALID;
    *out = nullptr;
    dlco_desc_ctx *c = nullptr;
    const int rc = guarded(nullptr, [&] {
        DLCO_CHECK(n_angle_bins == kBins, DLCO_ERR_INVALID, "dlco_desc: nAngleBins must be 8 (the callers' value, src/comp-uprjdists.cpp:66)");
        DLCO_CHECK(init_sigma > 0.f, DLCO_ERR_INVALID, "dlco_desc: InitSigma must be positive");
        const hipDeviceProp_t prop = use_gfx950_device(device);
        c = new dlco_desc_ctx();
        c->device = device; c->sigma = init_sigma; c->norm = norm != 0;
        c->n_cu = prop.multiProcessorCount;
        DLCO_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        // Gaussian taps exactly as cv::getGaussianKernel(ksize, sigma, CV_32F) forms them [OpenCV-src]
        int ks = (int)std::lrint((double)init_sigma * 4.0 * 2.0 + 1.0) | 1;
        DLCO_CHECK(ks <= 63, DLCO_ERR_INVALID, "dlco_desc: InitSigma too large for a 64 x 64 patch (kernel above 63 taps)");
        float cf[64] = {0};
        {
            const double scale2x = -0.5 / ((double)init_sigma * (double)init_sigma);
            double sum = 0.0;
            for (int i = 0; i < ks; i++) {
                const double x = i - (ks - 1) * 0.5;
                cf[i] = (float)std::exp(scale2x * x * x);
                sum += cf[i];
            }
            sum = 1.0 / sum;
            for (int i = 0; i < ks; i++) cf[i] = (float)(cf[i] * sum);
        }
        c->ks = ks;
        c->cf.alloc(64);
        DLCO_HIP(hipMemcpyAsync(c->cf.p, cf, sizeof(cf), hipMemcpyHostToDevice, c->stream));
        const double kPi = 3.1415926535897932384626433832795;
        const float step = (float)(2.0f * kPi / (double)(float)n_angle_bins);      // src/vgg-desc.cpp:71
        c->inv_step = (float)(1.0 / (double)step);
        // mquantiles constants for n = 4096, q = 0.8 (src/vgg-desc.cpp:113-126)
        const int n = kPix;
        const float aleph = (float)n * 0.8f + 0.5f;
        int k = (int)std::floor(aleph);
        if (k >= n - 1) k = n - 1;
        if (k <= 1) k = 1;
        float g = aleph - (float)k;
        if (g >= 1.0f) g = 1.0f;
        if (g <= 0.0f) g = 0.0f;
        c->qk = k; c->qgamma = g;
        sync(c);
    });
    if (rc != DLCO_OK) { delete c; return rc; }
    *out = c;
    return DLCO_OK;
}

void dlco_desc_destroy(dlco_desc_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    delete c;
}

// SelectPRFilters (src/misc.cpp:78-168): rows of PRFilters [8*wcols, cols] whose w entry is positive and
// that are not all zero, duplicates removed, sorted ascending lexicographically.  out may be NULL to
// query the count.  Pure host logic.
int dlco_desc_select_filters(const float *pr_filters, int32_t rows, int32_t cols, const float *w, int32_t wcols, float *out,
                             int32_t *nsel_out)
{
    if (!pr_filters || !w || !nsel_out || rows != wcols * 8 || cols < 1) return DLCO_ERR_INVALID;
    std::vector<int> keep;
    for (int i = 0; i < wcols; i++)
        for (int j = 0; j < 8; j++) {
            const int row = i * 8 + j;
            if (!(w[i] > 0.0f)) continue;
            const float *f = pr_filters + (size_t)row * cols;
            bool any = false;
            for (int k = 0; k < cols && !any; k++) any = f[k] != 0.0f;
            if (any) keep.push_back(row);
        }
    auto less = [&](int a, int b) {
        const float *x = pr_filters + (size_t)a * cols, *y = pr_filters + (size_t)b * cols;
        for (int k = 0; k < cols; k++) {
            if (x[k] == y[k]) continue;
            return x[k] < y[k];
        }
        return false;
    };
    auto same = [&](int a, int b) {
        const float *x = pr_filters + (size_t)a * cols, *y = pr_filters + (size_t)b * cols;
        for (int k = 0; k < cols; k++)
            if (!(x[k] == y[k])) return false;
        return true;
    };
    std::stable_sort(keep.begin(), keep.end(), less);
    keep.erase(std::unique(keep.begin(), keep.end(), same), keep.end());
    *nsel_out = (int32_t)keep.size();
    if (out)
        for (size_t i = 0; i < keep.size(); i++) std::memcpy(out + i * cols, pr_filters + (size_t)keep[i] * cols, (size_t)cols * sizeof(float));
    return DLCO_OK;
}

// sPRFilters [nsel, 4096] in the reference's column order (pixel x*64+y, the transposed patch)
int dlco_desc_set_filters(dlco_desc_ctx *c, const float *filters_host, int32_t nsel)
{
    if (!c || !filters_host || nsel < 1) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_CHECK(nsel <= 65536, DLCO_ERR_INVALID, "dlco_desc: too many filters");
        DLCO_HIP(hipSetDevice(c->device));
        c->nsel = nsel;
        c->nsel_pad = (nsel + 127) / 128 * 128;
        if (c->proj_F != nsel * kBins) { c->r = 0; c->proj_F = 0; c->proj_dim = 0; }     // a projection of another width no longer fits
        DevBuf<float> raw;
        raw.alloc((size_t)nsel * kPix);
        DLCO_HIP(hipMemcpyAsync(raw.p, filters_host, (size_t)nsel * kPix * sizeof(float), hipMemcpyHostToDevice, c->stream));
        c->filt.alloc((size_t)c->nsel_pad * kPix);
        c->filt.zero(c->stream);
        desc_permute_filters(raw.p, nsel, c->filt.p, c->stream);
        sync(c);
    });
}

int32_t dlco_desc_size(const dlco_desc_ctx *c) { return c ? c->nsel * kBins : 0; }

// get_desc of ONE patch in the reference's layout: PatchTrans [4096][8], row x*64+y (src/vgg-desc.cpp:41-152)
int dlco_desc_transform(dlco_desc_ctx *c, const uint8_t *patch_host, float *patch_trans_host)
{
    if (!c || !patch_host || !patch_trans_host) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_HIP(hipSetDevice(c->device));
        c->patches.alloc((size_t)kChunk * kPix);
        c->pt.alloc((size_t)kChunk * kBins * kPix);
        DLCO_HIP(hipMemcpyAsync(c->patches.p, patch_host, kPix, hipMemcpyHostToDevice, c->stream));
        desc_transform(c->patches.p, 1, c->cf.p, c->ks, c->inv_step, c->norm, c->qk, c->qgamma, c->pt.p, c->stream);
        std::vector<float> planes((size_t)kBins * kPix);
        DLCO_HIP(hipMemcpyAsync(planes.data(), c->pt.p, planes.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        sync(c);
        for (int y = 0; y < 64; y++)
            for (int x = 0; x < 64; x++)
                for (int b = 0; b < kBins; b++) patch_trans_host[(size_t)(x * 64 + y) * kBins + b] = planes[(size_t)b * kPix + y * 64 + x];
    });
}

// Desc [n, nsel*8] = min(sPRFilters * get_desc(patch), 1) per patch, row-major like Mat Desc1 flattened
int dlco_desc_compute(dlco_desc_ctx *c, const uint8_t *patches_host, int64_t n, float *desc_host)
{
    if (!c || !patches_host || !desc_host || n < 1) return DLCO_ERR_INVALID;
    return guarded(c, [&] { compute(c, PatchSource::patches(patches_host), n, RowsOut::pooled(desc_host, Where::Host, (long)c->nsel * kBins)); });
}

int dlco_desc_compute_device(dlco_desc_ctx *c, const uint8_t *patches_host, int64_t n, float *desc_dev, int64_t ld)
{
    if (!c || !patches_host || !desc_dev || n < 1) return DLCO_ERR_INVALID;
    return guarded(c, [&] { compute(c, PatchSource::patches(patches_host), n, RowsOut::pooled(desc_dev, Where::Device, (long)ld)); });
}

// The output of comp-uprjdists: Distance [n_pairs, nsel*8] and Label [n_pairs] for pairs [n_pairs,4] =
// (patchID1, 3DpointID1, patchID2, 3DpointID2).  Descriptors are computed once per patch.
namespace {
// sink of the non-streaming entry points: rows land in the caller's whole-matrix buffers
struct CopySink { float *dist; uint8_t *label; int64_t cols; };
int copy_sink(void *user, int64_t row0, int64_t rows, const float *dist, const uint8_t *label)
{
    CopySink *k = static_cast<CopySink *>(user);
    std::memcpy(k->dist + row0 * k->cols, dist, (size_t)rows * k->cols * sizeof(float));
    if (k->label) std::memcpy(k->label + row0, label, (size_t)rows);
    return 0;
}
void check_pairs(const int32_t *pairs_host, int64_t n_pairs, int64_t n_patches)
{
    for (int64_t i = 0; i < n_pairs; i++) {
        const int32_t *q = pairs_host + i * 4;
        DLCO_CHECK(q[0] >= 0 && q[0] < n_patches && q[2] >= 0 && q[2] < n_patches, DLCO_ERR_INVALID, "dlco_desc: patch id out of range");
    }
}
struct PinnedStage {
    float *dist = nullptr; uint8_t *label = nullptr;
    PinnedStage(size_t floats, size_t labels)
    {
        DLCO_HIP(hipHostMalloc((void **)&dist, std::max<size_t>(floats, 1) * sizeof(float)));
        if (hipHostMalloc((void **)&label, std::max<size_t>(labels, 1)) != hipSuccess) { (void)hipHostFree(dist); throw Error(DLCO_ERR_HIP, "hipHostMalloc failed"); }
    }
    ~PinnedStage() { (void)hipHostFree(dist); (void)hipHostFree(label); }
};
}  // namespace

// comp-uprjdists' Distance / Label rows, handed to `sink` chunk_rows pairs at a time in row order: the reference
// writes a 128-row hyperslab per chunk and checks it (src/comp-uprjdists.cpp:298-349), so its host memory stays at one
// chunk; a whole-matrix buffer (16 GB at 500k x 8192) is only needed by callers that ask for one.
int dlco_desc_pair_dists_stream(dlco_desc_ctx *c, const uint8_t *patches_host, int64_t n_patches, const int32_t *pairs_host,
                                int64_t n_pairs, int64_t chunk_rows, dlco_desc_sink_fn sink, void *user)
{
    if (!c || !patches_host || !pairs_host || !sink || n_patches < 1 || n_pairs < 1 || chunk_rows < 1) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        const int F = c->nsel * kBins;
        check_pairs(pairs_host, n_pairs, n_patches);
        DLCO_HIP(hipSetDevice(c->device));
        DevBuf<float> table, dist;
        table.alloc((size_t)n_patches * F);
        compute(c, PatchSource::patches(patches_host), n_patches, RowsOut::pooled(table.p, Where::Device, F));
        const int64_t pchunk = std::max<int64_t>(1, std::min<int64_t>(std::min(n_pairs, chunk_rows), ((int64_t)1 << 28) / F));
        DevBuf<int32_t> pairs;
        DevBuf<uint8_t> lab;
        pairs.alloc((size_t)pchunk * 4);
        lab.alloc((size_t)pchunk);
        dist.alloc((size_t)pchunk * F);
        PinnedStage st((size_t)pchunk * F, (size_t)pchunk);
        for (int64_t p0 = 0; p0 < n_pairs; p0 += pchunk) {
            const int64_t cnt = std::min(pchunk, n_pairs - p0);
            DLCO_HIP(hipMemcpyAsync(pairs.p, pairs_host + p0 * 4, (size_t)cnt * 4 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
            desc_pair_diff(table.p, F, F, pairs.p, cnt, dist.p, lab.p, c->stream);
            DLCO_HIP(hipMemcpyAsync(st.dist, dist.p, (size_t)cnt * F * sizeof(float), hipMemcpyDeviceToHost, c->stream));
            DLCO_HIP(hipMemcpyAsync(st.label, lab.p, (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
            sync(c);
            const int rc = sink(user, p0, cnt, st.dist, st.label);
            if (rc != 0) throw Error(DLCO_ERR_INVALID, "dlco_desc: the row sink failed with code " + std::to_string(rc));
        }
    });
}

int dlco_desc_pair_dists(dlco_desc_ctx *c, const uint8_t *patches_host, int64_t n_patches, const int32_t *pairs_host, int64_t n_pairs,
                         float *dist_host, uint8_t *label_host)
{
    if (!c || !dist_host) return DLCO_ERR_INVALID;
    CopySink k{dist_host, label_host, (int64_t)c->nsel * kBins};
    return dlco_desc_pair_dists_stream(c, patches_host, n_patches, pairs_host, n_pairs, (int64_t)1 << 40, copy_sink, &k);
}

// The output of comp-fulldists (src/comp-fulldists.cpp:285-369), the input of pr-learn: with ALL pooling-region
// filters set (rows = 8 * n_regions, one row per ring replica), Distance [n_pairs, n_regions] =
// sum over a region's 8 rows and 8 bins of (Desc2 - Desc1)^2, and Label.  A patch's full descriptor is
// rows * 8 floats (1.3 MB at 5120 regions), so the work goes by chunks of pairs: both patches of a chunk are
// transformed and pooled, reduced per pair, and dropped; `sink` receives the rows of every chunk in order.
int dlco_desc_full_dists_stream(dlco_desc_ctx *c, const uint8_t *patches_host, int64_t n_patches, const int32_t *pairs_host,
                                int64_t n_pairs, int64_t chunk_rows, dlco_desc_sink_fn sink, void *user)
{
    if (!c || !patches_host || !pairs_host || !sink || n_patches < 1 || n_pairs < 1 || chunk_rows < 1) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_CHECK(c->nsel > 0 && c->nsel % 8 == 0, DLCO_ERR_INVALID, "dlco_desc_full_dists: the filter bank must hold 8 rows per pooling region");
        const int F = c->nsel * kBins, groups = c->nsel / 8;
        check_pairs(pairs_host, n_pairs, n_patches);
        DLCO_HIP(hipSetDevice(c->device));
        // pairs per chunk: 2 * chunk descriptors of F floats within ~2 GB, and within one transform chunk
        const int64_t pchunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(kChunk / 2, chunk_rows), ((int64_t)1 << 29) / ((int64_t)2 * F)));
        DevBuf<float> desc, dist;
        desc.alloc((size_t)2 * pchunk * F);
        dist.alloc((size_t)pchunk * groups);
        std::vector<uint8_t> stage((size_t)2 * pchunk * kPix);
        PinnedStage st((size_t)pchunk * groups, (size_t)pchunk);
        double ms_total = 0.0;
        for (int64_t p0 = 0; p0 < n_pairs; p0 += pchunk) {
            const int64_t cnt = std::min(pchunk, n_pairs - p0);
            for (int64_t i = 0; i < cnt; i++) {
                const int32_t *q = pairs_host + (p0 + i) * 4;
                std::memcpy(stage.data() + (size_t)i * kPix, patches_host + (size_t)q[0] * kPix, kPix);
                std::memcpy(stage.data() + (size_t)(cnt + i) * kPix, patches_host + (size_t)q[2] * kPix, kPix);
                st.label[i] = (q[1] == q[3]) ? 1 : 0;                              // :268-272 of both tools
            }
            compute(c, PatchSource::patches(stage.data()), 2 * cnt, RowsOut::pooled(desc.p, Where::Device, F));
            ms_total += c->last_ms;
            desc_full_dist(desc.p, F, groups, (int)cnt, dist.p, c->stream);
            DLCO_HIP(hipMemcpyAsync(st.dist, dist.p, (size_t)cnt * groups * sizeof(float), hipMemcpyDeviceToHost, c->stream));
            sync(c);
            const int rc = sink(user, p0, cnt, st.dist, st.label);
            if (rc != 0) throw Error(DLCO_ERR_INVALID, "dlco_desc: the row sink failed with code " + std::to_string(rc));
        }
        c->last_ms = ms_total;
    });
}

int dlco_desc_full_dists(dlco_desc_ctx *c, const uint8_t *patches_host, int64_t n_patches, const int32_t *pairs_host, int64_t n_pairs,
                         float *dist_host, uint8_t *label_host)
{
    if (!c || !dist_host) return DLCO_ERR_INVALID;
    CopySink k{dist_host, label_host, (int64_t)c->nsel / 8};
    return dlco_desc_full_dists_stream(c, patches_host, n_patches, pairs_host, n_pairs, (int64_t)1 << 40, copy_sink, &k);
}

// ---- the learnt descriptor: y = W * min(sPRFilters * get_desc(patch), 1) --------------------------------------------
// W [r, F] is pj-learn's output (dataset "W"), applied there to pair differences (src/pj-learn.cpp:551, ComputePJStats);
// here it is applied to the descriptor of a patch, which is what a user of the trained model wants back.
int dlco_desc_set_projection(dlco_desc_ctx *c, const float *W_host, int32_t r, int32_t F)
{
    if (!c || !W_host) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_CHECK(c->nsel > 0, DLCO_ERR_INVALID, "dlco_desc_set_projection: set the filters first");
        DLCO_CHECK(F == c->nsel * kBins, DLCO_ERR_INVALID, "dlco_desc_set_projection: W has " + std::to_string(F) + " columns, the descriptor " +
                                                               std::to_string(c->nsel * kBins) + " entries");
        DLCO_CHECK(r >= 1 && r <= F, DLCO_ERR_INVALID, "dlco_desc_set_projection: r must be in [1, F]");
        int dim = 0;
        for (int i = 0; i < r; i++) {
            const float *row = W_host + (size_t)i * F;
            bool any = false;
            for (int f = 0; f < F && !any; f++) any = row[f] != 0.0f;
            dim += any ? 1 : 0;
        }
        DLCO_HIP(hipSetDevice(c->device));
        c->r = 0; c->proj_F = 0; c->proj_dim = 0;
        c->W.alloc((size_t)r * F);
        DLCO_HIP(hipMemcpyAsync(c->W.p, W_host, (size_t)r * F * sizeof(float), hipMemcpyHostToDevice, c->stream));
        sync(c);
        c->r = r; c->proj_F = F; c->proj_dim = dim;
        if (c->q_r != r) c->q_r = 0;                       // a quantiser of another width no longer fits
    });
}

int32_t dlco_desc_projected_size(const dlco_desc_ctx *c) { return c ? c->r : 0; }

// Y [n, r], one row per patch; the un-projected rows never leave the device
int dlco_desc_describe(dlco_desc_ctx *c, const uint8_t *patches_host, int64_t n, float *out_host)
{
    if (!c || !patches_host || !out_host || n < 1) return DLCO_ERR_INVALID;
    return guarded(c, [&] { compute(c, PatchSource::patches(patches_host), n, RowsOut::projected(out_host, Where::Host, (long)c->r)); });
}

int dlco_desc_describe_device(dlco_desc_ctx *c, const uint8_t *patches_host, int64_t n, float *out_dev, int64_t ld)
{
    if (!c || !patches_host || !out_dev || n < 1) return DLCO_ERR_INVALID;
    return guarded(c, [&] { compute(c, PatchSource::patches(patches_host), n, RowsOut::projected(out_dev, Where::Device, (long)ld)); });
}

// ---- keypoints of an image: the patches are sampled on the device (kernels_patch.hip) by the rule of patch_rules.hpp ------
namespace {
bool image_args_ok(const uint8_t *image, int32_t width, int32_t height, int64_t pitch)
{
    return image && width >= 1 && width <= 32768 && height >= 1 && height <= 32768 && pitch >= width;
}

bool keypoint_args_ok(const float *keypoints, int64_t n, float scale_factor)
{
    return keypoints && n >= 1 && std::isfinite(scale_factor) && scale_factor > 0.0f;
}

// the frames of keypoints [n][4] = (x, y, size, angle) on the context's image, and their status when asked for
void keypoint_frames(const dlco_desc_ctx *c, const float *keypoints, int64_t n, float scale_factor, bool use_orientation, uint8_t *status,
                     std::vector<patch_rules::Frame> &frames)
{
    DLCO_CHECK(c->img, DLCO_ERR_INVALID, "dlco_desc: set an image first");
    frames.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        const float *k = keypoints + 4 * i;
        frames[i] = patch_rules::make_frame(k[0], k[1], k[2], k[3], scale_factor, use_orientation);
        if (status) status[i] = (uint8_t)patch_rules::status(frames[i], c->img_w, c->img_h);
    }
}

void describe_keypoints(dlco_desc_ctx *c, const float *keypoints, int64_t n, float scale_factor, bool use_orientation, uint8_t *status,
                        const RowsOut &o)
{
    std::vector<patch_rules::Frame> frames;
    keypoint_frames(c, keypoints, n, scale_factor, use_orientation, status, frames);
    compute(c, PatchSource::keypoints(frames.data()), n, o);
}
}  // namespace

// image [height][pitch] u8 on the host; copied to rows of a 16-byte multiple
int dlco_desc_set_image(dlco_desc_ctx *c, const uint8_t *image_host, int32_t width, int32_t height, int64_t pitch)
{
    if (!c || !image_args_ok(image_host, width, height, pitch)) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_HIP(hipSetDevice(c->device));
        c->img = nullptr;
        c->d_S_valid = false;
        const size_t dpitch = ((size_t)width + 15) / 16 * 16;
        c->img_own.alloc(dpitch * (size_t)height);
        DLCO_HIP(hipMemcpy2DAsync(c->img_own.p, dpitch, image_host, (size_t)pitch, (size_t)width, (size_t)height, hipMemcpyHostToDevice, c->stream));
        sync(c);
        c->img = c->img_own.p; c->img_w = width; c->img_h = height; c->img_pitch = (long)dpitch;
    });
}

// the same image already in device memory: used where it is, the caller keeps it alive and unchanged while keypoint calls run
int dlco_desc_set_image_device(dlco_desc_ctx *c, const uint8_t *image_dev, int32_t width, int32_t height, int64_t pitch)
{
    if (!c || !image_args_ok(image_dev, width, height, pitch)) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_HIP(hipSetDevice(c->device));
        c->img_own.release();
        c->d_S_valid = false;
        c->img = image_dev; c->img_w = width; c->img_h = height; c->img_pitch = (long)pitch;
    });
}

// patches [n][64][64] u8 and status [n] (may be NULL) of keypoints [n][4]; needs neither filters nor a projection
int dlco_desc_extract_patches(dlco_desc_ctx *c, const float *keypoints_host, int64_t n, float scale_factor, int32_t use_orientation,
                              uint8_t *patches_host, uint8_t *status_host)
{
    if (!c || !patches_host || !keypoint_args_ok(keypoints_host, n, scale_factor)) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        std::vector<patch_rules::Frame> frames;
        keypoint_frames(c, keypoints_host, n, scale_factor, use_orientation != 0, status_host, frames);
        const PatchSource src = PatchSource::keypoints(frames.data());
        DLCO_HIP(hipSetDevice(c->device));
        c->patches.alloc((size_t)kChunk * kPix);
        c->frames.alloc((size_t)kChunk);
        EventPair ev;
        double ms_total = 0.0;
        for (int64_t p0 = 0; p0 < n; p0 += kChunk) {
            const int cnt = (int)std::min<int64_t>(kChunk, n - p0);
            upload_chunk(c, src, p0, cnt);
            ms_total += timed_ms(c, ev, [&] { sample_chunk(c, src.frames + p0, cnt); }, [&] {
                DLCO_HIP(hipMemcpyAsync(patches_host + p0 * kPix, c->patches.p, (size_t)cnt * kPix, hipMemcpyDeviceToHost, c->stream));
            });
        }
        c->last_ms = ms_total;
    });
}

// Y [n, r] of keypoints: dlco_desc_describe on the patches dlco_desc_extract_patches gives, which stay in HBM; the rows of
// status 0 are zero
int dlco_desc_describe_keypoints(dlco_desc_ctx *c, const float *keypoints_host, int64_t n, float scale_factor, int32_t use_orientation,
                                 float *out_host, uint8_t *status_host)
{
    if (!c || !out_host || !keypoint_args_ok(keypoints_host, n, scale_factor)) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        describe_keypoints(c, keypoints_host, n, scale_factor, use_orientation != 0, status_host, RowsOut::projected(out_host, Where::Host, (long)c->r));
    });
}

int dlco_desc_describe_keypoints_device(dlco_desc_ctx *c, const float *keypoints_host, int64_t n, float scale_factor, int32_t use_orientation,
                                        float *out_dev, int64_t ld, uint8_t *status_host)
{
    if (!c || !out_dev || !keypoint_args_ok(keypoints_host, n, scale_factor)) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        describe_keypoints(c, keypoints_host, n, scale_factor, use_orientation != 0, status_host, RowsOut::projected(out_dev, Where::Device, (long)ld));
    });
}

// ---- keypoints of the image set: the detector of detect_rules.hpp (kernels_detect.hip) ------------------------------------
namespace {
bool detect_args_ok(int32_t n_octaves, int64_t threshold, int64_t max_keypoints, const void *keypoints, const int64_t *n_out)
{
    return n_octaves >= 1 && n_octaves <= detect_rules::kMaxOctaves && threshold >= 1 && max_keypoints >= 1 && keypoints && n_out;
}

// The integral image of the image set, formed unless it is cached; returns the milliseconds of its kernels, 0 when cached.
double integral_image(dlco_desc_ctx *c, const EventPair &ev)
{
    if (c->d_S_valid) return 0.0;
    const int W = c->img_w, H = c->img_h;
    c->d_S.alloc((size_t)(H + 1) * (size_t)detect_integral_pitch(W));
    c->d_seg.alloc(detect_colsum_count(W, H));
    const double ms = timed_ms(c, ev, [&] { detect_integral(c->img, W, H, c->img_pitch, c->d_S.p, c->d_seg.p, c->stream); });
    c->d_S_valid = true;
    return ms;
}

// The orientation kernel on n keypoints in device memory (16-byte aligned): angles [n] to the host, at a stride of
// angle_stride floats, vectors and status too when asked for.  Sets c->o_ms; the stream has drained on return.
void orient_rows(dlco_desc_ctx *c, const EventPair &ev, const float *kp_dev, int64_t n, float *angles, int64_t angle_stride, int64_t *vectors,
                 uint8_t *status)
{
    c->o_vec.alloc((size_t)n * 2);
    c->o_status.alloc((size_t)n);
    std::vector<int64_t> vec_own;
    if (!vectors) { vec_own.resize((size_t)n * 2); vectors = vec_own.data(); }
    c->o_ms = timed_ms(c, ev, [&] { orient_keypoints(c->d_S.p, c->img_w, c->img_h, kp_dev, n, c->o_vec.p, c->o_status.p, c->stream); }, [&] {
        DLCO_HIP(hipMemcpyAsync(vectors, c->o_vec.p, (size_t)n * 2 * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        if (status) DLCO_HIP(hipMemcpyAsync(status, c->o_status.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    });
    for (int64_t k = 0; k < n; k++) angles[k * angle_stride] = orient_rules::angle_of(vectors[2 * k], vectors[2 * k + 1]);
}

// The first min(n_found, max_keypoints) keypoints in the rule's order, to device memory (dst_dev) or to the host.  The
// survivors of the octaves are counted even where their buffers are full: the octaves then run again with room for all.
void detect(dlco_desc_ctx *c, int n_octaves, int64_t threshold, int64_t max_keypoints, float *kp_dst, int64_t *resp_dst, bool dst_dev,
            int64_t *n_out, int64_t *n_found, bool oriented = false)
{
    DLCO_CHECK(c->img, DLCO_ERR_INVALID, "dlco_desc: set an image first");
    DLCO_HIP(hipSetDevice(c->device));
    const int W = c->img_w, H = c->img_h;
    EventPair ev;
    for (double &ms : c->d_stage_ms) ms = 0.0;
    c->d_stage_ms[0] = integral_image(c, ev);
    c->d_count.alloc(1);
    size_t cap = std::max<size_t>(std::max<size_t>(c->d_cap, 1024), (size_t)W * (size_t)H / 128);
    unsigned found = 0;
    for (;;) {
        c->d_pos.alloc(cap); c->d_resp.alloc(cap); c->d_kp.alloc(cap * 4);
        c->d_cap = cap;
        DLCO_HIP(hipMemsetAsync(c->d_count.p, 0, sizeof(unsigned), c->stream));
        for (int o = 0; o < n_octaves; o++)
            c->d_stage_ms[1 + o] += timed_ms(c, ev, [&] {
                detect_octave(c->d_S.p, W, H, o, threshold, (unsigned)cap, c->d_count.p, c->d_pos.p, c->d_resp.p, c->d_kp.p, c->stream);
            });
        DLCO_HIP(hipMemcpyAsync(&found, c->d_count.p, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        sync(c);
        if (found <= cap) break;
        cap = found;
    }
    const unsigned n = found, keep = (unsigned)std::min<int64_t>(n, max_keypoints);
    if (keep > 0) {
        c->d_key_a.alloc(n); c->d_key_b.alloc(n); c->d_idx_a.alloc(n); c->d_idx_b.alloc(n);
        const size_t tmp_bytes = detect_select_bytes(n);
        c->d_tmp.alloc(tmp_bytes + 256);
        if (!dst_dev) { c->d_kp_out.alloc((size_t)keep * 4); if (resp_dst) c->d_resp_out.alloc(keep); }
        float *kp_out = dst_dev ? kp_dst : c->d_kp_out.p;
        int64_t *resp_out = !resp_dst ? nullptr : (dst_dev ? resp_dst : c->d_resp_out.p);
        c->d_stage_ms[1 + detect_rules::kMaxOctaves] = timed_ms(c, ev, [&] {
            detect_select(c->d_pos.p, c->d_resp.p, c->d_kp.p, n, keep, c->d_key_a.p, c->d_key_b.p, c->d_idx_a.p, c->d_idx_b.p, c->d_tmp.p, tmp_bytes,
                          kp_out, resp_out, c->stream);
        }, [&] {
            if (dst_dev) return;
            DLCO_HIP(hipMemcpyAsync(kp_dst, kp_out, (size_t)keep * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
            if (resp_dst) DLCO_HIP(hipMemcpyAsync(resp_dst, resp_out, (size_t)keep * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        });
    }
    // oriented (host form only): the kernel takes the selected rows where the selection left them, in device scratch
    c->o_ms = 0.0;
    if (oriented && keep > 0) orient_rows(c, ev, c->d_kp_out.p, keep, kp_dst + 3, 4, nullptr, nullptr);
    *n_out = keep;
    if (n_found) *n_found = n;
    c->last_ms = std::accumulate(std::begin(c->d_stage_ms), std::end(c->d_stage_ms), 0.0) + (oriented ? c->o_ms : 0.0);
}
}  // namespace

// keypoints [n_out][4] = (x, y, size, -1) and their responses, strongest first; rows at and beyond *n_out are left untouched
int dlco_desc_detect(dlco_desc_ctx *c, int32_t n_octaves, int64_t threshold, int64_t max_keypoints, float *keypoints_host,
                     int64_t *response_host, int64_t *n_out, int64_t *n_found)
{
    if (!c || !detect_args_ok(n_octaves, threshold, max_keypoints, keypoints_host, n_out)) return DLCO_ERR_INVALID;
    return guarded(c, [&] { detect(c, n_octaves, threshold, max_keypoints, keypoints_host, response_host, false, n_out, n_found); });
}

// the same into device memory; keypoints_dev is 16-byte aligned (a row is one store)
int dlco_desc_detect_device(dlco_desc_ctx *c, int32_t n_octaves, int64_t threshold, int64_t max_keypoints, float *keypoints_dev,
                            int64_t *response_dev, int64_t *n_out, int64_t *n_found)
{
    if (!c || !detect_args_ok(n_octaves, threshold, max_keypoints, keypoints_dev, n_out)) return DLCO_ERR_INVALID;
    if ((uintptr_t)keypoints_dev % 16 != 0 || (uintptr_t)response_dev % 8 != 0) return DLCO_ERR_INVALID;
    return guarded(c, [&] { detect(c, n_octaves, threshold, max_keypoints, keypoints_dev, response_dev, true, n_out, n_found); });
}

// dlco_desc_detect with the fourth column filled by the rule of orient_rules.hpp: the orientation kernel runs on the selected
// rows before they leave the device; its time is dlco_desc_last_orient_ms and part of dlco_desc_last_kernel_ms, not of the
// six stages
int dlco_desc_detect_oriented(dlco_desc_ctx *c, int32_t n_octaves, int64_t threshold, int64_t max_keypoints, float *keypoints_host,
                              int64_t *response_host, int64_t *n_out, int64_t *n_found)
{
    if (!c || !detect_args_ok(n_octaves, threshold, max_keypoints, keypoints_host, n_out)) return DLCO_ERR_INVALID;
    return guarded(c, [&] { detect(c, n_octaves, threshold, max_keypoints, keypoints_host, response_host, false, n_out, n_found, true); });
}

// angles [n] of keypoints [n][4] on the image set, by the rule of orient_rules.hpp; vectors [n][2] and status [n] may be NULL
int dlco_desc_orient(dlco_desc_ctx *c, const float *keypoints_host, int64_t n, float *angles_host, int64_t *vectors_host, uint8_t *status_host)
{
    if (!c || !keypoints_host || !angles_host || n < 1) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_CHECK(c->img, DLCO_ERR_INVALID, "dlco_desc: set an image first");
        DLCO_HIP(hipSetDevice(c->device));
        EventPair ev;
        const double integral_ms = integral_image(c, ev);
        c->o_kp.alloc((size_t)n * 4);
        DLCO_HIP(hipMemcpyAsync(c->o_kp.p, keypoints_host, (size_t)n * 4 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        orient_rows(c, ev, c->o_kp.p, n, angles_host, 1, vectors_host, status_host);
        c->last_ms = integral_ms + c->o_ms;
    });
}

double dlco_desc_last_orient_ms(const dlco_desc_ctx *c) { return c ? c->o_ms : 0.0; }

// milliseconds of the last detect call by stage: ms[0] the integral image (0 when it was cached), ms[1 .. 4] the octaves,
// ms[5] the selection; their sum is dlco_desc_last_kernel_ms
int dlco_desc_detect_stage_ms(const dlco_desc_ctx *c, double *ms)
{
    if (!c || !ms) return DLCO_ERR_INVALID;
    for (int i = 0; i < 2 + detect_rules::kMaxOctaves; i++) ms[i] = c->d_stage_ms[i];
    return DLCO_OK;
}

namespace {
// The table Y [n_patches, r] of every patch's learnt descriptor (128 MB at 500k x 64) and, from it, the squared distance
// and label of every pair, all in device memory: what eval-fpr95 gets out of an N x F "-unproj" file, without that matrix.
struct PairDists {
    DevBuf<float> Y, dist;
    DevBuf<uint8_t> label;
    DevBuf<int32_t> pairs;
};
void projected_pair_dists(dlco_desc_ctx *c, const uint8_t *patches_host, int64_t n_patches, const int32_t *pairs_host, int64_t n_pairs,
                          PairDists &w)
{
    DLCO_CHECK(c->nsel > 0, DLCO_ERR_INVALID, "dlco_desc: set the filters first");
    DLCO_CHECK(c->r > 0 && c->proj_F == c->nsel * kBins, DLCO_ERR_INVALID, "dlco_desc: set a projection that fits the filters first");
    DLCO_CHECK(n_pairs <= (int64_t)0x7fffffff / 4, DLCO_ERR_INVALID, "dlco_desc: too many pairs for one call");
    check_pairs(pairs_host, n_pairs, n_patches);
    DLCO_HIP(hipSetDevice(c->device));
    w.Y.alloc((size_t)n_patches * c->r);
    w.dist.alloc((size_t)n_pairs);
    w.label.alloc((size_t)n_pairs);
    w.pairs.alloc((size_t)n_pairs * 4);
    compute(c, PatchSource::patches(patches_host), n_patches, RowsOut::projected(w.Y.p, Where::Device, (long)c->r));
    EventPair ev;
    DLCO_HIP(hipMemcpyAsync(w.pairs.p, pairs_host, (size_t)n_pairs * 4 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    c->last_ms += timed_ms(c, ev, [&] { desc_pair_sqdist(w.Y.p, c->r, c->r, w.pairs.p, n_pairs, w.dist.p, w.label.p, c->stream); });
}
}  // namespace

// per pair ||Y[a] - Y[b]||^2 and Label: the distances pj-learn's W gives on comp-uprjdists' rows (ComputePJStats forms
// them as ||W (Desc1 - Desc2)||^2, src/misc.cpp:279-292), computed from the projected descriptors of the patches
int dlco_desc_pair_sqdists(dlco_desc_ctx *c, const uint8_t *patches_host, int64_t n_patches, const int32_t *pairs_host, int64_t n_pairs,
                           float *dist_host, uint8_t *label_host)
{
    if (!c || !patches_host || !pairs_host || !dist_host || n_patches < 1 || n_pairs < 1) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        PairDists w;
        projected_pair_dists(c, patches_host, n_patches, pairs_host, n_pairs, w);
        DLCO_HIP(hipMemcpyAsync(dist_host, w.dist.p, (size_t)n_pairs * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (label_host) DLCO_HIP(hipMemcpyAsync(label_host, w.label.p, (size_t)n_pairs, hipMemcpyDeviceToHost, c->stream));
        sync(c);
    });
}

// ComputePJStats (src/misc.cpp:266-333) on those distances: FPR at 95 % recall and the area under the ROC curve by the
// trainer's own routine (kernels_stats.hip); dim counts the rows of W that have a non-zero entry (S1, :269-277)
int dlco_desc_pair_stats(dlco_desc_ctx *c, const uint8_t *patches_host, int64_t n_patches, const int32_t *pairs_host, int64_t n_pairs,
                         int32_t *dim, float *fpr95, double *auc)
{
    if (!c || !patches_host || !pairs_host || !fpr95 || !auc || n_patches < 1 || n_pairs < 1) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        PairDists w;
        projected_pair_dists(c, patches_host, n_patches, pairs_host, n_pairs, w);
        RocWork *roc = roc_work_create((int)n_pairs);
        try { roc_stats(roc, w.dist.p, w.label.p, (int)n_pairs, fpr95, auc, c->stream); } catch (...) { roc_work_destroy(roc); throw; }
        roc_work_destroy(roc);
        if (dim) *dim = c->proj_dim;
    });
}

// ---- matching: the float entry points; the host path they share with the byte ones is with compute(), outside extern "C" ----
int dlco_desc_match(dlco_desc_ctx *c, const float *query_host, int64_t nq, const float *train_host, int64_t nt, int32_t r, int32_t *idx_host,
                    float *sqdist_host)
{
    if (!c || !match_args_ok(query_host, train_host, idx_host, sqdist_host, nq, nt, r)) return DLCO_ERR_INVALID;
    return guarded(c, [&] { match_host<FloatLine>(c, query_host, nq, train_host, nt, r, idx_host, sqdist_host, nullptr); });
}

int dlco_desc_match_device(dlco_desc_ctx *c, const float *query_dev, int64_t ldq, int64_t nq, const float *train_dev, int64_t ldt, int64_t nt,
                           int32_t r, int32_t *idx_dev, float *sqdist_dev)
{
    if (!c || !match_args_ok(query_dev, train_dev, idx_dev, sqdist_dev, nq, nt, r)) return DLCO_ERR_INVALID;
    if (ldq < r || ldt < r || ldq % 4 != 0 || ldt % 4 != 0) return DLCO_ERR_INVALID;
    if (((uintptr_t)query_dev | (uintptr_t)train_dev) % 16 != 0) return DLCO_ERR_INVALID;          // 16-byte rows
    return guarded(c, [&] { match_device<FloatLine>(c, query_dev, (long)ldq, nq, train_dev, (long)ldt, nt, r, idx_dev, sqdist_dev); });
}

int dlco_desc_cross_sqdists(dlco_desc_ctx *c, const float *query_host, int64_t nq, const float *train_host, int64_t nt, int32_t r,
                            float *out_host)
{
    if (!c || !match_args_ok(query_host, train_host, out_host, out_host, nq, nt, r)) return DLCO_ERR_INVALID;
    if (nq > ((int64_t)1 << 28) / nt) return DLCO_ERR_INVALID;
    return guarded(c, [&] { match_host<FloatLine>(c, query_host, nq, train_host, nt, r, nullptr, nullptr, out_host); });
}

// ---- matching many pairs of images in one call (match_batch.hpp); the float entry points and the two that take no line ----
int dlco_desc_match_pairs_rows(const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs, int64_t *row0)
{
    if (!row0 || !match_pairs_args_ok(seg, n_img, pairs, n_pairs)) return DLCO_ERR_INVALID;
    match_batch::row_offsets(seg, pairs, n_pairs, row0);
    return DLCO_OK;
}

int dlco_desc_match_pairs(dlco_desc_ctx *c, const float *table_host, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs,
                          int32_t r, int32_t *idx_host, float *sqdist_host)
{
    if (!c || !table_host || !idx_host || !sqdist_host || r < 1 || r > 1024 || !match_pairs_args_ok(seg, n_img, pairs, n_pairs))
        return DLCO_ERR_INVALID;
    return guarded(c, [&] { match_pairs_host<FloatLine>(c, table_host, seg, n_img, pairs, n_pairs, r, idx_host, sqdist_host); });
}

int dlco_desc_match_pairs_device(dlco_desc_ctx *c, const float *table_dev, int64_t ld, const int64_t *seg, int32_t n_img, const int32_t *pairs,
                                 int64_t n_pairs, int32_t r, int32_t *idx_dev, float *sqdist_dev)
{
    if (!c || !table_dev || !idx_dev || !sqdist_dev || r < 1 || r > 1024 || !match_pairs_args_ok(seg, n_img, pairs, n_pairs))
        return DLCO_ERR_INVALID;
    if (ld < r || ld % 4 != 0 || (uintptr_t)table_dev % 16 != 0) return DLCO_ERR_INVALID;                  // 16-byte rows
    return guarded(c, [&] { match_pairs_device<FloatLine>(c, table_dev, (long)ld, seg, n_img, pairs, n_pairs, r, idx_dev, sqdist_dev); });
}

int dlco_desc_match_pairs_slices(dlco_desc_ctx *c, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs, int32_t u8,
                                 int32_t *slices)
{
    if (!c || !slices || (u8 != 0 && u8 != 1) || !match_pairs_args_ok(seg, n_img, pairs, n_pairs)) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        const match_batch::Plan pl = match_batch::plan(u8 ? ByteLine::shape : FloatLine::shape, seg, pairs, n_pairs, c->n_cu);
        std::copy(pl.slices.begin(), pl.slices.end(), slices);
    });
}

// ---- selecting matches from a batched answer (select_rules.hpp): the float line; the byte line is with the other _u8 calls ----
int dlco_desc_select_pairs(dlco_desc_ctx *c, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs, const int32_t *idx_host,
                           const float *sqdist_host, float ratio, const int32_t *back_idx_host, const int64_t *back_row0, int64_t n_back_rows,
                           const float *xy_host, int64_t *moff, int32_t *matches_host, float *dist_host, float *src_xy_host, float *dst_xy_host)
{
    return select_pairs_host_call<float>(c, SelectArgs{seg, n_img, pairs, n_pairs, ratio, back_row0, n_back_rows, moff}, idx_host, sqdist_host,
                                         back_idx_host, xy_host, matches_host, dist_host, src_xy_host, dst_xy_host);
}

int dlco_desc_select_pairs_device(dlco_desc_ctx *c, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs, const int32_t *idx_dev,
                                  const float *sqdist_dev, float ratio, const int32_t *back_idx_dev, const int64_t *back_row0, int64_t n_back_rows,
                                  const float *xy_dev, int64_t ldxy, int64_t *moff, int32_t *matches_dev, float *dist_dev, float *src_xy_dev,
                                  float *dst_xy_dev)
{
    return select_pairs_device_call<float>(c, SelectArgs{seg, n_img, pairs, n_pairs, ratio, back_row0, n_back_rows, moff}, idx_dev, sqdist_dev,
                                           back_idx_dev, xy_dev, ldxy, matches_dev, dist_dev, src_xy_dev, dst_xy_dev);
}

// ---- guided matching: the nearest two among the rows a two-view model admits: a homography (guided_rules.hpp) or a
// fundamental matrix (guided_epipolar_rules.hpp; records on both sides), the guided epilogue of the tile loop in
// kernels_match.hip and kernels_match_u8.hip.  Either line's host path with a Geometry: the calls below are one body per
// form (host, device, matrix) over the line, and the model is an argument. ------------------------------------------------------
extern "C++" {
namespace {
bool guided_args_ok(const float *qxy, const float *txy, const double *H, float radius, int32_t h_side)
{
    if (!qxy || !txy || !H || !std::isfinite(radius) || !(radius > 0.0f) || (h_side != 0 && h_side != 1)) return false;
    for (int i = 0; i < 9; i++)
        if (!std::isfinite(H[i])) return false;
    return true;
}

// a device table of the line: rows of at least r elements at a pitch of whole 16-byte pieces, 16-byte aligned
template <typename L>
bool device_table_ok(const typename L::Elem *table, int64_t ld, int32_t r)
{
    return ld >= r && ld % (kRowPitchBytes / (int64_t)sizeof(typename L::Elem)) == 0 && (uintptr_t)table % 16 == 0;
}

template <typename L>
int match_guided_call(dlco_desc_ctx *c, const typename L::Elem *query_host, const float *query_xy_host, int64_t nq,
                      const typename L::Elem *train_host, const float *train_xy_host, int64_t nt, int32_t r, const double *M, float radius,
                      int32_t side, int model, int32_t *idx_host, typename L::Dist *sqdist_host)
{
    if (!c || !match_args_ok(query_host, train_host, idx_host, sqdist_host, nq, nt, r)) return DLCO_ERR_INVALID;
    if (!guided_args_ok(query_xy_host, train_xy_host, M, radius, side)) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        const Geometry geo{query_xy_host, 2, train_xy_host, 2, M, verify_rules::threshold_sq(radius), side, model};
        match_host<L>(c, query_host, nq, train_host, nt, r, idx_host, sqdist_host, nullptr, &geo);
    });
}

template <typename L>
int match_guided_device_call(dlco_desc_ctx *c, const typename L::Elem *query_dev, int64_t ldq, const float *query_xy_dev, int64_t ldxy_q,
                             int64_t nq, const typename L::Elem *train_dev, int64_t ldt, const float *train_xy_dev, int64_t ldxy_t, int64_t nt,
                             int32_t r, const double *M, float radius, int32_t side, int model, int32_t *idx_dev, typename L::Dist *sqdist_dev)
{
    if (!c || !match_args_ok(query_dev, train_dev, idx_dev, sqdist_dev, nq, nt, r)) return DLCO_ERR_INVALID;
    if (!device_table_ok<L>(query_dev, ldq, r) || !device_table_ok<L>(train_dev, ldt, r)) return DLCO_ERR_INVALID;
    if (!guided_args_ok(query_xy_dev, train_xy_dev, M, radius, side) || ldxy_q < 2 || ldxy_t < 2) return DLCO_ERR_INVALID;
    if (((uintptr_t)query_xy_dev | (uintptr_t)train_xy_dev) % 4 != 0) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        const Geometry geo{query_xy_dev, (long)ldxy_q, train_xy_dev, (long)ldxy_t, M, verify_rules::threshold_sq(radius), side, model};
        match_device<L>(c, query_dev, (long)ldq, nq, train_dev, (long)ldt, nt, r, idx_dev, sqdist_dev, &geo);
    });
}

template <typename L>
int cross_guided_call(dlco_desc_ctx *c, const typename L::Elem *query_host, const float *query_xy_host, int64_t nq,
                      const typename L::Elem *train_host, const float *train_xy_host, int64_t nt, int32_t r, const double *M, float radius,
                      int32_t side, int model, typename L::Dist *out_host)
{
    if (!c || !match_args_ok(query_host, train_host, out_host, out_host, nq, nt, r)) return DLCO_ERR_INVALID;
    if (nq > ((int64_t)1 << 28) / nt) return DLCO_ERR_INVALID;
    if (!guided_args_ok(query_xy_host, train_xy_host, M, radius, side)) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        const Geometry geo{query_xy_host, 2, train_xy_host, 2, M, verify_rules::threshold_sq(radius), side, model};
        match_host<L>(c, query_host, nq, train_host, nt, r, nullptr, nullptr, out_host, &geo);
    });
}

// guided matching of many pairs in one call: the batch path with a PairsGeometry; a matrix per pair, one radius or threshold
// and one side per call
bool pairs_guided_args_ok(const float *xy, const double *M, int64_t n_pairs, float radius, int32_t side)
{
    if (!xy || !M || !std::isfinite(radius) || !(radius > 0.0f) || (side != 0 && side != 1)) return false;
    for (int64_t i = 0; i < 9 * n_pairs; i++)
        if (!std::isfinite(M[i])) return false;
    return true;
}

template <typename L>
int match_pairs_guided_call(dlco_desc_ctx *c, const typename L::Elem *table_host, const float *xy_host, const int64_t *seg, int32_t n_img,
                            const int32_t *pairs, int64_t n_pairs, int32_t r, const double *M, float radius, int32_t side, int model,
                            int32_t *idx_host, typename L::Dist *sqdist_host)
{
    if (!c || !table_host || !idx_host || !sqdist_host || r < 1 || r > 1024 || !match_pairs_args_ok(seg, n_img, pairs, n_pairs))
        return DLCO_ERR_INVALID;
    if (!pairs_guided_args_ok(xy_host, M, n_pairs, radius, side)) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        const PairsGeometry geo{xy_host, 2, M, verify_rules::threshold_sq(radius), side, model};
        match_pairs_host<L>(c, table_host, seg, n_img, pairs, n_pairs, r, idx_host, sqdist_host, &geo);
    });
}

template <typename L>
int match_pairs_guided_device_call(dlco_desc_ctx *c, const typename L::Elem *table_dev, int64_t ld, const float *xy_dev, int64_t ldxy,
                                   const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs, int32_t r, const double *M,
                                   float radius, int32_t side, int model, int32_t *idx_dev, typename L::Dist *sqdist_dev)
{
    if (!c || !table_dev || !idx_dev || !sqdist_dev || r < 1 || r > 1024 || !match_pairs_args_ok(seg, n_img, pairs, n_pairs))
        return DLCO_ERR_INVALID;
    if (!device_table_ok<L>(table_dev, ld, r)) return DLCO_ERR_INVALID;
    if (!pairs_guided_args_ok(xy_dev, M, n_pairs, radius, side) || ldxy < 2 || (uintptr_t)xy_dev % 4 != 0) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        const PairsGeometry geo{xy_dev, (long)ldxy, M, verify_rules::threshold_sq(radius), side, model};
        match_pairs_device<L>(c, table_dev, (long)ld, seg, n_img, pairs, n_pairs, r, idx_dev, sqdist_dev, &geo);
    });
}
}  // namespace
}  // extern "C++"

// the float line: a homography, a fundamental matrix, and their forms for many pairs
int dlco_desc_match_guided(dlco_desc_ctx *c, const float *query_host, const float *query_xy_host, int64_t nq, const float *train_host,
        const float *train_xy_host, int64_t nt, int32_t r, const double *H, float radius, int32_t h_side, int32_t *idx_host, float *sqdist_host)
{
    return match_guided_call<FloatLine>(c, query_host, query_xy_host, nq, train_host, train_xy_host, nt, r, H, radius, h_side, kGuideHomography, idx_host,
                                  sqdist_host);
}

int dlco_desc_match_guided_device(dlco_desc_ctx *c, const float *query_dev, int64_t ldq, const float *query_xy_dev, int64_t ldxy_q, int64_t nq,
        const float *train_dev, int64_t ldt, const float *train_xy_dev, int64_t ldxy_t, int64_t nt, int32_t r, const double *H, float radius,
        int32_t h_side, int32_t *idx_dev, float *sqdist_dev)
{
    return match_guided_device_call<FloatLine>(c, query_dev, ldq, query_xy_dev, ldxy_q, nq, train_dev, ldt, train_xy_dev, ldxy_t, nt, r, H, radius,
                                         h_side, kGuideHomography, idx_dev, sqdist_dev);
}

int dlco_desc_cross_sqdists_guided(dlco_desc_ctx *c, const float *query_host, const float *query_xy_host, int64_t nq, const float *train_host,
        const float *train_xy_host, int64_t nt, int32_t r, const double *H, float radius, int32_t h_side, float *out_host)
{
    return cross_guided_call<FloatLine>(c, query_host, query_xy_host, nq, train_host, train_xy_host, nt, r, H, radius, h_side, kGuideHomography, out_host);
}

int dlco_desc_match_guided_epipolar(dlco_desc_ctx *c, const float *query_host, const float *query_xy_host, int64_t nq, const float *train_host,
        const float *train_xy_host, int64_t nt, int32_t r, const double *F, float threshold, int32_t f_side, int32_t *idx_host, float *sqdist_host)
{
    return match_guided_call<FloatLine>(c, query_host, query_xy_host, nq, train_host, train_xy_host, nt, r, F, threshold, f_side, kGuideFundamental, idx_host,
                                  sqdist_host);
}

int dlco_desc_match_guided_epipolar_device(dlco_desc_ctx *c, const float *query_dev, int64_t ldq, const float *query_xy_dev, int64_t ldxy_q, int64_t nq,
        const float *train_dev, int64_t ldt, const float *train_xy_dev, int64_t ldxy_t, int64_t nt, int32_t r, const double *F, float threshold,
        int32_t f_side, int32_t *idx_dev, float *sqdist_dev)
{
    return match_guided_device_call<FloatLine>(c, query_dev, ldq, query_xy_dev, ldxy_q, nq, train_dev, ldt, train_xy_dev, ldxy_t, nt, r, F, threshold,
                                         f_side, kGuideFundamental, idx_dev, sqdist_dev);
}

int dlco_desc_cross_sqdists_guided_epipolar(dlco_desc_ctx *c, const float *query_host, const float *query_xy_host, int64_t nq, const float *train_host,
        const float *train_xy_host, int64_t nt, int32_t r, const double *F, float threshold, int32_t f_side, float *out_host)
{
    return cross_guided_call<FloatLine>(c, query_host, query_xy_host, nq, train_host, train_xy_host, nt, r, F, threshold, f_side, kGuideFundamental, out_host);
}

int dlco_desc_match_pairs_guided(dlco_desc_ctx *c, const float *table_host, const float *xy_host, const int64_t *seg, int32_t n_img,
        const int32_t *pairs, int64_t n_pairs, int32_t r, const double *H, float radius, int32_t h_side, int32_t *idx_host, float *sqdist_host)
{
    return match_pairs_guided_call<FloatLine>(c, table_host, xy_host, seg, n_img, pairs, n_pairs, r, H, radius, h_side, kGuideHomography, idx_host,
                                        sqdist_host);
}

int dlco_desc_match_pairs_guided_device(dlco_desc_ctx *c, const float *table_dev, int64_t ld, const float *xy_dev, int64_t ldxy, const int64_t *seg,
        int32_t n_img, const int32_t *pairs, int64_t n_pairs, int32_t r, const double *H, float radius, int32_t h_side, int32_t *idx_dev,
        float *sqdist_dev)
{
    return match_pairs_guided_device_call<FloatLine>(c, table_dev, ld, xy_dev, ldxy, seg, n_img, pairs, n_pairs, r, H, radius, h_side, kGuideHomography,
                                               idx_dev, sqdist_dev);
}

int dlco_desc_match_pairs_guided_epipolar(dlco_desc_ctx *c, const float *table_host, const float *xy_host, const int64_t *seg, int32_t n_img,
        const int32_t *pairs, int64_t n_pairs, int32_t r, const double *F, float threshold, int32_t f_side, int32_t *idx_host, float *sqdist_host)
{
    return match_pairs_guided_call<FloatLine>(c, table_host, xy_host, seg, n_img, pairs, n_pairs, r, F, threshold, f_side, kGuideFundamental, idx_host,
                                        sqdist_host);
}

int dlco_desc_match_pairs_guided_epipolar_device(dlco_desc_ctx *c, const float *table_dev, int64_t ld, const float *xy_dev, int64_t ldxy, const int64_t *seg,
        int32_t n_img, const int32_t *pairs, int64_t n_pairs, int32_t r, const double *F, float threshold, int32_t f_side, int32_t *idx_dev,
        float *sqdist_dev)
{
    return match_pairs_guided_device_call<FloatLine>(c, table_dev, ld, xy_dev, ldxy, seg, n_img, pairs, n_pairs, r, F, threshold, f_side, kGuideFundamental,
                                               idx_dev, sqdist_dev);
}

// the byte line: the same calls on byte tables, integer distances and pitches in bytes
int dlco_desc_match_guided_u8(dlco_desc_ctx *c, const uint8_t *query_host, const float *query_xy_host, int64_t nq, const uint8_t *train_host,
        const float *train_xy_host, int64_t nt, int32_t r, const double *H, float radius, int32_t h_side, int32_t *idx_host, int32_t *sqdist_host)
{
    return match_guided_call<ByteLine>(c, query_host, query_xy_host, nq, train_host, train_xy_host, nt, r, H, radius, h_side, kGuideHomography, idx_host,
                                  sqdist_host);
}

int dlco_desc_match_guided_u8_device(dlco_desc_ctx *c, const uint8_t *query_dev, int64_t ldq, const float *query_xy_dev, int64_t ldxy_q, int64_t nq,
        const uint8_t *train_dev, int64_t ldt, const float *train_xy_dev, int64_t ldxy_t, int64_t nt, int32_t r, const double *H, float radius,
        int32_t h_side, int32_t *idx_dev, int32_t *sqdist_dev)
{
    return match_guided_device_call<ByteLine>(c, query_dev, ldq, query_xy_dev, ldxy_q, nq, train_dev, ldt, train_xy_dev, ldxy_t, nt, r, H, radius,
                                         h_side, kGuideHomography, idx_dev, sqdist_dev);
}

int dlco_desc_cross_sqdists_guided_u8(dlco_desc_ctx *c, const uint8_t *query_host, const float *query_xy_host, int64_t nq, const uint8_t *train_host,
        const float *train_xy_host, int64_t nt, int32_t r, const double *H, float radius, int32_t h_side, int32_t *out_host)
{
    return cross_guided_call<ByteLine>(c, query_host, query_xy_host, nq, train_host, train_xy_host, nt, r, H, radius, h_side, kGuideHomography, out_host);
}

int dlco_desc_match_guided_epipolar_u8(dlco_desc_ctx *c, const uint8_t *query_host, const float *query_xy_host, int64_t nq, const uint8_t *train_host,
        const float *train_xy_host, int64_t nt, int32_t r, const double *F, float threshold, int32_t f_side, int32_t *idx_host, int32_t *sqdist_host)
{
    return match_guided_call<ByteLine>(c, query_host, query_xy_host, nq, train_host, train_xy_host, nt, r, F, threshold, f_side, kGuideFundamental, idx_host,
                                  sqdist_host);
}

int dlco_desc_match_guided_epipolar_u8_device(dlco_desc_ctx *c, const uint8_t *query_dev, int64_t ldq, const float *query_xy_dev, int64_t ldxy_q, int64_t nq,
        const uint8_t *train_dev, int64_t ldt, const float *train_xy_dev, int64_t ldxy_t, int64_t nt, int32_t r, const double *F, float threshold,
        int32_t f_side, int32_t *idx_dev, int32_t *sqdist_dev)
{
    return match_guided_device_call<ByteLine>(c, query_dev, ldq, query_xy_dev, ldxy_q, nq, train_dev, ldt, train_xy_dev, ldxy_t, nt, r, F, threshold,
                                         f_side, kGuideFundamental, idx_dev, sqdist_dev);
}

int dlco_desc_cross_sqdists_guided_epipolar_u8(dlco_desc_ctx *c, const uint8_t *query_host, const float *query_xy_host, int64_t nq, const uint8_t *train_host,
        const float *train_xy_host, int64_t nt, int32_t r, const double *F, float threshold, int32_t f_side, int32_t *out_host)
{
    return cross_guided_call<ByteLine>(c, query_host, query_xy_host, nq, train_host, train_xy_host, nt, r, F, threshold, f_side, kGuideFundamental, out_host);
}

int dlco_desc_match_pairs_guided_u8(dlco_desc_ctx *c, const uint8_t *table_host, const float *xy_host, const int64_t *seg, int32_t n_img,
        const int32_t *pairs, int64_t n_pairs, int32_t r, const double *H, float radius, int32_t h_side, int32_t *idx_host, int32_t *sqdist_host)
{
    return match_pairs_guided_call<ByteLine>(c, table_host, xy_host, seg, n_img, pairs, n_pairs, r, H, radius, h_side, kGuideHomography, idx_host,
                                        sqdist_host);
}

int dlco_desc_match_pairs_guided_u8_device(dlco_desc_ctx *c, const uint8_t *table_dev, int64_t ld, const float *xy_dev, int64_t ldxy, const int64_t *seg,
        int32_t n_img, const int32_t *pairs, int64_t n_pairs, int32_t r, const double *H, float radius, int32_t h_side, int32_t *idx_dev,
        int32_t *sqdist_dev)
{
    return match_pairs_guided_device_call<ByteLine>(c, table_dev, ld, xy_dev, ldxy, seg, n_img, pairs, n_pairs, r, H, radius, h_side, kGuideHomography,
                                               idx_dev, sqdist_dev);
}

int dlco_desc_match_pairs_guided_epipolar_u8(dlco_desc_ctx *c, const uint8_t *table_host, const float *xy_host, const int64_t *seg, int32_t n_img,
        const int32_t *pairs, int64_t n_pairs, int32_t r, const double *F, float threshold, int32_t f_side, int32_t *idx_host, int32_t *sqdist_host)
{
    return match_pairs_guided_call<ByteLine>(c, table_host, xy_host, seg, n_img, pairs, n_pairs, r, F, threshold, f_side, kGuideFundamental, idx_host,
                                        sqdist_host);
}

int dlco_desc_match_pairs_guided_epipolar_u8_device(dlco_desc_ctx *c, const uint8_t *table_dev, int64_t ld, const float *xy_dev, int64_t ldxy, const int64_t *seg,
        int32_t n_img, const int32_t *pairs, int64_t n_pairs, int32_t r, const double *F, float threshold, int32_t f_side, int32_t *idx_dev,
        int32_t *sqdist_dev)
{
    return match_pairs_guided_device_call<ByteLine>(c, table_dev, ld, xy_dev, ldxy, seg, n_img, pairs, n_pairs, r, F, threshold, f_side, kGuideFundamental,
                                               idx_dev, sqdist_dev);
}

// The four single calls are the _pairs forms below with one pair, moff = {0, m}, after their own check of the list: their
// outputs are the batch's arrays for one pair.
// H_all [n_hyp][9] and count [n_hyp] of every hypothesis of the rule: what dlco_desc_verify_homography selects from
int dlco_desc_verify_hypotheses(dlco_desc_ctx *c, const float *src_xy_host, const float *dst_xy_host, int64_t m, float threshold, int32_t n_hyp,
                                uint64_t seed, double *H_all_host, int32_t *count_host)
{
    if (!verify_args_ok<Homography>(src_xy_host, dst_xy_host, m, threshold, n_hyp)) return DLCO_ERR_INVALID;
    const int64_t moff[2] = {0, m};
    return verify_pairs_hypotheses_call<Homography>(c, src_xy_host, dst_xy_host, moff, 1, threshold, n_hyp, seed, H_all_host, count_host);
}

// H [9] row-major, the inlier mask [m] (may be NULL), its count and the winning hypothesis (may be NULL); no model is no
// error: H and the mask are zero, *n_inliers = 0, *best_hyp = -1.  The refit's rounds are formed on the host from the mask and
// scored by the mask kernel.
int dlco_desc_verify_homography(dlco_desc_ctx *c, const float *src_xy_host, const float *dst_xy_host, int64_t m, float threshold, int32_t n_hyp,
                                uint64_t seed, int32_t refine, double *H_out, uint8_t *inlier_host, int64_t *n_inliers, int32_t *best_hyp)
{
    if (!verify_args_ok<Homography>(src_xy_host, dst_xy_host, m, threshold, n_hyp)) return DLCO_ERR_INVALID;
    const int64_t moff[2] = {0, m};
    return verify_pairs_model_call<Homography>(c, src_xy_host, dst_xy_host, moff, 1, threshold, n_hyp, seed, refine, H_out, inlier_host, n_inliers,
                                                  best_hyp);
}

// the same two calls for a fundamental matrix F, x'^T F x = 0 (epipolar_rules.hpp), with m >= 8
int dlco_desc_verify_fundamental_hypotheses(dlco_desc_ctx *c, const float *src_xy_host, const float *dst_xy_host, int64_t m, float threshold,
                                            int32_t n_hyp, uint64_t seed, double *F_all_host, int32_t *count_host)
{
    if (!verify_args_ok<Fundamental>(src_xy_host, dst_xy_host, m, threshold, n_hyp)) return DLCO_ERR_INVALID;
    const int64_t moff[2] = {0, m};
    return verify_pairs_hypotheses_call<Fundamental>(c, src_xy_host, dst_xy_host, moff, 1, threshold, n_hyp, seed, F_all_host, count_host);
}

int dlco_desc_verify_fundamental(dlco_desc_ctx *c, const float *src_xy_host, const float *dst_xy_host, int64_t m, float threshold, int32_t n_hyp,
                                 uint64_t seed, int32_t refine, double *F_out, uint8_t *inlier_host, int64_t *n_inliers, int32_t *best_hyp)
{
    if (!verify_args_ok<Fundamental>(src_xy_host, dst_xy_host, m, threshold, n_hyp)) return DLCO_ERR_INVALID;
    const int64_t moff[2] = {0, m};
    return verify_pairs_model_call<Fundamental>(c, src_xy_host, dst_xy_host, moff, 1, threshold, n_hyp, seed, refine, F_out, inlier_host, n_inliers,
                                                   best_hyp);
}

// the four calls over the match lists of many pairs as one list cut by moff [n_pairs + 1]: pair p's answers are the single
// call's on its slice
int dlco_desc_verify_pairs_homography(dlco_desc_ctx *c, const float *src_xy_host, const float *dst_xy_host, const int64_t *moff, int64_t n_pairs,
                                      float threshold, int32_t n_hyp, uint64_t seed, int32_t refine, double *H_out, uint8_t *inlier_host,
                                      int64_t *n_inliers, int32_t *best_hyp)
{
    return verify_pairs_model_call<Homography>(c, src_xy_host, dst_xy_host, moff, n_pairs, threshold, n_hyp, seed, refine, H_out, inlier_host, n_inliers,
                                               best_hyp);
}

int dlco_desc_verify_pairs_fundamental(dlco_desc_ctx *c, const float *src_xy_host, const float *dst_xy_host, const int64_t *moff, int64_t n_pairs,
                                       float threshold, int32_t n_hyp, uint64_t seed, int32_t refine, double *F_out, uint8_t *inlier_host,
                                       int64_t *n_inliers, int32_t *best_hyp)
{
    return verify_pairs_model_call<Fundamental>(c, src_xy_host, dst_xy_host, moff, n_pairs, threshold, n_hyp, seed, refine, F_out, inlier_host, n_inliers,
                                                best_hyp);
}

int dlco_desc_verify_pairs_hypotheses(dlco_desc_ctx *c, const float *src_xy_host, const float *dst_xy_host, const int64_t *moff, int64_t n_pairs,
                                      float threshold, int32_t n_hyp, uint64_t seed, double *H_all_host, int32_t *count_host)
{
    return verify_pairs_hypotheses_call<Homography>(c, src_xy_host, dst_xy_host, moff, n_pairs, threshold, n_hyp, seed, H_all_host, count_host);
}

int dlco_desc_verify_pairs_fundamental_hypotheses(dlco_desc_ctx *c, const float *src_xy_host, const float *dst_xy_host, const int64_t *moff,
                                                  int64_t n_pairs, float threshold, int32_t n_hyp, uint64_t seed, double *F_all_host,
                                                  int32_t *count_host)
{
    return verify_pairs_hypotheses_call<Fundamental>(c, src_xy_host, dst_xy_host, moff, n_pairs, threshold, n_hyp, seed, F_all_host, count_host);
}

// the same on lists in device memory, as dlco_desc_select_pairs_device writes them, with the refit rounds on the device
int dlco_desc_verify_pairs_homography_device(dlco_desc_ctx *c, const float *src_xy_dev, const float *dst_xy_dev, const int64_t *moff, int64_t n_pairs,
                                             float threshold, int32_t n_hyp, uint64_t seed, int32_t refine, double *H_out, uint8_t *inlier_dev,
                                             int64_t *n_inliers, int32_t *best_hyp)
{
    return verify_pairs_device_call<Homography>(c, src_xy_dev, dst_xy_dev, moff, n_pairs, threshold, n_hyp, seed, refine, H_out, inlier_dev, n_inliers,
                                                best_hyp);
}

int dlco_desc_verify_pairs_fundamental_device(dlco_desc_ctx *c, const float *src_xy_dev, const float *dst_xy_dev, const int64_t *moff, int64_t n_pairs,
                                              float threshold, int32_t n_hyp, uint64_t seed, int32_t refine, double *F_out, uint8_t *inlier_dev,
                                              int64_t *n_inliers, int32_t *best_hyp)
{
    return verify_pairs_device_call<Fundamental>(c, src_xy_dev, dst_xy_dev, moff, n_pairs, threshold, n_hyp, seed, refine, F_out, inlier_dev, n_inliers,
                                                 best_hyp);
}

// one round of the refit kernel on the caller's masks: M_out [n_pairs][9] and ok [n_pairs], zero where the round is rejected
int dlco_desc_verify_pairs_refit_round(dlco_desc_ctx *c, const float *src_xy_host, const float *dst_xy_host, const int64_t *moff, int64_t n_pairs,
                                       const uint8_t *mask_host, int32_t fundamental, double *M_out, uint8_t *ok)
{
    if (!c || !src_xy_host || !dst_xy_host || !mask_host || !M_out || !ok || !verify_batch::offsets_ok(moff, n_pairs) ||
        (fundamental != 0 && fundamental != 1))
        return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        if (fundamental) verify_pairs_refit_round_call<Fundamental>(c, src_xy_host, dst_xy_host, moff, n_pairs, mask_host, M_out, ok);
        else verify_pairs_refit_round_call<Homography>(c, src_xy_host, dst_xy_host, moff, n_pairs, mask_host, M_out, ok);
    });
}

// the plan only: the launch of every pair, -1 for a pair that launches nothing; host only
int dlco_desc_verify_pairs_launches(const int64_t *moff, int64_t n_pairs, int32_t n_hyp, int32_t fundamental, int32_t *launch_of_pair)
{
    if (!launch_of_pair || !verify_batch::offsets_ok(moff, n_pairs) || n_hyp < 1 || n_hyp > verify_rules::kMaxHyp || (fundamental != 0 && fundamental != 1))
        return DLCO_ERR_INVALID;
    return guarded(nullptr, [&] {
        const verify_batch::Plan pl = verify_batch::plan(moff, n_pairs, n_hyp, fundamental ? Fundamental::kSample : Homography::kSample);
        std::copy(pl.launch_of_pair.begin(), pl.launch_of_pair.end(), launch_of_pair);
    });
}

// ---- byte descriptors: the quantiser (quant_rules.hpp), the _u8 forms of describe, the match of byte tables -------------------
// o_k = min_i Y[i][k], s = 255 / max_k (max_i Y[i][k] - o_k) or 1: host only
int dlco_desc_quant_fit(const float *Y_host, int64_t n, int32_t r, float *scale, float *offset_out)
{
    if (!Y_host || !scale || !offset_out || n < 1 || r < 1 || r > quant_rules::kMaxDim) return DLCO_ERR_INVALID;
    return quant_rules::fit(Y_host, n, r, scale, offset_out) ? DLCO_OK : DLCO_ERR_INVALID;
}

// bytes [n, r] of Y [n, r] by the rule of quant_rules.hpp: host only
int dlco_desc_quantize(const float *Y_host, int64_t n, int32_t r, float scale, const float *offset, uint8_t *out_u8)
{
    if (!Y_host || !out_u8 || n < 1 || r < 1 || r > quant_rules::kMaxDim || !quant_rules::scale_ok(scale)) return DLCO_ERR_INVALID;
    for (int k = 0; offset && k < r; k++)
        if (!std::isfinite(offset[k])) return DLCO_ERR_INVALID;
    quant_rules::quantize(Y_host, n, r, scale, offset, out_u8);
    return DLCO_OK;
}

int dlco_desc_set_quantizer(dlco_desc_ctx *c, float scale, const float *offset, int32_t r)
{
    if (!c || r < 1 || r > quant_rules::kMaxDim || !quant_rules::scale_ok(scale)) return DLCO_ERR_INVALID;
    for (int k = 0; offset && k < r; k++)
        if (!std::isfinite(offset[k])) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_HIP(hipSetDevice(c->device));
        c->q_r = 0;
        c->q_off.alloc((size_t)r);
        if (offset) DLCO_HIP(hipMemcpyAsync(c->q_off.p, offset, (size_t)r * sizeof(float), hipMemcpyHostToDevice, c->stream));
        else DLCO_HIP(hipMemsetAsync(c->q_off.p, 0, (size_t)r * sizeof(float), c->stream));
        sync(c);
        c->q_scale = scale; c->q_r = r;
    });
}

// dlco_desc_quantize of dlco_desc_describe's rows, quantised on the device
int dlco_desc_describe_u8(dlco_desc_ctx *c, const uint8_t *patches_host, int64_t n, uint8_t *out_host)
{
    if (!c || !patches_host || !out_host || n < 1) return DLCO_ERR_INVALID;
    return guarded(c, [&] { compute(c, PatchSource::patches(patches_host), n, RowsOut::bytes(out_host, Where::Host, (long)c->r)); });
}

int dlco_desc_describe_u8_device(dlco_desc_ctx *c, const uint8_t *patches_host, int64_t n, uint8_t *out_dev, int64_t ld)
{
    if (!c || !patches_host || !out_dev || n < 1) return DLCO_ERR_INVALID;
    return guarded(c, [&] { compute(c, PatchSource::patches(patches_host), n, RowsOut::bytes(out_dev, Where::Device, (long)ld)); });
}

// the same of dlco_desc_describe_keypoints' rows: a row of status 0 is the quantisation of the zero vector
int dlco_desc_describe_keypoints_u8(dlco_desc_ctx *c, const float *keypoints_host, int64_t n, float scale_factor, int32_t use_orientation,
                                    uint8_t *out_host, uint8_t *status_host)
{
    if (!c || !out_host || !keypoint_args_ok(keypoints_host, n, scale_factor)) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        describe_keypoints(c, keypoints_host, n, scale_factor, use_orientation != 0, status_host, RowsOut::bytes(out_host, Where::Host, (long)c->r));
    });
}

int dlco_desc_describe_keypoints_u8_device(dlco_desc_ctx *c, const float *keypoints_host, int64_t n, float scale_factor,
                                           int32_t use_orientation, uint8_t *out_dev, int64_t ld, uint8_t *status_host)
{
    if (!c || !out_dev || !keypoint_args_ok(keypoints_host, n, scale_factor)) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        describe_keypoints(c, keypoints_host, n, scale_factor, use_orientation != 0, status_host, RowsOut::bytes(out_dev, Where::Device, (long)ld));
    });
}

int dlco_desc_match_u8(dlco_desc_ctx *c, const uint8_t *query_u8, int64_t nq, const uint8_t *train_u8, int64_t nt, int32_t r, int32_t *idx_host,
                       int32_t *sqdist_host)
{
    if (!c || !match_args_ok(query_u8, train_u8, idx_host, sqdist_host, nq, nt, r)) return DLCO_ERR_INVALID;
    return guarded(c, [&] { match_host<ByteLine>(c, query_u8, nq, train_u8, nt, r, idx_host, sqdist_host, nullptr); });
}

int dlco_desc_match_u8_device(dlco_desc_ctx *c, const uint8_t *query_dev, int64_t ldq, int64_t nq, const uint8_t *train_dev, int64_t ldt,
                              int64_t nt, int32_t r, int32_t *idx_dev, int32_t *sqdist_dev)
{
    if (!c || !match_args_ok(query_dev, train_dev, idx_dev, sqdist_dev, nq, nt, r)) return DLCO_ERR_INVALID;
    if (ldq < r || ldt < r || ldq % 16 != 0 || ldt % 16 != 0) return DLCO_ERR_INVALID;
    if (((uintptr_t)query_dev | (uintptr_t)train_dev) % 16 != 0) return DLCO_ERR_INVALID;          // 16-byte pieces
    return guarded(c, [&] { match_device<ByteLine>(c, query_dev, (long)ldq, nq, train_dev, (long)ldt, nt, r, idx_dev, sqdist_dev); });
}

int dlco_desc_match_pairs_u8(dlco_desc_ctx *c, const uint8_t *table_u8, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs,
                             int32_t r, int32_t *idx_host, int32_t *sqdist_host)
{
    if (!c || !table_u8 || !idx_host || !sqdist_host || r < 1 || r > 1024 || !match_pairs_args_ok(seg, n_img, pairs, n_pairs))
        return DLCO_ERR_INVALID;
    return guarded(c, [&] { match_pairs_host<ByteLine>(c, table_u8, seg, n_img, pairs, n_pairs, r, idx_host, sqdist_host); });
}

int dlco_desc_match_pairs_u8_device(dlco_desc_ctx *c, const uint8_t *table_dev, int64_t ld, const int64_t *seg, int32_t n_img,
                                    const int32_t *pairs, int64_t n_pairs, int32_t r, int32_t *idx_dev, int32_t *sqdist_dev)
{
    if (!c || !table_dev || !idx_dev || !sqdist_dev || r < 1 || r > 1024 || !match_pairs_args_ok(seg, n_img, pairs, n_pairs))
        return DLCO_ERR_INVALID;
    if (ld < r || ld % 16 != 0 || (uintptr_t)table_dev % 16 != 0) return DLCO_ERR_INVALID;                 // 16-byte pieces
    return guarded(c, [&] { match_pairs_device<ByteLine>(c, table_dev, (long)ld, seg, n_img, pairs, n_pairs, r, idx_dev, sqdist_dev); });
}

int dlco_desc_select_pairs_u8(dlco_desc_ctx *c, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs, const int32_t *idx_host,
                              const int32_t *sqdist_host, float ratio, const int32_t *back_idx_host, const int64_t *back_row0, int64_t n_back_rows,
                              const float *xy_host, int64_t *moff, int32_t *matches_host, int32_t *dist_host, float *src_xy_host, float *dst_xy_host)
{
    return select_pairs_host_call<int32_t>(c, SelectArgs{seg, n_img, pairs, n_pairs, ratio, back_row0, n_back_rows, moff}, idx_host, sqdist_host,
                                           back_idx_host, xy_host, matches_host, dist_host, src_xy_host, dst_xy_host);
}

int dlco_desc_select_pairs_u8_device(dlco_desc_ctx *c, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs,
                                     const int32_t *idx_dev, const int32_t *sqdist_dev, float ratio, const int32_t *back_idx_dev,
                                     const int64_t *back_row0, int64_t n_back_rows, const float *xy_dev, int64_t ldxy, int64_t *moff,
                                     int32_t *matches_dev, int32_t *dist_dev, float *src_xy_dev, float *dst_xy_dev)
{
    return select_pairs_device_call<int32_t>(c, SelectArgs{seg, n_img, pairs, n_pairs, ratio, back_row0, n_back_rows, moff}, idx_dev, sqdist_dev,
                                             back_idx_dev, xy_dev, ldxy, matches_dev, dist_dev, src_xy_dev, dst_xy_dev);
}

int dlco_desc_build_tracks(dlco_desc_ctx *c, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs, const int64_t *moff,
                           const int32_t *matches_host, const uint8_t *keep_host, int32_t min_len, int32_t unique, int64_t *n_tracks, int64_t *toff_host,
                           int32_t *obs_host, int32_t *track_of_host, int32_t *label_host, int64_t counts[3])
{
    return build_tracks_host_call(c, TracksArgs{seg, n_img, pairs, n_pairs, moff, min_len, unique, n_tracks, counts}, matches_host, keep_host, toff_host,
                                  obs_host, track_of_host, label_host);
}

int dlco_desc_build_tracks_device(dlco_desc_ctx *c, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs, const int64_t *moff,
                                  const int32_t *matches_dev, const uint8_t *keep_dev, int32_t min_len, int32_t unique, int64_t *n_tracks,
                                  int64_t *toff_dev, int32_t *obs_dev, int32_t *track_of_dev, int32_t *label_dev, int64_t counts[3])
{
    return build_tracks_device_call(c, TracksArgs{seg, n_img, pairs, n_pairs, moff, min_len, unique, n_tracks, counts}, matches_dev, keep_dev, toff_dev,
                                    obs_dev, track_of_dev, label_dev);
}

int dlco_desc_cross_sqdists_u8(dlco_desc_ctx *c, const uint8_t *query_u8, int64_t nq, const uint8_t *train_u8, int64_t nt, int32_t r,
                               int32_t *out_host)
{
    if (!c || !match_args_ok(query_u8, train_u8, out_host, out_host, nq, nt, r)) return DLCO_ERR_INVALID;
    if (nq > ((int64_t)1 << 28) / nt) return DLCO_ERR_INVALID;
    return guarded(c, [&] { match_host<ByteLine>(c, query_u8, nq, train_u8, nt, r, nullptr, nullptr, out_host); });
}

// milliseconds the kernels of the last dlco_desc_compute* / dlco_desc_describe* call took (HIP events): transform and
// pooling, plus the projection for describe and the sampling for the keypoint calls (extract_patches: the sampling alone);
// the pair calls add their distance kernel; after a match call, float or byte, its kernels (norms, top two, merge, and for
// the guided forms, float or byte, single or many pairs, the record kernels: norms, record kernels, tile loop, merge); the _u8
// forms of describe add their quantising kernel; after an orient call the orientation kernel and the integral image when the
// call formed it; after a detect call the detector's kernels (the integral image when the call
// formed it, the octaves, the selection); after a verify or verify_pairs call every kernel of every launch of the call: for
// the _hypotheses forms the hypotheses and the scoring, for the model forms these, the selection, the mask of the best models
// and the mask launches of the lockstep refit rounds; after a select_pairs call its four kernels (flag, scan, scatter, offsets);
// after a build_tracks call its kernels and the sort between them
double dlco_desc_last_kernel_ms(const dlco_desc_ctx *c) { return c ? c->last_ms : 0.0; }

}  // extern "C"
