// kernels_verify.hip — geometric verification of match lists against a two-view model: the homography
// (dlco_desc_verify_homography, dlco_desc_verify_hypotheses and their _pairs forms; verify_rules::Homography) or the
// fundamental matrix (dlco_desc_verify_fundamental, dlco_desc_verify_fundamental_hypotheses and their _pairs forms;
// epipolar_rules::Fundamental).  The rules are verify_rules.hpp and epipolar_rules.hpp, where they are stated; this file only
// decides where the numbers are read from and in which order the work is done, once for every Model.  Every floating-point
// operation is the headers' (contraction off there), every sum is of integers.
//
// One kernel set.  It runs the entries of one launch of verify_batch.hpp's plan: many pairs of one segmented match list, or
// the one pair of a single call, whose launch has one entry.  The entry at position e of the launch owns slot e of every
// device array.  The functions of the rule headers are called on the pair's own base pointers and match count, so a pair's
// numbers do not depend on its neighbours.
//   hyp_pairs_kernel<Model>    one lane per (entry, hypothesis): its sample, its model, M_all [e][n_hyp][9] (all zero when
//                              invalid); every entry has the same ceil(n_hyp / kHypLanes) workgroups of kHypLanes<Model>.  For
//                              the fundamental matrix that is the 8 x 9 system eliminated with complete pivoting.  The system
//                              lives in registers: the header's loops unroll to constant indices and every run-time pivot is a
//                              predicated swap, so there is no scratch.
//   score_pairs_kernel<Model>  the hot loop, on a 1-D grid of workgroups of 256: a workgroup is (entry, block of 256
//                              hypotheses, chunk of kScoreChunk matches), the block the faster index; it finds its entry by a
//                              scalar binary search over swg0.  A lane owns one hypothesis and keeps its M in registers (9
//                              doubles).  The chunk's matches are widened to double once and staged in LDS as (x, y, u, v), 8 KB;
//                              in the loop every lane reads the same address, an LDS broadcast without conflicts: two 16-byte
//                              reads and about 19 (homography) or 33 (fundamental matrix) fp64 operations per (hypothesis,
//                              match).  A private int32 counter per lane, one integer atomicAdd per (hypothesis, chunk) into
//                              count [e][h]: integer sums do not depend on the order, so neither on the chunking.
//   select_pairs_kernel        one workgroup per entry: the maximum of the key (count << 32) | (0xFFFFFFFF - h) and, with no
//                              host round trip, the winning matrix in M_cur [e] (zero when the best count is 0).
//   mask_pairs_kernel<Model>   one lane per match: a workgroup is (active entry, 256 matches of it), found by the same search
//                              over the active list; M_cur [e] comes from device memory; the u8 trial mask at the entry's
//                              matches, the count by a ballot and one atomicAdd per wave into n [e].
#include "dlco_internal.hpp"
#include "epipolar_rules.hpp"

namespace dlco {

namespace {

namespace vr = verify_rules;
namespace vb = verify_batch;

constexpr int VTH = 256;
constexpr int VSEL = 1024;                                  // lanes of the selection's one workgroup

// lanes of a workgroup of the hypothesis kernel: 64 for the eight-point model, so that a lane may hold the 72 doubles of
// its system and the compiler need not spill
template <typename Model> constexpr int kHypLanes = VTH;
template <> constexpr int kHypLanes<epipolar_rules::Fundamental> = 64;

// the position of the last item whose first workgroup (first(item)) is not above wg; wg is the same for the whole workgroup,
// so the search is scalar loads and branches
template <typename Item, typename First>
__device__ __forceinline__ int pairs_item_of(const Item *__restrict__ items, int n, long wg, First first)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long)first(items[mid]) <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

template <typename Model>
__global__ __launch_bounds__(kHypLanes<Model>) void hyp_pairs_kernel(const float *src, const float *dst, const vb::Entry *__restrict__ ent,
                                                                     unsigned long long seed, int n_hyp, int hblocks, double *M_all)
{
    const int e = blockIdx.x / hblocks;
    const int h = (blockIdx.x - e * hblocks) * kHypLanes<Model> + threadIdx.x;
    if (h >= n_hyp) return;
    const vb::Entry en = ent[e];
    int32_t idx[Model::kSample];
    double M[9];
    Model::hypothesis(src + 2 * en.m0, dst + 2 * en.m0, (unsigned)en.m, seed, (uint32_t)h, idx, M);
    double *out = M_all + 9 * ((long)e * n_hyp + h);
    for (int i = 0; i < 9; i++) out[i] = M[i];
}

// workgroup wg_base + blockIdx.x of the launch's scoring grid: wg_base is 0 unless one entry's grid is walked in pieces
template <typename Model>
__global__ __launch_bounds__(VTH) void score_pairs_kernel(const float2 *src, const float2 *dst, const vb::Entry *__restrict__ ent, int n_ent,
                                                          const double *M_all, int n_hyp, int hblocks, double t2, int *count, long wg_base)
{
    __shared__ double4 pts[vr::kScoreChunk];
    static_assert(vr::kScoreChunk == VTH && vb::kLanes == VTH, "a lane stages one match of the chunk; the plan counts blocks of VTH");
    const long wg = wg_base + blockIdx.x;
    const int e = pairs_item_of(ent, n_ent, wg, [](const vb::Entry &x) { return x.swg0; });
    const vb::Entry en = ent[e];
    const long w = wg - en.swg0;
    const long chunk = w / hblocks;
    const int h = (int)(w - chunk * hblocks) * VTH + threadIdx.x;
    const long i0 = en.m0 + chunk * vr::kScoreChunk;
    const int cnt = (int)min((long)vr::kScoreChunk, en.m0 + en.m - i0);
    if ((int)threadIdx.x < cnt) {
        const float2 s = src[i0 + threadIdx.x], d = dst[i0 + threadIdx.x];
        pts[threadIdx.x] = make_double4((double)s.x, (double)s.y, (double)d.x, (double)d.y);
    }
    const long slot = (long)e * n_hyp + h;
    double M[9];
    for (int i = 0; i < 9; i++) M[i] = h < n_hyp ? M_all[9 * slot + i] : 0.0;
    __syncthreads();
    int n = 0;
    for (int j = 0; j < cnt; j++) {
        const double4 p = pts[j];
        n += Model::inlier(M, p.x, p.y, p.z, p.w, t2) ? 1 : 0;
    }
    if (h < n_hyp && n > 0) atomicAdd(&count[slot], n);
}

__global__ __launch_bounds__(VSEL) void select_pairs_kernel(const int *count, const double *M_all, int n_hyp, unsigned long long *best, double *M_cur)
{
    __shared__ unsigned long long part[VSEL / 64];
    const long e = blockIdx.x;
    const int *cnt = count + e * n_hyp;
    unsigned long long key = 0;
    for (int h = threadIdx.x; h < n_hyp; h += VSEL) {
        const unsigned long long k = vr::select_key(cnt[h], (uint32_t)h);
        key = k > key ? k : key;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long other = __shfl_xor(key, d);
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = key;
    __syncthreads();
    for (int w = 0; w < VSEL / 64; w++) key = part[w] > key ? part[w] : key;
    if (threadIdx.x == 0) best[e] = key;
    if (threadIdx.x < 9) {
        const bool any = vr::key_count(key) > 0;
        M_cur[9 * e + threadIdx.x] = any ? M_all[9 * (e * n_hyp + vr::key_hyp(key)) + threadIdx.x] : 0.0;
    }
}

template <typename Model>
__global__ __launch_bounds__(VTH) void mask_pairs_kernel(const float2 *src, const float2 *dst, const vb::Entry *__restrict__ ent,
                                                         const vb::Active *__restrict__ active, int n_active, const double *M_cur, double t2,
                                                         uint8_t *mask, int *count, const uint8_t *live)
{
    const long wg = blockIdx.x;
    const vb::Active a = active[pairs_item_of(active, n_active, wg, [](const vb::Active &x) { return x.wg0; })];
    if (live && !live[a.entry]) return;                     // the same for the whole workgroup
    const vb::Entry en = ent[a.entry];
    const long i = (wg - a.wg0) * VTH + threadIdx.x;
    double M[9];
    for (int k = 0; k < 9; k++) M[k] = M_cur[9 * (long)a.entry + k];
    bool in = false;
    if (i < en.m) {
        const float2 s = src[en.m0 + i], d = dst[en.m0 + i];
        in = Model::inlier(M, (double)s.x, (double)s.y, (double)d.x, (double)d.y, t2);
        mask[en.m0 + i] = in ? 1 : 0;
    }
    const int n = __popcll(__ballot(in));
    if ((threadIdx.x & 63) == 0 && n > 0) atomicAdd(&count[a.entry], n);
}

// ---- the refit round on the device ---------------------------------------------------------------------------------------------
constexpr int kRefitLanes = vr::kRefitChunk;                // a lane stages one match of the chunk
static_assert(kRefitLanes % 64 == 0, "whole waves");

__global__ __launch_bounds__(VTH) void live_pairs_kernel(const unsigned long long *best, int n_ent, uint8_t *live)
{
    const int e = blockIdx.x * VTH + threadIdx.x;
    if (e < n_ent) live[e] = vr::key_count(best[e]) > 0 ? 1 : 0;
}

template <typename Model>
__global__ __launch_bounds__(kRefitLanes) void refit_pairs_kernel(const float2 *src, const float2 *dst, const vb::Entry *__restrict__ ent,
                                                                  const uint8_t *mask, uint8_t *live, double *M_try)
{
    constexpr int C = vr::kRefitChunk;
    static_assert(Model::kRefitSums <= kRefitLanes && Model::kRefitSums <= Model::kRefitWork, "a lane for every sum, and the sums are the head of work");
    __shared__ double rows[C * Model::kRefitRow];                   // a chunk: (x, y, u, v), then the two distances, then the model's rows
    __shared__ double work[Model::kRefitWork];
    __shared__ double par[6];                               // cxs, cys, cxd, cyd, then the mean distances ds, dd
    __shared__ uint8_t in[C];
    const int e = blockIdx.x, l = threadIdx.x;
    if (!live[e]) return;                                   // the same for the whole workgroup
    const vb::Entry en = ent[e];
    const float2 *s2 = src + en.m0, *d2 = dst + en.m0;
    const uint8_t *mk = mask + en.m0;
    // the coordinate sums: lane k < 4 owns sum_x, sum_y of src and of dst; every lane counts the inliers
    int n = 0, first = -1;
    double sum = 0.0;
    for (int i0 = 0; i0 < en.m; i0 += C) {
        const int cnt = min(C, en.m - i0);
        if (l < cnt) {
            const float2 s = s2[i0 + l], d = d2[i0 + l];
            rows[4 * l] = (double)s.x; rows[4 * l + 1] = (double)s.y; rows[4 * l + 2] = (double)d.x; rows[4 * l + 3] = (double)d.y;
            in[l] = mk[i0 + l];
        }
        __syncthreads();
        for (int j = 0; j < cnt; j++) {
            if (!in[j]) continue;
            first = first < 0 ? i0 + j : first;
            n++;
            sum = sum + rows[4 * j + (l & 3)];
        }
        __syncthreads();
    }
    if (l < 4) par[l] = sum / (double)n;
    __syncthreads();
    const double cxs = par[0], cys = par[1], cxd = par[2], cyd = par[3];
    // the distance sums: the workgroup forms the square roots of a chunk, lane k < 2 adds those of src or dst in order
    sum = 0.0;
    for (int i0 = 0; i0 < en.m; i0 += C) {
        const int cnt = min(C, en.m - i0);
        if (l < cnt) {
            const float2 s = s2[i0 + l], d = d2[i0 + l];
            rows[2 * l] = vr::centred_length((double)s.x, (double)s.y, cxs, cys);
            rows[2 * l + 1] = vr::centred_length((double)d.x, (double)d.y, cxd, cyd);
            in[l] = mk[i0 + l];
        }
        __syncthreads();
        for (int j = 0; j < cnt; j++) {
            if (!in[j]) continue;
            sum = sum + rows[2 * j + (l & 1)];
        }
        __syncthreads();
    }
    if (l < 2) par[4 + l] = sum / (double)n;
    __syncthreads();
    double ss = 0.0, sd = 0.0;
    bool ok = !Model::refit_few(n);
    ok = vr::hartley_scale(par[4], ss) && ok;
    ok = vr::hartley_scale(par[5], sd) && ok;
    if (!ok) {                                              // uniform: every lane holds the same n and reads the same par
        if (l == 0) live[e] = 0;
        if (l < 9) M_try[9 * (long)e + l] = 0.0;
        return;
    }
    // the sums of N (and r): the workgroup forms the rows of a chunk, lane l < kSums adds its products in order
    const vr::Terms t = Model::refit_terms(l);
    sum = 0.0;
    for (int i0 = 0; i0 < en.m; i0 += C) {
        const int cnt = min(C, en.m - i0);
        if (l < cnt) {
            const float2 s = s2[i0 + l], d = d2[i0 + l];
            Model::refit_row(vr::normalised((double)s.x, cxs, ss), vr::normalised((double)s.y, cys, ss), vr::normalised((double)d.x, cxd, sd),
                             vr::normalised((double)d.y, cyd, sd), rows + Model::kRefitRow * l);
            in[l] = mk[i0 + l];
        }
        __syncthreads();
        for (int j = 0; j < cnt; j++) {
            if (!in[j]) continue;
            sum = Model::refit_add(sum, rows + Model::kRefitRow * j, t);
        }
        __syncthreads();
    }
    if (l < Model::kRefitSums) work[l] = sum;
    __syncthreads();
    if (l == 0) {
        const float2 f = s2[first];                         // n > 0 here: a mean distance above 0 has an inlier behind it
        double M[9];
        const bool good = Model::refit_solve(work, cxs, cys, ss, cxd, cyd, sd, (double)f.x, (double)f.y, M);
        for (int i = 0; i < 9; i++) M_try[9 * (long)e + i] = good ? M[i] : 0.0;
        if (!good) live[e] = 0;
    }
}

// verify_rules::refit_step of every live entry: (M_try, trial, n_try) of the round against (M_cur, mask, count)
__global__ __launch_bounds__(VTH) void step_pairs_kernel(const vb::Entry *__restrict__ ent, const double *M_try, const uint8_t *trial, int *n_try,
                                                         double *M_cur, uint8_t *mask, int *count, uint8_t *live)
{
    const int e = blockIdx.x;
    const bool alive = live[e] != 0;
    const int c = n_try[e], have = count[e];
    __syncthreads();                                        // every lane has read what lane 0 writes below
    if (!alive) return;
    if (threadIdx.x == 0) n_try[e] = 0;                     // the next round's mask launch adds into it
    if (c < have) {
        if (threadIdx.x == 0) live[e] = 0;
        return;
    }
    const vb::Entry en = ent[e];
    bool changed = false;
    for (int i = threadIdx.x; i < en.m; i += VTH) {
        const uint8_t b = trial[en.m0 + i];
        changed = changed || b != mask[en.m0 + i];
        mask[en.m0 + i] = b;
    }
    const int any = __syncthreads_or(changed ? 1 : 0);
    if (threadIdx.x < 9) M_cur[9 * (long)e + threadIdx.x] = M_try[9 * (long)e + threadIdx.x];
    if (threadIdx.x == 0) { count[e] = c; live[e] = any ? 1 : 0; }
}

}  // namespace

// ---- one launch of verify_batch.hpp's plan: ent [n_ent] and the launch's matches src, dst [.][2] (8-byte aligned) in device memory ----
// M_all [n_ent][n_hyp][9]
template <typename Model>
void verify_pairs_hypotheses(const float *src, const float *dst, const verify_batch::Entry *ent, int64_t n_ent, uint64_t seed, int n_hyp, double *M_all,
                             hipStream_t s)
{
    constexpr int lanes = kHypLanes<Model>;
    const int hblocks = (n_hyp + lanes - 1) / lanes;
    hipLaunchKernelGGL(hyp_pairs_kernel<Model>, dim3((unsigned)(n_ent * hblocks)), dim3(lanes), 0, s, src, dst, ent, (unsigned long long)seed, n_hyp,
                       hblocks, M_all);
    DLCO_HIP(hipGetLastError());
}

// count [n_ent][n_hyp] += the inliers of every hypothesis among its entry's matches; the caller zeroes count.  wgs is the
// launch's scoring grid; one entry's grid beyond a 1-D grid's reach goes in pieces.
template <typename Model>
void verify_pairs_score(const float *src, const float *dst, const verify_batch::Entry *ent, int64_t n_ent, int64_t wgs, const double *M_all, int n_hyp,
                        double t2, int32_t *count, hipStream_t s)
{
    const int hblocks = (int)verify_batch::blocks(n_hyp);
    for (int64_t base = 0; base < wgs; base += verify_batch::kLaunchWgs)
        hipLaunchKernelGGL(score_pairs_kernel<Model>, dim3((unsigned)std::min(verify_batch::kLaunchWgs, wgs - base)), dim3(VTH), 0, s,
                           reinterpret_cast<const float2 *>(src), reinterpret_cast<const float2 *>(dst), ent, (int)n_ent, M_all, n_hyp, hblocks, t2, count,
                           (long)base);
    DLCO_HIP(hipGetLastError());
}

// best [n_ent] = the largest selection key of every entry, M_cur [n_ent][9] = its matrix (zero: no model)
void verify_pairs_select(const int32_t *count, const double *M_all, int64_t n_ent, int n_hyp, uint64_t *best, double *M_cur, hipStream_t s)
{
    hipLaunchKernelGGL(select_pairs_kernel, dim3((unsigned)n_ent), dim3(VSEL), 0, s, count, M_all, n_hyp, reinterpret_cast<unsigned long long *>(best), M_cur);
    DLCO_HIP(hipGetLastError());
}

// for the entries of active [n_active] (wgs workgroups in all): the mask of M_cur [entry] at the entry's matches and
// n [entry] += its inliers; the caller zeroes n.  live (may be NULL: all) [n_ent]: an entry with live [entry] = 0 is left alone
template <typename Model>
void verify_pairs_mask(const float *src, const float *dst, const verify_batch::Entry *ent, const verify_batch::Active *active, int64_t n_active,
                       int64_t wgs, const double *M_cur, double t2, uint8_t *mask, int32_t *n, const uint8_t *live, hipStream_t s)
{
    hipLaunchKernelGGL(mask_pairs_kernel<Model>, dim3((unsigned)wgs), dim3(VTH), 0, s, reinterpret_cast<const float2 *>(src),
                       reinterpret_cast<const float2 *>(dst), ent, active, (int)n_active, M_cur, t2, mask, n, live);
    DLCO_HIP(hipGetLastError());
}

// live [n_ent] = the selection found a model for the entry (best [e] has a count above 0)
void verify_pairs_live(const uint64_t *best, int64_t n_ent, uint8_t *live, hipStream_t s)
{
    hipLaunchKernelGGL(live_pairs_kernel, dim3((unsigned)((n_ent + VTH - 1) / VTH)), dim3(VTH), 0, s, reinterpret_cast<const unsigned long long *>(best),
                       (int)n_ent, live);
    DLCO_HIP(hipGetLastError());
}

// one round of the refit for the entries with live [e] != 0: M_try [e] = Model::refit_round of the entry's matches under
// mask; a rejected round clears live [e] and zeroes M_try [e]
template <typename Model>
void verify_pairs_refit(const float *src, const float *dst, const verify_batch::Entry *ent, int64_t n_ent, const uint8_t *mask, uint8_t *live,
                        double *M_try, hipStream_t s)
{
    hipLaunchKernelGGL(refit_pairs_kernel<Model>, dim3((unsigned)n_ent), dim3(kRefitLanes), 0, s, reinterpret_cast<const float2 *>(src),
                       reinterpret_cast<const float2 *>(dst), ent, mask, live, M_try);
    DLCO_HIP(hipGetLastError());
}

// verify_rules::refit_step for the live entries: the round (M_try, trial, n_try) meets the model (M_cur, mask, count); n_try
// [e] is zeroed for the next round, live [e] cleared when the entry's refit ends
void verify_pairs_step(const verify_batch::Entry *ent, int64_t n_ent, const double *M_try, const uint8_t *trial, int32_t *n_try, double *M_cur,
                       uint8_t *mask, int32_t *count, uint8_t *live, hipStream_t s)
{
    hipLaunchKernelGGL(step_pairs_kernel, dim3((unsigned)n_ent), dim3(VTH), 0, s, ent, M_try, trial, n_try, M_cur, mask, count, live);
    DLCO_HIP(hipGetLastError());
}

#define DLCO_VERIFY_MODEL(Model)                                                                                                 \
    template void verify_pairs_hypotheses<Model>(const float *, const float *, const verify_batch::Entry *, int64_t, uint64_t, int, double *, hipStream_t); \
    template void verify_pairs_score<Model>(const float *, const float *, const verify_batch::Entry *, int64_t, int64_t, const double *, int, double,      \
                                            int32_t *, hipStream_t);                                                                                       \
    template void verify_pairs_mask<Model>(const float *, const float *, const verify_batch::Entry *, const verify_batch::Active *, int64_t, int64_t,      \
                                           const double *, double, uint8_t *, int32_t *, const uint8_t *, hipStream_t);                                    \
    template void verify_pairs_refit<Model>(const float *, const float *, const verify_batch::Entry *, int64_t, const uint8_t *, uint8_t *, double *,     \
                                            hipStream_t);
DLCO_VERIFY_MODEL(verify_rules::Homography)
DLCO_VERIFY_MODEL(epipolar_rules::Fundamental)
#undef DLCO_VERIFY_MODEL

}  // namespace dlco
