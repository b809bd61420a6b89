// kernels_select.hip — from the nearest-two tables of a batched match to the segmented match list of a batched verification
// (dlco_desc_select_pairs*): the ratio test, the mutual check and the compaction into (query, train) rows.  The rule is
// select_rules.hpp, where it is stated; this file only decides where the numbers are read from and in which order the work is
// done.  The call is ONE stable stream compaction over the R output rows of the batch, pairs in order and rows ascending
// inside a pair.  Everything is an integer or a comparison; the order comes from kernel boundaries, no workgroup waits for
// another, and there is no atomic operation at all.
//
// Rows are cut into blocks of kBlockRows = 256, a workgroup of four waves each.
//   select_flag_kernel<Dist>         one lane per row.  The workgroup finds the pairs of its first and last row by a scalar
//                                    binary search over the uploaded pairs (40 bytes each; empty pairs repeat a row0, the row
//                                    belongs to the last of them), a lane its own pair between the two, mostly in no step at
//                                    all.  The rule, then the 64-bit __ballot of the wave into word [block][4] and the
//                                    block's count.  A row whose index is outside its train image is dropped before anything
//                                    is read at that index.
//   select_scan_kernel               one workgroup of kScanChunk = 1024 lanes: the block counts into exclusive int64 offsets,
//                                    a chunk per step (a shuffle scan per wave, the sixteen wave sums through LDS) with a
//                                    carry that every lane keeps; off [blocks] = M.
//   select_scatter_kernel<Dist, XY>  one lane per row.  A kept row's position is its block's offset + the bits of the earlier
//                                    words of the block + the bits of its own word below its lane.  It writes (i, j), d1 and,
//                                    with XY, the (x, y) of row i of image a and row j of image b from the one coordinate
//                                    table.
//   select_offsets_kernel            one lane per pair and one more: moff [p] = the position of the row row0[p], M when
//                                    there is no such row (trailing empty pairs, and p = n_pairs).
// Index tables and distances are read and written in 4-byte pieces: the call asks no alignment beyond the element's.
#include "dlco_internal.hpp"
#include "select_rules.hpp"

namespace dlco {

namespace {

namespace sr = select_rules;

constexpr int SBL = sr::kBlockRows;
constexpr int SWAVES = SBL / 64;
constexpr int SSCAN = sr::kScanChunk;
static_assert(SBL % 64 == 0 && SSCAN % 64 == 0 && SSCAN <= 1024, "whole waves; the scan is one workgroup");

// the pair of row g of the block that starts at g0; the first two searches are the same for the whole workgroup
__device__ __forceinline__ sr::Pair pair_of(const sr::Pair *__restrict__ pairs, long n_pairs, long R, long g0, long g)
{
    const long last = (g0 + SBL < R ? g0 + SBL : R) - 1;
    const long plo = sr::pair_of_row(pairs, 0, n_pairs - 1, g0);
    const long phi = sr::pair_of_row(pairs, plo, n_pairs - 1, last);
    return pairs[sr::pair_of_row(pairs, plo, phi, g)];
}

template <typename Dist>
__global__ __launch_bounds__(SBL) void select_flag_kernel(const sr::Pair *__restrict__ pairs, long n_pairs, long R, const int32_t *idx,
                                                          const Dist *__restrict__ sqdist, float f, const int32_t *back,
                                                          unsigned long long *__restrict__ word, int *__restrict__ count)
{
    __shared__ int wave_n[SWAVES];
    const long g0 = (long)blockIdx.x * SBL, g = g0 + threadIdx.x;
    bool k = false;
    if (g < R) {
        const sr::Pair pr = pair_of(pairs, n_pairs, R, g0, g);
        const int32_t id[2] = {idx[2 * g], idx[2 * g + 1]};
        const Dist d[2] = {sqdist[2 * g], sqdist[2 * g + 1]};
        k = sr::keep(pr, g - pr.row0, id, d, f, back);
    }
    const unsigned long long b = __ballot(k);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        word[(long)blockIdx.x * SWAVES + wave] = b;
        wave_n[wave] = __popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < SWAVES; w++) n += wave_n[w];
        count[blockIdx.x] = n;
    }
}

__global__ __launch_bounds__(SSCAN) void select_scan_kernel(const int *__restrict__ count, long nb, long long *__restrict__ off)
{
    __shared__ int wave_sum[SSCAN / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    for (long c0 = 0; c0 < nb; c0 += SSCAN) {
        const long k = c0 + threadIdx.x;
        const int v = k < nb ? count[k] : 0;
        int inc = v;                                       // at most 64 x 256, far inside an int
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < SSCAN / 64; w++) {
            const int s = wave_sum[w];
            if (w < wave) before += s;
            total += s;
        }
        if (k < nb) off[k] = carry + before + (inc - v);
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) off[nb] = carry;
}

// the matches before row g: word and off as the two kernels above wrote them
__device__ __forceinline__ long long position_of(const unsigned long long *__restrict__ word, const long long *__restrict__ off, long g)
{
    const long blk = g / SBL;
    const int wave = (int)((g - blk * SBL) >> 6), lane = (int)(g & 63);
    long long pos = off[blk];
    for (int w = 0; w < wave; w++) pos += __popcll(word[blk * SWAVES + w]);
    return pos + __popcll(word[blk * SWAVES + wave] & (((unsigned long long)1 << lane) - 1));
}

template <typename Dist, bool XY>
__global__ __launch_bounds__(SBL) void select_scatter_kernel(const sr::Pair *__restrict__ pairs, long n_pairs, long R, const int32_t *__restrict__ idx,
                                                             const Dist *__restrict__ sqdist, const unsigned long long *__restrict__ word,
                                                             const long long *__restrict__ off, const float *__restrict__ xy, long ldxy,
                                                             int32_t *__restrict__ matches, Dist *__restrict__ dist, float *__restrict__ src,
                                                             float *__restrict__ dst)
{
    const long g0 = (long)blockIdx.x * SBL, g = g0 + threadIdx.x;
    if (g >= R) return;
    if (!((word[g >> 6] >> (g & 63)) & 1)) return;
    const long long pos = position_of(word, off, g);
    const sr::Pair pr = pair_of(pairs, n_pairs, R, g0, g);
    const long i = g - pr.row0;
    const int32_t j = idx[2 * g];                          // in [0, nt): the row was kept
    matches[2 * pos] = (int32_t)i;
    matches[2 * pos + 1] = j;
    dist[pos] = sqdist[2 * g];
    if (XY) {
        const float *a = xy + (pr.src0 + i) * ldxy, *b = xy + (pr.dst0 + j) * ldxy;
        src[2 * pos] = a[0];
        src[2 * pos + 1] = a[1];
        dst[2 * pos] = b[0];
        dst[2 * pos + 1] = b[1];
    }
}

__global__ __launch_bounds__(SBL) void select_offsets_kernel(const sr::Pair *__restrict__ pairs, long n_pairs, long R,
                                                             const unsigned long long *__restrict__ word, const long long *__restrict__ off,
                                                             long long *__restrict__ moff)
{
    const long p = (long)blockIdx.x * SBL + threadIdx.x;
    if (p > n_pairs) return;
    const long g = p < n_pairs ? pairs[p].row0 : R;
    moff[p] = g >= R ? off[sr::blocks(R)] : position_of(word, off, g);
}

}  // namespace

// ---- the steps of a select call; pairs [n_pairs] (select_rules::pair_records) and every table in device memory, R >= 1 rows in
// blocks = select_rules::blocks(R) blocks.  word [blocks][4] and count [blocks] out
template <typename Dist>
void select_flag(const select_rules::Pair *pairs, int64_t n_pairs, int64_t R, const int32_t *idx, const Dist *sqdist, float f, const int32_t *back,
                 uint64_t *word, int32_t *count, hipStream_t s)
{
    hipLaunchKernelGGL(select_flag_kernel<Dist>, dim3((unsigned)sr::blocks(R)), dim3(SBL), 0, s, pairs, (long)n_pairs, (long)R, idx, sqdist, f, back,
                       reinterpret_cast<unsigned long long *>(word), count);
    DLCO_HIP(hipGetLastError());
}

// off [blocks + 1]: the exclusive sums of count, off [blocks] = M
void select_scan(const int32_t *count, int64_t blocks, int64_t *off, hipStream_t s)
{
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SSCAN), 0, s, count, (long)blocks, reinterpret_cast<long long *>(off));
    DLCO_HIP(hipGetLastError());
}

// the first M entries of matches [.][2], dist [.] and, when xy (pitch ldxy floats) is not null, src, dst [.][2]
template <typename Dist>
void select_scatter(const select_rules::Pair *pairs, int64_t n_pairs, int64_t R, const int32_t *idx, const Dist *sqdist, const uint64_t *word,
                    const int64_t *off, const float *xy, int64_t ldxy, int32_t *matches, Dist *dist, float *src, float *dst, hipStream_t s)
{
    const auto *w = reinterpret_cast<const unsigned long long *>(word);
    const auto *o = reinterpret_cast<const long long *>(off);
    const dim3 grid((unsigned)sr::blocks(R)), wg(SBL);
    if (xy)
        hipLaunchKernelGGL((select_scatter_kernel<Dist, true>), grid, wg, 0, s, pairs, (long)n_pairs, (long)R, idx, sqdist, w, o, xy, (long)ldxy, matches,
                           dist, src, dst);
    else
        hipLaunchKernelGGL((select_scatter_kernel<Dist, false>), grid, wg, 0, s, pairs, (long)n_pairs, (long)R, idx, sqdist, w, o, xy, (long)ldxy, matches,
                           dist, src, dst);
    DLCO_HIP(hipGetLastError());
}

// moff [n_pairs + 1]
void select_offsets(const select_rules::Pair *pairs, int64_t n_pairs, int64_t R, const uint64_t *word, const int64_t *off, int64_t *moff, hipStream_t s)
{
    hipLaunchKernelGGL(select_offsets_kernel, dim3((unsigned)((n_pairs + 1 + SBL - 1) / SBL)), dim3(SBL), 0, s, pairs, (long)n_pairs, (long)R,
                       reinterpret_cast<const unsigned long long *>(word), reinterpret_cast<const long long *>(off), reinterpret_cast<long long *>(moff));
    DLCO_HIP(hipGetLastError());
}

#define DLCO_SELECT_DIST(Dist)                                                                                                               \
    template void select_flag<Dist>(const select_rules::Pair *, int64_t, int64_t, const int32_t *, const Dist *, float, const int32_t *, uint64_t *, \
                                    int32_t *, hipStream_t);                                                                                 \
    template void select_scatter<Dist>(const select_rules::Pair *, int64_t, int64_t, const int32_t *, const Dist *, const uint64_t *, const int64_t *, \
                                       const float *, int64_t, int32_t *, Dist *, float *, float *, hipStream_t);
DLCO_SELECT_DIST(float)
DLCO_SELECT_DIST(int32_t)
#undef DLCO_SELECT_DIST

}  // namespace dlco
