// kernels_tracks.hip — from the verified matches of many image pairs to multi-view tracks (dlco_desc_build_tracks*): a
// lock-free union-find over the rows of the batch's table, the grouping of the nodes by component, flags and a stable
// compaction.  The rule is track_rules.hpp, where it is stated together with the hook step and the arguments for its
// invariant, its termination and its stale reads; this file only decides where the numbers are read from and in which order
// the work is done.  Everything is an integer or a comparison; there is no float, no device assert and no printf.
//
// Nodes and matches are cut into blocks of kBlockNodes = 256, a workgroup of four waves each.
//   tracks_init_kernel     one lane per node: parent[g] = g, node[g] = g (the values of the sort), conf[g] = 0.
//   tracks_hook_kernel     one lane per match.  The workgroup finds the pairs of its first and last match by a binary search
//                          over the uploaded pairs (24 bytes each), a lane its own between the two; a match the mask drops or
//                          whose rows lie outside their images is skipped before anything is indexed with them; the others
//                          run track_rules::hook.  EVERY write to parent in this launch is an atomicMin, so a slot only ever
//                          decreases and parent[x] <= x holds throughout; there is no path shortening.  The walk of find_root
//                          strictly descends and a retry continues with a strictly smaller larger end, so every lane ends by
//                          itself: no loop waits for another lane.  parent is read with agent-scope relaxed atomic loads: the
//                          L2 of an XCD is not coherent with the others', and although a stale value is only an older, larger
//                          ancestor of the same component (which costs steps, not the result: the atomicMin sees the slot
//                          itself and a lost race is retried), a load the compiler may hoist or keep in a register could
//                          repeat one stale value for the whole walk.
//   tracks_label_kernel    after the kernel boundary, one lane per node: label[g] = the root of g.  Reads parent, writes
//                          label, nothing else.
//   (rocPRIM radix_sort_pairs) the nodes sorted by label; the sort is stable and the values start ascending, so inside a
//                          component the nodes ascend in id, and nodes of one image are neighbours.
//   tracks_flag_kernel     one lane per sorted node k.  A head (k == 0 or another label than k - 1) finds the end of its
//                          segment by a binary search in the sorted labels and stores the size at size[label]; a node that
//                          is no head and lies in the image of its predecessor stores conf[label] = 1 (every such lane stores
//                          the same 1).
//   tracks_keep_kernel     one lane per sorted node: the node is kept iff its component is a track (track_rules::is_track).
//                          The 64-bit __ballot of the wave for kept nodes and for kept heads into word [2][blocks][4], and the
//                          block's five counts (kept nodes, kept heads, and the heads that make up counts[0 .. 2]) into
//                          count [5][blocks].
//   tracks_scan_kernel     five workgroups of kScanChunk = 1024 lanes, one per counted quantity: the block counts into
//                          exclusive int64 offsets, a chunk per step with a carry that every lane keeps; total [q] = the sum.
//   tracks_scatter_kernel  one lane per sorted node.  A kept node's place in obs is its block's offset + the bits of the
//                          earlier words of the block + the bits of its own word below its lane; its track is the number of
//                          kept heads up to and including its own position, minus one.  A kept head writes toff[track], the
//                          last lane toff[n_tracks]; every lane writes track_of of its node, -1 for a node that is not kept.
// The order comes from kernel boundaries; the only atomic operation is the hook's minimum.
#include "dlco_internal.hpp"
#include "track_rules.hpp"

#include <rocprim/rocprim.hpp>

namespace dlco {

namespace {

namespace tr = track_rules;

constexpr int TBL = tr::kBlockNodes;
constexpr int TWAVES = TBL / 64;
constexpr int TSCAN = tr::kScanChunk;
constexpr int TQ = tr::kCounted;
static_assert(TBL % 64 == 0 && TSCAN % 64 == 0 && TSCAN <= 1024 && TQ == 5, "whole waves; the scan is one workgroup per quantity");

__global__ __launch_bounds__(TBL) void tracks_init_kernel(long N, int32_t *__restrict__ parent, int32_t *__restrict__ node, uint8_t *__restrict__ conf)
{
    const long g = (long)blockIdx.x * TBL + threadIdx.x;
    if (g >= N) return;
    parent[g] = (int32_t)g;
    node[g] = (int32_t)g;
    conf[g] = 0;
}

__global__ __launch_bounds__(TBL) void tracks_hook_kernel(const tr::Pair *__restrict__ pairs, long n_pairs, long M, const int32_t *__restrict__ matches,
                                                          const uint8_t *__restrict__ keep, int32_t *parent)
{
    const long m0 = (long)blockIdx.x * TBL, m = m0 + threadIdx.x;
    if (m >= M) return;
    if (keep && keep[m] == 0) return;
    const long last = (m0 + TBL < M ? m0 + TBL : M) - 1;
    const long plo = tr::pair_of_match(pairs, 0, n_pairs - 1, m0);
    const long phi = tr::pair_of_match(pairs, plo, n_pairs - 1, last);
    const tr::Pair pr = pairs[tr::pair_of_match(pairs, plo, phi, m)];
    int32_t u, v;
    if (!tr::edge_of(pr, matches[2 * m], matches[2 * m + 1], &u, &v)) return;
    tr::hook(u, v,
             [parent](int32_t x) { return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); },
             [parent](int32_t x, int32_t val) { return atomicMin(&parent[x], val); });
}

__global__ __launch_bounds__(TBL) void tracks_label_kernel(long N, const int32_t *__restrict__ parent, int32_t *__restrict__ label)
{
    const long g = (long)blockIdx.x * TBL + threadIdx.x;
    if (g >= N) return;
    label[g] = tr::find_root((int32_t)g, [parent](int32_t x) { return parent[x]; });
}

__global__ __launch_bounds__(TBL) void tracks_flag_kernel(long N, const int32_t *__restrict__ slabel, const int32_t *__restrict__ snode,
                                                          const int64_t *__restrict__ seg, int n_img, int32_t *__restrict__ size,
                                                          uint8_t *__restrict__ conf)
{
    const long k = (long)blockIdx.x * TBL + threadIdx.x;
    if (k >= N) return;
    const int32_t l = slabel[k];
    if (k == 0 || slabel[k - 1] != l) {
        long lo = k, hi = N - 1;                           // the last position with this label: the labels ascend
        while (lo < hi) {
            const long mid = lo + (hi - lo + 1) / 2;
            if (slabel[mid] == l) lo = mid; else hi = mid - 1;
        }
        size[l] = (int32_t)(lo - k + 1);
    } else if (tr::image_of(seg, n_img, snode[k]) == tr::image_of(seg, n_img, snode[k - 1])) {
        conf[l] = 1;
    }
}

__global__ __launch_bounds__(TBL) void tracks_keep_kernel(long N, long nb, const int32_t *__restrict__ slabel, const int32_t *__restrict__ size,
                                                          const uint8_t *__restrict__ conf, int min_len, int unique,
                                                          unsigned long long *__restrict__ word, int *__restrict__ count)
{
    __shared__ int wave_n[TWAVES][TQ];
    const long k = (long)blockIdx.x * TBL + threadIdx.x;
    bool q[TQ] = {false, false, false, false, false};
    if (k < N) {
        const int32_t l = slabel[k];
        const int32_t sz = size[l];
        const bool c = conf[l] != 0, head = k == 0 || slabel[k - 1] != l;
        q[0] = tr::is_track(sz, c, min_len, unique);
        q[1] = head && q[0];
        q[2] = head && sz >= 2;
        q[3] = head && sz >= 2 && sz < min_len;
        q[4] = head && sz >= min_len && unique && c;
    }
    const int wave = threadIdx.x >> 6;
    for (int i = 0; i < TQ; i++) {
        const unsigned long long b = __ballot(q[i]);
        if ((threadIdx.x & 63) == 0) {
            if (i < 2) word[((long)i * nb + blockIdx.x) * TWAVES + wave] = b;
            wave_n[wave][i] = __popcll(b);
        }
    }
    __syncthreads();
    if (threadIdx.x < TQ) {
        int n = 0;
        for (int w = 0; w < TWAVES; w++) n += wave_n[w][threadIdx.x];
        count[(long)threadIdx.x * nb + blockIdx.x] = n;
    }
}

// count [TQ][nb] -> off [TQ][nb + 1], total [TQ]; workgroup q scans row q
__global__ __launch_bounds__(TSCAN) void tracks_scan_kernel(const int *__restrict__ count_all, long nb, long long *__restrict__ off_all,
                                                            long long *__restrict__ total)
{
    __shared__ int wave_sum[TSCAN / 64];
    const int *count = count_all + (long)blockIdx.x * nb;
    long long *off = off_all + (long)blockIdx.x * (nb + 1);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long carry = 0;
    for (long c0 = 0; c0 < nb; c0 += TSCAN) {
        const long k = c0 + threadIdx.x;
        const int v = k < nb ? count[k] : 0;
        int inc = v;                                       // at most 1024 x 256, far inside an int
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        int before = 0, sum = 0;
        for (int w = 0; w < TSCAN / 64; w++) {
            const int s = wave_sum[w];
            if (w < wave) before += s;
            sum += s;
        }
        if (k < nb) off[k] = carry + before + (inc - v);
        carry += sum;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        off[nb] = carry;
        total[blockIdx.x] = carry;
    }
}

// the set bits before position k: word and off of one quantity as the two kernels above wrote them
__device__ __forceinline__ long long before_of(const unsigned long long *__restrict__ word, const long long *__restrict__ off, long k)
{
    const long blk = k / TBL;
    const int wave = (int)((k - blk * TBL) >> 6), lane = (int)(k & 63);
    long long pos = off[blk];
    for (int w = 0; w < wave; w++) pos += __popcll(word[blk * TWAVES + w]);
    return pos + __popcll(word[blk * TWAVES + wave] & (((unsigned long long)1 << lane) - 1));
}

__global__ __launch_bounds__(TBL) void tracks_scatter_kernel(long N, long nb, const int32_t *__restrict__ snode, const unsigned long long *__restrict__ word,
                                                             const long long *__restrict__ off, long long *__restrict__ toff, int32_t *__restrict__ obs,
                                                             int32_t *__restrict__ track_of)
{
    const long k = (long)blockIdx.x * TBL + threadIdx.x;
    if (k >= N) return;
    const unsigned long long *hword = word + nb * TWAVES;
    const long long *hoff = off + (nb + 1);
    if (k == N - 1) toff[hoff[nb]] = off[nb];              // toff[n_tracks] = the observations; toff[0] = 0 without a track
    const int32_t g = snode[k];
    if (!((word[k >> 6] >> (k & 63)) & 1)) {
        track_of[g] = -1;
        return;
    }
    const bool head = (hword[k >> 6] >> (k & 63)) & 1;
    const long long pos = before_of(word, off, k), t = before_of(hword, hoff, k) + (head ? 1 : 0) - 1;
    obs[pos] = g;
    track_of[g] = (int32_t)t;
    if (head) toff[t] = pos;
}

}  // namespace

// the bits of a label, a node id below N: the sort looks at no more
static unsigned label_bits(int64_t N)
{
    unsigned b = 1;
    while (b < 31 && ((int64_t)1 << b) < N) b++;
    return b;
}

// bytes of rocPRIM's workspace for the sort of N nodes by label
size_t tracks_sort_bytes(int64_t N)
{
    size_t b = 0;
    DLCO_HIP(rocprim::radix_sort_pairs(nullptr, b, (const int32_t *)nullptr, (int32_t *)nullptr, (const int32_t *)nullptr, (int32_t *)nullptr, (size_t)N, 0,
                                       label_bits(N), (hipStream_t)0));
    return b;
}

// label [N] of the components of the graph; parent, node [N] and conf [N] are written (node = 0 .. N - 1, conf = 0).  M may be 0
void tracks_labels(const track_rules::Pair *pairs, int64_t n_pairs, int64_t N, int64_t M, const int32_t *matches, const uint8_t *keep, int32_t *parent,
                   int32_t *node, uint8_t *conf, int32_t *label, hipStream_t s)
{
    const dim3 grid((unsigned)tr::blocks(N)), wg(TBL);
    hipLaunchKernelGGL(tracks_init_kernel, grid, wg, 0, s, (long)N, parent, node, conf);
    if (M > 0)
        hipLaunchKernelGGL(tracks_hook_kernel, dim3((unsigned)tr::blocks(M)), wg, 0, s, pairs, (long)n_pairs, (long)M, matches, keep, parent);
    hipLaunchKernelGGL(tracks_label_kernel, grid, wg, 0, s, (long)N, (const int32_t *)parent, label);
    DLCO_HIP(hipGetLastError());
}

// from label and node = 0 .. N - 1 to the outputs: slabel, snode, size [N] scratch, conf [N] zero on entry, tmp of
// tracks_sort_bytes(N) bytes, word [2][blocks][4], count [5][blocks], off [5][blocks + 1], total [5] = the observations, the
// tracks and counts [0 .. 2]; seg [n_img + 1] in device memory
void tracks_group(int64_t N, const int32_t *label, const int32_t *node, const int64_t *seg, int32_t n_img, int32_t min_len, int32_t unique,
                  int32_t *slabel, int32_t *snode, int32_t *size, uint8_t *conf, void *tmp, size_t tmp_bytes, uint64_t *word, int32_t *count,
                  int64_t *off, int64_t *total, int64_t *toff, int32_t *obs, int32_t *track_of, hipStream_t s)
{
    const long nb = (long)tr::blocks(N);
    const dim3 grid((unsigned)nb), wg(TBL);
    auto *w = reinterpret_cast<unsigned long long *>(word);
    auto *o = reinterpret_cast<long long *>(off);
    size_t bytes = tmp_bytes;
    DLCO_HIP(rocprim::radix_sort_pairs(tmp, bytes, label, slabel, node, snode, (size_t)N, 0, label_bits(N), s));
    hipLaunchKernelGGL(tracks_flag_kernel, grid, wg, 0, s, (long)N, (const int32_t *)slabel, (const int32_t *)snode, seg, (int)n_img, size, conf);
    hipLaunchKernelGGL(tracks_keep_kernel, grid, wg, 0, s, (long)N, nb, (const int32_t *)slabel, (const int32_t *)size, (const uint8_t *)conf, (int)min_len,
                       (int)unique, w, count);
    hipLaunchKernelGGL(tracks_scan_kernel, dim3(TQ), dim3(TSCAN), 0, s, (const int *)count, nb, o, reinterpret_cast<long long *>(total));
    hipLaunchKernelGGL(tracks_scatter_kernel, grid, wg, 0, s, (long)N, nb, (const int32_t *)snode, (const unsigned long long *)w, (const long long *)o,
                       reinterpret_cast<long long *>(toff), obs, track_of);
    DLCO_HIP(hipGetLastError());
}

}  // namespace dlco
