// kernels_orient.hip — the orientation of keypoints from the integral image in HBM (dlco_desc_orient,
// dlco_desc_detect_oriented).  The rule is orient_rules.hpp, where it is stated; this file only decides where the numbers are
// read from and in which order the work is done.
//
//   orient_kernel   one wavefront per keypoint, four keypoints per workgroup of 256.  A lane takes the samples `lane` and
//                   `lane + 64` of the 109: the Haar responses from 16 corners of S each, the weighted g and its bin.  The
//                   histogram of a wave, 36 x 2 sums, sits in LDS as int32 (orient_rules.hpp: a bin stays below 2^30) and is
//                   filled by LDS atomic adds: integer sums do not depend on the order.  Lanes 0 .. 35 then form the window
//                   sums in int64, and a butterfly of shuffles finds the winner by (score descending, k ascending); lane 0
//                   stores the vector (one 16-byte store) and the status byte.
//                   The corners are read from S directly, through L2: copying a keypoint's footprint of S, (14 s + 2)^2
//                   entries, to LDS first was measured for s <= 1, 2, 3 and 4 and was never faster (Orientation).
#include "dlco_internal.hpp"
#include "orient_rules.hpp"

namespace dlco {

namespace {

namespace dr = detect_rules;
namespace orr = orient_rules;

constexpr int OTH = 256, OWAVES = OTH / 64;
constexpr long kLaunchKeypoints = 1L << 24;                 // keypoints per launch: 2^22 workgroups

// the histogram of a wave: HX [36], then HY [36]
struct WaveHist {
    const int *h;
    __device__ int64_t x(int k) const { return h[k]; }
    __device__ int64_t y(int k) const { return h[orr::kBins + k]; }
};

__global__ __launch_bounds__(OTH) void orient_kernel(const uint32_t *S, long sp, int W, int H, const float4 *kp, long n, longlong2 *vec,
                                                     uint8_t *status)
{
    __shared__ int hist[OWAVES][2 * orr::kBins];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long k = (long)blockIdx.x * OWAVES + wave;
    const bool live = k < n;                                // the wave's: a ragged last workgroup has waves without a keypoint
    const float4 p = live ? kp[k] : make_float4(0.f, 0.f, 0.f, 0.f);
    const orr::Centre c = orr::centre_of(p.x, p.y, p.z);    // size 0 is invalid: a wave without a keypoint has no samples
    int *h = hist[wave];
    for (int q = lane; q < 2 * orr::kBins; q += 64) h[q] = 0;
    __syncthreads();
    int used = 0;
    if (c.valid)
        for (int t = lane; t < orr::kSamples; t += 64) {
            const orr::Offset o = orr::sample_offset(t);
            if (!orr::sample_used(c.X + o.i * c.s, c.Y + o.j * c.s, c.s, W, H)) continue;
            used++;
            const orr::Vec g = orr::gradient(dr::IntegralSrc{S, sp}, c.X, c.Y, c.s, o.i, o.j);
            const int b = orr::bin_of(g);
            if (b >= 0) {
                atomicAdd(&h[b], (int)g.x);
                atomicAdd(&h[orr::kBins + b], (int)g.y);
            }
        }
    __syncthreads();
    for (int d = 32; d >= 1; d >>= 1) used += __shfl_xor(used, d);
    orr::Vec v = {0, 0};
    long long best = -1;                                    // lanes 36 .. 63 hold no window: any score beats theirs
    int best_k = lane;
    if (lane < orr::kBins) {
        v = orr::window(WaveHist{h}, lane);
        best = orr::score(v);
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const long long other = __shfl_xor(best, d);
        const int other_k = __shfl_xor(best_k, d);
        if (orr::wins(other, other_k, best, best_k)) { best = other; best_k = other_k; }
    }
    const long long SX = __shfl((long long)v.x, best_k), SY = __shfl((long long)v.y, best_k);
    if (live && lane == 0) {
        vec[k] = make_longlong2(SX, SY);                    // an invalid keypoint has an empty histogram: (0, 0)
        status[k] = (uint8_t)(!c.valid ? 0 : used == orr::kSamples ? 2 : 1);
    }
}

}  // namespace

// vectors [n][2] and status [n] of keypoints [n][4] (16-byte aligned) on the image whose integral image is S, all in device memory
void orient_keypoints(const uint32_t *S, int W, int H, const float *kp, int64_t n, int64_t *vec, uint8_t *status, hipStream_t s)
{
    const long sp = detect_integral_pitch(W);
    for (int64_t k0 = 0; k0 < n; k0 += kLaunchKeypoints) {
        const long cnt = (long)std::min<int64_t>(kLaunchKeypoints, n - k0);
        hipLaunchKernelGGL(orient_kernel, dim3((unsigned)((cnt + OWAVES - 1) / OWAVES)), dim3(OTH), 0, s, S, sp, W, H,
                           reinterpret_cast<const float4 *>(kp) + k0, cnt, reinterpret_cast<longlong2 *>(vec) + k0, status + k0);
    }
    DLCO_HIP(hipGetLastError());
}

}  // namespace dlco
