// kernels_epipolar.hip — verification of a match list against a fundamental matrix (dlco_desc_verify_fundamental,
// dlco_desc_verify_fundamental_hypotheses).  The rule is epipolar_rules.hpp, where it is stated; this file only decides where
// the numbers are read from and in which order the work is done, as kernels_verify.hip does for the homography.  The
// selection is that file's verify_select_kernel.
//
//   epipolar_hyp_kernel    one lane per hypothesis: its sample of eight, the 8 x 9 system eliminated with complete pivoting,
//                          F_all [n_hyp][9] (all zero when invalid).  The system lives in registers: the header's loops unroll
//                          to constant indices and every run-time pivot is a predicated swap, so there is no scratch.
//                          Workgroups of 64, so that a lane may hold the 72 doubles and the compiler need not spill.
//   epipolar_score_kernel  the hot loop, verify_score_kernel's structure: a lane owns one hypothesis and keeps F in registers
//                          (9 doubles), the chunk's matches are staged in LDS as (x, y, u, v) doubles and read as a broadcast:
//                          two 16-byte reads and 33 fp64 operations per (hypothesis, match).  A private int32 counter, one
//                          integer atomicAdd per (hypothesis, chunk).
//   epipolar_mask_kernel   one lane per match for one F: the u8 mask and, by a ballot per wave and one atomicAdd, its count.
#include "dlco_internal.hpp"
#include "epipolar_rules.hpp"

namespace dlco {

namespace {

namespace er = epipolar_rules;
namespace vr = verify_rules;

constexpr int ETH = 256;
constexpr int EHYP = 64;                                    // lanes of a workgroup of the hypothesis kernel

struct Fundamental { double f[9]; };

__global__ __launch_bounds__(EHYP) void epipolar_hyp_kernel(const float *src, const float *dst, unsigned m, unsigned long long seed, int n_hyp,
                                                            double *F_all)
{
    const int h = blockIdx.x * EHYP + threadIdx.x;
    if (h >= n_hyp) return;
    int32_t idx[er::kSample];
    double F[9];
    er::hypothesis(src, dst, m, seed, (uint32_t)h, idx, F);
    for (int i = 0; i < 9; i++) F_all[9 * (long)h + i] = F[i];
}

__global__ __launch_bounds__(ETH) void epipolar_score_kernel(const float2 *src, const float2 *dst, int m, const double *F_all, int n_hyp, double t2,
                                                             int *count)
{
    __shared__ double4 pts[vr::kScoreChunk];
    static_assert(vr::kScoreChunk == ETH, "a lane stages one match of the chunk");
    const int h = blockIdx.x * ETH + threadIdx.x;
    const long i0 = (long)blockIdx.y * vr::kScoreChunk;
    const int cnt = (int)min((long)vr::kScoreChunk, (long)m - i0);
    if ((int)threadIdx.x < cnt) {
        const float2 s = src[i0 + threadIdx.x], d = dst[i0 + threadIdx.x];
        pts[threadIdx.x] = make_double4((double)s.x, (double)s.y, (double)d.x, (double)d.y);
    }
    double F[9];
    for (int i = 0; i < 9; i++) F[i] = h < n_hyp ? F_all[9 * (long)h + i] : 0.0;      // F = 0 has no inlier: S > 0 fails
    __syncthreads();
    int n = 0;
    for (int j = 0; j < cnt; j++) {
        const double4 p = pts[j];
        n += er::inlier(F, p.x, p.y, p.z, p.w, t2) ? 1 : 0;
    }
    if (h < n_hyp && n > 0) atomicAdd(&count[h], n);
}

__global__ __launch_bounds__(ETH) void epipolar_mask_kernel(const float2 *src, const float2 *dst, int m, Fundamental Fm, double t2, uint8_t *mask,
                                                            int *count)
{
    const long i = (long)blockIdx.x * ETH + threadIdx.x;
    bool in = false;
    if (i < m) {
        const float2 s = src[i], d = dst[i];
        in = er::inlier(Fm.f, (double)s.x, (double)s.y, (double)d.x, (double)d.y, t2);
        mask[i] = in ? 1 : 0;
    }
    const int n = __popcll(__ballot(in));
    if ((threadIdx.x & 63) == 0 && n > 0) atomicAdd(count, n);
}

}  // namespace

// F_all [n_hyp][9] of the matches src, dst [m][2] (8-byte aligned), all in device memory
void epipolar_hypotheses(const float *src, const float *dst, int64_t m, uint64_t seed, int n_hyp, double *F_all, hipStream_t s)
{
    hipLaunchKernelGGL(epipolar_hyp_kernel, dim3((unsigned)((n_hyp + EHYP - 1) / EHYP)), dim3(EHYP), 0, s, src, dst, (unsigned)m,
                       (unsigned long long)seed, n_hyp, F_all);
    DLCO_HIP(hipGetLastError());
}

// count [n_hyp] += the inliers of every hypothesis among the m matches; the caller zeroes count.  Launches are split as
// verify_score's are.
void epipolar_score(const float *src, const float *dst, int64_t m, const double *F_all, int n_hyp, double t2, int32_t *count, hipStream_t s)
{
    constexpr int64_t kLaunchMatches = (int64_t)32768 * vr::kScoreChunk;
    for (int64_t i0 = 0; i0 < m; i0 += kLaunchMatches) {
        const int cnt = (int)std::min<int64_t>(kLaunchMatches, m - i0);
        hipLaunchKernelGGL(epipolar_score_kernel, dim3((unsigned)((n_hyp + ETH - 1) / ETH), (unsigned)((cnt + vr::kScoreChunk - 1) / vr::kScoreChunk)),
                           dim3(ETH), 0, s, reinterpret_cast<const float2 *>(src) + i0, reinterpret_cast<const float2 *>(dst) + i0, cnt, F_all,
                           n_hyp, t2, count);
    }
    DLCO_HIP(hipGetLastError());
}

// mask [m] of the host's F [9] and *count += its inliers; the caller zeroes count
void epipolar_mask(const float *src, const float *dst, int64_t m, const double *F, double t2, uint8_t *mask, int32_t *count, hipStream_t s)
{
    Fundamental Fm;
    for (int i = 0; i < 9; i++) Fm.f[i] = F[i];
    hipLaunchKernelGGL(epipolar_mask_kernel, dim3((unsigned)((m + ETH - 1) / ETH)), dim3(ETH), 0, s, reinterpret_cast<const float2 *>(src),
                       reinterpret_cast<const float2 *>(dst), (int)m, Fm, t2, mask, count);
    DLCO_HIP(hipGetLastError());
}

}  // namespace dlco
