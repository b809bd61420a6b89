// kernels_detect.hip — keypoints of an image in HBM (dlco_desc_detect*).  The rule is detect_rules.hpp, where it is stated;
// this file only decides where the numbers are read from and in which order the work is done.
//
//   integral_rows_kernel     one wave per image row: a lane sums 4 pixels, the wave scans the lane sums, a carry runs along
//                            the row.  A lane owns the pixels 4k-1 .. 4k+2, so that its four prefix sums are the entries
//                            4k .. 4k+3 of the row of S: one aligned 16-byte store per lane, 1 KiB per wave, and entry 0 of
//                            every row (no pixel to its left) falls out as 0.
//   integral_colsum_kernel   a thread per column and a block of rows per workgroup in y: the sum of the column over 64 rows.
//   integral_colscan_kernel  the same geometry: the sums of the segments above, then the running sum down the 64 rows, in
//                            place.  Both column kernels read and write 256 consecutive entries of a row per workgroup.
//   detect_octave_kernel     a tile of 32 x 8 candidate grid points of one octave: the responses of the four layers on the
//                            tile and a one-point halo go to LDS (int64), then layers 1 and 2 take the 3 x 3 x 3 test there
//                            and a keypoint is refined from the same values: the R volume never reaches HBM.  Octaves 0 and
//                            1 first stage the tile's footprint of S in LDS (61 x 37 and 118 x 70 entries) and take the 32
//                            corners of every response from there; the footprint of octaves 2 and 3 (232 x 136 entries and
//                            more) is beyond LDS, they read S directly, on a grid of 1/16 and 1/64 of the points.
//                            Survivors are appended through a counter: their order is arbitrary here and is fixed below.
//   selection                the survivors are put in position order by a radix sort of their position keys and then, by a
//                            stable descending radix sort of their responses, in the rule's order (rocPRIM, both); one
//                            kernel copies the first rows out.
//
// The counter goes on counting beyond the capacity of the survivor buffers; the caller then enlarges them and runs the
// octaves again, so no result depends on a capacity.
#include "dlco_internal.hpp"
#include "detect_rules.hpp"

#include <rocprim/rocprim.hpp>

namespace dlco {

namespace {

namespace dr = detect_rules;

constexpr int CSEG = 64;                  // rows per segment of the column scan
constexpr int TX = 32, TY = 8;            // candidate grid points per tile
constexpr int PX = TX + 2, PY = TY + 2;   // with the halo
constexpr int DTH = 256;

__global__ __launch_bounds__(256) void integral_rows_kernel(const uint8_t *img, int W, int H, long pitch, uint32_t *S, long sp)
{
    const int lane = threadIdx.x & 63, y = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (y >= H) return;                                    // a whole wave: y is the wave's
    const uint8_t *row = img + (long)y * pitch;
    uint32_t *out = S + (long)(y + 1) * sp;
    uint32_t carry = 0;
    for (long c0 = 0; c0 < sp; c0 += 256) {
        const long c = c0 + 4 * lane;
        uint32_t p[4];
        for (int k = 0; k < 4; k++) {
            const long x = c - 1 + k;
            p[k] = (x >= 0 && x < W) ? row[x] : 0u;
        }
        p[1] += p[0]; p[2] += p[1]; p[3] += p[2];
        uint32_t t = p[3];
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_up(t, d);
            if (lane >= d) t += u;
        }
        const uint32_t base = carry + t - p[3];
        if (c < sp) *reinterpret_cast<uint4 *>(out + c) = make_uint4(base + p[0], base + p[1], base + p[2], base + p[3]);
        carry += __shfl(t, 63);
    }
}

__global__ __launch_bounds__(256) void integral_colsum_kernel(const uint32_t *S, long sp, int H, uint32_t *seg)
{
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= sp) return;
    const int y0 = blockIdx.y * CSEG + 1, y1 = min(y0 + CSEG - 1, H);
    uint32_t sum = 0;
    for (int y = y0; y <= y1; y++) sum += S[(long)y * sp + c];
    seg[(long)blockIdx.y * sp + c] = sum;
}

__global__ __launch_bounds__(256) void integral_colscan_kernel(uint32_t *S, long sp, int H, const uint32_t *seg)
{
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= sp) return;
    uint32_t acc = 0;
    for (int t = 0; t < (int)blockIdx.y; t++) acc += seg[(long)t * sp + c];
    const int y0 = blockIdx.y * CSEG + 1, y1 = min(y0 + CSEG - 1, H);
    for (int y = y0; y <= y1; y++) {
        acc += S[(long)y * sp + c];
        S[(long)y * sp + c] = acc;
    }
}

// a piece [y0, ..) x [x0, ..) of S in LDS, rows of `pitch` entries
struct LdsIntegral {
    const uint32_t *lds;
    int x0, y0, pitch;
    __device__ uint32_t at(int y, int x) const { return lds[(y - y0) * pitch + (x - x0)]; }
};

// the responses of a tile with its halo: layer, then grid row from pj0, then grid column from pi0
struct TileVolume {
    const int64_t *R;
    int pi0, pj0;
    __device__ int64_t at(int layer, int j, int i) const { return R[(layer * PY + (j - pj0)) * PX + (i - pi0)]; }
};

template <bool STAGED>
__global__ __launch_bounds__(DTH) void detect_octave_kernel(const uint32_t *S, long sp, int o, int nx, int ny, int64_t threshold, unsigned cap,
                                                            unsigned *count, uint64_t *pos, int64_t *resp, float4 *kp)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    int64_t *Rt = reinterpret_cast<int64_t *>(lds);
    uint32_t *St = reinterpret_cast<uint32_t *>(lds + sizeof(int64_t) * dr::kLayers * PY * PX);
    const int st = dr::step(o), m = dr::margin(o);
    // candidates [i0, i0 + TX) x [j0, j0 + TY) within [1, nx-2] x [1, ny-2]; responses one point around them, all on the grid
    const int i0 = blockIdx.x * TX + 1, j0 = blockIdx.y * TY + 1;
    const int pi0 = i0 - 1, pj0 = j0 - 1;
    const int pw = min(PX, nx - pi0), ph = min(PY, ny - pj0);
    // the entries of S the filters of these points touch: pixels [st pi0, st (pi0 + pw - 1) + 2m] and one entry beyond
    const int fx0 = st * pi0, fy0 = st * pj0;
    const int fw = st * (pw - 1) + 2 * m + 2, fh = st * (ph - 1) + 2 * m + 2;
    if (STAGED) {
        for (int q = threadIdx.x; q < fw * fh; q += DTH) {
            const int r = q / fw, c = q - r * fw;
            St[q] = S[(long)(fy0 + r) * sp + fx0 + c];
        }
        __syncthreads();
    }
    for (int q = threadIdx.x; q < dr::kLayers * pw * ph; q += DTH) {
        const int layer = q / (pw * ph), rem = q - layer * pw * ph, pj = rem / pw, pi = rem - pj * pw;
        const int X = m + st * (pi0 + pi), Y = m + st * (pj0 + pj), L = dr::filter_side(o, layer);
        int64_t R;
        if (STAGED) R = dr::response(LdsIntegral{St, fx0, fy0, fw}, X, Y, L);
        else R = dr::response(dr::IntegralSrc{S, sp}, X, Y, L);
        Rt[(layer * PY + pj) * PX + pi] = R;
    }
    __syncthreads();
    const TileVolume V{Rt, pi0, pj0};
    for (int q = threadIdx.x; q < 2 * TX * TY; q += DTH) {
        const int layer = 1 + q / (TX * TY), rem = q % (TX * TY), j = j0 + rem / TX, i = i0 + rem % TX;
        if (i > nx - 2 || j > ny - 2) continue;
        if (!dr::is_keypoint(V, layer, j, i, threshold)) continue;
        const unsigned slot = atomicAdd(count, 1u);
        if (slot >= cap) continue;                         // counted, not kept: the caller comes back with room
        const dr::Keypoint k = dr::refine(V, o, layer, j, i);
        pos[slot] = dr::position_key(o, layer, j, i);
        resp[slot] = k.R;
        kp[slot] = make_float4(k.x, k.y, k.size, -1.0f);
    }
}

__global__ void iota_kernel(uint32_t *idx, unsigned n)
{
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) idx[k] = k;
}

__global__ void gather_response_kernel(const int64_t *resp, const uint32_t *idx, unsigned n, uint64_t *key)
{
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) key[k] = (uint64_t)resp[idx[k]];            // R >= threshold >= 1: the unsigned order is the order of R
}

__global__ void write_keypoints_kernel(const float4 *kp, const uint64_t *key_sorted, const uint32_t *idx, unsigned n_out, float4 *kp_out,
                                       int64_t *resp_out)
{
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_out) return;
    kp_out[k] = kp[idx[k]];
    if (resp_out) resp_out[k] = (int64_t)key_sorted[k];
}

size_t staged_lds_bytes(int o)
{
    const int st = dr::step(o), m = dr::margin(o);
    const size_t fw = st * (PX - 1) + 2 * m + 2, fh = st * (PY - 1) + 2 * m + 2;
    return fw * fh * sizeof(uint32_t);
}

}  // namespace

// entries per row of the device's S: W + 1 rounded up to a multiple of 4 (16-byte rows); S has (H + 1) rows
long detect_integral_pitch(int W) { return ((long)W + 1 + 3) / 4 * 4; }
// entries of the column scan's workspace
size_t detect_colsum_count(int W, int H) { return (size_t)((H + CSEG - 1) / CSEG) * (size_t)detect_integral_pitch(W); }

void detect_integral(const uint8_t *img, int W, int H, long pitch, uint32_t *S, uint32_t *seg, hipStream_t s)
{
    const long sp = detect_integral_pitch(W);
    const int nseg = (H + CSEG - 1) / CSEG;
    DLCO_HIP(hipMemsetAsync(S, 0, (size_t)sp * sizeof(uint32_t), s));
    hipLaunchKernelGGL(integral_rows_kernel, dim3((unsigned)((H + 3) / 4)), dim3(256), 0, s, img, W, H, pitch, S, sp);
    const dim3 grid((unsigned)((sp + 255) / 256), (unsigned)nseg);
    if (nseg > 1) hipLaunchKernelGGL(integral_colsum_kernel, grid, dim3(256), 0, s, (const uint32_t *)S, sp, H, seg);
    hipLaunchKernelGGL(integral_colscan_kernel, grid, dim3(256), 0, s, S, sp, H, (const uint32_t *)seg);
    DLCO_HIP(hipGetLastError());
}

// the keypoints of octave o appended to (pos, resp, kp) [cap] through *count, which also counts those beyond cap
void detect_octave(const uint32_t *S, int W, int H, int o, int64_t threshold, unsigned cap, unsigned *count, uint64_t *pos, int64_t *resp,
                   float *kp, hipStream_t s)
{
    const int nx = dr::grid_size(W, o), ny = dr::grid_size(H, o);
    if (nx < 3 || ny < 3) return;
    const long sp = detect_integral_pitch(W);
    const dim3 grid((unsigned)((nx - 2 + TX - 1) / TX), (unsigned)((ny - 2 + TY - 1) / TY));
    const size_t vol = sizeof(int64_t) * dr::kLayers * PY * PX;
    if (o <= 1)
        hipLaunchKernelGGL(detect_octave_kernel<true>, grid, dim3(DTH), vol + staged_lds_bytes(o), s, S, sp, o, nx, ny, threshold, cap, count, pos,
                           resp, reinterpret_cast<float4 *>(kp));
    else
        hipLaunchKernelGGL(detect_octave_kernel<false>, grid, dim3(DTH), vol, s, S, sp, o, nx, ny, threshold, cap, count, pos, resp,
                           reinterpret_cast<float4 *>(kp));
    DLCO_HIP(hipGetLastError());
}

// bytes of rocPRIM's workspace for detect_select on n survivors
size_t detect_select_bytes(size_t n)
{
    size_t b1 = 0, b2 = 0;
    DLCO_HIP(rocprim::radix_sort_pairs(nullptr, b1, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, n, 0,
                                       33, (hipStream_t)0));
    DLCO_HIP(rocprim::radix_sort_pairs_desc(nullptr, b2, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                            n, 0, 39, (hipStream_t)0));
    return std::max(b1, b2);
}

// The first n_out of the n survivors in the rule's order: rows (x, y, size, -1) into kp_out, responses into resp_out (may
// be nullptr).  key_a, key_b [n] and idx_a, idx_b [n] are scratch, tmp is detect_select_bytes(n) bytes.
void detect_select(const uint64_t *pos, const int64_t *resp, const float *kp, unsigned n, unsigned n_out, uint64_t *key_a, uint64_t *key_b,
                   uint32_t *idx_a, uint32_t *idx_b, void *tmp, size_t tmp_bytes, float *kp_out, int64_t *resp_out, hipStream_t s)
{
    if (n == 0 || n_out == 0) return;
    const unsigned nb = (n + 255) / 256;
    hipLaunchKernelGGL(iota_kernel, dim3(nb), dim3(256), 0, s, idx_a, n);
    size_t bytes = tmp_bytes;
    DLCO_HIP(rocprim::radix_sort_pairs(tmp, bytes, pos, key_a, (const uint32_t *)idx_a, idx_b, (size_t)n, 0, 33, s));
    hipLaunchKernelGGL(gather_response_kernel, dim3(nb), dim3(256), 0, s, resp, (const uint32_t *)idx_b, n, key_a);
    bytes = tmp_bytes;
    DLCO_HIP(rocprim::radix_sort_pairs_desc(tmp, bytes, (const uint64_t *)key_a, key_b, (const uint32_t *)idx_b, idx_a, (size_t)n, 0, 39, s));
    hipLaunchKernelGGL(write_keypoints_kernel, dim3((n_out + 255) / 256), dim3(256), 0, s, reinterpret_cast<const float4 *>(kp),
                       (const uint64_t *)key_b, (const uint32_t *)idx_a, n_out, reinterpret_cast<float4 *>(kp_out), resp_out);
    DLCO_HIP(hipGetLastError());
}

}  // namespace dlco
