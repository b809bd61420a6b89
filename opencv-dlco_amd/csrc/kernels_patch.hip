// kernels_patch.hip — 64 x 64 patches cut out of an image in HBM around keypoints, the front of the describe chain:
//
//   patch_sample_kernel     one workgroup per keypoint frame (patch_rules.hpp, where the rule is stated; this file
//                           only decides where the taps are read from).  A thread forms 4 neighbouring patch pixels
//                           and stores them as one dword, so a wave writes 256 contiguous bytes per store, in the
//                           [n][64][64] u8 row-major layout desc_transform_kernel reads.
//
//     staged path           the box of pixels the taps can touch (patch_rules::stage_plan) is copied into LDS first, in
//                           16-byte blocks that keep the image's own alignment (16-byte loads wherever the block lies
//                           inside the image, bytes at its two ends), and the 4 k k taps of every pixel come from there:
//                           the image is read once, in rows, instead of 4 k k scattered bytes per pixel.
//     direct path           a box beyond patch_rules::kStageBudget: the taps are gathered from global memory.
//
// Both paths run patch_rules::sample_pixel on the same integers and give the same bytes.
#include "dlco_internal.hpp"
#include "patch_rules.hpp"

namespace dlco {

namespace {

using patch_rules::Frame;

constexpr int STH = 256;                  // threads per keypoint: 16 pixels each, as 4 passes of 4

// the staged box: row cy of the image starts at byte (cy - by0) * pitch + its offset in its 16-byte block
struct LdsSrc {
    const uint8_t *lds;
    int by0, bx0, pitch;
    uint32_t base_lo, pitch_lo;           // the address of (row 0, bx0) and the image pitch, both modulo 16
    __device__ int row(int cy) const { return (cy - by0) * pitch + (int)((base_lo + (uint32_t)cy * pitch_lo) & 15u) - bx0; }
    __device__ uint32_t at(int r, int cx) const { return lds[r + cx]; }
};

template <typename Src>
__device__ void write_patch(const Frame &f, int W, int H, const Src &src, uint8_t *patch)
{
    for (int q = threadIdx.x; q < 64 * 16; q += STH) {
        const int v = q >> 4, u0 = (q & 15) * 4;
        uint32_t w = 0;
        for (int j = 0; j < 4; j++) w |= (uint32_t)patch_rules::sample_pixel(f, W, H, v, u0 + j, src) << (8 * j);
        reinterpret_cast<uint32_t *>(patch)[q] = w;
    }
}

__global__ __launch_bounds__(STH) void patch_sample_kernel(const uint8_t *img, int W, int H, long pitch, const Frame *frames, uint8_t *patches)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t box[];
    const Frame f = frames[blockIdx.x];
    uint8_t *patch = patches + (size_t)blockIdx.x * 4096;
    if (!f.valid) {
        reinterpret_cast<uint4 *>(patch)[threadIdx.x] = make_uint4(0, 0, 0, 0);
        return;
    }
    const patch_rules::Stage st = patch_rules::stage_plan(f, W, H);
    if (!st.staged) {
        write_patch(f, W, H, patch_rules::ImageSrc{img, pitch}, patch);
        return;
    }
    // offsets are from img; [0, size) are the bytes of the image: a 16-byte block inside it is loaded whole, one across its
    // ends byte by byte
    const long size = (long)(H - 1) * pitch + W;
    const uint32_t img_lo = (uint32_t)((uintptr_t)img & 15), pitch_lo = (uint32_t)(pitch & 15);
    const int nb = st.pitch / 16;
    for (int i = threadIdx.x; i < st.bh * nb; i += STH) {
        const int r = i / nb, j = i - r * nb;
        const int sh = (int)((img_lo + (uint32_t)(st.by0 + r) * pitch_lo + (uint32_t)st.bx0) & 15u);
        if (16 * j >= sh + st.bw) continue;                    // no byte of the box in this block
        const long a = (long)(st.by0 + r) * pitch + st.bx0 - sh + 16 * j;
        uint4 blk;
        if (a >= 0 && a + 16 <= size) {
            blk = *reinterpret_cast<const uint4 *>(img + a);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (int b = 0; b < 16; b++)
                if (a + b >= 0 && a + b < size) w[b >> 2] |= (uint32_t)img[a + b] << (8 * (b & 3));
            blk = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4 *>(box + r * st.pitch + 16 * j) = blk;
    }
    __syncthreads();
    write_patch(f, W, H, LdsSrc{box, st.by0, st.bx0, st.pitch, img_lo + (uint32_t)st.bx0, pitch_lo}, patch);
}

}  // namespace

// LDS bytes a launch over these frames needs: the largest staged box among them (0: every patch takes the direct path)
int patch_stage_bytes(const Frame *frames_host, int n, int W, int H)
{
    int bytes = 0;
    for (int i = 0; i < n; i++) {
        const patch_rules::Stage st = patch_rules::stage_plan(frames_host[i], W, H);
        if (st.staged) bytes = std::max(bytes, st.pitch * st.bh);
    }
    return bytes;
}

// patches [n][64][64] u8 from frames [n] (device) on img [H][pitch] (device); lds_bytes = patch_stage_bytes of the frames
void patch_sample(const uint8_t *img, int W, int H, long pitch, const Frame *frames, int n, uint8_t *patches, int lds_bytes, hipStream_t s)
{
    if (n <= 0) return;
    DLCO_CHECK(lds_bytes >= 0 && lds_bytes <= patch_rules::kStageBudget, DLCO_ERR_INVALID, "patch_sample: staged box above the LDS budget");
    hipLaunchKernelGGL(patch_sample_kernel, dim3((unsigned)n), dim3(STH), (size_t)lds_bytes, s, img, W, H, pitch, frames, patches);
    DLCO_HIP(hipGetLastError());
}

}  // namespace dlco
