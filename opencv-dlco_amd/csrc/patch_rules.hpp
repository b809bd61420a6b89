// patch_rules.hpp — how a 64 x 64 patch is cut out of an image around a keypoint (dlco_desc_extract_patches /
// dlco_desc_describe_keypoints): the rule in integers, stated once for the host, the sampling kernel (kernels_patch.hip)
// and the CPU test (tests/shim/patch_rules_shim.cpp).  Plain C++: no HIP header, no device, no I/O.
//
// This is NOT the sampling of OpenCV's VGG::compute (a float warp of a smoothed image), which nothing here can run or
// pin.  It is a rule of this library: a similarity frame per keypoint rounded to 16.16 fixed point, bilinear taps with
// 8-bit weights on a replicated border and a k x k box prefilter, all in int64, so that every byte of a patch is the
// same on every machine and the tests compare with equality.
//
// A keypoint is (x, y, size, angle) with cv::KeyPoint's meaning: integer coordinates are pixel centres, angle in
// degrees, a negative angle means none.  The patch covers size * scale_factor source pixels on a side.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PATCH_RULES_HD __host__ __device__
#else
#define PATCH_RULES_HD
#endif

namespace patch_rules {

constexpr int kSide = 64;                      // patch pixels on a side
constexpr int kMaxSub = 8;                     // sub-samples per patch pixel and axis at most
constexpr int64_t kMaxCoord = (int64_t)1 << 20;
constexpr double kMaxStep = 64.0;              // source pixels per patch pixel at most

// The frame of one keypoint, the record the kernel takes: centre (X0, Y0) and the step (A, B) of half a sub-sample in
// 16.16 fixed point, k x k sub-samples per patch pixel.  valid == 0: the patch is all zeros.
struct Frame {
    int64_t X0, Y0;
    int32_t A, B;
    int32_t k;
    int32_t valid;
};

inline double rnd(double t) { return std::floor(t + 0.5); }

// s = size * scale_factor / 64 source pixels per patch pixel.  Invalid: x, y or s not finite, s <= 0, s > 64, |x| or
// |y| above 2^20.  a = 0 for angle < 0 or !use_orientation, else angle * pi / 180; k = min(8, max(1, ceil(s)));
// X0 = rnd(65536 x), Y0 = rnd(65536 y), A = rnd(s cos(a) 65536 / 2k), B = rnd(s sin(a) 65536 / 2k), all in double.
inline Frame make_frame(float x, float y, float size, float angle, float scale_factor, bool use_orientation)
{
    Frame f = {0, 0, 0, 0, 1, 0};
    const double s = (double)size * (double)scale_factor / 64.0;
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(s)) return f;
    if (!(s > 0.0) || s > kMaxStep) return f;
    if (std::fabs((double)x) > (double)kMaxCoord || std::fabs((double)y) > (double)kMaxCoord) return f;
    const double kPi = 3.1415926535897932384626433832795;
    const double a = (angle < 0.0f || !use_orientation) ? 0.0 : (double)angle * kPi / 180.0;
    const int k = (int)std::fmin((double)kMaxSub, std::fmax(1.0, std::ceil(s)));
    f.X0 = (int64_t)rnd((double)x * 65536.0);
    f.Y0 = (int64_t)rnd((double)y * 65536.0);
    f.A = (int32_t)rnd(s * std::cos(a) * 65536.0 / (2.0 * k));
    f.B = (int32_t)rnd(s * std::sin(a) * 65536.0 / (2.0 * k));
    f.k = k;
    f.valid = 1;
    return f;
}

// Sample (m, n) of the frame: m = (2u - 63) k + (2a + 1 - k) for patch column u and sub-sample a, n likewise from the
// row v and b.  Both run over the odd numbers of [-(64k - 1), 64k - 1].
PATCH_RULES_HD inline int64_t sample_x(const Frame &f, int64_t m, int64_t n) { return f.X0 + m * f.A - n * f.B; }
PATCH_RULES_HD inline int64_t sample_y(const Frame &f, int64_t m, int64_t n) { return f.Y0 + m * f.B + n * f.A; }

// The extremes of SX and SY over the samples of a patch.  SX and SY are linear in (m, n), and m and n reach both ends of
// their range independently, so the extremes are taken at the four corner samples: exact, not an estimate.
struct Extent { int64_t x0, x1, y0, y1; };
PATCH_RULES_HD inline Extent extent(const Frame &f)
{
    const int64_t e = (int64_t)kSide * f.k - 1;
    const int64_t ax = (f.A < 0 ? -(int64_t)f.A : (int64_t)f.A) * e, bx = (f.B < 0 ? -(int64_t)f.B : (int64_t)f.B) * e;
    return Extent{f.X0 - ax - bx, f.X0 + ax + bx, f.Y0 - ax - bx, f.Y0 + ax + bx};
}

// 0: invalid.  1: sampled, some sample outside 0 <= SX <= (W-1) 65536 or 0 <= SY <= (H-1) 65536.  2: every sample inside.
PATCH_RULES_HD inline int status(const Frame &f, int W, int H)
{
    if (!f.valid) return 0;
    const Extent e = extent(f);
    const bool inside = e.x0 >= 0 && e.x1 <= (int64_t)(W - 1) * 65536 && e.y0 >= 0 && e.y1 <= (int64_t)(H - 1) * 65536;
    return inside ? 2 : 1;
}

PATCH_RULES_HD inline int clampi(int64_t v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

// The pixels the taps of a patch can touch, and whether the kernel stages them in LDS.  The taps of a sample are at
// SX >> 16 and one beyond, clamped to the image: [bx0, bx0 + bw) x [by0, by0 + bh) holds them all.  An LDS row is `pitch`
// bytes: the box row behind the up to 15 bytes that precede it in its 16-byte block of the image.  The patch is staged
// iff pitch * rows of the box BEFORE clamping fits kStageBudget: the decision depends on the frame alone, the staged
// box (clamped) is never larger than the one decided on.
constexpr int kStageBudget = 40 * 1024;
struct Stage { int staged; int bx0, by0, bw, bh; int pitch; };
PATCH_RULES_HD inline Stage stage_plan(const Frame &f, int W, int H)
{
    const Extent e = extent(f);
    const int64_t fx0 = e.x0 >> 16, fx1 = (e.x1 >> 16) + 1, fy0 = e.y0 >> 16, fy1 = (e.y1 >> 16) + 1;
    const int64_t fw = fx1 - fx0 + 1, fh = fy1 - fy0 + 1;
    Stage st;
    st.staged = f.valid && ((fw + 30) / 16 * 16) * fh <= kStageBudget;
    st.bx0 = clampi(fx0, W - 1);
    st.by0 = clampi(fy0, H - 1);
    st.bw = clampi(fx1, W - 1) - st.bx0 + 1;
    st.bh = clampi(fy1, H - 1) - st.by0 + 1;
    st.pitch = (st.bw + 30) / 16 * 16;
    return st;
}

// Patch pixel (v, u).  src.row(cy) gives the handle of image row cy, src.at(row, cx) the pixel; cx, cy are clamped here,
// which replicates the border.  val = (256-fx)(256-fy) p00 + fx (256-fy) p01 + (256-fx) fy p10 + fx fy p11 per sample,
// the pixel is (sum of the k k vals + k k 32768) / (k k 65536) by integer division; the sum stays below 2^31.
template <typename Src>
PATCH_RULES_HD inline uint8_t sample_pixel(const Frame &f, int W, int H, int v, int u, const Src &src)
{
    const int k = f.k;
    const int64_t m0 = (int64_t)(2 * u - (kSide - 1)) * k + (1 - k), n0 = (int64_t)(2 * v - (kSide - 1)) * k + (1 - k);
    uint32_t sum = 0;
    for (int b = 0; b < k; b++) {
        int64_t SX = sample_x(f, m0, n0 + 2 * b), SY = sample_y(f, m0, n0 + 2 * b);
        for (int a = 0; a < k; a++, SX += 2 * (int64_t)f.A, SY += 2 * (int64_t)f.B) {
            const int64_t ix = SX >> 16, iy = SY >> 16;
            const uint32_t fx = (uint32_t)(SX & 0xFFFF) >> 8, fy = (uint32_t)(SY & 0xFFFF) >> 8;
            const int cx0 = clampi(ix, W - 1), cx1 = clampi(ix + 1, W - 1);
            const auto r0 = src.row(clampi(iy, H - 1)), r1 = src.row(clampi(iy + 1, H - 1));
            const uint32_t p00 = src.at(r0, cx0), p01 = src.at(r0, cx1), p10 = src.at(r1, cx0), p11 = src.at(r1, cx1);
            sum += (256 - fx) * (256 - fy) * p00 + fx * (256 - fy) * p01 + (256 - fx) * fy * p10 + fx * fy * p11;
        }
    }
    const uint32_t kk = (uint32_t)(k * k);
    return (uint8_t)((sum + kk * 32768u) / (kk * 65536u));
}

// an image in ordinary memory: the source of the kernel's direct path and of the CPU test
struct ImageSrc {
    const uint8_t *img;
    int64_t pitch;
    PATCH_RULES_HD const uint8_t *row(int cy) const { return img + (int64_t)cy * pitch; }
    PATCH_RULES_HD uint32_t at(const uint8_t *r, int cx) const { return r[cx]; }
};

}  // namespace patch_rules
