// orient_rules.hpp — how a keypoint gets its angle (dlco_desc_orient, dlco_desc_detect_oriented): Haar-wavelet responses on
// the detector's integral image around the keypoint, weighted, binned by direction, and the strongest 60-degree window of the
// bins.  The rule in integers, stated once for the host, the kernel (kernels_orient.hip) and the CPU test
// (tests/shim/orient_rules_shim.cpp).  Plain C++: no HIP header, no device, no I/O.
//
// This is NOT the orientation of OpenCV's SURF, which nothing here can run or pin, and no parity with it is claimed.  It is
// a rule of this library: everything up to the winning vector (SX, SY) is integer and exact, so that the vector is the same
// on every machine and the tests compare with equality; the only floating point is one atan2 on the host (angle_of).
//
// Out of scope: a device-memory form of the oriented keypoints (the angle is defined through the host's atan2); more than
// one orientation per keypoint.
//
// Validity.  A keypoint (x, y, size, .) is valid iff x, y and size are finite, size > 0 and |x|, |y| <= 2^20; the angle it
// comes with is ignored.  An invalid keypoint has status 0, vector (0, 0) and angle -1.
//
// Centre and scale, in double: X = floor((double)x + 0.5), Y likewise; s = min(128, max(1, floor((double)size / 7.5 + 0.5))),
// clamped before the conversion to int.  That is about 1.2 size / 9: the detector's sizes 9 .. 195 give s = 1 .. 26.  Every
// operation is one correctly rounded IEEE operation, so the host and the kernel agree.
//
// Samples.  Offsets (i, j) in [-6, 6]^2 with d2 = i^2 + j^2 < 36: 109 of them, in the order j ascending, then i ascending
// (rows j = -5 .. 5 of 7 9 11 11 11 11 11 11 11 9 7).  The centre of a sample is c = (X + i s, Y + j s).  A sample is used
// iff its whole Haar square [cx - 2s, cx + 2s] x [cy - 2s, cy + 2s] lies inside the image; no border is replicated, a sample
// that is skipped contributes nothing.
//
// Haar responses, from detect_rules::box on the integral image S (uint32 modulo 2^32; exact, as no box of the rule exceeds
// 255 * 256 * 513 < 2^32).  The centre column and the centre row are left out, so the rule is symmetric about the pixel:
//   dx = box(cx+1, cy-2s, cx+2s, cy+2s) - box(cx-2s, cy-2s, cx-1, cy+2s)
//   dy = box(cx-2s, cy+1, cx+2s, cy+2s) - box(cx-2s, cy-2s, cx+2s, cy-1)
//   N(d) = sgn(d) ((16 |d| + 4 s^2) / (8 s^2)) by integer division: |d| <= 255 * 2s (4s + 1), so |N| <= 5100
//   g = (w[d2] N(dx), w[d2] N(dy)),  w[d2] = round(1024 exp(-d2 / 8)) as literals (no entry within 0.0079 of a tie)
//
// Bins.  36 boundary vectors b_k ~ 1024 (cos 10k deg, sin 10k deg): nine literals and b_{k+9} = (-b_k.y, b_k.x), so the table
// is exactly invariant under quarter turns.  Consecutive boundaries are strictly counter-clockwise, so a non-zero g falls
// into exactly one bin k: cross(b_k, g) >= 0 and cross(b_{k+1 mod 36}, g) < 0, with cross(a, g) = a.x g.y - a.y g.x in int64.
// g = (0, 0) falls into none.  HX[k], HY[k] are the sums of g over bin k.
//
// Window.  For k = 0 .. 35, (SX, SY) = the sum of bins k .. k+5 (mod 36), 60 degrees; score = SX^2 + SY^2.  The winner is
// the largest score, a tie goes to the smallest k; the keypoint's vector is the winner's (SX, SY).
//   Bounds: a component of g is at most 1024 * 5100 < 2^23 in size; a bin or a window sums at most 109 samples, so
// |HX|, |SX| <= 109 * 1024 * 5100 < 2^30 (a bin fits an int32) and score <= 2 (109 * 1024 * 5100)^2 < 2^60.
//
// Angle, on the host only: angle_of(0, 0) = -1, none, which patch_rules::make_frame treats as upright; otherwise
// a = atan2((double)SY, (double)SX) * 180 / pi, plus 360 if a < 0, rounded to float, and a float >= 360 becomes 0.  The axes
// are the image's, y down: the convention of make_frame, whose patch x-axis points along (cos a, sin a).
//
// Status.  0 invalid; 1 valid and at least one of the 109 samples was skipped; 2 all 109 samples were used.
#pragma once

#include "detect_rules.hpp"

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define ORIENT_RULES_HD __host__ __device__
#else
#define ORIENT_RULES_HD
#endif

namespace orient_rules {

constexpr int kSamples = 109;
constexpr int kBins = 36;
constexpr int kWindow = 6;                     // bins of a window
constexpr int kMaxScale = 128;
constexpr int kRows = 11;                      // sample rows j = -5 .. 5 (j = +-6 has no offset with d2 < 36)
constexpr double kMaxCoord = 1048576.0;        // 2^20

ORIENT_RULES_HD inline int weight(int d2)
{
    constexpr int w[36] = {1024, 904, 797, 704, 621, 548, 484, 427, 377, 332, 293, 259, 228, 202, 178, 157, 139, 122,
                           108,  95,  84,  74,  65,  58,  51,  45,  40,  35,  31,  27,  24,  21,  19,  17,  15,  13};
    return w[d2];
}

struct Vec { int64_t x, y; };

// b_k for k = 0 .. 35
ORIENT_RULES_HD inline Vec boundary(int k)
{
    constexpr int bx[9] = {1024, 1008, 962, 887, 784, 658, 512, 350, 178};
    constexpr int by[9] = {0, 178, 350, 512, 658, 784, 887, 962, 1008};
    const int q = k / 9, r = k - 9 * q;
    const int64_t x = bx[r], y = by[r];
    return q == 0 ? Vec{x, y} : q == 1 ? Vec{-y, x} : q == 2 ? Vec{-x, -y} : Vec{y, -x};
}

ORIENT_RULES_HD inline int64_t cross(Vec a, Vec g) { return a.x * g.y - a.y * g.x; }

// The bin of g, -1 for (0, 0).  The definition above, evaluated through the table's symmetry: q quarter turns take g back to
// g' with g'.x > 0 and g'.y >= 0, and cross(b_{k+9q}, g) = cross(b_k, g') exactly, so the bin is 9 q + r with r the bin of g'
// among b_0 .. b_9.  There cross(b_0, g') = 1024 g'.y >= 0 and cross(b_9, g') = -1024 g'.x < 0 hold already, and the
// boundaries b_1 .. b_8 with cross(b_r, g') >= 0 are the first ones (they ascend in angle below g'): r is their number.
ORIENT_RULES_HD inline int bin_of(Vec g)
{
    if (g.x == 0 && g.y == 0) return -1;
    int q;
    Vec t;
    if (g.x > 0 && g.y >= 0) { q = 0; t = g; }
    else if (g.x <= 0 && g.y > 0) { q = 1; t = Vec{g.y, -g.x}; }
    else if (g.x < 0 && g.y <= 0) { q = 2; t = Vec{-g.x, -g.y}; }
    else { q = 3; t = Vec{-g.y, g.x}; }
    int r = 0;
    for (int k = 1; k < 9; k++) r += cross(boundary(k), t) >= 0 ? 1 : 0;
    return 9 * q + r;
}

// sample t = 0 .. 108 in the rule's order: its offset (i, j)
struct Offset { int i, j; };
ORIENT_RULES_HD inline Offset sample_offset(int t)
{
    constexpr int start[kRows + 1] = {0, 7, 16, 27, 38, 49, 60, 71, 82, 93, 102, 109};
    constexpr int half[kRows] = {3, 4, 5, 5, 5, 5, 5, 5, 5, 4, 3};
    int r = 0;
    while (t >= start[r + 1]) r++;
    return Offset{t - start[r] - half[r], r - 5};
}

// centre and scale of a keypoint; valid == 0: status 0
struct Centre { int X, Y, s, valid; };
ORIENT_RULES_HD inline Centre centre_of(float x, float y, float size)
{
    Centre c = {0, 0, 1, 0};
    if (!__builtin_isfinite(x) || !__builtin_isfinite(y) || !__builtin_isfinite(size)) return c;
    if (!(size > 0.0f)) return c;
    if (__builtin_fabs((double)x) > kMaxCoord || __builtin_fabs((double)y) > kMaxCoord) return c;
    c.X = (int)__builtin_floor((double)x + 0.5);
    c.Y = (int)__builtin_floor((double)y + 0.5);
    double s = __builtin_floor((double)size / 7.5 + 0.5);
    s = s < 1.0 ? 1.0 : (s > (double)kMaxScale ? (double)kMaxScale : s);
    c.s = (int)s;
    c.valid = 1;
    return c;
}

// the whole Haar square of a sample centred at (cx, cy) lies inside a W x H image
ORIENT_RULES_HD inline bool sample_used(int cx, int cy, int s, int W, int H)
{
    return cx - 2 * s >= 0 && cx + 2 * s <= W - 1 && cy - 2 * s >= 0 && cy + 2 * s <= H - 1;
}

// N(d) for |d| <= 255 * 2s (4s + 1), which every Haar response is: 16 |d| + 4 s^2 <= 16 * 255 * 256 * 513 + 65536 < 2^30, so the
// division is one of 32-bit numbers
ORIENT_RULES_HD inline int64_t normalise(int64_t d, int s)
{
    const uint32_t a = (uint32_t)(d < 0 ? -d : d), q = (uint32_t)(s * s);
    const int64_t n = (16u * a + 4u * q) / (8u * q);
    return d < 0 ? -n : n;
}

// g of the used sample with offset (i, j) around (X, Y).  S is any object with at(y, x) -> uint32_t, as for detect_rules::box
template <typename Src>
ORIENT_RULES_HD inline Vec gradient(const Src &S, int X, int Y, int s, int i, int j)
{
    namespace dr = detect_rules;
    const int cx = X + i * s, cy = Y + j * s, h = 2 * s;
    const int64_t dx = dr::box(S, cx + 1, cy - h, cx + h, cy + h) - dr::box(S, cx - h, cy - h, cx - 1, cy + h);
    const int64_t dy = dr::box(S, cx - h, cy + 1, cx + h, cy + h) - dr::box(S, cx - h, cy - h, cx + h, cy - 1);
    const int64_t w = weight(i * i + j * j);
    return Vec{w * normalise(dx, s), w * normalise(dy, s)};
}

// window k of the histogram: the sum of bins k .. k+5 (mod 36).  Hist is any object with x(k), y(k) -> int64_t
template <typename Hist>
ORIENT_RULES_HD inline Vec window(const Hist &h, int k)
{
    Vec v = {0, 0};
    for (int t = 0; t < kWindow; t++) {
        const int b = k + t < kBins ? k + t : k + t - kBins;
        v.x += h.x(b); v.y += h.y(b);
    }
    return v;
}

ORIENT_RULES_HD inline int64_t score(Vec v) { return v.x * v.x + v.y * v.y; }

// (score a, window ka) wins against (score b, window kb)
ORIENT_RULES_HD inline bool wins(int64_t a, int ka, int64_t b, int kb) { return a != b ? a > b : ka < kb; }

// the angle of a winning vector in degrees, on the host only; -1: none
inline float angle_of(int64_t SX, int64_t SY)
{
    if (SX == 0 && SY == 0) return -1.0f;
    const double kPi = 3.1415926535897932384626433832795;
    double a = std::atan2((double)SY, (double)SX) * 180.0 / kPi;
    if (a < 0.0) a += 360.0;
    const float f = (float)a;
    return f >= 360.0f ? 0.0f : f;
}

// ---- the rule on the host: what the kernel must reproduce ------------------------------------------------------------------
struct Result { int64_t SX, SY; int status; };

struct HostHist {
    int64_t hx[kBins], hy[kBins];
    int64_t x(int k) const { return hx[k]; }
    int64_t y(int k) const { return hy[k]; }
};

// S [(H+1)][pitch] is the integral image of a W x H image; keypoint = (x, y, size, angle), the angle is ignored
inline Result orient_host(const uint32_t *S, int64_t pitch, int W, int H, const float *keypoint)
{
    Result r = {0, 0, 0};
    const Centre c = centre_of(keypoint[0], keypoint[1], keypoint[2]);
    if (!c.valid) return r;
    const detect_rules::IntegralSrc src{S, pitch};
    HostHist h = {};
    int used = 0;
    for (int t = 0; t < kSamples; t++) {
        const Offset o = sample_offset(t);
        if (!sample_used(c.X + o.i * c.s, c.Y + o.j * c.s, c.s, W, H)) continue;
        used++;
        const Vec g = gradient(src, c.X, c.Y, c.s, o.i, o.j);
        const int b = bin_of(g);
        if (b >= 0) { h.hx[b] += g.x; h.hy[b] += g.y; }
    }
    Vec best = window(h, 0);
    int best_k = 0;
    for (int k = 1; k < kBins; k++) {
        const Vec v = window(h, k);
        if (wins(score(v), k, score(best), best_k)) { best = v; best_k = k; }
    }
    r.SX = best.x; r.SY = best.y;
    r.status = used == kSamples ? 2 : 1;
    return r;
}

}  // namespace orient_rules
