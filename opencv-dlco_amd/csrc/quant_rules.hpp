// quant_rules.hpp — how a float descriptor row becomes a row of bytes (dlco_desc_quant_fit / dlco_desc_quantize, the _u8
// forms of describe, the tool `quantize`): the rule stated once for the host, the kernel (kernels_match_u8.hip) and the
// CPU test (tests/shim/quant_rules_shim.cpp).  Plain C++: no HIP header, no device, no I/O.
//
// This is NOT OpenCV's VGG dsc_normalize, which nothing here can run or pin.  It is a rule of this library: one global
// scale s > 0 and one offset o_k per dimension.  Squared L2 distances do not see the offsets, so
// ||u_a - u_b|| ~ s ||y_a - y_b|| with an error of at most 1 per coordinate as long as nothing clamps: the geometry
// pj-learn trained is kept.
//
// One element:  t = y - o_k (float, rounded), v = t * s (float, rounded on its own: never an FMA with the subtraction),
// q = rintf(v) (half to even); the byte is 0 if v is NaN, else clamp(q, 0, 255): -inf gives 0, +inf gives 255.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define QUANT_RULES_HD __host__ __device__
#else
#define QUANT_RULES_HD
#endif

namespace quant_rules {

constexpr int kMaxDim = 1024;                  // r of a quantiser at most (the limit of the match calls)

QUANT_RULES_HD inline uint8_t quantize_one(float y, float o, float s)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const float v = __fmul_rn(__fsub_rn(y, o), s);
#else
    volatile float t = y - o;                  // the store rounds the difference before the product is formed
    const float v = t * s;
#endif
    if (!(v == v)) return 0;
    const float q = rintf(v);
    if (q <= 0.0f) return 0;
    if (q >= 255.0f) return 255;
    return (uint8_t)q;
}

// bytes out [n][r] of rows Y [n][r]; offset == nullptr: all offsets are zero
inline void quantize(const float *Y, int64_t n, int r, float s, const float *offset, uint8_t *out)
{
    for (int64_t i = 0; i < n; i++)
        for (int k = 0; k < r; k++) out[i * r + k] = quantize_one(Y[i * r + k], offset ? offset[k] : 0.0f, s);
}

// The quantiser fitted to a sample Y [n][r] of finite values, n >= 1: o_k = min_i Y[i][k], R = max_k (max_i Y[i][k] - o_k)
// with the subtraction in float, s = 255 / R, or 1 when R == 0.  The sample itself never clamps.  Returns false on a
// non-finite entry or a range beyond float; the outputs hold nothing of use then.
inline bool fit(const float *Y, int64_t n, int r, float *scale, float *offset)
{
    for (int64_t i = 0; i < n * r; i++)
        if (!std::isfinite(Y[i])) return false;
    float R = 0.0f;
    for (int k = 0; k < r; k++) {
        float lo = Y[k], hi = Y[k];
        for (int64_t i = 1; i < n; i++) {
            const float v = Y[i * r + k];
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
        offset[k] = lo;
        volatile float range = hi - lo;
        R = range > R ? (float)range : R;
    }
    if (!std::isfinite(R)) return false;       // a range beyond float: no scale fits
    *scale = R == 0.0f ? 1.0f : 255.0f / R;
    return true;
}

inline bool scale_ok(float s) { return std::isfinite(s) && s > 0.0f; }

}  // namespace quant_rules
