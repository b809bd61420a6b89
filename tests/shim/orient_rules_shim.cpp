// C entry points over opencv-dlco_amd/csrc/orient_rules.hpp for tests/test_orient_rules.py: pure host code, no libdlco.so.
#include "../../opencv-dlco_amd/csrc/orient_rules.hpp"

namespace orr = orient_rules;

extern "C" {

// w [36] and b [36][2]
void shim_orient_tables(int32_t *w, int64_t *b)
{
    for (int d2 = 0; d2 < 36; d2++) w[d2] = orr::weight(d2);
    for (int k = 0; k < orr::kBins; k++) { b[2 * k] = orr::boundary(k).x; b[2 * k + 1] = orr::boundary(k).y; }
}

// offsets [109][2] = (i, j) in the rule's order
void shim_orient_offsets(int32_t *ij)
{
    for (int t = 0; t < orr::kSamples; t++) { ij[2 * t] = orr::sample_offset(t).i; ij[2 * t + 1] = orr::sample_offset(t).j; }
}

// out = (X, Y, s, valid)
void shim_orient_centre(float x, float y, float size, int32_t *out)
{
    const orr::Centre c = orr::centre_of(x, y, size);
    out[0] = c.X; out[1] = c.Y; out[2] = c.s; out[3] = c.valid;
}

int shim_orient_bin(int64_t gx, int64_t gy) { return orr::bin_of(orr::Vec{gx, gy}); }

float shim_orient_angle_of(int64_t SX, int64_t SY) { return orr::angle_of(SX, SY); }

// the whole rule on S [(H+1)][(W+1)] for keypoints [n][4]: vectors [n][2], status [n], angles [n]
void shim_orient(const uint32_t *S, int W, int H, const float *keypoints, int64_t n, int64_t *vectors, uint8_t *status, float *angles)
{
    for (int64_t k = 0; k < n; k++) {
        const orr::Result r = orr::orient_host(S, (int64_t)W + 1, W, H, keypoints + 4 * k);
        vectors[2 * k] = r.SX; vectors[2 * k + 1] = r.SY;
        status[k] = (uint8_t)r.status;
        angles[k] = orr::angle_of(r.SX, r.SY);
    }
}

}  // extern "C"
