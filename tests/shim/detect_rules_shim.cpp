// C entry points over opencv-dlco_amd/csrc/detect_rules.hpp for tests/test_detect_rules.py: pure host code, no libdlco.so.
#include "../../opencv-dlco_amd/csrc/detect_rules.hpp"

namespace dr = detect_rules;

extern "C" {

// out = (filter side of (o, i), margin of o, step of o, grid size of o along `extent` pixels)
void shim_detect_geometry(int o, int i, int extent, int32_t *out)
{
    out[0] = dr::filter_side(o, i); out[1] = dr::margin(o); out[2] = dr::step(o); out[3] = dr::grid_size(extent, o);
}

int64_t shim_detect_normalise(int64_t D, int L) { return dr::normalise(D, L); }

// the inclusive box on S [..][pitch], which may hold the sums modulo 2^32
int64_t shim_detect_box(const uint32_t *S, int64_t pitch, int x0, int y0, int x1, int y1)
{
    return dr::box(dr::IntegralSrc{S, pitch}, x0, y0, x1, y1);
}

// S [(H+1)][(W+1)] of img [H][pitch]
void shim_detect_integral(const uint8_t *img, int W, int H, int64_t pitch, uint32_t *S) { dr::integral_host(img, W, H, pitch, S); }

// R [4][ny][nx] of octave o
void shim_detect_responses(const uint32_t *S, int W, int H, int o, int64_t *R)
{
    dr::HostVolume V;
    dr::responses_host(S, W, H, o, V);
    for (size_t k = 0; k < V.R.size(); k++) R[k] = V.R[k];
}

double shim_detect_offset(int64_t Rm, int64_t R0, int64_t Rp) { return dr::offset(Rm, R0, Rp); }
double shim_detect_offset6(int64_t Rm, int64_t R0, int64_t Rp) { return dr::offset6(Rm, R0, Rp); }

// the whole detection on S: returns n_found; the first min(n_found, cap) keypoints in the rule's order as kp [.][4] =
// (x, y, size, -1), resp [.] and where [.][4] = (octave, layer, j, i)
int64_t shim_detect(const uint32_t *S, int W, int H, int n_octaves, int64_t threshold, int64_t cap, float *kp, int64_t *resp, int32_t *where)
{
    std::vector<dr::Keypoint> out;
    dr::detect_host(S, W, H, n_octaves, threshold, out);
    for (int64_t k = 0; k < (int64_t)out.size() && k < cap; k++) {
        kp[4 * k] = out[k].x; kp[4 * k + 1] = out[k].y; kp[4 * k + 2] = out[k].size; kp[4 * k + 3] = -1.0f;
        resp[k] = out[k].R;
        where[4 * k] = out[k].octave; where[4 * k + 1] = out[k].layer; where[4 * k + 2] = out[k].j; where[4 * k + 3] = out[k].i;
    }
    return (int64_t)out.size();
}

}  // extern "C"
