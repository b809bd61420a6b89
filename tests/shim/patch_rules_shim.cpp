// C entry points over opencv-dlco_amd/csrc/patch_rules.hpp for tests/test_patch_rules.py: pure host code, no libdlco.so.
#include "../../opencv-dlco_amd/csrc/patch_rules.hpp"

extern "C" {

// out = (X0, Y0, A, B, k, valid)
void shim_patch_frame(float x, float y, float size, float angle, float scale_factor, int use_orientation, int64_t *out)
{
    const patch_rules::Frame f = patch_rules::make_frame(x, y, size, angle, scale_factor, use_orientation != 0);
    out[0] = f.X0; out[1] = f.Y0; out[2] = f.A; out[3] = f.B; out[4] = f.k; out[5] = f.valid;
}

static patch_rules::Frame frame_of(const int64_t *fr)
{
    return patch_rules::Frame{fr[0], fr[1], (int32_t)fr[2], (int32_t)fr[3], (int32_t)fr[4], (int32_t)fr[5]};
}

int shim_patch_status(const int64_t *fr, int W, int H) { return patch_rules::status(frame_of(fr), W, H); }

// out = (staged, bx0, by0, bw, bh, pitch)
void shim_patch_stage(const int64_t *fr, int W, int H, int32_t *out)
{
    const patch_rules::Stage st = patch_rules::stage_plan(frame_of(fr), W, H);
    out[0] = st.staged; out[1] = st.bx0; out[2] = st.by0; out[3] = st.bw; out[4] = st.bh; out[5] = st.pitch;
}

int shim_patch_stage_budget() { return patch_rules::kStageBudget; }

// the 64 x 64 patch of a valid frame on img [H][pitch], by patch_rules::sample_pixel on ordinary memory
void shim_patch_sample(const uint8_t *img, int W, int H, int64_t pitch, const int64_t *fr, uint8_t *patch)
{
    const patch_rules::Frame f = frame_of(fr);
    const patch_rules::ImageSrc src{img, pitch};
    for (int v = 0; v < 64; v++)
        for (int u = 0; u < 64; u++) patch[v * 64 + u] = patch_rules::sample_pixel(f, W, H, v, u, src);
}

}  // extern "C"
