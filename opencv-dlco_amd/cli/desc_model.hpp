// desc_model.hpp — how the descriptor tools read a trained model, shared by comp-uprjdists, describe, describe-image
// and eval-patches so that they select the same pooling regions from the same files and print the same lines:
// "PRFilters" [n,64,64] f32, row `rowid` of pr-learn's "w" (src/comp-uprjdists.cpp:143-232), "Patches" [n,64,64] u8
// (describe-image: "Image" [H,W] u8 and "Keypoints" [n,4] f32 in their place), and, for the tools that apply it,
// pj-learn's "W" [r, nsel*8].
#pragma once

#include "../../include/dlco.h"
#include "dlco_io.hpp"

#include <cstdio>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

namespace desc_model {

struct PRFilters {
    std::vector<size_t> shape;
    std::vector<float> data;
};

inline void load_pr_filters(const char *flt, PRFilters &f)
{
    std::cout << "Load PRFilters." << std::endl;
    dlco_io::read_dataset<float>(flt, "PRFilters", f.shape, f.data);
    if (f.shape.size() != 3 || f.shape[1] * f.shape[2] != 4096) throw std::runtime_error("PRFilters must be [n,64,64]");
    dlco_io::term_progress(1.0, -1);
}

inline void load_patches(const char *img, std::vector<size_t> &shape, std::vector<uint8_t> &patches)
{
    std::cout << "Load Patches." << std::endl;
    dlco_io::read_dataset<uint8_t>(img, "Patches", shape, patches);
    if (shape.size() != 3 || shape[1] != 64 || shape[2] != 64) throw std::runtime_error("Patches must be [n,64,64]");
    dlco_io::term_progress(1.0, -1);
}

// describe-image's input: one grey image and a detector's keypoints (x, y, size, angle) on it
inline void load_image_keypoints(const char *img, std::vector<size_t> &ishape, std::vector<uint8_t> &image, std::vector<size_t> &kshape,
                                 std::vector<float> &keypoints)
{
    std::cout << "Load Image." << std::endl;
    dlco_io::read_dataset<uint8_t>(img, "Image", ishape, image);
    if (ishape.size() != 2 || ishape[0] < 1 || ishape[1] < 1 || ishape[0] > 32768 || ishape[1] > 32768)
        throw std::runtime_error("Image must be [H,W] with 1 <= H, W <= 32768");
    dlco_io::read_dataset<float>(img, "Keypoints", kshape, keypoints);
    if (kshape.size() != 2 || kshape[0] < 1 || kshape[1] != 4) throw std::runtime_error("Keypoints must be a non-empty [n,4] table");
    dlco_io::term_progress(1.0, -1);
}

// SelectPRFilters on row widx of prj's "w": sPR [nsel, 4096]
inline void select(const PRFilters &f, const char *prj, int widx, std::vector<float> &sPR, int32_t &nsel)
{
    std::vector<size_t> wshape;
    std::vector<float> w;
    printf("Load Learnt Filters: [%s]#%i\n", prj, widx);
    dlco_io::read_dataset<float>(prj, "w", wshape, w);
    if (wshape.size() != 2 || widx < 0 || (size_t)widx >= wshape[0]) throw std::runtime_error("w has no such row");
    const size_t wcols = wshape[1];
    if (wcols * 8 != f.shape[0]) throw std::runtime_error("PRFilters needs 8 rows per column of w");
    const float *wrow = w.data() + (size_t)widx * wcols;
    nsel = 0;
    if (dlco_desc_select_filters(f.data.data(), (int32_t)f.shape[0], 4096, wrow, (int32_t)wcols, nullptr, &nsel) != DLCO_OK)
        throw std::runtime_error("filter selection failed");
    if (nsel < 1) throw std::runtime_error("no pooling region selected (w has no positive entry on a non-zero filter)");
    sPR.resize((size_t)nsel * 4096);
    dlco_desc_select_filters(f.data.data(), (int32_t)f.shape[0], 4096, wrow, (int32_t)wcols, sPR.data(), &nsel);
    printf("PRFilters: %i x %i\n", nsel, 4096);
    printf("Descriptor size: %i\n", nsel * 8);
}

// a descriptor context with the reference's InitSigma / nAngleBins / bNorm (src/comp-uprjdists.cpp:64-68) and sPR set
inline dlco_desc_ctx *open_ctx(const std::vector<float> &sPR, int32_t nsel, int device)
{
    dlco_desc_ctx *ctx = nullptr;
    if (dlco_desc_create(&ctx, 1.4f, 8, 1, device) != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(nullptr));
    if (dlco_desc_set_filters(ctx, sPR.data(), nsel) != DLCO_OK) {
        const std::string e = dlco_desc_last_error(ctx);
        dlco_desc_destroy(ctx);
        throw std::runtime_error(e);
    }
    return ctx;
}

// pj-learn's "W" [r, nsel*8] (what eval-fpr95 takes as its W file), checked against the selected filters before any
// device is touched
inline void load_projection(const char *pj, int32_t nsel, std::vector<size_t> &wshape, std::vector<float> &W)
{
    printf("Load Projection: [%s]\n", pj);
    dlco_io::read_dataset<float>(pj, "W", wshape, W);
    if (wshape.size() != 2 || wshape[0] < 1) throw std::runtime_error("W must be [r, F]");
    if (wshape[1] != (size_t)nsel * 8)
        throw std::runtime_error("W has " + std::to_string(wshape[1]) + " columns, the selected filters give a descriptor of " +
                                 std::to_string((size_t)nsel * 8));
    printf("Projection: %zu x %zu\n", wshape[0], wshape[1]);
}

}  // namespace desc_model
