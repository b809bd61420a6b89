// detect — the keypoints of an image, over libdlco.so: the front of describe-image.
//
//     detect src_h5_img_file -out dst [-octaves n] [-threshold t] [-max n] [-device n] [-orient]
//
// src_h5_img_file holds "Image" [H,W] u8.  The detector is the library's own (the rule: csrc/detect_rules.hpp): a
// multi-scale determinant of the Hessian on box filters, -octaves n of them (1 .. 4, default 3), keypoints with a response
// of at least -threshold t (default 655360000: a determinant of 100 squared grey levels), the strongest -max n (default
// 100000) strongest first.  It is not OpenCV's SURF.  Without -orient it assigns no orientation: every angle is -1.  With
// -orient every keypoint gets the angle of the library's orientation rule (csrc/orient_rules.hpp, dlco_desc_detect_oriented),
// which describe-image uses unless it is given -upright.  Writes
//     "Image" [H,W] u8           copied through
//     "Keypoints" [n,4] f32      (x, y, size, angle): with "Image", what describe-image takes as its second argument
//     "Response" [n] i64         the response of every keypoint, descending
// and prints "Keypoints: n of n_found".
// The reference has no such tool.  A path that does not end in .h5/.hdf5 is a directory of .npy files with the same
// dataset names (dlco_io.hpp).
#include "dlco_io.hpp"

#include "../../include/dlco.h"

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <iostream>

using std::cout;
using std::endl;

int main(int argc, char **argv)
{
    int octaves = 3, device = 0;
    long long threshold = 655360000LL, max_kp = 100000;
    bool help = false, orient = false;
    const char *img = nullptr, *out = nullptr;
    for (int i = 1; i < argc; i++) {
        if (argv[i][0] == '-') {
            const bool has_val = i + 1 < argc;
            if (std::strcmp(argv[i], "-help") == 0) { help = true; continue; }
            if (std::strcmp(argv[i], "-orient") == 0) { orient = true; continue; }
            if (std::strcmp(argv[i], "-out") == 0 && has_val) { out = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-octaves") == 0 && has_val) { octaves = atoi(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-threshold") == 0 && has_val) { threshold = atoll(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-max") == 0 && has_val) { max_kp = atoll(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-device") == 0 && has_val) { device = atoi(argv[++i]); continue; }
            cout << "ERROR: Invalid " << argv[i] << " option." << endl;
            help = true;
        } else {
            if (!img) { img = argv[i]; continue; }
            help = true;
        }
    }
    if (!img || !out) help = true;
    if (octaves < 1 || octaves > 4) {
        cout << "ERROR: -octaves must be 1 .. 4." << endl;
        help = true;
    }
    if (threshold < 1 || max_kp < 1) {
        cout << "ERROR: -threshold and -max must be at least 1." << endl;
        help = true;
    }
    if (help) {
        cout << endl;
        cout << "Usage: detect src_h5_img_file -out dst_h5_filename" << endl;
        cout << "        [-octaves n] [-threshold t] [-max n] [-device n]" << endl;
        cout << "        [-orient]      assign every keypoint its angle (default: every angle is -1)" << endl;
        cout << endl;
        return 1;
    }
    dlco_desc_ctx *ctx = nullptr;
    try {
        std::vector<size_t> ishape;
        std::vector<uint8_t> image;
        printf("Image: [%s]\n", img);
        dlco_io::read_dataset<uint8_t>(img, "Image", ishape, image);
        if (ishape.size() != 2 || ishape[0] < 1 || ishape[1] < 1 || ishape[0] > 32768 || ishape[1] > 32768)
            throw std::runtime_error("Image must be [H,W] with 1 <= H, W <= 32768");
        printf("Image: %zu x %zu\n", ishape[1], ishape[0]);
        if (dlco_desc_create(&ctx, 1.4f, 8, 1, device) != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(nullptr));
        auto ck = [&](int rc) { if (rc != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(ctx)); };
        ck(dlco_desc_set_image(ctx, image.data(), (int32_t)ishape[1], (int32_t)ishape[0], (int64_t)ishape[1]));
        const auto t0 = std::chrono::steady_clock::now();
        // no more rows than there can be keypoints: no two keypoints of an octave are neighbours, so an octave has fewer than a
        // quarter of its grid points, and the grids together fewer points than 4/3 of the image's pixels
        const int64_t rows = std::min<int64_t>(max_kp, (int64_t)image.size());
        std::vector<float> kp((size_t)rows * 4);
        std::vector<int64_t> resp((size_t)rows);
        int64_t n = 0, found = 0;
        ck((orient ? dlco_desc_detect_oriented : dlco_desc_detect)(ctx, octaves, threshold, rows, kp.data(), resp.data(), &n, &found));
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        {
            dlco_io::Writer wr(out);
            wr.write<uint8_t>("Image", image.data(), ishape[0], ishape[1]);
            wr.write<float>("Keypoints", kp.data(), (size_t)n, 4);
            wr.write_vec<int64_t>("Response", resp.data(), (size_t)n);
        }
        printf("Keypoints: %lld of %lld\n", (long long)n, (long long)found);
        printf("Total: %.09f sec\n\n", sec);
        dlco_desc_destroy(ctx);
    } catch (const std::exception &e) {
        if (ctx) dlco_desc_destroy(ctx);
        std::fprintf(stderr, "detect: %s\n", e.what());
        return 2;
    }
    return 0;
}
