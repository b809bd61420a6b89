// describe-image — the learnt descriptor of every keypoint of an image, over libdlco.so.
//
//     describe-image src_h5_filter_file src_h5_img_file -prj src_h5_prj_file -id rowid -pj pj_model -out dst
//                    [-quant quant_file] [-scale f] [-upright] [-patches] [-device n]
//
// The model files are describe's ("PRFilters", row `rowid` of pr-learn's "w", pj-learn's "W").  src_h5_img_file holds
// "Image" [H,W] u8 and "Keypoints" [n,4] f32 = (x, y, size, angle) with cv::KeyPoint's meaning.  A 64 x 64 patch is
// sampled around every keypoint on the device (the rule: csrc/patch_rules.hpp; it covers size * f source pixels, -scale f,
// default 6.25; -upright ignores the angles) and described as `describe` would.  Writes
//     "Descriptor" [n, r] f32    what `match` reads; the rows of invalid keypoints are zero
//     "Status" [n] u8            0 invalid, 1 sampled partly outside the image (border replicated), 2 wholly inside
//     "Patches" [n,64,64] u8     with -patches: the sampled patches, the input of describe, comp-uprjdists and comp-fulldists
// With -quant quant_file ("QuantScale", "QuantOffset": an output of `quantize`) the rows are quantised on the device and
// "DescriptorU8" [n, r] u8 with the two quantiser datasets takes the place of "Descriptor"; the row of an invalid keypoint
// is then the quantisation of the zero vector.
// The reference has no such tool.  A path that does not end in .h5/.hdf5 is a directory of .npy files with the same
// dataset names (dlco_io.hpp).
#include "desc_model.hpp"
#include "quant_io.hpp"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

using std::cout;
using std::endl;

int main(int argc, char **argv)
{
    int widx = 0, device = 0;
    bool help = false, upright = false, want_patches = false;
    float scale = 6.25f;
    const char *flt = nullptr, *img = nullptr, *prj = nullptr, *pj = nullptr, *out = nullptr, *quant = nullptr;
    const size_t sChunk = 2048;                             // keypoints per library call: host memory holds one chunk of patches
    for (int i = 1; i < argc; i++) {
        if (argv[i][0] == '-') {
            const bool has_val = i + 1 < argc;
            if (std::strcmp(argv[i], "-help") == 0) { help = true; continue; }
            if (std::strcmp(argv[i], "-prj") == 0 && has_val) { prj = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-id") == 0 && has_val) { widx = atoi(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-pj") == 0 && has_val) { pj = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-out") == 0 && has_val) { out = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-scale") == 0 && has_val) { scale = (float)atof(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-upright") == 0) { upright = true; continue; }
            if (std::strcmp(argv[i], "-patches") == 0) { want_patches = true; continue; }
            if (std::strcmp(argv[i], "-quant") == 0 && has_val) { quant = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-device") == 0 && has_val) { device = atoi(argv[++i]); continue; }
            cout << "ERROR: Invalid " << argv[i] << " option." << endl;
            help = true;
        } else {
            if (!flt) { flt = argv[i]; continue; }
            if (!img) { img = argv[i]; continue; }
            help = true;
        }
    }
    if (!flt || !img || !out || !prj || !pj) help = true;
    if (!(scale > 0.0f) || !std::isfinite(scale)) {
        cout << "ERROR: -scale must be positive." << endl;
        help = true;
    }
    if (help) {
        cout << endl;
        cout << "Usage: describe-image src_h5_filter_file src_h5_img_file" << endl;
        cout << "        -prj src_h5_prj_file -id src_h5_prj_matrix_rowid -pj src_h5_pj_file -out dst_h5_filename" << endl;
        cout << "        [-quant quant_file] [-scale f] [-upright] [-patches] [-device n]" << endl;
        cout << endl;
        return 1;
    }
    dlco_desc_ctx *ctx = nullptr;
    try {
        desc_model::PRFilters filters;
        std::vector<size_t> ishape, kshape, wshape;
        std::vector<uint8_t> image;
        std::vector<float> kp, sPR, W;
        int32_t nsel = 0;
        desc_model::load_pr_filters(flt, filters);
        printf("Image: [%s]\n", img);
        desc_model::load_image_keypoints(img, ishape, image, kshape, kp);
        desc_model::select(filters, prj, widx, sPR, nsel);
        desc_model::load_projection(pj, nsel, wshape, W);
        const size_t n = kshape[0], r = wshape[0];
        printf("Image: %zu x %zu, %zu keypoints\n", ishape[1], ishape[0], n);
        float qscale = 0.f;
        std::vector<float> qoff;
        if (quant) quant_io::read(quant, r, qscale, qoff);

        ctx = desc_model::open_ctx(sPR, nsel, device);
        auto ck = [&](int rc) { if (rc != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(ctx)); };
        ck(dlco_desc_set_projection(ctx, W.data(), (int32_t)r, (int32_t)wshape[1]));
        ck(dlco_desc_set_image(ctx, image.data(), (int32_t)ishape[1], (int32_t)ishape[0], (int64_t)ishape[1]));
        if (quant) ck(dlco_desc_set_quantizer(ctx, qscale, qoff.data(), (int32_t)r));
        cout << "Start Compute Descriptors: #" << n << endl;
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint8_t> status(n), patches;
        if (want_patches) patches.resize(n * 4096);
        size_t by_status[3] = {0, 0, 0};
        {
            dlco_io::Writer wr(out);
            if (quant) {
                dlco_io::RowStream<uint8_t> ds(wr, "DescriptorU8", n, r, 128, r, 0);
                std::vector<uint8_t> rows(std::min(sChunk, n) * r);
                for (size_t p0 = 0; p0 < n; p0 += sChunk) {
                    const size_t cnt = std::min(sChunk, n - p0);
                    const float *k = kp.data() + p0 * 4;
                    ck(dlco_desc_describe_keypoints_u8(ctx, k, (int64_t)cnt, scale, upright ? 0 : 1, rows.data(), status.data() + p0));
                    if (want_patches)
                        ck(dlco_desc_extract_patches(ctx, k, (int64_t)cnt, scale, upright ? 0 : 1, patches.data() + p0 * 4096, nullptr));
                    ds.write_rows(p0, cnt, rows.data());
                    printf("\rStep: %zu / %zu", p0 + cnt, n);
                    fflush(stdout);
                }
            } else {
                dlco_io::RowStream<float> ds(wr, "Descriptor", n, r, 128, r, 0);
                std::vector<float> rows(std::min(sChunk, n) * r);
                for (size_t p0 = 0; p0 < n; p0 += sChunk) {
                    const size_t cnt = std::min(sChunk, n - p0);
                    const float *k = kp.data() + p0 * 4;
                    ck(dlco_desc_describe_keypoints(ctx, k, (int64_t)cnt, scale, upright ? 0 : 1, rows.data(), status.data() + p0));
                    if (want_patches)
                        ck(dlco_desc_extract_patches(ctx, k, (int64_t)cnt, scale, upright ? 0 : 1, patches.data() + p0 * 4096, nullptr));
                    for (size_t i = 0; i < cnt * r; i++)
                        if (!(rows[i] == rows[i]) || rows[i] > 3.0e38f || rows[i] < -3.0e38f) { cout << "\nDescriptor contains NaN\n"; dlco_desc_destroy(ctx); return 255; }
                    ds.write_rows(p0, cnt, rows.data());
                    printf("\rStep: %zu / %zu", p0 + cnt, n);
                    fflush(stdout);
                }
            }
            if (quant) quant_io::write(wr, qscale, qoff);
            for (uint8_t s : status) by_status[s < 3 ? s : 0]++;
            wr.write_vec<uint8_t>("Status", status.data(), n);
            if (want_patches) wr.write_3d<uint8_t>("Patches", patches.data(), n, 64, 64);
        }
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        cout << "\nDone." << endl << endl;
        printf("Keypoints: %zu inside, %zu over the border, %zu invalid\n", by_status[2], by_status[1], by_status[0]);
        printf("Total: %.09f sec\n\n", sec);
        dlco_desc_destroy(ctx);
    } catch (const std::exception &e) {
        if (ctx) dlco_desc_destroy(ctx);
        std::fprintf(stderr, "describe-image: %s\n", e.what());
        return 2;
    }
    return 0;
}
