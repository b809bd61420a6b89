// describe — the learnt descriptor of every patch of a set, over libdlco.so.
//
//     describe src_h5_filter_file src_h5_img_file -prj src_h5_prj_file -id rowid -pj pj_model -out dst [-quant quant_file] [-device n]
//
// The first four inputs are comp-uprjdists' ("PRFilters", "Patches", row `rowid` of pr-learn's "w"); -pj is pj-learn's
// output, the file eval-fpr95 takes as its W (dataset "W" [r, nsel*8]).  Writes "Descriptor" [n_patches, r] f32 with
//     y = W * min(sPRFilters * get_desc(patch), 1)
// per row, a chunk of patches at a time.  The reference has no such tool: a user of its trained model goes through
// OpenCV's re-encoding of the exported files.  "Indices" is not needed.  A path that does not end in .h5/.hdf5 is a
// directory of .npy files with the same dataset names (dlco_io.hpp).
//   With -quant quant_file ("QuantScale", "QuantOffset": an output of `quantize`) the rows are quantised on the device
// (dlco_desc_describe_u8) and the output holds "DescriptorU8" [n_patches, r] u8 and the two quantiser datasets in place of
// "Descriptor": what `match -u8` reads.
#include "desc_model.hpp"
#include "quant_io.hpp"

#include <chrono>
#include <cstdlib>
#include <cstring>

using std::cout;
using std::endl;

int main(int argc, char **argv)
{
    int widx = 0, device = 0;
    bool help = false;
    const char *flt = nullptr, *img = nullptr, *prj = nullptr, *pj = nullptr, *out = nullptr, *quant = nullptr;
    const size_t sChunk = 2048;                             // patches per library call: host memory holds one chunk of rows
    for (int i = 1; i < argc; i++) {
        if (argv[i][0] == '-') {
            const bool has_val = i + 1 < argc;
            if (std::strcmp(argv[i], "-help") == 0) { help = true; continue; }
            if (std::strcmp(argv[i], "-prj") == 0 && has_val) { prj = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-id") == 0 && has_val) { widx = atoi(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-pj") == 0 && has_val) { pj = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-out") == 0 && has_val) { out = argv[++i]; continue; }
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
    if (help) {
        cout << endl;
        cout << "Usage: describe src_h5_filter_file src_h5_img_file" << endl;
        cout << "        -prj src_h5_prj_file -id src_h5_prj_matrix_rowid -pj src_h5_pj_file -out dst_h5_filename [-quant quant_file] [-device n]" << endl;
        cout << endl;
        return 1;
    }
    try {
        desc_model::PRFilters filters;
        std::vector<size_t> pshape, wshape;
        std::vector<uint8_t> patches;
        std::vector<float> sPR, W;
        int32_t nsel = 0;
        desc_model::load_pr_filters(flt, filters);
        printf("ImageSet: [%s]\n", img);
        desc_model::load_patches(img, pshape, patches);
        desc_model::select(filters, prj, widx, sPR, nsel);
        desc_model::load_projection(pj, nsel, wshape, W);
        const size_t n = pshape[0], r = wshape[0];
        if (n < 1) throw std::runtime_error("Patches is empty");
        float qscale = 0.f;
        std::vector<float> qoff;
        if (quant) quant_io::read(quant, r, qscale, qoff);

        dlco_desc_ctx *ctx = desc_model::open_ctx(sPR, nsel, device);
        if (dlco_desc_set_projection(ctx, W.data(), (int32_t)r, (int32_t)wshape[1]) != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(ctx));
        if (quant && dlco_desc_set_quantizer(ctx, qscale, qoff.data(), (int32_t)r) != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(ctx));
        cout << "Start Compute Descriptors: #" << n << endl;
        const auto t0 = std::chrono::steady_clock::now();
        if (quant) {
            dlco_io::Writer wr(out);
            {
                dlco_io::RowStream<uint8_t> ds(wr, "DescriptorU8", n, r, 128, r, 0);
                std::vector<uint8_t> rows(std::min(sChunk, n) * r);
                for (size_t p0 = 0; p0 < n; p0 += sChunk) {
                    const size_t cnt = std::min(sChunk, n - p0);
                    if (dlco_desc_describe_u8(ctx, patches.data() + p0 * 4096, (int64_t)cnt, rows.data()) != DLCO_OK)
                        throw std::runtime_error(dlco_desc_last_error(ctx));
                    ds.write_rows(p0, cnt, rows.data());
                    printf("\rStep: %zu / %zu", p0 + cnt, n);
                    fflush(stdout);
                }
            }
            quant_io::write(wr, qscale, qoff);
        } else {
            dlco_io::Writer wr(out);
            dlco_io::RowStream<float> ds(wr, "Descriptor", n, r, 128, r, 0);
            std::vector<float> rows(std::min(sChunk, n) * r);
            for (size_t p0 = 0; p0 < n; p0 += sChunk) {
                const size_t cnt = std::min(sChunk, n - p0);
                if (dlco_desc_describe(ctx, patches.data() + p0 * 4096, (int64_t)cnt, rows.data()) != DLCO_OK)
                    throw std::runtime_error(dlco_desc_last_error(ctx));
                for (size_t i = 0; i < cnt * r; i++)
                    if (!(rows[i] == rows[i]) || rows[i] > 3.0e38f || rows[i] < -3.0e38f) { cout << "\nDescriptor contains NaN\n"; return 255; }
                ds.write_rows(p0, cnt, rows.data());
                printf("\rStep: %zu / %zu", p0 + cnt, n);
                fflush(stdout);
            }
        }
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        cout << "\nDone." << endl << endl;
        printf("Total: %.09f sec\n\n", sec);
        dlco_desc_destroy(ctx);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "describe: %s\n", e.what());
        return 2;
    }
    return 0;
}
