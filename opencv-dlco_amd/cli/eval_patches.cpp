// eval-patches — FPR@95 / AUC of a trained descriptor on a raw patch-pair set, over libdlco.so.
//
//     eval-patches src_h5_filter_file src_h5_img_file -prj src_h5_prj_file -id rowid -pj pj_model [-device n]
//
// eval-fpr95 scores pj-learn's W on the "-unproj" file of a set: the N x nsel*8 matrix comp-uprjdists writes.  This
// tool takes that set's "Indices" [pairs,4] and "Patches" [n,64,64] instead, describes every patch once with
//     y = W * min(sPRFilters * get_desc(patch), 1)
// and runs ComputePJStats (src/misc.cpp:266-333) on ||y_a - y_b||^2: no N x F matrix on disk, on the host or in HBM.
// Prints the reference's "Stat:" line (src/misc.cpp:326-330), as eval-fpr95 does.
#include "desc_model.hpp"

#include <cstdlib>
#include <cstring>

using std::cout;
using std::endl;

int main(int argc, char **argv)
{
    int widx = 0, device = 0;
    bool help = false;
    const char *flt = nullptr, *img = nullptr, *prj = nullptr, *pj = nullptr;
    for (int i = 1; i < argc; i++) {
        if (argv[i][0] == '-') {
            const bool has_val = i + 1 < argc;
            if (std::strcmp(argv[i], "-help") == 0) { help = true; continue; }
            if (std::strcmp(argv[i], "-prj") == 0 && has_val) { prj = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-id") == 0 && has_val) { widx = atoi(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-pj") == 0 && has_val) { pj = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-device") == 0 && has_val) { device = atoi(argv[++i]); continue; }
            cout << "ERROR: Invalid " << argv[i] << " option." << endl;
            help = true;
        } else {
            if (!flt) { flt = argv[i]; continue; }
            if (!img) { img = argv[i]; continue; }
            help = true;
        }
    }
    if (!flt || !img || !prj || !pj) help = true;
    if (help) {
        cout << endl;
        cout << "Usage: eval-patches src_h5_filter_file src_h5_img_file" << endl;
        cout << "        -prj src_h5_prj_file -id src_h5_prj_matrix_rowid -pj src_h5_pj_file [-device n]" << endl;
        cout << endl;
        return 1;
    }
    try {
        desc_model::PRFilters filters;
        std::vector<size_t> ishape, pshape, wshape;
        std::vector<int32_t> pairs;
        std::vector<uint8_t> patches;
        std::vector<float> sPR, W;
        int32_t nsel = 0;
        desc_model::load_pr_filters(flt, filters);
        printf("ImageSet: [%s]\n", img);
        cout << "Load Indices." << endl;
        dlco_io::read_dataset<int32_t>(img, "Indices", ishape, pairs);
        if (ishape.size() != 2 || ishape[1] != 4) throw std::runtime_error("Indices must be [pairs,4]");
        desc_model::load_patches(img, pshape, patches);
        desc_model::select(filters, prj, widx, sPR, nsel);
        desc_model::load_projection(pj, nsel, wshape, W);
        if (ishape[0] < 1 || pshape[0] < 1) throw std::runtime_error("Indices or Patches is empty");

        dlco_desc_ctx *ctx = desc_model::open_ctx(sPR, nsel, device);
        if (dlco_desc_set_projection(ctx, W.data(), (int32_t)wshape[0], (int32_t)wshape[1]) != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(ctx));
        int32_t dim = 0;
        float fpr95 = 0.f;
        double auc = 0.0;
        if (dlco_desc_pair_stats(ctx, patches.data(), (int64_t)pshape[0], pairs.data(), (int64_t)ishape[0], &dim, &fpr95, &auc) != DLCO_OK)
            throw std::runtime_error(dlco_desc_last_error(ctx));
        std::printf("Stat: Dim [%i] AUC: %.6f (%.6f) FPR95: %.2f (%.2f)\n", dim, auc, auc, fpr95 * 100, fpr95 * 100);
        dlco_desc_destroy(ctx);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "eval-patches: %s\n", e.what());
        return 2;
    }
    return 0;
}
