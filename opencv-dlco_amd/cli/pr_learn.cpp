// pr-learn — command-line front end of the pooling-region stage with the reference's interface:
//
//     pr-learn src_h5_filter_file src_h5_dist_file dst_h5_output_file [-mu f] [-gamma f] [-maxdim n] [-iters n] [-help]
//
// Same flags, defaults, usage text, exit codes and stdout grammar as the reference's main()
// (src/pr-learn.cpp:78-176,200-262,282-287,366-403; the logs are scraped by workspace/05-prstats.sh).
// All compute is behind the dlco_pr_* block of include/dlco.h; this file parses, loads, prints and
// appends the saved weight vectors to the "w" dataset of the output file (:385-400).  Extra flags
// (defaults = the reference's constants): -logstep n, -seed n, -device n.
#include "../../include/dlco.h"
#include "pr_cli.hpp"
#include "pr_logstep.hpp"

#include <iostream>

using std::cout;
using std::endl;

int main(int argc, char **argv)
{
    float mu = 0.025f, gamma = 0.10f;                        // src/pr-learn.cpp:78-79
    pr_cli::CommonFlags f;
    bool help = false;
    const char *flt = nullptr, *src = nullptr, *dst = nullptr;

    for (int i = 1; i < argc; i++) {
        if (argv[i][0] == '-') {
            const bool has_val = i + 1 < argc;
            if (std::strcmp(argv[i], "-help") == 0) { help = true; continue; }
            if (std::strcmp(argv[i], "-mu") == 0 && has_val) { mu = (float)atof(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-gamma") == 0 && has_val) { gamma = (float)atof(argv[++i]); continue; }
            if (f.parse(argc, argv, i)) continue;
            cout << "ERROR: Invalid " << argv[i] << " option." << endl;
            help = true;
        } else {
            if (!flt) { flt = argv[i]; continue; }
            if (!src) { src = argv[i]; continue; }
            if (!dst) { dst = argv[i]; continue; }
        }
    }
    if (!flt || !src || !dst) help = true;
    if (f.LogStep < 1) { cout << "ERROR: -logstep must be at least 1." << endl; help = true; }
    if (help) {
        cout << endl;
        cout << "Usage: pr-learn  src_h5_filter_file" << endl;
        cout << "       src_h5_dist_file dst_h5_output_file" << endl;
        cout << "       -mu <0.0-1.0, 0.025=default> " << endl;
        cout << "       -gamma <0.0-10.0, 0.10=default> " << endl;
        cout << "       -maxdim <64-768, 640=default> " << endl;
        cout << "       -iters <0-N, 5000000=default> " << endl;
        cout << endl;
        return 1;
    }
    pr_log::config(cout, mu, gamma, f.MaxDim, f.nIter);

    try {
        pr_cli::Inputs in = pr_cli::load(flt, src, &cout);
        const int nDists = in.nDists, FeatDim = in.FeatDim;
        pr_log::loaded(cout, nDists, FeatDim);
        int tick = -1;
        for (int i = 0; i < nDists; i += 128) tick = dlco_io::term_progress((double)i / (double)nDists, tick);
        dlco_io::term_progress(1.0, tick);

        dlco_pr_ctx *ctx = nullptr;
        if (dlco_pr_create(&ctx, FeatDim, nDists, mu, gamma, f.seed, f.device) != DLCO_OK) throw std::runtime_error(dlco_pr_last_error(nullptr));
        if (dlco_pr_set_data(ctx, in.dists.data(), in.labels.data()) != DLCO_OK) throw std::runtime_error(dlco_pr_last_error(ctx));
        in.dists.clear(); in.dists.shrink_to_fit();
        int32_t n_pos = 0, n_pos_trn = 0, n_neg = 0, n_neg_trn = 0;
        dlco_pr_get_index(ctx, &n_pos, &n_pos_trn, &n_neg, &n_neg_trn);
        char name[256];
        int cc_major = 0, cc_minor = 0;
        dlco_pr_device_name(ctx, name, sizeof(name), &cc_major, &cc_minor);
        pr_log::split(cout, n_pos, n_pos_trn, n_neg, n_neg_trn, name, cc_major, cc_minor);

        pr_log::Best best;
        std::vector<float> w(FeatDim);
        pr_cli::logstep_schedule(
            f.nIter, f.LogStep,
            [&](unsigned n) {
                if (dlco_pr_steps(ctx, n) != DLCO_OK) throw std::runtime_error(dlco_pr_last_error(ctx));
            },
            [&](unsigned t, pr_cli::Clock::time_point train_start) {
                uint32_t tt = 0;
                dlco_pr_get_state(ctx, &tt, w.data(), nullptr);    // also synchronises
                const double ttime = pr_cli::seconds_since(train_start);
                const auto v0 = pr_cli::Clock::now();
                float LossVal = 0.f, Regul = 0.f;
                int32_t nnz = 0;
                if (dlco_pr_validate(ctx, &LossVal, &Regul, &nnz) != DLCO_OK) throw std::runtime_error(dlco_pr_last_error(ctx));
                const double vtime = pr_cli::seconds_since(v0);
                std::string line;
                const bool is_best = pr_log::objective(line, best, t, LossVal, Regul, nnz, w.data(), (size_t)FeatDim, ttime, vtime);   // :364
                std::fputs(line.c_str(), stdout);
                if (is_best) {
                    int32_t nPR = 0, Dim = 0, nzDim = 0;
                    float FPR95 = -1.f;
                    double AUC = 0.0;
                    if (dlco_pr_stats(ctx, w.data(), in.PRParams.data(), (int32_t)in.pshape[0], (int32_t)in.pshape[1], 8, -1, &nPR, &Dim, &nzDim,
                                      &FPR95, &AUC) != DLCO_OK)
                        throw std::runtime_error(dlco_pr_last_error(ctx));
                    const bool saved = pr_log::saves(Dim, f.MaxDim);
                    if (saved) dlco_io::append_row_f32(dst, "w", best.w_Best.data(), (size_t)FeatDim);   // :385-400
                    line.clear();
                    pr_log::stat(line, nPR, nzDim, Dim, f.MaxDim, AUC, FPR95, saved);
                    std::fputs(line.c_str(), stdout);
                }
                cout << std::flush;
            });
        dlco_pr_destroy(ctx);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "pr-learn: %s\n", e.what());
        return 2;
    }
    return 0;
}
