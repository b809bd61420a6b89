// pr-learn-grid — pr-learn for a grid of (mu, gamma) settings in one run:
//
//     pr-learn-grid src_h5_filter_file src_h5_dist_file dst_dir -mus a,b,... -gammas x,y,...
//                   [-name tag] [-npy] [-maxdim n] [-iters n] [-logstep n] [-seed n] [-device n]
//
// The reference runs pr-learn once per data set and (mu, gamma) pair and keeps one log per run
// (workspace/pr-learn/logging/<tag>-<mu>-<gamma>-pr.log).  This tool trains the Cartesian product of the
// two lists together (dlco_pr_grid_*: the settings share every sampled row pair) and writes, per setting,
// dst_dir/<tag>-<mu %.3f>-<gamma %.3f>-pr.log with exactly the stdout pr-learn prints for that setting
// (Ttime / Vtime are the grid's shared window times) and the output dst_dir/<tag>-<mu>-<gamma>-pr.h5
// ("w" rows appended as pr-learn appends them), or with -npy the .npy directory <...>-pr.
// Defaults are pr-learn's (mu 0.025, gamma 0.10, maxdim 640, 5 000 000 iterations, LogStep 100 000,
// seed 2215); -name defaults to the file name of src_h5_dist_file without its extension.
#include "../../include/dlco.h"
#include "pr_cli.hpp"
#include "pr_logstep.hpp"

#include <iostream>
#include <set>
#include <sstream>

using std::cout;
using std::endl;

static bool parse_list(const char *s, std::vector<float> &out)
{
    out.clear();
    std::stringstream ss(s);
    std::string item;
    while (std::getline(ss, item, ',')) {
        if (item.empty()) return false;
        char *end = nullptr;
        const float v = (float)std::strtod(item.c_str(), &end);     // as pr-learn's (float)atof
        if (*end != '\0') return false;
        out.push_back(v);
    }
    return !out.empty();
}

static void append_text(const std::string &path, const std::string &text)
{
    FILE *f = std::fopen(path.c_str(), "a");
    if (!f) throw std::runtime_error("cannot open " + path + " for writing");
    const bool ok = std::fwrite(text.data(), 1, text.size(), f) == text.size();
    if (std::fclose(f) != 0 || !ok) throw std::runtime_error("cannot write " + path);
}

int main(int argc, char **argv)
{
    std::vector<float> mus{0.025f}, gammas{0.10f};          // pr-learn's defaults, src/pr-learn.cpp:78-79
    pr_cli::CommonFlags f;
    bool help = false, npy = false;
    std::string tag;
    const char *flt = nullptr, *src = nullptr, *dst = nullptr;

    for (int i = 1; i < argc; i++) {
        if (argv[i][0] == '-') {
            const bool has_val = i + 1 < argc;
            if (std::strcmp(argv[i], "-help") == 0) { help = true; continue; }
            if (std::strcmp(argv[i], "-npy") == 0) { npy = true; continue; }
            if (std::strcmp(argv[i], "-mus") == 0 && has_val) {
                if (!parse_list(argv[++i], mus)) { cout << "ERROR: Invalid -mus list." << endl; help = true; }
                continue;
            }
            if (std::strcmp(argv[i], "-gammas") == 0 && has_val) {
                if (!parse_list(argv[++i], gammas)) { cout << "ERROR: Invalid -gammas list." << endl; help = true; }
                continue;
            }
            if (std::strcmp(argv[i], "-name") == 0 && has_val) { tag = argv[++i]; continue; }
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

    // the settings (mu-major) and their file names
    struct Setting { float mu, gamma; std::string log, out; pr_log::Best best; std::string text; };
    std::vector<Setting> set;
    if (!help) {
        if (tag.empty()) {
            std::string b = src;
            while (b.size() > 1 && b.back() == '/') b.pop_back();
            b = b.substr(b.find_last_of('/') == std::string::npos ? 0 : b.find_last_of('/') + 1);
            const size_t dot = b.find_last_of('.');
            tag = dot == std::string::npos || dot == 0 ? b : b.substr(0, dot);
        }
        std::set<std::string> names;
        for (float m : mus)
            for (float g : gammas) {
                char stem[64];
                std::snprintf(stem, sizeof(stem), "-%.3f-%.3f-pr", m, g);
                const std::string base = std::string(dst) + "/" + tag + stem;
                if (!names.insert(base).second) {
                    cout << "ERROR: settings mu " << m << " gamma " << g << " repeat the file name " << base << ".log" << endl;
                    help = true;
                }
                set.push_back(Setting{m, g, base + ".log", npy ? base : base + ".h5", pr_log::Best(), std::string()});
            }
    }
    if (help) {
        cout << endl;
        cout << "Usage: pr-learn-grid  src_h5_filter_file" << endl;
        cout << "       src_h5_dist_file dst_dir" << endl;
        cout << "       -mus <a,b,... 0.0-1.0, 0.025=default> " << endl;
        cout << "       -gammas <x,y,... 0.0-10.0, 0.10=default> " << endl;
        cout << "       -name <tag of the file names, name of src_h5_dist_file=default> " << endl;
        cout << "       -npy <write .npy directories instead of .h5 files> " << endl;
        cout << "       -maxdim <64-768, 640=default> " << endl;
        cout << "       -iters <0-N, 5000000=default> " << endl;
        cout << endl;
        return 1;
    }
    const int G = (int)set.size();
    cout << "Grid: " << mus.size() << " mu x " << gammas.size() << " gamma = " << G << " settings, maxdim: " << f.MaxDim << " nIters: " << f.nIter
         << endl;

    try {
        mkdir(dst, 0777);
        pr_cli::Inputs in = pr_cli::load(flt, src, nullptr);
        const int nDists = in.nDists, FeatDim = in.FeatDim;

        dlco_pr_ctx *ctx = nullptr;
        if (dlco_pr_create(&ctx, FeatDim, nDists, set[0].mu, set[0].gamma, f.seed, f.device) != DLCO_OK) throw std::runtime_error(dlco_pr_last_error(nullptr));
        if (dlco_pr_set_data(ctx, in.dists.data(), in.labels.data()) != DLCO_OK) throw std::runtime_error(dlco_pr_last_error(ctx));
        in.dists.clear(); in.dists.shrink_to_fit();
        std::vector<float> mu(G), gamma(G);
        for (int k = 0; k < G; k++) { mu[k] = set[k].mu; gamma[k] = set[k].gamma; }
        dlco_pr_grid *grid = nullptr;
        if (dlco_pr_grid_create(&grid, ctx, G, mu.data(), gamma.data(), f.seed) != DLCO_OK) throw std::runtime_error(dlco_pr_grid_last_error(nullptr));
        int32_t n_pos = 0, n_pos_trn = 0, n_neg = 0, n_neg_trn = 0;
        dlco_pr_get_index(ctx, &n_pos, &n_pos_trn, &n_neg, &n_neg_trn);
        char name[256];
        int cc_major = 0, cc_minor = 0;
        dlco_pr_device_name(ctx, name, sizeof(name), &cc_major, &cc_minor);

        // each log opens with the lines pr-learn prints before its first LogStep (src/pr-learn.cpp:200-262)
        std::string progress;
        int tick = -1;
        for (int i = 0; i < nDists; i += 128) tick = dlco_io::term_progress((double)i / (double)nDists, tick, &progress);
        dlco_io::term_progress(1.0, tick, &progress);
        for (Setting &s : set) {
            std::ostringstream o;
            pr_log::config(o, s.mu, s.gamma, f.MaxDim, f.nIter);
            o << "Load PRParams." << endl;
            o << "Load RingParams." << endl;
            pr_log::loaded(o, nDists, FeatDim);
            o << progress;
            pr_log::split(o, n_pos, n_pos_trn, n_neg, n_neg_trn, name, cc_major, cc_minor);
            std::FILE *f = std::fopen(s.log.c_str(), "w");
            if (!f) throw std::runtime_error("cannot create " + s.log);
            std::fclose(f);
            append_text(s.log, o.str());
        }

        // the LogStep schedule of pr-learn: lines at t = LogStep, 2 LogStep, ... <= nIter
        std::vector<float> w((size_t)G * FeatDim), loss(G), regul(G);
        std::vector<int32_t> nnz(G);
        pr_cli::logstep_schedule(
            f.nIter, f.LogStep,
            [&](unsigned n) {
                if (dlco_pr_grid_steps(grid, n) != DLCO_OK) throw std::runtime_error(dlco_pr_grid_last_error(grid));
            },
            [&](unsigned t, pr_cli::Clock::time_point train_start) {
                uint32_t tt = 0;
                dlco_pr_grid_get_state(grid, &tt, w.data(), nullptr);   // also synchronises
                const double ttime = pr_cli::seconds_since(train_start);
                const auto v0 = pr_cli::Clock::now();
                if (dlco_pr_grid_validate(grid, loss.data(), regul.data(), nnz.data()) != DLCO_OK)
                    throw std::runtime_error(dlco_pr_grid_last_error(grid));
                const double vtime = pr_cli::seconds_since(v0);
                std::vector<int32_t> bests;
                for (int k = 0; k < G; k++) {
                    Setting &s = set[k];
                    if (pr_log::objective(s.text, s.best, t, loss[k], regul[k], nnz[k], w.data() + (size_t)k * FeatDim, (size_t)FeatDim, ttime, vtime))
                        bests.push_back(k);
                }
                if (!bests.empty()) {                                   // ComputePRStats of every new best in one call
                    const int nb = (int)bests.size();
                    std::vector<int32_t> nPR(nb), Dim(nb), nzDim(nb);
                    std::vector<float> FPR95(nb, -1.f);
                    std::vector<double> AUC(nb, 0.0);
                    if (dlco_pr_grid_stats(grid, bests.data(), nb, nullptr, in.PRParams.data(), (int32_t)in.pshape[0], (int32_t)in.pshape[1], 8, -1,
                                           nPR.data(), Dim.data(), nzDim.data(), FPR95.data(), AUC.data()) != DLCO_OK)
                        throw std::runtime_error(dlco_pr_grid_last_error(grid));
                    for (int i = 0; i < nb; i++) {
                        Setting &s = set[bests[i]];
                        const bool saved = pr_log::saves(Dim[i], f.MaxDim);
                        if (saved) dlco_io::append_row_f32(s.out, "w", s.best.w_Best.data(), (size_t)FeatDim);
                        pr_log::stat(s.text, nPR[i], nzDim[i], Dim[i], f.MaxDim, AUC[i], FPR95[i], saved);
                    }
                }
                for (Setting &s : set) { append_text(s.log, s.text); s.text.clear(); }
                std::printf("Grid: %u  Best: %i of %i  Ttime: %.4f Vtime: %.4f\n", t, (int)bests.size(), G, ttime, vtime);
                cout << std::flush;
            });
        dlco_pr_grid_destroy(grid);
        dlco_pr_destroy(ctx);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "pr-learn-grid: %s\n", e.what());
        return 2;
    }
    return 0;
}
