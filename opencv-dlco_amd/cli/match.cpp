// match — nearest-neighbour matching of two descriptor tables, over libdlco.so.
//
//     match query_desc_file train_desc_file -out dst [-ratio f] [-cross] [-device n]
//
// Both inputs hold the dataset "Descriptor" [n, r] f32 that `describe` writes (the two r must agree).  Writes
//     "Nearest" [nq,2] i32 and "NearestSqDist" [nq,2] f32   the library's answer for every query (dlco_desc_match)
//     "Matches" [m,2] i32 = (query, train), ascending in query, and "MatchSqDist" [m] f32   the filtered list
// The filters are host rules (match_rules.hpp): -ratio f (0 < f <= 1) is Lowe's test d1 < f^2 d2 on the squared
// distances, -cross keeps (i, j) iff the nearest query of train row j is i (a second library call with the tables
// swapped).  Both may be given; without either every query with a neighbour is a match.  The reference has no such tool.
// A path that does not end in .h5/.hdf5 is a directory of .npy files with the same dataset names (dlco_io.hpp).
#include "../../include/dlco.h"
#include "dlco_io.hpp"
#include "match_rules.hpp"

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <iostream>

using std::cout;
using std::endl;

namespace {
void load_table(const char *path, std::vector<size_t> &shape, std::vector<float> &rows)
{
    dlco_io::read_dataset<float>(path, "Descriptor", shape, rows);
    if (shape.size() != 2 || shape[0] < 1 || shape[1] < 1) throw std::runtime_error(std::string(path) + ": Descriptor must be a non-empty [n, r] table");
    for (float v : rows)
        if (!(v == v) || v > 3.0e38f || v < -3.0e38f) throw std::runtime_error(std::string(path) + ": Descriptor contains NaN");
}
}  // namespace

int main(int argc, char **argv)
{
    int device = 0;
    bool help = false, cross = false, use_ratio = false;
    float ratio = 1.0f;
    const char *qf = nullptr, *tf = nullptr, *out = nullptr;
    for (int i = 1; i < argc; i++) {
        if (argv[i][0] == '-') {
            const bool has_val = i + 1 < argc;
            if (std::strcmp(argv[i], "-help") == 0) { help = true; continue; }
            if (std::strcmp(argv[i], "-out") == 0 && has_val) { out = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-ratio") == 0 && has_val) { ratio = (float)atof(argv[++i]); use_ratio = true; continue; }
            if (std::strcmp(argv[i], "-cross") == 0) { cross = true; continue; }
            if (std::strcmp(argv[i], "-device") == 0 && has_val) { device = atoi(argv[++i]); continue; }
            cout << "ERROR: Invalid " << argv[i] << " option." << endl;
            help = true;
        } else {
            if (!qf) { qf = argv[i]; continue; }
            if (!tf) { tf = argv[i]; continue; }
            help = true;
        }
    }
    if (!qf || !tf || !out) help = true;
    if (use_ratio && !(ratio > 0.0f && ratio <= 1.0f)) {
        cout << "ERROR: -ratio must be in (0, 1]." << endl;
        help = true;
    }
    if (help) {
        cout << endl;
        cout << "Usage: match query_desc_file train_desc_file -out dst_h5_filename [-ratio f] [-cross] [-device n]" << endl;
        cout << endl;
        return 1;
    }
    dlco_desc_ctx *ctx = nullptr;
    try {
        std::vector<size_t> qs, ts;
        std::vector<float> Q, T;
        load_table(qf, qs, Q);
        load_table(tf, ts, T);
        if (qs[1] != ts[1])
            throw std::runtime_error("the descriptors differ in size: " + std::to_string(qs[1]) + " (query) against " + std::to_string(ts[1]) + " (train)");
        const size_t nq = qs[0], nt = ts[0], r = qs[1];
        printf("Queries: %zu x %zu\n", nq, r);
        printf("Train: %zu x %zu\n", nt, r);

        if (dlco_desc_create(&ctx, 1.4f, 8, 1, device) != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(nullptr));
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<int32_t> nearest(nq * 2), back;
        std::vector<float> sqdist(nq * 2);
        if (dlco_desc_match(ctx, Q.data(), (int64_t)nq, T.data(), (int64_t)nt, (int32_t)r, nearest.data(), sqdist.data()) != DLCO_OK)
            throw std::runtime_error(dlco_desc_last_error(ctx));
        if (cross) {
            back.resize(nt * 2);
            std::vector<float> back_d(nt * 2);
            if (dlco_desc_match(ctx, T.data(), (int64_t)nt, Q.data(), (int64_t)nq, (int32_t)r, back.data(), back_d.data()) != DLCO_OK)
                throw std::runtime_error(dlco_desc_last_error(ctx));
        }
        std::vector<int32_t> pairs;
        std::vector<float> dists;
        match_rules::select((int64_t)nq, nearest.data(), sqdist.data(), use_ratio, ratio, cross ? back.data() : nullptr, pairs, dists);
        {
            dlco_io::Writer wr(out);
            wr.write<int32_t>("Nearest", nearest.data(), nq, 2);
            wr.write<float>("NearestSqDist", sqdist.data(), nq, 2);
            wr.write<int32_t>("Matches", pairs.data(), dists.size(), 2);
            wr.write_vec<float>("MatchSqDist", dists.data(), dists.size());
        }
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("Matches: %zu / %zu\n", dists.size(), nq);
        printf("Total: %.09f sec\n", sec);
        dlco_desc_destroy(ctx);
    } catch (const std::exception &e) {
        if (ctx) dlco_desc_destroy(ctx);
        std::fprintf(stderr, "match: %s\n", e.what());
        return 2;
    }
    return 0;
}
