// tracks — the keypoints of many images that are one scene point, from the verified matches of many pairs in one library
// call, over libdlco.so: the step behind detect -> describe-image -> match-pairs -> verify-pairs.
//
//     tracks pairs_out -out dst [-min n] [-all] [-device n] kp_file_0 kp_file_1 ...
//
// pairs_out is what `verify-pairs` wrote: "Pairs" [P,2] i32 of (query file, train file), "VerifiedOffsets" [P+1] i64 and
// "VerifiedMatches" [K,2] i32 = (query, train) as rows of the pair's own two tables.  Where those two are absent it is what
// `match-pairs` wrote: "Pairs", "MatchOffsets" and "Matches", every match counting.  The kp_files hold "Keypoints" [n,4] f32
// as `detect` writes them, in match-pairs' file order; their row counts are the images of ONE dlco_desc_build_tracks call
// (csrc/track_rules.hpp states the rule): a node is a keypoint, a match joins two, a track is a connected component of at
// least -min nodes (default 2) without two keypoints of one image; -all keeps the components that have two (unique = 0).
// Writes
//     "TrackOffsets" [T+1] i64: track t owns the entries TrackOffsets[t] .. TrackOffsets[t+1] - 1 of
//     "TrackImage" [K] i32, "TrackKeypoint" [K] i32   the file and the row of "Keypoints" in it; tracks ascend in their first
//                                                     keypoint, images ascend inside a track
//     "TrackXY" [K,2] f32                 the (x, y) of that keypoint
//     "TrackOf" [N] i32                   for the keypoints of all files one after another: the track, or -1
//     "Counts" [3] i64                    components of at least 2 keypoints, those below -min, those dropped for a conflict
// and prints one summary line.  An index of the matches outside its keypoint table is an error before a device is opened.
// A path that does not end in .h5/.hdf5 is a directory of .npy files with the same dataset names (dlco_io.hpp).
#include "../../include/dlco.h"
#include "dlco_io.hpp"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <iostream>

using std::cout;
using std::endl;

int main(int argc, char **argv)
{
    int device = 0;
    long long min_len = 2;
    bool help = false, all = false;
    const char *mf = nullptr, *out = nullptr;
    std::vector<const char *> files;
    for (int i = 1; i < argc; i++) {
        if (argv[i][0] == '-') {
            const bool has_val = i + 1 < argc;
            if (std::strcmp(argv[i], "-help") == 0) { help = true; continue; }
            if (std::strcmp(argv[i], "-out") == 0 && has_val) { out = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-min") == 0 && has_val) { min_len = atoll(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-all") == 0) { all = true; continue; }
            if (std::strcmp(argv[i], "-device") == 0 && has_val) { device = atoi(argv[++i]); continue; }
            cout << "ERROR: Invalid " << argv[i] << " option." << endl;
            help = true;
        } else {
            if (!mf) { mf = argv[i]; continue; }
            files.push_back(argv[i]);
        }
    }
    if (!mf || !out || files.empty()) help = true;
    if (min_len < 2 || min_len > 2147483647LL) { cout << "ERROR: -min must be at least 2." << endl; help = true; }
    if (help) {
        cout << endl;
        cout << "Usage: tracks pairs_out -out dst_h5_filename [-min n] [-all] [-device n] kp_file_0 kp_file_1 ..." << endl;
        cout << endl;
        return 1;
    }
    dlco_desc_ctx *ctx = nullptr;
    try {
        const size_t n_img = files.size();
        std::vector<std::vector<float>> kp(n_img);
        std::vector<int64_t> seg(n_img + 1, 0);
        for (size_t f = 0; f < n_img; f++) {
            std::vector<size_t> shape;
            dlco_io::read_dataset<float>(files[f], "Keypoints", shape, kp[f]);
            if (shape.size() != 2 || shape[1] != 4) throw std::runtime_error(std::string(files[f]) + ": Keypoints must be an [n, 4] table");
            seg[f + 1] = seg[f] + (int64_t)shape[0];
        }
        const bool verified = dlco_io::has_dataset(mf, "VerifiedOffsets") && dlco_io::has_dataset(mf, "VerifiedMatches");
        const char *off_name = verified ? "VerifiedOffsets" : "MatchOffsets", *list_name = verified ? "VerifiedMatches" : "Matches";
        std::vector<size_t> ps, os, ms;
        std::vector<int32_t> pairs, M;
        std::vector<int64_t> moff;
        dlco_io::read_dataset<int32_t>(mf, "Pairs", ps, pairs);
        dlco_io::read_dataset<int64_t>(mf, off_name, os, moff);
        dlco_io::read_dataset<int32_t>(mf, list_name, ms, M);
        if (ps.size() != 2 || ps[0] < 1 || ps[1] != 2) throw std::runtime_error(std::string(mf) + ": Pairs must be a non-empty [P, 2] table");
        const size_t P = ps[0];
        if (ms.size() != 2 || ms[1] != 2) throw std::runtime_error(std::string(mf) + ": " + list_name + " must be an [M, 2] table");
        const size_t m_all = ms[0];
        if (os.size() != 1 || os[0] != P + 1 || moff[0] != 0 || moff[P] != (int64_t)m_all)
            throw std::runtime_error(std::string(mf) + ": " + off_name + " must be [P + 1], from 0 to the rows of " + list_name);
        for (size_t p = 0; p < P; p++)
            if (moff[p + 1] < moff[p]) throw std::runtime_error(std::string(mf) + ": " + off_name + " decreases at pair " + std::to_string(p));
        for (size_t i = 0; i < 2 * P; i++)
            if (pairs[i] < 0 || (size_t)pairs[i] >= n_img)
                throw std::runtime_error(std::string(mf) + ": pair " + std::to_string(i / 2) + " names file " + std::to_string(pairs[i]) + " of " +
                                         std::to_string(n_img));
        for (size_t p = 0; p < P; p++) {
            const size_t a = (size_t)pairs[2 * p], b = (size_t)pairs[2 * p + 1];
            const int64_t na = seg[a + 1] - seg[a], nb = seg[b + 1] - seg[b];
            for (size_t i = (size_t)moff[p]; i < (size_t)moff[p + 1]; i++) {
                const int32_t q = M[2 * i], t = M[2 * i + 1];
                if (q < 0 || q >= na || t < 0 || t >= nb)
                    throw std::runtime_error("pair " + std::to_string(p) + ": match " + std::to_string(i - (size_t)moff[p]) + " = (" + std::to_string(q) + ", " +
                                             std::to_string(t) + ") is outside the keypoint tables of " + std::to_string(na) + " and " + std::to_string(nb) +
                                             " rows");
            }
        }
        const size_t N = (size_t)seg[n_img];
        printf("Pairs: %zu\n", P);
        printf("Matches: %zu (%s)\n", m_all, list_name);
        printf("Keypoints: %zu\n", N);

        const auto t0 = std::chrono::steady_clock::now();
        int64_t n_tracks = 0, counts[3] = {0, 0, 0};
        std::vector<int64_t> toff(N / 2 + 1, 0);
        std::vector<int32_t> obs(N + 1, 0), track_of(N + 1, -1);
        M.resize(M.size() + 2, 0);                         // an empty list still has an address
        if (dlco_desc_create(&ctx, 1.4f, 8, 1, device) != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(nullptr));
        if (dlco_desc_build_tracks(ctx, seg.data(), (int32_t)n_img, pairs.data(), (int64_t)P, moff.data(), M.data(), nullptr, (int32_t)min_len, all ? 0 : 1,
                                   &n_tracks, toff.data(), obs.data(), track_of.data(), nullptr, counts) != DLCO_OK)
            throw std::runtime_error(dlco_desc_last_error(ctx));
        const size_t T = (size_t)n_tracks, K = (size_t)toff[T];
        std::vector<int32_t> image(K + 1), row(K + 1);
        std::vector<float> xy(2 * K + 2);
        size_t longest = 0;
        for (size_t t = 0; t < T; t++) {
            longest = std::max(longest, (size_t)(toff[t + 1] - toff[t]));
            size_t f = 0;                                  // nodes ascend inside a track, so files do
            for (size_t k = (size_t)toff[t]; k < (size_t)toff[t + 1]; k++) {
                while (seg[f + 1] <= obs[k]) f++;
                image[k] = (int32_t)f;
                row[k] = (int32_t)(obs[k] - seg[f]);
                xy[2 * k] = kp[f][4 * (size_t)row[k]];
                xy[2 * k + 1] = kp[f][4 * (size_t)row[k] + 1];
            }
        }
        {
            dlco_io::Writer wr(out);
            wr.write_vec<int64_t>("TrackOffsets", toff.data(), T + 1);
            wr.write_vec<int32_t>("TrackImage", image.data(), K);
            wr.write_vec<int32_t>("TrackKeypoint", row.data(), K);
            wr.write<float>("TrackXY", xy.data(), K, 2);
            wr.write_vec<int32_t>("TrackOf", track_of.data(), N);
            wr.write_vec<int64_t>("Counts", counts, 3);
        }
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("Tracks: %zu of %zu observations, longest %zu; components %lld, below -min %lld, conflicting %lld\n", T, K, longest, (long long)counts[0],
               (long long)counts[1], (long long)counts[2]);
        printf("Kernels: %.6f ms\n", dlco_desc_last_kernel_ms(ctx));
        printf("Total: %.09f sec\n", sec);
        dlco_desc_destroy(ctx);
    } catch (const std::exception &e) {
        if (ctx) dlco_desc_destroy(ctx);
        std::fprintf(stderr, "tracks: %s\n", e.what());
        return 2;
    }
    return 0;
}
