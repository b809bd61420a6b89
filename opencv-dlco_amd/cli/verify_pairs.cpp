// verify-pairs — geometric verification of the match lists of many pairs in one library call, over libdlco.so: the end of
// detect -> describe-image -> match-pairs.
//
//     verify-pairs match_pairs_out -out dst [-thresh f] [-hyp n] [-seed n] [-refine n] [-model homography|fundamental]
//                  [-device n] kp_file_0 kp_file_1 ...
//
// match_pairs_out is what `match-pairs` wrote: "Pairs" [P,2] i32 of (query file, train file), "MatchOffsets" [P+1] i64 and
// "Matches" [M,2] i32 = (query, train) as rows of the pair's own two tables.  The kp_files hold "Keypoints" [n,4] f32 as
// `detect` writes them, in match-pairs' file order.  The (x, y) columns of the matched keypoints of all pairs go to ONE
// dlco_desc_verify_pairs_homography call (-model fundamental: dlco_desc_verify_pairs_fundamental); the options are
// `verify`'s, one setting for all pairs.  Writes
//     "Pairs" [P,2] i32 and "MatchOffsets" [P+1] i64 as read: pair p owns the entries MatchOffsets[p] .. MatchOffsets[p+1] - 1 of
//     "Inlier" [M] u8                     1 where the match agrees with its pair's model
//     "Homography" [P,3,3] f32            every pair's H rounded for reading ("Fundamental" with -model fundamental)
//     "HomographyBits" [P,9] i64          the bits of H's doubles, row-major: the exact answer ("FundamentalBits")
//     "Inliers" [P] i64, "BestHypothesis" [P] i32   -1: no model (H and the pair's Inlier are zero)
//     "VerifiedOffsets" [P+1] i64: pair p owns the rows VerifiedOffsets[p] .. VerifiedOffsets[p+1] - 1 of
//     "VerifiedMatches" [K,2] i32         the rows of "Matches" with Inlier == 1
// and prints "Pair p: k / m inliers, hypothesis h" per pair.  Every pair's datasets are what `verify` writes for its slice.
// A pair with fewer matches than a sample (4, fundamental: 8) gets the no-model result; when no pair has a sample no device
// is opened.  An index of "Matches" outside its keypoint table is an error before a device is opened.
// A path that does not end in .h5/.hdf5 is a directory of .npy files with the same dataset names (dlco_io.hpp).
#include "../../include/dlco.h"
#include "dlco_io.hpp"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>

using std::cout;
using std::endl;

int main(int argc, char **argv)
{
    int device = 0;
    long long n_hyp = 2048, refine = 2;
    unsigned long long seed = 0;
    float thresh = 3.0f;
    bool help = false, fundamental = false;
    const char *mf = nullptr, *out = nullptr;
    std::vector<const char *> files;
    for (int i = 1; i < argc; i++) {
        if (argv[i][0] == '-') {
            const bool has_val = i + 1 < argc;
            if (std::strcmp(argv[i], "-help") == 0) { help = true; continue; }
            if (std::strcmp(argv[i], "-out") == 0 && has_val) { out = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-thresh") == 0 && has_val) { thresh = (float)atof(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-hyp") == 0 && has_val) { n_hyp = atoll(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-seed") == 0 && has_val) { seed = strtoull(argv[++i], nullptr, 0); continue; }
            if (std::strcmp(argv[i], "-refine") == 0 && has_val) { refine = atoll(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-device") == 0 && has_val) { device = atoi(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-model") == 0 && has_val) {
                const char *name = argv[++i];
                if (std::strcmp(name, "fundamental") == 0) { fundamental = true; continue; }
                if (std::strcmp(name, "homography") == 0) { fundamental = false; continue; }
                cout << "ERROR: -model must be homography or fundamental." << endl;
                help = true;
                continue;
            }
            cout << "ERROR: Invalid " << argv[i] << " option." << endl;
            help = true;
        } else {
            if (!mf) { mf = argv[i]; continue; }
            files.push_back(argv[i]);
        }
    }
    if (!mf || !out || files.empty()) help = true;
    if (!(std::isfinite(thresh) && thresh > 0.0f)) { cout << "ERROR: -thresh must be positive." << endl; help = true; }
    if (n_hyp < 1 || n_hyp > 1048576) { cout << "ERROR: -hyp must be in 1 .. 1048576." << endl; help = true; }
    if (refine < 0 || refine > 8) { cout << "ERROR: -refine must be in 0 .. 8." << endl; help = true; }
    if (help) {
        cout << endl;
        cout << "Usage: verify-pairs match_pairs_out -out dst_h5_filename [-thresh f] [-hyp n] [-seed n] [-refine n] [-model homography|fundamental] "
                "[-device n] kp_file_0 kp_file_1 ..." << endl;
        cout << endl;
        return 1;
    }
    dlco_desc_ctx *ctx = nullptr;
    try {
        const size_t n_img = files.size();
        std::vector<std::vector<float>> kp(n_img);
        std::vector<size_t> kp_rows(n_img);
        for (size_t f = 0; f < n_img; f++) {
            std::vector<size_t> shape;
            dlco_io::read_dataset<float>(files[f], "Keypoints", shape, kp[f]);
            if (shape.size() != 2 || shape[1] != 4) throw std::runtime_error(std::string(files[f]) + ": Keypoints must be an [n, 4] table");
            kp_rows[f] = shape[0];
        }
        std::vector<size_t> ps, os, ms;
        std::vector<int32_t> pairs, M;
        std::vector<int64_t> moff;
        dlco_io::read_dataset<int32_t>(mf, "Pairs", ps, pairs);
        dlco_io::read_dataset<int64_t>(mf, "MatchOffsets", os, moff);
        dlco_io::read_dataset<int32_t>(mf, "Matches", ms, M);
        if (ps.size() != 2 || ps[0] < 1 || ps[1] != 2) throw std::runtime_error(std::string(mf) + ": Pairs must be a non-empty [P, 2] table");
        const size_t P = ps[0];
        if (ms.size() != 2 || ms[1] != 2) throw std::runtime_error(std::string(mf) + ": Matches must be an [M, 2] table");
        const size_t m_all = ms[0];
        if (os.size() != 1 || os[0] != P + 1 || moff[0] != 0 || moff[P] != (int64_t)m_all)
            throw std::runtime_error(std::string(mf) + ": MatchOffsets must be [P + 1], from 0 to the rows of Matches");
        for (size_t p = 0; p < P; p++)
            if (moff[p + 1] < moff[p]) throw std::runtime_error(std::string(mf) + ": MatchOffsets decreases at pair " + std::to_string(p));
        for (size_t i = 0; i < 2 * P; i++)
            if (pairs[i] < 0 || (size_t)pairs[i] >= n_img)
                throw std::runtime_error(std::string(mf) + ": pair " + std::to_string(i / 2) + " names file " + std::to_string(pairs[i]) + " of " +
                                         std::to_string(n_img));
        std::vector<float> src(m_all * 2), dst(m_all * 2);
        bool any_sample = false;
        for (size_t p = 0; p < P; p++) {
            const size_t a = (size_t)pairs[2 * p], b = (size_t)pairs[2 * p + 1];
            any_sample = any_sample || moff[p + 1] - moff[p] >= (fundamental ? 8 : 4);
            for (size_t i = (size_t)moff[p]; i < (size_t)moff[p + 1]; i++) {
                const int32_t q = M[2 * i], t = M[2 * i + 1];
                if (q < 0 || (size_t)q >= kp_rows[a] || t < 0 || (size_t)t >= kp_rows[b])
                    throw std::runtime_error("pair " + std::to_string(p) + ": match " + std::to_string(i - (size_t)moff[p]) + " = (" + std::to_string(q) + ", " +
                                             std::to_string(t) + ") is outside the keypoint tables of " + std::to_string(kp_rows[a]) + " and " +
                                             std::to_string(kp_rows[b]) + " rows");
                src[2 * i] = kp[a][4 * (size_t)q]; src[2 * i + 1] = kp[a][4 * (size_t)q + 1];
                dst[2 * i] = kp[b][4 * (size_t)t]; dst[2 * i + 1] = kp[b][4 * (size_t)t + 1];
            }
        }
        printf("Pairs: %zu\n", P);
        printf("Matches: %zu\n", m_all);

        const auto t0 = std::chrono::steady_clock::now();
        std::vector<double> H(P * 9, 0.0);
        std::vector<uint8_t> inlier(m_all, 0);
        std::vector<int64_t> k(P, 0);
        std::vector<int32_t> best(P, -1);
        if (any_sample) {
            if (dlco_desc_create(&ctx, 1.4f, 8, 1, device) != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(nullptr));
            const auto verify = fundamental ? dlco_desc_verify_pairs_fundamental : dlco_desc_verify_pairs_homography;      // one signature
            if (verify(ctx, src.data(), dst.data(), moff.data(), (int64_t)P, thresh, (int32_t)n_hyp, (uint64_t)seed, (int32_t)refine, H.data(), inlier.data(),
                       k.data(), best.data()) != DLCO_OK)
                throw std::runtime_error(dlco_desc_last_error(ctx));
        }
        std::vector<float> Hf(P * 9);
        std::vector<int64_t> bits(P * 9), voff(P + 1, 0);
        for (size_t i = 0; i < P * 9; i++) { Hf[i] = (float)H[i]; std::memcpy(&bits[i], &H[i], sizeof(double)); }
        std::vector<int32_t> kept;
        for (size_t p = 0; p < P; p++) {
            for (size_t i = (size_t)moff[p]; i < (size_t)moff[p + 1]; i++)
                if (inlier[i]) { kept.push_back(M[2 * i]); kept.push_back(M[2 * i + 1]); }
            voff[p + 1] = (int64_t)kept.size() / 2;
        }
        {
            dlco_io::Writer wr(out);
            wr.write<int32_t>("Pairs", pairs.data(), P, 2);
            wr.write_vec<int64_t>("MatchOffsets", moff.data(), P + 1);
            wr.write_3d<float>(fundamental ? "Fundamental" : "Homography", Hf.data(), P, 3, 3);
            wr.write<int64_t>(fundamental ? "FundamentalBits" : "HomographyBits", bits.data(), P, 9);
            wr.write_vec<uint8_t>("Inlier", inlier.data(), m_all);
            wr.write_vec<int64_t>("Inliers", k.data(), P);
            wr.write_vec<int32_t>("BestHypothesis", best.data(), P);
            wr.write_vec<int64_t>("VerifiedOffsets", voff.data(), P + 1);
            wr.write<int32_t>("VerifiedMatches", kept.data(), kept.size() / 2, 2);
        }
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        for (size_t p = 0; p < P; p++)
            printf("Pair %zu: %lld / %lld inliers, hypothesis %d\n", p, (long long)k[p], (long long)(moff[p + 1] - moff[p]), best[p]);
        if (ctx) printf("Kernels: %.6f ms\n", dlco_desc_last_kernel_ms(ctx));
        printf("Total: %.09f sec\n", sec);
        if (ctx) dlco_desc_destroy(ctx);
    } catch (const std::exception &e) {
        if (ctx) dlco_desc_destroy(ctx);
        std::fprintf(stderr, "verify-pairs: %s\n", e.what());
        return 2;
    }
    return 0;
}
