// verify — geometric verification of a match list, over libdlco.so: the end of detect -> describe-image -> match.
//
//     verify query_kp_file train_kp_file match_file -out dst [-thresh f] [-hyp n] [-seed n] [-refine n] [-device n]
//            [-model homography|fundamental]
//
// The two keypoint files hold "Keypoints" [n,4] f32 as `detect` writes them, match_file holds "Matches" [m,2] i32 =
// (query, train) as `match` writes them.  The (x, y) columns of the matched keypoints go to the library's deterministic
// RANSAC for a homography from query to train (dlco_desc_verify_homography; the rule: csrc/verify_rules.hpp): -hyp n
// hypotheses (default 2048, 1 .. 1048576), inliers within -thresh f pixels of forward transfer error (default 3), at most
// -refine n refit rounds (default 2, 0 .. 8), sampler seed -seed n (default 0).  It is not cv::findHomography.  Writes
//     "Homography" [3,3] f32        H rounded for reading
//     "HomographyBits" [9] i64      the bits of H's doubles, row-major: the exact answer
//     "Inlier" [m] u8               1 where the match agrees with H
//     "VerifiedMatches" [k,2] i32   the rows of "Matches" with Inlier == 1
//     "BestHypothesis" [1] i32      the winning hypothesis, -1: no model (H and Inlier are zero)
// and prints "Matches: m", "Inliers: k / m", "Hypothesis: h".  Fewer than 4 matches give the no-model result without a device.
// An index of "Matches" outside its keypoint table is an error before a device is opened.
// With -model fundamental the model is a fundamental matrix F, train^T F query = 0 (dlco_desc_verify_fundamental; the rule:
// csrc/epipolar_rules.hpp; it is not cv::findFundamentalMat): -thresh bounds the Sampson error, and the first two datasets
// are "Fundamental" [3,3] f32 and "FundamentalBits" [9] i64 instead.  Fewer than 8 matches give the no-model result.  Without
// the option the tool does what it did before the option existed.
// The reference has no such tool.  A path that does not end in .h5/.hdf5 is a directory of .npy files with the same
// dataset names (dlco_io.hpp).
#include "../../include/dlco.h"
#include "dlco_io.hpp"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>

using std::cout;
using std::endl;

namespace {
void load_keypoints(const char *path, std::vector<size_t> &shape, std::vector<float> &rows)
{
    dlco_io::read_dataset<float>(path, "Keypoints", shape, rows);
    if (shape.size() != 2 || shape[1] != 4) throw std::runtime_error(std::string(path) + ": Keypoints must be an [n, 4] table");
}
}  // namespace

int main(int argc, char **argv)
{
    int device = 0;
    long long n_hyp = 2048, refine = 2;
    unsigned long long seed = 0;
    float thresh = 3.0f;
    bool help = false, fundamental = false, model_given = false;
    const char *qf = nullptr, *tf = nullptr, *mf = nullptr, *out = nullptr;
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
                model_given = true;
                if (std::strcmp(name, "fundamental") == 0) { fundamental = true; continue; }
                if (std::strcmp(name, "homography") == 0) { fundamental = false; continue; }
                cout << "ERROR: -model must be homography or fundamental." << endl;
                help = true;
                continue;
            }
            cout << "ERROR: Invalid " << argv[i] << " option." << endl;
            help = true;
        } else {
            if (!qf) { qf = argv[i]; continue; }
            if (!tf) { tf = argv[i]; continue; }
            if (!mf) { mf = argv[i]; continue; }
            help = true;
        }
    }
    if (!qf || !tf || !mf || !out) help = true;
    if (!(std::isfinite(thresh) && thresh > 0.0f)) { cout << "ERROR: -thresh must be positive." << endl; help = true; }
    if (n_hyp < 1 || n_hyp > 1048576) { cout << "ERROR: -hyp must be in 1 .. 1048576." << endl; help = true; }
    if (refine < 0 || refine > 8) { cout << "ERROR: -refine must be in 0 .. 8." << endl; help = true; }
    if (help) {
        cout << endl;
        cout << "Usage: verify query_kp_file train_kp_file match_file -out dst_h5_filename [-thresh f] [-hyp n] [-seed n] [-refine n] [-device n]" << endl;
        if (model_given) cout << "       -model homography|fundamental (default homography)" << endl;
        cout << endl;
        return 1;
    }
    dlco_desc_ctx *ctx = nullptr;
    try {
        std::vector<size_t> qs, ts, ms;
        std::vector<float> Q, T;
        std::vector<int32_t> M;
        load_keypoints(qf, qs, Q);
        load_keypoints(tf, ts, T);
        dlco_io::read_dataset<int32_t>(mf, "Matches", ms, M);
        if (ms.size() != 2 || ms[1] != 2) throw std::runtime_error(std::string(mf) + ": Matches must be an [m, 2] table");
        const size_t m = ms[0];
        std::vector<float> src(m * 2), dst(m * 2);
        for (size_t i = 0; i < m; i++) {
            const int32_t q = M[2 * i], t = M[2 * i + 1];
            if (q < 0 || (size_t)q >= qs[0] || t < 0 || (size_t)t >= ts[0])
                throw std::runtime_error("match " + std::to_string(i) + " = (" + std::to_string(q) + ", " + std::to_string(t) + ") is outside the keypoint tables of " +
                                         std::to_string(qs[0]) + " and " + std::to_string(ts[0]) + " rows");
            src[2 * i] = Q[4 * (size_t)q]; src[2 * i + 1] = Q[4 * (size_t)q + 1];
            dst[2 * i] = T[4 * (size_t)t]; dst[2 * i + 1] = T[4 * (size_t)t + 1];
        }
        printf("Matches: %zu\n", m);

        const auto t0 = std::chrono::steady_clock::now();
        double H[9] = {0};
        std::vector<uint8_t> inlier(m, 0);
        int64_t k = 0;
        int32_t best = -1;
        if (m >= (fundamental ? 8u : 4u)) {
            if (dlco_desc_create(&ctx, 1.4f, 8, 1, device) != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(nullptr));
            const auto verify = fundamental ? dlco_desc_verify_fundamental : dlco_desc_verify_homography;      // one signature
            if (verify(ctx, src.data(), dst.data(), (int64_t)m, thresh, (int32_t)n_hyp, (uint64_t)seed, (int32_t)refine, H, inlier.data(), &k, &best) !=
                DLCO_OK)
                throw std::runtime_error(dlco_desc_last_error(ctx));
        }
        float Hf[9];
        int64_t bits[9];
        for (int i = 0; i < 9; i++) { Hf[i] = (float)H[i]; std::memcpy(&bits[i], &H[i], sizeof(double)); }
        std::vector<int32_t> kept;
        for (size_t i = 0; i < m; i++)
            if (inlier[i]) { kept.push_back(M[2 * i]); kept.push_back(M[2 * i + 1]); }
        {
            dlco_io::Writer wr(out);
            wr.write<float>(fundamental ? "Fundamental" : "Homography", Hf, 3, 3);
            wr.write_vec<int64_t>(fundamental ? "FundamentalBits" : "HomographyBits", bits, 9);
            wr.write_vec<uint8_t>("Inlier", inlier.data(), m);
            wr.write<int32_t>("VerifiedMatches", kept.data(), kept.size() / 2, 2);
            wr.write_vec<int32_t>("BestHypothesis", &best, 1);
        }
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("Inliers: %lld / %zu\n", (long long)k, m);
        printf("Hypothesis: %d\n", best);
        printf("Total: %.09f sec\n", sec);
        if (ctx) dlco_desc_destroy(ctx);
    } catch (const std::exception &e) {
        if (ctx) dlco_desc_destroy(ctx);
        std::fprintf(stderr, "verify: %s\n", e.what());
        return 2;
    }
    return 0;
}
