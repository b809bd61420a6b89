// The host loop of opencv-dlco_amd/csrc/guided_epipolar_rules.hpp as a program of its own for the sanitizers:
//     g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined guided_epipolar_asan_main.cpp && ./a.out
// tests/test_guided_epipolar_rules.py builds and runs it as a child process.  No libdlco.so, no GPU.  It checks what must hold
// of any answer (indices in range and admitted, the two columns ordered by the key, empty rows left at -1 / +inf), not
// particular values: those are compared against numpy by the tests.
#include "../../opencv-dlco_amd/csrc/guided_epipolar_rules.hpp"

#include <cstdio>
#include <limits>

namespace ge = guided_epipolar;
namespace vr = verify_rules;

namespace {

uint64_t g_state = 4711;
double uniform() { g_state += vr::kGolden; return (double)(vr::mix(g_state) >> 11) / 9007199254740992.0; }

// model 0: [e']x H of a mild homography, a generic F; 1: all zero (admits nothing); 2: rectified stereo
int run(const char *name, int64_t nq, int64_t nt, float threshold, int f_side, bool poison, int model)
{
    const double S = 8.0 * std::sqrt((double)nt);
    const double H[9] = {0.98, -0.05, 0.03 * S, 0.04, 1.02, -0.02 * S, 0.02 / S, -0.01 / S, 1.0};
    const double ex = 3.0 * S, ey = 0.4 * S;
    double F[9] = {0};
    if (model == 0) {
        for (int j = 0; j < 3; j++) {
            F[j] = -H[3 + j] + ey * H[6 + j];
            F[3 + j] = H[j] - ex * H[6 + j];
            F[6 + j] = -ey * H[j] + ex * H[3 + j];
        }
    } else if (model == 2) {
        F[5] = -1.0; F[7] = 1.0;
    }
    std::vector<float> qxy((size_t)nq * 2), txy((size_t)nt * 2), dist((size_t)nq * nt);
    for (float &v : qxy) v = (float)(S * uniform());
    for (float &v : txy) v = (float)(S * uniform());
    for (float &v : dist) v = (float)(int)(8 * uniform());                    // many ties
    if (poison && nq >= 3) {
        qxy[0] = std::numeric_limits<float>::quiet_NaN();                     // admits nothing
        qxy[2] = (float)(-60.0 * S); qxy[3] = 0.f;
        qxy[4] = std::numeric_limits<float>::infinity();                      // inf - inf somewhere: NaN, admits nothing
        txy[1] = std::numeric_limits<float>::quiet_NaN();
    }
    std::vector<int32_t> idx((size_t)nq * 2, -7);
    std::vector<float> d((size_t)nq * 2, -7.f);
    ge::guided_top2_host(dist.data(), qxy.data(), nq, txy.data(), nt, F, threshold, f_side, idx.data(), d.data());
    const double t2 = vr::threshold_sq(threshold);
    const float inf = std::numeric_limits<float>::infinity();
    bool ok = true;
    int64_t empty = 0;
    for (int64_t i = 0; i < nq; i++) {
        int64_t admitted = 0;
        for (int64_t j = 0; j < nt; j++) admitted += ge::pair_admitted(F, t2, f_side, &qxy[2 * i], &txy[2 * j]) ? 1 : 0;
        empty += admitted == 0;
        for (int k = 0; k < 2; k++) {
            const int32_t j = idx[2 * i + k];
            const bool want = admitted > k;
            ok = ok && (want ? (j >= 0 && j < nt && ge::pair_admitted(F, t2, f_side, &qxy[2 * i], &txy[2 * (int64_t)j]) && d[2 * i + k] == dist[i * nt + j])
                             : (j == -1 && d[2 * i + k] == inf));
        }
        if (admitted >= 2)
            ok = ok && idx[2 * i] != idx[2 * i + 1] && (d[2 * i] < d[2 * i + 1] || (d[2 * i] == d[2 * i + 1] && idx[2 * i] < idx[2 * i + 1]));
    }
    if (poison && nq >= 3) ok = ok && idx[0] == -1;                           // the NaN query
    if (model == 1) ok = ok && empty == nq;
    std::printf("%-10s nq %5lld nt %5lld threshold %g f_side %d model %d  empty rows %lld  %s\n", name, (long long)nq, (long long)nt, (double)threshold,
                f_side, model, (long long)empty, ok ? "ok" : "WRONG");
    return ok ? 0 : 1;
}

}  // namespace

int main()
{
    int bad = 0;
    for (int f_side = 0; f_side < 2; f_side++) {
        bad += run("uniform", 300, 500, 2.f, f_side, false, 0);
        bad += run("poisoned", 130, 129, 2.f, f_side, true, 0);
        bad += run("sparse", 200, 300, 0.01f, f_side, true, 0);               // most rows empty or with one candidate
        bad += run("zero", 17, 40, 2.f, f_side, false, 1);                    // the all-zero F: every row empty
        bad += run("all", 40, 17, 1048576.f, f_side, true, 0);
        bad += run("stereo", 60, 70, 0.5f, f_side, true, 2);
        bad += run("one", 1, 1, 2.f, f_side, false, 0);
    }
    std::printf(bad ? "guided_epipolar_asan: %d cases wrong\n" : "guided_epipolar_asan: ok\n", bad);
    return bad ? 1 : 0;
}
