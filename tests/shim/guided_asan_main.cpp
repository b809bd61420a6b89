// The host loop of opencv-dlco_amd/csrc/guided_rules.hpp as a program of its own for the sanitizers:
//     g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined guided_asan_main.cpp && ./a.out
// tests/test_guided_rules.py builds and runs it as a child process.  No libdlco.so, no GPU.  It checks what must hold of any
// answer (indices in range and admitted, the two columns ordered by the key, empty rows left at -1 / +inf), not particular
// values: those are compared against numpy by the tests.
#include "../../opencv-dlco_amd/csrc/guided_rules.hpp"

#include <cstdio>
#include <limits>

namespace gr = guided_rules;
namespace vr = verify_rules;

namespace {

uint64_t g_state = 4711;
double uniform() { g_state += vr::kGolden; return (double)(vr::mix(g_state) >> 11) / 9007199254740992.0; }

int run(const char *name, int64_t nq, int64_t nt, float radius, int h_side, bool poison)
{
    const double S = 8.0 * std::sqrt((double)nt);
    const double H[9] = {0.98, -0.05, 0.03 * S, 0.04, 1.02, -0.02 * S, 0.02 / S, -0.01 / S, 1.0};
    std::vector<float> qxy((size_t)nq * 2), txy((size_t)nt * 2), dist((size_t)nq * nt);
    for (float &v : qxy) v = (float)(S * uniform());
    for (float &v : txy) v = (float)(S * uniform());
    for (float &v : dist) v = (float)(int)(8 * uniform());                    // many ties
    if (poison && nq >= 3) {
        qxy[0] = std::numeric_limits<float>::quiet_NaN();                     // admits nothing
        qxy[2] = (float)(-60.0 * S); qxy[3] = 0.f;                            // W < 0: admits nothing
        qxy[4] = std::numeric_limits<float>::infinity();
        txy[1] = std::numeric_limits<float>::quiet_NaN();
    }
    std::vector<int32_t> idx((size_t)nq * 2, -7);
    std::vector<float> d((size_t)nq * 2, -7.f);
    gr::guided_top2_host(dist.data(), qxy.data(), nq, txy.data(), nt, H, radius, h_side, idx.data(), d.data());
    const double t2 = vr::threshold_sq(radius);
    const float inf = std::numeric_limits<float>::infinity();
    bool ok = true;
    int64_t empty = 0;
    for (int64_t i = 0; i < nq; i++) {
        int64_t admitted = 0;
        for (int64_t j = 0; j < nt; j++) admitted += gr::pair_admitted(H, t2, h_side, &qxy[2 * i], &txy[2 * j]) ? 1 : 0;
        empty += admitted == 0;
        for (int k = 0; k < 2; k++) {
            const int32_t j = idx[2 * i + k];
            const bool want = admitted > k;
            ok = ok && (want ? (j >= 0 && j < nt && gr::pair_admitted(H, t2, h_side, &qxy[2 * i], &txy[2 * (int64_t)j]) && d[2 * i + k] == dist[i * nt + j])
                             : (j == -1 && d[2 * i + k] == inf));
        }
        if (admitted >= 2)
            ok = ok && idx[2 * i] != idx[2 * i + 1] && (d[2 * i] < d[2 * i + 1] || (d[2 * i] == d[2 * i + 1] && idx[2 * i] < idx[2 * i + 1]));
    }
    if (poison && nq >= 3 && h_side == 0) ok = ok && idx[0] == -1 && idx[2] == -1 && idx[4] == -1;
    std::printf("%-10s nq %5lld nt %5lld radius %g h_side %d  empty rows %lld  %s\n", name, (long long)nq, (long long)nt, (double)radius, h_side,
                (long long)empty, ok ? "ok" : "WRONG");
    return ok ? 0 : 1;
}

}  // namespace

int main()
{
    int bad = 0;
    for (int h_side = 0; h_side < 2; h_side++) {
        bad += run("uniform", 300, 500, 12.f, h_side, false);
        bad += run("poisoned", 130, 129, 12.f, h_side, true);
        bad += run("sparse", 200, 300, 1.5f, h_side, true);                   // most rows empty or with one candidate
        bad += run("none", 17, 40, 1e-3f, h_side, false);                     // every row empty
        bad += run("all", 40, 17, 1048576.f, h_side, true);
        bad += run("one", 1, 1, 12.f, h_side, false);
    }
    std::printf(bad ? "guided_asan: %d cases wrong\n" : "guided_asan: ok\n", bad);
    return bad ? 1 : 0;
}
