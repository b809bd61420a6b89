// The host loops of opencv-dlco_amd/csrc/epipolar_rules.hpp, refit included, as a program of its own for the sanitizers:
//     g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined epipolar_asan_main.cpp && ./a.out
// tests/test_epipolar_rules.py builds and runs it as a child process.  No libdlco.so, no GPU.  It checks what must hold of any
// answer (counts within range, mask and count agree, no model where none can be), not particular values: those are compared
// against the numpy restatement by the tests.
#include "../../opencv-dlco_amd/csrc/epipolar_rules.hpp"

#include <cstdio>
#include <cstdlib>
#include <limits>

namespace er = epipolar_rules;
namespace vr = verify_rules;

namespace {

struct Case { const char *name; std::vector<float> src, dst; bool expect_model; };

uint64_t g_state = 12345;
double uniform() { g_state += vr::kGolden; return (double)(vr::mix(g_state) >> 11) / 9007199254740992.0; }

// points in front of two cameras of focal length 800: the second turned about the y axis and moved sideways
Case planted(const char *name, int m, double outliers)
{
    Case c{name, std::vector<float>((size_t)m * 2), std::vector<float>((size_t)m * 2), true};
    const double cs = std::cos(0.1), sn = std::sin(0.1);
    for (int i = 0; i < m; i++) {
        const double X = 4 * uniform() - 2, Y = 3 * uniform() - 1.5, Z = 4 + 4 * uniform();
        const double X2 = cs * X + sn * Z - 0.5, Z2 = -sn * X + cs * Z + 0.05;
        c.src[2 * i] = (float)(800 * X / Z + 512); c.src[2 * i + 1] = (float)(800 * Y / Z + 384);
        if (uniform() < outliers) { c.dst[2 * i] = (float)(1024 * uniform()); c.dst[2 * i + 1] = (float)(768 * uniform()); }
        else { c.dst[2 * i] = (float)(800 * X2 / Z2 + 512); c.dst[2 * i + 1] = (float)(800 * (Y + 0.02) / Z2 + 384); }
    }
    return c;
}

int run(const Case &c, int32_t n_hyp, int32_t refine)
{
    const int64_t m = (int64_t)c.src.size() / 2;
    std::vector<double> F_all((size_t)n_hyp * 9), rounds((size_t)(refine > 0 ? refine : 1) * 9);
    std::vector<int32_t> counts((size_t)n_hyp);
    std::vector<uint8_t> mask((size_t)m);
    double F[9];
    int64_t count = -1;
    int32_t best = -2, n_rounds = -1;
    er::verify_host(c.src.data(), c.dst.data(), m, 1.0f, n_hyp, 99, refine, F_all.data(), counts.data(), F, mask.data(), &count, &best, rounds.data(), &n_rounds);
    int64_t in_mask = 0;
    for (uint8_t b : mask) in_mask += b;
    bool ok = in_mask == count && count >= 0 && count <= m && best >= -1 && best < n_hyp && n_rounds >= 0 && n_rounds <= refine;
    for (int32_t h = 0; h < n_hyp; h++) ok = ok && counts[h] >= 0 && counts[h] <= m && (best < 0 ? counts[h] == 0 : counts[h] <= counts[best]);
    ok = ok && (best >= 0) == c.expect_model && (best >= 0 || count == 0);
    for (int i = 0; i < 9; i++) ok = ok && F[i] == F[i] && (best >= 0 || F[i] == 0.0);
    std::printf("%-12s m %5lld  best %5d  inliers %5lld  rounds %d  %s\n", c.name, (long long)m, best, (long long)count, n_rounds, ok ? "ok" : "WRONG");
    return ok ? 0 : 1;
}

}  // namespace

int main()
{
    int bad = 0;
    bad += run(planted("planted", 257, 0.3), 256, 2);
    bad += run(planted("refine8", 1000, 0.5), 128, 8);
    bad += run(planted("norefine", 63, 0.25), 65, 0);
    bad += run(planted("eight", 8, 0.0), 64, 2);
    Case point{"one_point", std::vector<float>(128, 7.f), std::vector<float>(128, 9.f), false};
    bad += run(point, 256, 2);
    Case line{"collinear", {}, {}, false};                     // every sample's system loses rank: x, y, u, v are affine in i
    for (int i = 0; i < 64; i++) { line.src.insert(line.src.end(), {10.f + 8 * i, 20.f + 4 * i}); line.dst.insert(line.dst.end(), {5.f + 2 * i, 400.f - 4 * i}); }
    bad += run(line, 256, 2);
    Case nan = planted("nan", 120, 0.0);
    nan.src[0] = nan.dst[11] = nan.src[35] = std::numeric_limits<float>::quiet_NaN();
    nan.dst[40] = std::numeric_limits<float>::infinity();
    bad += run(nan, 256, 2);
    Case all_nan = planted("all_nan", 16, 0.0);
    for (float &v : all_nan.src) v = std::numeric_limits<float>::quiet_NaN();
    all_nan.expect_model = false;
    bad += run(all_nan, 64, 2);
    std::printf(bad ? "epipolar_asan: %d cases wrong\n" : "epipolar_asan: ok\n", bad);
    return bad ? 1 : 0;
}
