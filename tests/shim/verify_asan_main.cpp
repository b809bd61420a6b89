// The host loops of opencv-dlco_amd/csrc/verify_rules.hpp, refit included, as a program of its own for the sanitizers:
//     g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined verify_asan_main.cpp && ./a.out
// tests/test_verify_rules.py builds and runs it as a child process.  No libdlco.so, no GPU.  It checks what must hold of any
// answer (counts within range, mask and count agree, no model where none can be), not particular values: those are compared
// against the numpy restatement by the tests.
#include "../../opencv-dlco_amd/csrc/verify_rules.hpp"

#include <cstdio>
#include <cstdlib>
#include <limits>

namespace vr = verify_rules;

namespace {

struct Case { const char *name; std::vector<float> src, dst; bool expect_model; };

uint64_t g_state = 12345;
double uniform() { g_state += vr::kGolden; return (double)(vr::mix(g_state) >> 11) / 9007199254740992.0; }

Case planted(const char *name, int m, double outliers, double span)
{
    Case c{name, std::vector<float>((size_t)m * 2), std::vector<float>((size_t)m * 2), true};
    for (int i = 0; i < m; i++) {
        const double x = span * (2 * uniform() - 1), y = span * (2 * uniform() - 1);
        const double w = 1.5e-8 * x - 1.0e-8 * y + 1.0;
        c.src[2 * i] = (float)x; c.src[2 * i + 1] = (float)y;
        if (uniform() < outliers) { c.dst[2 * i] = (float)(span * uniform()); c.dst[2 * i + 1] = (float)(span * uniform()); }
        else { c.dst[2 * i] = (float)((0.92 * x - 0.11 * y + 140.0) / w + uniform() - 0.5); c.dst[2 * i + 1] = (float)((0.08 * x + 0.7 * y - 60.0) / w + uniform() - 0.5); }
    }
    return c;
}

int run(const Case &c, int32_t n_hyp, int32_t refine)
{
    const int64_t m = (int64_t)c.src.size() / 2;
    std::vector<double> H_all((size_t)n_hyp * 9), rounds((size_t)(refine > 0 ? refine : 1) * 9);
    std::vector<int32_t> counts((size_t)n_hyp);
    std::vector<uint8_t> mask((size_t)m);
    double H[9];
    int64_t count = -1;
    int32_t best = -2, n_rounds = -1;
    vr::verify_host(c.src.data(), c.dst.data(), m, 3.0f, n_hyp, 99, refine, H_all.data(), counts.data(), H, mask.data(), &count, &best, rounds.data(), &n_rounds);
    int64_t in_mask = 0;
    for (uint8_t b : mask) in_mask += b;
    bool ok = in_mask == count && count >= 0 && count <= m && best >= -1 && best < n_hyp && n_rounds >= 0 && n_rounds <= refine;
    for (int32_t h = 0; h < n_hyp; h++) ok = ok && counts[h] >= 0 && counts[h] <= m && (best < 0 ? counts[h] == 0 : counts[h] <= counts[best]);
    ok = ok && (best >= 0) == c.expect_model && (best >= 0 || count == 0);
    for (int i = 0; i < 9; i++) ok = ok && H[i] == H[i] && (best >= 0 || H[i] == 0.0);
    std::printf("%-12s m %5lld  best %5d  inliers %5lld  rounds %d  %s\n", c.name, (long long)m, best, (long long)count, n_rounds, ok ? "ok" : "WRONG");
    return ok ? 0 : 1;
}

}  // namespace

int main()
{
    int bad = 0;
    bad += run(planted("planted", 257, 0.5, 2000.0), 256, 2);
    bad += run(planted("refine8", 1000, 0.6, 2000.0), 128, 8);
    bad += run(planted("norefine", 63, 0.3, 2000.0), 65, 0);
    bad += run(planted("four", 4, 0.0, 500.0), 64, 2);
    bad += run(planted("far", 150, 0.2, 1048576.0), 256, 2);
    Case line{"collinear", {}, {}, false};
    for (int i = 0; i < 64; i++) { line.src.insert(line.src.end(), {10.f + 7 * i, 20.f + 3 * i}); line.dst.insert(line.dst.end(), {5.f + 2 * i, 400.f - 5 * i}); }
    bad += run(line, 256, 2);
    Case nan = planted("nan", 120, 0.0, 2000.0);
    nan.src[0] = nan.dst[11] = nan.src[35] = std::numeric_limits<float>::quiet_NaN();
    nan.dst[40] = std::numeric_limits<float>::infinity();
    bad += run(nan, 256, 2);
    Case all_nan = planted("all_nan", 16, 0.0, 2000.0);
    for (float &v : all_nan.src) v = std::numeric_limits<float>::quiet_NaN();
    all_nan.expect_model = false;
    bad += run(all_nan, 64, 2);
    Case shift{"translation", {}, {}, true};
    for (int i = 0; i < 200; i++) {
        const float x = (float)(int)(2000 * uniform()), y = (float)(int)(2000 * uniform());
        shift.src.insert(shift.src.end(), {x, y}); shift.dst.insert(shift.dst.end(), {x + 37.f, y - 12.f});
    }
    bad += run(shift, 256, 2);
    std::printf(bad ? "verify_asan: %d cases wrong\n" : "verify_asan: ok\n", bad);
    return bad ? 1 : 0;
}
