// The pieces of the refit round that opencv-dlco_amd/csrc/verify_rules.hpp and epipolar_rules.hpp share between the host and
// refit_pairs_kernel (kernels_verify.hip), walked on the CPU the way the kernel walks them, as a program of its own for the
// sanitizers:
//     g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined verify_refit_asan_main.cpp && ./a.out
// tests/test_verify_refit_rules.py builds and runs it as a child process.  No libdlco.so, no GPU.  walk() is the kernel's
// arithmetic on indices: chunks of kRefitChunk matches staged in arrays of exactly the kernel's LDS sizes, one "lane" per sum
// reading the staged rows at the positions dlt_terms / refit_terms give it, then the headers' solve on N, r, V in a work array
// of the kernel's size.  A read or write past a staged chunk, a row or the work array is the sanitizer's to find; the result
// must equal the host's refit_round in every bit, rejected rounds included.
#include "../../opencv-dlco_amd/csrc/epipolar_rules.hpp"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>

namespace vr = verify_rules;
namespace er = epipolar_rules;

namespace {

constexpr int C = vr::kRefitChunk, kLanes = vr::kRefitChunk;

using H = vr::Homography;
using F = er::Fundamental;

// the kernel's three passes and its solve; every array is on the heap at its exact size, so that the sanitizer sees its ends
template <typename R>
bool walk(const float *src, const float *dst, int m, const uint8_t *mask, double M[9])
{
    std::unique_ptr<double[]> rows(new double[C * R::kRefitRow]), work(new double[R::kRefitWork]), par(new double[6]), sum(new double[kLanes]);
    std::unique_ptr<uint8_t[]> in(new uint8_t[C]);
    int n = 0, first = -1;
    for (int l = 0; l < kLanes; l++) sum[l] = 0.0;
    for (int i0 = 0; i0 < m; i0 += C) {
        const int cnt = m - i0 < C ? m - i0 : C;
        for (int l = 0; l < cnt; l++) {
            rows[4 * l] = (double)src[2 * (i0 + l)]; rows[4 * l + 1] = (double)src[2 * (i0 + l) + 1];
            rows[4 * l + 2] = (double)dst[2 * (i0 + l)]; rows[4 * l + 3] = (double)dst[2 * (i0 + l) + 1];
            in[l] = mask[i0 + l];
        }
        for (int j = 0; j < cnt; j++) {
            if (!in[j]) continue;
            first = first < 0 ? i0 + j : first;
            n++;
            for (int l = 0; l < kLanes; l++) sum[l] = sum[l] + rows[4 * j + (l & 3)];
        }
    }
    for (int l = 0; l < 4; l++) par[l] = sum[l] / (double)n;
    for (int l = 0; l < kLanes; l++) sum[l] = 0.0;
    for (int i0 = 0; i0 < m; i0 += C) {
        const int cnt = m - i0 < C ? m - i0 : C;
        for (int l = 0; l < cnt; l++) {
            rows[2 * l] = vr::centred_length((double)src[2 * (i0 + l)], (double)src[2 * (i0 + l) + 1], par[0], par[1]);
            rows[2 * l + 1] = vr::centred_length((double)dst[2 * (i0 + l)], (double)dst[2 * (i0 + l) + 1], par[2], par[3]);
            in[l] = mask[i0 + l];
        }
        for (int j = 0; j < cnt; j++)
            if (in[j])
                for (int l = 0; l < kLanes; l++) sum[l] = sum[l] + rows[2 * j + (l & 1)];
    }
    for (int l = 0; l < 2; l++) par[4 + l] = sum[l] / (double)n;
    double ss = 0.0, sd = 0.0;
    bool ok = !R::refit_few(n);
    ok = vr::hartley_scale(par[4], ss) && ok;
    ok = vr::hartley_scale(par[5], sd) && ok;
    if (!ok) return false;
    for (int l = 0; l < kLanes; l++) sum[l] = 0.0;
    for (int i0 = 0; i0 < m; i0 += C) {
        const int cnt = m - i0 < C ? m - i0 : C;
        for (int l = 0; l < cnt; l++) {
            R::refit_row(vr::normalised((double)src[2 * (i0 + l)], par[0], ss), vr::normalised((double)src[2 * (i0 + l) + 1], par[1], ss),
                   vr::normalised((double)dst[2 * (i0 + l)], par[2], sd), vr::normalised((double)dst[2 * (i0 + l) + 1], par[3], sd), rows.get() + R::kRefitRow * l);
            in[l] = mask[i0 + l];
        }
        for (int j = 0; j < cnt; j++)
            if (in[j])
                for (int l = 0; l < kLanes; l++) sum[l] = R::refit_add(sum[l], rows.get() + R::kRefitRow * j, R::refit_terms(l));
    }
    for (int l = 0; l < R::kRefitSums; l++) work[l] = sum[l];
    return R::refit_solve(work.get(), par[0], par[1], ss, par[2], par[3], sd, (double)src[2 * first], (double)src[2 * first + 1], M);
}

uint64_t g_state = 777;
double uniform() { g_state += vr::kGolden; return (double)(vr::mix(g_state) >> 11) / 9007199254740992.0; }

struct List { std::vector<float> src, dst; };

// a homography with a little depth: both models find something to fit
List scene(int m, double span)
{
    List c{std::vector<float>((size_t)m * 2), std::vector<float>((size_t)m * 2)};
    for (int i = 0; i < m; i++) {
        const double x = span * (2 * uniform() - 1), y = span * (2 * uniform() - 1), z = 1.0 + 0.3 * uniform();
        const double w = 1.5e-8 * x - 1.0e-8 * y + 1.0;
        c.src[2 * i] = (float)x; c.src[2 * i + 1] = (float)y;
        c.dst[2 * i] = (float)((0.92 * x - 0.11 * y) / w + 140.0 / z); c.dst[2 * i + 1] = (float)((0.08 * x + 0.7 * y) / w - 60.0 + 5.0 * z);
    }
    return c;
}

int g_bad = 0, g_accepted[2] = {0, 0}, g_rejected[2] = {0, 0};

template <typename R>
void check(const char *name, const List &c, const std::vector<uint8_t> &mask, int model)
{
    const int m = (int)mask.size();
    double A[9], B[9];
    const bool a = walk<R>(c.src.data(), c.dst.data(), m, mask.data(), A), b = R::refit_round(c.src.data(), c.dst.data(), m, mask.data(), B);
    bool same = a == b;
    if (a && b) same = std::memcmp(A, B, sizeof A) == 0;
    (a ? g_accepted : g_rejected)[model]++;
    if (!same) { g_bad++; std::printf("%s %-22s m %4d: the walk and the host differ (%d, %d)\n", model ? "F" : "H", name, m, (int)a, (int)b); }
}

void both(const char *name, const List &c, const std::vector<uint8_t> &mask)
{
    check<H>(name, c, mask, 0);
    check<F>(name, c, mask, 1);
}

std::vector<uint8_t> ones(int m) { return std::vector<uint8_t>((size_t)m, 1); }
std::vector<uint8_t> at(int m, std::initializer_list<int> idx)
{
    std::vector<uint8_t> k((size_t)m, 0);
    for (int i : idx) k[(size_t)i] = 1;
    return k;
}

}  // namespace

int main()
{
    for (int m : {4, 8, C - 1, C, C + 1, 3 * C + 7}) {
        const List c = scene(m, 2000.0);
        both("all ones", c, ones(m));
        std::vector<uint8_t> some((size_t)m);
        for (int i = 0; i < m; i++) some[(size_t)i] = uniform() < 0.6 ? 1 : 0;
        both("random mask", c, some);
    }
    const int m = 3 * C + 7;
    const List c = scene(m, 2000.0);
    both("last of every chunk", c, at(m, {C - 1, 2 * C - 1, 3 * C - 1, m - 1}));
    both("last two of every chunk", c, at(m, {C - 2, C - 1, 2 * C - 2, 2 * C - 1, 3 * C - 2, 3 * C - 1, m - 2, m - 1}));
    std::vector<uint8_t> hole = ones(m), late = ones(m);
    for (int i = 0; i < C; i++) { hole[(size_t)(C + i)] = 0; late[(size_t)i] = 0; }
    both("a chunk without inlier", c, hole);
    both("first inlier at C", c, late);
    both("four inliers", c, at(m, {3, C, 2 * C + 5, m - 1}));
    both("eight inliers", c, at(m, {0, 1, C - 1, C, 2 * C, 2 * C + 1, 3 * C, m - 1}));
    both("seven inliers", c, at(m, {0, 1, C - 1, C, 2 * C, 2 * C + 1, 3 * C}));
    both("no inlier", c, at(m, {}));
    both("one inlier", c, at(m, {C}));
    List point{std::vector<float>(128, 7.f), std::vector<float>(128, 9.f)};
    both("one point", point, ones(64));
    List line;
    for (int i = 0; i < 64; i++) { line.src.insert(line.src.end(), {10.f + 7 * i, 20.f + 3 * i}); line.dst.insert(line.dst.end(), {5.f + 2 * i, 400.f - 5 * i}); }
    both("collinear", line, ones(64));
    List nan = scene(120, 2000.0);
    nan.src[10] = std::numeric_limits<float>::quiet_NaN();
    nan.dst[41] = std::numeric_limits<float>::infinity();
    both("nan masked in", nan, ones(120));
    std::vector<uint8_t> out = ones(120);
    out[5] = out[20] = 0;
    both("nan masked out", nan, out);
    both("far", scene(150, 1048576.0), ones(150));
    List shift;
    for (int i = 0; i < 200; i++) {
        const float x = (float)(int)(2000 * uniform()), y = (float)(int)(2000 * uniform());
        shift.src.insert(shift.src.end(), {x, y}); shift.dst.insert(shift.dst.end(), {x + 37.f, y - 12.f});
    }
    both("translation", shift, ones(200));
    // the index rule itself: every sum reads inside its row, and the sums of N are the products of all pairs of positions
    for (int l = 0; l < kLanes; l++) {
        const vr::Terms h = vr::dlt_terms(l), f = er::refit_terms(l);
        for (int i : {h.a, h.b, h.c, h.d}) g_bad += i < 0 || i >= vr::kDltRow;
        for (int i : {f.a, f.b}) g_bad += i < 0 || i >= er::kRefitRow;
        if (l < 64) g_bad += h.a != l / 8 || h.b != l % 8 || h.c != 8 + l / 8 || h.d != 8 + l % 8;
        if (l < er::kRefitSums) g_bad += f.a != l / 9 || f.b != l % 9;
    }
    for (int k = 0; k < 2; k++)
        if (g_accepted[k] == 0 || g_rejected[k] == 0) { g_bad++; std::printf("model %d: the cases hold no accepted or no rejected round\n", k); }
    std::printf("accepted H %d F %d, rejected H %d F %d\n", g_accepted[0], g_accepted[1], g_rejected[0], g_rejected[1]);
    std::printf(g_bad ? "verify_refit_asan: %d wrong\n" : "verify_refit_asan: ok\n", g_bad);
    return g_bad ? 1 : 0;
}
