// Sanitizer walk of the host side of dlco_desc_select_pairs* (opencv-dlco_amd/csrc/select_rules.hpp): built with
// -fsanitize=address,undefined by tests/test_select_rules.py and run as a program.  The synthetic set of that test (nine images
// of 0 .. 300 rows, all 81 ordered pairs, answers with missing candidates and planted agreement) from a generator of its own,
// batches of empty images only, and seeded sets of sizes and pairs: the pair records, the search of a row's pair, the bound
// check of the reverse table and the whole call in the kernels' cut (flag words, block counts, the scan in chunks with a
// carry, the scatter, the offsets) against a plain loop over the pairs.  Every buffer has its exact size.  Pure host code.
#include "../../opencv-dlco_amd/csrc/select_rules.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>

namespace sr = select_rules;

namespace {
uint64_t state = 0x9e3779b97f4a7c15ull;
uint64_t next() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state >> 33; }

#define REQUIRE(c) do { if (!(c)) { std::printf("select_rules_asan: FAILED %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

template <typename Dist> Dist none();
template <> float none<float>() { return __builtin_inff(); }
template <> int32_t none<int32_t>() { return INT32_MAX; }

struct Batch {
    std::vector<int64_t> seg, row0;
    std::vector<int32_t> pairs;
    int64_t P = 0, R = 0;
};

Batch batch_of(const std::vector<int64_t> &sizes, const std::vector<int32_t> &pairs)
{
    Batch b;
    b.seg.assign(1, 0);
    for (int64_t n : sizes) b.seg.push_back(b.seg.back() + n);
    b.pairs = pairs;
    b.P = (int64_t)pairs.size() / 2;
    b.row0.assign(1, 0);
    for (int64_t p = 0; p < b.P; p++) b.row0.push_back(b.row0.back() + sizes[(size_t)pairs[2 * (size_t)p]]);
    b.R = b.row0.back();
    return b;
}

// answers of the synthetic kind; stray: some indices outside [-1, nt), which the rule must drop without a read
template <typename Dist>
void answers(const Batch &b, const std::vector<int64_t> &sizes, bool stray, std::vector<int32_t> &idx, std::vector<Dist> &d)
{
    idx.assign((size_t)b.R * 2, -1);
    d.assign((size_t)b.R * 2, none<Dist>());
    for (int64_t p = 0; p < b.P; p++) {
        const int64_t na = sizes[(size_t)b.pairs[2 * (size_t)p]], nb = sizes[(size_t)b.pairs[2 * (size_t)p + 1]];
        for (int64_t i = 0; i < na && nb > 0; i++) {
            const size_t g = (size_t)(b.row0[(size_t)p] + i);
            if (next() % 10 == 0) continue;
            const int64_t j = (int64_t)(next() % (uint64_t)nb), k = 1 + (int64_t)(next() % 999), m = (int64_t)(next() % 5);
            idx[2 * g] = (int32_t)j;
            d[2 * g] = (Dist)(m * k);
            if (nb > 1) { idx[2 * g + 1] = (int32_t)((j + 1 + (int64_t)(next() % (uint64_t)(nb - 1))) % nb); d[2 * g + 1] = (Dist)(4 * k); }
            if (stray && next() % 16 == 0) idx[2 * g] = (next() & 1) ? (int32_t)(nb + (int64_t)(next() % 100000)) : -2 - (int32_t)(next() % 100000);
        }
    }
}

// the reverse tables of all pairs, one after another, each of exactly nt_b rows; every second pair has none
void reverse_tables(const Batch &b, const std::vector<int64_t> &sizes, std::vector<int32_t> &back, std::vector<int64_t> &back_row0)
{
    back.clear();
    back_row0.assign((size_t)b.P, -1);
    for (int64_t p = 0; p < b.P; p++) {
        const int64_t na = sizes[(size_t)b.pairs[2 * (size_t)p]], nb = sizes[(size_t)b.pairs[2 * (size_t)p + 1]];
        if (p % 2 == 1) continue;
        back_row0[(size_t)p] = (int64_t)back.size() / 2;
        for (int64_t j = 0; j < nb; j++) { back.push_back(na > 0 ? (int32_t)(next() % (uint64_t)na) : -1); back.push_back(-1); }
    }
}

template <typename Dist>
void check(const std::vector<int64_t> &sizes, const std::vector<int32_t> &pairs, float f, bool mutual, bool with_xy, bool stray)
{
    const Batch b = batch_of(sizes, pairs);
    std::vector<int32_t> idx, back;
    std::vector<Dist> d;
    std::vector<int64_t> back_row0;
    answers(b, sizes, stray, idx, d);
    if (mutual) {
        reverse_tables(b, sizes, back, back_row0);
        REQUIRE(sr::back_rows_ok(b.seg.data(), b.pairs.data(), b.P, back_row0.data(), (int64_t)back.size() / 2));
        if (!back.empty()) REQUIRE(!sr::back_rows_ok(b.seg.data(), b.pairs.data(), b.P, back_row0.data(), (int64_t)back.size() / 2 - 1));
    }
    const int64_t ldxy = 3;
    std::vector<float> xy;
    if (with_xy)
        for (int64_t r = 0; r < b.seg.back() * ldxy; r++) xy.push_back((float)(next() % 4096) * 0.25f);

    std::vector<sr::Pair> rec;
    REQUIRE(sr::pair_records(b.seg.data(), b.pairs.data(), b.P, mutual ? back_row0.data() : nullptr, rec) == b.R);
    for (int64_t p = 0; p < b.P; p++)
        for (int64_t g = b.row0[(size_t)p]; g < b.row0[(size_t)p + 1]; g++) REQUIRE(sr::pair_of_row(rec.data(), 0, b.P - 1, g) == p);

    // the plain loop: pair by pair, row by row
    std::vector<int64_t> want_off(1, 0);
    std::vector<int32_t> want_m;
    std::vector<Dist> want_d;
    std::vector<float> want_src, want_dst;
    for (int64_t p = 0; p < b.P; p++) {
        const int32_t a = b.pairs[2 * (size_t)p], t = b.pairs[2 * (size_t)p + 1];
        const int64_t nt = sizes[(size_t)t];
        for (int64_t i = 0; i < sizes[(size_t)a]; i++) {
            const size_t g = (size_t)(b.row0[(size_t)p] + i);
            const int32_t j = idx[2 * g];
            if (j < 0 || j >= nt) continue;
            if (f != 0.0f && idx[2 * g + 1] != -1 && !((double)d[2 * g] < (double)f * (double)f * (double)d[2 * g + 1])) continue;
            if (mutual && back_row0[(size_t)p] >= 0 && back[2 * (size_t)(back_row0[(size_t)p] + j)] != (int32_t)i) continue;
            want_m.push_back((int32_t)i);
            want_m.push_back(j);
            want_d.push_back(d[2 * g]);
            if (with_xy)
                for (int k = 0; k < 2; k++) {
                    want_src.push_back(xy[(size_t)((b.seg[(size_t)a] + i) * ldxy + k)]);
                    want_dst.push_back(xy[(size_t)((b.seg[(size_t)t] + j) * ldxy + k)]);
                }
        }
        want_off.push_back((int64_t)want_d.size());
    }
    const size_t M = want_d.size();

    // outputs of exactly M entries: a write beyond the list is the sanitizer's to find
    std::vector<int64_t> moff((size_t)b.P + 1, -7);
    std::vector<int32_t> m(2 * M);
    std::vector<Dist> dd(M);
    std::vector<float> src(with_xy ? 2 * M : 0), dst(with_xy ? 2 * M : 0);
    sr::select_host(rec.data(), b.P, b.R, idx.data(), d.data(), f, mutual ? back.data() : nullptr, with_xy ? xy.data() : nullptr, ldxy, moff.data(),
                    m.data(), dd.data(), with_xy ? src.data() : nullptr, with_xy ? dst.data() : nullptr);
    REQUIRE(moff == want_off && m == want_m && dd == want_d && src == want_src && dst == want_dst);
}

int runs = 0;
void check_all(const std::vector<int64_t> &sizes, const std::vector<int32_t> &pairs)
{
    const float ratios[] = {0.0f, 0.5f, 0.8f, 1.0f};
    for (float f : ratios)
        for (int k = 0; k < 8; k++) {
            check<float>(sizes, pairs, f, (k & 1) != 0, (k & 2) != 0, (k & 4) != 0);
            check<int32_t>(sizes, pairs, f, (k & 1) != 0, (k & 2) != 0, (k & 4) != 0);
            runs += 2;
        }
}
}  // namespace

int main()
{
    // the synthetic set
    const std::vector<int64_t> sizes = {0, 1, 63, 64, 65, 255, 256, 257, 300};
    std::vector<int32_t> all;
    for (int32_t a = 0; a < 9; a++)
        for (int32_t b = 0; b < 9; b++) { all.push_back(a); all.push_back(b); }
    check_all(sizes, all);
    // batches of empty images only (R = 0), and of empty query or train images only
    check_all({0, 0, 0}, {0, 1, 1, 2, 2, 2});
    check_all({0}, {0, 0});
    check_all({0, 5}, {0, 1, 0, 0, 0, 1});
    check_all({0, 5}, {1, 0, 1, 0});
    // rows beyond one chunk of the scan, from two images and repeated pairs
    {
        const int64_t rows = (int64_t)sr::kScanChunk * sr::kBlockRows + 1;
        std::vector<int32_t> rep;
        for (int k = 0; k < 5; k++) { rep.push_back(k & 1); rep.push_back(1 - (k & 1)); }
        check<float>({rows / 2, rows - rows / 2}, rep, 0.8f, true, true, false);
        check<int32_t>({rows / 2, rows - rows / 2}, rep, 0.0f, false, false, true);
        runs += 2;
    }
    // seeded sets
    const int64_t some[] = {0, 1, 63, 64, 65, 255, 256, 257, 1000};
    for (int set = 0; set < 6; set++) {
        const int n_img = 1 + (int)(next() % 8);
        std::vector<int64_t> sz;
        for (int i = 0; i < n_img; i++) sz.push_back((next() & 1) ? some[next() % 9] : (int64_t)(next() % 600));
        const int64_t P = 1 + (int64_t)(next() % 60);
        std::vector<int32_t> pr;
        for (int64_t p = 0; p < 2 * P; p++) pr.push_back((int32_t)(next() % (uint64_t)n_img));
        check_all(sz, pr);
    }
    std::printf("select_rules_asan: ok (%d runs)\n", runs);
    return 0;
}
