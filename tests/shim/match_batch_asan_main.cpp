// Sanitizer walk of the batch planner (opencv-dlco_amd/csrc/match_batch.hpp): built with -fsanitize=address,undefined by
// tests/test_match_batch_rules.py and run as a program.  Seeded sets of image sizes and pairs, both shapes, several CU
// counts; every plan is checked for the properties the kernels rely on.  Pure host code.
#include "../../opencv-dlco_amd/csrc/match_batch.hpp"

#include <cstdio>
#include <cstdlib>

namespace {
uint64_t state = 0x9e3779b97f4a7c15ull;
uint64_t next() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state >> 33; }

#define REQUIRE(c) do { if (!(c)) { std::printf("match_batch_asan: FAILED %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

void check(const match_slicing::Shape &s, const std::vector<int64_t> &seg, const std::vector<int32_t> &pairs, int n_cu)
{
    const int64_t P = (int64_t)pairs.size() / 2;
    const match_batch::Plan pl = match_batch::plan(s, seg.data(), pairs.data(), P, n_cu);
    REQUIRE((int64_t)pl.row0.size() == P + 1 && (int64_t)pl.slices.size() == P);
    std::vector<int64_t> covered((size_t)P, 0);
    for (const match_batch::Launch &l : pl.launches) {
        int64_t wg = 0, mwg = 0, parts = 0, rows = 0, qblocks = 0;
        REQUIRE(l.n >= 1 && l.e0 >= 0 && l.e0 + l.n <= (int64_t)pl.entries.size());
        for (int64_t k = l.e0; k < l.e0 + l.n; k++) {
            const match_batch::Entry &e = pl.entries[(size_t)k];
            const int64_t tiles = (e.nt + s.tile - 1) / s.tile;
            REQUIRE(e.nq >= 1 && e.nt >= 1 && e.slices >= 1 && e.tiles_per_slice >= 1);
            REQUIRE((int64_t)(e.slices - 1) * e.tiles_per_slice < tiles && (int64_t)e.slices * e.tiles_per_slice >= tiles);
            REQUIRE(e.wg0 == wg && e.mwg0 == mwg && e.part0 == parts);
            REQUIRE(e.qblocks == (e.nq + s.qblock - 1) / s.qblock);
            const int32_t a = pairs[2 * (size_t)e.pair], b = pairs[2 * (size_t)e.pair + 1];
            REQUIRE(e.t0 == seg[(size_t)b] && e.nt == seg[(size_t)b + 1] - seg[(size_t)b]);
            REQUIRE(e.q0 >= seg[(size_t)a] && e.q0 + e.nq <= seg[(size_t)a + 1]);
            REQUIRE(e.out0 - pl.row0[(size_t)e.pair] == e.q0 - seg[(size_t)a]);
            wg += (int64_t)e.qblocks * e.slices;
            if (e.slices > 1) { mwg += (e.nq + 255) / 256; parts += (int64_t)e.slices * e.nq; }
            rows += e.nq;
            qblocks += e.qblocks;
            covered[(size_t)e.pair] += e.nq;
        }
        REQUIRE(wg == l.wgs && mwg == l.merge_wgs && parts == l.parts && rows == l.rows && qblocks == l.qblocks);
        REQUIRE(l.rows <= match_batch::kLaunchRows && l.parts <= pl.max_parts && l.wgs < ((int64_t)1 << 31));
    }
    int64_t first = 0;
    for (const match_batch::Fill &f : pl.fills) {
        REQUIRE(f.first == first && f.n >= 1 && f.out0 == pl.row0[(size_t)f.pair]);
        covered[(size_t)f.pair] += f.n;
        first += f.n;
    }
    REQUIRE(first == pl.fill_rows);
    for (int64_t p = 0; p < P; p++) REQUIRE(covered[(size_t)p] == pl.row0[(size_t)p + 1] - pl.row0[(size_t)p]);
}
}  // namespace

int main()
{
    const int64_t sizes[] = {0, 1, 15, 16, 17, 127, 128, 129, 257, 5000};
    const int cus[] = {1, 64, 256, 304};
    int plans = 0;
    for (int set = 0; set < 12; set++) {
        const int n_img = 2 + (int)(next() % 14);
        std::vector<int64_t> seg(1, 0);
        for (int i = 0; i < n_img; i++) seg.push_back(seg.back() + ((next() & 1) ? sizes[next() % 10] : (int64_t)(next() % 3000)));
        if (set % 4 == 3) seg.push_back(seg.back() + match_batch::kLaunchRows + 77);      // one image that a launch cannot hold
        if (seg.back() == 0) seg.push_back(1);
        const int n = (int)seg.size() - 1;
        const int64_t P = set == 0 ? 1 : 1 + (int64_t)(next() % 2000);
        std::vector<int32_t> pairs;
        for (int64_t p = 0; p < P; p++) { pairs.push_back((int32_t)(next() % n)); pairs.push_back((int32_t)(next() % n)); }
        if (set % 4 == 3) { pairs[0] = n - 1; pairs[1] = 0; }
        for (int n_cu : cus) {
            check(match_slicing::kFloat, seg, pairs, n_cu);
            check(match_slicing::kU8, seg, pairs, n_cu);
            plans += 2;
        }
    }
    std::printf("match_batch_asan: ok (%d plans)\n", plans);
    return 0;
}
