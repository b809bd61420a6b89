// Sanitizer walk of the batched verification's plan (opencv-dlco_amd/csrc/verify_batch.hpp) and of the refit loop through
// verify_rules::refit_step: built with -fsanitize=address,undefined by tests/test_verify_batch_rules.py and run as a
// program.  Seeded offset tables under the library's limits and under small ones; every plan is checked for the properties
// the kernels rely on, and the kernels' index arithmetic is replayed on the host over every workgroup of the small plans
// and of the plan of one pair, which is what a single call runs.
// Pure host code.
#include "../../opencv-dlco_amd/csrc/verify_batch.hpp"
#include "../../opencv-dlco_amd/csrc/epipolar_rules.hpp"

#include <cstdio>
#include <cstdlib>

namespace {
namespace vb = verify_batch;

uint64_t state = 0x9e3779b97f4a7c15ull;
uint64_t next() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state >> 33; }

#define REQUIRE(c) do { if (!(c)) { std::printf("verify_batch_asan: FAILED %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

// the kernels' search: the last item whose first workgroup is not above wg
template <typename Item, typename First>
int item_of(const Item *items, int n, int64_t wg, First first)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)first(items[mid]) <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

void check(const std::vector<int64_t> &moff, int32_t n_hyp, int k_sample, int64_t max_hyp, int64_t max_wgs, bool walk)
{
    const int64_t P = (int64_t)moff.size() - 1;
    REQUIRE(vb::offsets_ok(moff.data(), P));
    const vb::Plan pl = vb::plan(moff.data(), P, n_hyp, k_sample, max_hyp, max_wgs);
    REQUIRE((int64_t)pl.launch_of_pair.size() == P);
    const int64_t hb = vb::blocks(n_hyp);
    int64_t e_next = 0, p_next = 0;
    for (size_t k = 0; k < pl.launches.size(); k++) {
        const vb::Launch &l = pl.launches[k];
        REQUIRE(l.e0 == e_next && l.n >= 1 && l.e0 + l.n <= (int64_t)pl.entries.size());
        int64_t swg = 0, mwg = 0;
        for (int64_t j = 0; j < l.n; j++) {
            const vb::Entry &e = pl.entries[(size_t)(l.e0 + j)];
            REQUIRE(e.pair >= p_next && e.m >= k_sample && e.m == moff[(size_t)e.pair + 1] - moff[(size_t)e.pair]);
            for (int64_t p = p_next; p < e.pair; p++) REQUIRE(moff[(size_t)p + 1] - moff[(size_t)p] < k_sample && pl.launch_of_pair[(size_t)p] == -1);
            p_next = e.pair + 1;
            REQUIRE(pl.launch_of_pair[(size_t)e.pair] == (int32_t)k);
            REQUIRE(l.match0 + e.m0 == moff[(size_t)e.pair] && e.m0 >= 0 && e.m0 + e.m <= l.matches);
            REQUIRE(e.swg0 == swg && e.mwg0 == mwg);
            swg += hb * vb::blocks(e.m);
            mwg += vb::blocks(e.m);
        }
        REQUIRE(swg == l.score_wgs && mwg == l.mask_wgs && l.hyps == l.n * n_hyp);
        REQUIRE(l.hyps <= max_hyp && (l.score_wgs <= max_wgs || l.n == 1));
        REQUIRE(l.n <= pl.max_entries && l.matches <= pl.max_matches && l.hyps <= pl.max_hyps);
        e_next += l.n;
        if (!walk) continue;
        // every workgroup of the scoring grid lands in its entry on a (block, chunk) of it, every one once
        const vb::Entry *ent = pl.entries.data() + l.e0;
        std::vector<int> seen((size_t)l.score_wgs, 0);
        for (int64_t wg = 0; wg < l.score_wgs; wg++) {
            const int e = item_of(ent, (int)l.n, wg, [](const vb::Entry &x) { return x.swg0; });
            const int64_t w = wg - ent[e].swg0, chunk = w / hb, block = w - chunk * hb;
            REQUIRE(w >= 0 && chunk < vb::blocks(ent[e].m) && block < hb && chunk * vb::kLanes < ent[e].m);
            seen[(size_t)(ent[e].swg0 + chunk * hb + block)]++;
        }
        for (int s : seen) REQUIRE(s == 1);
        // the mask grid over every second entry, as a later round of the refit has it
        std::vector<vb::Active> act;
        int64_t wgs = 0;
        for (int64_t j = 0; j < l.n; j += 2) { act.push_back(vb::Active{(int32_t)j, (int32_t)wgs}); wgs += vb::blocks(ent[j].m); }
        int64_t covered = 0;
        for (int64_t wg = 0; wg < wgs; wg++) {
            const vb::Active a = act[(size_t)item_of(act.data(), (int)act.size(), wg, [](const vb::Active &x) { return x.wg0; })];
            const int64_t i0 = (wg - a.wg0) * vb::kLanes;
            REQUIRE(i0 >= 0 && i0 < ent[a.entry].m);
            covered += std::min<int64_t>(vb::kLanes, ent[a.entry].m - i0);
        }
        int64_t want = 0;
        for (const vb::Active &a : act) want += ent[a.entry].m;
        REQUIRE(covered == want);
    }
    REQUIRE(e_next == (int64_t)pl.entries.size());
    for (int64_t p = p_next; p < P; p++) REQUIRE(pl.launch_of_pair[(size_t)p] == -1);
}

// the plan a single call hands the batch path, n_pairs = 1 and moff = {0, m} under the library's limits: one launch of one
// entry that starts every range at 0, and the replay of the kernels' index arithmetic over it
void check_one_pair(int64_t m, int32_t n_hyp, int k_sample)
{
    const std::vector<int64_t> moff = {0, m};
    const vb::Plan pl = vb::plan(moff.data(), 1, n_hyp, k_sample);
    REQUIRE(pl.launches.size() == 1 && pl.entries.size() == 1 && pl.launch_of_pair[0] == 0);
    const vb::Entry &e = pl.entries[0];
    const vb::Launch &l = pl.launches[0];
    REQUIRE(e.m0 == 0 && e.m == m && e.pair == 0 && e.swg0 == 0 && e.mwg0 == 0);
    REQUIRE(l.e0 == 0 && l.n == 1 && l.match0 == 0 && l.matches == m && l.hyps == n_hyp);
    REQUIRE(l.score_wgs == vb::blocks(n_hyp) * vb::blocks(m) && l.mask_wgs == vb::blocks(m));
    REQUIRE(pl.max_entries == 1 && pl.max_matches == m && pl.max_hyps == n_hyp);
    check(moff, n_hyp, k_sample, vb::kLaunchHyp, vb::kLaunchWgs, true);
}

// the refit loop of both models on a small planted list: the loop and its step under the sanitizers
template <typename Model>
void refit(int64_t m)
{
    std::vector<float> src((size_t)m * 2), dst((size_t)m * 2);
    for (int64_t i = 0; i < m; i++) {
        const double x = (double)(next() % 4000), y = (double)(next() % 3000), z = 4.0 + (double)(next() % 400) / 100.0;
        src[2 * (size_t)i] = (float)x; src[2 * (size_t)i + 1] = (float)y;
        const bool out = i % 3 == 2;
        dst[2 * (size_t)i] = (float)(out ? (double)(next() % 4000) : x - 800.0 / z + (double)(next() % 100) / 100.0);
        dst[2 * (size_t)i + 1] = (float)(out ? (double)(next() % 3000) : y + (double)(next() % 100) / 100.0);
    }
    const int32_t n_hyp = 40, refine = 8;
    std::vector<double> M_all((size_t)n_hyp * 9), rounds((size_t)refine * 9);
    std::vector<int32_t> counts((size_t)n_hyp);
    std::vector<uint8_t> mask((size_t)m);
    double M[9];
    int64_t count = -1;
    int32_t best = -2, n_rounds = -1;
    verify_rules::verify_host<Model>(src.data(), dst.data(), m, 1.5f, n_hyp, 5, refine, M_all.data(), counts.data(), M, mask.data(), &count, &best,
                                     rounds.data(), &n_rounds);
    int64_t n = 0;
    for (uint8_t b : mask) n += b;
    REQUIRE(n == count && n_rounds >= 0 && n_rounds <= refine && best >= -1 && best < n_hyp);
}
}  // namespace

int main()
{
    const int64_t sizes[] = {0, 3, 4, 7, 8, 9, 255, 256, 257, 775};
    int plans = 0;
    for (int set = 0; set < 16; set++) {
        const int64_t P = set == 0 ? 1 : 1 + (int64_t)(next() % 600);
        std::vector<int64_t> moff(1, 0);
        for (int64_t p = 0; p < P; p++) moff.push_back(moff.back() + ((next() & 1) ? sizes[next() % 10] : (int64_t)(next() % 1500)));
        if (set == 1) std::fill(moff.begin(), moff.end(), 0);                // no match at all
        for (int fundamental = 0; fundamental < 2; fundamental++) {
            const int k = fundamental ? epipolar_rules::Fundamental::kSample : verify_rules::Homography::kSample;
            for (int32_t n_hyp : {1, 65, 256, 300}) {
                check(moff, n_hyp, k, vb::kLaunchHyp, vb::kLaunchWgs, false);
                check(moff, n_hyp, k, 4 * (int64_t)n_hyp, vb::kLaunchWgs, true);          // four entries a launch
                check(moff, n_hyp, k, n_hyp, vb::kLaunchWgs, true);                       // one
                check(moff, n_hyp, k, vb::kLaunchHyp, 7, true);                           // entries larger than the grid limit
                plans += 4;
            }
        }
    }
    for (int fundamental = 0; fundamental < 2; fundamental++) {
        const int k = fundamental ? epipolar_rules::Fundamental::kSample : verify_rules::Homography::kSample;
        for (int64_t m : {(int64_t)k, (int64_t)255, (int64_t)256, (int64_t)257})
            for (int32_t n_hyp : {1, 256, 257}) { check_one_pair(m, n_hyp, k); plans++; }
    }
    // offsets that must be refused
    const int64_t bad0[] = {1, 5}, bad1[] = {0, 5, 4}, bad2[] = {0, (int64_t)1 << 31};
    REQUIRE(!vb::offsets_ok(bad0, 1) && !vb::offsets_ok(bad1, 2) && !vb::offsets_ok(bad2, 1) && !vb::offsets_ok(nullptr, 1) && !vb::offsets_ok(bad1, 0));
    refit<verify_rules::Homography>(120);
    refit<epipolar_rules::Fundamental>(120);
    std::printf("verify_batch_asan: ok (%d plans)\n", plans);
    return 0;
}
