// Sanitizer walk of the guided arguments of the batch planner (opencv-dlco_amd/csrc/match_batch.hpp): built with
// -fsanitize=address,undefined by tests/test_match_batch_guided_rules.py and run as a program.  Seeded sets of image sizes and
// pairs under shrunken limits (64 record rows, 256 query rows a launch) and under the library's; every plan is checked, and
// the index arithmetic of the record kernel (match_records_batch_kernel: a lane per record row, the entry by a search over
// the first record rows) and of the tile loop's batch prologue is replayed over every record row on buffers of exactly the
// size the host path allocates.  Pure host code.
#include "../../opencv-dlco_amd/csrc/match_batch.hpp"

#include <cstdio>
#include <cstdlib>

namespace {
uint64_t state = 0x2545f4914f6cdd1dull;
uint64_t next() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state >> 33; }

#define REQUIRE(c) do { if (!(c)) { std::printf("match_batch_guided_asan: FAILED %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

int64_t rows_walked = 0;

void check(const std::vector<int64_t> &seg, const std::vector<int32_t> &pairs, int n_cu, bool both, int side, int64_t rec_limit, int64_t launch_rows)
{
    const int64_t P = (int64_t)pairs.size() / 2, n_rows = seg.back();
    std::vector<uint8_t> none((size_t)P);
    for (auto &f : none) f = next() % 5 == 0;
    match_batch::Guide g;
    g.no_model = none.data(); g.both_sides = both; g.side = side;
    if (rec_limit > 0) g.rec_limit = rec_limit;
    if (launch_rows > 0) g.launch_rows = launch_rows;
    const match_batch::Plan pl = match_batch::plan(match_slicing::kFloat, seg.data(), pairs.data(), P, n_cu, &g);
    REQUIRE(pl.guide.size() == pl.entries.size());
    std::vector<int64_t> covered((size_t)P, 0);
    std::vector<uint8_t> xy((size_t)n_rows, 1);                // a byte per row of the coordinate table: every read is checked
    std::vector<uint8_t> rec((size_t)pl.max_rec_rows);         // a byte per record row of the shared buffer
    for (const match_batch::Launch &l : pl.launches) {
        REQUIRE(l.n >= 1 && l.rows <= g.launch_rows && l.rec_rows <= pl.max_rec_rows && (l.rec_rows <= g.rec_limit || l.n == 1));
        const match_batch::Entry *ent = pl.entries.data() + l.e0;
        const match_batch::GuideOff *off = pl.guide.data() + l.e0;
        int64_t recs = 0;
        for (int64_t k = 0; k < l.n; k++) {
            REQUIRE(!none[(size_t)ent[k].pair] && ent[k].nt >= 1 && ent[k].nq >= 1);
            REQUIRE(off[k].rec0 == recs);
            REQUIRE(off[k].nqrec == ((both || side == 0) ? ent[k].nq : 0) && off[k].ntrec == ((both || side != 0) ? ent[k].nt : 0));
            recs += (int64_t)off[k].nqrec + off[k].ntrec;
            covered[(size_t)ent[k].pair] += ent[k].nq;
        }
        REQUIRE(recs == l.rec_rows && recs >= 1);
        // the record kernel, lane i
        for (auto &b : rec) b = 0;
        for (int64_t i = 0; i < l.rec_rows; i++) {
            int lo = 0, hi = (int)l.n;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (off[mid].rec0 <= i) lo = mid; else hi = mid;
            }
            const int64_t k = i - off[lo].rec0;
            REQUIRE(k >= 0 && k < (int64_t)off[lo].nqrec + off[lo].ntrec);
            const bool is_query = k < off[lo].nqrec;
            const int64_t row = is_query ? ent[lo].q0 + k : ent[lo].t0 + (k - off[lo].nqrec);
            const int32_t a = pairs[2 * (size_t)ent[lo].pair], b = pairs[2 * (size_t)ent[lo].pair + 1];
            REQUIRE(ent[lo].pair >= 0 && ent[lo].pair < P);
            REQUIRE(is_query ? (row >= seg[(size_t)a] && row < seg[(size_t)a + 1]) : (row >= seg[(size_t)b] && row < seg[(size_t)b + 1]));
            REQUIRE(xy[(size_t)row] == 1);
            rec[(size_t)i] += 1;
            rows_walked++;
        }
        for (int64_t i = 0; i < l.rec_rows; i++) REQUIRE(rec[(size_t)i] == 1);
        // the tile loop's prologue: the rows of the records and of the coordinates an entry reads
        for (int64_t k = 0; k < l.n; k++) {
            const int64_t qr = off[k].rec0, tr = qr + off[k].nqrec;
            if (off[k].nqrec) REQUIRE(rec[(size_t)qr] == 1 && rec[(size_t)(qr + ent[k].nq - 1)] == 1);
            if (off[k].ntrec) REQUIRE(rec[(size_t)tr] == 1 && rec[(size_t)(tr + ent[k].nt - 1)] == 1);
            if (!both) {
                const int64_t x0 = side == 0 ? ent[k].t0 : ent[k].q0, n = side == 0 ? ent[k].nt : ent[k].nq;
                REQUIRE(xy[(size_t)x0] == 1 && xy[(size_t)(x0 + n - 1)] == 1);
            }
        }
    }
    for (const match_batch::Fill &f : pl.fills) covered[(size_t)f.pair] += f.n;
    for (int64_t p = 0; p < P; p++) {
        REQUIRE(covered[(size_t)p] == pl.row0[(size_t)p + 1] - pl.row0[(size_t)p]);
        const int64_t nt = seg[(size_t)pairs[2 * (size_t)p + 1] + 1] - seg[(size_t)pairs[2 * (size_t)p + 1]];
        bool filled = false;
        for (const match_batch::Fill &f : pl.fills) filled = filled || f.pair == p;
        REQUIRE(filled == (pl.row0[(size_t)p + 1] > pl.row0[(size_t)p] && (nt == 0 || none[(size_t)p])));
    }
}
}  // namespace

int main()
{
    const int64_t sizes[] = {0, 1, 15, 16, 17, 127, 128, 129, 257, 700};
    int plans = 0;
    for (int set = 0; set < 40; set++) {
        const int n_img = 2 + (int)(next() % 8);
        std::vector<int64_t> seg(1, 0);
        for (int i = 0; i < n_img; i++) seg.push_back(seg.back() + ((next() & 1) ? sizes[next() % 10] : (int64_t)(next() % 400)));
        if (seg.back() == 0) seg.push_back(1);
        const int n = (int)seg.size() - 1;
        const int64_t P = set == 0 ? 1 : 1 + (int64_t)(next() % 60);
        std::vector<int32_t> pairs;
        for (int64_t p = 0; p < P; p++) { pairs.push_back((int32_t)(next() % n)); pairs.push_back((int32_t)(next() % n)); }
        for (int form = 0; form < 3; form++) {             // the homography of side 0, of side 1, the fundamental matrix
            check(seg, pairs, 256, form == 2, form == 1, 64, 256);
            check(seg, pairs, 8, form == 2, form == 1, 1000, 300);
            check(seg, pairs, 256, form == 2, form == 1, 0, 0);
            plans += 3;
        }
    }
    std::printf("match_batch_guided_asan: ok (%d plans, %lld record rows)\n", plans, (long long)rows_walked);
    return 0;
}
