// Sanitizer walk of the host rule of dlco_desc_build_tracks* (opencv-dlco_amd/csrc/track_rules.hpp): built with
// -fsanitize=address,undefined by tests/test_track_rules.py and run as a program.  With a file name it reads the cases that the
// test wrote, inputs and the answers of the Python reference (the synthetic set at every setting, stray indices, chain, star,
// cycle, empty batches), as a stream of int64, runs track_rules::tracks_host and the hook step in reversed order on each and
// compares.  Then, and without a file only, seeded sets of its own against a plain relabelling loop.  Every buffer has its
// exact size, so a read or write outside a list is the sanitizer's to find.  Pure host code.
#include "../../opencv-dlco_amd/csrc/track_rules.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>

namespace tr = track_rules;

namespace {
uint64_t state = 0x9e3779b97f4a7c15ull;
uint64_t next() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state >> 33; }

#define REQUIRE(c) do { if (!(c)) { std::printf("track_rules_asan: FAILED %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

struct Case {
    std::vector<int64_t> seg, moff;
    std::vector<int32_t> pairs, matches;
    std::vector<uint8_t> keep;
    bool has_keep = false;
    int32_t min_len = 2, unique = 1;
};

struct Answer {
    int64_t n_tracks = 0;
    std::vector<int64_t> toff, counts;
    std::vector<int32_t> obs, track_of, label;
};

// the call on buffers of exactly the sizes the rule promises to stay inside: toff [n_tracks + 1], obs [toff[n_tracks]]
Answer run(const Case &c, const Answer *sized_by)
{
    const int32_t n_img = (int32_t)c.seg.size() - 1;
    const int64_t N = c.seg.back(), P = (int64_t)c.pairs.size() / 2;
    Answer a;
    a.toff.assign(sized_by ? sized_by->toff.size() : (size_t)N / 2 + 1, -7);
    a.obs.assign(sized_by ? sized_by->obs.size() : (size_t)N, -7);
    a.track_of.assign((size_t)N, -7);
    a.label.assign((size_t)N, -7);
    a.counts.assign(3, -7);
    a.n_tracks = tr::tracks_host(c.seg.data(), n_img, c.pairs.data(), P, c.moff.data(), c.matches.data(), c.has_keep ? c.keep.data() : nullptr, c.min_len,
                                 c.unique, a.toff.data(), a.obs.data(), a.track_of.data(), a.label.data(), a.counts.data());
    return a;
}

// labels by relabelling until nothing changes: no union-find
std::vector<int32_t> plain_labels(const Case &c)
{
    const int64_t N = c.seg.back(), P = (int64_t)c.pairs.size() / 2;
    std::vector<int32_t> label((size_t)N);
    for (int64_t g = 0; g < N; g++) label[(size_t)g] = (int32_t)g;
    for (bool changed = true; changed;) {
        changed = false;
        for (int64_t p = 0; p < P; p++) {
            const int32_t a = c.pairs[2 * (size_t)p], b = c.pairs[2 * (size_t)p + 1];
            const int64_t na = c.seg[(size_t)a + 1] - c.seg[(size_t)a], nb = c.seg[(size_t)b + 1] - c.seg[(size_t)b];
            for (int64_t m = c.moff[(size_t)p]; m < c.moff[(size_t)p + 1]; m++) {
                const int64_t i = c.matches[2 * (size_t)m], j = c.matches[2 * (size_t)m + 1];
                if ((c.has_keep && !c.keep[(size_t)m]) || i < 0 || i >= na || j < 0 || j >= nb) continue;
                int32_t &x = label[(size_t)(c.seg[(size_t)a] + i)], &y = label[(size_t)(c.seg[(size_t)b] + j)];
                if (x != y) { x = y = x < y ? x : y; changed = true; }
            }
        }
    }
    return label;
}

void check_against_plain(const Case &c)
{
    const int32_t n_img = (int32_t)c.seg.size() - 1;
    const int64_t N = c.seg.back(), M = c.moff.back(), P = (int64_t)c.pairs.size() / 2;
    const std::vector<int32_t> want = plain_labels(c);
    const Answer a = run(c, nullptr);
    REQUIRE(a.label == want);
    // the hook step in reversed order gives the same labels
    std::vector<int64_t> order((size_t)M);
    for (int64_t k = 0; k < M; k++) order[(size_t)k] = M - 1 - k;
    std::vector<int32_t> rev((size_t)N, -7);
    tr::labels_host(c.seg.data(), n_img, c.pairs.data(), P, c.moff.data(), c.matches.data(), c.has_keep ? c.keep.data() : nullptr, order.data(), rev.data());
    REQUIRE(rev == want);
    // the outputs follow from the labels
    std::vector<int64_t> size((size_t)N, 0);
    for (int64_t g = 0; g < N; g++) size[(size_t)want[(size_t)g]]++;
    int64_t T = 0, K = 0, c0 = 0, c1 = 0, c2 = 0;
    for (int64_t l = 0; l < N; l++) {
        if (size[(size_t)l] < 2) continue;
        c0++;
        bool conflict = false;
        int32_t last = -1;
        for (int64_t g = 0; g < N; g++)
            if (want[(size_t)g] == l) { const int32_t im = tr::image_of(c.seg.data(), n_img, g); conflict |= im == last; last = im; }
        if (size[(size_t)l] < c.min_len) { c1++; continue; }
        if (c.unique && conflict) { c2++; continue; }
        REQUIRE(a.toff[(size_t)T] == K);
        for (int64_t g = 0; g < N; g++)
            if (want[(size_t)g] == l) { REQUIRE(a.obs[(size_t)K] == g && a.track_of[(size_t)g] == T); K++; }
        T++;
    }
    REQUIRE(a.n_tracks == T && a.toff[(size_t)T] == K && a.counts[0] == c0 && a.counts[1] == c1 && a.counts[2] == c2);
    for (size_t t = (size_t)T + 1; t < a.toff.size(); t++) REQUIRE(a.toff[t] == -7);
    for (size_t k = (size_t)K; k < a.obs.size(); k++) REQUIRE(a.obs[k] == -7);
    int64_t loose = 0;
    for (int64_t g = 0; g < N; g++) loose += a.track_of[(size_t)g] == -1;
    REQUIRE(loose == N - K);
    // and again on buffers of exactly T + 1 and K entries
    Answer exact;
    exact.toff.resize((size_t)T + 1);
    exact.obs.resize((size_t)K);
    const Answer b = run(c, &exact);
    REQUIRE(b.n_tracks == T && b.track_of == a.track_of);
}

int64_t read_i64(std::FILE *f)
{
    int64_t v = 0;
    REQUIRE(std::fread(&v, sizeof v, 1, f) == 1);
    return v;
}
template <typename T>
void read_vec(std::FILE *f, std::vector<T> &v, int64_t n)
{
    v.resize((size_t)n);
    for (int64_t k = 0; k < n; k++) v[(size_t)k] = (T)read_i64(f);
}

int from_file(const char *path)
{
    std::FILE *f = std::fopen(path, "rb");
    REQUIRE(f != nullptr);
    const int64_t n_cases = read_i64(f);
    for (int64_t k = 0; k < n_cases; k++) {
        Case c;
        Answer want;
        const int64_t n_img = read_i64(f);
        read_vec(f, c.seg, n_img + 1);
        const int64_t P = read_i64(f);
        read_vec(f, c.pairs, 2 * P);
        read_vec(f, c.moff, P + 1);
        const int64_t M = c.moff.back(), N = c.seg.back();
        read_vec(f, c.matches, 2 * M);
        c.has_keep = read_i64(f) != 0;
        if (c.has_keep) read_vec(f, c.keep, M);
        c.min_len = (int32_t)read_i64(f);
        c.unique = (int32_t)read_i64(f);
        want.n_tracks = read_i64(f);
        read_vec(f, want.toff, want.n_tracks + 1);
        read_vec(f, want.obs, want.toff.back());
        read_vec(f, want.track_of, N);
        read_vec(f, want.label, N);
        read_vec(f, want.counts, 3);
        REQUIRE(tr::moff_ok(c.moff.data(), P) && tr::settings_ok(c.min_len, c.unique));
        const Answer got = run(c, &want);
        REQUIRE(got.n_tracks == want.n_tracks && got.toff == want.toff && got.obs == want.obs && got.track_of == want.track_of && got.label == want.label &&
                got.counts == want.counts);
        if (N <= 2000) check_against_plain(c);
    }
    std::fclose(f);
    return (int)n_cases;
}

int seeded()
{
    int runs = 0;
    const int64_t some[] = {0, 1, 2, 63, 64, 65, 100};
    for (int set = 0; set < 40; set++) {
        Case c;
        const int n_img = 1 + (int)(next() % 8);
        c.seg.assign(1, 0);
        for (int i = 0; i < n_img; i++) c.seg.push_back(c.seg.back() + ((set % 7 == 0) ? 0 : some[next() % 7]));
        const int64_t P = 1 + (int64_t)(next() % 30);
        c.moff.assign(1, 0);
        for (int64_t p = 0; p < P; p++) {
            const int32_t a = (int32_t)(next() % (uint64_t)n_img), b = (int32_t)(next() % (uint64_t)n_img);
            c.pairs.push_back(a);
            c.pairs.push_back(b);
            const int64_t na = c.seg[(size_t)a + 1] - c.seg[(size_t)a], nb = c.seg[(size_t)b + 1] - c.seg[(size_t)b];
            const int64_t m = (next() % 4 == 0) ? 0 : (int64_t)(next() % 12);
            for (int64_t k = 0; k < m; k++) {
                const uint64_t kind = next() % 12;
                const int32_t stray[] = {-1, INT32_MAX, INT32_MIN, (int32_t)na, (int32_t)nb, -2};
                c.matches.push_back(kind == 0 || na == 0 ? stray[next() % 6] : (int32_t)(next() % (uint64_t)na));
                c.matches.push_back(kind == 1 || nb == 0 ? stray[next() % 6] : (int32_t)(next() % (uint64_t)nb));
                c.keep.push_back((uint8_t)(next() % 5 != 0 ? 1 + next() % 255 : 0));
            }
            c.moff.push_back((int64_t)c.matches.size() / 2);
        }
        for (int k = 0; k < 8; k++) {
            c.has_keep = (k & 1) != 0;
            c.unique = (k & 2) ? 1 : 0;
            c.min_len = (k & 4) ? 3 : 2;
            check_against_plain(c);
            runs++;
        }
    }
    return runs;
}
}  // namespace

int main(int argc, char **argv)
{
    const int from = argc > 1 ? from_file(argv[1]) : 0;
    const int own = seeded();
    std::printf("track_rules_asan: ok (%d cases of the file, %d runs of seeded sets)\n", from, own);
    return 0;
}
