// match — nearest-neighbour matching of two descriptor tables, over libdlco.so.
//
//     match query_desc_file train_desc_file -out dst [-u8] [-ratio f] [-cross] [-device n]
//           [-guided verify_out -kp query_kp_file train_kp_file [-radius f]] [-model homography|fundamental]
//
// Both inputs hold the dataset "Descriptor" [n, r] f32 that `describe` writes (the two r must agree).  Writes
//     "Nearest" [nq,2] i32 and "NearestSqDist" [nq,2] f32   the library's answer for every query (dlco_desc_match)
//     "Matches" [m,2] i32 = (query, train), ascending in query, and "MatchSqDist" [m] f32   the filtered list
// The filters are the library's too: the answer is a batch answer of one pair, and dlco_desc_select_pairs turns it into the
// list (include/dlco.h states the rule).  -ratio f (0 < f <= 1) is Lowe's test d1 < f^2 d2 on the squared distances, -cross
// keeps (i, j) iff the nearest query of train row j is i (a second match call with the tables swapped gives the reverse
// answer).  Both may be given; without either every query with a neighbour is a match.  The select call takes fewer than
// 2^31 query rows, and so does this tool.  The reference has no such tool.
//   With -u8 both inputs hold "DescriptorU8" [n, r] u8 (`quantize`, `describe -quant`) instead, the library calls are
// dlco_desc_match_u8 and dlco_desc_select_pairs_u8, and "NearestSqDist" / "MatchSqDist" are i32: exact integer distances.  If
// both files carry a quantiser ("QuantScale", "QuantOffset") and the two differ in any bit the tool refuses: distances between
// differently quantised tables mean nothing.
//   With -guided the library call is dlco_desc_match_guided: every query is matched among the train keypoints that the
// homography of a `verify` output ("HomographyBits", query image -> train image) puts within -radius pixels (default 6) of
// it.  The two -kp files hold "Keypoints" [n,4] f32 as `detect` writes them, row for row the keypoints of the two descriptor
// tables (a row count that differs is an error, and so is a verify output without a model, "BestHypothesis" = -1).  -cross
// makes its second call with the tables swapped and h_side = 1, which sees the transpose of the same admissible set; -ratio
// and -cross are the same select call on the guided answer (a query with no admitted row is no match).  There is no guided
// form of -u8.
//   -model fundamental (with -guided only; the default is homography) guides by the fundamental matrix of a
// `verify -model fundamental` output instead ("FundamentalBits", src = the query image): the library call is
// dlco_desc_match_guided_epipolar with -radius as its threshold, the Sampson error in pixels, and f_side = 1 for -cross.
// A path that does not end in .h5/.hdf5 is a directory of .npy files with the same dataset names (dlco_io.hpp).
#include "match_tool.hpp"
#include "quant_io.hpp"

#include <chrono>
#include <cstdlib>

using std::cout;
using std::endl;
using match_tool::Line;

namespace {
struct Options {
    int device = 0;
    bool cross = false, use_ratio = false, fundamental = false;
    float ratio = 1.0f, radius = 6.0f;
    const char *qf = nullptr, *tf = nullptr, *out = nullptr, *guided = nullptr, *qkp = nullptr, *tkp = nullptr;
};

// H [9] of a verify output, the dataset `name` of it ("HomographyBits", "FundamentalBits"); refuses one without a model
void load_model(const char *path, const char *name, double H[9])
{
    std::vector<size_t> shape;
    std::vector<int32_t> best;
    std::vector<int64_t> bits;
    dlco_io::read_dataset<int32_t>(path, "BestHypothesis", shape, best);
    if (best.size() != 1) throw std::runtime_error(std::string(path) + ": BestHypothesis must hold one value");
    if (best[0] < 0) throw std::runtime_error(std::string(path) + ": the verification found no model (BestHypothesis = -1): nothing to guide by");
    dlco_io::read_dataset<int64_t>(path, name, shape, bits);
    if (bits.size() != 9) throw std::runtime_error(std::string(path) + ": " + name + " must hold nine values");
    std::memcpy(H, bits.data(), 9 * sizeof(double));
}

// the tool on one line: T = float, or uint8_t for -u8
template <typename T> void run(const Options &o, dlco_desc_ctx *&ctx)
{
    using Dist = typename Line<T>::Dist;
    std::vector<size_t> qs, ts;
    std::vector<T> Q, Tr;
    match_tool::load_table<T>(o.qf, false, qs, Q);
    match_tool::load_table<T>(o.tf, false, ts, Tr);
    if (qs[1] != ts[1])
        throw std::runtime_error("the descriptors differ in size: " + std::to_string(qs[1]) + " (query) against " + std::to_string(ts[1]) + " (train)");
    const size_t nq = qs[0], nt = ts[0], r = qs[1];
    if constexpr (std::is_same<T, uint8_t>::value) {
        float sq = 0.f, st = 0.f;
        std::vector<float> oq, ot;
        if (quant_io::present(o.qf, r, sq, oq) && quant_io::present(o.tf, r, st, ot) && !quant_io::same_bits(sq, oq, st, ot))
            throw std::runtime_error("the two tables were quantised differently (QuantScale / QuantOffset differ): their distances mean nothing");
    }
    printf("Queries: %zu x %zu%s\n", nq, r, Line<T>::tag);
    printf("Train: %zu x %zu%s\n", nt, r, Line<T>::tag);
    double H[9] = {0};
    std::vector<float> qxy, txy;
    if (o.guided) {
        qxy.resize(2 * nq);
        txy.resize(2 * nt);
        load_model(o.guided, o.fundamental ? "FundamentalBits" : "HomographyBits", H);
        match_tool::load_xy(o.qkp, nq, o.qf, qxy.data());
        match_tool::load_xy(o.tkp, nt, o.tf, txy.data());
        match_tool::print_guided(o.fundamental, o.radius);
    }

    if (dlco_desc_create(&ctx, 1.4f, 8, 1, o.device) != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(nullptr));
    const auto t0 = std::chrono::steady_clock::now();
    // one direction: `side` 0 is query against train, 1 (-cross) the tables swapped; the two guided calls take the same
    // arguments, the model [9] kept, the radius or threshold, the side: side 1 sees the transpose of the same admissible set
    const auto guided_call = o.fundamental ? Line<T>::guided_epipolar : Line<T>::guided;
    auto match = [&](int side, std::vector<int32_t> &idx, std::vector<Dist> &d) {
        const T *a = side ? Tr.data() : Q.data(), *b = side ? Q.data() : Tr.data();
        const float *axy = side ? txy.data() : qxy.data(), *bxy = side ? qxy.data() : txy.data();
        const int64_t na = (int64_t)(side ? nt : nq), nb = (int64_t)(side ? nq : nt);
        idx.resize((size_t)na * 2);
        d.resize((size_t)na * 2);
        const int rc = o.guided ? guided_call(ctx, a, axy, na, b, bxy, nb, (int32_t)r, H, o.radius, side, idx.data(), d.data())
                                : Line<T>::match(ctx, a, na, b, nb, (int32_t)r, idx.data(), d.data());
        if (rc != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(ctx));
    };
    std::vector<int32_t> nearest, back, pairs;
    std::vector<Dist> sqdist, back_d, dists;
    match(0, nearest, sqdist);
    if (o.cross) match(1, back, back_d);
    // the answer as a batch answer of one pair, image 0 the queries and image 1 the train rows
    const int32_t pair[2] = {0, 1};
    std::vector<int64_t> moff;
    match_tool::select<T>(ctx, {0, (int64_t)nq, (int64_t)(nq + nt)}, pair, 1, nq, nearest.data(), sqdist.data(), o.use_ratio ? o.ratio : 0.0f,
                          o.cross ? back.data() : nullptr, {0}, (int64_t)nt, moff, pairs, dists);
    {
        dlco_io::Writer wr(o.out);
        wr.write<int32_t>("Nearest", nearest.data(), nq, 2);
        wr.write<Dist>("NearestSqDist", sqdist.data(), nq, 2);
        wr.write<int32_t>("Matches", pairs.data(), dists.size(), 2);
        wr.write_vec<Dist>("MatchSqDist", dists.data(), dists.size());
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("Matches: %zu / %zu\n", dists.size(), nq);
    printf("Total: %.09f sec\n", sec);
}
}  // namespace

int main(int argc, char **argv)
{
    Options o;
    bool help = false, u8 = false;
    const char *model = nullptr;
    for (int i = 1; i < argc; i++) {
        if (argv[i][0] == '-') {
            const bool has_val = i + 1 < argc;
            if (std::strcmp(argv[i], "-help") == 0) { help = true; continue; }
            if (std::strcmp(argv[i], "-out") == 0 && has_val) { o.out = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-ratio") == 0 && has_val) { o.ratio = (float)atof(argv[++i]); o.use_ratio = true; continue; }
            if (std::strcmp(argv[i], "-cross") == 0) { o.cross = true; continue; }
            if (std::strcmp(argv[i], "-u8") == 0) { u8 = true; continue; }
            if (std::strcmp(argv[i], "-guided") == 0 && has_val) { o.guided = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-kp") == 0 && i + 2 < argc) { o.qkp = argv[++i]; o.tkp = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-model") == 0 && has_val) { model = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-radius") == 0 && has_val) { o.radius = (float)atof(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-device") == 0 && has_val) { o.device = atoi(argv[++i]); continue; }
            cout << "ERROR: Invalid " << argv[i] << " option." << endl;
            help = true;
        } else {
            if (!o.qf) { o.qf = argv[i]; continue; }
            if (!o.tf) { o.tf = argv[i]; continue; }
            help = true;
        }
    }
    if (!o.qf || !o.tf || !o.out) help = true;
    if (!match_tool::ratio_ok(o.use_ratio, o.ratio)) help = true;
    if (o.guided && u8) {
        cout << "ERROR: -guided has no -u8 form." << endl;
        help = true;
    }
    if ((o.guided != nullptr) != (o.qkp != nullptr)) {
        cout << "ERROR: -guided and -kp go together." << endl;
        help = true;
    }
    o.fundamental = model && std::strcmp(model, "fundamental") == 0;
    if (!match_tool::model_ok(model)) help = true;
    if (model && !o.guided) {
        cout << "ERROR: -model needs -guided." << endl;
        help = true;
    }
    if (!match_tool::radius_ok(o.radius)) help = true;
    if (help) {
        cout << endl;
        cout << "Usage: match query_desc_file train_desc_file -out dst_h5_filename [-u8] [-ratio f] [-cross] [-device n] "
                "[-guided verify_out -kp query_kp_file train_kp_file [-radius f]] [-model homography|fundamental]" << endl;
        cout << endl;
        return 1;
    }
    dlco_desc_ctx *ctx = nullptr;
    try {
        if (u8) run<uint8_t>(o, ctx);
        else run<float>(o, ctx);
        dlco_desc_destroy(ctx);
    } catch (const std::exception &e) {
        if (ctx) dlco_desc_destroy(ctx);
        std::fprintf(stderr, "match: %s\n", e.what());
        return 2;
    }
    return 0;
}
