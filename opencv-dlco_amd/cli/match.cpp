// match — nearest-neighbour matching of two descriptor tables, over libdlco.so.
//
//     match query_desc_file train_desc_file -out dst [-u8] [-ratio f] [-cross] [-device n]
//           [-guided verify_out -kp query_kp_file train_kp_file [-radius f]] [-model homography|fundamental]
//
// Both inputs hold the dataset "Descriptor" [n, r] f32 that `describe` writes (the two r must agree).  Writes
//     "Nearest" [nq,2] i32 and "NearestSqDist" [nq,2] f32   the library's answer for every query (dlco_desc_match)
//     "Matches" [m,2] i32 = (query, train), ascending in query, and "MatchSqDist" [m] f32   the filtered list
// The filters are host rules (match_rules.hpp): -ratio f (0 < f <= 1) is Lowe's test d1 < f^2 d2 on the squared
// distances, -cross keeps (i, j) iff the nearest query of train row j is i (a second library call with the tables
// swapped).  Both may be given; without either every query with a neighbour is a match.  The reference has no such tool.
//   With -u8 both inputs hold "DescriptorU8" [n, r] u8 (`quantize`, `describe -quant`) instead, the library call is
// dlco_desc_match_u8, and "NearestSqDist" / "MatchSqDist" are i32: exact integer distances.  If both files carry a quantiser
// ("QuantScale", "QuantOffset") and the two differ in any bit the tool refuses: distances between differently quantised
// tables mean nothing.
//   With -guided the library call is dlco_desc_match_guided: every query is matched among the train keypoints that the
// homography of a `verify` output ("HomographyBits", query image -> train image) puts within -radius pixels (default 6) of
// it.  The two -kp files hold "Keypoints" [n,4] f32 as `detect` writes them, row for row the keypoints of the two descriptor
// tables (a row count that differs is an error, and so is a verify output without a model, "BestHypothesis" = -1).  -cross
// makes its second call with the tables swapped and h_side = 1, which sees the transpose of the same admissible set; -ratio
// and -cross are the same host rules on the guided answer (a query with no admitted row is no match).  There is no guided
// form of -u8.
//   -model fundamental (with -guided only; the default is homography) guides by the fundamental matrix of a
// `verify -model fundamental` output instead ("FundamentalBits", src = the query image): the library call is
// dlco_desc_match_guided_epipolar with -radius as its threshold, the Sampson error in pixels, and f_side = 1 for -cross.
// A path that does not end in .h5/.hdf5 is a directory of .npy files with the same dataset names (dlco_io.hpp).
#include "../../include/dlco.h"
#include "dlco_io.hpp"
#include "match_rules.hpp"
#include "quant_io.hpp"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>

using std::cout;
using std::endl;

namespace {
void load_table(const char *path, std::vector<size_t> &shape, std::vector<float> &rows)
{
    dlco_io::read_dataset<float>(path, "Descriptor", shape, rows);
    if (shape.size() != 2 || shape[0] < 1 || shape[1] < 1) throw std::runtime_error(std::string(path) + ": Descriptor must be a non-empty [n, r] table");
    for (float v : rows)
        if (!(v == v) || v > 3.0e38f || v < -3.0e38f) throw std::runtime_error(std::string(path) + ": Descriptor contains NaN");
}

void load_table_u8(const char *path, std::vector<size_t> &shape, std::vector<uint8_t> &rows)
{
    dlco_io::read_dataset<uint8_t>(path, "DescriptorU8", shape, rows);
    if (shape.size() != 2 || shape[0] < 1 || shape[1] < 1) throw std::runtime_error(std::string(path) + ": DescriptorU8 must be a non-empty [n, r] table");
}

// the (x, y) of the "Keypoints" [n,4] of a detect output, which must have `rows` rows: those of its descriptor table
void load_xy(const char *path, size_t rows, const char *desc_path, std::vector<float> &xy)
{
    std::vector<size_t> shape;
    std::vector<float> kp;
    dlco_io::read_dataset<float>(path, "Keypoints", shape, kp);
    if (shape.size() != 2 || shape[1] != 4) throw std::runtime_error(std::string(path) + ": Keypoints must be an [n, 4] table");
    if (shape[0] != rows)
        throw std::runtime_error(std::string(path) + ": " + std::to_string(shape[0]) + " keypoints against " + std::to_string(rows) + " descriptors in " + desc_path);
    xy.resize(rows * 2);
    for (size_t i = 0; i < rows; i++) { xy[2 * i] = kp[4 * i]; xy[2 * i + 1] = kp[4 * i + 1]; }
}

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

// the -u8 line of main: the same steps on byte tables
void match_u8(const char *qf, const char *tf, const char *out, bool use_ratio, float ratio, bool cross, int device, dlco_desc_ctx *&ctx)
{
    std::vector<size_t> qs, ts;
    std::vector<uint8_t> Q, T;
    load_table_u8(qf, qs, Q);
    load_table_u8(tf, ts, T);
    if (qs[1] != ts[1])
        throw std::runtime_error("the descriptors differ in size: " + std::to_string(qs[1]) + " (query) against " + std::to_string(ts[1]) + " (train)");
    const size_t nq = qs[0], nt = ts[0], r = qs[1];
    float sq = 0.f, st = 0.f;
    std::vector<float> oq, ot;
    if (quant_io::present(qf, r, sq, oq) && quant_io::present(tf, r, st, ot) && !quant_io::same_bits(sq, oq, st, ot))
        throw std::runtime_error("the two tables were quantised differently (QuantScale / QuantOffset differ): their distances mean nothing");
    printf("Queries: %zu x %zu (u8)\n", nq, r);
    printf("Train: %zu x %zu (u8)\n", nt, r);

    if (dlco_desc_create(&ctx, 1.4f, 8, 1, device) != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(nullptr));
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> nearest(nq * 2), sqdist(nq * 2), back;
    if (dlco_desc_match_u8(ctx, Q.data(), (int64_t)nq, T.data(), (int64_t)nt, (int32_t)r, nearest.data(), sqdist.data()) != DLCO_OK)
        throw std::runtime_error(dlco_desc_last_error(ctx));
    if (cross) {
        back.resize(nt * 2);
        std::vector<int32_t> back_d(nt * 2);
        if (dlco_desc_match_u8(ctx, T.data(), (int64_t)nt, Q.data(), (int64_t)nq, (int32_t)r, back.data(), back_d.data()) != DLCO_OK)
            throw std::runtime_error(dlco_desc_last_error(ctx));
    }
    std::vector<int32_t> pairs, dists;
    match_rules::select((int64_t)nq, nearest.data(), sqdist.data(), use_ratio, ratio, cross ? back.data() : nullptr, pairs, dists);
    {
        dlco_io::Writer wr(out);
        wr.write<int32_t>("Nearest", nearest.data(), nq, 2);
        wr.write<int32_t>("NearestSqDist", sqdist.data(), nq, 2);
        wr.write<int32_t>("Matches", pairs.data(), dists.size(), 2);
        wr.write_vec<int32_t>("MatchSqDist", dists.data(), dists.size());
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("Matches: %zu / %zu\n", dists.size(), nq);
    printf("Total: %.09f sec\n", sec);
}
}  // namespace

int main(int argc, char **argv)
{
    int device = 0;
    bool help = false, cross = false, use_ratio = false, u8 = false;
    float ratio = 1.0f, radius = 6.0f;
    const char *qf = nullptr, *tf = nullptr, *out = nullptr, *guided = nullptr, *qkp = nullptr, *tkp = nullptr, *model = nullptr;
    for (int i = 1; i < argc; i++) {
        if (argv[i][0] == '-') {
            const bool has_val = i + 1 < argc;
            if (std::strcmp(argv[i], "-help") == 0) { help = true; continue; }
            if (std::strcmp(argv[i], "-out") == 0 && has_val) { out = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-ratio") == 0 && has_val) { ratio = (float)atof(argv[++i]); use_ratio = true; continue; }
            if (std::strcmp(argv[i], "-cross") == 0) { cross = true; continue; }
            if (std::strcmp(argv[i], "-u8") == 0) { u8 = true; continue; }
            if (std::strcmp(argv[i], "-guided") == 0 && has_val) { guided = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-kp") == 0 && i + 2 < argc) { qkp = argv[++i]; tkp = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-model") == 0 && has_val) { model = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-radius") == 0 && has_val) { radius = (float)atof(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-device") == 0 && has_val) { device = atoi(argv[++i]); continue; }
            cout << "ERROR: Invalid " << argv[i] << " option." << endl;
            help = true;
        } else {
            if (!qf) { qf = argv[i]; continue; }
            if (!tf) { tf = argv[i]; continue; }
            help = true;
        }
    }
    if (!qf || !tf || !out) help = true;
    if (use_ratio && !(ratio > 0.0f && ratio <= 1.0f)) {
        cout << "ERROR: -ratio must be in (0, 1]." << endl;
        help = true;
    }
    if (guided && u8) {
        cout << "ERROR: -guided has no -u8 form." << endl;
        help = true;
    }
    if ((guided != nullptr) != (qkp != nullptr)) {
        cout << "ERROR: -guided and -kp go together." << endl;
        help = true;
    }
    const bool fundamental = model && std::strcmp(model, "fundamental") == 0;
    if (model && !fundamental && std::strcmp(model, "homography") != 0) {
        cout << "ERROR: -model must be homography or fundamental." << endl;
        help = true;
    }
    if (model && !guided) {
        cout << "ERROR: -model needs -guided." << endl;
        help = true;
    }
    if (!(std::isfinite(radius) && radius > 0.0f)) {
        cout << "ERROR: -radius must be finite and > 0." << endl;
        help = true;
    }
    if (help) {
        cout << endl;
        cout << "Usage: match query_desc_file train_desc_file -out dst_h5_filename [-u8] [-ratio f] [-cross] [-device n] "
                "[-guided verify_out -kp query_kp_file train_kp_file [-radius f]] [-model homography|fundamental]" << endl;
        cout << endl;
        return 1;
    }
    dlco_desc_ctx *ctx = nullptr;
    try {
        if (u8) {
            match_u8(qf, tf, out, use_ratio, ratio, cross, device, ctx);
            dlco_desc_destroy(ctx);
            return 0;
        }
        std::vector<size_t> qs, ts;
        std::vector<float> Q, T;
        load_table(qf, qs, Q);
        load_table(tf, ts, T);
        if (qs[1] != ts[1])
            throw std::runtime_error("the descriptors differ in size: " + std::to_string(qs[1]) + " (query) against " + std::to_string(ts[1]) + " (train)");
        const size_t nq = qs[0], nt = ts[0], r = qs[1];
        printf("Queries: %zu x %zu\n", nq, r);
        printf("Train: %zu x %zu\n", nt, r);
        double H[9] = {0};
        std::vector<float> qxy, txy;
        if (guided) {
            load_model(guided, fundamental ? "FundamentalBits" : "HomographyBits", H);
            load_xy(qkp, nq, qf, qxy);
            load_xy(tkp, nt, tf, txy);
            if (fundamental) printf("Guided: fundamental, radius %g\n", radius);
            else printf("Guided: radius %g\n", radius);
        }

        if (dlco_desc_create(&ctx, 1.4f, 8, 1, device) != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(nullptr));
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<int32_t> nearest(nq * 2), back;
        std::vector<float> sqdist(nq * 2);
        // the two guided calls take the same arguments: the model [9], the radius or threshold, the side
        const auto guided_call = fundamental ? dlco_desc_match_guided_epipolar : dlco_desc_match_guided;
        const int rc = guided ? guided_call(ctx, Q.data(), qxy.data(), (int64_t)nq, T.data(), txy.data(), (int64_t)nt, (int32_t)r, H, radius, 0,
                                                       nearest.data(), sqdist.data())
                              : dlco_desc_match(ctx, Q.data(), (int64_t)nq, T.data(), (int64_t)nt, (int32_t)r, nearest.data(), sqdist.data());
        if (rc != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(ctx));
        if (cross) {
            back.resize(nt * 2);
            std::vector<float> back_d(nt * 2);
            // guided: the tables swapped and the model kept, side = 1: the transpose of the same admissible set
            const int rb = guided ? guided_call(ctx, T.data(), txy.data(), (int64_t)nt, Q.data(), qxy.data(), (int64_t)nq, (int32_t)r, H, radius, 1,
                                                           back.data(), back_d.data())
                                  : dlco_desc_match(ctx, T.data(), (int64_t)nt, Q.data(), (int64_t)nq, (int32_t)r, back.data(), back_d.data());
            if (rb != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(ctx));
        }
        std::vector<int32_t> pairs;
        std::vector<float> dists;
        match_rules::select((int64_t)nq, nearest.data(), sqdist.data(), use_ratio, ratio, cross ? back.data() : nullptr, pairs, dists);
        {
            dlco_io::Writer wr(out);
            wr.write<int32_t>("Nearest", nearest.data(), nq, 2);
            wr.write<float>("NearestSqDist", sqdist.data(), nq, 2);
            wr.write<int32_t>("Matches", pairs.data(), dists.size(), 2);
            wr.write_vec<float>("MatchSqDist", dists.data(), dists.size());
        }
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        printf("Matches: %zu / %zu\n", dists.size(), nq);
        printf("Total: %.09f sec\n", sec);
        dlco_desc_destroy(ctx);
    } catch (const std::exception &e) {
        if (ctx) dlco_desc_destroy(ctx);
        std::fprintf(stderr, "match: %s\n", e.what());
        return 2;
    }
    return 0;
}
