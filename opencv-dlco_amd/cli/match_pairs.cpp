// match-pairs — nearest-neighbour matching of many pairs of descriptor tables in one library call, over libdlco.so.
//
//     match-pairs -pairs pairs_file -out dst [-u8] [-ratio f] [-cross] [-device n] desc_file_0 desc_file_1 ...
//                 [-guided verify_pairs_out -kp kp_file_0 kp_file_1 ... [-radius f] [-model homography|fundamental]]
//
// Every desc_file holds the dataset "Descriptor" [n, r] f32 that `describe` writes (the r must agree; n may be 0: an image
// without keypoints), pairs_file the dataset "Pairs" [P, 2] i32 of (query file, train file), numbers in the file list.
// The tables are concatenated and matched by ONE dlco_desc_match_pairs call.  Writes
//     "Pairs" [P,2] i32 and "RowOffsets" [P+1] i64: pair p owns the rows RowOffsets[p] .. RowOffsets[p+1] - 1 of
//     "Nearest" [.,2] i32 and "NearestSqDist" [.,2] f32   the library's answer for the queries of every pair, which is what
//                                                          `match` writes for the pair's two files
//     "MatchOffsets" [P+1] i64: pair p owns the rows MatchOffsets[p] .. MatchOffsets[p+1] - 1 of
//     "Matches" [M,2] i32 = (query, train) as rows of the pair's own two tables, and "MatchSqDist" [M] f32   the filtered lists
// The filters are the library's, ONE dlco_desc_select_pairs call over the P pairs (include/dlco.h states the rule): -ratio f
// (0 < f <= 1) is Lowe's test, -cross the mutual check, for which the reversed pairs are appended to the same batch instead of
// making second calls.
//   With -u8 the files hold "DescriptorU8" [n, r] u8 instead, the calls are dlco_desc_match_pairs_u8 and
// dlco_desc_select_pairs_u8, and the distances are i32.  Files that carry a quantiser ("QuantScale", "QuantOffset") must all carry the same one, bit for bit.
//   With -guided the call is dlco_desc_match_pairs_guided: every pair is matched again under its own model of a `verify-pairs`
// output ("HomographyBits" [P,9], query image -> train image), among the train keypoints the model puts within -radius pixels
// (default 6) of the query.  The output's "Pairs" must be the -pairs list, row for row; a pair without a model (an all-zero
// matrix) is valid and gets -1 / +inf.  The files after -kp, up to the next option, hold "Keypoints" [n,4] f32 as `detect`
// writes them, one per descriptor file in the same order and row for row its keypoints.  -cross runs the reversed pairs as a
// second call with side 1 and the same matrices, as `match -guided -cross` does for one pair.  -model fundamental guides by
// "FundamentalBits" of a `verify-pairs -model fundamental` output (dlco_desc_match_pairs_guided_epipolar, -radius its
// threshold).  The datasets written are the same; per pair they are what `match -guided` writes.  There is no guided -u8.
// A path that does not end in .h5/.hdf5 is a directory of .npy files with the same dataset names (dlco_io.hpp).
#include "match_tool.hpp"
#include "quant_io.hpp"

#include <chrono>
#include <cstdlib>

using std::cout;
using std::endl;
using match_tool::Line;

namespace {
// -guided: the verify-pairs output, the keypoint files, the radius or threshold and the model
struct Guided {
    const char *verify_out = nullptr;
    std::vector<const char *> kp;
    float radius = 6.0f;
    bool fundamental = false;
};

template <typename T>
void run(const char *pairs_file, const std::vector<const char *> &files, const char *out, bool use_ratio, float ratio, bool cross, int device,
         dlco_desc_ctx *&ctx, const Guided *guided = nullptr)
{
    using Dist = typename Line<T>::Dist;
    const size_t n_img = files.size();
    std::vector<T> table;
    std::vector<int64_t> seg(n_img + 1, 0);
    size_t r = 0;
    for (size_t f = 0; f < n_img; f++) {
        std::vector<size_t> shape;
        std::vector<T> rows;
        match_tool::load_table<T>(files[f], true, shape, rows);
        if (f == 0) r = shape[1];
        if (shape[1] != r)
            throw std::runtime_error("the descriptors differ in size: " + std::to_string(r) + " (" + files[0] + ") against " + std::to_string(shape[1]) +
                                     " (" + files[f] + ")");
        seg[f + 1] = seg[f] + (int64_t)shape[0];
        table.insert(table.end(), rows.begin(), rows.end());
    }
    if (seg[n_img] < 1) throw std::runtime_error("every descriptor table is empty");
    if (std::is_same<T, uint8_t>::value) {              // match's rule across all files: the quantisers that are there agree
        float s0 = 0.f;
        std::vector<float> o0;
        const char *first = nullptr;
        for (size_t f = 0; f < n_img; f++) {
            float s = 0.f;
            std::vector<float> o;
            if (!quant_io::present(files[f], r, s, o)) continue;
            if (!first) { first = files[f]; s0 = s; o0 = o; continue; }
            if (!quant_io::same_bits(s0, o0, s, o))
                throw std::runtime_error(std::string(first) + " and " + files[f] +
                                         " were quantised differently (QuantScale / QuantOffset differ): their distances mean nothing");
        }
    }
    std::vector<size_t> pshape;
    std::vector<int32_t> pairs;
    dlco_io::read_dataset<int32_t>(pairs_file, "Pairs", pshape, pairs);
    if (pshape.size() != 2 || pshape[0] < 1 || pshape[1] != 2) throw std::runtime_error(std::string(pairs_file) + ": Pairs must be a non-empty [P, 2] table");
    const size_t P = pshape[0];
    for (size_t i = 0; i < 2 * P; i++)
        if (pairs[i] < 0 || (size_t)pairs[i] >= n_img)
            throw std::runtime_error(std::string(pairs_file) + ": pair " + std::to_string(i / 2) + " names file " + std::to_string(pairs[i]) + " of " +
                                     std::to_string(n_img));
    // -guided: the coordinates of every row, and the matrix of every pair of a verify-pairs output on the same pairs
    std::vector<float> xy;
    std::vector<double> models;
    if (guided) {
        xy.resize((size_t)seg[n_img] * 2);
        for (size_t f = 0; f < n_img; f++) match_tool::load_xy(guided->kp[f], (size_t)(seg[f + 1] - seg[f]), files[f], xy.data() + 2 * seg[f]);
        std::vector<size_t> vs, bs;
        std::vector<int32_t> vpairs;
        std::vector<int64_t> bits;
        dlco_io::read_dataset<int32_t>(guided->verify_out, "Pairs", vs, vpairs);
        if (vs.size() != 2 || vs[0] != P || vs[1] != 2 || vpairs != pairs)
            throw std::runtime_error(std::string(guided->verify_out) + ": its Pairs are not the pairs of " + pairs_file + ": the models belong to other pairs");
        const char *name = guided->fundamental ? "FundamentalBits" : "HomographyBits";
        dlco_io::read_dataset<int64_t>(guided->verify_out, name, bs, bits);
        if (bs.size() != 2 || bs[0] != P || bs[1] != 9) throw std::runtime_error(std::string(guided->verify_out) + ": " + name + " must be a [P, 9] table");
        models.resize(9 * P);
        std::memcpy(models.data(), bits.data(), 9 * P * sizeof(double));
        for (double v : models)
            if (!std::isfinite(v)) throw std::runtime_error(std::string(guided->verify_out) + ": " + name + " holds a value that is not finite");
    }
    printf("Tables: %zu, %lld x %zu%s\n", n_img, (long long)seg[n_img], r, Line<T>::tag);
    printf("Pairs: %zu\n", P);
    if (guided) match_tool::print_guided(guided->fundamental, guided->radius);

    // -cross: the reversed pairs ride in the same batch, pair P + p is pair p swapped
    std::vector<int32_t> batch(pairs);
    if (cross)
        for (size_t p = 0; p < P; p++) { batch.push_back(pairs[2 * p + 1]); batch.push_back(pairs[2 * p]); }
    const size_t B = batch.size() / 2;
    std::vector<int64_t> row0(B + 1);
    if (dlco_desc_match_pairs_rows(seg.data(), (int32_t)n_img, batch.data(), (int64_t)B, row0.data()) != DLCO_OK)
        throw std::runtime_error("the segment table or the pairs are invalid");

    if (dlco_desc_create(&ctx, 1.4f, 8, 1, device) != DLCO_OK) throw std::runtime_error(dlco_desc_last_error(nullptr));
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> nearest((size_t)row0[B] * 2);
    std::vector<Dist> sqdist((size_t)row0[B] * 2);
    double kernel_ms = 0.0;
    if (guided) {
        // the pairs under side 0, then (-cross) the reversed pairs under side 1 and the same matrices: two calls, one output
        const auto call = guided->fundamental ? Line<T>::pairs_guided_epipolar : Line<T>::pairs_guided;
        for (size_t k = 0; k < B / P; k++) {
            if (call(ctx, table.data(), xy.data(), seg.data(), (int32_t)n_img, batch.data() + 2 * P * k, (int64_t)P, (int32_t)r, models.data(),
                     guided->radius, (int32_t)k, nearest.data() + 2 * row0[P * k], sqdist.data() + 2 * row0[P * k]) != DLCO_OK)
                throw std::runtime_error(dlco_desc_last_error(ctx));
            kernel_ms += dlco_desc_last_kernel_ms(ctx);
        }
    } else {
        if (Line<T>::match_pairs(ctx, table.data(), seg.data(), (int32_t)n_img, batch.data(), (int64_t)B, (int32_t)r, nearest.data(), sqdist.data()) != DLCO_OK)
            throw std::runtime_error(dlco_desc_last_error(ctx));
        kernel_ms = dlco_desc_last_kernel_ms(ctx);
    }
    // the lists of the first P pairs; -cross: pair p's reverse answer is pair P + p's rows of the same buffer, whichever call wrote them
    std::vector<int64_t> moff;
    std::vector<int32_t> matches;
    std::vector<Dist> mdist;
    const std::vector<int64_t> back_row0(row0.begin() + (B - P), row0.begin() + B);
    match_tool::select<T>(ctx, seg, batch.data(), P, (size_t)row0[P], nearest.data(), sqdist.data(), use_ratio ? ratio : 0.0f,
                          cross ? nearest.data() : nullptr, back_row0, row0[B], moff, matches, mdist);
    {
        dlco_io::Writer wr(out);
        wr.write<int32_t>("Pairs", pairs.data(), P, 2);
        wr.write_vec<int64_t>("RowOffsets", row0.data(), P + 1);
        wr.write<int32_t>("Nearest", nearest.data(), (size_t)row0[P], 2);
        wr.write<Dist>("NearestSqDist", sqdist.data(), (size_t)row0[P], 2);
        wr.write_vec<int64_t>("MatchOffsets", moff.data(), P + 1);
        wr.write<int32_t>("Matches", matches.data(), mdist.size(), 2);
        wr.write_vec<Dist>("MatchSqDist", mdist.data(), mdist.size());
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("Matches: %zu / %lld\n", mdist.size(), (long long)row0[P]);
    printf("Kernels: %.6f ms\n", kernel_ms);
    printf("Total: %.09f sec\n", sec);
}
}  // namespace

int main(int argc, char **argv)
{
    int device = 0;
    bool help = false, cross = false, use_ratio = false, u8 = false;
    float ratio = 1.0f;
    const char *pairs_file = nullptr, *out = nullptr, *model = nullptr;
    std::vector<const char *> files;
    Guided guided;
    bool kp_given = false;
    for (int i = 1; i < argc; i++) {
        if (argv[i][0] == '-') {
            const bool has_val = i + 1 < argc;
            if (std::strcmp(argv[i], "-guided") == 0 && has_val && argv[i + 1][0] != '-') { guided.verify_out = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-kp") == 0) {            // the files up to the next option
                kp_given = true;
                while (i + 1 < argc && argv[i + 1][0] != '-') guided.kp.push_back(argv[++i]);
                continue;
            }
            if (std::strcmp(argv[i], "-radius") == 0 && has_val) { guided.radius = (float)atof(argv[++i]); continue; }
            if (std::strcmp(argv[i], "-model") == 0 && has_val) { model = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-help") == 0) { help = true; continue; }
            if (std::strcmp(argv[i], "-pairs") == 0 && has_val) { pairs_file = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-out") == 0 && has_val) { out = argv[++i]; continue; }
            if (std::strcmp(argv[i], "-ratio") == 0 && has_val) { ratio = (float)atof(argv[++i]); use_ratio = true; continue; }
            if (std::strcmp(argv[i], "-cross") == 0) { cross = true; continue; }
            if (std::strcmp(argv[i], "-u8") == 0) { u8 = true; continue; }
            if (std::strcmp(argv[i], "-device") == 0 && has_val) { device = atoi(argv[++i]); continue; }
            cout << "ERROR: Invalid " << argv[i] << " option." << endl;
            help = true;
        } else {
            files.push_back(argv[i]);
        }
    }
    if (!pairs_file || !out || files.empty()) help = true;
    if (!match_tool::ratio_ok(use_ratio, ratio)) help = true;
    guided.fundamental = model && std::strcmp(model, "fundamental") == 0;
    if (!match_tool::model_ok(model)) help = true;
    if ((model || kp_given) && !guided.verify_out) {
        cout << "ERROR: -kp and -model need -guided." << endl;
        help = true;
    }
    if (guided.verify_out && (guided.kp.empty() || guided.kp.size() != files.size())) {
        cout << "ERROR: Invalid -guided option: it needs -kp with one keypoint file per descriptor file." << endl;
        help = true;
    }
    if (guided.verify_out && u8) {
        cout << "ERROR: -guided has no -u8 form." << endl;
        help = true;
    }
    if (!match_tool::radius_ok(guided.radius)) help = true;
    if (help) {
        cout << endl;
        cout << "Usage: match-pairs -pairs pairs_file -out dst_h5_filename [-u8] [-ratio f] [-cross] [-device n] desc_file_0 desc_file_1 ..." << endl;
        cout << "       [-guided verify_pairs_out -kp kp_file_0 kp_file_1 ... [-radius f] [-model homography|fundamental]]" << endl;
        cout << endl;
        return 1;
    }
    dlco_desc_ctx *ctx = nullptr;
    try {
        if (u8) run<uint8_t>(pairs_file, files, out, use_ratio, ratio, cross, device, ctx);
        else run<float>(pairs_file, files, out, use_ratio, ratio, cross, device, ctx, guided.verify_out ? &guided : nullptr);
        dlco_desc_destroy(ctx);
    } catch (const std::exception &e) {
        if (ctx) dlco_desc_destroy(ctx);
        std::fprintf(stderr, "match-pairs: %s\n", e.what());
        return 2;
    }
    return 0;
}
