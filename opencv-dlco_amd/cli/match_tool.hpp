// match_tool.hpp — what the tools `match` and `match-pairs` share: the float and the byte line as one trait over the library's
// calls, the loaders of a descriptor table and of a keypoint file, the option checks with one text, and the step from a
// nearest-two answer to the match list, which is the library's own (dlco_desc_select_pairs*: -ratio, -cross).
#pragma once

#include "../../include/dlco.h"
#include "dlco_io.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

namespace match_tool {

// A line: the element type of the tables, the type of the distances, the dataset the tables are read from, the tag of the
// printed lines, and the library's calls as the tools make them.  The byte line's guided calls are named for the day the
// tools grow a guided -u8 form; today both refuse it.
template <typename T> struct Line;
template <> struct Line<float> {
    using Dist = float;
    static constexpr const char *dataset = "Descriptor";
    static constexpr const char *tag = "";
    static constexpr auto match = dlco_desc_match;
    static constexpr auto guided = dlco_desc_match_guided;
    static constexpr auto guided_epipolar = dlco_desc_match_guided_epipolar;
    static constexpr auto match_pairs = dlco_desc_match_pairs;
    static constexpr auto pairs_guided = dlco_desc_match_pairs_guided;
    static constexpr auto pairs_guided_epipolar = dlco_desc_match_pairs_guided_epipolar;
    static constexpr auto select_pairs = dlco_desc_select_pairs;
};
template <> struct Line<uint8_t> {
    using Dist = int32_t;
    static constexpr const char *dataset = "DescriptorU8";
    static constexpr const char *tag = " (u8)";
    static constexpr auto match = dlco_desc_match_u8;
    static constexpr auto guided = dlco_desc_match_guided_u8;
    static constexpr auto guided_epipolar = dlco_desc_match_guided_epipolar_u8;
    static constexpr auto match_pairs = dlco_desc_match_pairs_u8;
    static constexpr auto pairs_guided = dlco_desc_match_pairs_guided_u8;
    static constexpr auto pairs_guided_epipolar = dlco_desc_match_pairs_guided_epipolar_u8;
    static constexpr auto select_pairs = dlco_desc_select_pairs_u8;
};

// The table [n, r] of a line's dataset; allow_empty: n = 0 is an image without keypoints (match-pairs), else an error
// (match).  A float table with a NaN or a value beyond float's range is refused.
template <typename T> void load_table(const char *path, bool allow_empty, std::vector<size_t> &shape, std::vector<T> &rows)
{
    dlco_io::read_dataset<T>(path, Line<T>::dataset, shape, rows);
    if (shape.size() != 2 || shape[1] < 1 || (!allow_empty && shape[0] < 1))
        throw std::runtime_error(std::string(path) + ": " + Line<T>::dataset + (allow_empty ? " must be an [n, r] table" : " must be a non-empty [n, r] table"));
    if constexpr (std::is_same<T, float>::value) {
        for (float v : rows)
            if (!(v == v) || v > 3.0e38f || v < -3.0e38f) throw std::runtime_error(std::string(path) + ": Descriptor contains NaN");
    }
}

// the (x, y) of the "Keypoints" [n,4] of a detect output, which must have `rows` rows, those of its descriptor table in
// desc_path, into xy_out [rows][2]: the caller's slice of a coordinate table
inline void load_xy(const char *path, size_t rows, const char *desc_path, float *xy_out)
{
    std::vector<size_t> shape;
    std::vector<float> kp;
    dlco_io::read_dataset<float>(path, "Keypoints", shape, kp);
    if (shape.size() != 2 || shape[1] != 4) throw std::runtime_error(std::string(path) + ": Keypoints must be an [n, 4] table");
    if (shape[0] != rows)
        throw std::runtime_error(std::string(path) + ": " + std::to_string(shape[0]) + " keypoints against " + std::to_string(rows) + " descriptors in " + desc_path);
    for (size_t i = 0; i < rows; i++) { xy_out[2 * i] = kp[4 * i]; xy_out[2 * i + 1] = kp[4 * i + 1]; }
}

// The option checks with one text in both tools: each reports on stdout and returns whether the value is valid.
inline bool ratio_ok(bool use_ratio, float ratio)
{
    if (!use_ratio || (ratio > 0.0f && ratio <= 1.0f)) return true;
    std::cout << "ERROR: -ratio must be in (0, 1]." << std::endl;
    return false;
}
inline bool model_ok(const char *model)
{
    if (!model || std::strcmp(model, "fundamental") == 0 || std::strcmp(model, "homography") == 0) return true;
    std::cout << "ERROR: -model must be homography or fundamental." << std::endl;
    return false;
}
inline bool radius_ok(float radius)
{
    if (std::isfinite(radius) && radius > 0.0f) return true;
    std::cout << "ERROR: -radius must be finite and > 0." << std::endl;
    return false;
}
inline void print_guided(bool fundamental, float radius) { printf(fundamental ? "Guided: fundamental, radius %g\n" : "Guided: radius %g\n", radius); }

// The match lists of the first n_pairs pairs of an answer idx / sqdist [rows][2] (rows = the query rows of those pairs), by
// dlco_desc_select_pairs*: ratio 0 is no ratio test, back (null: no mutual check) [n_back_rows][2] the reverse answers, pair
// p's from row back_row0[p].  moff [n_pairs + 1]; matches [moff[n_pairs]][2] and dists [moff[n_pairs]].
template <typename T>
void select(dlco_desc_ctx *ctx, const std::vector<int64_t> &seg, const int32_t *pairs, size_t n_pairs, size_t rows, const int32_t *idx,
            const typename Line<T>::Dist *sqdist, float ratio, const int32_t *back, const std::vector<int64_t> &back_row0, int64_t n_back_rows,
            std::vector<int64_t> &moff, std::vector<int32_t> &matches, std::vector<typename Line<T>::Dist> &dists)
{
    moff.assign(n_pairs + 1, 0);
    matches.resize(2 * std::max<size_t>(rows, 1));         // never a null pointer, which the call refuses
    dists.resize(std::max<size_t>(rows, 1));
    if (Line<T>::select_pairs(ctx, seg.data(), (int32_t)(seg.size() - 1), pairs, (int64_t)n_pairs, idx, sqdist, ratio, back, back_row0.data(), n_back_rows,
                              nullptr, moff.data(), matches.data(), dists.data(), nullptr, nullptr) != DLCO_OK)
        throw std::runtime_error(dlco_desc_last_error(ctx));
    matches.resize(2 * (size_t)moff[n_pairs]);
    dists.resize((size_t)moff[n_pairs]);
}

}  // namespace match_tool
