// quant_io.hpp — the two datasets that carry a quantiser next to a "DescriptorU8" table ("QuantScale" [1] f32,
// "QuantOffset" [r] f32), shared by quantize, describe, describe-image and match.
#pragma once

#include "dlco_io.hpp"

#include <cmath>
#include <cstring>

namespace quant_io {

// the quantiser of `path` for rows of r bytes; throws when a dataset is missing or does not fit
inline void read(const char *path, size_t r, float &scale, std::vector<float> &offset)
{
    std::vector<size_t> s1, s2;
    std::vector<float> sc;
    dlco_io::read_dataset<float>(path, "QuantScale", s1, sc);
    dlco_io::read_dataset<float>(path, "QuantOffset", s2, offset);
    if (sc.size() != 1) throw std::runtime_error(std::string(path) + ": QuantScale must hold one value");
    if (offset.size() != r) throw std::runtime_error(std::string(path) + ": QuantOffset has " + std::to_string(offset.size()) + " entries, the descriptor " + std::to_string(r));
    scale = sc[0];
    if (!(scale > 0.0f) || !std::isfinite(scale)) throw std::runtime_error(std::string(path) + ": QuantScale must be finite and positive");
}

inline void write(dlco_io::Writer &wr, float scale, const std::vector<float> &offset)
{
    wr.write_vec<float>("QuantScale", &scale, 1);
    wr.write_vec<float>("QuantOffset", offset.data(), offset.size());
}

// whether `path` carries a quantiser at all ("QuantScale" can be read); one that is there is read like read() does
inline bool present(const char *path, size_t r, float &scale, std::vector<float> &offset)
{
    std::vector<size_t> s;
    std::vector<float> sc;
    try { dlco_io::read_dataset<float>(path, "QuantScale", s, sc); } catch (const std::exception &) { return false; }
    read(path, r, scale, offset);                          // a quantiser that is there has to fit
    return true;
}

inline bool same_bits(float s1, const std::vector<float> &o1, float s2, const std::vector<float> &o2)
{
    return o1.size() == o2.size() && std::memcmp(&s1, &s2, sizeof(float)) == 0 &&
           (o1.empty() || std::memcmp(o1.data(), o2.data(), o1.size() * sizeof(float)) == 0);
}

}  // namespace quant_io
