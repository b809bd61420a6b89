// match_rules.hpp — the filters of the tool `match` on the library's nearest / second-nearest answer: pure host
// functions, no device, no I/O (tests/shim/match_rules_shim.cpp runs them on a machine without a GPU).
#pragma once

#include "../csrc/select_rules.hpp"

#include <cstdint>
#include <vector>

namespace match_rules {

// Lowe's ratio test on L2 distances, stated on the squared ones: the nearest row is kept iff it is closer than f times
// the second nearest, d1 < f^2 d2 in double (so d1 == f^2 d2 is dropped, and d1 = d2 = 0 is dropped).  A query without
// a second neighbour (idx2 == -1, a train table of one row) has nothing to be compared with and is kept.  On the exact
// integer distances of byte tables (dlco_desc_match_u8) the same comparison in double, in which an int32 and its product
// with f^2 of a float f are exact enough that d1 == f^2 d2 is still dropped.  csrc/select_rules.hpp states both, for these
// filters and for the library's dlco_desc_select_pairs*:
//   bool ratio_keep(float d1, float d2, int32_t idx2, float f);   bool ratio_keep(int32_t d1, int32_t d2, int32_t idx2, float f);
using select_rules::ratio_keep;

// The mutual rule: (i, j) is kept iff the nearest query of train row j is i.  back [nt][2] is the library's answer with
// the tables swapped.
//   bool cross_keep(int64_t i, int32_t j, const int32_t *back);
using select_rules::cross_keep;

// The filtered list for nearest [nq][2] / sqdist [nq][2]: pairs (query, train) ascending in query and their squared
// distances.  use_ratio / back (NULL: no mutual check) select the rules; both may be given; an empty list is a valid result.
// A query whose nearest index is -1 (no usable neighbour) is never a match.
inline void select(int64_t nq, const int32_t *nearest, const float *sqdist, bool use_ratio, float f, const int32_t *back,
                   std::vector<int32_t> &pairs, std::vector<float> &dists)
{
    pairs.clear();
    dists.clear();
    for (int64_t i = 0; i < nq; i++) {
        const int32_t j = nearest[2 * i];
        if (j < 0) continue;
        if (use_ratio && !ratio_keep(sqdist[2 * i], sqdist[2 * i + 1], nearest[2 * i + 1], f)) continue;
        if (back && !cross_keep(i, j, back)) continue;
        pairs.push_back((int32_t)i);
        pairs.push_back(j);
        dists.push_back(sqdist[2 * i]);
    }
}

// The same list for the int32 distances of dlco_desc_match_u8.
inline void select(int64_t nq, const int32_t *nearest, const int32_t *sqdist, bool use_ratio, float f, const int32_t *back,
                   std::vector<int32_t> &pairs, std::vector<int32_t> &dists)
{
    pairs.clear();
    dists.clear();
    for (int64_t i = 0; i < nq; i++) {
        const int32_t j = nearest[2 * i];
        if (j < 0) continue;
        if (use_ratio && !ratio_keep(sqdist[2 * i], sqdist[2 * i + 1], nearest[2 * i + 1], f)) continue;
        if (back && !cross_keep(i, j, back)) continue;
        pairs.push_back((int32_t)i);
        pairs.push_back(j);
        dists.push_back(sqdist[2 * i]);
    }
}

}  // namespace match_rules
