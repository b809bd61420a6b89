// C entry points over opencv-dlco_amd/csrc/match_slices.hpp for tests/test_match_slices.py: pure host code, no libdlco.so.
#include "../../opencv-dlco_amd/csrc/match_slices.hpp"

#include <cstdint>

extern "C" {

// kind 0: the float matcher, kind 1: the byte matcher
static const match_slicing::Shape &shape(int kind) { return kind ? match_slicing::kU8 : match_slicing::kFloat; }

int shim_tiles_per_slice(int64_t nq, int64_t nt, int n_cu, int kind) { return match_slicing::tiles_per_slice(shape(kind), (long)nq, (long)nt, n_cu); }

int shim_slices(int64_t nt, int tiles_per_slice, int kind) { return match_slicing::slices(shape(kind), (long)nt, tiles_per_slice); }

int shim_query_block(int kind) { return kind ? match_slicing::UQ : match_slicing::MQ; }

int shim_tile(int kind) { return kind ? match_slicing::UT : match_slicing::TN; }

}  // extern "C"
