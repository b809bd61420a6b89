// C entry points over opencv-dlco_amd/csrc/match_slices.hpp for tests/test_match_slices.py: pure host code, no libdlco.so.
#include "../../opencv-dlco_amd/csrc/match_slices.hpp"

#include <cstdint>

extern "C" {

// kind 0: the float matcher, kind 1: the byte matcher
int shim_tiles_per_slice(int64_t nq, int64_t nt, int n_cu, int kind)
{
    return kind ? match_slicing::match_u8_tiles_per_slice((long)nq, (long)nt, n_cu) : match_slicing::match_tiles_per_slice((long)nq, (long)nt, n_cu);
}

int shim_slices(int64_t nt, int tiles_per_slice, int kind)
{
    return kind ? match_slicing::match_u8_slices((long)nt, tiles_per_slice) : match_slicing::match_slices((long)nt, tiles_per_slice);
}

int shim_query_block(int kind) { return kind ? match_slicing::UQ : match_slicing::MQ; }

int shim_tile(int kind) { return kind ? match_slicing::UT : match_slicing::TN; }

}  // extern "C"
