// match_slices.hpp — how the matchers cut the train table into slices (dlco_desc_match*, dlco_desc_cross_sqdists*): the
// rule stated once for the host loops (dlco_desc_api.cpp), the kernels (kernels_match.hip, kernels_match_u8.hip), which
// share the tile sizes below with it, and the CPU test (tests/shim/match_slices_shim.cpp).  Plain C++: no HIP header, no
// device, no I/O.
//
// A launch is a grid of (query blocks) x (slices); the workgroup of a slice walks whole tiles of train,
// [slice * tiles_per_slice * tile, ...), and the top two of the slices are merged by a second kernel when there is more
// than one.  The kernels rely on one property of the rule: NO SLICE IS EMPTY, (slices - 1) * tiles_per_slice < tiles, so
// that the first row of every slice is a row of the table (jbeg < nt); their loads clamp to the last step of a slice and
// would index below the table if a slice had none.
#pragma once

#include <algorithm>

namespace match_slicing {

constexpr int MQ = 128;                // float matcher: queries per workgroup
constexpr int TN = 128;                //                train rows per staged tile
constexpr int UQ = 256;                // byte matcher: queries per workgroup
constexpr int UT = 128;                //               train rows per staged tile

// Slices of train for nq queries, whole tiles per slice.  One workgroup runs per CU.  First enough slices that every
// CU has one (2048 x 2048: 16 query blocks x 16 one-tile slices took 41 us, x 4 four-tile slices 70).  Beyond that a
// launch is a number of rounds of n_cu workgroups and the last round may be nearly empty (782 query blocks on 256 CUs:
// 3.05 rounds take the time of 4; 100 000 x 100 000 at r = 128 went from 63.8 to 48.5 ms with three slices, 9.2 rounds):
// enough slices for eight rounds keep that loss near a tenth, as long as a slice keeps four tiles (a workgroup's start -
// its A fragments, the first tile's latency - is paid per slice).  Returns the tiles per slice; the slice count is
// ceil(tiles / that).
inline int match_tiles_per_slice(long nq, long nt, int n_cu)
{
    const long qblocks = (nq + MQ - 1) / MQ, tiles = (nt + TN - 1) / TN;
    const long fill = std::min(tiles, (n_cu + qblocks - 1) / qblocks);
    const long rounds = std::min(tiles / 4, (8L * n_cu + qblocks - 1) / qblocks);
    const long want = std::max(1L, std::max(fill, rounds));
    return (int)((tiles + want - 1) / want);
}
inline int match_slices(long nt, int tiles_per_slice)
{
    const long tiles = (nt + TN - 1) / TN;
    return (int)((tiles + tiles_per_slice - 1) / tiles_per_slice);
}

// The same for the byte matcher: the rule of match_tiles_per_slice with that kernel's numbers, which is why it is not
// that function: a query block is 256 rows, and a CU holds several workgroups (37 KB of LDS, one wave per SIMD each), so
// twice the CUs are to be filled first and sixteen workgroups per CU keep the loss of the last round small, as long as a
// slice keeps four tiles.
inline int match_u8_tiles_per_slice(long nq, long nt, int n_cu)
{
    const long qblocks = (nq + UQ - 1) / UQ, tiles = (nt + UT - 1) / UT;
    const long fill = std::min(tiles, (2L * n_cu + qblocks - 1) / qblocks);
    const long rounds = std::min(tiles / 4, (16L * n_cu + qblocks - 1) / qblocks);
    const long want = std::max(1L, std::max(fill, rounds));
    return (int)((tiles + want - 1) / want);
}
inline int match_u8_slices(long nt, int tiles_per_slice)
{
    const long tiles = (nt + UT - 1) / UT;
    return (int)((tiles + tiles_per_slice - 1) / tiles_per_slice);
}

}  // namespace match_slicing
