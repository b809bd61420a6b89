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

// The numbers of a matcher's kernel that the rule takes.
struct Shape {
    int qblock;                        // queries per workgroup
    int tile;                          // train rows per staged tile
    int fill_cu;                       // workgroups that a CU holds at once
    int per_cu;                        // workgroups per CU wanted from a launch
};
// The float matcher: one workgroup runs per CU (133 KB of LDS).  The byte matcher: a CU holds several workgroups (37 KB of
// LDS, one wave per SIMD each), so twice the CUs are to be filled first and sixteen workgroups per CU wanted.
constexpr Shape kFloat{128, 128, 1, 8}, kU8{256, 128, 2, 16};

constexpr int MQ = kFloat.qblock, TN = kFloat.tile;        // the kernels' compile-time ints
constexpr int UQ = kU8.qblock, UT = kU8.tile;

// Slices of train for nq queries, whole tiles per slice.  First enough slices that every CU has its workgroups (float,
// 2048 x 2048: 16 query blocks x 16 one-tile slices took 41 us, x 4 four-tile slices 70).  Beyond that a launch is a
// number of rounds of fill_cu * n_cu workgroups and the last round may be nearly empty (float, 782 query blocks on 256 CUs:
// 3.05 rounds take the time of 4; 100 000 x 100 000 at r = 128 went from 63.8 to 48.5 ms with three slices, 9.2 rounds):
// enough slices for per_cu workgroups per CU keep that loss near a tenth, as long as a slice keeps four tiles (a
// workgroup's start - its A fragments, the first tile's latency - is paid per slice).  Returns the tiles per slice; the
// slice count is slices() of that.
// tiles_per_slice_of takes the query blocks counted by the caller: those of one call (tiles_per_slice), or of every pair of
// a batched launch (match_batch.hpp), whose workgroups fill the CUs together.
inline int tiles_per_slice_of(const Shape &s, long qblocks, long nt, int n_cu)
{
    const long tiles = (nt + s.tile - 1) / s.tile;
    const long fill = std::min(tiles, ((long)s.fill_cu * n_cu + qblocks - 1) / qblocks);
    const long rounds = std::min(tiles / 4, ((long)s.per_cu * n_cu + qblocks - 1) / qblocks);
    const long want = std::max(1L, std::max(fill, rounds));
    return (int)((tiles + want - 1) / want);
}
inline int tiles_per_slice(const Shape &s, long nq, long nt, int n_cu)
{
    return tiles_per_slice_of(s, (nq + s.qblock - 1) / s.qblock, nt, n_cu);
}
inline int slices(const Shape &s, long nt, int tiles_per_slice)
{
    const long tiles = (nt + s.tile - 1) / s.tile;
    return (int)((tiles + tiles_per_slice - 1) / tiles_per_slice);
}

}  // namespace match_slicing
