// split_bf16_dev.hpp — device code shared by the kernels that form a product on the bf16 matrix cores from operands split
// into bf16 planes: skinny_bf16x2_kernel, skinny_rows_kernel, skinny_sym_kernel (kernels_bf16x2.hip) and
// project_rows_kernel (kernels_project.hip).  The plane layout is also what split_x_kernel, reduce_split_kernel and
// rank_first_term_kernel write, and syrk_split_rows_kernel (which has a layout of its own) splits with split_f32.  What
// differs between the product kernels stays with them: their loaders, how a compute wave fetches its fragments from
// LDS, and the exchange of the two K halves.
//
// With these helpers every kernel of the library compiles to the instructions it had with its own copy
// (tools/kernel_resources.py --compare on the assembly of hipcc --cuda-device-only -S: all identical).  A helper that
// reorders a kernel, or shifts its address arithmetic or instruction counts, does not belong here, however alike the
// copies look.
#pragma once

#include "dlco_internal.hpp"

namespace dlco {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- the split ------------------------------------------------------------------------------------------------------------
// x = h + l (+ l2): NS bf16 parts, 8 mantissa bits each, every part the rounding of what the parts before it left over;
// they go to element j of the vectors of their parts.  Parts beyond NS are not formed.
template <int NS>
__device__ __forceinline__ void split_f32(float x, int j, bf16x8 &h, bf16x8 &l, bf16x8 &l2)
{
    h[j] = (__bf16)x;
    if (NS >= 2) {
        const float r1 = x - (float)h[j];
        l[j] = (__bf16)r1;
        if (NS == 3) l2[j] = (__bf16)(r1 - (float)l[j]);
    }
}

// eight consecutive k values of one column (two 16-byte halves) -> the B fragments of their parts
template <int NS>
__device__ __forceinline__ void split_frag(const f32x4 &g0, const f32x4 &g1, bf16x8 &bh, bf16x8 &bl, bf16x8 &bl2)
{
#pragma unroll
    for (int j = 0; j < 8; j++) split_f32<NS>(j < 4 ? g0[j & 3] : g1[j & 3], j, bh, bl, bl2);
}

template <int NS>
__device__ __forceinline__ void split_frag(const float (&g)[8], bf16x8 &bh, bf16x8 &bl, bf16x8 &bl2)
{
#pragma unroll
    for (int j = 0; j < 8; j++) split_f32<NS>(g[j], j, bh, bl, bl2);
}

// ---- the plane layout -----------------------------------------------------------------------------------------------------
// A plane holds one part of X [32 MT][K] in MFMA A-fragment order, in 16-byte entries of eight values: entry
// plane_entry(k16, MT, tile, lane) = X[tile*32 + (lane & 31)][k16*16 + 8*(lane >> 5) .. + 7].  The 64 entries of a
// (k16, tile) pair are one whole 1-KiB fragment load, the MT tiles of a K step are adjacent, and a chunk of four K steps
// is MT * 256 consecutive entries.  The index has the type of k16.
template <typename I>
__host__ __device__ constexpr I plane_entry(I k16, int MT, int tile, int lane) { return (k16 * MT + tile) * 64 + lane; }
// The entry that holds X[row][8 c8 .. 8 c8 + 7]: plane_entry(c8 >> 1, MT, row >> 5, (row & 31) + 32 * (c8 & 1)), written out
// because the kernels that emit planes come out of the compiler reordered when it goes through the call; the assertion
// below keeps the two in step.
__host__ __device__ __forceinline__ constexpr long plane_entry_at(int MT, int row, int c8)
{
    return ((long)(c8 >> 1) * MT + (row >> 5)) * 64 + (row & 31) + 32 * (c8 & 1);
}
constexpr bool plane_entry_at_is_plane_entry()
{
    for (int MT = 1; MT <= 5; MT++)
        for (int row = 0; row < 32 * MT; row++)
            for (int c8 = 0; c8 < 8; c8++)
                if (plane_entry_at(MT, row, c8) != plane_entry((long)(c8 >> 1), MT, row >> 5, (row & 31) + 32 * (c8 & 1))) return false;
    return true;
}
static_assert(plane_entry_at_is_plane_entry(), "plane_entry_at must name the entry plane_entry gives for (row, c8)");

// ---- the product of one K step --------------------------------------------------------------------------------------------
// acc[t] += A_t * B for the MT row tiles, A = ah + al (+ al2), B = bh + bl (+ bl2); parts beyond NS are not read.
// NS = 3 keeps the six terms down to 2^-16 (h*l2, l2*h, l*l, h*l, l*h, h*h), NS = 2 the three down to 2^-8 (h*l, l*h,
// h*h), NS = 1 is one MFMA on operands rounded once.
// The terms are added smallest first, so that the small ones are not rounded away against a large partial sum.  This
// order fixes the last bits of every filter product and every projected distance: the tracker's products and the
// statistics pass agree because they all come through here.
template <int MT, int NS>
__device__ __forceinline__ void mfma_split_terms(const bf16x8 *ah, const bf16x8 *al, const bf16x8 *al2, const bf16x8 &bh, const bf16x8 &bl,
                                                 const bf16x8 &bl2, f32x16 (&acc)[MT])
{
#pragma unroll
    for (int t = 0; t < MT; t++) {
        if (NS == 3) {
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[t], bl2, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al2[t], bh, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[t], bl, acc[t], 0, 0, 0);
        }
        if (NS >= 2) {
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[t], bl, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[t], bh, acc[t], 0, 0, 0);
        }
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[t], bh, acc[t], 0, 0, 0);
    }
}

// ---- the LDS images of the kernels with loader waves ----------------------------------------------------------------------
// A workgroup of 8 compute + 4 loader waves owns 128 rows of the streamed fp32 operand and walks K in chunks of 64: an
// image of that operand is [128][SB_RS] floats, the A image beside it the chunk's slice of every plane.
constexpr int SB_KC = 64;                  // chunk depth (floats)
constexpr int SB_RS = SB_KC + 4;           // LDS row stride of the streamed image (floats): conflict-free 32-byte fragment reads
constexpr int SB_T = 768;                  // 8 compute + 4 loader waves
constexpr int SB_ROWS = 128;               // rows of the streamed operand per workgroup
constexpr int SB_GBYTES = SB_ROWS * SB_RS * 4;                                                    // one streamed image
__host__ __device__ constexpr int sb_abytes(int mt, int ns) { return ns * mt * 4 * 64 * 16; }     // one A image: ns planes x 4 steps x mt tiles x 1 KiB
inline size_t sb_lds_bytes(int mt, int ns) { return (size_t)2 * (SB_GBYTES + sb_abytes(mt, ns)); }   // two images of each operand

// The loaders' view of the planes: one buffer resource per part (a part beyond NS is never read).
struct PlaneRsrc { __amdgpu_buffer_rsrc_t part[3]; };
template <int MT, int NS>
__device__ __forceinline__ PlaneRsrc make_plane_rsrc(const bf16x8 *hi, const bf16x8 *lo, const bf16x8 *lo2, int K)
{
    const int plane_bytes = MT * 32 * K * 2;
    PlaneRsrc r;
    r.part[0] = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16x8 *>(hi), 0, plane_bytes, 0x00020000);
    r.part[1] = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16x8 *>(NS >= 2 ? lo : hi), 0, plane_bytes, 0x00020000);
    r.part[2] = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16x8 *>(NS == 3 ? lo2 : hi), 0, plane_bytes, 0x00020000);
    return r;
}
// Entry lt + 256 v (v static) of the A image of the chunk that starts at K step k16: its slice of every plane is MT * 256
// consecutive entries from byte a0 = slice_bytes<MT>(k16) on, so entry lt + 256 v belongs to part v / MT - a static
// resource, a scalar offset and one per-lane offset (16 lt) for all of a loader thread's requests.
template <int MT>
__device__ __forceinline__ int slice_bytes(int k16) { return plane_entry(k16, MT, 0, 0) * 16; }
template <int MT>
__device__ __forceinline__ bf16x8 load_slice_entry(const PlaneRsrc &rs, int a0, int lt, int v)
{
    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs.part[v / MT], 16 * lt, a0 + (v % MT) * 256 * 16, 0));
}

// Operands of one K step of a compute wave, as it reads them from the LDS images: the eight k values of its row of the
// streamed image (two 16-byte halves) and the step's fragment of every plane and row tile.  The fetch itself, the
// accumulator zeroing and the K-half exchange are still spelled out in each kernel: as helpers here (arguments or
// threadIdx inside, forced or plain inlining, index or base-pointer form) they changed the LDS and slab address
// arithmetic of most instantiations - other instruction counts, ds_write2st64 pairs lost, up to 3 VGPRs and in one
// case 8 bytes of scratch more.  The step's product is split_frag + mfma_split_terms inside a lambda of the kernel:
// the same two calls in a function of this header renamed registers in six instantiations.
template <int MT, int NS>
struct Frag { f32x4 g0, g1; bf16x8 a[NS][MT]; };

}  // namespace dlco
