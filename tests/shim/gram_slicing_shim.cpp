// C entry to eig_rules::gram_slicing for tests/test_gram_slicing.py (no HIP, no GPU).
#include "../../opencv-dlco_amd/csrc/eig_rules.hpp"

extern "C" {

// out[0] = split_k (what the GEMM is asked for), out[1] = chunk, out[2] = slices, out[3] = whole(F)
void shim_gram_slicing(long F, long tiles, long slab_cap, int *out)
{
    const dlco::eig_rules::GramSlicing g = dlco::eig_rules::gram_slicing(F, tiles, slab_cap);
    out[0] = g.split_k; out[1] = g.chunk; out[2] = g.slices; out[3] = g.whole(F) ? 1 : 0;
}

}
