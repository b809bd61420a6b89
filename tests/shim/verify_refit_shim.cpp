// The constants of the refit round on the device (opencv-dlco_amd/csrc/verify_rules.hpp, epipolar_rules.hpp) for the tests of
// tests/test_verify_refit_rules.py and tests/test_verify_refit_gpu.py, which place their inliers around the kernel's staging
// chunk: g++ -shared -fPIC -ffp-contract=off.  The rounds themselves are exported by verify_rules_shim.cpp and
// epipolar_rules_shim.cpp.
#include "../../opencv-dlco_amd/csrc/epipolar_rules.hpp"

extern "C" {

int shim_refit_chunk() { return verify_rules::kRefitChunk; }
int shim_refit_sums(int fundamental) { return fundamental ? epipolar_rules::kRefitSums : verify_rules::kDltSums; }
int shim_refit_row(int fundamental) { return fundamental ? epipolar_rules::kRefitRow : verify_rules::kDltRow; }
// the positions of a match's row that sum l multiplies: t [4]
void shim_refit_terms(int fundamental, int l, int *t)
{
    const verify_rules::Terms x = fundamental ? epipolar_rules::refit_terms(l) : verify_rules::dlt_terms(l);
    t[0] = x.a; t[1] = x.b; t[2] = x.c; t[3] = x.d;
}

}
