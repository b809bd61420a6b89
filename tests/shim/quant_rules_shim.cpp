// C entry points over opencv-dlco_amd/csrc/quant_rules.hpp for tests/test_quant_rules.py: pure host code, no libdlco.so.
#include "../../opencv-dlco_amd/csrc/quant_rules.hpp"

extern "C" {

int shim_quant_one(float y, float o, float s) { return quant_rules::quantize_one(y, o, s); }

void shim_quantize(const float *Y, int64_t n, int r, float s, const float *offset, uint8_t *out) { quant_rules::quantize(Y, n, r, s, offset, out); }

int shim_quant_fit(const float *Y, int64_t n, int r, float *scale, float *offset) { return quant_rules::fit(Y, n, r, scale, offset) ? 1 : 0; }

}  // extern "C"
