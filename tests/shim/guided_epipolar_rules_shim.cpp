// The epipolar guided-matching rule of opencv-dlco_amd/csrc/guided_epipolar_rules.hpp as a C ABI for
// tests/test_guided_epipolar_rules.py: plain C++, no libdlco.so, no GPU.  Build with -ffp-contract=off (the header switches
// contraction off itself only under clang).
#include "../../opencv-dlco_amd/csrc/guided_epipolar_rules.hpp"

namespace ge = guided_epipolar;

extern "C" {

double shim_epi_threshold_sq(float threshold) { return verify_rules::threshold_sq(threshold); }

void shim_epi_src_record(const double *F, double x, double y, double *rec)
{
    const ge::SrcRec s = ge::src_record(F, x, y);
    rec[0] = s.l0; rec[1] = s.l1; rec[2] = s.l2; rec[3] = s.L;
}

void shim_epi_dst_record(const double *F, double u, double v, double *rec)
{
    const ge::DstRec d = ge::dst_record(F, u, v);
    rec[0] = d.u; rec[1] = d.v; rec[2] = d.A; rec[3] = d.B;
}

// n pairs: the src point (x, y) against the dst point (u, v); admits(src_record, dst_record) and epipolar_rules::inlier
void shim_epi_pairs(const double *F, double t2, const double *x, const double *y, const double *u, const double *v, int64_t n, uint8_t *admitted,
                    uint8_t *inlier)
{
    for (int64_t k = 0; k < n; k++) {
        admitted[k] = ge::admits(ge::src_record(F, x[k], y[k]), ge::dst_record(F, u[k], v[k]), t2) ? 1 : 0;
        inlier[k] = epipolar_rules::inlier(F, x[k], y[k], u[k], v[k], t2) ? 1 : 0;
    }
}

// P(i, j) of two tables: mask [nq][nt]
void shim_epi_mask(const double *F, float threshold, int32_t f_side, const float *qxy, int64_t nq, const float *txy, int64_t nt, uint8_t *mask)
{
    const double t2 = verify_rules::threshold_sq(threshold);
    for (int64_t i = 0; i < nq; i++)
        for (int64_t j = 0; j < nt; j++) mask[i * nt + j] = ge::pair_admitted(F, t2, f_side, qxy + 2 * i, txy + 2 * j) ? 1 : 0;
}

void shim_epi_top2(const float *dist, const float *qxy, int64_t nq, const float *txy, int64_t nt, const double *F, float threshold, int32_t f_side,
                   int32_t *idx, float *sqdist)
{
    ge::guided_top2_host(dist, qxy, nq, txy, nt, F, threshold, f_side, idx, sqdist);
}

}  // extern "C"
