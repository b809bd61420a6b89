// The guided-matching rule of opencv-dlco_amd/csrc/guided_rules.hpp as a C ABI for tests/test_guided_rules.py: plain C++, no
// libdlco.so, no GPU.  Build with -ffp-contract=off (the header switches contraction off itself only under clang).
#include "../../opencv-dlco_amd/csrc/guided_rules.hpp"

namespace gr = guided_rules;

extern "C" {

double shim_guided_threshold_sq(float radius) { return verify_rules::threshold_sq(radius); }

void shim_guided_record(const double *H, double x, double y, double t2, double *rec)
{
    const gr::Rec r = gr::record(H, x, y, t2);
    rec[0] = r.X; rec[1] = r.Y; rec[2] = r.W; rec[3] = r.T;
}

// n pairs: the point (px, py) on the side H applies to against (u, v); admits(record(...)) and verify_rules::inlier
void shim_guided_pairs(const double *H, double t2, const double *px, const double *py, const double *u, const double *v, int64_t n, uint8_t *admitted,
                       uint8_t *inlier)
{
    for (int64_t k = 0; k < n; k++) {
        admitted[k] = gr::admits(gr::record(H, px[k], py[k], t2), u[k], v[k]) ? 1 : 0;
        inlier[k] = verify_rules::inlier(H, px[k], py[k], u[k], v[k], t2) ? 1 : 0;
    }
}

// P(i, j) of two tables: mask [nq][nt]
void shim_guided_mask(const double *H, float radius, int32_t h_side, const float *qxy, int64_t nq, const float *txy, int64_t nt, uint8_t *mask)
{
    const double t2 = verify_rules::threshold_sq(radius);
    for (int64_t i = 0; i < nq; i++)
        for (int64_t j = 0; j < nt; j++) mask[i * nt + j] = gr::pair_admitted(H, t2, h_side, qxy + 2 * i, txy + 2 * j) ? 1 : 0;
}

void shim_guided_top2(const float *dist, const float *qxy, int64_t nq, const float *txy, int64_t nt, const double *H, float radius, int32_t h_side,
                      int32_t *idx, float *sqdist)
{
    gr::guided_top2_host(dist, qxy, nq, txy, nt, H, radius, h_side, idx, sqdist);
}

}  // extern "C"
