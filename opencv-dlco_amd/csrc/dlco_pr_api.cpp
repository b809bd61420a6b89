// dlco_pr_api.cpp — C ABI of the pooling-region stage (pr-learn): see the dlco_pr_*
// block of include/dlco.h.  Host orchestration only; the iterations, the validation products and the
// statistics run in HIP kernels (kernels_pr.hip, kernels_step.hip, kernels_stats.hip).
#include "../../include/dlco.h"

#include "dlco_internal.hpp"
#include "pair_index.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace dlco;

struct dlco_pr_ctx {
    int F = 0, N = 0, device = 0;
    float mu = 0.025f, gamma = 0.10f;
    hipStream_t stream = nullptr;
    std::string err;
    DevBuf<float> dists, w, df, vdist, hrows, wtmp;
    DevBuf<uint8_t> labels_dev;
    DevBuf<int32_t> val_pos_ids, val_neg_ids, win_pos, win_neg;
    DevBuf<double> dscal;
    std::vector<uint8_t> labels;
    std::vector<int32_t> h_pos, h_neg;
    PairIndex idx;
    CvRng rng{2215};
    uint32_t t = 0;
    bool have_data = false;
    RocWork *roc = nullptr;
    size_t win_cap = 0;
};

// G settings (mu[k], gamma[k]) trained on the data of `src` (not copied) with a sampler of their own.
// w and dfAvg are [G][F] (rows of F floats, 16-byte aligned since F % 4 == 0; no padding).
struct dlco_pr_grid {
    dlco_pr_ctx *src = nullptr;
    int F = 0, N = 0, G = 0, device = 0, cus = 0;
    int group = 0;                                    // settings per workgroup, 0 = pr_grid_group's rule
    hipStream_t stream = nullptr;
    std::string err;
    std::vector<float> mu, gamma;
    DevBuf<float> w, df, mu_dev, gamma_dev, vdist, hrows, wtmp, sdist;
    DevBuf<int32_t> win_pos, win_neg, sel;
    DevBuf<double> dscal;
    std::vector<int32_t> h_pos, h_neg;
    CvRng rng{2215};
    uint32_t t = 0;
    RocWork *roc = nullptr;
    size_t win_cap = 0;
};

static thread_local std::string g_pr_error;

namespace {

template <typename Ctx, typename Fn>
int guarded(Ctx *c, Fn &&fn)
{
    return guarded_call(g_pr_error, c ? &c->err : nullptr, fn);
}

template <typename Ctx>
void sync(Ctx *c) { DLCO_HIP(hipStreamSynchronize(c->stream)); }
template <typename Ctx>
void h2d(Ctx *c, void *dst, const void *src, size_t bytes)
{
    DLCO_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    sync(c);
}
template <typename Ctx>
void d2h(Ctx *c, void *dst, const void *src, size_t bytes)
{
    DLCO_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    sync(c);
}

// The window's row pairs from the sampler, iPos then iNeg per iteration (src/pr-learn.cpp:303-306)
void draw_window(CvRng &rng, const PairIndex &idx, uint32_t n, std::vector<int32_t> &h_pos, std::vector<int32_t> &h_neg)
{
    h_pos.resize(n); h_neg.resize(n);
    for (uint32_t s = 0; s < n; s++) {
        const int ip = rng.uniform(0, idx.n_pos_trn);
        const int in = rng.uniform(0, idx.n_neg_trn);
        h_pos[s] = idx.pos[ip];
        h_neg[s] = idx.neg[in];
    }
}

// regul = mu * sum|w| (double, index order) and countNonZero(w), src/pr-learn.cpp:357-358
void regul_nnz(const float *w, int F, float mu, float *regul, int32_t *nnz)
{
    double s = 0.0;
    int nz = 0;
    for (int i = 0; i < F; i++) { s += std::fabs((double)w[i]); nz += w[i] != 0.0f; }
    *regul = (float)((double)mu * s);
    if (nnz) *nnz = nz;
}

// The pooling-region counts of ComputePRStats (src/misc.cpp:183-217): rows of the selected regions that are
// not all zero (nzDim), those with a twin among them (dup), nPR = nzDim - dup / 2, Dim = nPR * nchannels
void pr_counts(const float *w, int F, const float *prparams, int pr_cols, int nchannels, int32_t *nPR, int32_t *dim, int32_t *nzdim)
{
    std::vector<const float *> sel;                                     // :183-193
    for (int i = 0; i < F; i++)
        for (int j = 0; j < 8; j++) {
            const float *row = prparams + (size_t)(i * 8 + j) * pr_cols;
            if (!(w[i] > 0.0f)) continue;
            bool any = false;
            for (int k = 0; k < pr_cols && !any; k++) any = row[k] != 0.0f;
            if (any) sel.push_back(row);
        }
    int dup = 0;                                                         // :196-213
    for (size_t i = 0; i < sel.size(); i++) {
        bool inside = false;
        for (size_t j = 0; j < sel.size() && !inside; j++) {
            if (i == j) continue;
            bool same = true;
            for (int k = 0; k < pr_cols && same; k++) same = sel[i][k] == sel[j][k];
            inside = same;
        }
        dup += inside ? 1 : 0;
    }
    *nzdim = (int32_t)sel.size();
    *nPR = *nzdim - dup / 2;
    *dim = *nPR * nchannels;
}

}  // namespace

extern "C" {

const char *dlco_pr_last_error(const dlco_pr_ctx *c) { return c ? c->err.c_str() : g_pr_error.c_str(); }

int dlco_pr_create(dlco_pr_ctx **out, int32_t F, int32_t N, float mu, float gamma, uint64_t seed, int32_t device)
{
    if (!out) return DLCO_ERR_INVALID;
    *out = nullptr;
    dlco_pr_ctx *c = nullptr;
    const int rc = guarded((dlco_pr_ctx *)nullptr, [&] {
        DLCO_CHECK(F >= 4 && F % 4 == 0 && F <= 8192, DLCO_ERR_INVALID, "pr-learn: F must be a multiple of 4, at most 8192");
        DLCO_CHECK(N >= 2 && gamma > 0.f, DLCO_ERR_INVALID, "pr-learn: N >= 2 and gamma > 0 required");
        use_gfx950_device(device);
        c = new dlco_pr_ctx();
        c->F = F; c->N = N; c->mu = mu; c->gamma = gamma; c->device = device;
        c->rng = CvRng(seed);
        DLCO_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->w.alloc(F); c->df.alloc(F); c->wtmp.alloc(F);
        c->w.zero(c->stream); c->df.zero(c->stream);              // src/pr-learn.cpp:195-196
        c->dscal.alloc(4);
        sync(c);
    });
    if (rc != DLCO_OK) { delete c; return rc; }
    *out = c;
    return DLCO_OK;
}

void dlco_pr_destroy(dlco_pr_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->roc) roc_work_destroy(c->roc);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// Uploads Distance [N,F] and Label [N]; index build, shuffle and 80/20 split as src/pr-learn.cpp:229-253
int dlco_pr_set_data(dlco_pr_ctx *c, const float *dists_host, const uint8_t *labels_host)
{
    if (!c || !dists_host || !labels_host) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_HIP(hipSetDevice(c->device));
        c->dists.alloc((size_t)c->N * c->F);
        h2d(c, c->dists.p, dists_host, (size_t)c->N * c->F * sizeof(float));
        c->labels.assign(labels_host, labels_host + c->N);
        c->labels_dev.alloc(c->N);
        h2d(c, c->labels_dev.p, c->labels.data(), c->N);
        c->idx.build(c->labels.data(), c->N);
        const int npv = (int)c->idx.pos.size() - c->idx.n_pos_trn, nnv = (int)c->idx.neg.size() - c->idx.n_neg_trn;
        c->val_pos_ids.alloc(std::max(npv, 1)); c->val_neg_ids.alloc(std::max(nnv, 1));
        if (npv > 0) h2d(c, c->val_pos_ids.p, c->idx.pos.data() + c->idx.n_pos_trn, (size_t)npv * sizeof(int32_t));
        if (nnv > 0) h2d(c, c->val_neg_ids.p, c->idx.neg.data() + c->idx.n_neg_trn, (size_t)nnv * sizeof(int32_t));
        c->vdist.alloc((size_t)c->N + 16);
        c->hrows.alloc((size_t)std::max(npv, 1));
        if (c->roc) roc_work_destroy(c->roc);
        c->roc = roc_work_create(c->N);
        c->have_data = true;
    });
}

int dlco_pr_get_index(const dlco_pr_ctx *c, int32_t *n_pos, int32_t *n_pos_trn, int32_t *n_neg, int32_t *n_neg_trn)
{
    if (!c || !c->have_data) return DLCO_ERR_INVALID;
    if (n_pos) *n_pos = (int32_t)c->idx.pos.size();
    if (n_neg) *n_neg = (int32_t)c->idx.neg.size();
    if (n_pos_trn) *n_pos_trn = c->idx.n_pos_trn;
    if (n_neg_trn) *n_neg_trn = c->idx.n_neg_trn;
    return DLCO_OK;
}

// n iterations of the loop body, src/pr-learn.cpp:302-329 (one launch; the sample list of the window is
// drawn on the host from the reference's generator, iPos then iNeg per iteration)
int dlco_pr_steps(dlco_pr_ctx *c, uint32_t n)
{
    if (!c) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_HIP(hipSetDevice(c->device));
        DLCO_CHECK(c->have_data, DLCO_ERR_INVALID, "dlco_pr_steps: no data set");
        DLCO_CHECK(c->idx.n_pos_trn > 0 && c->idx.n_neg_trn > 0, DLCO_ERR_INVALID, "dlco_pr_steps: empty training split");
        if (n == 0) return;
        if (n > c->win_cap) {
            sync(c);
            c->win_cap = std::max<size_t>(n, 1024);
            c->win_pos.alloc(c->win_cap); c->win_neg.alloc(c->win_cap);
        }
        draw_window(c->rng, c->idx, n, c->h_pos, c->h_neg);
        h2d(c, c->win_pos.p, c->h_pos.data(), (size_t)n * sizeof(int32_t));
        h2d(c, c->win_neg.p, c->h_neg.data(), (size_t)n * sizeof(int32_t));
        const bool ok = pr_steps(c->dists.p, c->F, c->win_pos.p, c->win_neg.p, n, c->t, c->mu, c->gamma, c->F, c->w.p, c->df.p, nullptr,
                                 c->stream);
        DLCO_CHECK(ok, DLCO_ERR_INVALID, "dlco_pr_steps: shape not supported");
        c->t += n;
    });
}

int dlco_pr_get_state(dlco_pr_ctx *c, uint32_t *t, float *w_host, float *dfavg_host)
{
    if (!c) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        if (t) *t = c->t;
        if (w_host) d2h(c, w_host, c->w.p, (size_t)c->F * sizeof(float));
        if (dfavg_host) d2h(c, dfavg_host, c->df.p, (size_t)c->F * sizeof(float));
    });
}

int dlco_pr_set_state(dlco_pr_ctx *c, uint32_t t, const float *w_host, const float *dfavg_host)
{
    if (!c) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        c->t = t;
        if (w_host) h2d(c, c->w.p, w_host, (size_t)c->F * sizeof(float));
        if (dfavg_host) h2d(c, c->df.p, dfavg_host, (size_t)c->F * sizeof(float));
    });
}

// src/pr-learn.cpp:340-361: validation objective on the current w
int dlco_pr_validate(dlco_pr_ctx *c, float *loss_val, float *regul, int32_t *nnz)
{
    if (!c || !loss_val || !regul) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_HIP(hipSetDevice(c->device));
        DLCO_CHECK(c->have_data, DLCO_ERR_INVALID, "dlco_pr_validate: no data set");
        const int npv = (int)c->idx.pos.size() - c->idx.n_pos_trn, nnv = (int)c->idx.neg.size() - c->idx.n_neg_trn;
        DLCO_CHECK(npv > 0 && nnv > 0, DLCO_ERR_INVALID, "dlco_pr_validate: empty validation split");
        float *pdv = c->vdist.p, *ndv = c->vdist.p + npv;
        pr_gemv(c->dists.p, c->F, c->val_pos_ids.p, npv, c->w.p, c->F, pdv, false, c->stream);     // :343
        pr_gemv(c->dists.p, c->F, c->val_neg_ids.p, nnv, c->w.p, c->F, ndv, false, c->stream);     // :344
        hinge_rows(pdv, npv, ndv, nnv, c->hrows.p, c->stream);                                      // :348
        sum_f32_to_f64(c->hrows.p, npv, c->dscal.p, c->stream);                                     // :351
        double total = 0.0;
        d2h(c, &total, c->dscal.p, sizeof(double));
        const float Loss = (float)total;
        *loss_val = Loss / (float)((size_t)npv * (size_t)nnv);                                      // :355
        std::vector<float> w(c->F);
        d2h(c, w.data(), c->w.p, (size_t)c->F * sizeof(float));
        regul_nnz(w.data(), c->F, c->mu, regul, nnz);                                               // :358
    });
}

// ComputePRStats (src/misc.cpp:171-264): pooling-region counts on the host, distances + ROC on the device
int dlco_pr_stats(dlco_pr_ctx *c, const float *w_host, const float *prparams_host, int32_t pr_rows, int32_t pr_cols, int32_t nchannels,
                  int32_t max_dim, int32_t *nPR, int32_t *dim, int32_t *nzdim, float *fpr95, double *auc)
{
    if (!c || !prparams_host || !nPR || !dim || !nzdim || !fpr95 || !auc) return DLCO_ERR_INVALID;
    return guarded(c, [&] {
        DLCO_HIP(hipSetDevice(c->device));
        DLCO_CHECK(c->have_data, DLCO_ERR_INVALID, "dlco_pr_stats: no data set");
        DLCO_CHECK(pr_rows >= 8 * c->F && pr_cols >= 1, DLCO_ERR_INVALID, "dlco_pr_stats: PRParams needs 8 rows per weight");
        std::vector<float> w(c->F);
        if (w_host) std::memcpy(w.data(), w_host, (size_t)c->F * sizeof(float));
        else d2h(c, w.data(), c->w.p, (size_t)c->F * sizeof(float));
        pr_counts(w.data(), c->F, prparams_host, pr_cols, nchannels, nPR, dim, nzdim);              // :183-217
        if (max_dim != -1 && *dim > max_dim) return;                        // :219-221
        const float *wd = c->w.p;
        if (w_host) { h2d(c, c->wtmp.p, w.data(), (size_t)c->F * sizeof(float)); wd = c->wtmp.p; }
        pr_gemv(c->dists.p, c->F, nullptr, c->N, wd, c->F, c->vdist.p, true, c->stream);             // :226
        roc_stats(c->roc, c->vdist.p, c->labels_dev.p, c->N, fpr95, auc, c->stream);                 // :227-263
    });
}

// ---- a grid of settings on one data set -----------------------------------------------------------

const char *dlco_pr_grid_last_error(const dlco_pr_grid *g) { return g ? g->err.c_str() : g_pr_error.c_str(); }

int dlco_pr_grid_create(dlco_pr_grid **out, dlco_pr_ctx *src, int32_t G, const float *mu, const float *gamma, uint64_t seed)
{
    if (!out) return DLCO_ERR_INVALID;
    *out = nullptr;
    dlco_pr_grid *g = nullptr;
    const int rc = guarded((dlco_pr_grid *)nullptr, [&] {
        DLCO_CHECK(src && mu && gamma, DLCO_ERR_INVALID, "dlco_pr_grid_create: NULL argument");
        DLCO_CHECK(G >= 1 && G <= 65535, DLCO_ERR_INVALID, "dlco_pr_grid_create: G must be 1 .. 65535");
        for (int k = 0; k < G; k++) DLCO_CHECK(gamma[k] > 0.f, DLCO_ERR_INVALID, "dlco_pr_grid_create: every gamma must be > 0");
        DLCO_CHECK(src->have_data, DLCO_ERR_INVALID, "dlco_pr_grid_create: src has no data");
        const int npv = (int)src->idx.pos.size() - src->idx.n_pos_trn, nnv = (int)src->idx.neg.size() - src->idx.n_neg_trn;
        DLCO_CHECK(src->idx.n_pos_trn > 0 && src->idx.n_neg_trn > 0 && npv > 0 && nnv > 0, DLCO_ERR_INVALID,
                   "dlco_pr_grid_create: empty training or validation split");
        DLCO_HIP(hipSetDevice(src->device));
        g = new dlco_pr_grid();
        g->src = src; g->F = src->F; g->N = src->N; g->G = G; g->device = src->device;
        hipDeviceProp_t prop;
        DLCO_HIP(hipGetDeviceProperties(&prop, g->device));
        g->cus = prop.multiProcessorCount;
        g->mu.assign(mu, mu + G); g->gamma.assign(gamma, gamma + G);
        g->rng = CvRng(seed);
        DLCO_HIP(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
        g->w.alloc((size_t)G * g->F); g->df.alloc((size_t)G * g->F);
        g->w.zero(g->stream); g->df.zero(g->stream);
        g->mu_dev.alloc(G); g->gamma_dev.alloc(G);
        h2d(g, g->mu_dev.p, mu, (size_t)G * sizeof(float));
        h2d(g, g->gamma_dev.p, gamma, (size_t)G * sizeof(float));
        g->vdist.alloc((size_t)G * (npv + nnv));
        g->hrows.alloc((size_t)G * npv);
        g->dscal.alloc(G);
        g->roc = roc_work_create(g->N);
        sync(g);
    });
    if (rc != DLCO_OK) { dlco_pr_grid_destroy(g); return rc; }
    *out = g;
    return DLCO_OK;
}

void dlco_pr_grid_destroy(dlco_pr_grid *g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    if (g->roc) roc_work_destroy(g->roc);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
}

int dlco_pr_grid_set_group(dlco_pr_grid *g, int32_t per_group)
{
    if (!g) return DLCO_ERR_INVALID;
    return guarded(g, [&] {
        DLCO_CHECK(per_group == 0 || per_group == 1 || per_group == 2 || per_group == 4, DLCO_ERR_INVALID,
                   "dlco_pr_grid_set_group: 0, 1, 2 or 4");
        DLCO_CHECK(per_group != 4 || g->F <= 1024 * 5, DLCO_ERR_INVALID, "dlco_pr_grid_set_group: 4 settings per workgroup need F <= 5120");
        g->group = per_group;
    });
}

int32_t dlco_pr_grid_group(const dlco_pr_grid *g)
{
    if (!g) return DLCO_ERR_INVALID;
    return g->group ? g->group : pr_grid_group(g->G, g->F, g->cus);
}

// n iterations of every setting: one window of row pairs from the grid's sampler, one launch
int dlco_pr_grid_steps(dlco_pr_grid *g, uint32_t n)
{
    if (!g) return DLCO_ERR_INVALID;
    return guarded(g, [&] {
        DLCO_HIP(hipSetDevice(g->device));
        if (n == 0) return;
        if (n > g->win_cap) {
            sync(g);
            g->win_cap = std::max<size_t>(n, 1024);
            g->win_pos.alloc(g->win_cap); g->win_neg.alloc(g->win_cap);
        }
        draw_window(g->rng, g->src->idx, n, g->h_pos, g->h_neg);
        h2d(g, g->win_pos.p, g->h_pos.data(), (size_t)n * sizeof(int32_t));
        h2d(g, g->win_neg.p, g->h_neg.data(), (size_t)n * sizeof(int32_t));
        const bool ok = pr_grid_steps(g->src->dists.p, g->F, g->win_pos.p, g->win_neg.p, n, g->t, g->mu_dev.p, g->gamma_dev.p, g->G,
                                      dlco_pr_grid_group(g), g->F, g->F, g->w.p, g->df.p, g->stream);
        DLCO_CHECK(ok, DLCO_ERR_INVALID, "dlco_pr_grid_steps: shape not supported");
        g->t += n;
    });
}

int dlco_pr_grid_get_state(dlco_pr_grid *g, uint32_t *t, float *w_host, float *dfavg_host)
{
    if (!g) return DLCO_ERR_INVALID;
    return guarded(g, [&] {
        DLCO_HIP(hipSetDevice(g->device));
        if (t) *t = g->t;
        if (w_host) d2h(g, w_host, g->w.p, (size_t)g->G * g->F * sizeof(float));
        if (dfavg_host) d2h(g, dfavg_host, g->df.p, (size_t)g->G * g->F * sizeof(float));
        if (!w_host && !dfavg_host) sync(g);
    });
}

// dlco_pr_validate for every setting: the validation rows are read once for all of them, one launch each for
// the products, the hinge rows and the double sums; regul / NNZ summed on the host in index order
int dlco_pr_grid_validate(dlco_pr_grid *g, float *loss_val, float *regul, int32_t *nnz)
{
    if (!g || !loss_val || !regul) return DLCO_ERR_INVALID;
    return guarded(g, [&] {
        DLCO_HIP(hipSetDevice(g->device));
        const dlco_pr_ctx *c = g->src;
        const int npv = (int)c->idx.pos.size() - c->idx.n_pos_trn, nnv = (int)c->idx.neg.size() - c->idx.n_neg_trn;
        const long ldv = (long)npv + nnv;
        float *pdv = g->vdist.p, *ndv = g->vdist.p + npv;
        pr_gemv_multi(c->dists.p, g->F, c->val_pos_ids.p, npv, g->w.p, g->F, nullptr, g->G, g->F, pdv, ldv, false, g->stream);   // :343
        pr_gemv_multi(c->dists.p, g->F, c->val_neg_ids.p, nnv, g->w.p, g->F, nullptr, g->G, g->F, ndv, ldv, false, g->stream);   // :344
        hinge_rows_batched(pdv, npv, ndv, nnv, ldv, g->hrows.p, npv, g->G, g->stream);                                           // :348
        sum_f32_to_f64_batched(g->hrows.p, npv, npv, g->dscal.p, g->G, g->stream);                                                // :351
        std::vector<double> total(g->G);
        d2h(g, total.data(), g->dscal.p, (size_t)g->G * sizeof(double));
        std::vector<float> w((size_t)g->G * g->F);
        d2h(g, w.data(), g->w.p, w.size() * sizeof(float));
        for (int k = 0; k < g->G; k++) {
            const float Loss = (float)total[k];
            loss_val[k] = Loss / (float)((size_t)npv * (size_t)nnv);                                                              // :355
            regul_nnz(w.data() + (size_t)k * g->F, g->F, g->mu[k], regul + k, nnz ? nnz + k : nullptr);                           // :358
        }
    });
}

// ComputePRStats for the settings configs[0..n) (repeats allowed): counts on the host per setting, the all-N
// distances of those that pass max_dim in one pass over the rows, then the ROC per setting
int dlco_pr_grid_stats(dlco_pr_grid *g, const int32_t *configs, int32_t n, const float *w_host, const float *prparams_host, int32_t pr_rows,
                       int32_t pr_cols, int32_t nchannels, int32_t max_dim, int32_t *nPR, int32_t *dim, int32_t *nzdim, float *fpr95, double *auc)
{
    if (!g || !configs || !prparams_host || !nPR || !dim || !nzdim || !fpr95 || !auc) return DLCO_ERR_INVALID;
    return guarded(g, [&] {
        DLCO_HIP(hipSetDevice(g->device));
        DLCO_CHECK(n >= 0, DLCO_ERR_INVALID, "dlco_pr_grid_stats: n < 0");
        for (int i = 0; i < n; i++) DLCO_CHECK(configs[i] >= 0 && configs[i] < g->G, DLCO_ERR_INVALID, "dlco_pr_grid_stats: config out of range");
        DLCO_CHECK(pr_rows >= 8 * g->F && pr_cols >= 1, DLCO_ERR_INVALID, "dlco_pr_grid_stats: PRParams needs 8 rows per weight");
        if (n == 0) return;
        const size_t F = (size_t)g->F;
        std::vector<float> w;
        if (w_host) w.assign(w_host, w_host + (size_t)n * F);
        else {
            std::vector<float> all((size_t)g->G * F);
            d2h(g, all.data(), g->w.p, all.size() * sizeof(float));
            w.resize((size_t)n * F);
            for (int i = 0; i < n; i++) std::memcpy(w.data() + i * F, all.data() + (size_t)configs[i] * F, F * sizeof(float));
        }
        std::vector<int32_t> sel;                                    // list positions that need the ROC pass
        for (int i = 0; i < n; i++) {
            pr_counts(w.data() + i * F, g->F, prparams_host, pr_cols, nchannels, nPR + i, dim + i, nzdim + i);   // :183-217
            if (max_dim != -1 && dim[i] > max_dim) continue;                                                     // :219-221
            sel.push_back(i);
        }
        if (sel.empty()) return;
        const int ns = (int)sel.size();
        g->wtmp.alloc((size_t)n * F);
        g->sel.alloc(ns);
        g->sdist.alloc((size_t)ns * g->N);
        h2d(g, g->wtmp.p, w.data(), w.size() * sizeof(float));
        h2d(g, g->sel.p, sel.data(), sel.size() * sizeof(int32_t));
        pr_gemv_multi(g->src->dists.p, g->F, nullptr, g->N, g->wtmp.p, g->F, g->sel.p, ns, g->F, g->sdist.p, g->N, true, g->stream);   // :226
        for (int j = 0; j < ns; j++)
            roc_stats(g->roc, g->sdist.p + (size_t)j * g->N, g->src->labels_dev.p, g->N, fpr95 + sel[j], auc + sel[j], g->stream);     // :227-263
    });
}

int dlco_pr_device_name(const dlco_pr_ctx *c, char *buf, size_t cap, int *cc_major, int *cc_minor)
{
    if (!c || !buf || cap == 0) return DLCO_ERR_INVALID;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) return DLCO_ERR_HIP;
    std::snprintf(buf, cap, "%s (%s)", prop.name, prop.gcnArchName);
    if (cc_major) *cc_major = prop.major;
    if (cc_minor) *cc_minor = prop.minor;
    return DLCO_OK;
}

}  // extern "C"
