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

// What training, validation and statistics read and never write: Distance [N,F], Label [N], the index split and
// the validation row ids of one context.
struct PrData {
    int F = 0, N = 0;
    bool have = false;
    DevBuf<float> dists;
    DevBuf<uint8_t> labels_dev;
    DevBuf<int32_t> val_pos_ids, val_neg_ids;
    PairIndex idx;
    int npv() const { return (int)idx.pos.size() - idx.n_pos_trn; }
    int nnv() const { return (int)idx.neg.size() - idx.n_neg_trn; }
};

// A chain set: G settings (mu[k], gamma[k]) trained together from w = dfAvg = 0 at t = 0 on one stream with one
// sampler.  w and dfAvg are [G][F] (rows of F floats, 16-byte aligned since F % 4 == 0; no padding).
struct PrChains {
    int G = 0, device = 0, cus = 0;
    int group = 0;                                    // settings per workgroup, 0 = pr_grid_group's rule
    bool solo = false;                                // a context's own chain: launches the single-setting kernels
    hipStream_t stream = nullptr;
    std::vector<float> mu, gamma;
    DevBuf<float> mu_dev, gamma_dev, w, df, vdist, hrows, wtmp, sdist;
    DevBuf<int32_t> win_pos, win_neg, sel;
    DevBuf<double> dscal;
    std::vector<int32_t> h_pos, h_neg;
    CvRng rng{2215};
    uint32_t t = 0;
    RocWork *roc = nullptr;

    // on the current device, which is `device`
    void init(int G_, const float *mu_, const float *gamma_, uint64_t seed, int F, int N, int device_, int cus_);
    // the validation and statistics workspaces for the data d (a split may be empty; statistics of more than one
    // setting at a time grow theirs on demand)
    void fit(const PrData &d)
    {
        vdist.alloc((size_t)G * std::max(d.npv() + d.nnv(), 1));
        hrows.alloc((size_t)G * std::max(d.npv(), 1));
        wtmp.alloc(d.F);
        sdist.alloc(d.N);
    }
    int per_group(int F) const { return group ? group : pr_grid_group(G, F, cus); }
    ~PrChains()
    {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (roc) roc_work_destroy(roc);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

struct dlco_pr_ctx {
    PrData data;
    PrChains ch;                                      // G = 1
    std::string err;
};

// trains on the data of `src` (not copied); never touches src's chain
struct dlco_pr_grid {
    const PrData *data = nullptr;
    PrChains ch;
    std::string err;
};

static thread_local std::string g_pr_error;

namespace {

// The body of an entry point on a live context or grid: makes its device current, runs fn and turns an exception
// into its code and a message that starts with the entry point's name.
template <typename H, typename Fn>
int entry(H *h, const char *who, Fn &&fn)
{
    return guarded_call(g_pr_error, &h->err, [&] {
        try {
            DLCO_HIP(hipSetDevice(h->ch.device));
            fn();
        } catch (const Error &e) {
            throw Error(e.code, std::string(who) + ": " + e.what());
        } catch (const std::exception &e) {
            throw Error(DLCO_ERR_INVALID, std::string(who) + ": " + e.what());
        }
    });
}

void sync(hipStream_t s) { DLCO_HIP(hipStreamSynchronize(s)); }
void h2d(hipStream_t s, void *dst, const void *src, size_t bytes)
{
    DLCO_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    sync(s);
}
void d2h(hipStream_t s, void *dst, const void *src, size_t bytes)
{
    DLCO_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    sync(s);
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

void PrChains::init(int G_, const float *mu_, const float *gamma_, uint64_t seed, int F, int N, int device_, int cus_)
{
    G = G_; device = device_; cus = cus_;
    mu.assign(mu_, mu_ + G); gamma.assign(gamma_, gamma_ + G);
    rng = CvRng(seed);
    DLCO_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    w.alloc((size_t)G * F); df.alloc((size_t)G * F);
    w.zero(stream); df.zero(stream);                              // src/pr-learn.cpp:195-196
    mu_dev.alloc(G); gamma_dev.alloc(G);
    h2d(stream, mu_dev.p, mu_, (size_t)G * sizeof(float));
    h2d(stream, gamma_dev.p, gamma_, (size_t)G * sizeof(float));
    dscal.alloc(G);
    roc = roc_work_create(N);
    sync(stream);
}

namespace {

// n iterations of the loop body, src/pr-learn.cpp:302-329, for every setting: one window of row pairs drawn on the
// host from the chain set's sampler, one launch
void steps(PrChains &ch, const PrData &d, uint32_t n)
{
    if (n == 0) return;
    if (n > ch.win_pos.n) {
        sync(ch.stream);
        ch.win_pos.alloc(std::max<size_t>(n, 1024)); ch.win_neg.alloc(std::max<size_t>(n, 1024));
    }
    draw_window(ch.rng, d.idx, n, ch.h_pos, ch.h_neg);
    h2d(ch.stream, ch.win_pos.p, ch.h_pos.data(), (size_t)n * sizeof(int32_t));
    h2d(ch.stream, ch.win_neg.p, ch.h_neg.data(), (size_t)n * sizeof(int32_t));
    const bool ok = ch.solo ? pr_steps(d.dists.p, d.F, ch.win_pos.p, ch.win_neg.p, n, ch.t, ch.mu[0], ch.gamma[0], d.F, ch.w.p, ch.df.p, nullptr,
                                       ch.stream)
                            : pr_grid_steps(d.dists.p, d.F, ch.win_pos.p, ch.win_neg.p, n, ch.t, ch.mu_dev.p, ch.gamma_dev.p, ch.G,
                                            ch.per_group(d.F), d.F, d.F, ch.w.p, ch.df.p, ch.stream);
    DLCO_CHECK(ok, DLCO_ERR_INVALID, "shape not supported");
    ch.t += n;
}

// w_host / dfavg_host [G][F] or NULL; synchronises the stream either way
void get_state(PrChains &ch, const PrData &d, uint32_t *t, float *w_host, float *dfavg_host)
{
    const size_t bytes = (size_t)ch.G * d.F * sizeof(float);
    if (t) *t = ch.t;
    if (w_host) d2h(ch.stream, w_host, ch.w.p, bytes);
    if (dfavg_host) d2h(ch.stream, dfavg_host, ch.df.p, bytes);
    if (!w_host && !dfavg_host) sync(ch.stream);
}

void set_state(PrChains &ch, const PrData &d, uint32_t t, const float *w_host, const float *dfavg_host)
{
    const size_t bytes = (size_t)ch.G * d.F * sizeof(float);
    ch.t = t;
    if (w_host) h2d(ch.stream, ch.w.p, w_host, bytes);
    if (dfavg_host) h2d(ch.stream, ch.df.p, dfavg_host, bytes);
}

// src/pr-learn.cpp:340-361, the validation objective on the current w of every setting (loss_val, regul [G], nnz [G]
// or NULL): the validation rows are read once for all settings, one launch each for the products, the hinge rows and
// the double sums; regul / NNZ summed on the host in index order
void validate(PrChains &ch, const PrData &d, float *loss_val, float *regul, int32_t *nnz)
{
    const int npv = d.npv(), nnv = d.nnv(), G = ch.G, F = d.F;
    DLCO_CHECK(npv > 0 && nnv > 0, DLCO_ERR_INVALID, "empty validation split");
    const long ldv = (long)npv + nnv;
    float *pdv = ch.vdist.p, *ndv = ch.vdist.p + npv;
    if (ch.solo) {
        pr_gemv(d.dists.p, F, d.val_pos_ids.p, npv, ch.w.p, F, pdv, false, ch.stream);                         // :343
        pr_gemv(d.dists.p, F, d.val_neg_ids.p, nnv, ch.w.p, F, ndv, false, ch.stream);                         // :344
    } else {
        pr_gemv_multi(d.dists.p, F, d.val_pos_ids.p, npv, ch.w.p, F, nullptr, G, F, pdv, ldv, false, ch.stream);
        pr_gemv_multi(d.dists.p, F, d.val_neg_ids.p, nnv, ch.w.p, F, nullptr, G, F, ndv, ldv, false, ch.stream);
    }
    hinge_rows_batched(pdv, npv, ndv, nnv, ldv, ch.hrows.p, npv, G, ch.stream);                                // :348
    sum_f32_to_f64_batched(ch.hrows.p, npv, npv, ch.dscal.p, G, ch.stream);                                    // :351
    std::vector<double> total(G);
    d2h(ch.stream, total.data(), ch.dscal.p, (size_t)G * sizeof(double));
    std::vector<float> w((size_t)G * F);
    d2h(ch.stream, w.data(), ch.w.p, w.size() * sizeof(float));
    for (int k = 0; k < G; k++) {
        const float Loss = (float)total[k];
        loss_val[k] = Loss / (float)((size_t)npv * (size_t)nnv);                                               // :355
        regul_nnz(w.data() + (size_t)k * F, F, ch.mu[k], regul + k, nnz ? nnz + k : nullptr);                  // :358
    }
}

// ComputePRStats (src/misc.cpp:171-264) for the settings configs[0..n) (repeats allowed) with w_host [n][F] or NULL
// (their current w): counts on the host per setting, the all-N distances of those that pass max_dim in one pass over
// the rows, then the ROC per setting.  Every output is an array of n; fpr95 / auc of a setting cut by max_dim stay.
void stats(PrChains &ch, const PrData &d, const int32_t *configs, int32_t n, const float *w_host, const float *prparams_host, int32_t pr_rows,
           int32_t pr_cols, int32_t nchannels, int32_t max_dim, int32_t *nPR, int32_t *dim, int32_t *nzdim, float *fpr95, double *auc)
{
    DLCO_CHECK(n >= 0, DLCO_ERR_INVALID, "n < 0");
    for (int i = 0; i < n; i++) DLCO_CHECK(configs[i] >= 0 && configs[i] < ch.G, DLCO_ERR_INVALID, "config out of range");
    DLCO_CHECK(pr_rows >= 8 * d.F && pr_cols >= 1, DLCO_ERR_INVALID, "PRParams needs 8 rows per weight");
    if (n == 0) return;
    const size_t F = (size_t)d.F;
    std::vector<float> w;
    if (w_host) w.assign(w_host, w_host + (size_t)n * F);
    else {
        std::vector<float> all((size_t)ch.G * F);
        d2h(ch.stream, all.data(), ch.w.p, all.size() * sizeof(float));
        w.resize((size_t)n * F);
        for (int i = 0; i < n; i++) std::memcpy(w.data() + i * F, all.data() + (size_t)configs[i] * F, F * sizeof(float));
    }
    std::vector<int32_t> sel;                                    // list positions that need the ROC pass
    for (int i = 0; i < n; i++) {
        pr_counts(w.data() + i * F, d.F, prparams_host, pr_cols, nchannels, nPR + i, dim + i, nzdim + i);   // :183-217
        if (max_dim != -1 && dim[i] > max_dim) continue;                                                    // :219-221
        sel.push_back(i);
    }
    if (sel.empty()) return;
    const int ns = (int)sel.size();
    ch.wtmp.alloc((size_t)n * F);
    ch.sel.alloc(ns);
    ch.sdist.alloc((size_t)ns * d.N);
    h2d(ch.stream, ch.wtmp.p, w.data(), w.size() * sizeof(float));
    h2d(ch.stream, ch.sel.p, sel.data(), sel.size() * sizeof(int32_t));
    if (ch.solo) pr_gemv(d.dists.p, d.F, nullptr, d.N, ch.wtmp.p, d.F, ch.sdist.p, true, ch.stream);                      // :226
    else pr_gemv_multi(d.dists.p, d.F, nullptr, d.N, ch.wtmp.p, d.F, ch.sel.p, ns, d.F, ch.sdist.p, d.N, true, ch.stream);
    for (int j = 0; j < ns; j++)
        roc_stats(ch.roc, ch.sdist.p + (size_t)j * d.N, d.labels_dev.p, d.N, fpr95 + sel[j], auc + sel[j], ch.stream);    // :227-263
}

}  // namespace

extern "C" {

const char *dlco_pr_last_error(const dlco_pr_ctx *c) { return c ? c->err.c_str() : g_pr_error.c_str(); }

int dlco_pr_create(dlco_pr_ctx **out, int32_t F, int32_t N, float mu, float gamma, uint64_t seed, int32_t device)
{
    if (!out) return DLCO_ERR_INVALID;
    *out = nullptr;
    dlco_pr_ctx *c = nullptr;
    const int rc = guarded_call(g_pr_error, nullptr, [&] {
        DLCO_CHECK(F >= 4 && F % 4 == 0 && F <= 8192, DLCO_ERR_INVALID, "pr-learn: F must be a multiple of 4, at most 8192");
        DLCO_CHECK(N >= 2 && gamma > 0.f, DLCO_ERR_INVALID, "pr-learn: N >= 2 and gamma > 0 required");
        const hipDeviceProp_t prop = use_gfx950_device(device);
        c = new dlco_pr_ctx();
        c->data.F = F; c->data.N = N;
        c->ch.init(1, &mu, &gamma, seed, F, N, device, prop.multiProcessorCount);
        c->ch.solo = true;
    });
    if (rc != DLCO_OK) { delete c; return rc; }
    *out = c;
    return DLCO_OK;
}

void dlco_pr_destroy(dlco_pr_ctx *c) { delete c; }

// Uploads Distance [N,F] and Label [N]; index build, shuffle and 80/20 split as src/pr-learn.cpp:229-253.  A split may
// come out empty: the context then refuses at dlco_pr_steps / dlco_pr_validate, not here.
int dlco_pr_set_data(dlco_pr_ctx *c, const float *dists_host, const uint8_t *labels_host)
{
    if (!c || !dists_host || !labels_host) return DLCO_ERR_INVALID;
    return entry(c, "dlco_pr_set_data", [&] {
        PrData &d = c->data;
        const hipStream_t s = c->ch.stream;
        d.dists.alloc((size_t)d.N * d.F);
        h2d(s, d.dists.p, dists_host, (size_t)d.N * d.F * sizeof(float));
        d.labels_dev.alloc(d.N);
        h2d(s, d.labels_dev.p, labels_host, d.N);
        d.idx.build(labels_host, d.N);
        const int npv = d.npv(), nnv = d.nnv();
        d.val_pos_ids.alloc(std::max(npv, 1)); d.val_neg_ids.alloc(std::max(nnv, 1));
        if (npv > 0) h2d(s, d.val_pos_ids.p, d.idx.pos.data() + d.idx.n_pos_trn, (size_t)npv * sizeof(int32_t));
        if (nnv > 0) h2d(s, d.val_neg_ids.p, d.idx.neg.data() + d.idx.n_neg_trn, (size_t)nnv * sizeof(int32_t));
        c->ch.fit(d);
        d.have = true;
    });
}

int dlco_pr_get_index(const dlco_pr_ctx *c, int32_t *n_pos, int32_t *n_pos_trn, int32_t *n_neg, int32_t *n_neg_trn)
{
    if (!c || !c->data.have) return DLCO_ERR_INVALID;
    const PairIndex &idx = c->data.idx;
    if (n_pos) *n_pos = (int32_t)idx.pos.size();
    if (n_neg) *n_neg = (int32_t)idx.neg.size();
    if (n_pos_trn) *n_pos_trn = idx.n_pos_trn;
    if (n_neg_trn) *n_neg_trn = idx.n_neg_trn;
    return DLCO_OK;
}

int dlco_pr_steps(dlco_pr_ctx *c, uint32_t n)
{
    if (!c) return DLCO_ERR_INVALID;
    return entry(c, "dlco_pr_steps", [&] {
        DLCO_CHECK(c->data.have, DLCO_ERR_INVALID, "no data set");
        DLCO_CHECK(c->data.idx.n_pos_trn > 0 && c->data.idx.n_neg_trn > 0, DLCO_ERR_INVALID, "empty training split");
        steps(c->ch, c->data, n);
    });
}

int dlco_pr_get_state(dlco_pr_ctx *c, uint32_t *t, float *w_host, float *dfavg_host)
{
    if (!c) return DLCO_ERR_INVALID;
    return entry(c, "dlco_pr_get_state", [&] { get_state(c->ch, c->data, t, w_host, dfavg_host); });
}

int dlco_pr_set_state(dlco_pr_ctx *c, uint32_t t, const float *w_host, const float *dfavg_host)
{
    if (!c) return DLCO_ERR_INVALID;
    return entry(c, "dlco_pr_set_state", [&] { set_state(c->ch, c->data, t, w_host, dfavg_host); });
}

int dlco_pr_validate(dlco_pr_ctx *c, float *loss_val, float *regul, int32_t *nnz)
{
    if (!c || !loss_val || !regul) return DLCO_ERR_INVALID;
    return entry(c, "dlco_pr_validate", [&] {
        DLCO_CHECK(c->data.have, DLCO_ERR_INVALID, "no data set");
        validate(c->ch, c->data, loss_val, regul, nnz);
    });
}

int dlco_pr_stats(dlco_pr_ctx *c, const float *w_host, const float *prparams_host, int32_t pr_rows, int32_t pr_cols, int32_t nchannels,
                  int32_t max_dim, int32_t *nPR, int32_t *dim, int32_t *nzdim, float *fpr95, double *auc)
{
    if (!c || !prparams_host || !nPR || !dim || !nzdim || !fpr95 || !auc) return DLCO_ERR_INVALID;
    return entry(c, "dlco_pr_stats", [&] {
        DLCO_CHECK(c->data.have, DLCO_ERR_INVALID, "no data set");
        const int32_t only = 0;
        stats(c->ch, c->data, &only, 1, w_host, prparams_host, pr_rows, pr_cols, nchannels, max_dim, nPR, dim, nzdim, fpr95, auc);
    });
}

// ---- a grid of settings on one data set -----------------------------------------------------------

const char *dlco_pr_grid_last_error(const dlco_pr_grid *g) { return g ? g->err.c_str() : g_pr_error.c_str(); }

int dlco_pr_grid_create(dlco_pr_grid **out, dlco_pr_ctx *src, int32_t G, const float *mu, const float *gamma, uint64_t seed)
{
    if (!out) return DLCO_ERR_INVALID;
    *out = nullptr;
    dlco_pr_grid *g = nullptr;
    const int rc = guarded_call(g_pr_error, nullptr, [&] {
        DLCO_CHECK(src && mu && gamma, DLCO_ERR_INVALID, "dlco_pr_grid_create: NULL argument");
        DLCO_CHECK(G >= 1 && G <= 65535, DLCO_ERR_INVALID, "dlco_pr_grid_create: G must be 1 .. 65535");
        for (int k = 0; k < G; k++) DLCO_CHECK(gamma[k] > 0.f, DLCO_ERR_INVALID, "dlco_pr_grid_create: every gamma must be > 0");
        const PrData &d = src->data;
        DLCO_CHECK(d.have, DLCO_ERR_INVALID, "dlco_pr_grid_create: src has no data");
        DLCO_CHECK(d.idx.n_pos_trn > 0 && d.idx.n_neg_trn > 0 && d.npv() > 0 && d.nnv() > 0, DLCO_ERR_INVALID,
                   "dlco_pr_grid_create: empty training or validation split");
        DLCO_HIP(hipSetDevice(src->ch.device));
        g = new dlco_pr_grid();
        g->data = &d;
        g->ch.init(G, mu, gamma, seed, d.F, d.N, src->ch.device, src->ch.cus);
        g->ch.fit(d);
    });
    if (rc != DLCO_OK) { delete g; return rc; }
    *out = g;
    return DLCO_OK;
}

void dlco_pr_grid_destroy(dlco_pr_grid *g) { delete g; }

int dlco_pr_grid_set_group(dlco_pr_grid *g, int32_t per_group)
{
    if (!g) return DLCO_ERR_INVALID;
    return entry(g, "dlco_pr_grid_set_group", [&] {
        DLCO_CHECK(per_group == 0 || per_group == 1 || per_group == 2 || per_group == 4, DLCO_ERR_INVALID, "0, 1, 2 or 4");
        DLCO_CHECK(per_group != 4 || g->data->F <= 1024 * 5, DLCO_ERR_INVALID, "4 settings per workgroup need F <= 5120");
        g->ch.group = per_group;
    });
}

int32_t dlco_pr_grid_group(const dlco_pr_grid *g)
{
    if (!g) return DLCO_ERR_INVALID;
    return g->ch.per_group(g->data->F);
}

int dlco_pr_grid_steps(dlco_pr_grid *g, uint32_t n)
{
    if (!g) return DLCO_ERR_INVALID;
    return entry(g, "dlco_pr_grid_steps", [&] { steps(g->ch, *g->data, n); });
}

int dlco_pr_grid_get_state(dlco_pr_grid *g, uint32_t *t, float *w_host, float *dfavg_host)
{
    if (!g) return DLCO_ERR_INVALID;
    return entry(g, "dlco_pr_grid_get_state", [&] { get_state(g->ch, *g->data, t, w_host, dfavg_host); });
}

int dlco_pr_grid_validate(dlco_pr_grid *g, float *loss_val, float *regul, int32_t *nnz)
{
    if (!g || !loss_val || !regul) return DLCO_ERR_INVALID;
    return entry(g, "dlco_pr_grid_validate", [&] { validate(g->ch, *g->data, loss_val, regul, nnz); });
}

int dlco_pr_grid_stats(dlco_pr_grid *g, const int32_t *configs, int32_t n, const float *w_host, const float *prparams_host, int32_t pr_rows,
                       int32_t pr_cols, int32_t nchannels, int32_t max_dim, int32_t *nPR, int32_t *dim, int32_t *nzdim, float *fpr95, double *auc)
{
    if (!g || !configs || !prparams_host || !nPR || !dim || !nzdim || !fpr95 || !auc) return DLCO_ERR_INVALID;
    return entry(g, "dlco_pr_grid_stats", [&] {
        stats(g->ch, *g->data, configs, n, w_host, prparams_host, pr_rows, pr_cols, nchannels, max_dim, nPR, dim, nzdim, fpr95, auc);
    });
}

int dlco_pr_device_name(const dlco_pr_ctx *c, char *buf, size_t cap, int *cc_major, int *cc_minor)
{
    if (!c || !buf || cap == 0) return DLCO_ERR_INVALID;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->ch.device) != hipSuccess) return DLCO_ERR_HIP;
    std::snprintf(buf, cap, "%s (%s)", prop.name, prop.gcnArchName);
    if (cc_major) *cc_major = prop.major;
    if (cc_minor) *cc_minor = prop.minor;
    return DLCO_OK;
}

}  // extern "C"
