// eig_tracker.cpp — host orchestration of the positive-eigenspace tracker (see the header).
#include "eig_tracker.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <initializer_list>

namespace dlco {

namespace {
inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }
}  // namespace

// Inside a filter chain the reduction of one product emits the two-way planes of its result, which is the X of the next
// product: that one then skips its split.  The chain lives as long as one filter (filter_plain).
struct EigTracker::PlaneChain {
    const float *planes_of = nullptr;   // the matrix whose two-way planes sit in plane_hi_/plane_lo_ (emitted by a reduction)
    int rows = 0;
    bool next = false;                  // the product being issued feeds the next one of the chain
};

// A product whose result goes straight into a Gram product (CholQR's first pass, the Rayleigh-Ritz T): its reduction may
// form that product's K-slice partials while the result is still on chip (skinny_product_sym).  `done` then tells the
// caller to finish with gram_finish() instead of gram_rect().
struct EigTracker::GramTail {
    const float *with = nullptr;        // the second row block; nullptr: the result itself
    bool done = false;
};

EigTracker::EigTracker(int F, int max_rows, int guard, float tol, int max_iter, hipStream_t stream, int live_cols)
    : F_(F), live_(live_cols > 0 ? std::min(live_cols, F) : F), guard_(guard), max_iter_(max_iter), tol_(tol), s_(stream)
{
    cap_ = std::min(live_, std::max(max_rows, 2 * guard + 32));
    if (guard_ > cap_ / 2) guard_ = std::max(1, cap_ / 2);
    for (int i = 0; i < 6; i++) { buf_[i].alloc((size_t)cap_ * F_); all_[i] = buf_[i].p; }
    Q_ = all_[0]; Y_ = all_[1];
    Tm_.alloc((size_t)cap_ * cap_);
    Vm_.alloc((size_t)cap_ * cap_);
    Cw_.alloc((size_t)cap_ * cap_);
    ritz_block_.alloc((size_t)2 * (cap_ + 8) + 8);
    evals_.p = ritz_block_.p;
    res_.p = ritz_block_.p + (cap_ + 8);
    sweeps_dev_ = reinterpret_cast<int *>(ritz_block_.p + 2 * (cap_ + 8));
    DLCO_HIP(hipMemsetAsync(sweeps_dev_, 0, 8 * sizeof(int), s_));   // [0] Jacobi sweeps, [4] ticket of the residual / publish kernel
    scale_.alloc(cap_ + 8);
    wscale_.alloc(cap_ + 8);
    srcrow_.alloc(cap_ + 8);
    jwork_.alloc(jacobi_work_floats(cap_));
    dead_.alloc(CHOL_INV_MAX_N);
    // K slices of a product over a full (unpacked) matrix: a divisor of the tile count, four where it divides
    {
        const int nt = F_ / 128;
        ks_ = 1;
        for (int d : {4, 2, 8, 7, 6, 5, 3})
            if (nt > 0 && nt % d == 0) { ks_ = d; break; }
    }
    // split-bf16 products (F is whole 128-column tiles): two-way planes for the filter, three-way for the Rayleigh-Ritz product
    plane_hi_.alloc(bf16x2_plane_bytes(std::min(cap_, 160), F_));
    plane_lo_.alloc(bf16x2_plane_bytes(std::min(cap_, 160), F_));
    plane_lo2_.alloc(bf16x2_plane_bytes(std::min(cap_, 128), F_));
    pv_.alloc(F_);
    pw_.alloc(F_);
    slab_floats_ = std::max((size_t)4 * cap_ * F_, (size_t)8 << 20);
    slab_floats_ = std::min(slab_floats_, (size_t)64 << 20);
    slab_floats_ = std::max(slab_floats_, (size_t)cap_ * F_);
    slab_.alloc(slab_floats_);
    pin_floats_ = (size_t)3 * cap_ + 64;                  // >= the Ritz block (2*(cap+8)+1 floats); the last 16 hold the poll flag, the 16 before them the caller's extra word
    // coherent (fine-grained) on purpose: the host polls a sequence number that a kernel writes with a
    // system-scope release; with HIP_HOST_COHERENT=0 a default allocation would only be seen at a sync
    DLCO_HIP(hipHostMalloc((void **)&pin_, pin_floats_ * sizeof(float), hipHostMallocCoherent));
    std::memset(pin_, 0, pin_floats_ * sizeof(float));
    h_theta_.assign(cap_, 0.f);
    h_res_.assign(cap_, 0.f);
}

EigTracker::~EigTracker()
{
    if (pin_) (void)hipHostFree(pin_);
}

float *EigTracker::pick(std::initializer_list<const float *> busy) const
{
    for (int i = 0; i < 6; i++) {
        bool used = false;
        for (const float *b : busy) used = used || (b == all_[i]);
        if (!used) return all_[i];
    }
    throw Error(-2, "eig tracker: no free work buffer");
}

void EigTracker::reset()
{
    m_ = 0;
    have_theta_ = false;
    have_lo_ = false;
    steps_since_lo_ = 0;
    cold_ = true;
    wext_rows_ = 0;
    ru_offered_ = false;
}

void EigTracker::seed_rows(const float *src, long ld, const int32_t *ids_dev, int n, const int32_t *ids2_dev)
{
    const int k = std::min(n, cap_);
    have_theta_ = false;
    wext_rows_ = 0;
    ru_offered_ = false;
    if (k <= 0) { m_ = 0; return; }
    scale_rows(Q_, F_, src, ld, nullptr, ids_dev, ids2_dev, k, F_, s_);
    m_ = k;
}

bool EigTracker::rank_coeff_job(RankCoeffJob *job, int kmax)
{
    if (wext_rows_ <= 0 || wext_rows_ != m_ || m_ > 160 || !packed_ || shard_ || kmax % 32 != 0) return false;
    coeff_.alloc(rank_coeff_bytes(cap_ < 160 ? cap_ : 160, kmax));
    job->nw = wext_nw_; job->m = m_; job->MT = (m_ + 31) / 32;
    job->wscale = wscale_.p; job->frag = coeff_.p;
    return true;
}

float EigTracker::next_uniform()
{
    rng_ ^= rng_ << 13; rng_ ^= rng_ >> 7; rng_ ^= rng_ << 17;
    return (float)((double)(rng_ >> 11) * (2.0 / 9007199254740992.0) - 1.0);
}

void EigTracker::append_random(float *Q, int have, int add)
{
    if (add <= 0) return;
    y_ok_ = false;
    h_tmp_.assign((size_t)add * F_, 0.f);
    for (int i = 0; i < add; i++)
        for (int j = 0; j < live_; j++) h_tmp_[(size_t)i * F_ + j] = next_uniform();   // (zero in the pad columns)
    DLCO_HIP(hipMemcpyAsync(Q + (size_t)have * F_, h_tmp_.data(), h_tmp_.size() * sizeof(float), hipMemcpyHostToDevice, s_));
    DLCO_HIP(hipStreamSynchronize(s_));
}

// out[rows][F] = alpha * X*G + b1*E1 + b2*E2     (G symmetric F x F)
void EigTracker::product(const float *X, int rows, const float *G, float alpha, float *out, const float *E1, float b1,
                         const float *E2, float b2, bool approx, PlaneChain *chain, GramTail *gram)
{
    // the split-bf16 kernels take up to 128 rows: a taller block goes through them in row chunks
    // (one HBM-bound pass over G per chunk, still cheaper than the generic fp32 GEMM)
    // (the row-streaming kernel takes 160 rows with the two-way split - a block of rank ~128 plus its guards
    // in ONE pass over G - and 96 with the three-way split; a sharded rank's slab kernel 128)
    const int one_pass = (approx && !shard_) ? 160 : (packed_ ? 96 : 128);   // (symmetric three-way kernel: 96 rows)
    if (rows > one_pass && (packed_ || F_ >= 256)) {
        if (chain) chain->next = false;                          // row chunks share the plane buffers: no carried planes
        const int step = approx ? (rows <= 2 * one_pass ? (rows / 2 + 31) / 32 * 32 : one_pass) : 96;
        for (int r0 = 0; r0 < rows; r0 += step) {
            const int nr = std::min(step, rows - r0);
            const size_t o = (size_t)r0 * F_;
            product(X + o, nr, G, alpha, out + o, E1 ? E1 + o : nullptr, b1, E2 ? E2 + o : nullptr, b2, approx, chain);
        }
        return;
    }
    st_.product_rows += rows;
    // what the three split-bf16 forms below share; each adds its G, N and the fields only it has
    SkinnyArgs a;
    a.X = X; a.ldx = F_; a.M = rows; a.K = F_;
    a.alpha = alpha; a.C = out; a.ldc = F_;
    a.E1 = E1; a.b1 = b1; a.E2 = E2; a.b2 = b2;
    a.planes.hi = plane_hi_.p; a.planes.lo = plane_lo_.p;
    a.planes.lo2 = approx ? nullptr : plane_lo2_.p;             // exact products: the three-way split
    a.slab = slab_.p;
    if (packed_) {
        // G = packed upper tiles: the symmetric kernel (every tile fetched once); two-way split for the filter, three-way
        // for the exact products (rows <= 96 there: the chunking above)
        if (prof_) prof_->begin(PROF_EIG_PRODUCT);
        // inside a filter chain the planes of X are those the previous product's reduction emitted
        // (an exact product right behind CholQR finds the three-way planes its second pass wrote)
        const bool ready = (approx && chain && chain->planes_of == X && chain->rows == rows) ||
                           (!approx && planes3_of_ == X && planes3_rows_ == rows);
        planes3_of_ = nullptr;                                   // whatever runs now overwrites the planes
        const bool emit = approx && chain && chain->next;
        a.G = G; a.N = F_;
        a.planes_ready = ready; a.emit_planes = emit;
        if (gram && fuse_gram_ && !emit && rows <= 96) {
            // the Gram partials go behind the product's own four slabs
            const eig_rules::GramSlicing gs = gram_slices(rows, rows);
            const size_t off = (size_t)4 * rows * F_;
            if (gs.whole(F_) && off + (size_t)gs.slices * rows * rows <= slab_floats_) {
                a.gram_with = gram->with; a.gram_ld = F_;
                a.gram_slab = slab_.p + off; a.gram_chunk = gs.chunk;
                a.gram_done = &gram->done;
            }
        }
        const bool ok = skinny_product_sym(a, s_);
        if (gram && gram->done) st_.fused_gram_reductions++;
        if (chain) { chain->planes_of = emit ? out : nullptr; chain->rows = rows; }   // (a product without `emit` has overwritten the planes with X's)
        if (prof_) prof_->end(PROF_EIG_PRODUCT);
        DLCO_CHECK(ok, -2, "eig tracker: the symmetric product rejected a shape of the packed layout");
        return;
    }
    if (shard_) {
        // the rank's column slab out[:, c0:c0+cw] = alpha * X * G[:, c0:c0+cw] + ..., then all-gather
        const int c0 = shard_->c0, cw = shard_->cw, world = shard_->world;
        DLCO_CHECK((size_t)world * rows * cw <= shard_->gather_floats, -2, "eig tracker: exchange buffer too small");
        const float *E1s = E1 ? E1 + c0 : nullptr, *E2s = E2 ? E2 + c0 : nullptr;
        if (prof_) prof_->begin(PROF_EIG_PRODUCT);
        bool done = false;
        if (rows <= 128) {
            int ks = ks_;                                            // keep ~256 workgroups in flight
            while (ks < 4 * world && F_ % (128 * ks * 2) == 0 && bf16x2_slab_floats(rows, cw, ks * 2) <= slab_floats_) ks *= 2;
            a.G = G + c0; a.ldg = F_; a.N = cw;
            a.C = out + c0; a.E1 = E1s; a.E2 = E2s;
            a.ksplit = ks;
            done = skinny_product_bf16x2(a, s_);
        }
        if (!done) {
            GemmArgs g;
            g.M = rows; g.N = cw; g.K = F_;
            g.A.p = X; g.A.ld = F_; g.A.kmajor = false;
            g.B.p = G + c0; g.B.ld = F_; g.B.kmajor = true;
            g.C = out + c0; g.ldc = F_;
            g.alpha = alpha; g.E1 = E1s; g.b1 = b1; g.E2 = E2s; g.b2 = b2;
            const long tiles = (long)ceil_div(rows, rows <= 64 ? 64 : 128) * ceil_div(cw, 128);
            g.split_k = split_k_slices(tiles, 512, F_, 256, (long)(slab_floats_ / ((size_t)rows * cw)));
            g.slab = slab_.p;
            gemm_f32(g, s_);
        }
        if (prof_) prof_->end(PROF_EIG_PRODUCT);
        pack_cols(shard_->gather + (size_t)shard_->rank * rows * cw, out, F_, c0, cw, rows, s_);
        shard_->allgather((size_t)rows * cw * sizeof(float));
        unpack_cols(out, F_, shard_->gather, cw, rows, world, s_);
        return;
    }
    if (rows <= one_pass && F_ >= 256) {
        // filter products: two-way split (~1e-5); exact products (Rayleigh-Ritz): three-way split (~1e-7)
        if (prof_) prof_->begin(PROF_EIG_PRODUCT);
        a.G = G; a.ldg = F_; a.N = F_;
        a.ksplit = ks_;
        const bool ok = skinny_product_bf16x2(a, s_);
        if (prof_) prof_->end(PROF_EIG_PRODUCT);
        if (ok) return;
    }
    GemmArgs g;
    g.M = rows; g.N = F_; g.K = F_;
    g.A.p = X; g.A.ld = F_; g.A.kmajor = false;
    g.B.p = G; g.B.ld = F_; g.B.kmajor = true;
    g.C = out; g.ldc = F_;
    g.alpha = alpha; g.E1 = E1; g.b1 = b1; g.E2 = E2; g.b2 = b2;
    const int bm = rows <= 64 ? 64 : 128;
    const long tiles = (long)ceil_div(rows, bm) * ceil_div(F_, 128);
    g.split_k = split_k_slices(tiles, 1024, F_, 256, (long)(slab_floats_ / ((size_t)rows * F_)));
    g.slab = slab_.p;
    if (prof_) prof_->begin(PROF_EIG_PRODUCT);
    gemm_f32(g, s_);
    if (prof_) prof_->end(PROF_EIG_PRODUCT);
}

// out[k_out][F] = C X with C [k_out][ldc] holding the coefficient vectors in its rows (jacobi_eigh's layout)
void EigTracker::rotate(const float *C, long ldc, int k_in, int k_out, const float *X, float *out, const float *X2, float *out2)
{
    GemmArgs g;
    g.M = k_out; g.N = F_; g.K = k_in;
    g.A.p = C; g.A.ld = ldc; g.A.kmajor = false;
    g.B.p = X; g.B.ld = F_; g.B.kmajor = true;
    g.C = out; g.ldc = F_;
    g.B2 = X2; g.C2 = out2;                                          // the Ritz step rotates Q and Y = Q H with one launch
    gemm_f32(g, s_);
}

// T[xrows][yrows] (ld cap_) = X * Y^T
void EigTracker::gram_rect(const float *X, int xrows, const float *Y, int yrows, float *T)
{
    GemmArgs g;
    g.M = xrows; g.N = yrows; g.K = F_;
    g.A.p = X; g.A.ld = F_; g.A.kmajor = false;
    g.B.p = Y; g.B.ld = F_; g.B.kmajor = false;
    g.C = T; g.ldc = cap_;
    g.split_k = gram_slices(xrows, yrows).split_k;
    g.slab = slab_.p;
    gemm_f32(g, s_);
}

eig_rules::GramSlicing EigTracker::gram_slices(int xrows, int yrows) const
{
    const long tiles = (long)ceil_div(xrows, xrows <= 64 ? 64 : 128) * ceil_div(yrows, yrows <= 64 ? 64 : 128);
    return eig_rules::gram_slicing(F_, tiles, (long)(slab_floats_ / ((size_t)xrows * yrows)));
}

// T[rows][rows] (ld cap_) from the partials a product's reduction left behind its slabs (GramTail::done): gram_rect's second launch
void EigTracker::gram_finish(int rows, float *T)
{
    splitk_reduce_f32(slab_.p + (size_t)4 * rows * F_, gram_slices(rows, rows).slices, rows, rows, T, cap_, 1.0f, 0.f, nullptr, 0.f,
                      nullptr, 0.f, s_);
}

// Wp[np][F] -= (Wp Q^T) Q for the `kept` orthonormal rows of Q
void EigTracker::project_out(float *Wp, int np, const float *Q, int kept)
{
    gram_rect(Wp, np, Q, kept, Cw_.p);
    GemmArgs g;
    g.M = np; g.N = F_; g.K = kept;
    g.A.p = Cw_.p; g.A.ld = cap_; g.A.kmajor = false;
    g.B.p = Q; g.B.ld = F_; g.B.kmajor = true;
    g.C = Wp; g.ldc = F_;
    g.alpha = -1.0f; g.beta = 1.0f;
    gemm_f32(g, s_);
}

// Orthonormalise the rows of Z in place (`scratch` is a second [rows][F] buffer); returns rows.
// Block Gram-Schmidt over panels of at most 128 rows: a panel is projected (twice) against the
// rows already accepted and renormalised, then CholQR2: Gram matrix -> L^-1 on one workgroup
// -> rows = L^-1 * rows as a GEMM, twice (Z -> scratch -> Z).  The rows arrive ordered by Ritz
// value, i.e. by how strongly the filter amplified them; the caller cuts the panels so that
// rows of different provenance or of very different amplification never share one.  Nothing
// here synchronises with the host and no row is dropped (dependent rows become zero rows).
int EigTracker::orthonormalize(float *Z, int rows, float *scratch, const std::vector<int> &panel_ends, int skip, bool gram_ready)
{
    // One panel (the steady state): Cholesky QR is invariant under a scaling of the rows - the Gram entries keep their
    // relative accuracy, the dead-row rule compares a pivot with the row's own diagonal entry - so the rows go in as the
    // filter left them.  With several panels the rows are normalised first: the Gram-Schmidt step between panels zeroes
    // what is left of a row after projection against a threshold that assumes unit rows.
    const bool one_panel = is_one_panel(rows, panel_ends, skip);
    DLCO_CHECK(!gram_ready || one_panel, -2, "eig tracker: Gram partials were formed for a block that is not one panel");
    if (!one_panel) row_normalize(Z + (size_t)skip * F_, F_, rows - skip, F_, 0.f, s_);
    size_t pi = 0;
    bool applied = false;                                        // the last L^-1 application was the column-slab kernel
    // (the first `skip` rows are orthonormal as they are - locked Ritz vectors - and only serve as the span the panels
    // behind them are projected against)
    for (int p0 = skip; p0 < rows;) {
        while (pi < panel_ends.size() && panel_ends[pi] <= p0) pi++;
        int pend = pi < panel_ends.size() ? std::min(rows, panel_ends[pi]) : rows;
        if (pend - p0 > CHOL_INV_MAX_N) pend = p0 + CHOL_INV_MAX_N;
        const int np = pend - p0;
        float *Wp = Z + (size_t)p0 * F_, *Sp = scratch + (size_t)p0 * F_;
        if (p0 > 0) {
            for (int pass = 0; pass < 2; pass++) {
                project_out(Wp, np, Z, p0);
                // after the first projection, rows that lie (to fp32 accuracy) inside the span above are zeroed
                row_normalize(Wp, F_, np, F_, pass == 0 ? 2e-5f : 0.f, s_);
            }
        }
        for (int pass = 0; pass < 2; pass++) {
            const float *src = pass == 0 ? Wp : Sp;
            float *dst = pass == 0 ? Sp : Wp;
            if (gram_ready && pass == 0) gram_finish(np, Tm_.p);   // the last filter product's reduction formed the partials
            else if (applied && pass == 1) gram_finish(np, Tm_.p);   // ... the first pass's application did
            else gram_rect(src, np, src, np, Tm_.p);
            chol_inverse128(Tm_.p, cap_, np, 1e-5f, Vm_.p, cap_, dead_.p, s_);
            if (one_panel && fuse_apply_ && packed_ && !shard_) {
                // dst = Linv * src by column slabs; the first pass leaves the Gram partials of the second, the second the
                // three-way planes of the block for the exact product of the Rayleigh-Ritz step
                LinvApplyArgs la;
                la.Linv = Vm_.p; la.ldl = cap_; la.n = np; la.F = F_;
                la.src = src; la.dst = dst; la.ld = F_;
                const eig_rules::GramSlicing gs = gram_slices(np, np);
                const size_t off = (size_t)4 * np * F_;
                bool fits = np <= 96;
                if (pass == 0) {
                    fits = fits && gs.whole(F_) && off + (size_t)gs.slices * np * np <= slab_floats_;
                    la.gram_slab = slab_.p + off; la.gram_chunk = gs.chunk;
                } else {
                    la.planes.hi = plane_hi_.p; la.planes.lo = plane_lo_.p; la.planes.lo2 = plane_lo2_.p;
                }
                applied = fits && linv_apply_slab(la, s_);
                if (applied) {
                    st_.fused_applications++;
                    if (pass == 1) { planes3_of_ = dst; planes3_rows_ = np; }
                    continue;
                }
            }
            GemmArgs g;                                           // dst = Linv * src
            g.M = np; g.N = F_; g.K = np;
            g.A.p = Vm_.p; g.A.ld = cap_; g.A.kmajor = false;
            g.B.p = src; g.B.ld = F_; g.B.kmajor = true;
            g.C = dst; g.ldc = F_;
            gemm_f32(g, s_);
        }
        p0 = pend;
    }
    return rows;
}

// Remove rows that the orthonormalisation zeroed (they surface as exact-zero Ritz pairs).
int EigTracker::drop_dead_rows()
{
    std::vector<int32_t> live;
    for (int i = 0; i < m_; i++)
        if (!(h_theta_[i] == 0.f && h_res_[i] == 0.f)) live.push_back(i);
    const int k = (int)live.size();
    if (k == m_ || k == 0) return m_;
    DLCO_HIP(hipMemcpyAsync(srcrow_.p, live.data(), (size_t)k * sizeof(int32_t), hipMemcpyHostToDevice, s_));
    DLCO_HIP(hipStreamSynchronize(s_));
    float *Qn = pick({Q_, Y_});
    scale_rows(Qn, F_, Q_, F_, nullptr, srcrow_.p, nullptr, k, F_, s_);
    float *Yn = pick({Q_, Y_, Qn});
    scale_rows(Yn, F_, Y_, F_, nullptr, srcrow_.p, nullptr, k, F_, s_);
    Q_ = Qn; Y_ = Yn;
    for (int j = 0; j < k; j++) { h_theta_[j] = h_theta_[live[j]]; h_res_[j] = h_res_[live[j]]; }
    m_ = k;
    return k;
}

// Power iteration for lambda_max(G); the lower end of H = -G is -lambda_max(G).
void EigTracker::refresh_lower_bound(const float *G, int iters, float theta_top)
{
    static const float kZero = 0.f;
    const bool cold = !have_lo_;
    if (cold) {
        std::vector<float> v(F_, 0.f);
        for (int i = 0; i < live_; i++) v[i] = next_uniform();
        DLCO_HIP(hipMemcpyAsync(pv_.p, v.data(), F_ * sizeof(float), hipMemcpyHostToDevice, s_));
        DLCO_HIP(hipStreamSynchronize(s_));
        row_normalize(pv_.p, F_, 1, F_, 0.f, s_);
    }
    DLCO_HIP(hipMemcpyAsync(scale_.p, &kZero, sizeof(float), hipMemcpyHostToDevice, s_));   // theta = 0: plain norm
    auto run = [&](float shift, int n) -> float {
        float *v = pv_.p, *w = pw_.p;
        for (int i = 0; i < n; i++) {
            if (shard_ || packed_) product(v, 1, G, 1.0f, w, nullptr, 0.f, nullptr, 0.f, false);   // v^T G = (G v)^T, G symmetric
            else symv(G, F_, F_, v, w, s_);
            if (shift != 0.f) axpby_inplace(w, v, 1.0f, shift, F_, s_);
            if (i == n - 1) residual_norms(v, w, F_, scale_.p, 1, F_, res_.p, s_);   // |w|
            row_normalize(w, F_, 1, F_, 0.f, s_);
            std::swap(v, w);
        }
        if (v != pv_.p) DLCO_HIP(hipMemcpyAsync(pv_.p, v, F_ * sizeof(float), hipMemcpyDeviceToDevice, s_));
        DLCO_HIP(hipMemcpyAsync(pin_, res_.p, sizeof(float), hipMemcpyDeviceToHost, s_));
        DLCO_HIP(hipStreamSynchronize(s_));
        return pin_[0];
    };
    // |G v| <= spectral radius; the shift must dominate -lambda_min(G) = top eigenvalue of H
    const float rho = run(0.f, cold ? 12 : 2);
    const float shift = std::max(cold ? 2.0f * rho : 1.05f * rho, 1.1f * std::max(theta_top, 0.f)) + 1e-30f;
    const float top = run(shift, iters) - shift;        // <= lambda_max(G), tight once converged
    const float lam_max = std::max(top, 0.f);
    lo_bound_ = -(1.3f * lam_max + 0.05f * std::max(rho, theta_top)) - 1e-12f;
    have_lo_ = true;
    steps_since_lo_ = 0;
}

// What one update() carries from stage to stage.
struct EigTracker::UpdateState {
    const float *G = nullptr;        // update()'s arguments
    float mu = 0.f, cscale = 0.f;
    float *W = nullptr;
    float tol = 0.f;                 // tolerance of this update (a quarter of tol_ when the block is cold)
    bool ru_ok = false;              // the caller's rank update may form the first filter term of pass 0
    int ru_nw = 0;                   // Ritz rows of the W its projections were made with
    int it = 0;                      // pass
    int nw = 0;                      // Ritz pairs above mu as of the last pass
    int n_ritz = 0;                  // leading rows that are Ritz vectors with a known theta
    float theta_top = 0.f, block_min = 0.f;
    bool conv = false, cheap_done = false;
    bool w_emitted = false;          // the last pass's residual kernel has written W (all rows of that pass's block, scales too)
    bool gram_wanted = false;        // the filtered block goes into CholQR as one panel: its last product may form the Gram partials
    bool gram_ready = false;         // ... and did
    eig_rules::FilterPlan plan;      // of the current pass
    std::vector<int> panel_ends;
};

eig_rules::Block EigTracker::block_of(const UpdateState &u) const
{
    eig_rules::Block b;
    b.theta = h_theta_.data(); b.res = h_res_.data();
    b.m = m_; b.live = live_; b.guard = guard_;
    b.mu = u.mu; b.cscale = u.cscale; b.tol = u.tol;
    return b;
}

int EigTracker::update(const float *G, float mu, float cscale, float *W, double *trace, bool *converged)
{
    st_.updates++;
    UpdateState u;
    u.G = G; u.mu = mu; u.cscale = cscale; u.W = W;
    open_update(u);                                                  // seed an empty block, refresh the lower bound
    for (; u.it < max_iter_; u.it++) {
        u.plan = eig_rules::plan_filter(block_of(u), u.n_ritz, u.nw, u.it, deg0_, lo_bound_, u.block_min, u.theta_top, lock_,
                                        !u.cheap_done && y_ok_, last_crit_);
        // (the panels depend on the plan alone: cut before the filter, which has to know whether one panel follows it)
        eig_rules::cut_panels(block_of(u), u.n_ritz, u.plan, CHOL_INV_MAX_N, u.panel_ends);
        u.gram_wanted = is_one_panel(m_, u.panel_ends, u.plan.n_lock);
        u.gram_ready = false;
        float *Z = Q_;
        if (u.plan.cheap) { u.cheap_done = true; Z = filter_cheap(u); }
        else if (u.plan.n_lock > 0) Z = filter_locked(u);
        else if (u.plan.filtered) Z = filter_plain(u);
        if (u.plan.filtered) last_deg_ = u.plan.d;
        orthonormalize(Z, m_, pick({Z}), u.panel_ends, u.plan.n_lock, u.gram_ready);   // in place
        rayleigh_ritz(u, Z);
        judge(u);
        // a block whose positive eigenspace reaches into its guards grows; a full one that cannot
        // cannot certify the rank: the reference keeps EVERY positive eigen-direction
        // (src/pj-learn.cpp:480-484), so this is reported, never silently truncated
        const bool crowded = m_ < live_ && eig_rules::reaches_guards(u.nw, m_, guard_);
        if (crowded) u.conv = false;
        if (crowded && m_ < cap_) { grow(u); continue; }
        if (crowded || u.conv) { u.it++; break; }
    }
    const double tr = trim_and_emit(u);
    if (converged) *converged = u.conv;
    if (trace) *trace = tr;
    return u.nw;
}

void EigTracker::open_update(UpdateState &u)
{
    // The caller may have told what changed: G = beta G_prev + alpha X_a^T diag(w) X_a (offer_rank_update).  With Y_ = Q_ H_prev
    // still there from the last Rayleigh-Ritz step and the projections of X_a on exactly these rows, the first filter
    // term needs no pass over G (kernels_rankupd.hip).
    u.ru_ok = ru_offered_ && y_ok_ && have_theta_ && packed_ && !shard_ && wext_rows_ == m_ &&
              ru_.rows == m_ && m_ >= 1 && m_ <= 160 && m_ < live_ && ru_.proj && ru_.planes;
    ru_offered_ = false;
    u.ru_nw = wext_nw_;
    wext_rows_ = 0;                                                  // W is rewritten by this update
    y_ok_ = false;                                                   // G changed since the last Rayleigh-Ritz step
    if (m_ == 0) {
        m_ = std::min(cap_, 2 * guard_ + 32);
        append_random(Q_, 0, m_);
        have_theta_ = false;
    }
    u.theta_top = have_theta_ ? h_theta_[0] : 0.f;
    u.block_min = have_theta_ ? std::min(h_theta_[m_ - 1], u.mu) : u.mu;
    u.n_ritz = have_theta_ ? m_ : 0;
    steps_since_lo_++;
    if (!have_lo_) refresh_lower_bound(u.G, 30, u.theta_top);
    else if (steps_since_lo_ >= eig_rules::lower_bound_period(st_.updates)) refresh_lower_bound(u.G, 6, u.theta_top);

    // A block that has just been (re)started - the first step of a run, a teacher-forced state - has no accuracy of
    // earlier steps to lean on: in the steady state a step inherits Ritz vectors that already met the tolerance and the
    // measured error of A+ sits 5-10x below it (1.5e-5 / 3.6e-5 at eig_tol = 2e-4 on the two full-width workloads),
    // while a cold block stops right AT the tolerance (1-2e-4).  The cold update therefore converges to a quarter of
    // it; it happens once per run.
    u.tol = cold_ ? 0.25f * tol_ : tol_;
    cold_ = false;
}

// The degree-1 pass: (H - c0) Q / e0 = (Y - c0 Q) / e0 from the Y = Q H the last Rayleigh-Ritz step left, no product
float *EigTracker::filter_cheap(const UpdateState &u)
{
    const float c0 = u.plan.c0, e0 = u.plan.e0;
    axpby_inplace(Y_, Q_, 1.0f / e0, -c0 / e0, (size_t)m_ * F_, s_);
    y_ok_ = false;
    st_.cheap_passes++;
    return Y_;
}

// the recurrence on the rows below the locked ones, every term cleaned of the locked span (its top
// components would otherwise grow by ~2 x_top per product against ~2 x_j for the rows' own); no carried
// planes here: the projection changes a term after its product's reduction has split it
float *EigTracker::filter_locked(const UpdateState &u)
{
    const float c0 = u.plan.c0, e0 = u.plan.e0;
    const int n_lock = u.plan.n_lock, na = m_ - n_lock;
    const size_t off = (size_t)n_lock * F_;
    y_ok_ = false;
    const float *prev = Q_;
    float *cur = pick({Q_, Y_});
    product(Q_ + off, na, u.G, -1.0f / e0, cur + off, Q_ + off, -c0 / e0, nullptr, 0.f, true);
    project_out(cur + off, na, Q_, n_lock);
    for (int k = 2; k <= u.plan.d; k++) {
        float *nxt = pick({Q_, prev, cur});
        product(cur + off, na, u.G, -2.0f / e0, nxt + off, cur + off, -2.0f * c0 / e0, prev + off, -1.0f, true);
        project_out(nxt + off, na, Q_, n_lock);
        prev = cur; cur = nxt;
    }
    DLCO_HIP(hipMemcpyAsync(cur, Q_, off * sizeof(float), hipMemcpyDeviceToDevice, s_));
    st_.locked_passes++;
    st_.locked_rows += n_lock;
    return cur;
}

// The three-term recurrence on the whole block; the first term comes from the step's rank update where the caller offered one
float *EigTracker::filter_plain(UpdateState &u)
{
    const float c0 = u.plan.c0, e0 = u.plan.e0;
    const int d = u.plan.d;
    const float *prev = Q_;
    float *cur = pick({Q_, Y_});
    PlaneChain chain;
    chain.next = d >= 2;                                 // the result is the X of the next product: emit its planes
    bool first_done = false;
    planes3_of_ = nullptr;
    if (u.it == 0 && u.ru_ok && u.n_ritz == m_) {
        // (H - c0) Q / e0 = (beta / e0) Y - (alpha / e0) C_w X_a - (c0 / e0) Q, H = -G
        coeff_.alloc(rank_coeff_bytes(cap_ < 160 ? cap_ : 160, ru_.kmax));
        if (prof_) prof_->begin(PROF_RANK_UPDATE);
        RankTermBlock b;
        b.Y = Y_; b.Q = Q_; b.ld = F_; b.m = m_; b.F = F_;
        b.ay = ru_.beta / e0; b.aq = -c0 / e0; b.ac = -ru_.alpha / e0;
        b.out = cur;
        b.nw = u.ru_nw; b.wscale = wscale_.p; b.coeff_ws = coeff_.p;
        b.out_planes.hi = chain.next ? plane_hi_.p : nullptr; b.out_planes.lo = plane_lo_.p;
        first_done = rank_first_term(b, ru_, s_);
        if (prof_) prof_->end(PROF_RANK_UPDATE);
        if (first_done) {
            st_.rank_update_passes++;
            chain.planes_of = chain.next ? cur : nullptr;
            chain.rows = m_;
            if (ru_check_) check_first_term(u, cur);
        }
    }
    // the last product of the recurrence is the block CholQR takes next
    GramTail tail;
    if (!first_done) product(Q_, m_, u.G, -1.0f / e0, cur, Q_, -c0 / e0, nullptr, 0.f, true, &chain, d == 1 && u.gram_wanted ? &tail : nullptr);
    for (int k = 2; k <= d; k++) {
        float *nxt = pick({prev, cur});
        chain.next = k < d;
        product(cur, m_, u.G, -2.0f / e0, nxt, cur, -2.0f * c0 / e0, prev, -1.0f, true, &chain, k == d && u.gram_wanted ? &tail : nullptr);
        prev = cur; cur = nxt;
    }
    u.gram_ready = tail.done;
    return cur;
}

// DLCO_RANK_UPDATE_CHECK (developer aid): the shortcut's first term `cur` against the product it replaces
void EigTracker::check_first_term(const UpdateState &u, const float *cur)
{
    const float c0 = u.plan.c0, e0 = u.plan.e0;
    float *ref = pick({Q_, Y_, cur});
    std::vector<char> ph(bf16x2_plane_bytes(m_, F_)), pl(ph.size());   // the check must not disturb the planes
    DLCO_HIP(hipMemcpyAsync(ph.data(), plane_hi_.p, ph.size(), hipMemcpyDeviceToHost, s_));
    DLCO_HIP(hipMemcpyAsync(pl.data(), plane_lo_.p, pl.size(), hipMemcpyDeviceToHost, s_));
    product(Q_, m_, u.G, -1.0f / e0, ref, Q_, -c0 / e0, nullptr, 0.f, true);
    std::vector<float> a((size_t)m_ * F_), b(a.size());
    DLCO_HIP(hipMemcpyAsync(a.data(), cur, a.size() * sizeof(float), hipMemcpyDeviceToHost, s_));
    DLCO_HIP(hipMemcpyAsync(b.data(), ref, b.size() * sizeof(float), hipMemcpyDeviceToHost, s_));
    DLCO_HIP(hipMemcpyAsync(plane_hi_.p, ph.data(), ph.size(), hipMemcpyHostToDevice, s_));
    DLCO_HIP(hipMemcpyAsync(plane_lo_.p, pl.data(), pl.size(), hipMemcpyHostToDevice, s_));
    DLCO_HIP(hipStreamSynchronize(s_));
    double dmax = 0.0, rmax = 0.0;
    for (size_t e = 0; e < a.size(); e++) { dmax = std::max(dmax, (double)std::fabs(a[e] - b[e])); rmax = std::max(rmax, (double)std::fabs(b[e])); }
    st_.rank_update_check = std::max(st_.rank_update_check, rmax > 0.0 ? dmax / rmax : 0.0);
    st_.product_rows -= m_;
}

// Yb = Qo * H (exact fp32) and T = Yb * Qo^T into Tm_
void EigTracker::project_block(const float *G, const float *Qo, float *Yb)
{
    GramTail tail;
    tail.with = Qo;
    product(Qo, m_, G, -1.0f, Yb, nullptr, 0.f, nullptr, 0.f, false, nullptr, &tail);
    if (tail.done) gram_finish(m_, Tm_.p);
    else gram_rect(Yb, m_, Qo, m_, Tm_.p);
}

// One panel (orthonormalize): the whole block goes through CholQR2 as it is
bool EigTracker::is_one_panel(int rows, const std::vector<int> &panel_ends, int skip)
{
    return skip == 0 && rows <= CHOL_INV_MAX_N && (panel_ends.empty() || panel_ends[0] >= rows);
}

// Rayleigh-Ritz on the orthonormal rows Qo: Q_ and Y_ = Q_ H become the Ritz vectors and their products, the Ritz
// values and residual norms come back into h_theta_ / h_res_ (one polled read-back per pass)
void EigTracker::rayleigh_ritz(UpdateState &u, float *Qo)
{
    float *Yb = pick({Qo});
    project_block(u.G, Qo, Yb);
    if (prof_) prof_->begin(PROF_JACOBI);
    const float lam_cut = eig_rules::jacobi_lam_cut(block_of(u), have_theta_ && u.n_ritz == m_);
    float *Qn = pick({Qo, Yb});
    float *Yn = pick({Qo, Yb, Qn});
    u.w_emitted = false;
    const size_t blk = (size_t)2 * (cap_ + 8) + 1;               // evals | res | sweeps in one copy
    // (second attempt: only after the multi-workgroup Jacobi gave up at its grid barrier - T, Qo and Yb are untouched
    // by a failed attempt, the m x m problem is then solved again by the single-workgroup kernel)
    for (int attempt = 0;; attempt++) {
        jacobi_eigh(Tm_.p, cap_, m_, evals_.p, Vm_.p, cap_, jwork_.p, sweeps_dev_, lam_cut, attempt > 0, s_);
        if (prof_) prof_->end(PROF_JACOBI);
        rotate(Vm_.p, cap_, m_, m_, Qo, Qn, Yb, Yn);
        Q_ = Qn; Y_ = Yn;
        y_ok_ = true;                                                // Y_ = Q_ H for the current H
        // the block is written into pinned memory by a kernel that raises a sequence number last; polling it
        // costs a few microseconds where copy + hipStreamSynchronize cost tens (one read-back per pass)
        unsigned *flag = reinterpret_cast<unsigned *>(pin_ + pin_floats_ - 16);
        const unsigned seq = ++publish_seq_;
        int *extra_host = reinterpret_cast<int *>(pin_ + pin_floats_ - 32);
        // (the residual kernel's last workgroup publishes: one launch)
        // (the kernel also writes this pass's rows of W, guard rows and scales included: if the pass is the update's last,
        // W is already where it belongs)
        ResidualPublish rp;
        rp.X = Q_; rp.Y = Y_; rp.ld = F_; rp.theta = evals_.p; rp.m = m_; rp.F = F_; rp.res = res_.p;
        rp.ticket = reinterpret_cast<unsigned *>(sweeps_dev_ + 4);
        rp.src = ritz_block_.p; rp.dst_host = pin_; rp.n = (int)blk;
        rp.flag_host = flag; rp.seq = seq;
        rp.extra_dev = extra_dev_; rp.extra_host = extra_host;
        rp.emit.W = u.W; rp.emit.ldw = F_; rp.emit.mu = u.mu; rp.emit.cscale = u.cscale;
        rp.emit.wscale = wscale_.p; rp.emit.guards = emit_guards_;
        u.w_emitted = residual_norms_publish(rp, s_);
        const auto t0 = std::chrono::steady_clock::now();
        bool seen = false;
        for (long spins = 0;; spins++) {
            if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) { seen = true; break; }
            if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) break;
        }
        if (!seen) {                                             // slow box or a faulted kernel: let the runtime tell
            DLCO_HIP(hipStreamSynchronize(s_));
            DLCO_CHECK(__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq, -3, "eig tracker: read-back did not arrive");
        }
        if (extra_dev_) extra_val_ = *reinterpret_cast<int *>(pin_ + pin_floats_ - 32);
        const int sweeps = *reinterpret_cast<int *>(pin_ + 2 * (cap_ + 8));
        if (sweeps >= 0) { st_.jacobi_sweeps += sweeps; break; }
        // the kernel wrote neither Ritz values nor V: nothing read back in this attempt may be used
        st_.jacobi_barrier_timeouts++;
        DLCO_CHECK(attempt == 0, -3, "eig tracker: the Jacobi kernel reported a failure twice (grid barrier of jacobi_mw_kernel, then the single-workgroup kernel)");
        if (prof_) prof_->begin(PROF_JACOBI);
    }
    std::memcpy(h_theta_.data(), pin_, (size_t)m_ * sizeof(float));
    std::memcpy(h_res_.data(), pin_ + (cap_ + 8), (size_t)m_ * sizeof(float));
    have_theta_ = true;
    const int before = m_;
    theta_dev_valid_ = (drop_dead_rows() == before);            // a compaction leaves evals_ on the device stale
    u.theta_top = h_theta_[0];
    u.block_min = std::min(h_theta_[m_ - 1], u.mu);
    u.n_ritz = m_;
}

void EigTracker::ortho_probe(const float *X, const float *Xprev, int m, const float *G, float alpha, float b1, float b2, int panel_end,
                             int n_lock, float *Qo, float *Yb, float *T)
{
    DLCO_CHECK(packed_ && !shard_ && m >= 1 && m <= cap_ && n_lock >= 0 && n_lock < m, -2, "eig tracker: ortho_probe needs a packed single-rank tracker that holds m rows");
    m_ = m;
    const size_t bytes = (size_t)m * F_ * sizeof(float);
    float *cur = all_[0], *prev = all_[1], *Z = all_[2], *scratch = all_[3], *Yp = all_[4];
    DLCO_HIP(hipMemcpyAsync(cur, X, bytes, hipMemcpyDeviceToDevice, s_));
    if (Xprev) DLCO_HIP(hipMemcpyAsync(prev, Xprev, bytes, hipMemcpyDeviceToDevice, s_));
    std::vector<int> panel_ends;
    if (n_lock > 0) panel_ends.push_back(n_lock);
    if (panel_end > n_lock && panel_end < m) panel_ends.push_back(panel_end);
    panel_ends.push_back(m);
    GramTail tail;
    product(cur, m, G, alpha, Z, cur, b1, Xprev ? prev : nullptr, b2, true, nullptr, is_one_panel(m, panel_ends, n_lock) ? &tail : nullptr);
    if (n_lock > 0) DLCO_HIP(hipMemcpyAsync(Z, cur, (size_t)n_lock * F_ * sizeof(float), hipMemcpyDeviceToDevice, s_));   // locked rows pass the filter untouched
    orthonormalize(Z, m, scratch, panel_ends, n_lock, tail.done);
    project_block(G, Z, Yp);
    DLCO_HIP(hipMemcpyAsync(Qo, Z, bytes, hipMemcpyDeviceToDevice, s_));
    DLCO_HIP(hipMemcpyAsync(Yb, Yp, bytes, hipMemcpyDeviceToDevice, s_));
    DLCO_HIP(hipMemcpy2DAsync(T, (size_t)m * sizeof(float), Tm_.p, (size_t)cap_ * sizeof(float), (size_t)m * sizeof(float), m,
                              hipMemcpyDeviceToDevice, s_));
    DLCO_HIP(hipStreamSynchronize(s_));
    m_ = 0;
}

void EigTracker::judge(UpdateState &u)
{
    const eig_rules::Verdict v = eig_rules::judge(block_of(u), u.it);
    u.nw = v.nw;
    u.conv = v.conv;
    last_crit_ = v.crit;
    if (debug_)
        std::fprintf(stderr, "[eig] upd %ld it %d deg %d lock %d m %d nw %d theta[%.5g .. %.5g] mu %.5g lo %.5g crit/emax %.3g guards_ok %d conv %d\n",
                     (long)st_.updates, u.it, last_deg_, u.plan.n_lock, m_, u.nw, h_theta_[0], h_theta_[m_ - 1], u.mu, lo_bound_, last_crit_,
                     (int)v.guards_ok, (int)u.conv);
    lo_bound_ = eig_rules::lowered_bound(lo_bound_, h_theta_[m_ - 1]);
}

// ---- grow the block when the positive eigenspace reaches into the guard ------------------
void EigTracker::grow(UpdateState &u)
{
    const int add = eig_rules::growth_rows(m_, cap_, guard_, u.nw);
    // half of the new rows from the caller's source (rows of the step's batch), the rest random: the directions
    // that have just risen above mu lie mostly in the span of recent batch rows, and a block that starts there
    // needs fewer passes than one that starts from noise; the random half keeps the block able to find the rest
    int got = 0;
    if (grow_cb_) got = std::max(0, std::min(add / 2, grow_cb_(Q_ + (size_t)m_ * F_, add / 2)));
    append_random(Q_, m_ + got, add - got);
    for (int i = m_; i < m_ + add; i++) { h_theta_[i] = u.block_min; h_res_[i] = 0.f; }
    m_ += add;
}

// ---- adapt the next starting degree, trim the block, emit W (ascending eigenvalue order, like LAPACK's) --------
// returns the trace of the projected A
double EigTracker::trim_and_emit(UpdateState &u)
{
    st_.iters += u.it;
    deg0_ = eig_rules::next_deg0(deg0_, u.it, u.conv, last_crit_, tol_);
    if (!u.conv) st_.nonconverged++;
    m_ = eig_rules::trimmed_rows(m_, u.nw, guard_);
    const int nw = u.nw;
    double tr = 0.0;
    if (nw > 0) {
        for (int i = 0; i < nw; i++) tr += (double)(u.cscale * (h_theta_[i] - u.mu));
        if (theta_dev_valid_) {
            // the Ritz values are still on the device in the order of the rows of Q: scale and reverse there
            const bool ext = emit_guards_ && y_ok_ && m_ > nw;
            if (!u.w_emitted) emit_w_rows(u.W, F_, Q_, F_, evals_.p, nw, u.mu, u.cscale, F_, ext ? m_ : 0, ext ? wscale_.p : nullptr, s_);
            if (ext) { wext_rows_ = m_; wext_nw_ = nw; }
        } else {
            h_sc_.resize(nw);
            h_sr_.resize(nw);
            for (int j = 0; j < nw; j++) {
                const int i = nw - 1 - j;
                h_sc_[j] = std::sqrt(u.cscale * (h_theta_[i] - u.mu));
                h_sr_[j] = i;
            }
            DLCO_HIP(hipMemcpyAsync(scale_.p, h_sc_.data(), nw * sizeof(float), hipMemcpyHostToDevice, s_));
            DLCO_HIP(hipMemcpyAsync(srcrow_.p, h_sr_.data(), nw * sizeof(int32_t), hipMemcpyHostToDevice, s_));
            DLCO_HIP(hipStreamSynchronize(s_));
            scale_rows(u.W, F_, Q_, F_, scale_.p, srcrow_.p, nullptr, nw, F_, s_);
        }
    }
    return tr;
}

}  // namespace dlco
