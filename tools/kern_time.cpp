// kern_time.cpp — developer micro-benchmark of the single-workgroup kernels of the tracker
// (links against libdlco.so; not part of the product or of the tests).
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -I opencv-dlco_amd/csrc tools/kern_time.cpp \
//         -L opencv-dlco_amd -ldlco -Wl,-rpath,'$ORIGIN/../opencv-dlco_amd' -o tools/kern_time
// modes: (none) everything; `small` the m x m kernels; `prod` the tracker's product passes; `gram` the fused reductions and
// L^-1 applications of CholQR / Rayleigh-Ritz against the launches they replace
#include "dlco_internal.hpp"

#include <cmath>
#include <cstdio>
#include <functional>
#include <random>
#include <string>
#include <vector>

using namespace dlco;

static float time_ms(hipStream_t s, int reps, const std::function<void()> &fn)
{
    hipEvent_t a, b;
    hipEventCreate(&a); hipEventCreate(&b);
    fn();
    hipStreamSynchronize(s);
    hipEventRecord(a, s);
    for (int i = 0; i < reps; i++) fn();
    hipEventRecord(b, s);
    hipEventSynchronize(b);
    float ms = 0.f;
    hipEventElapsedTime(&ms, a, b);
    return ms / reps;
}

// a product over a whole F x F matrix G (or, with n < F, over n of its columns), no epilogue terms
static SkinnyArgs skinny_args(const float *X, int M, const float *G, int n, int F, float *out, void *hi, void *lo, void *lo2, float *slab, int ksplit)
{
    SkinnyArgs a;
    a.X = X; a.ldx = F; a.M = M;
    a.G = G; a.ldg = F; a.N = n; a.K = F;
    a.C = out; a.ldc = F;
    a.planes.hi = hi; a.planes.lo = lo; a.planes.lo2 = lo2;
    a.slab = slab; a.ksplit = ksplit;
    return a;
}

int main(int argc, char **argv)
{
    const bool small_only = argc > 1 && std::string(argv[1]) == "small";
    const bool prod_only = argc > 1 && std::string(argv[1]) == "prod";
    hipStream_t s0;
    hipStreamCreate(&s0);
    if (prod_only) {
        // one pass of the tracker over a symmetric F x F matrix: two-way (filter) and three-way (Rayleigh-Ritz) split
        const int F = 8192, M = 96;
        std::mt19937 r0(11);
        std::normal_distribution<float> g0(0.f, 1.f);
        DevBuf<float> C, X, out, slab; DevBuf<char> ph, pl, pl2;
        C.alloc((size_t)F * F); X.alloc((size_t)128 * F); out.alloc((size_t)128 * F); slab.alloc(bf16x2_slab_floats(128, F, 8));   // the ks = 8 case below needs 8 slices
        ph.alloc(bf16x2_plane_bytes(128, F)); pl.alloc(bf16x2_plane_bytes(128, F)); pl2.alloc(bf16x2_plane_bytes(128, F));
        std::vector<float> h((size_t)128 * F);
        for (auto &x : h) x = g0(r0);
        hipMemcpy(X.p, h.data(), h.size() * 4, hipMemcpyHostToDevice);
        for (int i = 0; i < 64; i++) hipMemcpy(C.p + (size_t)i * 128 * F, h.data(), h.size() * 4, hipMemcpyHostToDevice);
        const SkinnyArgs two = skinny_args(X.p, M, C.p, F, F, out.p, ph.p, pl.p, nullptr, slab.p, 0);
        const SkinnyArgs three = skinny_args(X.p, M, C.p, F, F, out.p, ph.p, pl.p, pl2.p, slab.p, 0);
        const SkinnyArgs two8 = skinny_args(X.p, M, C.p, F, F, out.p, ph.p, pl.p, nullptr, slab.p, 8);
        const float a = time_ms(s0, 30, [&] { skinny_product_bf16x2(two, s0); });
        const float b = time_ms(s0, 30, [&] { skinny_product_bf16x2(three, s0); });
        const float c8 = time_ms(s0, 30, [&] { skinny_product_bf16x2(two8, s0); });
        {   // symmetric G as packed upper tiles: every tile fetched once (skinny_sym_kernel)
            DevBuf<float> Gp, slab4, X160, out160; DevBuf<char> qh, ql;
            Gp.alloc(syrk_packed_floats(F)); slab4.alloc((size_t)4 * 160 * F); X160.alloc((size_t)160 * F); out160.alloc((size_t)160 * F);
            qh.alloc(bf16x2_plane_bytes(160, F)); ql.alloc(bf16x2_plane_bytes(160, F));
            hipMemcpy(X160.p, h.data(), (size_t)128 * F * 4, hipMemcpyHostToDevice);
            hipMemcpy(X160.p + (size_t)128 * F, h.data(), (size_t)32 * F * 4, hipMemcpyHostToDevice);
            syrk_pack_upper(C.p, F, F, Gp.p, s0);
            const SkinnyArgs sym2 = skinny_args(X.p, M, Gp.p, F, F, out.p, ph.p, pl.p, nullptr, slab4.p, 0);
            const SkinnyArgs sym3 = skinny_args(X.p, M, Gp.p, F, F, out.p, ph.p, pl.p, pl2.p, slab4.p, 0);
            const SkinnyArgs sym160 = skinny_args(X160.p, 160, Gp.p, F, F, out160.p, qh.p, ql.p, nullptr, slab4.p, 0);
            const SkinnyArgs full160 = skinny_args(X160.p, 160, C.p, F, F, out160.p, qh.p, ql.p, nullptr, slab4.p, 0);
            const float y2 = time_ms(s0, 30, [&] { skinny_product_sym(sym2, s0); });
            const float y3 = time_ms(s0, 30, [&] { skinny_product_sym(sym3, s0); });
            const float y5 = time_ms(s0, 30, [&] { skinny_product_sym(sym160, s0); });
            const float z5 = time_ms(s0, 30, [&] { skinny_product_bf16x2(full160, s0); });
            std::printf("SYMMETRIC product on packed upper tiles (136 MB): M=96 two-way %.1f us, three-way %.1f us; M=160 two-way %.1f us (full-matrix kernel %.1f us)  [split + kernel + reduce]\n",
                        y2 * 1e3, y3 * 1e3, y5 * 1e3, z5 * 1e3);
        }
        std::printf("product M=%d F=%d: two-way %.1f us (%.2f TB/s), three-way %.1f us (%.2f TB/s), two-way ks=8 %.1f us  [split + kernel + reduce]\n", M, F,
                    a * 1e3, 4.0 * F * F / (a * 1e-3) / 1e12, b * 1e3, 4.0 * F * F / (b * 1e-3) / 1e12, c8 * 1e3);
        return 0;
    }
    if (argc > 1 && std::string(argv[1]) == "gram") {
        // `kern_time gram`: the reduction of a symmetric product that also emits the Gram partials (reduce_gram_kernel) against
        // the two launches it replaces (ordered reduce, Gram GEMM); the ordered reduce of the Gram slab follows both forms
        const int M = 96;
        for (int F : {640, 8192}) {
            const int chunk = F == 8192 ? 128 : 64, slices = F / chunk;      // eig_rules::gram_slicing at these widths
            DevBuf<float> slab, C, E1, E2, Q, gslab, T;
            slab.alloc((size_t)4 * M * F); C.alloc((size_t)M * F); E1.alloc((size_t)M * F); E2.alloc((size_t)M * F); Q.alloc((size_t)M * F);
            gslab.alloc((size_t)slices * M * M); T.alloc((size_t)M * M);
            std::mt19937 r0(5);
            std::normal_distribution<float> g0(0.f, 1.f);
            std::vector<float> h((size_t)4 * M * F);
            for (auto &x : h) x = g0(r0);
            hipMemcpy(slab.p, h.data(), h.size() * 4, hipMemcpyHostToDevice);
            for (float *p : {E1.p, E2.p, Q.p}) hipMemcpy(p, h.data() + (p == Q.p ? 1000 : 0), (size_t)M * F * 4, hipMemcpyHostToDevice);
            for (int with = 0; with < 2; with++) {
                SkinnyArgs a;
                a.M = M; a.N = F; a.K = F; a.C = C.p; a.ldc = F; a.slab = slab.p;
                a.alpha = -0.4f; a.E1 = E1.p; a.b1 = 0.2f; a.E2 = E2.p; a.b2 = -1.0f;
                a.gram_slab = gslab.p; a.gram_chunk = chunk; a.gram_with = with ? Q.p : nullptr; a.gram_ld = F;
                GemmArgs g;
                g.M = M; g.N = M; g.K = F;
                g.A.p = C.p; g.A.ld = F; g.B.p = with ? Q.p : C.p; g.B.ld = F;
                g.C = T.p; g.ldc = M; g.split_k = slices; g.slab = gslab.p;
                bool ok = true;
                const float pair = time_ms(s0, 200, [&] { splitk_reduce_f32(slab.p, 4, M, F, C.p, F, a.alpha, 0.f, a.E1, a.b1, a.E2, a.b2, s0); gemm_f32(g, s0); });
                const float fused = time_ms(s0, 200, [&] { ok = reduce_gram_sym(a, s0) && ok; splitk_reduce_f32(gslab.p, slices, M, M, T.p, M, 1.0f, 0.f, nullptr, 0.f, nullptr, 0.f, s0); });
                const float tail = time_ms(s0, 200, [&] { splitk_reduce_f32(gslab.p, slices, M, M, T.p, M, 1.0f, 0.f, nullptr, 0.f, nullptr, 0.f, s0); });
                std::printf("gram F=%4d M=%d %s: reduce + Gram GEMM + Gram reduce %.1f us; reduce_gram%s + Gram reduce %.1f us; the Gram reduce alone %.1f us\n", F, M,
                            with ? "C * Q^T" : "C * C^T", pair * 1e3, ok ? "" : " (REFUSED)", fused * 1e3, tail * 1e3);
            }
            // CholQR's dst = Linv * src: the column-slab kernel against the GEMM plus the launch it feeds (the Gram GEMM of the
            // second pass, or the three-way split of the result)
            DevBuf<float> Linv; DevBuf<char> ph, pl, pl2;
            Linv.alloc((size_t)M * M);
            ph.alloc(bf16x2_plane_bytes(M, F)); pl.alloc(bf16x2_plane_bytes(M, F)); pl2.alloc(bf16x2_plane_bytes(M, F));
            hipMemcpy(Linv.p, h.data() + 77, (size_t)M * M * 4, hipMemcpyHostToDevice);
            GemmArgs ap;
            ap.M = M; ap.N = F; ap.K = M;
            ap.A.p = Linv.p; ap.A.ld = M; ap.B.p = Q.p; ap.B.ld = F; ap.B.kmajor = true;
            ap.C = C.p; ap.ldc = F;
            GemmArgs g2;
            g2.M = M; g2.N = M; g2.K = F;
            g2.A.p = C.p; g2.A.ld = F; g2.B.p = C.p; g2.B.ld = F;
            g2.C = T.p; g2.ldc = M; g2.split_k = slices; g2.slab = gslab.p;
            LinvApplyArgs la;
            la.Linv = Linv.p; la.ldl = M; la.n = M; la.F = F; la.src = Q.p; la.dst = C.p; la.ld = F;
            LinvApplyArgs la1 = la, la2 = la;
            la1.gram_slab = gslab.p; la1.gram_chunk = chunk;
            la2.planes.hi = ph.p; la2.planes.lo = pl.p; la2.planes.lo2 = pl2.p;
            bool ok = true;
            const float p1 = time_ms(s0, 200, [&] { gemm_f32(ap, s0); gemm_f32(g2, s0); });
            const float f1 = time_ms(s0, 200, [&] { ok = linv_apply_slab(la1, s0) && ok; splitk_reduce_f32(gslab.p, slices, M, M, T.p, M, 1.0f, 0.f, nullptr, 0.f, nullptr, 0.f, s0); });
            const float p2 = time_ms(s0, 200, [&] { gemm_f32(ap, s0); split_planes_bf16(C.p, F, M, F, ph.p, pl.p, pl2.p, s0); });
            const float f2 = time_ms(s0, 200, [&] { ok = linv_apply_slab(la2, s0) && ok; });
            std::printf("apply F=%4d M=%d: L^-1 GEMM + Gram GEMM + Gram reduce %.1f us; linv_apply%s + Gram reduce %.1f us;  L^-1 GEMM + three-way split %.1f us; linv_apply with planes %.1f us\n",
                        F, M, p1 * 1e3, ok ? "" : " (REFUSED)", f1 * 1e3, p2 * 1e3, f2 * 1e3);
        }
        return 0;
    }
    hipStream_t s;
    hipStreamCreate(&s);
    std::mt19937 rng(7);
    std::normal_distribution<float> nd(0.f, 1.f);
    const bool big = argc > 2 && std::string(argv[2]) == "big";      // `kern_time small big`: the transient's block sizes too
    for (int n : {32, 64, 70, 96, 97, 128, 150, 160, 200, 256, 400, 800}) {
        if (n > 160 && !big) break;
        // ---- Cholesky inverse on M = B B^T (rows of B random, nearly orthogonal after scaling) ----
        const int K = 512, ld = 1024;
        std::vector<double> B((size_t)n * K);
        for (auto &x : B) x = nd(rng);
        std::vector<float> M((size_t)n * ld, 0.f);
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
                double acc = 0;
                for (int k = 0; k < K; k++) acc += B[(size_t)i * K + k] * B[(size_t)j * K + k];
                M[(size_t)i * ld + j] = (float)(acc / K);
            }
        if (n <= CHOL_INV_MAX_N) {
        DevBuf<float> dM, dL; DevBuf<int> dead;
        dM.alloc(M.size()); dL.alloc(M.size()); dead.alloc(CHOL_INV_MAX_N);
        hipMemcpy(dM.p, M.data(), M.size() * 4, hipMemcpyHostToDevice);
        hipMemset(dL.p, 0, M.size() * 4);
        const float ms = time_ms(s, 200, [&] { chol_inverse128(dM.p, ld, n, 1e-5f, dL.p, ld, dead.p, s); });
        std::vector<float> L(M.size());
        hipMemcpy(L.data(), dL.p, M.size() * 4, hipMemcpyDeviceToHost);
        double err = 0;
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++) {
                double acc = 0;                                   // (Linv M Linv^T)_ij
                for (int a = 0; a < n; a++) {
                    double t = 0;
                    for (int b = 0; b < n; b++) t += (double)M[(size_t)a * ld + b] * L[(size_t)j * ld + b];
                    acc += (double)L[(size_t)i * ld + a] * t;
                }
                err = std::max(err, std::fabs(acc - (i == j ? 1.0 : 0.0)));
            }
        std::printf("chol_inverse128 n=%3d  %.1f us  |Linv M Linv^T - I|max = %.2e\n", n, ms * 1e3, err);
        if (n % 32 == 0) {
            // phase stamps of the eliminating wave (the build with stamps; one launch after a warm one)
            constexpr int NP = 6;
            static const char *const phase[NP] = {"D to LDS + barrier", "2a elimination of D", "3a rows/columns to LDS + barrier",
                                                  "2b T by columns + barrier", "3b P and F + barrier", "4 trailing update"};
            DevBuf<unsigned long long> tr;
            tr.alloc(CHOL_INV_STAMPS);
            std::vector<unsigned long long> h(CHOL_INV_STAMPS);
            for (int rep = 0; rep < 2; rep++) {
                hipMemsetAsync(tr.p, 0, CHOL_INV_STAMPS * 8, s);
                chol_inverse128_stamped(dM.p, ld, n, 1e-5f, dL.p, ld, dead.p, tr.p, s);
                hipStreamSynchronize(s);
            }
            hipMemcpy(h.data(), tr.p, CHOL_INV_STAMPS * 8, hipMemcpyDeviceToHost);
            const int ns = (int)h[0];
            const double cyc_per_us = (double)(h[ns] - h[1]) / ((double)(h[CHOL_INV_STAMPS - 1] - h[CHOL_INV_STAMPS - 2]) / 100.0);
            std::printf("  chol phases n=%3d (s_memtime cycles of wave 0, %.0f cycles/us, stamped build %.1f us from first to last stamp)\n", n,
                        cyc_per_us, (double)(h[ns] - h[1]) / cyc_per_us);
            std::printf("    %-36s %8llu\n", "load, fast-path test", h[2] - h[1]);
            for (int b = 0; b < n / 32; b++)
                for (int p = 0; p < NP; p++) {
                    const int i = 2 + NP * b + p;
                    if (i + 1 <= ns - 1) std::printf("    block %d  %-28s %8llu\n", b, phase[p], h[i + 1] - h[i]);
                }
            std::printf("    %-36s %8llu\n", "barrier, scale and store", h[ns] - h[ns - 1]);
        }
        }

        // ---- Jacobi on a nearly diagonal symmetric matrix (steady-state Rayleigh-Ritz); eigenvectors = ROWS of V ----
        std::vector<float> T((size_t)n * ld, 0.f);
        for (int i = 0; i < n; i++)
            for (int j = 0; j <= i; j++) {
                const float v = (i == j) ? (1.0f - 0.9f * i / n) : 2e-3f * nd(rng) / std::sqrt((float)n);
                T[(size_t)i * ld + j] = v; T[(size_t)j * ld + i] = v;
            }
        DevBuf<float> dT, dV, ev, work; DevBuf<int> sw;
        dT.alloc(T.size()); dV.alloc(T.size()); ev.alloc(n + 8); work.alloc(jacobi_work_floats(n)); sw.alloc(4);
        hipMemcpy(dT.p, T.data(), T.size() * 4, hipMemcpyHostToDevice);
        const float msj = time_ms(s, n > 160 ? 5 : 100, [&] { jacobi_eigh(dT.p, ld, n, ev.p, dV.p, ld, work.p, sw.p, JACOBI_COUNT_ALL, false, s); });
        int sweeps = 0;
        hipMemcpy(&sweeps, sw.p, 4, hipMemcpyDeviceToHost);
        std::vector<float> V(T.size()), e(n);
        hipMemcpy(V.data(), dV.p, T.size() * 4, hipMemcpyDeviceToHost);
        hipMemcpy(e.data(), ev.p, n * 4, hipMemcpyDeviceToHost);
        double res = 0, orth = 0;
        for (int j = 0; j < n; j++) {
            for (int i = 0; i < n; i++) {
                double acc = 0;
                for (int k = 0; k < n; k++) acc += (double)T[(size_t)i * ld + k] * V[(size_t)j * ld + k];
                res = std::max(res, std::fabs(acc - (double)e[j] * V[(size_t)j * ld + i]));
            }
            for (int k = 0; k < n; k++) {
                double acc = 0;
                for (int i = 0; i < n; i++) acc += (double)V[(size_t)j * ld + i] * V[(size_t)k * ld + i];
                orth = std::max(orth, std::fabs(acc - (j == k ? 1.0 : 0.0)));
            }
        }
        std::printf("jacobi_eigh     n=%3d  %.1f us  sweeps %d (%.1f us/sweep)  |TV - VE|max = %.2e  |V^T V - I|max = %.2e\n", n,
                    msj * 1e3, sweeps, msj * 1e3 / std::max(1, sweeps), res, orth);
        // ---- the same on a matrix that needs large rotations: M above (eigenvalues clustered around 1) and a wide spectrum ----
        for (int kind = 0; kind < 2; kind++) {
            std::vector<float> H((size_t)n * ld, 0.f);
            for (int i = 0; i < n; i++)
                for (int j = 0; j < n; j++) {
                    if (kind == 0) { H[(size_t)i * ld + j] = M[(size_t)i * ld + j]; continue; }
                    double acc = 0;                               // B diag(10^(-6 k / K)) B^T / K: six decades
                    for (int k = 0; k < K; k++) acc += B[(size_t)i * K + k] * B[(size_t)j * K + k] * std::pow(10.0, -6.0 * k / K) * (k % 7 == 0 ? 100.0 : 1.0);
                    H[(size_t)i * ld + j] = (float)(acc / K);
                }
            hipMemcpy(dT.p, H.data(), H.size() * 4, hipMemcpyHostToDevice);
            const float msh = time_ms(s, n > 160 ? 3 : 20, [&] { jacobi_eigh(dT.p, ld, n, ev.p, dV.p, ld, work.p, sw.p, JACOBI_COUNT_ALL, false, s); });
            hipMemcpy(&sweeps, sw.p, 4, hipMemcpyDeviceToHost);
            hipMemcpy(V.data(), dV.p, T.size() * 4, hipMemcpyDeviceToHost);
            hipMemcpy(e.data(), ev.p, n * 4, hipMemcpyDeviceToHost);
            double resh = 0, orthh = 0, emax = 0;
            for (int j = 0; j < n; j++) {
                emax = std::max(emax, (double)std::fabs(e[j]));
                for (int i = 0; i < n; i++) {
                    double acc = 0;
                    for (int k = 0; k < n; k++) acc += (double)H[(size_t)i * ld + k] * V[(size_t)j * ld + k];
                    resh = std::max(resh, std::fabs(acc - (double)e[j] * V[(size_t)j * ld + i]));
                }
                for (int k = 0; k < n; k++) {
                    double acc = 0;
                    for (int i = 0; i < n; i++) acc += (double)V[(size_t)j * ld + i] * V[(size_t)k * ld + i];
                    orthh = std::max(orthh, std::fabs(acc - (j == k ? 1.0 : 0.0)));
                }
            }
            std::printf("jacobi_eigh     n=%3d  dense %s  %.1f us  sweeps %d  |HV - VE|max / |E|max = %.2e  |V^T V - I|max = %.2e\n", n,
                        kind == 0 ? "clustered" : "wide     ", msh * 1e3, sweeps, resh / emax, orthh);
        }
    }
    if (small_only) return 0;
    // ---- slab-mode kernels at the 8-GPU shape (F = 8192, slab of 1024 columns, global batch 1600+1600) ----
    {
        const int F = 8192, R = 4096, world = 8, cw = F / world;
        DevBuf<float> D, C, X, out, slab; DevBuf<int32_t> ids; DevBuf<float> w; DevBuf<int> kd; DevBuf<char> ph, pl, syrk_planes;
        D.alloc((size_t)R * F); C.alloc((size_t)F * F); X.alloc((size_t)128 * F); out.alloc((size_t)128 * F);
        slab.alloc((size_t)32 * 128 * F / 4); ids.alloc(3200); w.alloc(3200); kd.alloc(4);
        ph.alloc(bf16x2_plane_bytes(128, F)); pl.alloc(bf16x2_plane_bytes(128, F));
        syrk_planes.alloc(syrk_planes_bytes(3200, F));
        // the gradient over the first kmax list entries: the whole symmetric matrix, or (cols > 0) the column slab [cols, 2 * cols)
        auto syrk_args = [&](int kmax, float beta, int cols) {
            SyrkArgs a;
            a.D = D.p; a.ldd = F; a.ids = ids.p; a.w = w.p; a.k_dev = kd.p; a.kmax = kmax; a.F = F;
            a.alpha = 1e-3f; a.beta = beta; a.C = C.p; a.ldc = F;
            a.slab_col0 = cols; a.slab_cols = cols;
            a.planes = syrk_planes.p;
            return a;
        };
        std::vector<float> h((size_t)R * F);
        for (auto &x : h) x = 0.1f * nd(rng);
        hipMemcpy(D.p, h.data(), h.size() * 4, hipMemcpyHostToDevice);
        hipMemcpy(X.p, h.data(), (size_t)128 * F * 4, hipMemcpyHostToDevice);
        hipMemset(C.p, 0, (size_t)F * F * 4);
        std::vector<int32_t> hid(3200); std::vector<float> hw(3200);
        for (int i = 0; i < 3200; i++) { hid[i] = (int)(rng() % R); hw[i] = (float)(1 + rng() % 50); }
        hipMemcpy(ids.p, hid.data(), 3200 * 4, hipMemcpyHostToDevice);
        hipMemcpy(w.p, hw.data(), 3200 * 4, hipMemcpyHostToDevice);
        for (int K : {0, 32, 64, 128, 224, 448, 896}) {                      // fixed cost vs per-K-tile cost of the SYRK
            hipMemcpy(kd.p, &K, 4, hipMemcpyHostToDevice);
            const float a = time_ms(s, 20, [&] { syrk_rda_f32(syrk_args(3200, 0.5f, 0), s); });
            const float b0 = time_ms(s, 20, [&] { syrk_rda_f32(syrk_args(3200, 0.0f, 0), s); });
            std::printf("syrk K=%4d  symmetric full: beta=0.5 %.1f us   beta=0 (no read of the old tile) %.1f us\n", K, a * 1e3, b0 * 1e3);
        }
        for (int K : {224, 1696}) {
            hipMemcpy(kd.p, &K, 4, hipMemcpyHostToDevice);
            const float a = time_ms(s, 20, [&] { syrk_rda_f32(syrk_args(3200, 0.5f, 0), s); });
            const float b = time_ms(s, 20, [&] { syrk_rda_f32(syrk_args(3200, 0.5f, cw), s); });
            std::printf("syrk K=%4d  symmetric full %.1f us   column slab 1/%d (dense) %.1f us\n", K, a * 1e3, world, b * 1e3);
        }
        // the per-rank kernels of the same-global-batch (strong scaling) mode at G = 2, 4, 8: column slab of the gradient over the
        // 305 active rows of the c2 step, slab of a 96-row tracker product (the projection's inputs)
        for (int G : {2, 4, 8}) {
            const int cwg = F / G, K = 305;
            hipMemcpy(kd.p, &K, 4, hipMemcpyHostToDevice);
            const SkinnyArgs pslab = skinny_args(X.p, 96, C.p + cwg, cwg, F, out.p + cwg, ph.p, pl.p, nullptr, slab.p, 4 * G);
            const float a = time_ms(s, 20, [&] { syrk_rda_f32(syrk_args(416, 0.5f, cwg), s); });
            const float b = time_ms(s, 20, [&] { skinny_product_bf16x2(pslab, s); });
            const float e = time_ms(s, 20, [&] { pack_cols(slab.p, out.p, F, cwg, cwg, 96, s); unpack_cols(out.p, F, slab.p, cwg, 96, G, s); });
            std::printf("G=%d: gradient column slab (K = 305 active rows, %d dense tiles) %.1f us; product slab 96 x 8192 x %d (two-way, ks %d) %.1f us; pack + unpack %.1f us\n",
                        G, (F / 128) * (cwg / 128), a * 1e3, cwg, 4 * G, b * 1e3, e * 1e3);
        }
        for (int M : {96}) {
            const SkinnyArgs pfull = skinny_args(X.p, M, C.p, F, F, out.p, ph.p, pl.p, nullptr, slab.p, 0);
            const SkinnyArgs pslab = skinny_args(X.p, M, C.p + cw, cw, F, out.p + cw, ph.p, pl.p, nullptr, slab.p, 32);
            const float a = time_ms(s, 20, [&] { skinny_product_bf16x2(pfull, s); });
            const float b = time_ms(s, 20, [&] { skinny_product_bf16x2(pslab, s); });
            GemmArgs g;
            g.M = M; g.N = cw; g.K = F;
            g.A.p = X.p; g.A.ld = F; g.A.kmajor = false;
            g.B.p = C.p + cw; g.B.ld = F; g.B.kmajor = true;
            g.C = out.p + cw; g.ldc = F; g.split_k = 32; g.slab = slab.p;
            const float c = time_ms(s, 20, [&] { gemm_f32(g, s); });
            std::printf("product M=%d  bf16x2 full %.1f us, slab 1/%d (ks 32) %.1f us;  fp32 slab (gemm split 32) %.1f us\n",
                        M, a * 1e3, world, b * 1e3, c * 1e3);
            const float e = time_ms(s, 20, [&] { pack_cols(slab.p, out.p, F, cw, cw, M, s); unpack_cols(out.p, F, slab.p, cw, M, world, s); });
            std::printf("pack + unpack %.1f us\n", e * 1e3);
        }
    }
    return 0;
}
