// dlco_internal.hpp — shared declarations for libdlco.so (gfx950 only).
// Host side C++17, device side HIP.  No torch types, no OpenCV, no CUDA shims.
#pragma once

#include "../../include/dlco.h"
#include "match_batch.hpp"
#include "match_slices.hpp"
#include "select_rules.hpp"
#include "track_rules.hpp"
#include "verify_batch.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <utility>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

namespace patch_rules { struct Frame; }                      // patch_rules.hpp

namespace dlco {

// ---------------------------------------------------------------------------
// error handling: exceptions inside the library, converted to codes at the ABI
// ---------------------------------------------------------------------------
struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

#define DLCO_HIP(expr)                                                             \
    do {                                                                           \
        hipError_t e__ = (expr);                                                   \
        if (e__ != hipSuccess)                                                     \
            throw ::dlco::Error(-3, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

#define DLCO_CHECK(cond, code, msg)                                                \
    do {                                                                           \
        if (!(cond)) throw ::dlco::Error((code), std::string(msg));                \
    } while (0)

// The body of every ABI entry point: runs fn and turns an exception into its code; the message
// goes to the calling file's thread-local string and, when there is a context, to its error string.
template <typename Fn>
int guarded_call(std::string &thread_err, std::string *ctx_err, Fn &&fn)
{
    try {
        fn();
        return DLCO_OK;
    } catch (const Error &e) {
        thread_err = e.what();
        if (ctx_err) *ctx_err = e.what();
        return e.code;
    } catch (const std::exception &e) {
        thread_err = e.what();
        if (ctx_err) *ctx_err = e.what();
        return DLCO_ERR_INVALID;
    }
}

// Makes `device` current and returns its properties; throws DLCO_ERR_NODEVICE unless it is a gfx950.
inline hipDeviceProp_t use_gfx950_device(int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device >= ndev)
        throw Error(DLCO_ERR_NODEVICE, "no usable HIP device (this library has no CPU fallback)");
    DLCO_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    DLCO_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        throw Error(DLCO_ERR_NODEVICE, std::string("device is ") + prop.gcnArchName + ", this build targets gfx950 only");
    return prop;
}

// Runtime count of 32-row tiles -> template argument: calls f(std::integral_constant<int, MT>) with MT = mt clamped to
// [1, MAX].  MAX is per call: only the forms a caller names are instantiated.
template <int MAX, typename F>
void dispatch_mt(int mt, F &&f)
{
    if constexpr (MAX > 1) {
        if (mt < MAX) return dispatch_mt<MAX - 1>(mt, f);
    }
    f(std::integral_constant<int, MAX>{});
}

// The value of one of the library's environment switches, nullptr when it is not set.  The library reads its environment
// nowhere else: the switches and what each is for are listed beside it (dlco_api.cpp); a name outside that list throws.
const char *env_switch(const char *name);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device): the attribute is per device, and contexts may
// be created on several devices and from several threads (cfg.device)
inline void ensure_dynamic_lds(const void *func, int bytes)
{
    static std::mutex mu;
    static std::vector<std::pair<const void *, int>> done;
    int dev = 0;
    DLCO_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    for (const auto &d : done)
        if (d.first == func && d.second == dev) return;
    DLCO_HIP(hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.emplace_back(func, dev);
}

// simple owning device buffer
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void alloc(size_t count) {
        if (count <= n && p) return;
        release();
        if (count == 0) count = 1;
        DLCO_HIP(hipMalloc((void **)&p, count * sizeof(T)));
        n = count;
    }
    void zero(hipStream_t s) { if (p) DLCO_HIP(hipMemsetAsync(p, 0, n * sizeof(T), s)); }
};

// ---------------------------------------------------------------------------
// HIP-event timers on the launch stream, one slot per named kernel group
// ---------------------------------------------------------------------------
enum ProfSlot { PROF_GRAD_SYRK = 0, PROF_EIG_PRODUCT = 1, PROF_JACOBI = 2, PROF_PROJECT = 3, PROF_RANK_UPDATE = 4, PROF_SLOTS = 5 };

struct Profiler {
    bool on = false;
    unsigned mask = ~0u;          // slots that record (bit per ProfSlot): every record costs a few microseconds of queue time
    hipStream_t s = nullptr;
    struct Rec { std::vector<hipEvent_t> ev; size_t used = 0; double ms = 0.0; int64_t n = 0; };
    Rec rec[PROF_SLOTS];
    ~Profiler() { for (auto &r : rec) for (hipEvent_t e : r.ev) (void)hipEventDestroy(e); }
    void mark(int slot) {
        if (!on || !((mask >> slot) & 1u)) return;
        Rec &r = rec[slot];
        // timing-only events: without the system-scope fence a default event carries (hipEventDisableSystemFence), a
        // record is a time stamp in the queue instead of a cache flush - the default form cost ~6 us of idle GPU per record
        if (r.used == r.ev.size()) { hipEvent_t e; DLCO_HIP(hipEventCreateWithFlags(&e, hipEventDisableSystemFence)); r.ev.push_back(e); }
        DLCO_HIP(hipEventRecord(r.ev[r.used++], s));
        if (r.used >= 8192 && (r.used % 2) == 0) drain(slot);
    }
    void begin(int slot) { mark(slot); }
    void end(int slot) { mark(slot); }
    void drain(int slot) {
        Rec &r = rec[slot];
        if (r.used == 0) return;
        DLCO_HIP(hipStreamSynchronize(s));
        for (size_t i = 0; i + 1 < r.used; i += 2) {
            float ms = 0.f;
            DLCO_HIP(hipEventElapsedTime(&ms, r.ev[i], r.ev[i + 1]));
            r.ms += ms; r.n++;
        }
        r.used = 0;
    }
    void drain_all() { for (int i = 0; i < PROF_SLOTS; i++) drain(i); }
    void reset() { drain_all(); for (auto &r : rec) { r.ms = 0.0; r.n = 0; } }
};

// ---------------------------------------------------------------------------
// generic fp32 MFMA GEMM (kernels_gemm.hip)
//   C[M,N] = alpha * A(M,K) * B(K,N)  (+ epilogue)
// Operand addressing:
//   A.kmajor : element (i,k) at A.p[row(k)*A.ld + i]   (memory rows run along K)
//   else     : element (i,k) at A.p[row(i)*A.ld + k]   (memory rows run along M)
//   B.kmajor : element (k,j) at B.p[row(k)*B.ld + j]
//   else     : element (k,j) at B.p[row(j)*B.ld + k]
//   row(x) = row_ids ? row_ids[x] : x ; k-major rows may carry a per-row scale.
// Epilogue:  C = alpha*acc + beta*C_in + b1*E1 + b2*E2   (E1/E2 share C's ld)
// ---------------------------------------------------------------------------
struct GemmOperand {
    const float *p = nullptr;
    long ld = 0;
    bool kmajor = false;
    const int32_t *row_ids = nullptr;
    const int32_t *row_ids2 = nullptr;  // optional: the operand row is p[row_ids[x]] - p[row_ids2[x]] (pair mode)
    const float *row_scale = nullptr;   // only for k-major operands
};

struct GemmArgs {
    int M = 0, N = 0, K = 0;
    GemmOperand A, B;
    float *C = nullptr;
    long ldc = 0;
    float alpha = 1.0f, beta = 0.0f;
    const float *E1 = nullptr;
    float b1 = 0.0f;
    const float *E2 = nullptr;
    float b2 = 0.0f;
    const int *k_dev = nullptr;         // optional device-resident K (<= K)
    int split_k = 1;                    // >1: partial slabs + ordered reduce
    float *slab = nullptr;              // workspace >= split_k*M*N floats when split_k > 1
    bool upper_only = false;            // M==N: compute tiles with j-block >= i-block, mirror the rest
    const float *B2 = nullptr;          // twin product in the same launch: C2 = alpha * A * B2 (+ the same epilogue terms), B2 laid
    float *C2 = nullptr;                // out like B; needs split_k == 1
    bool small_m_tiles = false;         // 64-row tiles whatever M ...
    bool small_n_tiles = false;         // ... and 64-column tiles whatever N: the 96 x 400 batch projection fills 64 x 64 tiles to 67 %, 64 x 128 ones to 58 % (-6 us)
    int depth = 0;                      // K tiles in flight: 0 = gemm_f32's own choice (what every library path passes), 1 = one; same bits
    int *depth_used = nullptr;          // host pointer, optional: the depth the launch ran with
};

void gemm_f32(const GemmArgs &a, hipStream_t s);
// K tiles gemm_f32 keeps in flight at depth 0 where it takes 64-wide tiles of plain operands (elsewhere: 1)
int gemm_ring_depth();
// Same product on the bf16 matrix cores with split operands (x = hi + lo, three MFMAs per term,
// fp32 accumulation; ~1e-5 relative error): kernels_bf16x2.hip.  The planes are workspaces of
// bf16x2_plane_bytes(M, K) bytes each.  Returns false for unsupported shapes (the caller then takes gemm_f32).
size_t bf16x2_plane_bytes(int M, int K);
size_t bf16x2_slab_floats(int M, int N, int ksplit);     // ksplit as in SkinnyArgs (0: the default four slices)
// fragment-ordered bf16 planes of X [M][K] (M <= 160): hi, lo (and lo2 when given); layout: split_bf16_dev.hpp
void split_planes_bf16(const float *X, long ldx, int M, int K, void *hi, void *lo, void *lo2, hipStream_t s);
// The plane workspaces of a split operand.  lo2 != nullptr selects the three-way split (x = hi + mid + lo, six MFMAs
// per term): fp32-level accuracy.
struct SplitPlanes {
    void *hi = nullptr, *lo = nullptr, *lo2 = nullptr;
};
// C[M][N] = alpha * X[M][K] * G + b1*E1 + b2*E2 (E1/E2 share C's ld), for skinny_product_bf16x2 and skinny_product_sym
struct SkinnyArgs {
    const float *X = nullptr;
    long ldx = 0;
    int M = 0;
    const float *G = nullptr;           // bf16x2: [K][ldg], N of its columns; sym: the packed upper tiles (ldg unused)
    long ldg = 0;
    int N = 0, K = 0;                   // sym: N == K == F
    float alpha = 1.0f;
    float *C = nullptr;
    long ldc = 0;
    const float *E1 = nullptr;
    float b1 = 0.0f;
    const float *E2 = nullptr;
    float b2 = 0.0f;
    SplitPlanes planes;                 // workspaces of bf16x2_plane_bytes(M, K) bytes each for the planes of X
    float *slab = nullptr;              // bf16x2: >= bf16x2_slab_floats(M, N, ksplit) floats; sym: >= 4*M*F
    int ksplit = 0;                     // bf16x2: number of K slices (grid y, 0 = the default 4); K must be a multiple of 128 * ksplit.
                                        // A column slab of G (N < K) takes ksplit = 4 * K / N so that the launch still fills the chip.
    // sym only.  planes_ready: the planes already hold the split of X, two-way or, with planes.lo2, three-way (skip the split); emit_planes: the reduction
    // also writes the two-way planes of the RESULT into planes.hi / lo (the next product of a Chebyshev chain takes it as X)
    bool planes_ready = false;
    bool emit_planes = false;
    // sym only, M <= 96, without emit_planes.  gram_slab != nullptr: the reduction also writes the raw K-slice partials
    // [K / gram_chunk][M][M] of C * C^T (gram_with == nullptr) or of C * gram_with^T (gram_with [M][gram_ld]), bit for bit
    // what gemm_f32 puts into its slab for that product split into slices of gram_chunk (64 or 128) columns; the caller
    // finishes with splitk_reduce_f32.  *gram_done (host, optional) is set when that form ran; otherwise the plain
    // reduction ran and the caller forms the Gram product itself.
    const float *gram_with = nullptr;
    long gram_ld = 0;
    float *gram_slab = nullptr;
    int gram_chunk = 0;
    bool *gram_done = nullptr;
};
bool skinny_product_bf16x2(const SkinnyArgs &a, hipStream_t s);
// P1 + P2 for many rows without the r x N projection (kernels_project.hip): dist[n] = |W x_n|^2, x_n = row ids[n] (or
// row0 + n) of D, minus row ids2[n] in pair mode.  Three-way split-bf16 MFMA (fp32-level accuracy) or, with bf16 = true,
// operands rounded to bf16 once (BASELINE configs[4]).  planes: workspaces of project_rows_plane_bytes(F) bytes each.
size_t project_rows_plane_bytes(int K);
struct ProjectRowsArgs {
    const float *W = nullptr;           // [r][ldw]
    long ldw = 0;
    int r = 0;
    const float *D = nullptr;
    long ldd = 0;
    int F = 0;
    const int32_t *ids = nullptr, *ids2 = nullptr;
    long row0 = 0;                      // sqdist form without ids: the rows row0 .. row0 + nrows of D
    int nrows = 0;
    SplitPlanes planes;                 // all three are used (bf16: hi and lo only)
    bool bf16 = false;
    float *dist = nullptr;              // project_rows_sqdist: out [nrows]
    float *slab = nullptr;              // project_rows_slab: out [ksplit][r][ldn]
    long ldn = 0;
    int ksplit = 1;
};
bool project_rows_sqdist(const ProjectRowsArgs &a, hipStream_t s);
// raw partial projections of a few rows (ids required), K split over ksplit slices: slab [ksplit][r][ldn] (r <= 96)
bool project_rows_slab(const ProjectRowsArgs &a, hipStream_t s);
// The coefficient fragments of the rank-update first filter term (kernels_rankupd.hip), as a job that rides in the
// gradient's row-split launch (its extra column of blocks): frag = nullptr means no job.
struct RankCoeffJob {
    const float *proj = nullptr;     // [rows of W incl. guard rows][ldp] projections of the batch slots
    long ldp = 0;
    int nw = 0, m = 0, MT = 0;       // Ritz rows among them, rows in all, 32-row tiles
    const float *wscale = nullptr;   // scale row i of the block went into W with
    const int32_t *slot = nullptr;   // slot[k]: column of proj of active row k
    void *frag = nullptr;            // out: rank_coeff_bytes(m, kmax) bytes
};
// What the trainer knows about the matrix of the tracker's NEXT update(): G = beta * G_prev + alpha * X_a^T diag(w) X_a, G_prev
// the matrix of the last update(), X_a the active rows of the step (kernels_rankupd.hip).
struct RankUpdate {
    const float *proj = nullptr;     // [rows][ldp]: projections of the batch slots on the rows of W as the last update() emitted them (guard rows included)
    long ldp = 0;
    int rows = 0;
    const int32_t *slot = nullptr;   // slot[k]: column of proj that belongs to active row k
    const float *w = nullptr;        // weights of the active rows
    const int *k_dev = nullptr;      // their count (device)
    int kmax = 0;                    // capacity of the lists (multiple of 32, zero padded)
    const void *planes = nullptr;    // syrk_split_rows_kernel's planes of the active rows
    float alpha = 0.f, beta = 1.f;
    int planes_mode = 3;             // syrk_planes_mode(): 3 = three-way split planes, 1 = bf16-once planes
    bool coeff_ready = false;        // the coefficient fragments were written by the gradient's row split (rank_coeff_job)
};
// Fused gradient SYRK + dual average (kernels_syrk.hip): C = beta*C + alpha * sum_k w_k x_k x_k^T over the
// rows ids[0 .. *k_dev) of D, upper tiles computed and mirrored.  ids/w hold kmax entries (multiple of 32,
// zero padded beyond *k_dev).  Returns false when the shape is not supported (F % 128 != 0).
// ids2 != nullptr (pair mode): row k is D[ids[k]] - D[ids2[k]], formed on the fly.
// slab_cols > 0 (dual average sharded over GPUs): only the columns [slab_col0, slab_col0 + slab_cols)
// of C are computed and stored (all rows, no mirror); both must be multiples of 128.
// lower triangle := upper triangle: the fused SYRK relies on an exactly symmetric dual average (it keeps
// it so itself); a matrix that comes from outside (dlco_set_state, dlco_grad_rda) is symmetrised first
void syrk_mirror_upper(float *C, long ldc, int F, hipStream_t s);
// packed = true: C holds the packed upper tiles (syrk_packed_floats(F) floats, ldc ignored): tile (bi, bj), bi <= bj, is a
// contiguous row-major 128 x 128 block at tile index bi*nt - bi*(bi-1)/2 + (bj - bi); no mirrored store.
// planes: >= syrk_planes_bytes(kmax, F) bytes of device memory for the split (or bf16-rounded) row planes of the launch,
// the caller's own (launches of two contexts on two streams must not share planes).
size_t syrk_planes_bytes(int kmax, int F);
struct SyrkArgs {
    const float *D = nullptr;
    long ldd = 0;
    const int32_t *ids = nullptr, *ids2 = nullptr;
    const float *w = nullptr;
    const int *k_dev = nullptr;
    int kmax = 0;
    int F = 0;
    float alpha = 1.0f, beta = 0.0f;
    float *C = nullptr;
    long ldc = 0;
    int slab_col0 = 0, slab_cols = 0;
    bool bf16 = false;                  // operands rounded to bf16 once (cfg.grad_bf16)
    bool packed = false;
    void *planes = nullptr;             // required
    RankCoeffJob coeff_job;             // rides in the row split of the default arithmetic (frag = nullptr: no job)
};
bool syrk_rda_f32(const SyrkArgs &a, hipStream_t s);
// which planes syrk_rda_f32 writes into SyrkArgs::planes: rank_first_term() reads operand 1 of them
int syrk_planes_mode(bool bf16);     // 3: three-way split planes (default arithmetic), 1: bf16-once planes (cfg.grad_bf16), 0: no planes (DLCO_SYRK_FP32)
// The first Chebyshev term of a step's filter from the step's own rank update, without a pass over the matrix
// (kernels_rankupd.hip): out = ay*Y + aq*Q + ac * C_w X_a, C_w[i][k] = ru.w[k] * ru.proj[row(i)][ru.slot[k]] / wscale[i] with
// row(i) = nw-1-i for i < nw (W's ascending order), i for the guard rows behind; X_a = operand 1 of ru.planes.
// The block side of that term:
size_t rank_coeff_bytes(int m, int kmax);
struct RankTermBlock {
    const float *Y = nullptr, *Q = nullptr;   // [m][ld]
    long ld = 0;
    int m = 0, F = 0;
    float ay = 0.f, aq = 0.f, ac = 0.f;
    float *out = nullptr;               // [m][ld]
    int nw = 0;                         // Ritz rows among the m
    const float *wscale = nullptr;      // scale row i of the block went into W with
    void *coeff_ws = nullptr;           // rank_coeff_bytes(m, ru.kmax) bytes; with ru.coeff_ready it already holds the fragments
    SplitPlanes out_planes;             // hi / lo given: also emits the two-way planes of `out` (split_x_kernel's order)
};
// (of ru, the lists, planes, planes_mode and coeff_ready are read; alpha / beta have gone into ay and ac)
bool rank_first_term(const RankTermBlock &b, const RankUpdate &ru, hipStream_t s);
size_t syrk_packed_floats(int F);
void syrk_pack_upper(const float *C, long ldc, int F, float *packed, hipStream_t s);      // upper tiles of a full matrix -> packed
void syrk_unpack_upper(const float *packed, int F, float *C, long ldc, hipStream_t s);    // packed -> full symmetric matrix
// out[M][F] = alpha * X[M][F] * G + b1*E1 + b2*E2 for a symmetric G given as its packed upper tiles, every tile fetched
// from HBM once (kernels_bf16x2.hip, skinny_sym_kernel).  F == 8192 only (64 x 64 tiles on 8 XCDs x 32 CUs); M <= 160
// (two-way split) / 96 (three-way, planes.lo2 != nullptr).  slab: >= 4*M*F floats.  Returns false for other shapes.
bool skinny_product_sym(const SkinnyArgs &a, hipStream_t s);
// its reduction alone where it is the form that also emits the Gram partials (SkinnyArgs::gram_slab); false: nothing launched
bool reduce_gram_sym(const SkinnyArgs &a, hipStream_t s);
// CholQR's dst[n][F] = Linv[n][n] * src[n][F] (n <= 96, F whole 128-column tiles) with gemm_f32's bits, by column slabs,
// and one of: the raw Gram partials of dst (gram_slab [F / gram_chunk][n][n], as SkinnyArgs::gram_slab) or the three-way
// split planes of dst (all of planes.hi / lo / lo2).  Returns false, nothing launched, for other shapes.
struct LinvApplyArgs {
    const float *Linv = nullptr;
    long ldl = 0;
    int n = 0, F = 0;
    const float *src = nullptr;
    float *dst = nullptr;
    long ld = 0;
    float *gram_slab = nullptr;
    int gram_chunk = 0;
    SplitPlanes planes;
};
bool linv_apply_slab(const LinvApplyArgs &a, hipStream_t s);
size_t gemm_slab_floats(int M, int N, int split_k);
// K slices (GemmArgs::split_k) for a product whose M x N tile grid alone would leave the chip idle: enough that
// tiles * slices reaches `target` workgroups, no slice shorter than kmin, no more slices than the slab holds
// (slab_cap = slab floats / (M * N), LONG_MAX where the caller sizes the slab by the result); never fewer than one.
inline int split_k_slices(long tiles, long target, long K, long kmin, long slab_cap)
{
    const long split = std::min(std::min((target + tiles - 1) / tiles, K / kmin), slab_cap);
    return (int)std::max(1L, split);
}
void splitk_reduce_f32(const float *slab, int split, int M, int N, float *C, long ldc, float alpha, float beta,
                       const float *E1, float b1, const float *E2, float b2, hipStream_t s);
// which of its two kernels splitk_reduce_f32 takes for these arguments: the wide one adds the slices one after the other,
// the other one pairs them in a butterfly over 16 lanes.  A kernel that stands in for the launch has to add the same way.
bool splitk_reduce_is_wide(const float *slab, int split, int M, int N, const float *C, long ldc, const float *E1, const float *E2);

// ---------------------------------------------------------------------------
// step kernels (kernels_step.hip)
// ---------------------------------------------------------------------------
// dist[j] = sum_q (sum_z slab[z][q][j])^2 for a [split][r][n] projection slab
void sqdist_from_proj(const float *proj, int split, int r, int n, long ld, float *dist, hipStream_t s, int r_all = 0,
                      float *reduced = nullptr);   // r_all > r (slab form): the slabs hold r_all rows, all reduced into `reduced`, the first r summed
// rho/kappa + signed weights + compact active list for one batch
//   pd, nd: [B] distances; out rho[B], kappa[B]; weights[2B] (rho_i for positives, -kappa_j for negatives)
void viol_counts(const float *pd, const float *nd, int B, int32_t *rho, int32_t *kappa, hipStream_t s);
// viol_counts + build_active_rows in one launch; slots (may be null): slots[k] = position of active row k in the rank's
// [pos | neg] slot list
void viol_counts_active_rows(const float *pd, const float *nd, int B, int32_t *rho, int32_t *kappa, const int32_t *pos_rows,
                             const int32_t *neg_rows, int slot_lo, int slot_hi, int32_t *ids, float *w, int *k_active, int32_t *slots,
                             hipStream_t s);
// build the stacked weighted row list of the SYRK: ids[2B] = (pos rows, neg rows), w[2B] = (rho, -kappa);
// rows with zero weight are dropped; *k_active receives the count. [lo,hi) selects the slots owned by a rank.
void build_active_rows(const int32_t *pos_rows, const int32_t *neg_rows, const int32_t *rho, const int32_t *kappa,
                       int B, int slot_lo, int slot_hi, int32_t *ids, float *w, int *k_active, hipStream_t s);
// per-row sequential hinge sum (src/kernelop-opencv.cu:49-66), rows then summed in double
void hinge_rows(const float *pos, int n_pos, const float *neg, int n_neg, float *row_sums, hipStream_t s);
void sum_f32_to_f64(const float *x, int n, double *out, hipStream_t s);
// count independent problems of the two calls above in one launch each (problem k at + k * ld)
void hinge_rows_batched(const float *pos, int n_pos, const float *neg, int n_neg, long ld_in, float *row_sums, long ld_out, int count,
                        hipStream_t s);
void sum_f32_to_f64_batched(const float *x, int n, long ldx, double *out, int count, hipStream_t s);
void axpby_inplace(float *y, const float *x, float a, float b, size_t n, hipStream_t s);  // y = a*y + b*x
// dst[i] = scale[i] * (src[src_rows[i]] - src[src_rows2[i]]); scale, src_rows and src_rows2 may each be null (1, i, no subtrahend)
void scale_rows(float *dst, long ldd, const float *src, long lds, const float *scale, const int32_t *src_rows,
                const int32_t *src_rows2, int rows, int cols, hipStream_t s);
// out_a[i] = pa[ids ? ids[i] : base + i], out_b likewise: row ids -> (patch, patch) ids of the pair table
// W[j][:] = sqrt(cscale * (theta[nw-1-j] - mu)) * Q[nw-1-j][:] for j < nw: the kept Ritz pairs in ascending
// eigenvalue order, scaled like the reference's W = sqrt(e) * v^T (src/pj-learn.cpp:480-487)
// m_ext > nw: the rows nw..m_ext-1 of Q (the guard rows) are copied unscaled behind the nw rows of W, and wscale[i]
// receives the factor row i of Q went out with (1 for guards) - what the next step's rank update divides by
// (m_ext = 0, wscale = nullptr: the nw rows only)
void emit_w_rows(float *W, long ldw, const float *Q, long ldq, const float *theta, int nw, float mu, float cscale, int F,
                 int m_ext, float *wscale, hipStream_t s);
void translate_ids(const int32_t *ids, int base, int n, const int32_t *pa, const int32_t *pb, int32_t *out_a, int32_t *out_b,
                   hipStream_t s);
void fill_f32(float *p, float v, size_t n, hipStream_t s);

// Column-sharded dual average (one slab of F/world columns per rank): what the tracker and the
// step need to know about the decomposition and how they reach the other ranks.  `allgather`
// performs an in-place all-gather of `gather` viewed as [world][bytes_per_rank] (the rank's own
// chunk is filled by the caller), stream-ordered after the work already queued on the library
// stream; it throws on failure.
struct ShardComm {
    int world = 1, rank = 0;
    int c0 = 0, cw = 0;                  // this rank's columns [c0, c0 + cw)
    float *gather = nullptr;             // exchange buffer, >= gather_floats
    size_t gather_floats = 0;
    std::function<void(size_t bytes_per_rank)> allgather;
};
void pack_cols(float *dst, const float *src, long ld, int c0, int cw, int rows, hipStream_t s);
void unpack_cols(float *dst, long ld, const float *src, int cw, int rows, int world, hipStream_t s);

// synthetic stand-in for a *-unproj.h5 generated in HBM (bench): d = U^T z + eps, clipped
// (rows of F values at row stride ld >= F; columns beyond F are left alone)
void synth_rows(float *D, int N, int F, long ld, const float *U, int k, uint64_t seed, float sig_pos, float sig_neg,
                float noise, float jitter, hipStream_t s);

// ---------------------------------------------------------------------------
// small dense eigen problems (kernels_jacobi.hip, kernels_eig.hip)
// ---------------------------------------------------------------------------
// One-sided Jacobi on a symmetric n x n matrix T (ld = ldt; symmetric up to rounding: for n <= 160 the rows of T are
// taken as the columns of the work image without averaging).  Output: evals[n] descending, V[n][ldv] with ROW j =
// eigenvector j.  work: >= jacobi_work_floats(n) floats.  n <= 4096.
// lam_cut: a pair of columns whose eigenvalue estimates are BOTH below it is still rotated but does not
// keep the sweeps going (the tracker's guard vectors: only their span matters, and the caller checks the
// residuals of the pairs it keeps); JACOBI_COUNT_ALL counts every pair.
// *sweeps_out < 0: the multi-workgroup kernel (160 < n <= 2048) gave up at its bounded grid barrier (its workgroups were
// not all resident at once); evals / V are then NOT written and the caller repeats the call with single_workgroup = true.
constexpr float JACOBI_COUNT_ALL = -3.0e38f;
void jacobi_eigh(const float *T, long ldt, int n, float *evals, float *V, long ldv, float *work, int *sweeps_out,
                 float lam_cut, bool single_workgroup, hipStream_t s);
size_t jacobi_work_floats(int n);
// CholQR building block for panels of <= 160 rows: factors the panel's Gram matrix M = L L^T
// (only its lower triangle is read) and returns Linv = L^-1 [n][ldl] (lower triangular, upper
// part zero), so that the orthonormal rows are the plain product Linv * Z.  A row whose pivot
// falls below rel_thresh * M_jj lies in the span of the rows before it: dead[j] = 1 and row j of
// Linv is zero.
constexpr int CHOL_INV_MAX_N = 160;
void chol_inverse128(const float *M, long ldm, int n, float rel_thresh, float *Linv, long ldl, int *dead, hipStream_t s);
// developer aid (tools/kern_time): the same launch built with phase time stamps; trace [CHOL_INV_STAMPS] on the device
// receives the stamp count in [0], the s_memtime stamps of the eliminating wave behind it and s_memrealtime of both ends last
constexpr int CHOL_INV_STAMPS = 64;
void chol_inverse128_stamped(const float *M, long ldm, int n, float rel_thresh, float *Linv, long ldl, int *dead, unsigned long long *trace,
                             hipStream_t s);
// row norms of (Y - theta_i X); the publishing form also copies the n floats at `src` into pinned host memory and then
// sets *flag_host = seq with a system-scope release (the host polls flag_host; extra: one device int copied along)
// What the residual kernel may emit on the way (see residual_publish_kernel): the rows of W of the pass it closes
struct ResidualEmit {
    float *W = nullptr;
    long ldw = 0;
    float mu = 0.f, cscale = 0.f;
    float *wscale = nullptr;         // scale row i of the block went out with (1 for the rows behind the nw kept ones)
    bool guards = false;             // also write the rows with theta <= mu, unscaled and in place
};
struct ResidualPublish {
    const float *X = nullptr, *Y = nullptr;   // [m][ld]
    long ld = 0;
    const float *theta = nullptr;
    int m = 0, F = 0;
    float *res = nullptr;            // out [m]
    unsigned *ticket = nullptr;      // device word, zero between launches: finds the workgroup that finishes last
    const float *src = nullptr;      // the n device floats that workgroup copies ...
    float *dst_host = nullptr;       // ... into pinned host memory
    int n = 0;
    unsigned *flag_host = nullptr;   // pinned: receives seq once the copy is visible
    unsigned seq = 0;
    const int *extra_dev = nullptr;  // optional: one device int copied along ...
    int *extra_host = nullptr;       // ... to here
    ResidualEmit emit;               // W = nullptr: no rows of W
};
// returns whether the launch writes emit's rows (false: W not given, or a pointer / stride the vector stores do not take)
bool residual_norms_publish(const ResidualPublish &a, hipStream_t s);
void residual_norms(const float *X, const float *Y, long ld, const float *theta, int m, int F, float *res,
                    hipStream_t s);
// rows whose norm is below min_norm become zero rows (0: every row is scaled)
void row_normalize(float *X, long ld, int m, int F, float min_norm, hipStream_t s);
// y = H x style GEMV on a symmetric matrix (memory-bound), used by the spectral-bound estimator
void symv(const float *H, long ld, int F, const float *x, float *y, hipStream_t s);

// ---------------------------------------------------------------------------
// ROC statistics on device (kernels_stats.hip) — src/misc.cpp:297-332
// ---------------------------------------------------------------------------
struct RocWork;
RocWork *roc_work_create(int n_max);
void roc_work_destroy(RocWork *w);
void roc_stats(RocWork *w, const float *dist_dev, const uint8_t *labels_dev, int n, float *fpr95, double *auc,
               hipStream_t s);

// ---------------------------------------------------------------------------
// pooling-region stage (kernels_pr.hip), called from dlco_pr_api.cpp
// ---------------------------------------------------------------------------
bool pr_steps(const float *D, long ld, const int32_t *pos_rows, const int32_t *neg_rows, unsigned n, unsigned t0, float mu, float gamma,
              int F, float *w_io, float *df_io, float *last_f, hipStream_t s);
void pr_gemv(const float *D, long ld, const int32_t *ids, int n, const float *w, int F, float *out, bool in_double, hipStream_t s);
int pr_grid_group(int G, int F, int cus);
bool pr_grid_steps(const float *D, long ld, const int32_t *pos_rows, const int32_t *neg_rows, unsigned n, unsigned t0, const float *mu,
                   const float *gamma, int G, int group, int F, long ldw, float *w_io, float *df_io, hipStream_t s);
void pr_gemv_multi(const float *D, long ld, const int32_t *ids, int n, const float *W, long ldw, const int32_t *sel, int nsel, int F,
                   float *out, long ldo, bool in_double, hipStream_t s);

// ---------------------------------------------------------------------------
// descriptor generation, projection and matching (kernels_desc.hip, kernels_describe.hip, kernels_match.hip),
// called from dlco_desc_api.cpp
// ---------------------------------------------------------------------------
void desc_permute_filters(const float *src, int nsel, float *dst, hipStream_t s);
void desc_transform(const uint8_t *patches, int n_patches, const float *cf, int ks, float inv_step, bool norm, int qk, float qgamma,
                    float *PT, hipStream_t s);
void desc_pool(const float *PT, int n_patches, const float *Fl, int nsel, int nsel_pad, float *desc, long desc_ld, hipStream_t s);
void desc_pair_diff(const float *desc, long ld, int F, const int32_t *pairs, long n_pairs, float *dist, uint8_t *label, hipStream_t s);
void desc_full_dist(const float *desc, long ld, int n_groups, int n_pairs, float *dist, hipStream_t s);
void desc_project(const float *desc, long desc_ld, int n, const float *W, int r, int F, float *Y, long y_ld, hipStream_t s);
void desc_pair_sqdist(const float *Y, long ld, int r, const int32_t *pairs, long n_pairs, float *dist, uint8_t *label, hipStream_t s);
void match_norms(const float *x, long ld, long n, int r, double *norm, hipStream_t s);
// The geometry of a guided launch (the rule is guided_rules.hpp): rec [n][4] doubles, the records of the rows of the side the
// homography applies to (match_records; 16-byte aligned), and xy, the (x, y) floats of the other side's rows at a pitch of
// ldxy floats.  side 0: rec belongs to the launch's queries and xy to train; side 1: rec to train and xy to the queries.
// The epipolar model (guided_epipolar_rules.hpp) has records on both sides and no xy: rec [nt][4] are train's, qrec [nq][4] the
// launch's queries' (match_epi_records), the src records of the side F applies to (side 0: the queries, side 1: train) and
// the dst records of the other; t2 is the squared threshold, which the pair predicate takes itself.
enum { kGuideHomography = 0, kGuideFundamental = 1 };
// The guided batch (match_batch.hpp): rec is the record buffer of a launch (match_records_batch), off [n_ent] the record rows of
// its entries and xy the coordinates of the whole table; qrec is unused.
struct MatchGuide { const double *rec = nullptr; const float *xy = nullptr; long ldxy = 0; int side = 0; int model = kGuideHomography;
                    const double *qrec = nullptr; double t2 = 0.0; const match_batch::GuideOff *off = nullptr; };
void match_records(const float *xy, long ld, long n, const double H[9], double t2, double *rec, hipStream_t s);
void match_epi_records(const float *xy, long ld, long n, const double F[9], int dst_side, double *rec, hipStream_t s);
void match_top2(const float *query, long ldq, int nq, const float *train, long ldt, int nt, int r, const double *qnorm, const double *tnorm,
                int tiles_per_slice, int32_t *idx, float *sqdist, void *part, float *out, const MatchGuide *guide, hipStream_t s);
// the batch forms (match_batch.hpp states the plan): one launch of the plan over the one table [.][ld] and the norms of all its
// rows, ent [n_ent] in device memory; and the rows of the pairs with an empty train image, `none` the bits of "no candidate"
void match_top2_batch(const float *table, long ld, int r, const double *norm, const match_batch::Entry *ent, int n_ent, long wgs, long merge_wgs,
                      int32_t *idx, float *sqdist, void *part, const MatchGuide *guide, const match_batch::Entry *ent_host,
                      const match_batch::GuideOff *off_host, hipStream_t s);
void match_records_batch(const float *xy, long ldxy, const match_batch::Entry *ent, const match_batch::GuideOff *off, int n_ent, long rows,
                         const double *M, double t2, int side, int model, double *rec, hipStream_t s);
void match_u8_top2_batch(const uint8_t *table, long ld, int r, const int32_t *qnorm, const int32_t *tneg, const match_batch::Entry *ent, int n_ent,
                         long wgs, long merge_wgs, int32_t *idx, int32_t *sqdist, void *part, const MatchGuide *guide, hipStream_t s);
void match_fill(const match_batch::Fill *fill, int n_fill, long rows, int32_t none, int32_t *idx, void *sqdist, hipStream_t s);
// byte descriptors (kernels_match_u8.hip; the quantiser is quant_rules.hpp): float rows to bytes, and the match of byte tables;
// guide as match_top2 and match_top2_batch take it: the records and coordinates are the float line's
void desc_quantize_rows(const float *Y, long ldy, int n, int r, float scale, const float *offset, uint8_t *out, long ldo, hipStream_t s);
void match_u8_norms(const uint8_t *x, long ld, long n, int r, bool negate, int32_t *norm, hipStream_t s);
void match_u8_top2(const uint8_t *query, long ldq, int nq, const uint8_t *train, long ldt, int nt, int r, const int32_t *qnorm,
                   const int32_t *tneg, int tiles_per_slice, int32_t *idx, int32_t *sqdist, void *part, int32_t *out, const MatchGuide *guide,
                   hipStream_t s);
// keypoint patches (kernels_patch.hip;the frames and the sampling rule are patch_rules.hpp)
int patch_stage_bytes(const patch_rules::Frame *frames_host, int n, int W, int H);
void patch_sample(const uint8_t *img, int W, int H, long pitch, const patch_rules::Frame *frames, int n, uint8_t *patches, int lds_bytes,
                  hipStream_t s);
// the detector (kernels_detect.hip; the rule is detect_rules.hpp): the integral image S [(H+1)][detect_integral_pitch(W)] u32,
// the keypoints of an octave appended through a counter, and the first rows of the survivors in the rule's order
long detect_integral_pitch(int W);
size_t detect_colsum_count(int W, int H);
void detect_integral(const uint8_t *img, int W, int H, long pitch, uint32_t *S, uint32_t *seg, hipStream_t s);
void detect_octave(const uint32_t *S, int W, int H, int o, int64_t threshold, unsigned cap, unsigned *count, uint64_t *pos, int64_t *resp,
                   float *kp, hipStream_t s);
size_t detect_select_bytes(size_t n);
void detect_select(const uint64_t *pos, const int64_t *resp, const float *kp, unsigned n, unsigned n_out, uint64_t *key_a, uint64_t *key_b,
                   uint32_t *idx_a, uint32_t *idx_b, void *tmp, size_t tmp_bytes, float *kp_out, int64_t *resp_out, hipStream_t s);
// orientation (kernels_orient.hip; the rule is orient_rules.hpp): vectors [n][2] and status [n] of keypoints [n][4] from S
void orient_keypoints(const uint32_t *S, int W, int H, const float *kp, int64_t n, int64_t *vec, uint8_t *status, hipStream_t s);

// verification (kernels_verify.hip): the matches src, dst [m][2] in device memory, 8-byte aligned.  Model is
// verify_rules::Homography (the rule is verify_rules.hpp) or epipolar_rules::Fundamental (epipolar_rules.hpp), the two that
// kernels_verify.hip instantiates.  The steps of one launch of verify_batch.hpp's plan (a single call's launch has one entry):
// ent [n_ent] and the launch's matches in device memory, slot e of M_all [.][n_hyp][9], count [.][n_hyp], best, M_cur [.][9]
// and n belongs to the entry at position e.  M_all of every hypothesis; count += their inliers (the caller zeroes it);
// best [e] = the largest key of entry e and M_cur [e] its matrix (zero: no model); the mask kernel scores M_cur [entry] for
// the entries of active [n_active] (mask_wgs workgroups) into mask at the entry's matches and n [entry] (the caller zeroes it)
template <typename Model>
void verify_pairs_hypotheses(const float *src, const float *dst, const verify_batch::Entry *ent, int64_t n_ent, uint64_t seed, int n_hyp, double *M_all,
                             hipStream_t s);
template <typename Model>
void verify_pairs_score(const float *src, const float *dst, const verify_batch::Entry *ent, int64_t n_ent, int64_t wgs, const double *M_all, int n_hyp,
                        double t2, int32_t *count, hipStream_t s);
void verify_pairs_select(const int32_t *count, const double *M_all, int64_t n_ent, int n_hyp, uint64_t *best, double *M_cur, hipStream_t s);
template <typename Model>
void verify_pairs_mask(const float *src, const float *dst, const verify_batch::Entry *ent, const verify_batch::Active *active, int64_t n_active,
                       int64_t mask_wgs, const double *M_cur, double t2, uint8_t *mask, int32_t *n, const uint8_t *live, hipStream_t s);
// The refit on the device, live [n_ent] saying which entries still refine: live from the selection keys; a round's matrices
// M_try [.][9] from the entries' matches under mask (a rejected round clears live [e]); the round against the model, which it
// replaces when its count n_try [e] is no smaller (n_try [e] is zeroed, live [e] cleared when the entry's refit ends).  The
// mask launch in between takes live as its last argument; the host forms pass NULL there
void verify_pairs_live(const uint64_t *best, int64_t n_ent, uint8_t *live, hipStream_t s);
template <typename Model>
void verify_pairs_refit(const float *src, const float *dst, const verify_batch::Entry *ent, int64_t n_ent, const uint8_t *mask, uint8_t *live,
                        double *M_try, hipStream_t s);
void verify_pairs_step(const verify_batch::Entry *ent, int64_t n_ent, const double *M_try, const uint8_t *trial, int32_t *n_try, double *M_cur,
                       uint8_t *mask, int32_t *count, uint8_t *live, hipStream_t s);

// selecting matches (kernels_select.hip; the rule is select_rules.hpp): the steps of a dlco_desc_select_pairs* call over the
// R >= 1 rows of a batched answer idx, sqdist [R][2], pairs [n_pairs] = select_rules::pair_records and every table in device
// memory.  Dist is float or int32_t, the two that kernels_select.hip instantiates.  f == 0: no ratio test; back: the reverse
// table or null; word [blocks][4] the kept rows as bits and count [blocks] theirs per block, blocks = select_rules::blocks(R);
// off [blocks + 1] the exclusive sums, off [blocks] = M; the first M entries of matches [.][2], dist [.] and, when xy (pitch
// ldxy floats) is not null, src, dst [.][2]; moff [n_pairs + 1]
template <typename Dist>
void select_flag(const select_rules::Pair *pairs, int64_t n_pairs, int64_t R, const int32_t *idx, const Dist *sqdist, float f, const int32_t *back,
                 uint64_t *word, int32_t *count, hipStream_t s);
void select_scan(const int32_t *count, int64_t blocks, int64_t *off, hipStream_t s);
template <typename Dist>
void select_scatter(const select_rules::Pair *pairs, int64_t n_pairs, int64_t R, const int32_t *idx, const Dist *sqdist, const uint64_t *word,
                    const int64_t *off, const float *xy, int64_t ldxy, int32_t *matches, Dist *dist, float *src, float *dst, hipStream_t s);
void select_offsets(const select_rules::Pair *pairs, int64_t n_pairs, int64_t R, const uint64_t *word, const int64_t *off, int64_t *moff, hipStream_t s);

// building tracks (kernels_tracks.hip; the rule is track_rules.hpp): the two halves of a dlco_desc_build_tracks* call over the
// N >= 1 nodes of a batch, every table in device memory.  tracks_labels: pairs [n_pairs] = track_rules::pair_records, matches
// [M][2], keep [M] or null, M may be 0; parent, node, conf [N] are written (node = 0 .. N - 1, conf = 0) and label [N] is the
// smallest node of every node's component.  tracks_group: from label and node to toff, obs, track_of; seg [n_img + 1] in device
// memory, slabel, snode, size [N] scratch, tmp tracks_sort_bytes(N) bytes, word [2][blocks][4], count [5][blocks],
// off [5][blocks + 1], blocks = track_rules::blocks(N); total [5] = observations, tracks, counts [0 .. 2]
size_t tracks_sort_bytes(int64_t N);
void tracks_labels(const track_rules::Pair *pairs, int64_t n_pairs, int64_t N, int64_t M, const int32_t *matches, const uint8_t *keep, int32_t *parent,
                   int32_t *node, uint8_t *conf, int32_t *label, hipStream_t s);
void tracks_group(int64_t N, const int32_t *label, const int32_t *node, const int64_t *seg, int32_t n_img, int32_t min_len, int32_t unique,
                  int32_t *slabel, int32_t *snode, int32_t *size, uint8_t *conf, void *tmp, size_t tmp_bytes, uint64_t *word, int32_t *count,
                  int64_t *off, int64_t *total, int64_t *toff, int32_t *obs, int32_t *track_of, hipStream_t s);

}  // namespace dlco
