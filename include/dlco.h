/*
 * dlco.h — C ABI of libdlco.so: the MI355X (gfx950) implementation of opencv-dlco's
 * projection-learning hot path (pj-learn).
 *
 * The reference (cbalint13/opencv-dlco) has no plugin or FFI interface: the path is a
 * monolithic main() (src/pj-learn.cpp:57-600) plus the free functions declared in
 * include/trainer.hpp:43-64.  Each entry point below names the reference code it
 * replaces; a maintainer's pj-learn main() would call them in the order shown in
 * INTEGRATION.md.  Plain pointers and sizes only; every buffer is caller-owned and
 * copied by the library unless a function says otherwise.  All functions return
 * DLCO_OK (0) or a negative error code; dlco_last_error() gives the message.  A context
 * is driven by one host thread; distinct contexts are independent.
 *
 * There is no CPU fallback: dlco_ctx_create fails when no gfx950 device is usable.
 */
#ifndef DLCO_H
#define DLCO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DLCO_OK            0
#define DLCO_ERR_INVALID  -2   /* bad argument / wrong call order          */
#define DLCO_ERR_HIP      -3   /* HIP runtime error (message has details)  */
#define DLCO_ERR_NODEVICE -4   /* no usable gfx950 device                  */
#define DLCO_ERR_NOCONV   -5   /* eigen tracker did not reach its tolerance */
#define DLCO_ERR_COMM     -6   /* the host's collective callback failed      */

typedef struct dlco_ctx dlco_ctx;

/* Hyper-parameters and shapes.  Defaults (dlco_cfg_default) are the reference's
 * hard-coded values, src/pj-learn.cpp:89-96,225. */
typedef struct dlco_cfg {
    int32_t  F;          /* FeatDim: columns of "Distance"                 (:179) */
    int32_t  N;          /* nDists: rows of "Distance"/"Label"             (:178) */
    int32_t  B;          /* szBatch per class, GLOBAL over all ranks       (:93)  */
    float    mu;         /* trace-norm weight                              (:89)  */
    float    gamma;      /* RDA step parameter                             (:90)  */
    uint64_t seed;       /* sampler RNG seed                               (:225) */
    int32_t  device;     /* HIP device ordinal                             (:267) */
    int32_t  rank;       /* data-parallel rank: owns batch slots [rank*B/world, (rank+1)*B/world) */
    int32_t  world;      /* number of ranks (1 = the reference's single device)           */
    float    eig_tol;    /* subspace tracker tolerance on the weighted c*|residual| / max e (default 2e-4; the first
                          * update after a (re)start converges to a quarter of it).  Measured error of A+ against
                          * ssyevr at the default: 1.5e-5 (rank 64) / 3.6e-5 (rank 128) of its largest entry at
                          * F = 8192, i.e. inside SURVEY 8(d)'s 1e-4 gate; 5e-5 costs 6 % / 40 % of the step rate */
    int32_t  eig_guard;  /* guard vectors kept beyond the positive eigenspace (default 32)  */
    int32_t  eig_max_iter; /* filter+Rayleigh-Ritz iterations per step before giving up      */
                          /* The tracker block holds at most min(F, max(1024, 2*B + 2*eig_guard)) rows (positive
                           * rank + guards); a positive eigenspace that does not fit is reported as a
                           * non-converged step, never truncated silently.                              */
    int32_t  shard;      /* world > 1 only.  0: every rank keeps the whole dual average, the F x F
                          * partial gradients are all-reduced (dlco_step_begin/grad/finish).
                          * 1: the dual average is sharded by columns, rank g owns columns
                          * [g*F/world, (g+1)*F/world); no F x F exchange, the step (dlco_step) calls
                          * the all-gather registered with dlco_set_allgather.  F % (128*world) == 0
                          * selects the fused kernels.                                            */
    int32_t  strict_conv; /* 1: dlco_step returns DLCO_ERR_NOCONV when the tracker misses eig_tol (the step is
                          * still applied).  0 (default): the miss is counted (dlco_counters out[2],
                          * dlco_log_entry.nonconv) and the run goes on with the approximate W.            */
    int32_t  grad_bf16;  /* 1: BASELINE configs[4], "bf16 MFMA + fp32 accumulate": every GEMM whose operand is the resident
                          * Distance matrix multiplies on the bf16 matrix cores with fp32 accumulation, operands rounded
                          * to bf16 once when the MFMA fragments are formed - the gradient SYRK (Q1), the projection of
                          * the batch (P1), of the validation rows (T1) and of all N rows in the statistics pass (S2).
                          * Gather, weights, dual average, squared sums, the PSD projection stay fp32.  Not the
                          * reference's arithmetic: the result is gated on the FPR@95 band, not on the fp32
                          * tolerances.  Needs F % 128 == 0.  0 (default): fp32 results (fp32 MFMA, or split-bf16
                          * MFMA carrying all 24 mantissa bits where a pass would otherwise be matrix-bound).      */
    int32_t  reserved[5];
} dlco_cfg;

void dlco_cfg_default(dlco_cfg *cfg);

const char *dlco_version(void);
/* Message of the last error on this thread (ctx may be NULL for create failures). */
const char *dlco_last_error(const dlco_ctx *ctx);

/* Allocates device state; replaces cuda::setDevice(0) and the Mat::zeros block,
 * src/pj-learn.cpp:259-291. */
int dlco_ctx_create(dlco_ctx **out, const dlco_cfg *cfg);
void dlco_ctx_destroy(dlco_ctx *ctx);
/* "Found GPU: <name>" line of the reference log, src/pj-learn.cpp:259-263. */
int dlco_device_name(const dlco_ctx *ctx, char *buf, size_t cap, int *cc_major, int *cc_minor);

/* Uploads Distance [N,F] row-major f32 and Label [N] u8 (1 = match, 0 = non-match) to HBM,
 * builds IdxPos/IdxNeg, shuffles and splits them.  Replaces src/pj-learn.cpp:214-256,277-281. */
int dlco_set_data(dlco_ctx *ctx, const float *dists_host, const uint8_t *labels_host);
/* Same, but `dists_dev` [N,F] (row stride F) already lives in device memory.  When F is a multiple of the
 * device width's granularity (dlco_device_width(ctx) == F) it is adopted, not copied, and must stay valid
 * for the life of the context; otherwise it is copied once into the padded resident layout. */
int dlco_set_data_device(dlco_ctx *ctx, const float *dists_dev, const uint8_t *labels_host);
/* FeatDim is whatever the input file says (src/pj-learn.cpp:176-179: 480, 544, 608 in the reference's own
 * runs).  On the device every row is kept at dlco_device_width(ctx) floats: F rounded up to whole 128-column
 * tiles (to 128*world when the dual average is column-sharded), the extra columns zero.  Zero columns add
 * zero rows and columns to the dual average; their eigenvalue of A = -c (dfAvg + mu I) is -c mu <= 0 and is
 * never kept (src/pj-learn.cpp:452,480-484), so W, A, dfAvg, distances and statistics restricted to the
 * first F columns are those of the unpadded computation.  Every host-side argument and result of this
 * header has the caller's width F; only DLCO_BUF_* device buffers show the padded width. */
int dlco_device_width(const dlco_ctx *ctx);
/* The resident matrix (row or pair mode, labels, pair index) of another context on the same device with the
 * same F and N: shared, not copied (`src` must outlive ctx).  What bench.py's second trainer uses. */
int dlco_set_data_shared(dlco_ctx *ctx, dlco_ctx *src);
/* Pair mode: instead of the N x F "Distance" matrix that comp-uprjdists materialises
 * (Dist = Desc1 - Desc2 per pair, src/comp-uprjdists.cpp:308-327; 16 GB for 500k x 8192)
 * the caller uploads the P per-patch descriptors desc_host [P,F] once and the pair table
 * pairs_host [N,4] = (patchID1, 3DpointID1, patchID2, 3DpointID2) of the reference's
 * "Indices" dataset.  Row i of the training matrix is desc[pairs[i][0]] - desc[pairs[i][2]],
 * formed in fp32 inside the kernels (the same single rounding as the reference's Mat
 * subtraction); Label[i] = (pairs[i][1] == pairs[i][3]), src/comp-uprjdists.cpp:268-272.
 * Every result is bit-identical to dlco_set_data on the pre-differenced matrix. */
int dlco_set_pairs(dlco_ctx *ctx, const float *desc_host, int32_t P, const int32_t *pairs_host);
/* same with the descriptor table already in device memory (e.g. written by dlco_desc_compute_device);
 * the caller keeps it alive for the life of the context */
int dlco_set_pairs_device(dlco_ctx *ctx, const float *desc_dev, int32_t P, const int32_t *pairs_host);
/* Bench helper (no reference counterpart: the Brown/Winder sets are not redistributable):
 * fills the context's Distance matrix in HBM with d = U^T z + noise*eps clipped to [-1,1],
 * z ~ N(0, (sigma * s_i)^2 I_k), s_i = exp(scale_jitter * g_i) a per-row log-normal scale (0 = none),
 * label = 1 for even rows; U is [k,F] on the host. */
int dlco_synth_data(dlco_ctx *ctx, const float *U_host, int32_t k, uint64_t seed,
                    float sigma_pos, float sigma_neg, float noise, float scale_jitter);
/* Copies `n` rows [row0, row0+n) of the device-resident Distance matrix back to the host. */
int dlco_get_rows(dlco_ctx *ctx, int32_t row0, int32_t n, float *out_host);

/* Pair indexing (bit-exact contract): shuffled index vectors and the 80/20 split,
 * src/pj-learn.cpp:214-237.  pos/neg may be NULL to query sizes only. */
int dlco_get_index(const dlco_ctx *ctx, int32_t *pos, int32_t *n_pos, int32_t *n_pos_trn,
                   int32_t *neg, int32_t *n_neg, int32_t *n_neg_trn);

/* One iteration of the training loop, src/pj-learn.cpp:305-490 (sampling, distances,
 * violation counts, gradient, dual average, PSD projection).  dlco_steps runs n of them
 * without host synchronisation beyond what the eigen tracker needs. */
int dlco_step(dlco_ctx *ctx);
int dlco_steps(dlco_ctx *ctx, int32_t n);

/* The same iteration split at its two exchange points, for data-parallel runs (one
 * process per GPU; the caller moves the buffers with RCCL between the phases):
 *   dlco_step_begin  : sample the global batch, project the rank's own slots;
 *                      fills the rank's slice of the distance buffer
 *   -- all-gather DLCO_BUF_DIST (2*B floats) --
 *   dlco_step_grad   : violation counts over the global batch, the rank's partial
 *                      gradient P^T diag(rho) P - N^T diag(kappa) N into DLCO_BUF_GRAD
 *   -- sum all-reduce DLCO_BUF_GRAD (F*F floats) --
 *   dlco_step_finish : dual average, PSD projection (replicated on every rank)
 * With world == 1 the three calls in sequence equal dlco_step. */
int dlco_step_begin(dlco_ctx *ctx);
int dlco_step_grad(dlco_ctx *ctx);
int dlco_step_finish(dlco_ctx *ctx);

#define DLCO_BUF_DIST   1   /* f32 [world][2*B/world]: rank g's slice holds the distances of its
                               B/world positive slots, then of its B/world negative slots   */
/* (device buffers: F below is the padded device width Fd = dlco_device_width(ctx), not cfg.F) */
#define DLCO_BUF_GRAD   2   /* f32 [Fd*Fd]: this rank's dLoss partial                  */
#define DLCO_BUF_DFAVG  3   /* f32 [Fd*Fd]: running dual average.  A single-rank context with Fd <= 8192 keeps only the
                               nt (nt + 1) / 2 tiles on or above the diagonal (nt = Fd / 128): contiguous row-major
                               128 x 128 blocks, tile (I, J), I <= J, at block index nt I - I (I - 1) / 2 + J - I
                               (dlco_get_dfavg / dlco_set_state convert)                                           */
#define DLCO_BUF_W      4   /* f32 [r*Fd]: current projection                          */
#define DLCO_BUF_GATHER 5   /* f32 [world][rows*F/world]: column slabs of a tracker product
                               (sharded contexts only)                                   */
#define DLCO_BUF_DATA   6   /* f32 [N*Fd] (row mode) or [P*Fd] (pair mode): the resident Distance /
                               descriptor matrix (dlco_set_data_shared shares it with a second context) */
/* Device pointer and byte size of an exchange buffer (valid until ctx is destroyed). */
int dlco_dev_buffer(dlco_ctx *ctx, int32_t which, void **dev_ptr, size_t *bytes);
/* Makes the context use caller-owned device memory for an exchange buffer (DLCO_BUF_DIST,
 * DLCO_BUF_GRAD or DLCO_BUF_GATHER), e.g. a tensor the caller's RCCL communicator operates
 * on.  The memory must outlive the context. */
int dlco_bind_buffer(dlco_ctx *ctx, int32_t which, void *dev_ptr, size_t bytes);

/* Sharded contexts (cfg.shard = 1, world > 1): the collective the step needs, supplied by the
 * host.  fn(user, which, bytes_per_rank) must all-gather, IN PLACE, the first
 * world*bytes_per_rank bytes of exchange buffer `which` (DLCO_BUF_DIST or DLCO_BUF_GATHER)
 * viewed as [world][bytes_per_rank] — the rank's own chunk is already filled — ordered after
 * the work queued on dlco_stream() and visible to work queued there afterwards (enqueue the
 * RCCL call on that stream, or synchronise around it).  Return 0 on success.  dlco_step calls
 * it once for the 2B distances and once per product of the eigen tracker with the dual
 * average (about six times a step, 4*rows*F/world bytes per rank each); every rank makes the
 * same sequence of calls.  The reference has no counterpart (single device). */
typedef int (*dlco_allgather_fn)(void *user, int32_t which, size_t bytes_per_rank);
int dlco_set_allgather(dlco_ctx *ctx, dlco_allgather_fn fn, void *user);
/* Alternative to the callback: the library performs the all-gathers itself with RCCL
 * (ncclAllGather over xGMI, in place, on its own stream; librccl is reached through dlopen:
 * the copy already loaded in the process, else `rccl_path`, else the system one).  Rank 0 obtains
 * a 128-byte ncclUniqueId with dlco_comm_unique_id, the host hands the same bytes to every rank
 * (MPI, torch.distributed, a file ...), and every rank calls dlco_comm_init (a collective:
 * ncclCommInitRank with cfg.rank / cfg.world).  A communicator, once created, takes precedence
 * over the callback; dlco_comm_destroy (or dlco_ctx_destroy) releases it.
 * A REPLICATED context (cfg.shard = 0, world > 1) with a communicator runs the literal exchange of BASELINE configs[3]
 * inside dlco_step: all-gather of the 2B distances, then ncclAllReduce (sum, f32) of the F x F partial gradients, then
 * the dual average and PSD projection on every rank (= dlco_step_begin / grad / finish with the library moving the
 * buffers).  The reference has no counterpart: it is single-device (src/pj-learn.cpp:267). */
int dlco_comm_unique_id(void *out_id, size_t cap, const char *rccl_path);
int dlco_comm_init(dlco_ctx *ctx, const void *id, size_t id_bytes, const char *rccl_path);
/* Fallback transport for ranks that are processes of one node when RCCL cannot be used (no librccl, or
 * several ranks sharing one GPU, which RCCL refuses): the all-gathers go through the POSIX shared-memory
 * segment `shm_name` (device -> host -> device, barriers on counters inside the segment).  Every rank
 * calls it (a collective); the segment must not exist beforehand or be all zeros, and is unlinked once
 * every rank has attached.  Correct and deterministic but host-staged: a test / fallback path, an RCCL
 * communicator takes precedence. */
int dlco_comm_init_host(dlco_ctx *ctx, const char *shm_name);
int dlco_comm_destroy(dlco_ctx *ctx);
/* The HIP stream the context launches on (as void*), so callers can order collectives. */
int dlco_stream(dlco_ctx *ctx, void **stream);
int dlco_sync(dlco_ctx *ctx);

/* Row ids (into Distance) of the last sampled batch and their squared distances
 * (src/pj-learn.cpp:311-314, 346-363); rho/kappa = violation counts (:373-376).
 * Valid once a step has run (DLCO_ERR_INVALID before that). */
int dlco_get_batch(const dlco_ctx *ctx, int32_t *pos_rows, int32_t *neg_rows,
                   float *pos_dist, float *neg_dist, int32_t *rho, int32_t *kappa);

/* State access.  Rank follows the reference: rows of W with a strictly positive
 * eigenvalue; when there are none, *r = F and W is F*F zeros (src/pj-learn.cpp:481-490). */
int dlco_get_t(const dlco_ctx *ctx, uint32_t *t);
int dlco_get_W(dlco_ctx *ctx, float *W_host /* cap F*F */, int32_t *r);
int dlco_get_A(dlco_ctx *ctx, float *A_host /* F*F: PSD-projected A = W^T W */);
int dlco_get_dfavg(dlco_ctx *ctx, float *dfavg_host /* F*F */);
/* Teacher forcing: overwrite t, dfAvg and W (W may be NULL with r = 0 for the zero start).
 * The eigen tracker restarts from the given W's row space. */
int dlco_set_state(dlco_ctx *ctx, uint32_t t, const float *dfavg_host, const float *W_host, int32_t r);

/* Validation objective, src/pj-learn.cpp:501-527: loss_val = hinge sum over the
 * validation positives x negatives / nPosVal / nNegVal, regul = mu * trace(A). */
int dlco_validate(dlco_ctx *ctx, float *loss_val, float *regul, int32_t *rank);

/* ComputePJStats (src/misc.cpp:266-333) on all N rows.  W_host == NULL uses the
 * context's current W. */
int dlco_stats(dlco_ctx *ctx, const float *W_host, int32_t r, int32_t *dim, float *fpr95, double *auc);

/* ---- single operators, exposed for parity tests and for eval-fpr95 ------------------- */
/* P1+P2: out[i] = || W x_{row_ids[i]} ||^2 over rows of the resident Distance matrix. */
int dlco_project_sqdist(dlco_ctx *ctx, const int32_t *row_ids_host, int32_t n,
                        const float *W_host, int32_t r, float *out_host);
/* V1: rho_i = #{j : pd_i + 1 > nd_j}, kappa_j = #{i : pd_i + 1 > nd_j}. */
int dlco_viol_counts(dlco_ctx *ctx, const float *pd_host, const float *nd_host, int32_t B,
                     int32_t *rho_host, int32_t *kappa_host);
/* Q1+U1: dfavg_out = beta*dfavg_in + alpha*(P^T diag(rho) P - N^T diag(kappa) N) with rows
 * taken from the resident Distance matrix (fused SYRK + dual average; the step uses alpha = 1/(B*B*(t+1)),
 * beta = t/(t+1), src/pj-learn.cpp:422). */
int dlco_grad_rda(dlco_ctx *ctx, const int32_t *pos_rows_host, const int32_t *neg_rows_host,
                  const int32_t *rho_host, const int32_t *kappa_host, int32_t B,
                  float alpha, float beta, const float *dfavg_in_host, float *dfavg_out_host);
/* E1+E2: PSD projection of A = -(sqrt(t+1)/gamma)(dfavg + mu I); returns W (rows ascending
 * in eigenvalue, as LAPACK orders them) and optionally A+. */
int dlco_psd_project(dlco_ctx *ctx, const float *dfavg_host, uint32_t t,
                     float *W_host, int32_t *r, float *A_host /* may be NULL */);
/* Building block of E1 (no single reference line: the reference calls LAPACKE_ssyevr, :440):
 * out[rows,F] = X[rows,F] * G[F,F] for a symmetric G, rows <= 128.  mode 0 = the generic fp32 MFMA GEMM (k-ordered
 * fmaf chains, K slices summed in a fixed order: the tracker's products where no split-bf16 kernel applies), mode 1 = two-way split-bf16 MFMA with fp32 accumulation (the Chebyshev filter;
 * relative error ~1e-5), mode 2 = three-way split-bf16 MFMA (the Rayleigh-Ritz product when
 * F % 512 == 0; error at the level of fp32 rounding, ~1e-7).  Modes 3 / 4 (F == 8192 only) are modes 1 / 2 on the packed
 * upper-tile form of G that a single-rank trainer keeps its dual average in: only the upper triangle of G_host is read,
 * and every 128 x 128 tile is fetched from HBM once per product.  rows <= 160 for modes 1 / 3. */
int dlco_sym_product(dlco_ctx *ctx, const float *X_host, int32_t rows, const float *G_host, int32_t mode,
                     float *out_host);
/* The generic fp32 GEMM under every Gram matrix, rotation and projection of the step (no reference line: the reference
 * calls cuBLAS / OpenBLAS sgemm), on host arrays, for tests and for timing single shapes:
 *   C [M,N] = alpha * A(M,K) * B(K,N) + beta * C + b1 * E1 + b2 * E2, and with a twin operand C2 = the same with B2.
 * An operand is `rows` memory rows of pitch ld.  kmajor: memory rows run along K, element (x, k) at row(k) * ld + x; else
 * along M / N, element (x, k) at row(x) * ld + k.  row(i) = row_ids ? row_ids[i] : i, and with row_ids2 the operand row is
 * memory row row_ids[i] minus memory row row_ids2[i]; row_scale [K] (k-major operands only) scales row k.
 * split_k > 1: K slices summed in a fixed order.  k_dev >= 0: a K limit the kernel reads from device memory (<= K), -1:
 * none.  B2_host: laid out like B; needs split_k == 1.  small_m_tiles / small_n_tiles: 64-wide tiles whatever M / N.
 * depth: K tiles of global loads in flight per workgroup, 0 = the library's choice (what every other entry point runs),
 * 1 = one tile (the schedule every launch had before the choice existed).  Results do not depend on it bit for bit; it
 * exists for measurement.  *depth_used (may be NULL): the depth the launch ran with.  reps > 0: the launch is also
 * repeated reps times between two HIP events, *us_per_launch (may be NULL) = their distance / reps.
 * C_host [M,N] holds C on entry (read when beta != 0) and the result on return; C2_host likewise, NULL without B2. */
typedef struct dlco_gemm_operand {
    const float   *host;
    int32_t        rows, ld;
    int32_t        kmajor;
    const int32_t *row_ids, *row_ids2;
    const float   *row_scale;
} dlco_gemm_operand;
typedef struct dlco_gemm_probe_args {
    int32_t M, N, K;
    dlco_gemm_operand A, B;
    const float *B2_host;
    int32_t split_k, k_dev, small_m_tiles, small_n_tiles, depth, reps;
    float   alpha, beta, b1, b2;
    const float *E1_host, *E2_host;     /* [M,N] or NULL */
} dlco_gemm_probe_args;
int dlco_gemm_probe(dlco_ctx *ctx, const dlco_gemm_probe_args *args, float *C_host, float *C2_host, int32_t *depth_used,
                    double *us_per_launch);
/* CholQR's Cholesky inverse alone (no reference line: the reference orthonormalises by LAPACK), on host arrays, for
 * tests: M_host [n, ld] is a symmetric positive semi-definite Gram matrix (lower triangle read), 1 <= n <= 160, ld >= n.
 * Linv_host [n, ld] receives L^-1 of M = L L^T (lower triangular, entries beyond column n untouched), dead_host [n] a 1 for
 * every row whose pivot fell below rel_thresh times its diagonal entry of M (that row of Linv is zero). */
int dlco_chol_probe(dlco_ctx *ctx, const float *M_host, int32_t n, int32_t ld, float rel_thresh, float *Linv_host,
                    int32_t *dead_host);
/* The tail of one eigen-tracker pass on host arrays, for tests (no reference line): the last filter product
 * Z' = alpha * Z * G + b1 * Z + b2 * Zprev (split-bf16, two-way), CholQR2 of Z' -> Qo, the exact product Yb = -Qo * G and
 * T = Yb * Qo^T.  The context's F must be whole 128-column tiles (at most 64).  Gp_host is G as its packed upper tiles:
 * tile (I, J), I <= J, is a contiguous row-major 128 x 128 block at tile index I*nt - I*(I-1)/2 + (J - I), nt = F / 128,
 * diagonal tiles stored whole.  Zprev_host may be NULL (no third term).  panel_end = 0 and n_lock = 0: the block is one
 * orthonormalisation panel, the steady state; panel_end cuts a second panel there, n_lock > 0 leaves that many leading rows
 * as they are.  unfused != 0 forces every Gram product, every application of L^-1 and the split of Qo into a launch of
 * its own.  Qo_host, Yb_host [m, F], T_host [m, m]; fused (may be NULL): [0] = reductions that also formed the Gram
 * partials behind them, [1] = applications of L^-1 that also fed the next launch (two each in the steady state). */
typedef struct dlco_ortho_probe_args {
    const float *Z_host, *Zprev_host, *Gp_host;
    int32_t m, panel_end, n_lock, unfused;
    float   alpha, b1, b2;
} dlco_ortho_probe_args;
int dlco_ortho_probe(dlco_ctx *ctx, const dlco_ortho_probe_args *args, float *Qo_host, float *Yb_host, float *T_host,
                     int64_t fused[2]);
/* out[0] = product reductions of the context's eigen tracker that also formed the Gram partials behind them; out[1] =
 * CholQR applications of L^-1 that also fed the next launch (Gram partials or split planes). */
int dlco_fused_counters(const dlco_ctx *ctx, int64_t out[2]);
/* H1: sum_i sum_j max(pos_i + 1 - neg_j, 0)  (src/kernelop-opencv.cu:49-80). */
int dlco_hinge_sum(dlco_ctx *ctx, const float *pos_host, int32_t n_pos,
                   const float *neg_host, int32_t n_neg, double *out);
/* S3+S4 on host arrays. */
int dlco_roc_stats(dlco_ctx *ctx, const float *dist_host, const uint8_t *labels_host, int32_t n,
                   float *fpr95, double *auc);

/* ---- model selection and logging, src/pj-learn.cpp:492-587 ---------------------------- */
typedef struct dlco_log_entry {
    uint32_t t;
    int32_t  is_best;      /* 1: "Best:" line + "Stat:" line, 0: "Step:" line */
    int32_t  saved;        /* 1: "[saved]" */
    float    loss_val, regul, obj, obj_best;
    int32_t  rank, rank_best;
    int32_t  dim;
    double   auc, auc_best;
    float    fpr95, fpr95_best;
    double   vtime;        /* seconds spent in this call (Vtime) */
    int32_t  nonconv;      /* training steps since the previous dlco_log_step whose eigen tracker stopped
                              short of eig_tol (no reference counterpart: LAPACKE_ssyevr is direct)      */
    int32_t  reserved;
} dlco_log_entry;
/* Runs the LogStep block once: validation, best-objective test, stats and save rule.
 * Keeps W_Best / W_Save / A_Save inside the context. */
int dlco_log_step(dlco_ctx *ctx, dlco_log_entry *out);
/* W_Save [r,F] and A_Save [F,F] (src/pj-learn.cpp:592-597); *r = 0 when nothing was saved. */
int dlco_get_saved(dlco_ctx *ctx, float *W_host, int32_t *r, float *A_host);

/* ---- measurement ------------------------------------------------------------------------ */
/* on = 1: the launches of the kernel groups "grad_syrk", "eig_product", "jacobi", "project", "rank_update" are bracketed by HIP events on
 * the context's stream; dlco_profile_read returns launches and their summed duration.  on = 2: the gradient SYRK only
 * (two records per step; all four groups cost ~3 % of the step in event records, measured).  on = 0: off. */
int dlco_profile_enable(dlco_ctx *ctx, int32_t on);
int dlco_profile_read(dlco_ctx *ctx, const char *kernel, int64_t *launches, double *total_ms);
/* Counters since creation: out[0] = training steps run, out[1] = sum over those steps of the
 * rows that entered this rank's gradient SYRK (rows with a non-zero violation count),
 * out[2] = steps whose eigen tracker stopped at its iteration cap, out[3] = calls of the multi-workgroup
 * Jacobi kernel that gave up at its bounded grid barrier (the m x m problem was then solved again on one
 * workgroup: a slow event, never a wrong result), out[4] = tracker updates whose first filter term came from the
 * step's own rank update (dfAvg_{t+1} = beta dfAvg_t + alpha X_a^T diag(w) X_a, src/pj-learn.cpp:367-422) instead
 * of a pass over the dual average, out[5] = with DLCO_RANK_UPDATE_CHECK=1 in the environment, 1e9 x the largest
 * relative deviation of such a term from the product it replaces (developer aid), out[6] = tracker passes that ran
 * with the converged top of the block locked out of the filter (start-up transient), out[7] = rows locked in them. */
int dlco_counters(const dlco_ctx *ctx, int64_t out[8]);
/* Tracker statistics since creation: filter/RR iterations, H-products (in rows), restarts. */
int dlco_eig_stats(const dlco_ctx *ctx, int64_t *iters, int64_t *product_rows, int64_t *jacobi_sweeps,
                   int32_t *block_rows);

/* ======================================================================================================
 * pr-learn — the pooling-region stage that precedes pj-learn.
 * Replaces the loop and the LogStep block of src/pr-learn.cpp:229-434 and ComputePRStats
 * (src/misc.cpp:171-264).  L1-regularised dual averaging on the weight vector w [F] of the F candidate
 * pooling regions: one (positive, negative) row pair per iteration, strictly sequential, so a window of
 * iterations is ONE kernel launch on one workgroup (w and dfAvg in registers).  The arithmetic follows
 * the reference operation for operation (single-thread order of its OpenMP loop), see
 * opencv-dlco_amd/csrc/kernels_pr.hip.
 * ====================================================================================================== */
typedef struct dlco_pr_ctx dlco_pr_ctx;
const char *dlco_pr_last_error(const dlco_pr_ctx *ctx);
/* F = FeatDim (5120 in the reference's runs; a multiple of 4, at most 8192), N rows; defaults of the
 * reference: mu 0.025, gamma 0.10, seed 2215 (src/pr-learn.cpp:78-82,241). */
int dlco_pr_create(dlco_pr_ctx **out, int32_t F, int32_t N, float mu, float gamma, uint64_t seed, int32_t device);
void dlco_pr_destroy(dlco_pr_ctx *ctx);
int dlco_pr_device_name(const dlco_pr_ctx *ctx, char *buf, size_t cap, int *cc_major, int *cc_minor);
/* Distance [N,F] f32 + Label [N] u8; index build, randShuffle and 80/20 split, src/pr-learn.cpp:229-253. */
int dlco_pr_set_data(dlco_pr_ctx *ctx, const float *dists_host, const uint8_t *labels_host);
int dlco_pr_get_index(const dlco_pr_ctx *ctx, int32_t *n_pos, int32_t *n_pos_trn, int32_t *n_neg, int32_t *n_neg_trn);
/* n iterations of src/pr-learn.cpp:302-329 (sample, subtract, dot product, dual average, soft threshold). */
int dlco_pr_steps(dlco_pr_ctx *ctx, uint32_t n);
int dlco_pr_get_state(dlco_pr_ctx *ctx, uint32_t *t, float *w_host /* F */, float *dfavg_host /* F */);
int dlco_pr_set_state(dlco_pr_ctx *ctx, uint32_t t, const float *w_host, const float *dfavg_host);
/* Validation objective of the current w, src/pr-learn.cpp:340-361: hinge loss over validation positives x
 * negatives / (nPosVal * nNegVal), regul = mu * sum|w|, nnz = countNonZero(w). */
int dlco_pr_validate(dlco_pr_ctx *ctx, float *loss_val, float *regul, int32_t *nnz);
/* ComputePRStats (src/misc.cpp:171-264) for w_host (NULL: the current w) on all N rows.  PRParams is the
 * [pr_rows >= 8*F, pr_cols] table of the filter file; nPR / Dim / nzDim as the reference counts them; when
 * max_dim != -1 and Dim > max_dim the function returns before the ROC pass (fpr95 / auc untouched). */
int dlco_pr_stats(dlco_pr_ctx *ctx, const float *w_host, const float *prparams_host, int32_t pr_rows, int32_t pr_cols,
                  int32_t nchannels, int32_t max_dim, int32_t *nPR, int32_t *dim, int32_t *nzdim, float *fpr95, double *auc);

/* A grid of pr-learn settings in one launch per window (the reference runs pr-learn once per data set and
 * (mu, gamma) pair).  G settings (mu[k], gamma[k]) trained on the resident data of `src` (shared, not
 * copied: src must outlive the grid), each from w = dfAvg = 0 at t = 0 with the sampler CvRng(seed).
 * Setting k's w / dfAvg after any sequence of dlco_pr_grid_steps are bit-identical to a dlco_pr_ctx
 * created with (F, N, mu[k], gamma[k], seed) on the same data after the same total number of iterations:
 * the settings share the sampled row pairs (the sampler does not depend on w) and each workgroup applies
 * every pair it fetches to several settings.  The grid has its own stream and sampler; it never advances
 * src's sampler or t.  DLCO_ERR_INVALID: G outside 1 .. 65535, a gamma <= 0, src without data or with an
 * empty training or validation split, a configs entry out of range. */
typedef struct dlco_pr_grid dlco_pr_grid;
int  dlco_pr_grid_create(dlco_pr_grid **out, dlco_pr_ctx *src, int32_t G, const float *mu, const float *gamma, uint64_t seed);
void dlco_pr_grid_destroy(dlco_pr_grid *grid);
const char *dlco_pr_grid_last_error(const dlco_pr_grid *grid);
/* n iterations of every setting (one launch) */
int  dlco_pr_grid_steps(dlco_pr_grid *grid, uint32_t n);
int  dlco_pr_grid_get_state(dlco_pr_grid *grid, uint32_t *t, float *w_host /* [G][F] or NULL */, float *dfavg_host /* [G][F] or NULL */);
/* dlco_pr_validate of every setting, equal to each setting's own: loss_val [G], regul [G], nnz [G] or NULL */
int  dlco_pr_grid_validate(dlco_pr_grid *grid, float *loss_val, float *regul, int32_t *nnz);
/* dlco_pr_stats for the settings configs[0..n) (in any order, repeats allowed), with w_host [n][F] or NULL
 * (their current w); every output is an array of n, entry i as dlco_pr_stats gives it for configs[i] */
int  dlco_pr_grid_stats(dlco_pr_grid *grid, const int32_t *configs, int32_t n, const float *w_host, const float *prparams_host,
                        int32_t pr_rows, int32_t pr_cols, int32_t nchannels, int32_t max_dim,
                        int32_t *nPR, int32_t *dim, int32_t *nzdim, float *fpr95, double *auc);
/* Settings per workgroup of later steps: 0 = the library's rule (the default), else 1, 2 or 4 (4 only for
 * F <= 5120).  Results do not depend on it; it exists for measurement.  dlco_pr_grid_group returns the
 * value the next steps will use. */
int  dlco_pr_grid_set_group(dlco_pr_grid *grid, int32_t per_group);
int32_t dlco_pr_grid_group(const dlco_pr_grid *grid);

/* ===========================================================================================
 * Descriptor generation — comp-uprjdists: the producer of pj-learn's input.
 * Replaces get_desc (src/vgg-desc.cpp:41-152), SelectPRFilters (src/misc.cpp:78-168) and the
 * per-pair loop of src/comp-uprjdists.cpp:298-349.  Descriptors are computed once per PATCH
 * (the reference recomputes both patches of every pair) and can stay in HBM for the trainer's
 * pair mode (dlco_set_pairs_device).
 * =========================================================================================== */
typedef struct dlco_desc_ctx dlco_desc_ctx;

/* InitSigma / nAngleBins / bNorm of src/comp-uprjdists.cpp:64-68 (1.4, 8, true); nAngleBins must be 8 */
int  dlco_desc_create(dlco_desc_ctx **out, float init_sigma, int32_t n_angle_bins, int32_t norm, int32_t device);
void dlco_desc_destroy(dlco_desc_ctx *ctx);
const char *dlco_desc_last_error(const dlco_desc_ctx *ctx);
/* SelectPRFilters: rows of pr_filters [8*wcols, cols] with w > 0 that are not all zero, unique,
 * ascending.  out [nsel, cols] may be NULL to query *nsel_out.  Host logic, no device needed. */
int  dlco_desc_select_filters(const float *pr_filters, int32_t rows, int32_t cols, const float *w, int32_t wcols,
                              float *out, int32_t *nsel_out);
/* sPRFilters [nsel, 4096], columns in the reference's order (pixel x*64+y of the transposed patch) */
int  dlco_desc_set_filters(dlco_desc_ctx *ctx, const float *filters_host, int32_t nsel);
int32_t dlco_desc_size(const dlco_desc_ctx *ctx);                         /* nsel * 8 */
/* get_desc of one 64x64 u8 patch: PatchTrans [4096][8] in the reference's layout */
int  dlco_desc_transform(dlco_desc_ctx *ctx, const uint8_t *patch_host, float *patch_trans_host);
/* Desc [n, nsel*8] = min(sPRFilters * get_desc(patch), 1), one row per patch [n,64,64] u8 */
int  dlco_desc_compute(dlco_desc_ctx *ctx, const uint8_t *patches_host, int64_t n, float *desc_host);
int  dlco_desc_compute_device(dlco_desc_ctx *ctx, const uint8_t *patches_host, int64_t n, float *desc_dev, int64_t ld);
/* Distance [n_pairs, nsel*8] and Label [n_pairs] (may be NULL) for pairs [n_pairs,4] =
 * (patchID1, 3DpointID1, patchID2, 3DpointID2): the two datasets comp-uprjdists writes */
int  dlco_desc_pair_dists(dlco_desc_ctx *ctx, const uint8_t *patches_host, int64_t n_patches, const int32_t *pairs_host,
                          int64_t n_pairs, float *dist_host, uint8_t *label_host);
/* comp-fulldists (src/comp-fulldists.cpp:285-369), the producer of pr-learn's input: with ALL pooling-region
 * filters set (8 rows per region), Distance [n_pairs, rows/8] = per region, the sum over its 8 rows and 8 bins of
 * (Desc2 - Desc1)^2 (cuda::subtract / pow / reduce there), and Label (may be NULL) */
int  dlco_desc_full_dists(dlco_desc_ctx *ctx, const uint8_t *patches_host, int64_t n_patches, const int32_t *pairs_host,
                          int64_t n_pairs, float *dist_host, uint8_t *label_host);
/* Streaming forms of the two calls above: the rows are handed to `sink` at most chunk_rows pairs at a time, in row
 * order (row0 = first pair of the chunk; dist [rows, cols] and label [rows] are library-owned staging buffers, valid
 * during the call only), so a tool can write each chunk as a hyperslab and check it, as the reference's loops do
 * (src/comp-uprjdists.cpp:298-349, src/comp-fulldists.cpp:300-369), without ever holding the whole Distance matrix.
 * A non-zero return of sink aborts the call with DLCO_ERR_INVALID. */
typedef int (*dlco_desc_sink_fn)(void *user, int64_t row0, int64_t rows, const float *dist, const uint8_t *label);
int  dlco_desc_pair_dists_stream(dlco_desc_ctx *ctx, const uint8_t *patches_host, int64_t n_patches, const int32_t *pairs_host,
                                 int64_t n_pairs, int64_t chunk_rows, dlco_desc_sink_fn sink, void *user);
int  dlco_desc_full_dists_stream(dlco_desc_ctx *ctx, const uint8_t *patches_host, int64_t n_patches, const int32_t *pairs_host,
                                 int64_t n_pairs, int64_t chunk_rows, dlco_desc_sink_fn sink, void *user);
/* ---- Using the learnt model: y = W * min(sPRFilters * get_desc(patch), 1), the descriptor all of the training is for.
 * The reference has no such call: W (pj-learn's dataset "W", src/pj-learn.cpp:592-597) is only ever applied to pair
 * differences inside ComputePJStats, and the per-patch form exists in OpenCV's re-encoding of the exported model alone.
 * The product follows cv::gemm's rule for floats (double accumulation, one rounding to float). ---- */
/* W [r, F] row-major, F must equal dlco_desc_size(), 1 <= r <= F; copied.  Replaces any earlier projection; rows are used
 * as given (an all-zero row gives a zero column).  dlco_desc_set_filters drops a projection whose F no longer fits. */
int  dlco_desc_set_projection(dlco_desc_ctx *ctx, const float *W_host, int32_t r, int32_t F);
int32_t dlco_desc_projected_size(const dlco_desc_ctx *ctx);               /* r, 0 when none is set */
/* Y [n, r], one row per patch [n,64,64] u8: stands in for Desc1 of src/comp-uprjdists.cpp:318-325 followed by W * Desc1.
 * The device form writes r floats per row of pitch ld >= r and leaves the other ld - r untouched. */
int  dlco_desc_describe(dlco_desc_ctx *ctx, const uint8_t *patches_host, int64_t n, float *out_host);
int  dlco_desc_describe_device(dlco_desc_ctx *ctx, const uint8_t *patches_host, int64_t n, float *out_dev, int64_t ld);
/* ---- From an image and a detector's keypoints (dlco_desc_detect below, or any other detector's): the patches are sampled on the device, so that image -> descriptors ->
 * dlco_desc_match_device never leaves HBM (a keypoint is 16 bytes on the way up, a ready patch 4 KiB).
 *   A keypoint is four floats (x, y, size, angle) with cv::KeyPoint's meaning: integer coordinates are pixel centres, angle
 * in degrees, a negative angle means none.  The patch covers size * scale_factor source pixels on a side; without
 * use_orientation every patch is upright.  The sampling rule is this library's own, in integers and bit-exact on every
 * machine: csrc/patch_rules.hpp states it.  It is NOT the sampling of OpenCV's VGG::compute, which nothing here can run
 * or pin.
 *   status [n] (may be NULL): 0 the keypoint is invalid (x, y or size not finite, size * scale_factor outside (0, 4096],
 * |x| or |y| above 2^20): its patch and its descriptor row are all zeros; 1 sampled, part of the patch lies outside the
 * image, whose border is replicated; 2 sampled wholly inside.
 *   Limits: 1 <= width, height <= 32768, pitch >= width (bytes per row), n >= 1, scale_factor finite and > 0; anything
 * else, a null pointer, or a keypoint call before an image is set is DLCO_ERR_INVALID. ---- */
/* image [height][pitch] u8, one image per context: copied */
int  dlco_desc_set_image(dlco_desc_ctx *ctx, const uint8_t *image_host, int32_t width, int32_t height, int64_t pitch);
/* the same in device memory: adopted, the caller keeps it alive and unchanged for the keypoint calls that follow */
int  dlco_desc_set_image_device(dlco_desc_ctx *ctx, const uint8_t *image_dev, int32_t width, int32_t height, int64_t pitch);
/* patches [n][64][64] u8 of keypoints [n][4], the table every patch call above takes; needs neither filters nor a projection */
int  dlco_desc_extract_patches(dlco_desc_ctx *ctx, const float *keypoints_host, int64_t n, float scale_factor,
                               int32_t use_orientation, uint8_t *patches_host, uint8_t *status_host);
/* Y [n, r]: dlco_desc_describe of those patches bit for bit, with the rows of status 0 set to zero; the patches stay in HBM.
 * The device form writes r floats per row of pitch ld >= r and leaves the other ld - r untouched. */
int  dlco_desc_describe_keypoints(dlco_desc_ctx *ctx, const float *keypoints_host, int64_t n, float scale_factor,
                                  int32_t use_orientation, float *out_host, uint8_t *status_host);
int  dlco_desc_describe_keypoints_device(dlco_desc_ctx *ctx, const float *keypoints_host, int64_t n, float scale_factor,
                                         int32_t use_orientation, float *out_dev, int64_t ld, uint8_t *status_host);
/* ---- The keypoints themselves: a detector on the image of dlco_desc_set_image*, so that image -> keypoints -> descriptors
 * -> matches runs on this library alone.  A multi-scale determinant of the Hessian on box filters over an integral image
 * (the Fast-Hessian family, whose keypoint sizes the scale factor 6.25 belongs to), by a rule of this library's own, in
 * integers and bit-exact on every machine: csrc/detect_rules.hpp states it.  It is NOT OpenCV's SURF; these two calls assign
 * no orientation (every angle is -1: dlco_desc_detect_oriented and dlco_desc_orient below do) and the refinement is one
 * parabola per axis.  Needs neither filters nor a projection.
 *   n_octaves in 1 .. 4 (filter sides 9 .. 27, 15 .. 51, 27 .. 99, 51 .. 195 on grids of step 1, 2, 4, 8); a keypoint has a
 * response R >= threshold >= 1, where R = 100 N(Dxx) N(Dyy) - 81 N(Dxy)^2 on box differences scaled by 256 / L^2: 6 553 600
 * times a determinant in squared grey levels.  *n_found is the number of keypoints of the whole image (may be NULL); they
 * are ordered by R descending, then by (octave, layer, row, column), and the first *n_out = min(n_found, max_keypoints) are
 * returned in that order: keypoints [n_out][4] = (x, y, size, -1), what dlco_desc_extract_patches /
 * dlco_desc_describe_keypoints* take, and response [n_out] (may be NULL).  Rows at and beyond *n_out are left untouched.
 * An image too small for octave 0 (below 27 x 27, or without a candidate) is no error: *n_out = 0.  The integral image is
 * kept with the image until the next dlco_desc_set_image*.  DLCO_ERR_INVALID: no image, n_octaves outside 1 .. 4,
 * threshold < 1, max_keypoints < 1, keypoints or n_out NULL.
 *   The device form writes to device memory (keypoints_dev 16-byte aligned); n_out and n_found are host pointers. */
int  dlco_desc_detect(dlco_desc_ctx *ctx, int32_t n_octaves, int64_t threshold, int64_t max_keypoints, float *keypoints_host,
                      int64_t *response_host, int64_t *n_out, int64_t *n_found);
int  dlco_desc_detect_device(dlco_desc_ctx *ctx, int32_t n_octaves, int64_t threshold, int64_t max_keypoints, float *keypoints_dev,
                             int64_t *response_dev, int64_t *n_out, int64_t *n_found);
/* HIP-event time of the last detect call by stage, ms [6]: the integral image (0 when the call found it cached), octaves
 * 0 .. 3, the selection (ordering and copy-out); the sum is dlco_desc_last_kernel_ms */
int  dlco_desc_detect_stage_ms(const dlco_desc_ctx *ctx, double *ms);
/* ---- The orientation of keypoints, so that the chain is rotation invariant on this library alone: Haar-wavelet responses
 * on the detector's integral image at 109 samples around the keypoint (scale s = round(size / 7.5) in 1 .. 128), weighted,
 * binned into 36 directions, and the strongest window of 60 degrees; csrc/orient_rules.hpp states the rule.  It is NOT the
 * orientation of OpenCV's SURF.  Everything up to the winning vector (SX, SY) is integer and bit-exact on every machine; the
 * angle is atan2(SY, SX) in degrees in [0, 360), image axes with y down (what use_orientation above expects), computed on
 * the host, and -1 (none: the patch is upright) for the vector (0, 0).
 *   angles [n] of keypoints [n][4] on the context's image; the fourth column that comes in is ignored.  vectors [n][2]
 * int64 and status [n] may be NULL; status 0: the keypoint is invalid (x, y or size not finite, size <= 0, |x| or |y| above
 * 2^20: vector (0, 0), angle -1), 1: some of the 109 samples were skipped because their Haar square leaves the image, 2: all
 * were used.  The integral image is formed if the context has none for its image and is shared with dlco_desc_detect*.
 * DLCO_ERR_INVALID: no image, n < 1, keypoints or angles NULL.
 *   Out of scope: a device-memory form of the oriented keypoints (the angle is defined through the host's atan2); more than
 * one orientation per keypoint. */
int  dlco_desc_orient(dlco_desc_ctx *ctx, const float *keypoints_host, int64_t n, float *angles_host, int64_t *vectors_host,
                      uint8_t *status_host);
/* dlco_desc_detect with the fourth column filled by the rule: the selected keypoints never leave the device before
 * orientation.  The first three columns, the responses, *n_out and *n_found are dlco_desc_detect's; dlco_desc_detect_stage_ms
 * keeps its six entries, dlco_desc_last_kernel_ms is their sum plus the orientation kernel. */
int  dlco_desc_detect_oriented(dlco_desc_ctx *ctx, int32_t n_octaves, int64_t threshold, int64_t max_keypoints, float *keypoints_host,
                               int64_t *response_host, int64_t *n_out, int64_t *n_found);
/* HIP-event time of the last orientation kernel (dlco_desc_orient, dlco_desc_detect_oriented) */
double dlco_desc_last_orient_ms(const dlco_desc_ctx *ctx);
/* per pair ||Y[a] - Y[b]||^2 [n_pairs] and Label [n_pairs] (may be NULL) for pairs [n_pairs,4]: the distances
 * ComputePJStats forms as ||W (Desc1 - Desc2)||^2 from comp-uprjdists' N x F rows (src/misc.cpp:279-292), taken from
 * the table of projected descriptors instead; that table and the un-projected rows never leave HBM */
int  dlco_desc_pair_sqdists(dlco_desc_ctx *ctx, const uint8_t *patches_host, int64_t n_patches, const int32_t *pairs_host,
                            int64_t n_pairs, float *dist_host, uint8_t *label_host);
/* ComputePJStats semantics (src/misc.cpp:266-333) on those distances, i.e. dlco_stats without the "-unproj" matrix:
 * dim (may be NULL) = rows of W with a non-zero entry, FPR at 95 % recall, area under the ROC curve */
int  dlco_desc_pair_stats(dlco_desc_ctx *ctx, const uint8_t *patches_host, int64_t n_patches, const int32_t *pairs_host,
                          int64_t n_pairs, int32_t *dim, float *fpr95, double *auc);
/* ---- Matching two descriptor tables: for every row of one, its nearest and second-nearest row in the other (the input
 * of Lowe's ratio test and of a mutual check; the tool `match` applies both).  The calls use the context for its device,
 * stream and scratch only: neither filters nor a projection have to be set.  Limits: 1 <= r <= 1024, 1 <= nq,
 * 1 <= nt < 2^31; anything else is DLCO_ERR_INVALID.
 *   Arithmetic: d(i,j) = max(0, |q_i|^2 + |t_j|^2 - 2 q_i.t_j), formed in double (dot products on the f64 matrix cores,
 * squared norms summed in double) and rounded to float once.  Products of two floats are exact in double, so the value
 * is within 2^-24 d + 4 (r + 2) 2^-53 (|q_i|^2 + |t_j|^2) of the exact distance of the float inputs.  Unlike
 * dlco_desc_pair_sqdists, which subtracts first, a row against an identical row is NOT guaranteed to give exactly 0: the
 * value is >= 0 and inside that bound.
 *   Order: candidates are ordered by the pair (returned float distance, train index), smaller distance first, equal
 * distances by smaller index; idx[i] are the first two of that order, i.e. the top two of row i of the matrix
 * dlco_desc_cross_sqdists returns.  The order of an entry's accumulation depends on r alone: no result depends on nq,
 * on where a row sits in its table, on how the work is split, or on the run.
 *   Inputs are expected to be finite; with NaN or infinity in a table the values are unspecified, every index stays in
 * [-1, nt) and nothing faults. ---- */
/* For every row i of query [nq, r]: the two rows of train [nt, r] with the smallest squared L2 distance
 * d(i,j) = sum_k (query[i][k] - train[j][k])^2.
 * idx [nq][2] / sqdist [nq][2]: column 0 the nearest, column 1 the second nearest (another j).
 * nt == 1: idx[i][1] = -1, sqdist[i][1] = +inf.  train is held in device memory whole (an allocation failure is
 * DLCO_ERR_HIP), the queries go up a chunk at a time. */
int dlco_desc_match(dlco_desc_ctx *ctx, const float *query_host, int64_t nq, const float *train_host, int64_t nt,
                    int32_t r, int32_t *idx_host, float *sqdist_host);
/* the same on tables that already live in HBM (e.g. written by dlco_desc_describe_device), row pitches ldq, ldt >= r and
 * multiples of 4, tables 16-byte aligned (rows are read in 16-byte pieces: the ceil(r/4)*4 floats at the start of every
 * row must be readable, the ones at and beyond r are ignored); idx_dev / sqdist_dev are device memory; queued on the
 * context's stream, synchronised on return */
int dlco_desc_match_device(dlco_desc_ctx *ctx, const float *query_dev, int64_t ldq, int64_t nq,
                           const float *train_dev, int64_t ldt, int64_t nt, int32_t r,
                           int32_t *idx_dev, float *sqdist_dev);
/* the whole matrix out[nq][nt] of the same distances, for small problems, tests and tools (nq * nt <= 2^28) */
int dlco_desc_cross_sqdists(dlco_desc_ctx *ctx, const float *query_host, int64_t nq, const float *train_host, int64_t nt,
                            int32_t r, float *out_host);
/* ---- Matching many pairs of images in one call.  Structure from motion, retrieval re-ranking and loop closure match one set of
 * images pairwise; a call per pair forms every image's norms once per pair it appears in and launches kernels that cannot fill
 * the device at a few thousand rows an image.  Here the set is ONE table [n_rows][r] holding the rows of image 0, then image 1,
 * and so on: seg [n_img + 1] int64, host memory in every form, seg[0] = 0, non-decreasing, image s owns the rows
 * [seg[s], seg[s + 1]) and n_rows = seg[n_img].  pairs [n_pairs][2] int32, host memory in every form, each (a, b) = (query
 * image, train image); self pairs and repeated pairs are allowed.  csrc/match_batch.hpp states how a call is cut into launches.
 *   Output: row0[p] = the running sum of the query images' row counts over the pairs in order (dlco_desc_match_pairs_rows);
 * pair p owns the rows row0[p] .. row0[p + 1] - 1 of idx [.][2] / sqdist [.][2], and those rows are, byte for byte, what
 * dlco_desc_match(query = image a, train = image b) returns: indices are rows of image b counted from its own first row, the
 * second column is -1 / +inf when b has one row (-1 / INT32_MAX on the byte line).  No result depends on the other pairs of
 * the batch, on their order, or on the run.
 *   Empty images are normal: a pair whose query image is empty owns no rows; a pair whose train image is empty gets -1 / +inf
 * (-1 / INT32_MAX) in both columns of every row.
 *   DLCO_ERR_INVALID, before the handle is used and with no output touched: a null handle or pointer, n_img < 1, n_pairs < 1 or
 * n_pairs >= 2^31, seg[0] != 0, a decreasing seg, an image of 2^31 rows or more, seg[n_img] < 1, a pair index outside
 * [0, n_img), r outside 1 .. 1024; in the device forms ld < r, ld not a multiple of 4 floats (16 bytes on the byte line), a
 * table that is not 16-byte aligned.
 *   Out of scope: a batched distance matrix; seg / pairs in device memory.
 *   In scope since: a batched verify, dlco_desc_verify_pairs_* below; guided forms of the batch,
 * dlco_desc_match_pairs_guided* below.
 *   In scope since: the step from idx / sqdist to the match list of dlco_desc_verify_pairs_* (ratio test, mutual check,
 * compaction) on the device, dlco_desc_select_pairs* below. ---- */
/* row0 [n_pairs + 1]; needs neither a context nor a device */
int dlco_desc_match_pairs_rows(const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs, int64_t *row0);
/* the table on the host, [n_rows][r] dense; idx_host / sqdist_host [row0[n_pairs]][2].  The table is held in device memory
 * whole, padded to 16-byte rows, and so are the results (an allocation failure is DLCO_ERR_HIP) */
int dlco_desc_match_pairs(dlco_desc_ctx *ctx, const float *table_host, const int64_t *seg, int32_t n_img,
                          const int32_t *pairs, int64_t n_pairs, int32_t r, int32_t *idx_host, float *sqdist_host);
/* the same on a table that already lives in HBM, as dlco_desc_match_device takes one (row pitch ld floats); idx_dev /
 * sqdist_dev are device memory; queued on the context's stream, synchronised on return */
int dlco_desc_match_pairs_device(dlco_desc_ctx *ctx, const float *table_dev, int64_t ld, const int64_t *seg, int32_t n_img,
                                 const int32_t *pairs, int64_t n_pairs, int32_t r, int32_t *idx_dev, float *sqdist_dev);
/* the plan only, nothing is launched: slices [n_pairs] = the slices of train that pair p is cut into in such a call on this
 * context's device (the most of its row ranges when a pair of more than 2^20 query rows is cut), 0 for a pair that launches
 * nothing (an empty image on either side); u8 = 0: the float line, 1: the byte line.  More than one: the pair goes through
 * partials and a merge.  For tests and tools */
int dlco_desc_match_pairs_slices(dlco_desc_ctx *ctx, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs,
                                 int32_t u8, int32_t *slices);
/* ---- Guided matching: the nearest two among the rows a homography admits.  Once a model exists (dlco_desc_verify_homography)
 * every query is matched again, but only against the train keypoints the model puts within `radius` pixels of it: the step
 * that recovers the correspondences the ratio test and the mutual check threw away in repeated structure, and the input of
 * a second, tighter verification.  csrc/guided_rules.hpp states the rule.
 *   Geometry: query_xy [nq][2] and train_xy [nt][2] float, the (x, y) of the keypoint each descriptor row belongs to; H [9]
 * row-major, it need not be normalised; radius in pixels of the image H maps to.  The pair predicate P(i, j) is the inlier
 * test of the verification, (X - u W)^2 + (Y - v W)^2 <= radius^2 W^2 with W > 0, in IEEE double + - x without fused
 * multiply-add or division, the same in every bit on every machine:
 *     h_side = 0: H maps the query image to the train image, (X, Y, W) = H (qx_i, qy_i, 1) and (u, v) = train_xy[j]
 *     h_side = 1: H maps the train image to the query image, (X, Y, W) = H (tx_j, ty_j, 1) and (u, v) = query_xy[i]
 * h_side = 1 exists so that a mutual check can swap the tables and keep H: that call sees the transpose of the same
 * admissible set.
 *   Result: idx[i] / sqdist[i] are the first two admitted candidates of row i under dlco_desc_match's (distance, index) key,
 * i.e. the top two of the finite entries of row i of the matrix dlco_desc_cross_sqdists_guided returns; every distance has
 * the bits of the same entry of dlco_desc_cross_sqdists.  Fewer than two admitted candidates leave -1 / +inf in the free
 * columns.  A point with a non-finite coordinate is admitted, and admits, where the rule's comparisons say so (a NaN fails
 * them all); indices stay in [-1, nt) and nothing faults.  The limits and the arithmetic of the distances are
 * dlco_desc_match's.
 *   DLCO_ERR_INVALID, before the handle is used and with no output touched: whatever dlco_desc_match (_device, cross_sqdists)
 * rejects, a null coordinate pointer or a null H, an entry of H that is not finite, a radius that is not finite or <= 0, an
 * h_side other than 0 or 1, a coordinate pitch below 2 (device form).
 *   Out of scope: a spatially bucketed form that skips tiles no query of which can admit a row (a distance's bits are defined
 * by the tile loop's chain of matrix-core operations, which a kernel that gathers candidates does not reproduce); the byte
 * line (there is no dlco_desc_match_u8_guided).  In scope since: a fundamental-matrix predicate, which has calls of its own,
 * dlco_desc_match_guided_epipolar below.  In scope since: the byte line, which has calls of its own with _u8 at the end of the
 * name, dlco_desc_match_guided_u8 below. ---- */
int dlco_desc_match_guided(dlco_desc_ctx *ctx, const float *query_host, const float *query_xy_host, int64_t nq,
                           const float *train_host, const float *train_xy_host, int64_t nt, int32_t r, const double *H,
                           float radius, int32_t h_side, int32_t *idx_host, float *sqdist_host);
/* the same on tables in HBM, as dlco_desc_match_device takes them.  The coordinates are device memory as well, 4-byte aligned,
 * row i at xy + i * ldxy with a pitch in floats >= 2: with pitch 4 the [n][4] keypoint rows (x, y, scale, angle) that
 * dlco_desc_detect_device wrote can be passed as they are.  H is host memory. */
int dlco_desc_match_guided_device(dlco_desc_ctx *ctx, const float *query_dev, int64_t ldq, const float *query_xy_dev,
                                  int64_t ldxy_q, int64_t nq, const float *train_dev, int64_t ldt,
                                  const float *train_xy_dev, int64_t ldxy_t, int64_t nt, int32_t r, const double *H,
                                  float radius, int32_t h_side, int32_t *idx_dev, float *sqdist_dev);
/* the matrix out[nq][nt] of dlco_desc_cross_sqdists with +inf where P fails (nq * nt <= 2^28) */
int dlco_desc_cross_sqdists_guided(dlco_desc_ctx *ctx, const float *query_host, const float *query_xy_host, int64_t nq,
                                   const float *train_host, const float *train_xy_host, int64_t nt, int32_t r,
                                   const double *H, float radius, int32_t h_side, float *out_host);
/* ---- Guided matching under a fundamental matrix: the same second pass for a scene with depth, where no single homography
 * admits the matches (dlco_desc_verify_fundamental below gives the model).  csrc/guided_epipolar_rules.hpp states the rule.
 *   Geometry: query_xy, train_xy as above; F [9] row-major, it need not be normalised; threshold in pixels.  The pair
 * predicate P(i, j) is the inlier test of that verification, the Sampson error without a division: with x = (x, y, 1) of the
 * image F applies to (src) and x' = (u, v, 1) of the other (dst),
 *     l = F x, e = (u l0 + v l1) + l2, m = F^T x' (its first two entries), S = ((l0 l0 + l1 l1) + m0 m0) + m1 m1,
 *     P = S > 0 and e e <= threshold^2 S
 * in IEEE double + - x without fused multiply-add or division, the same in every bit on every machine.  The library forms
 * l0, l1, l2 and l0 l0 + l1 l1 once per src point, u, v, m0 m0 and m1 m1 once per dst point, and spends 8 operations a pair.
 *     f_side = 0: the query image is src, x = query_xy[i] and x' = train_xy[j]: F as
 *                 dlco_desc_verify_fundamental(src = query keypoints, dst = train keypoints) returns it
 *     f_side = 1: the train image is src, x = train_xy[j] and x' = query_xy[i]
 * f_side = 1 exists so that a mutual check can swap the tables and keep F: that call sees the transpose of the same
 * admissible set.
 *   Documented and not detected: an all-zero F (what the verification returns for "no model") is valid and admits nothing,
 * S = 0; a point at an epipole of F (l = 0, or m = 0) admits every point of the other side, which is the verdict of the
 * verification's own inlier test.
 *   Result, limits, the arithmetic of the distances and the treatment of non-finite coordinates: as dlco_desc_match_guided,
 * with dlco_desc_cross_sqdists_guided_epipolar as the matrix.
 *   DLCO_ERR_INVALID, before the handle is used and with no output touched: whatever dlco_desc_match (_device, cross_sqdists)
 * rejects, a null coordinate pointer or a null F, an entry of F that is not finite, a threshold that is not finite or <= 0, an
 * f_side other than 0 or 1, a coordinate pitch below 2 (device form).
 *   Out of scope: the byte line; a spatially bucketed form; a choice between H and F.  In scope since: the byte line,
 * dlco_desc_match_guided_epipolar_u8 below. ---- */
int dlco_desc_match_guided_epipolar(dlco_desc_ctx *ctx, const float *query_host, const float *query_xy_host, int64_t nq,
                                    const float *train_host, const float *train_xy_host, int64_t nt, int32_t r, const double *F,
                                    float threshold, int32_t f_side, int32_t *idx_host, float *sqdist_host);
/* the same on tables in HBM, tables and coordinates as dlco_desc_match_guided_device takes them.  F is host memory. */
int dlco_desc_match_guided_epipolar_device(dlco_desc_ctx *ctx, const float *query_dev, int64_t ldq, const float *query_xy_dev,
                                           int64_t ldxy_q, int64_t nq, const float *train_dev, int64_t ldt,
                                           const float *train_xy_dev, int64_t ldxy_t, int64_t nt, int32_t r, const double *F,
                                           float threshold, int32_t f_side, int32_t *idx_dev, float *sqdist_dev);
/* the matrix out[nq][nt] of dlco_desc_cross_sqdists with +inf where P fails (nq * nt <= 2^28) */
int dlco_desc_cross_sqdists_guided_epipolar(dlco_desc_ctx *ctx, const float *query_host, const float *query_xy_host, int64_t nq,
                                            const float *train_host, const float *train_xy_host, int64_t nt, int32_t r,
                                            const double *F, float threshold, int32_t f_side, float *out_host);
/* ---- Guided matching of many pairs of images in one call: the last step of the two-view chain over an image set, after
 * dlco_desc_match_pairs and dlco_desc_verify_pairs_*.  table, seg, pairs, the output layout and row0 are
 * dlco_desc_match_pairs' own (dlco_desc_match_pairs_rows serves unchanged).  xy is ONE coordinate table with the rows of
 * table: row i of the table is the keypoint (x, y) at xy + i * ldxy ([n_rows][2] dense in the host forms).  The model belongs
 * to the PAIR: H (F) [n_pairs][9] row-major doubles, host memory in every form, as dlco_desc_verify_pairs_* writes H_out; the
 * same image meets another matrix in every pair it appears in.  radius / threshold and the side are one per call.
 *   Contract: pair p = (a, b) owns the rows row0[p] .. row0[p + 1] - 1, and those rows are, byte for byte, what
 * dlco_desc_match_guided (dlco_desc_match_guided_epipolar) returns for query = image a with its coordinates, train = image b
 * with its coordinates, the matrix H + 9 p and the same radius (threshold) and side.  Nothing depends on the other pairs,
 * their order or the run.
 *   An all-zero matrix is the verification's "no model": it is valid and admits nothing, the pair's rows are -1 / +inf in
 * both columns (what the single call returns) and the pair launches nothing.  A pair with an empty train image is filled the
 * same way; a pair with an empty query image owns no rows.
 *   DLCO_ERR_INVALID, before the handle is used and with no output touched: whatever dlco_desc_match_pairs (_device) rejects,
 * a null xy or matrix pointer, an entry of any of the n_pairs matrices that is not finite, a radius or threshold that is not
 * finite or <= 0, a side other than 0 or 1, ldxy < 2 or an xy that is not 4-byte aligned (device forms).
 *   csrc/match_batch.hpp states the plan: records are per pair, 32 bytes a row in one buffer per launch of at most 2^22 record
 * rows.  Out of scope: the byte line; a batched guided distance matrix; seg, pairs or the matrices in device memory; a radius
 * per pair; a choice between H and F.  In scope since: the byte line, dlco_desc_match_pairs_guided_u8 and
 * dlco_desc_match_pairs_guided_epipolar_u8 below. ---- */
int dlco_desc_match_pairs_guided(dlco_desc_ctx *ctx, const float *table_host, const float *xy_host, const int64_t *seg,
                                 int32_t n_img, const int32_t *pairs, int64_t n_pairs, int32_t r, const double *H, float radius,
                                 int32_t h_side, int32_t *idx_host, float *sqdist_host);
/* the same on a table in HBM, as dlco_desc_match_pairs_device takes it; xy_dev is device memory, 4-byte aligned, at a pitch of
 * ldxy >= 2 floats: with pitch 4 the [n][4] keypoint rows dlco_desc_detect_device wrote pass as they are.  H is host memory */
int dlco_desc_match_pairs_guided_device(dlco_desc_ctx *ctx, const float *table_dev, int64_t ld, const float *xy_dev, int64_t ldxy,
                                        const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs, int32_t r,
                                        const double *H, float radius, int32_t h_side, int32_t *idx_dev, float *sqdist_dev);
/* under fundamental matrices F [n_pairs][9]: every pair is what dlco_desc_match_guided_epipolar returns for it */
int dlco_desc_match_pairs_guided_epipolar(dlco_desc_ctx *ctx, const float *table_host, const float *xy_host, const int64_t *seg,
                                          int32_t n_img, const int32_t *pairs, int64_t n_pairs, int32_t r, const double *F,
                                          float threshold, int32_t f_side, int32_t *idx_host, float *sqdist_host);
int dlco_desc_match_pairs_guided_epipolar_device(dlco_desc_ctx *ctx, const float *table_dev, int64_t ld, const float *xy_dev,
                                                 int64_t ldxy, const int64_t *seg, int32_t n_img, const int32_t *pairs,
                                                 int64_t n_pairs, int32_t r, const double *F, float threshold, int32_t f_side,
                                                 int32_t *idx_dev, float *sqdist_dev);
/* ---- Eight-bit descriptors: a table of bytes is a quarter of the float one, and its distances are integers.
 *   The quantiser is a scale s > 0 and an offset o[r]; csrc/quant_rules.hpp states the rule.  One element:
 * t = y - o_k in float, v = t * s in float (two roundings, never an FMA), q = rintf(v) (half to even); the byte is 0 if v is
 * NaN, else clamp(q, 0, 255).  It is this library's own rule, NOT OpenCV's VGG dsc_normalize, which nothing here can run or
 * pin.  One global scale and a per-dimension offset: distances do not see the offset, so ||u_a - u_b|| ~ s ||y_a - y_b||
 * with an error of at most 1 per coordinate while nothing clamps.
 *   Limits: 1 <= r <= 1024, n >= 1, scale finite and > 0, offsets finite (NULL = all zero); anything else, or a null
 * pointer, is DLCO_ERR_INVALID. ---- */
/* The quantiser fitted to a sample Y [n, r] of finite values: o_k = min_i Y[i][k], s = 255 / max_k (max_i Y[i][k] - o_k)
 * with the subtraction in float, s = 1 when that range is 0: the sample itself never clamps.  A non-finite entry (or a
 * range beyond float) is DLCO_ERR_INVALID.  Host logic, no device needed. */
int  dlco_desc_quant_fit(const float *Y_host, int64_t n, int32_t r, float *scale, float *offset_out);
/* out_u8 [n, r] of Y [n, r] by the rule above.  Host logic, no device needed. */
int  dlco_desc_quantize(const float *Y_host, int64_t n, int32_t r, float scale, const float *offset, uint8_t *out_u8);
/* Attaches a quantiser to the context for the _u8 calls below: copied, replaces any earlier one.  dlco_desc_set_projection
 * drops a quantiser whose r is not the projection's. */
int  dlco_desc_set_quantizer(dlco_desc_ctx *ctx, float scale, const float *offset, int32_t r);
/* The bytes dlco_desc_quantize gives on the rows of dlco_desc_describe / dlco_desc_describe_keypoints, bit for bit, quantised
 * on the device (a keypoint row of status 0 is therefore the quantisation of the zero vector).  The device forms write r
 * bytes per row of pitch ld >= r bytes and leave the other ld - r untouched.  Without a quantiser, or with one whose r is not
 * dlco_desc_projected_size(): DLCO_ERR_INVALID. */
int  dlco_desc_describe_u8(dlco_desc_ctx *ctx, const uint8_t *patches_host, int64_t n, uint8_t *out_host);
int  dlco_desc_describe_u8_device(dlco_desc_ctx *ctx, const uint8_t *patches_host, int64_t n, uint8_t *out_dev, int64_t ld);
int  dlco_desc_describe_keypoints_u8(dlco_desc_ctx *ctx, const float *keypoints_host, int64_t n, float scale_factor,
                                     int32_t use_orientation, uint8_t *out_host, uint8_t *status_host);
int  dlco_desc_describe_keypoints_u8_device(dlco_desc_ctx *ctx, const float *keypoints_host, int64_t n, float scale_factor,
                                            int32_t use_orientation, uint8_t *out_dev, int64_t ld, uint8_t *status_host);
/* Matching two tables of bytes, the limits of dlco_desc_match: 1 <= r <= 1024, 1 <= nq, 1 <= nt < 2^31.
 *   d(i,j) = sum_k (query[i][k] - train[j][k])^2 as an int32, at most 1024 * 255^2 = 66 585 600.  The distances are exact:
 * integer dot products on the int8 matrix cores, no rounding anywhere, so the result depends on nothing but the bytes.
 *   Order: candidates are ordered by (d, train index); idx[i] / sqdist[i] are the first two of that order, i.e. the top two
 * of row i of the matrix dlco_desc_cross_sqdists_u8 returns.  nt == 1: idx[i][1] = -1, sqdist[i][1] = INT32_MAX. */
int dlco_desc_match_u8(dlco_desc_ctx *ctx, const uint8_t *query_u8, int64_t nq, const uint8_t *train_u8, int64_t nt,
                       int32_t r, int32_t *idx_host, int32_t *sqdist_host);
/* the same on tables that already live in HBM (e.g. written by dlco_desc_describe_u8_device): pitches ldq, ldt in bytes,
 * >= r and multiples of 16, tables 16-byte aligned (rows are read in 16-byte pieces: the ceil(r/16)*16 bytes at the start of
 * every row must be readable, the ones at and beyond r are ignored); idx_dev / sqdist_dev are device memory; queued on the
 * context's stream, synchronised on return */
int dlco_desc_match_u8_device(dlco_desc_ctx *ctx, const uint8_t *query_dev, int64_t ldq, int64_t nq,
                              const uint8_t *train_dev, int64_t ldt, int64_t nt, int32_t r,
                              int32_t *idx_dev, int32_t *sqdist_dev);
/* the whole matrix out[nq][nt] of the same distances, for small problems, tests and tools (nq * nt <= 2^28) */
int dlco_desc_cross_sqdists_u8(dlco_desc_ctx *ctx, const uint8_t *query_u8, int64_t nq, const uint8_t *train_u8, int64_t nt,
                               int32_t r, int32_t *out_host);
/* dlco_desc_match_pairs on a table of bytes (see there for seg, pairs, the output layout, empty images and the checks): every
 * pair's rows are what dlco_desc_match_u8 returns for it */
int dlco_desc_match_pairs_u8(dlco_desc_ctx *ctx, const uint8_t *table_u8, const int64_t *seg, int32_t n_img,
                             const int32_t *pairs, int64_t n_pairs, int32_t r, int32_t *idx_host, int32_t *sqdist_host);
/* the same on a table in HBM, as dlco_desc_match_u8_device takes one (row pitch ld bytes, a multiple of 16) */
int dlco_desc_match_pairs_u8_device(dlco_desc_ctx *ctx, const uint8_t *table_dev, int64_t ld, const int64_t *seg, int32_t n_img,
                                    const int32_t *pairs, int64_t n_pairs, int32_t r, int32_t *idx_dev, int32_t *sqdist_dev);
/* ---- Guided matching on byte tables: the second pass of the two-view chain for descriptors that were quantised, so that the
 * float tables need not be kept.  Ten calls, each its float counterpart argument for argument with uint8_t tables, int32_t
 * distances and, in the device forms, pitches in bytes that are multiples of 16 (as dlco_desc_match_u8_device takes tables).
 * The geometry, the two models, the pair predicate P(i, j), the sides and the coordinates are those of dlco_desc_match_guided
 * and dlco_desc_match_guided_epipolar above: the verdict is formed by the same rule headers in the same IEEE double
 * arithmetic, as a further epilogue of the int8 tile loop.
 *   Result: idx[i] / sqdist[i] are the first two admitted candidates of dlco_desc_match_u8's (d, train index) order, i.e. the
 * top two of the entries below INT32_MAX of row i of the matrix dlco_desc_cross_sqdists_guided_u8
 * (dlco_desc_cross_sqdists_guided_epipolar_u8) returns, which is the matrix of dlco_desc_cross_sqdists_u8 with INT32_MAX where P
 * fails; every distance is the integer dlco_desc_cross_sqdists_u8 gives for that entry.  Fewer than two admitted candidates
 * leave -1 / INT32_MAX in the free columns.  Non-finite coordinates: as dlco_desc_match_guided.
 *   The pair calls: pair p owns the rows row0[p] .. row0[p + 1] - 1, and they are, byte for byte, what the single byte guided
 * call returns for that pair with the matrix M + 9 p.  An all-zero matrix ("no model") launches nothing and fills -1 /
 * INT32_MAX; a pair with an empty train image likewise.
 *   DLCO_ERR_INVALID, before the handle is used and with no output touched: whatever the byte call of the same form
 * (dlco_desc_match_u8, _device, dlco_desc_cross_sqdists_u8, dlco_desc_match_pairs_u8, _device) and the float guided call of
 * the same form reject: a null pointer; an entry of a matrix that is not finite; a radius or threshold that is not finite or
 * <= 0; a side other than 0 or 1; a coordinate pitch below 2 or coordinates that are not 4-byte aligned (device forms); a
 * table pitch below r or not a multiple of 16, or a table that is not 16-byte aligned (device forms); the limits on nq, nt
 * and r, and nq * nt <= 2^28 for the matrices.
 *   Out of scope: a slicing rule tuned to the guided forms' occupancy (they use the byte matcher's); a spatially bucketed
 * form; a batched guided matrix; seg, pairs or the matrices in device memory; a choice between H and F. ---- */
int dlco_desc_match_guided_u8(dlco_desc_ctx *ctx, const uint8_t *query_u8, const float *query_xy_host, int64_t nq,
                              const uint8_t *train_u8, const float *train_xy_host, int64_t nt, int32_t r, const double *H,
                              float radius, int32_t h_side, int32_t *idx_host, int32_t *sqdist_host);
int dlco_desc_match_guided_u8_device(dlco_desc_ctx *ctx, const uint8_t *query_dev, int64_t ldq, const float *query_xy_dev,
                                     int64_t ldxy_q, int64_t nq, const uint8_t *train_dev, int64_t ldt,
                                     const float *train_xy_dev, int64_t ldxy_t, int64_t nt, int32_t r, const double *H,
                                     float radius, int32_t h_side, int32_t *idx_dev, int32_t *sqdist_dev);
/* the matrix out[nq][nt] of dlco_desc_cross_sqdists_u8 with INT32_MAX where P fails (nq * nt <= 2^28) */
int dlco_desc_cross_sqdists_guided_u8(dlco_desc_ctx *ctx, const uint8_t *query_u8, const float *query_xy_host, int64_t nq,
                                      const uint8_t *train_u8, const float *train_xy_host, int64_t nt, int32_t r,
                                      const double *H, float radius, int32_t h_side, int32_t *out_host);
int dlco_desc_match_guided_epipolar_u8(dlco_desc_ctx *ctx, const uint8_t *query_u8, const float *query_xy_host, int64_t nq,
                                       const uint8_t *train_u8, const float *train_xy_host, int64_t nt, int32_t r,
                                       const double *F, float threshold, int32_t f_side, int32_t *idx_host, int32_t *sqdist_host);
int dlco_desc_match_guided_epipolar_u8_device(dlco_desc_ctx *ctx, const uint8_t *query_dev, int64_t ldq, const float *query_xy_dev,
                                              int64_t ldxy_q, int64_t nq, const uint8_t *train_dev, int64_t ldt,
                                              const float *train_xy_dev, int64_t ldxy_t, int64_t nt, int32_t r, const double *F,
                                              float threshold, int32_t f_side, int32_t *idx_dev, int32_t *sqdist_dev);
int dlco_desc_cross_sqdists_guided_epipolar_u8(dlco_desc_ctx *ctx, const uint8_t *query_u8, const float *query_xy_host, int64_t nq,
                                               const uint8_t *train_u8, const float *train_xy_host, int64_t nt, int32_t r,
                                               const double *F, float threshold, int32_t f_side, int32_t *out_host);
int dlco_desc_match_pairs_guided_u8(dlco_desc_ctx *ctx, const uint8_t *table_u8, const float *xy_host, const int64_t *seg,
                                    int32_t n_img, const int32_t *pairs, int64_t n_pairs, int32_t r, const double *H,
                                    float radius, int32_t h_side, int32_t *idx_host, int32_t *sqdist_host);
int dlco_desc_match_pairs_guided_u8_device(dlco_desc_ctx *ctx, const uint8_t *table_dev, int64_t ld, const float *xy_dev,
                                           int64_t ldxy, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs,
                                           int32_t r, const double *H, float radius, int32_t h_side, int32_t *idx_dev,
                                           int32_t *sqdist_dev);
int dlco_desc_match_pairs_guided_epipolar_u8(dlco_desc_ctx *ctx, const uint8_t *table_u8, const float *xy_host, const int64_t *seg,
                                             int32_t n_img, const int32_t *pairs, int64_t n_pairs, int32_t r, const double *F,
                                             float threshold, int32_t f_side, int32_t *idx_host, int32_t *sqdist_host);
int dlco_desc_match_pairs_guided_epipolar_u8_device(dlco_desc_ctx *ctx, const uint8_t *table_dev, int64_t ld, const float *xy_dev,
                                                    int64_t ldxy, const int64_t *seg, int32_t n_img, const int32_t *pairs,
                                                    int64_t n_pairs, int32_t r, const double *F, float threshold, int32_t f_side,
                                                    int32_t *idx_dev, int32_t *sqdist_dev);
/* ---- Geometric verification: a homography between the two sides of a match list, so that the chain ends in a verified
 * result on this library alone.  A deterministic RANSAC by a rule of this library's own, csrc/verify_rules.hpp states it:
 * n_hyp hypotheses from four matches each (a counter-based sampler on `seed`), scored on the device by forward transfer
 * error (X - u W)^2 + (Y - v W)^2 <= threshold^2 W^2 with W > 0, the best by (count descending, hypothesis ascending), then at
 * most `refine` rounds of a normalised DLT on the inliers, formed on the host and scored on the device.  Every step of the
 * device path is IEEE double + - x without fused multiply-add or division, counts are integers: the answer is the same in
 * every bit on every machine.  It is NOT cv::findHomography.  Like the matcher, the calls use the context for its device,
 * stream and scratch only.
 *   src_xy, dst_xy [m][2] float (x, y), expected finite with |x|, |y| <= 2^20 (not checked: a match with a non-finite
 * coordinate is never an inlier).  H_out [9] row-major maps src to dst, max |H| in [1, 2); inlier_host [m] (0 / 1) and
 * best_hyp may be NULL.  No model (no valid hypothesis) is no error: DLCO_OK with *n_inliers = 0, *best_hyp = -1, H and the
 * mask all zero.
 *   DLCO_ERR_INVALID, before the handle is used and with no output touched: a null handle, a required pointer NULL, m < 4 or
 * m >= 2^31, a threshold that is not finite or <= 0, n_hyp outside 1 .. 2^20, refine outside 0 .. 8.
 *   Out of scope of this call: a device-memory form (the match list is filtered on the host); a fundamental or essential matrix
 * (the fundamental matrix has calls of its own, dlco_desc_verify_fundamental below; an essential matrix has none);
 * symmetric transfer error; an adaptive hypothesis count.
 *   In scope since: filtering the match list on the device, dlco_desc_select_pairs* below, which writes the lists of
 * dlco_desc_verify_pairs_* from a batched answer in device memory; dlco_desc_verify_pairs_*_device below take them there. */
int  dlco_desc_verify_homography(dlco_desc_ctx *ctx, const float *src_xy_host, const float *dst_xy_host, int64_t m, float threshold,
                                 int32_t n_hyp, uint64_t seed, int32_t refine, double *H_out, uint8_t *inlier_host, int64_t *n_inliers,
                                 int32_t *best_hyp);
/* every hypothesis of that call and its inlier count, H_all [n_hyp][9] (all zero: invalid) and count [n_hyp]: for tests and
 * tools, what dlco_desc_cross_sqdists is to the matcher */
int  dlco_desc_verify_hypotheses(dlco_desc_ctx *ctx, const float *src_xy_host, const float *dst_xy_host, int64_t m, float threshold,
                                 int32_t n_hyp, uint64_t seed, double *H_all_host, int32_t *count_host);
/* ---- The same verification against a fundamental matrix F, x'^T F x = 0 with x = (x, y, 1) of src and x' = (u, v, 1) of dst:
 * the model of a camera that moves in front of a scene with depth, where a homography keeps one plane only.
 * csrc/epipolar_rules.hpp states the rule: n_hyp hypotheses from eight matches each (the same sampler), the linear eight-point
 * system of locally normalised points solved by Gaussian elimination with complete pivoting, scored on the device by the
 * Sampson error without a division, e^2 <= threshold^2 S with S > 0, the same selection, then at most `refine` rounds on the
 * host: Hartley normalisation, the smallest eigenvector of the 9 x 9 normal matrix by a cyclic Jacobi rule, the nearest
 * rank-2 matrix, scored on the device.  The device path is IEEE double + - x / without fused multiply-add, the host adds
 * sqrt: the answer is the same in every bit on every machine.  It is NOT cv::findFundamentalMat.
 *   The arguments, the optional outputs, "no model" and DLCO_ERR_INVALID are dlco_desc_verify_homography's, except m >= 8.
 * F_out [9] row-major, max |F| in [1, 2), its first entry of that magnitude positive.  With refine = 0, or when no round was
 * accepted, F is the linear eight-point hypothesis, which need not be singular; after an accepted round it is of rank 2 up to
 * rounding.
 *   Degeneracy is documented and not detected: matches related by a homography (a plane, a camera that only rotates, a
 * shifted image) satisfy a three-dimensional family of F, and the call returns some member of it.
 *   Out of scope: a choice between H and F; a seven-point solver; an essential matrix; an adaptive hypothesis count.
 * In scope since: an epipolar predicate for guided matching, dlco_desc_match_guided_epipolar above. */
int  dlco_desc_verify_fundamental(dlco_desc_ctx *ctx, const float *src_xy_host, const float *dst_xy_host, int64_t m, float threshold,
                                  int32_t n_hyp, uint64_t seed, int32_t refine, double *F_out, uint8_t *inlier_host, int64_t *n_inliers,
                                  int32_t *best_hyp);
/* every hypothesis of that call and its inlier count, F_all [n_hyp][9] (all zero: invalid) and count [n_hyp] */
int  dlco_desc_verify_fundamental_hypotheses(dlco_desc_ctx *ctx, const float *src_xy_host, const float *dst_xy_host, int64_t m,
                                             float threshold, int32_t n_hyp, uint64_t seed, double *F_all_host, int32_t *count_host);
/* ---- Verifying many pairs in one call.  Every caller of dlco_desc_match_pairs verifies each matched pair next, and a call per
 * pair is launch-bound: four launches of a few dozen workgroups and a stream synchronisation per refit round for a few
 * thousand matches.  Here the match lists of all pairs are ONE list: src_xy, dst_xy [M][2] float, host memory; moff [n_pairs + 1] int64,
 * host memory, moff[0] = 0, non-decreasing, pair p owns the matches [moff[p], moff[p + 1]) and M = moff[n_pairs] (match-pairs'
 * MatchOffsets).  csrc/verify_batch.hpp states how a call is cut into launches; a launch carries the workgroups of many pairs,
 * and the refit rounds of all pairs still refining share one mask launch per round.
 *   Output: M_out [n_pairs][9], inlier_host [M] (may be NULL), n_inliers [n_pairs], best_hyp [n_pairs] (may be NULL).  Pair p's
 * matrix, its slice of the mask, its count and its best hypothesis are, byte for byte, what dlco_desc_verify_homography
 * (dlco_desc_verify_fundamental) returns for src_xy + 2 moff[p], dst_xy + 2 moff[p], m_p and the same threshold, n_hyp, seed
 * and refine: one seed serves all pairs, as a loop of single calls would use it.  No result depends on the other pairs of the
 * batch, on their order, or on the run.
 *   A pair with fewer matches than a sample (4, or 8 for the fundamental matrix; 0 is normal) is no error: it gets the "no
 * model" answer, matrix and mask zero, count 0, best -1; in the hypotheses forms all-zero matrices and counts.  moff[n_pairs]
 * = 0 is valid: every pair gets that answer.
 *   DLCO_ERR_INVALID, before the handle is used and with no output touched: a null handle or required pointer, n_pairs < 1 or
 * n_pairs >= 2^31, moff[0] != 0, a decreasing moff, a pair of 2^31 matches or more, a threshold, n_hyp or refine outside the
 * single call's limits.
 *   Out of scope: a device-memory form; seeds or thresholds per pair; a choice between H and F.
 *   In scope since: the device-memory form, dlco_desc_verify_pairs_*_device below, with its refit on the device. ---- */
int  dlco_desc_verify_pairs_homography(dlco_desc_ctx *ctx, const float *src_xy_host, const float *dst_xy_host, const int64_t *moff,
                                       int64_t n_pairs, float threshold, int32_t n_hyp, uint64_t seed, int32_t refine, double *H_out,
                                       uint8_t *inlier_host, int64_t *n_inliers, int32_t *best_hyp);
int  dlco_desc_verify_pairs_fundamental(dlco_desc_ctx *ctx, const float *src_xy_host, const float *dst_xy_host, const int64_t *moff,
                                        int64_t n_pairs, float threshold, int32_t n_hyp, uint64_t seed, int32_t refine, double *F_out,
                                        uint8_t *inlier_host, int64_t *n_inliers, int32_t *best_hyp);
/* every hypothesis of every pair and its count, M_all [n_pairs][n_hyp][9] and count [n_pairs][n_hyp]: for tests and tools */
int  dlco_desc_verify_pairs_hypotheses(dlco_desc_ctx *ctx, const float *src_xy_host, const float *dst_xy_host, const int64_t *moff,
                                       int64_t n_pairs, float threshold, int32_t n_hyp, uint64_t seed, double *H_all_host,
                                       int32_t *count_host);
int  dlco_desc_verify_pairs_fundamental_hypotheses(dlco_desc_ctx *ctx, const float *src_xy_host, const float *dst_xy_host,
                                                   const int64_t *moff, int64_t n_pairs, float threshold, int32_t n_hyp, uint64_t seed,
                                                   double *F_all_host, int32_t *count_host);
/* the plan only, needs neither a context nor a device: launch_of_pair [n_pairs] = the launch that carries pair p in such a
 * call, -1 for a pair that launches nothing (fewer matches than a sample); fundamental = 0: the homography, 1: the fundamental
 * matrix.  DLCO_ERR_INVALID as above, and for another value of fundamental.  For tests and tools */
int  dlco_desc_verify_pairs_launches(const int64_t *moff, int64_t n_pairs, int32_t n_hyp, int32_t fundamental, int32_t *launch_of_pair);
/* ---- The batched verification on lists in device memory: the step behind dlco_desc_select_pairs_device, so that the chain
 * match_pairs_device -> select_pairs_device -> verify_pairs_*_device -> match_pairs_guided*_device moves only moff, the matrices
 * (72 bytes per pair) and the counts to the host.  src_xy_dev, dst_xy_dev [M][2] float in device memory, as
 * dlco_desc_select_pairs_device wrote them, 8-byte aligned (the kernels read pairs of floats); moff [n_pairs + 1] host memory, as
 * that call returns it.  A launch of the plan (csrc/verify_batch.hpp, unchanged) reads its range of the lists in place: nothing
 * is copied.  The refit runs on the device: a kernel forms the round's matrices from the current masks (refit_pairs_kernel,
 * csrc/kernels_verify.hip: the sums of the rule in ascending match index, one lane per sum; the rule headers' elimination or
 * Jacobi), the mask kernel scores them, a third kernel is verify_rules::refit_step.  Per launch the hypotheses, the scoring, the
 * selection, the first mask and the `refine` rounds are queued without a host sync; then one download of matrices, counts and
 * keys, and one sync.
 *   Output: M_out [n_pairs][9], n_inliers [n_pairs] and best_hyp [n_pairs] (may be NULL) in host memory; inlier_dev [M] (may be
 * NULL) in device memory, written in place, the slices of pairs below the sample zeroed.  Pair p's matrix, mask slice, count
 * and best hypothesis are, byte for byte, what dlco_desc_verify_pairs_homography (dlco_desc_verify_pairs_fundamental) returns for
 * the same lists on the host: the refit kernel calls the rule headers' functions, and its double sqrt and division are the
 * correctly rounded ones.
 *   "No model", a pair below the sample, M = 0 and DLCO_ERR_INVALID are those of the host forms; a src_xy_dev or dst_xy_dev
 * that is not 8-byte aligned is DLCO_ERR_INVALID as well.
 *   Out of scope: the host forms and the tools on these rounds (they keep their host refit); moff in device memory. ---- */
int  dlco_desc_verify_pairs_homography_device(dlco_desc_ctx *ctx, const float *src_xy_dev, const float *dst_xy_dev, const int64_t *moff,
                                              int64_t n_pairs, float threshold, int32_t n_hyp, uint64_t seed, int32_t refine, double *H_out,
                                              uint8_t *inlier_dev, int64_t *n_inliers, int32_t *best_hyp);
int  dlco_desc_verify_pairs_fundamental_device(dlco_desc_ctx *ctx, const float *src_xy_dev, const float *dst_xy_dev, const int64_t *moff,
                                               int64_t n_pairs, float threshold, int32_t n_hyp, uint64_t seed, int32_t refine, double *F_out,
                                               uint8_t *inlier_dev, int64_t *n_inliers, int32_t *best_hyp);
/* one round of the refit kernel on masks of the caller's, for tests and tools: lists and moff as dlco_desc_verify_pairs_* take
 * them, mask_host [M] (0 / non-zero), fundamental = 0 or 1.  M_out [n_pairs][9] is the round's matrix, byte for byte
 * verify_rules::refit_round's (epipolar_rules::refit_round's) on the pair's slice; ok [n_pairs] = 1.  A rejected round, and a
 * pair below the sample, give ok = 0 and a zero matrix.  DLCO_ERR_INVALID as the _pairs forms, and for another value of
 * fundamental */
int  dlco_desc_verify_pairs_refit_round(dlco_desc_ctx *ctx, const float *src_xy_host, const float *dst_xy_host, const int64_t *moff,
                                        int64_t n_pairs, const uint8_t *mask_host, int32_t fundamental, double *M_out, uint8_t *ok);
/* ---- Selecting matches: from the answer of a dlco_desc_match_pairs* call to the lists of a dlco_desc_verify_pairs_* call.  The
 * link between the two: Lowe's ratio test, the mutual check and the compaction into (query, train) rows, on the device, so that
 * a caller whose idx / sqdist live in HBM need not download them, restate the rule and gather coordinates.
 * csrc/select_rules.hpp states the rule; it is the rule of the tools match and match-pairs (-ratio, -cross).
 *   Input: seg, n_img, pairs, n_pairs as the match_pairs call took them; idx / sqdist [R][2], R = row0[n_pairs], exactly what that
 * call wrote, plain or guided, float or byte line (the _u8 forms take the int32 distances).  seg, pairs, back_row0 and moff are
 * host memory in every form.  Row i of pair p = (a, b), with j = idx[i][0] and nt_b the rows of image b:
 *     never a match if j < 0 or j >= nt_b, decided before anything is read at j: no content of idx makes the call read outside
 *   a buffer;
 *     ratio != 0 (it must lie in (0, 1]; 0: no ratio test): kept iff idx[i][1] == -1 or
 *   (double)sqdist[i][0] < (double)ratio * (double)ratio * (double)sqdist[i][1]; equality is dropped, and so is 0 < 0;
 *     back_idx != NULL (NULL: no mutual check): back_idx [n_back_rows][2] holds the reverse answers, back_row0 [n_pairs] the
 *   first row of pair p's, image b's rows matched against image a, or -1 for "no mutual check for this pair"; kept iff
 *   back_idx[back_row0[p] + j][0] == i.  back_idx may be idx itself with back_row0[p] = row0[q], q the reversed pair of the same
 *   batch (how match-pairs -cross batches them), or the answer of a second call (how the guided tools run side 1).
 *     xy != NULL (NULL: no coordinates, and then src_xy and dst_xy must be NULL): the batch's coordinate table as
 *   dlco_desc_match_pairs_guided* takes it, [seg[n_img]][2] on the host, pitch ldxy >= 2 floats on the device (4 takes the rows
 *   dlco_desc_detect_device wrote).
 *   Output: moff [n_pairs + 1]; matches [.][2] int32, (i, j) as rows of the pair's own two images; dist [.], sqdist[i][0], float
 * or int32; src_xy, dst_xy [.][2] float, the (x, y) of row i of image a and row j of image b.  The caller provides R entries of
 * each list; the first M = moff[n_pairs] are written, pairs in order and rows ascending inside a pair, the rest is not touched.
 * moff, src_xy and dst_xy are the arguments of dlco_desc_verify_pairs_*.  Everything is an integer or a comparison: no result
 * depends on the other pairs of the batch or on the run.  Empty images, pairs that keep nothing and M = 0 are normal.
 *   The device forms are queued on the context's stream and synchronised on return.  Like the matcher, the calls use the context
 * for its device, stream and scratch only.
 *   DLCO_ERR_INVALID, before the handle is used and with no output touched: a null handle or required pointer (seg, pairs, idx,
 * sqdist, moff, matches, dist), whatever dlco_desc_match_pairs rejects of seg / pairs, R >= 2^31, a ratio that is NaN, negative or
 * above 1, back_idx without back_row0, a back_row0[p] below -1 or one whose nt_b rows end beyond n_back_rows, src_xy or dst_xy
 * without xy or only one of the two, ldxy < 2 with xy.
 *   Out of scope: seg / pairs in device memory; the tools, which keep their host rule; single-pair entry points: a batch of one pair is the
 * single call.
 *   In scope since: the tools.  match and match-pairs make their lists with the host forms of these calls (cli/match_tool.hpp),
 * match as a batch of one pair with the reverse answer of its second call as back_idx; no host restatement of the rule is
 * left in them.  Also a device-memory form of dlco_desc_verify_pairs_*: dlco_desc_verify_pairs_*_device above take src_xy_dev
 * and dst_xy_dev as these calls write them. ---- */
int  dlco_desc_select_pairs(dlco_desc_ctx *ctx, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs,
                            const int32_t *idx_host, const float *sqdist_host, float ratio, const int32_t *back_idx_host,
                            const int64_t *back_row0, int64_t n_back_rows, const float *xy_host, int64_t *moff, int32_t *matches_host,
                            float *dist_host, float *src_xy_host, float *dst_xy_host);
int  dlco_desc_select_pairs_device(dlco_desc_ctx *ctx, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs,
                                   const int32_t *idx_dev, const float *sqdist_dev, float ratio, const int32_t *back_idx_dev,
                                   const int64_t *back_row0, int64_t n_back_rows, const float *xy_dev, int64_t ldxy, int64_t *moff,
                                   int32_t *matches_dev, float *dist_dev, float *src_xy_dev, float *dst_xy_dev);
/* the same on the answer of the byte line (dlco_desc_match_pairs_u8, dlco_desc_match_pairs_guided*_u8): int32 distances */
int  dlco_desc_select_pairs_u8(dlco_desc_ctx *ctx, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs,
                               const int32_t *idx_host, const int32_t *sqdist_host, float ratio, const int32_t *back_idx_host,
                               const int64_t *back_row0, int64_t n_back_rows, const float *xy_host, int64_t *moff, int32_t *matches_host,
                               int32_t *dist_host, float *src_xy_host, float *dst_xy_host);
int  dlco_desc_select_pairs_u8_device(dlco_desc_ctx *ctx, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs,
                                      const int32_t *idx_dev, const int32_t *sqdist_dev, float ratio, const int32_t *back_idx_dev,
                                      const int64_t *back_row0, int64_t n_back_rows, const float *xy_dev, int64_t ldxy, int64_t *moff,
                                      int32_t *matches_dev, int32_t *dist_dev, float *src_xy_dev, float *dst_xy_dev);
/* HIP-event time of the kernels of the last compute / describe call (transform, pooling, projection, and the sampling
 * for the keypoint calls; extract_patches: the sampling alone); the pair_sqdists /
 * pair_stats calls add their distance kernel; after a match / cross_sqdists call, float or _u8, the time of its kernels
 * (norms, tile loop, merge of the slices, and for the guided forms the kernel that writes the records, launched once per side for the epipolar ones; the guided _u8 calls, single or pairs, likewise: norms, record kernels, tile loop, merge); after a match_pairs call, float or _u8, every kernel of the call (the norms of
 * the whole table, the fill of the pairs with an empty train image, the tile loop and the merge of every launch); the _u8 forms of describe add their quantising kernel; after a detect call the
 * detector's kernels (the integral image when the call formed it, the octaves, the selection; detect_oriented adds the
 * orientation kernel); after an orient call the orientation kernel and the integral image when the call formed it; after a
 * verify call the verify kernels, of either model, as after a verify_pairs call of one pair, which is what a verify call
 * runs; after a verify_pairs call every kernel of the call (the hypotheses and the scoring of every launch; the model forms,
 * verify_homography, verify_fundamental, verify_pairs_homography and verify_pairs_fundamental, add the selection, the mask
 * of the best models and the mask launch of every lockstep refit round; the _device forms all of that and, for every round,
 * the refit and the step kernel; verify_pairs_refit_round its one refit launch per launch of the plan); after a select_pairs call, float or _u8, its kernels
 * (the flags, the scan of the block counts, the scatter, the match offsets; 0 when the batch has no row) */
double dlco_desc_last_kernel_ms(const dlco_desc_ctx *ctx);
/* ---- Building tracks: from the match lists and inlier masks of many ordered pairs to the keypoints that are one scene point
 * across all images, the step behind dlco_desc_select_pairs* and dlco_desc_verify_pairs_*, on the device, so that a caller whose
 * lists live in HBM need not download them, run a union-find and upload the result.  csrc/track_rules.hpp states the rule.
 *   Input: seg, n_img, pairs, n_pairs as the match_pairs call took them; moff [n_pairs + 1] and matches [M][2] int32,
 * M = moff[n_pairs], as dlco_desc_select_pairs* wrote them; keep [M] (may be NULL: every match counts), 0 / non-zero, the inlier
 * mask as dlco_desc_verify_pairs_* wrote it.  seg, pairs, moff, n_tracks and counts are host memory in every form.
 *     Nodes: the rows of the batch's table, N = seg[n_img]; row i of image a is node seg[a] + i.
 *     Edges: match m of pair p = (a, b) with matches[m] = (i, j) joins the nodes seg[a] + i and seg[b] + j.  It is skipped, not
 *   an error, if keep != NULL && keep[m] == 0, or if i or j lies outside its image, decided before anything is indexed with it:
 *   no content of matches makes the call read or write outside a buffer.  Duplicate edges, both directions of a pair and
 *   edges with equal ends are harmless.
 *     label[g] is the smallest node of g's connected component.  A track is a component of at least min_len nodes
 *   (min_len >= 2) and, when unique != 0, without two nodes in one image; a conflicting component is dropped whole.
 *   Output: counts[0] the components of at least 2 nodes, counts[1] those of fewer than min_len nodes, counts[2] those of at
 * least min_len nodes dropped for a conflict; *n_tracks = counts[0] - counts[1] - counts[2].  Tracks ascend in label and,
 * inside a track, nodes ascend in id, so images ascend as well: toff [n_tracks + 1] int64 with toff[0] = 0, obs [toff[n_tracks]]
 * int32 node ids, track_of [N] int32 the node's track or -1, label [N] int32 (may be NULL).  The caller provides N / 2 + 1 entries
 * of toff and N of obs; entries beyond those used are not touched.  Everything is an integer or a comparison: no result depends
 * on the order of the matches, on scheduling or on the run.  M = 0, N = 0, empty images and pairs without a match are normal:
 * *n_tracks = 0, toff[0] = 0, track_of all -1.
 *   The device form reads matches_dev and keep_dev and writes toff_dev, obs_dev, track_of_dev and label_dev in device memory;
 * it is queued on the context's stream and synchronised on return, and only n_tracks and counts cross to the host.  The host
 * form uploads, runs the same kernels and downloads.  Like the matcher, the calls use the context for its device, stream and
 * scratch only.  After either, dlco_desc_last_kernel_ms is the time of the call's kernels (the union-find, the labels, the
 * sort of the nodes by label, the flags, the scan and the scatter; 0 when the batch has no node).
 *   DLCO_ERR_INVALID, before the handle is used and with no output touched: a null handle or required pointer (seg, pairs,
 * moff, matches, n_tracks, toff, obs, track_of, counts), whatever dlco_desc_match_pairs rejects of seg / pairs (but a table of
 * no rows, seg all zero, is a batch here), moff[0] != 0 or a decreasing moff, M or N >= 2^31, min_len < 2, unique not 0 or 1.
 *   Out of scope: seg / pairs / moff in device memory; splitting a conflicting component instead of dropping it; a min_len per
 * pair; triangulation. ---- */
int  dlco_desc_build_tracks(dlco_desc_ctx *ctx, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs,
                            const int64_t *moff, const int32_t *matches_host, const uint8_t *keep_host, int32_t min_len, int32_t unique,
                            int64_t *n_tracks, int64_t *toff_host, int32_t *obs_host, int32_t *track_of_host, int32_t *label_host,
                            int64_t counts[3]);
int  dlco_desc_build_tracks_device(dlco_desc_ctx *ctx, const int64_t *seg, int32_t n_img, const int32_t *pairs, int64_t n_pairs,
                                   const int64_t *moff, const int32_t *matches_dev, const uint8_t *keep_dev, int32_t min_len,
                                   int32_t unique, int64_t *n_tracks, int64_t *toff_dev, int32_t *obs_dev, int32_t *track_of_dev,
                                   int32_t *label_dev, int64_t counts[3]);

#ifdef __cplusplus
}
#endif
#endif
