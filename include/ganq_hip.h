/*
 * ganq_hip.h -- C-ABI of libganq_hip.so: the MI355X (gfx950) implementation of GANQ's per-layer
 * alternating optimisation and of the LUT-dequant linear forward.
 *
 * This is the drop-in boundary for ONE path of smpanaro/ganq (a GPTQModel fork): what
 * `GANQ._perform_quantization_loop` (gptqmodel/quantization/ganq.py:456-646), the Hessian
 * accumulation it inherits (gptqmodel/quantization/gptq.py:88-131) and
 * `FakeQuantLinear.forward` (gptqmodel/nn_modules/qlinear/fake.py:88-89) compute.  The
 * reference has no FFI for this path (its only native code is Metal source embedded in
 * ganq.py:39-328); each entry point below names the reference lines it replaces, and
 * INTEGRATION.md shows the ctypes binding a maintainer would add to ganq.py.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch tensor.data_ptr()) unless marked host;
 *     buffers are borrowed for the duration of the call only, outputs are caller-allocated;
 *   - matrices are row-major and contiguous unless a leading dimension is given;
 *   - m = out_features (rows of W), n = in_features (columns), V = 2^bits codebook entries;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     calls are asynchronous on that stream and re-entrant per stream;
 *   - return value 0 = ok; <0 = error, text via ganq_hip_last_error() (thread-local).
 *   - Q is one uint8 per index ([m,n]); bits in {2,3,4} (V <= 16) are implemented.
 */
#ifndef GANQ_HIP_H
#define GANQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GANQ_HIP_ABI_VERSION 4

/* flags for ganq_run_layer */
#define GANQ_FLAG_ALIAS_Q 1u /* reference torch-branch behaviour: indices of the LAST iteration are returned with \
                                the codebook of the BEST one (ganq.py:487,550,625-626) */
#define GANQ_FLAG_NO_HELPERS 2u /* the S-solve launches no helper workgroups: for callers that run several layers side by \
                                   side on one device (streams), where a helper may not be resident with its tile */

int ganq_hip_version(void);
const char* ganq_hip_last_error(void);

/* Device self-test: determines the accumulation order of v_mfma_f32_16x16x4_f32 on this GPU and
 * checks it against an fmaf chain (the S-solve's bit-exactness contract depends on it).
 * Returns 0 and caches the result; the compute entry points call it lazily. */
int ganq_hip_selftest(void* stream);

/* Developer check (tests): counts operand pairs for which the S-solve's reciprocal-based quotient differs from the IEEE
 * division; mismatches_dev: one uint64 on the device, first_bad_dev: two floats (a, b) of one offending pair. */
int ganq_debug_div_check(uint64_t count, uint32_t seed, unsigned long long* mismatches_dev, float* first_bad_dev,
                         void* stream);

/* Developer check (tests): WH_out [m,n] fp64 = the W @ H_fixed product the fused driver feeds to the T-update (fp16 matrix
 * cores, operands split into two fp16 pieces; option GANQ_WH_F64=1: the fp64 GEMM), Hfixed_out [n,n] fp64 (may be NULL) = the
 * 31-bit fixed-point H it is formed with.  Allocates its own scratch and synchronises the stream. */
int ganq_debug_wh_product(const float* W, const float* H, int64_t m, int64_t n, double* WH_out, double* Hfixed_out, void* stream);

/* Developer check (tests): the T-update of the fused loop on a GIVEN index sequence Qseq [K,m,n], with the integers behind it.
 * Runs what ganq_run_layer runs per iteration (fixed-point conversion once, then K T-updates that keep the bucket sums between
 * iterations, loss rows, changed rows re-solved in place from the second iteration on) under the current developer options; same
 * limits (V in 2..16, n <= 16384).  Allocates its own scratch and synchronises the stream.  Outputs (device, each may be NULL):
 *   after the conversion  scale (fp64), ext (int: the extension word is in use), Hint [n,n] / J [n,n] int32 with
 *                         H ~= scale * (Hint + J / 65536) (J all zero without the extension), hdiag_int [n], hdiag_j [n];
 *   after iteration k     F_hi / F_lo [K,m,16,16] int64: the bucket sums F[a][b] = sum_{u != v} [Q_u = a][Q_v = b] Hint[u][v] (resp. J)
 *                         the per-row solve reads, without the diagonal term (F_lo all zero without the extension);
 *                         chgcnt [K,m]: indices of the row that differ from iteration k - 1 (zeros for k = 0 and with GANQ_T_FULL=1);
 *                         Qprev [K,m,n]: the indices the kept sums belong to (not written with GANQ_T_FULL=1);
 *                         T_all [K,m,V], loss_rows_all [K,m] fp64;
 *                         active_rows [K,m] / active_count [K]: the ascending list of changed rows the solve ran on and its length
 *                         (all -1 where no list was built: k = 0, GANQ_T_FULL=1, GANQ_SOLVE_ALL_ROWS=1);
 *                         full_ran [K]: 1 if the full accumulation produced the sums of iteration k, 0 if they were moved
 *                         incrementally (read off a probe value the host puts into the partial sums, which only the full pass
 *                         overwrites; no kernel is changed for it). */
int ganq_debug_t_sums(const float* W, const float* H, const uint8_t* Qseq, int64_t m, int64_t n, int V, int K, double rcond,
                      double* scale_out, int* ext_out, int* Hint_out, int* J_out, int* hdiag_int_out, int* hdiag_j_out,
                      long long* F_hi, long long* F_lo, int* chgcnt_out, uint8_t* Qprev_out, float* T_all, double* loss_rows_all,
                      int* active_rows, int* active_count, int* full_ran, void* stream);

/* Developer / tests: the dense fp16 / bf16 GEMM the LUT forward uses from ~1024 rows of x on (csrc/gemm_h16.hip), on its own:
 * y [M,N] = x [M,K] @ w [N,K]^T (+ bias [N]) (+ addend [M,N] fp32), dtype 0 = fp16, 1 = bf16; K a multiple of 64, N of 4. */
int ganq_debug_gemm_h16(const void* x, const void* w, const void* bias, const float* addend, int dtype, int64_t M, int64_t N,
                        int64_t K, void* y, void* stream);

/* ---- a1: Hessian accumulation (gptq.py:96-131 process_batch) --------------------------------
 * One calibration batch: X [rows, n] fp16 or bf16 (dtype: 0 = fp16, 1 = bf16), `batch` = number
 * of sequences in it (gptq.py:104), nsamples_before = sequences accumulated so far.
 *     H <- H * N/(N+batch) + (2/(N+batch)) * X^T X          H [n,n] fp32, updated in place
 * workspace: ganq_hessian_workspace_bytes() of caller-owned device scratch (partial tiles of the token-split launches
 * of staged groups; borrowed for the call, nothing is retained).  NULL / too small is allowed: the call then uses the
 * whole-tile kernel only (same H up to fp32 summation order).                                                   */
size_t ganq_hessian_workspace_bytes(int64_t rows, int64_t n);
int ganq_hessian_accum(float* H, const void* X, int dtype, int64_t rows, int64_t n, int64_t nsamples_before,
                       int64_t batch, void* workspace, size_t workspace_bytes, void* stream);

/* ---- a1, staged groups from TRANSPOSED activations (round 4).  The reference multiplies every batch as it arrives
 * (gptq.py:122-131: inp.t() in [in_features, tokens] layout, `self.H += inp.matmul(inp.t())`).  H telescopes over a
 * group of batches, so the host stages them and hands the group over once -- and because the matrix cores want the
 * TOKENS of a feature contiguous (the layout of the reference's `inp` after its `.t()`), the staging copy transposes:
 *     ganq_hessian_stage_t:  Xt[:, tok0 : tok0 + rows] = X^T          X [rows, n] one batch, Xt [n, ldt] fp16 / bf16
 *     ganq_hessian_accum_t:  H <- H * N/(N+batch) + (2/(N+batch)) * Xt[:, :rows] Xt[:, :rows]^T
 * rows of accum_t: a multiple of 32 (the host zero-fills the columns of a ragged last slice); tok0, rows of stage_t and
 * n: multiples of 8.  ganq_hessian_t_supported(n, ldt) says whether a layer is served (in_features >= 3072, a multiple
 * of 8, n * ldt * 2 B < 4 GiB); otherwise the host stages row-major and calls ganq_hessian_accum.  workspace:
 * ganq_hessian_t_workspace_bytes(n) of caller-owned scratch (three partial tiles per workgroup of the launch: one per
 * compute unit, or option GANQ_HESS_W4_WGS; sized at the call's option value).
 * Same products as ganq_hessian_accum, another grouping of the fp32 sums; exactly symmetric; deterministic.       */
int ganq_hessian_t_supported(int64_t n, int64_t ldt);
size_t ganq_hessian_t_workspace_bytes(int64_t n);
int ganq_hessian_stage_t(void* Xt, int64_t ldt, const void* X, int64_t rows, int64_t n, int64_t tok0, void* stream);
int ganq_hessian_accum_t(float* H, const void* Xt, int64_t ldt, int dtype, int64_t rows, int64_t n, int64_t nsamples_before,
                         int64_t batch, void* workspace, size_t workspace_bytes, void* stream);
/* tests (host only, no GPU): how ganq_hessian_accum_t cuts its (tile, token slice) pairs over `ncu` workgroups, computed by
 * the code the kernels run.  hdr[7] = {Ks, G, W, R, nprim, P, Sh}; segs [ncu][W + 3][5] = {tile, s0, s1, parts, slot}
 * (tile -1: unused); parts_loc [R][max_parts][2] = {workgroup, slot} of the parts the fix kernel sums for a left-over tile, in
 * summation order (-1 padded; all -1 for a tile of one part, which the main kernel finishes and the fix kernel leaves alone). */
int ganq_debug_hessian_t_cut(int64_t n, int64_t rows, int ncu, int* hdr, int* segs, int segs_cap, int* parts_loc, int max_parts);
/* tests (host only): the properties of that cut -> 0, or a negative code for the first violated one: -11 a (tile, slice) pair not
 * covered exactly once, -12 slices dropped by the three-segment cap, -13 a part of a multi-part tile without a distinct partial slot
 * or not where the fix kernel reads it, -14 the tiles the fix kernel finishes are not exactly the left-over tiles of >= 2 parts. */
int ganq_debug_hessian_t_check(int64_t n, int64_t rows, int ncu);

/* ---- a2: prologue (gptq.py:280-309) -- lower Cholesky factor A = L L^T in fp32, in place (row-major, leading
 * dimension lda; the strictly upper triangle is zeroed like torch.linalg.cholesky does).  *info (device int32) is 0
 * on success or the 1-based column of the first non-positive pivot (the factor then holds NaN); nothing is
 * synchronised.  workspace: ganq_cholesky_workspace_bytes().                                                   */
size_t ganq_cholesky_workspace_bytes(int64_t n);
int ganq_cholesky(float* A, int64_t n, int64_t lda, int32_t* info, void* workspace, size_t workspace_bytes, void* stream);

/* ---- a3: codebook initialisation (ganq.py:423-438, kmeans_fit :27-30) -----------------------
 * Optimal weighted 1-D k-means per row; col_weight [n] fp64 (caller passes diag(Hinv)^-4).
 * T0 [m,V] fp32 ascending per row.  workspace: ganq_kmeans_workspace_bytes().               */
size_t ganq_kmeans_workspace_bytes(int64_t m, int64_t n, int V);
int ganq_kmeans_init(const float* W, const double* col_weight, int64_t m, int64_t n, int V, float* T0,
                     void* workspace, size_t workspace_bytes, void* stream);
/* what ganq_kmeans_init launches for this shape under the current developer options (host only, no GPU needed; the plan function
 * the launch itself uses).  out[8] = { 1 LDS-resident kernel / 0 windowed kernel, workgroups per CU (1 or 2), P (power of two >= n),
 * queue capacity of the balanced levels (resident), window in candidates (windowed; 0 resident), grid, dynamic LDS bytes,
 * node spacing from which the windowed kernel may solve its levels span by span (0: never, and for the resident kernel) }.
 * Same argument checks as ganq_kmeans_init: n > 16384 is the same error. */
int ganq_debug_kmeans_plan(int64_t m, int64_t n, int V, int* out);

/* ---- a4/a5: S-solve (ganq.py:533-565 torch branch == Metal kernel compute_s :39-270) --------
 * W [m,n], L [n,n] lower-triangular with leading dimension ldl, T [m,V].
 * Q_out [m,n] uint8.  Err_out [m,n] fp32 (W - T[Q]; the Metal kernel's `Werr`) or NULL.
 * workspace: ganq_solve_s_workspace_bytes() -- the per-tile Err scratch and the packed copy of L, plus the
 * hand-over buffers of the helper workgroups that launches with fewer 16-row tiles than the chip has
 * CUs use (csrc/solve_s.hip, "duo" / "shared"); contents need no initialisation.                */
size_t ganq_solve_s_workspace_bytes(int64_t m, int64_t n, int V);
int ganq_solve_s(const float* W, const float* L, int64_t ldl, const float* T, int64_t m, int64_t n, int V,
                 uint8_t* Q_out, float* Err_out, void* workspace, size_t workspace_bytes, void* stream);
/* which helper workgroups a launch of ganq_solve_s with `active_tiles` 16-row tiles still to solve gets under the current
 * developer options, from the plan function the kernel itself evaluates (host only; the device is asked for its CU count only
 * when ncu == 0, and GANQ_SOLVE_CUS caps either).  grid: workgroups of the launch, <= 0 = what the host launches for a layer
 * of active_tiles tiles.  Chains are assumed long enough for helpers (more than GANQ_SOLVE_DUO_CMIN + 1 panels of 64 columns).
 * out[4] = { regime, k: tiles per first helper (1 for DUO / TRIO, 0 for NONE), helper workgroups, grid }. */
#define GANQ_SOLVE_PLAN_NONE 0   /* no helpers: no tickets are drawn */
#define GANQ_SOLVE_PLAN_SHARED 1 /* one helper for every k = 2 .. 4 tiles of a ticket class */
#define GANQ_SOLVE_PLAN_DUO 2    /* a helper per tile (at most half as many tiles as CUs) */
#define GANQ_SOLVE_PLAN_TRIO 3   /* two helpers per tile (at most a third) */
int ganq_debug_solve_plan(int active_tiles, int grid, int ncu, int* out);
/* ... and what ticket `ticket` of class cls (blockIdx mod 8) makes a workgroup of that launch:
 * out[3] = { tile (a helper: the first tile it serves; -1: no role, the workgroup leaves), 0 tile / 1 first / 2 second helper,
 *            tiles a helper serves: tile, tile + 8, .. }. */
int ganq_debug_solve_role(int active_tiles, int grid, int ncu, int cls, int ticket, int* out);

/* which kernel sums the buckets of an [m, n] layer in full under the current developer options (host only, no device is asked):
 * out[2] = { 0 onehot_accum_kernel / 1 onehot_accum_w4_kernel (four waves, LDS-DMA ring), 1 if the four-wave kernel supports the
 * shape at all: in_features a multiple of 256 up to 32768, m n < 2^31 }.  GANQ_ACCUM_W4: -1 by shape, 0 never, 1 wherever supported. */
int ganq_debug_accum_plan(int64_t m, int64_t n, int* out);
/* The four-wave kernel sums only the D lowest digit planes of the fixed-point H that are not sparse; the entries (u > v) with a
 * non-zero digit 3 (c3 of them) or a non-zero digit 2 or 3 (c2) come from exception lists that the preparation fills:
 * D = 2 if c2 <= cap, else 3 if c3 <= cap, else 4.  GANQ_T_TOP: -1 as described, 0 always D = 4.  GANQ_T_TOP_CAP: the cap (-1: the
 * built-in default; clamped to the lists' capacity).  The rule alone, host only: out[3] = { D, cap in force (< 0: no list is wanted:
 * GANQ_T_TOP=0 or the layer takes the first kernel), capacity of a list }. */
int ganq_debug_top_rule(int64_t m, int64_t n, long long c3, long long c2, int* out);
/* ... and on the device: the quantisation of the preparation for H [n,n] (device) of an [m, n] layer.
 * out[5] (host) = { c3, c2, cap in force, capacity of a list, D }. */
int ganq_debug_top_planes(const float* H, int64_t n, int64_t m, long long* out, void* stream);
/* The incremental bucket sums on the matrix cores (m_update_mfma_kernel) read the same D digit planes and take the entries above them
 * from a per-column index of the list in force.  GANQ_MU_TOP: -1 as described, 0 always all four planes, 3 (A/B) as described
 * but never fewer than three planes (with D = 2 in the full sum the entries above digit 2 come from the other list).  The rule alone, host only,
 * from the function the kernel evaluates: out[2] = { D of the incremental kernel, D of the full sum }. */
int ganq_debug_mu_planes(int64_t m, int64_t n, long long c3, long long c2, int* out);

/* ---- dense fp32 product C[m,n] = A[m,k] @ B[k,n] on the fp32 matrix cores (W@H, ganq.py:590) */
int ganq_matmul_f32(const float* A, const float* B, int64_t m, int64_t k, int64_t n, float* C, void* stream);

/* ---- a6: T-update (ganq.py:570-591, CPU/gelsd branch) ---------------------------------------
 * WH = W @ H [m,n], H = Xxt_damped [n,n], Q [m,n].  T_out [m,V] = min-norm lstsq(S H S^T, S (WH)^T)
 * with cut-off rcond (<0: eps_fp32 * V, the torch default).  A_out [m,V,V] / b_out [m,V]: the
 * normal-equation matrices (optional, may be NULL).                                            */
size_t ganq_update_t_workspace_bytes(int64_t m, int64_t n, int V);
int ganq_update_t(const float* WH, const float* H, const uint8_t* Q, int64_t m, int64_t n, int V, double rcond,
                  float* T_out, float* A_out, float* b_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- a7: loss (ganq.py:392-395 quad_loss_2 on Wq = T.gather(1,Q), :621-622) -----------------
 * loss_out: one fp64 on the device.  workspace: ganq_quad_loss_workspace_bytes().             */
size_t ganq_quad_loss_workspace_bytes(int64_t m, int64_t n, int V);
int ganq_quad_loss(const float* W, const float* H, const float* T, const uint8_t* Q, int64_t m, int64_t n, int V,
                   double* loss_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- a7: outputs (ganq.py:633-638): Wq = T.gather(1,Q); Losses = (W-Wq)^2 / diag(Hinv)^2 / 2 -
 * Wq_out / Losses_out [m,n] fp32, either may be NULL.                                          */
int ganq_dequant_losses(const float* W, const float* T, const uint8_t* Q, const float* hinv_diag, int64_t m,
                        int64_t n, int V, float* Wq_out, float* Losses_out, void* stream);

/* ---- the whole loop (ganq.py:516-634): K x (S-solve, T-update, loss) + best-of-K ------------
 * Inputs as above plus T0 [m,V].  Outputs: T_best [m,V], Q_out [m,n], dists [K] fp64 (device),
 * best_k (device int32).  No host synchronisation inside.                                      */
size_t ganq_run_layer_workspace_bytes(int64_t m, int64_t n, int V);
int ganq_run_layer(const float* W, const float* H, const float* L, int64_t ldl, const float* T0, int64_t m,
                   int64_t n, int V, int K, uint32_t flags, double rcond, float* T_best, uint8_t* Q_out,
                   double* dists, int32_t* best_k, void* workspace, size_t workspace_bytes, void* stream);

/* ---- e: the same fused loop on a SLICE of a layer's rows, for a layer whose rows are sharded over several GPUs
 * (rows are independent in every stage of ganq.py:525-634; only the best-of-K decision :621-626 sums over all rows).
 * Same arguments as ganq_run_layer for the slice's m rows, plus optional per-iteration records (device, may be NULL):
 *   T_all [K,m,V] fp32 codebook after each iteration, loss_rows_all [K,m] fp64 per-row loss of each iteration,
 *   Q_all [K,m,n] uint8 indices of each iteration (only needed without GANQ_FLAG_ALIAS_Q).
 * T_best / Q_out / dists / best_k describe the slice alone.  The owner of the layer gathers loss_rows_all of every
 * slice in row order and calls ganq_select_best, which forms the distances in the single-call loop's own summation
 * order: a sharded layer takes bit-for-bit the decision of the unsharded one.  No collective is needed inside the loop. */
int ganq_run_layer_rows(const float* W, const float* H, const float* L, int64_t ldl, const float* T0, int64_t m,
                        int64_t n, int V, int K, uint32_t flags, double rcond, float* T_best, uint8_t* Q_out,
                        double* dists, int32_t* best_k, float* T_all, double* loss_rows_all, uint8_t* Q_all,
                        void* workspace, size_t workspace_bytes, void* stream);
/* loss_rows_all [K,m] (all rows of the layer, row order) -> dists [K] fp64, best_k int32 (device): first k with the
 * smallest distance, strict <, NaN never wins (ganq.py:625); -1 if no iteration wins. */
int ganq_select_best(const double* loss_rows_all, int64_t m, int K, double* dists, int32_t* best_k, void* stream);

/* ---- a2: prologue of GPTQ.quantize() (gptq.py:259-319) in three passes -- dead columns, act_sort permutation, ganq-style
 * offset, damping and the inputs of the two factorisations; the n-vector steps between them (dead = diag == 0, argsort, offset,
 * damp) stay with the host.
 *   ganq_prologue_rowstats: diag[i] = H[i][i], rowabs[i] = sum_j |H[i][j]|                         (gptq.py:267-269, :289-291)
 *   ganq_prologue_gather:   out_k[i][j] = H'[perm i][perm j] + (i == j ? add_k[i] : 0), index-reversed when flip_k; H' = H with
 *                           diag_fixed on its diagonal (dead columns read 1, gptq.py:268); perm NULL = identity; any out_k / add_k
 *                           may be NULL; outputs must not alias H                                   (gptq.py:281-308)
 *   ganq_prologue_weights:  W_out[r][c] = dead[perm c] ? fill_r : W[r][perm c]; fill_r = 0 (mean_fill 0, dead="zero") or the
 *                           row's mean over the live columns (dead="mean")                         (gptq.py:270-276, :283)      */
int ganq_prologue_rowstats(const float* H, int64_t n, float* diag, float* rowabs, void* stream);
int ganq_prologue_gather(const float* H, const int64_t* perm, const float* diag_fixed, int64_t n, float* out0, const float* add0,
                         int flip0, float* out1, const float* add1, int flip1, float* out2, const float* add2, int flip2,
                         void* stream);
int ganq_prologue_weights(const float* W, const int64_t* perm, const uint8_t* dead, int64_t m, int64_t n, int mean_fill,
                          float* W_out, void* stream);

/* ---- a9: LUT-dequant linear forward (replaces FakeQuantLinear.forward, fake.py:88-89) -------
 * y[M,m] = x[M,n] @ dequant(qweight, lut)^T + bias.   dtype: 0 = fp16, 1 = bf16 (x, lut, bias, y).
 * qweight: indices packed `bits` per index along the in_features dimension in the GPTQ int32
 * layout qweight[n*bits/32, m] (qlinear/__init__.py:508-517); lut [m,V]; bias [m] or NULL.     */
/* Any M, x 16-byte aligned.  M <= 64 (decode / small batches): one kernel, split-K partial tiles plus one ticket
 * counter per block of 128 features live in the workspace; the last workgroup of a block reduces and writes y.
 * M > 64 (prefill, perplexity evaluation): the fused LUT-dequant GEMM (csrc/lut_gemm.hip) -- weights decoded into the
 * matrix-core operand tile, never materialised; for few row blocks in_features is split over workgroups, the fp32
 * partial tiles live in the workspace and a second launch sums them in split order (deterministic).
 * The workspace must be zero-filled ONCE after allocation (ganq_lut_linear_workspace_init); every call leaves the
 * counters zero again, so it can be reused by later calls of any shape that fits.  One workspace serves one stream
 * at a time.
 * Contract of every sizer below (ganq_lut_linear*_workspace_bytes), enforced by the guarded-buffer tests
 * (tests/lut_arena.py): a forward call given exactly the returned bytes writes nothing beyond them, nothing outside y's
 * M * m elements, and leaves the first 64 KB of the workspace (the ticket counters) zero.                        */
size_t ganq_lut_linear_workspace_bytes(int64_t M, int64_t m, int64_t n, int bits);
int ganq_lut_linear_workspace_init(void* workspace, size_t workspace_bytes, void* stream);
int ganq_lut_linear_fwd(const void* x, const int32_t* qweight, const void* lut, const void* bias, int dtype,
                        int64_t M, int64_t m, int64_t n, int bits, void* y, void* workspace, size_t workspace_bytes,
                        void* stream);
/* same with an fp32 addend [M,m] (or NULL) added before the single rounding to the activation dtype: the sparse-outlier
 * product of ganq_outlier_matmul */
int ganq_lut_linear_fwd_add(const void* x, const int32_t* qweight, const void* lut, const void* bias, const float* addend,
                            int dtype, int64_t M, int64_t m, int64_t n, int bits, void* y, void* workspace,
                            size_t workspace_bytes, void* stream);
/* both in one call for a layer with outliers (ganq_outlier_matmul into the tail of the workspace, then the LUT kernel);
 * the workspace is initialised like the plain one (ganq_lut_linear_workspace_init over all of it).  The sizer's contract is
 * the plain one's: nothing is written beyond the returned bytes, the first 64 KB are left zero. */
size_t ganq_lut_linear_outliers_workspace_bytes(int64_t M, int64_t m, int64_t n, int bits);
int ganq_lut_linear_fwd_outliers(const void* x, const int32_t* qweight, const void* lut, const void* bias,
                                 const int32_t* rowptr, const int32_t* cols, const void* vals, int dtype, int64_t M, int64_t m,
                                 int64_t n, int bits, void* y, void* workspace, size_t workspace_bytes, void* stream);
/* LUT forward of a layer with a low-rank adapter (LoRA / EoRA): lora_A [r, n], lora_B [m, r] in the activation dtype, both
 * contiguous along the dimension the kernels reduce over, 16-byte aligned; r a multiple of 16 in [16, 256].
 *   y = round(x Wq^T + t lora_B^T (+ addend) (+ bias)),   t = round(x lora_A^T) [M, r] in the activation dtype:
 * fp32 accumulation, ONE rounding of y; t is rounded once (it is the matrix-core operand of the second product).  t is formed in
 * the workspace by a thin-product kernel of its own; the LUT kernel of the regime
 * then runs r / 32 further matrix-core steps on (t, lora_B) -- no library GEMM, bitwise repeatable.  With an adapter every
 * M > 64 goes through the fused LUT-dequant GEMM.  addend: fp32 [M, m] or NULL.  The workspace
 * is 256-byte aligned and initialised like the plain one (ganq_lut_linear_workspace_init over all of it); the sizer's contract
 * is the plain one's (nothing written beyond the returned bytes, the first 64 KB -- the adapter's tickets are its last 1024 ints --
 * left zero). */
size_t ganq_lut_linear_lora_workspace_bytes(int64_t M, int64_t m, int64_t n, int bits, int r);
int ganq_lut_linear_fwd_lora(const void* x, const int32_t* qweight, const void* lut, const void* bias, const void* lora_A,
                             const void* lora_B, int r, const float* addend, int dtype, int64_t M, int64_t m, int64_t n,
                             int bits, void* y, void* workspace, size_t workspace_bytes, void* stream);
/* the same for a layer with sparse outliers (arguments as ganq_lut_linear_fwd_outliers): at decode sizes ONE LUT launch adds the
 * CSR entries and the adapter steps; otherwise ganq_outlier_matmul into the tail of the workspace is the addend.  Same sizer
 * contract: nothing written beyond the returned bytes, the first 64 KB left zero. */
size_t ganq_lut_linear_lora_outliers_workspace_bytes(int64_t M, int64_t m, int64_t n, int bits, int r);
int ganq_lut_linear_fwd_lora_outliers(const void* x, const int32_t* qweight, const void* lut, const void* bias, const void* lora_A,
                                      const void* lora_B, int r, const int32_t* rowptr, const int32_t* cols, const void* vals,
                                      int dtype, int64_t M, int64_t m, int64_t n, int bits, void* y, void* workspace,
                                      size_t workspace_bytes, void* stream);
/* tests / developers (host only; no GPU is touched when ncu > 0): which kernels the forward entry points above launch for x [M,n]
 * and a layer [m,n] of `bits` with an adapter of rank r (0: none) and with / without sparse outliers, under the current developer
 * options, computed by the plan functions the forward itself calls.  ncu: compute units to plan for, 0 = the current device's.
 * out[8] = { regime (GANQ_LUT_REGIME_*),
 *            row tiles: 16-row tiles per workgroup (1, 2, 4) for M <= 64, tiles of 256 / 128 rows of the launch above,
 *            KS: splits of in_features across workgroups (1: none),
 *            outliers: -1 none, 1 added inside the decode launch, 0 their fp32 product is the addend,
 *            adapter: -1 none, 1 further matrix-core steps of the LUT kernel, 0 its fp32 product is the addend of the dense path,
 *            KS of the adapter's t kernel (0 without an adapter),
 *            workgroups of the main launch,
 *            the CU count planned for }.
 * The four-wave developer kernel of GANQ_GEMM_H16_BM=512 reports as DENSE256. */
#define GANQ_LUT_REGIME_DECODE16 0    /* M <= 32: 16 waves split in_features inside the workgroup, 16 features per workgroup */
#define GANQ_LUT_REGIME_DECODE32 1    /* ... 32 features per workgroup (M <= 16, even m) */
#define GANQ_LUT_REGIME_MFMA_SMALL 2  /* M <= 64: matrix-core kernel, split-K through memory */
#define GANQ_LUT_REGIME_GEMM 3        /* M > 64: fused LUT-dequant GEMM, whole K */
#define GANQ_LUT_REGIME_GEMM_SPLITK 4 /* ... in_features split over workgroups + reduce launch */
#define GANQ_LUT_REGIME_GEMM_PIPE 5   /* ... one-workgroup-per-CU pipelined kernel */
#define GANQ_LUT_REGIME_DENSE128 6    /* dequantise once + dense GEMM, 128-row tiles */
#define GANQ_LUT_REGIME_DENSE256 7    /* ... 256-row tiles */
int ganq_debug_lut_plan(int64_t M, int64_t m, int64_t n, int bits, int r, int outliers, int ncu, int* out, int out_len);
/* prefill path: materialise Wq [m,n] = lut[o][index] in the activation dtype for a library GEMM */
int ganq_lut_dequant(const int32_t* qweight, const void* lut, int dtype, int64_t m, int64_t n, int bits, void* Wq_out,
                     void* stream);

/* embedding lookup out of the packed stream of a LUT layer (a model whose input embedding shares the quantized head's table):
 *   out [N, n] (dtype 0 = fp16, 1 = bf16; 16-byte aligned) row t = lut[id][Q[id][:]] (+ the CSR entries of row id, ONE rounded add in
 *   dtype per element, as Wq + W_sparse), id = ids[t]; an id outside [0, m) gives a row of zeros and reads nothing.
 * qweight / lut / the CSR by output feature (vals in dtype) as ganq_lut_linear_fwd_outliers takes them; the three outlier pointers
 * may be NULL (no outliers: no add).  No workspace, no host synchronisation, no allocation: one launch, capturable in a HIP graph. */
int ganq_lut_embedding(const int64_t* ids, int64_t N, const int32_t* qweight, const void* lut, int dtype, int64_t m, int64_t n,
                       int bits, const int32_t* outlier_rowptr, const int32_t* outlier_cols, const void* outlier_vals, void* out,
                       void* stream);

/* a LUT-quantized table whose ROWS are looked up (an input embedding quantized on its own), in a row-packed layout:
 *   qrows [m, n * bits / 32] int32, row-major; row `id` holds the little-endian bit stream column `id` of the GPTQ layout holds
 *   (32 indices in `bits` words), so qrows == transpose(qweight): a token's row is n * bits / 8 contiguous bytes.
 *   n a multiple of 32, bits 2, 3 or 4.  m == 0 (and N == 0) is a no-op.
 * ganq_lut_table_assign: W [m,n] fp32 (16-byte aligned), T [m, 2^bits] fp32 -> qrows, Q[o][j] = the FIRST v that minimises
 *   fabsf(W[o][j] - T[o][v]) (fp32 subtraction, v scanned upwards with a strict <), written straight into the packed words;
 *   sqerr_rows [m] fp64 (or NULL) = sum_j (double)d * d of the fp32 differences d to the chosen codes, summed in a fixed order
 *   (no atomics: bitwise repeatable).
 * ganq_lut_table_lookup: out [N, n] (dtype 0 = fp16, 1 = bf16; 16-byte aligned) row t = lut[id][Q[id][:]], id = ids[t]; an id outside
 *   [0, m) gives a row of zeros and reads nothing.  lut [m, 2^bits] in dtype.  No workspace, no host synchronisation, no allocation:
 *   one launch, capturable in a HIP graph. */
int ganq_lut_table_assign(const float* W, const float* T, int64_t m, int64_t n, int bits, int32_t* qrows, double* sqerr_rows,
                          void* stream);
int ganq_lut_table_lookup(const int64_t* ids, int64_t N, const int32_t* qrows, const void* lut, int dtype, int64_t m, int64_t n,
                          int bits, void* out, void* stream);

/* codebook gradient of the two lookups above (csrc/lut_table_backward.hip), the term autograd takes through
 * F.embedding(ids, lut.gather(1, Q)) with respect to lut:
 *   dlut [m, 2^bits] fp32 (16-byte aligned), dlut[id][v] = sum over the positions p with ids[p] == id and the columns j with
 *   Q[id][j] == v of dy[p][j].  EVERY element of dlut is written: rows no id selects, codes no index of a row uses, an id outside
 *   [0, m) and the id `padding_idx` (-1: none; nn.Embedding masks that row's gradient) contribute exactly 0; N == 0 gives zeros.
 *   ganq_lut_table_bwd_lut takes the row-packed qrows [m, n * bits / 32] of ganq_lut_table_lookup, ganq_lut_embedding_bwd_lut the
 *   GPTQ column layout qweight [n * bits / 32, m] of ganq_lut_embedding (the head's outliers are frozen: no gradient; the codes at
 *   outlier positions count, as in ganq_lut_linear_bwd_lut).
 *   ids int64 [N]; order int64 [N]: a STABLE ascending sort permutation of ids, computed by the caller (it is not trusted: an entry
 *   outside [0, N) is skipped, never dereferenced; what a wrong permutation gives is unspecified but writes only dlut);
 *   dy [N, n] (dtype 0 = fp16, 1 = bf16; 16-byte aligned), n a multiple of 32, bits 2, 3 or 4, N below 2^40 (-1 otherwise).
 *   n == 0 or N == 0 needs no workspace (the query returns 0) and zero-fills dlut; m == 0 is a no-op.
 * Deterministic: no floating-point atomics, the summation order is a function of (ids, dy) alone -- per position the columns in a
 * fixed lane pattern, per id its positions in ascending order.  No host synchronisation, no allocation: a memset and two launches
 * whatever the ids hold, capturable in a HIP graph.  The workspace (16-byte aligned) needs no initialisation; its size depends on
 * the arguments alone (0 for N = 0) and is the same for both layouts. */
size_t ganq_lut_table_bwd_lut_workspace_bytes(int64_t N, int64_t m, int64_t n, int bits);
int ganq_lut_table_bwd_lut(const int64_t* ids, const int64_t* order, int64_t N, const void* dy, int dtype, const int32_t* qrows,
                           int64_t m, int64_t n, int bits, int64_t padding_idx, float* dlut, void* workspace, size_t workspace_bytes,
                           void* stream);
size_t ganq_lut_embedding_bwd_lut_workspace_bytes(int64_t N, int64_t m, int64_t n, int bits);
int ganq_lut_embedding_bwd_lut(const int64_t* ids, const int64_t* order, int64_t N, const void* dy, int dtype, const int32_t* qweight,
                               int64_t m, int64_t n, int bits, int64_t padding_idx, float* dlut, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---- per-token negative log-likelihood straight from a packed head (csrc/lut_head_nll.hip): the logits
 *   logits[M,m] = x[M,n] @ dequant(qweight, lut)^T (+ bias)   (fp32, not rounded)
 * are never written.  Same qweight / lut / bias layout and dtypes as ganq_lut_linear_fwd; bits 2, 3 or 4, n a multiple of 32, any
 * M >= 1 and m >= 1; x 16-byte aligned; targets int64 [M].  Outputs, fp32 [M] each:
 *   lse[row] = log sum_o exp(logits[row][o]),  tgt_logit[row] = logits[row][targets[row]],  nll[row] = lse[row] - tgt_logit[row].
 * A row whose target lies outside [0, m) (-100 or anything else) is ignored: nll = tgt_logit = 0, lse still written.
 * Two launches: 256 x 128 tiles of the fused LUT-dequant GEMM reduce every row to (max, sum of exp) per feature tile, a second
 * kernel merges the tiles in a fixed order.  No atomics, no memset, no host synchronisation: the same bytes on every call,
 * capturable in a HIP graph.  The workspace (8-byte aligned, no initialisation) holds 8 bytes per row and 128-feature tile plus
 * 4 bytes per row: 8 * M * ceil(m / 128) + 4 * M.  Error codes as ganq_lut_linear_fwd (-4: workspace too small, nothing written;
 * -1: x or qweight beyond the 2 GB window of the 32-bit buffer offsets -- split the rows of x over several calls). */
size_t ganq_lut_head_nll_workspace_bytes(int64_t M, int64_t m, int64_t n, int bits);
int ganq_lut_head_nll(const void* x, const int32_t* qweight, const void* lut, const void* bias, const int64_t* targets, int dtype,
                      int64_t M, int64_t m, int64_t n, int bits, float* nll, float* lse, float* tgt_logit, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- next token straight from a packed head (csrc/lut_head_pick.hip): the decode-side counterpart of ganq_lut_head_nll.  For
 * x [M, n], a packed head (qweight, lut, bias) of m features, inv_t > 0 and an optional noise [M, m] (finite fp32, or NULL):
 *   l[r][o] = x[r] . dequant(qweight, lut)[o] (+ bias[o])      fp32, never rounded, never written
 *   s[r][o] = l[r][o] * inv_t
 *   lse[r]  = log sum_o exp(s[r][o])
 *   z[r][o] = s[r][o] + noise[r][o]        (noise absent: z = s)
 *   token[r]   = the SMALLEST o with z[r][o] = max_o z[r][o]
 *   score[r]   = s[r][token[r]]            (without the noise)
 *   logprob[r] = score[r] - lse[r]
 * Only valid features (o < m) take part.  Greedy: noise = NULL, inv_t = 1.  Exact sampling from softmax(l / T): inv_t = 1 / T and
 * noise = -log(E), E ~ Exp(1) iid (Gumbel-max).  The library draws nothing: the call is deterministic and the random numbers are
 * the caller's.  Same qweight / lut / bias layout and dtypes as ganq_lut_linear_fwd; bits 2, 3 or 4, n a multiple of 32, any
 * M >= 1 and m >= 1; x 16-byte aligned.  Outputs [M]: token int64, score / lse / logprob fp32.
 * One tile launch per 64 rows (a workgroup of 4 waves owns 128 features and all of in_features and leaves one record
 * (max, sum of exp, best z, its s, its index) per row), then one merge launch: a wave per row, its lanes over 64 contiguous
 * ranges of the feature blocks in ascending order.  No atomics, no memset, no host synchronisation: the same bytes on every call,
 * capturable in a HIP graph.  The workspace (16-byte
 * aligned, no initialisation) holds 20 bytes per row and 128-feature block: 20 * M * ceil(m / 128), whatever n and bits are.
 * Error codes: -2 bits outside {2, 3, 4}, n not a multiple of 32, unknown dtype, inv_t not finite or <= 0; -1 M < 0, or x or
 * qweight beyond the 2 GB window of the 32-bit offsets (split the rows of x over several calls); -3 null pointer; -4 workspace
 * too small.  A refused call writes nothing.
 * ganq_debug_head_pick_plan (host only): out = { tile launches, feature blocks, workgroups of the merge launch, then the row tiles
 * RT = ceil(rows / 16) of each tile launch, as many as out_len leaves room for }; out_len >= 3. */
size_t ganq_lut_head_pick_workspace_bytes(int64_t M, int64_t m, int64_t n, int bits);
int ganq_lut_head_pick(const void* x, const int32_t* qweight, const void* lut, const void* bias, const float* noise, float inv_t,
                       int dtype, int64_t M, int64_t m, int64_t n, int bits, int64_t* token, float* score, float* lse, float* logprob,
                       void* workspace, size_t workspace_bytes, void* stream);
int ganq_debug_head_pick_plan(int64_t M, int64_t m, int64_t n, int bits, int* out, int out_len);

/* ---- the sampled pick with the noise drawn inside the kernel (csrc/lut_head_pick.hip).  ganq_lut_head_pick_seeded is
 * ganq_lut_head_pick with noise[r][o] = g(r, o) computed in the epilogue of the tile kernel instead of read: nothing of size [M, m]
 * is drawn, written or read, and the call is a pure function of (inputs, seed, offset).
 *   rng_state  device memory, 8-byte aligned: { uint64 seed, uint64 offset }
 *   g(r, o)    Philox4x32-10 with key (seed_lo, seed_hi) and counter (o, r >> 2, offset_lo, offset_hi); of its four words the
 *              word w = out[r & 3] belongs to (r, o); u = (2 (w >> 9) + 1) 2^-24 (exact in fp32, in [2^-24, 1 - 2^-24]),
 *              g = -logf(-logf(u)) in [-2.82, 16.64]: always finite; the mass of a Gumbel variable above 16.64 (6e-8 per draw)
 *              falls on the top value.  r is the row of x within the call, whatever the launches the call is cut into.
 *   advance    one call consumes ONE unit of offset whatever its shape.  Non-zero: one lane of the merge launch, which is
 *              stream-ordered after every tile launch of the call, stores offset + 1 (64-bit), so the next call -- or the next
 *              replay of a captured call -- draws fresh noise without the host.  Zero: the 16 bytes are only read.
 * Same workspace and sizer, same outputs, tie rule and error codes as ganq_lut_head_pick, and -3 for a null, -2 for a misaligned
 * rng_state.  No atomics, no memset, no host synchronisation; M == 0 is a no-op that leaves the state.
 * ganq_lut_head_pick_noise writes noise[M][m] = g(r, o) of the state (fp32) and, if words is not NULL, the raw Philox word of
 * every element (uint32 [M][m]) through the same device functions; it never advances the state.  ganq_lut_head_pick on that
 * noise returns the bytes ganq_lut_head_pick_seeded returns. */
int ganq_lut_head_pick_seeded(const void* x, const int32_t* qweight, const void* lut, const void* bias, uint64_t* rng_state, int advance,
                              float inv_t, int dtype, int64_t M, int64_t m, int64_t n, int bits, int64_t* token, float* score, float* lse,
                              float* logprob, void* workspace, size_t workspace_bytes, void* stream);
int ganq_lut_head_pick_noise(const uint64_t* rng_state, int64_t M, int64_t m, float* noise, uint32_t* words, void* stream);

/* ---- a9 backward -- the gradients autograd takes through FakeQuantLinear.forward (fake.py:88-89).  Same qweight / lut layout,
 * dtypes and shapes as ganq_lut_linear_fwd (any M >= 1, any m >= 1, n a multiple of 32; dtype 0 = fp16, 1 = bf16 for dy, x, lut, dx):
 *   bwd_input: dx [M,n] = dy [M,m] @ dequant(qweight, lut) (+ addend [M,n] fp32, or NULL); fp32 accumulation over all of m,
 *              ONE rounding to dtype.  M <= 64: one kernel decodes the packed indices (splits of m summed by a second launch);
 *              M > 64: Wq^T [n][ceil64(m)] is written to the workspace and multiplied by the forward's dense GEMM.  A layer with
 *              outliers passes dy @ W_sparse (ganq_outlier_matmul on the transposed CSR) as the addend.  dx 8-byte aligned, addend
 *              16-byte aligned; dy 16-byte aligned when m is a multiple of 64 and M > 64.
 *   bwd_lut:   dlut [m,V] fp32 = sum_b sum_j [Q[o][j] == v] * dy[b][o] * x[b][j]   (codes no index uses: exactly 0)
 *              dy^T and x^T are staged in the workspace with tokens contiguous, the dense GEMM forms dy^T x and sums each product
 *              into the bin of its code in its epilogue.
 * Deterministic: bitwise repeatable, no floating-point atomics.  Workspaces need no initialisation, and their sizes depend
 * only on the arguments (0 for M = 0). */
size_t ganq_lut_linear_bwd_input_workspace_bytes(int64_t M, int64_t m, int64_t n, int bits);
int ganq_lut_linear_bwd_input(const void* dy, const int32_t* qweight, const void* lut, const float* addend, int dtype,
                              int64_t M, int64_t m, int64_t n, int bits, void* dx, void* workspace, size_t workspace_bytes,
                              void* stream);
size_t ganq_lut_linear_bwd_lut_workspace_bytes(int64_t M, int64_t m, int64_t n, int bits);
int ganq_lut_linear_bwd_lut(const void* dy, const void* x, const int32_t* qweight, int dtype, int64_t M, int64_t m,
                            int64_t n, int bits, float* dlut, void* workspace, size_t workspace_bytes, void* stream);

/* pack Q [m,n] uint8 (original column order) into qweight [n*bits/32, m] int32, and back */
int ganq_pack_indices(const uint8_t* Q, int64_t m, int64_t n, int bits, int32_t* qweight, void* stream);
int ganq_unpack_indices(const int32_t* qweight, int64_t m, int64_t n, int bits, uint8_t* Q, void* stream);

/* ---- outlier split in front of GANQ (paper section 3.3 + Appendix A Algorithm 2, paper.md:195-197,882-899; SURVEY
 * 8(f) row 4 -- the reference repository does not implement it).  Row by row, with p = 1 - ratio/2, the entries
 * w >= sorted[floor(n p)] or w <= sorted[ceil(n (1-p))] are outliers; they are kept exactly in a CSR matrix and zeroed
 * in W, which GANQ then quantizes; the layer computes LUT(x) + x @ W_sparse^T.
 *   ganq_outlier_cutoffs: cut [m,2] = (c_lower, c_upper), counts [m], rowptr [m+1] (exclusive scan; rowptr[m] = nnz).
 *                         n <= 16384.  The caller reads rowptr[m] to size cols / vals.
 *   ganq_outlier_extract: cols / vals [nnz] in ascending column order per row; W is overwritten by W_dense.
 *   ganq_outlier_matmul:  out [M,m] fp32 = x [M,n] @ W_sparse^T, x and vals in `dtype` (0 = fp16, 1 = bf16).       */
int ganq_outlier_cutoffs(const float* W, int64_t m, int64_t n, double ratio, float* cut, int32_t* counts, int32_t* rowptr,
                         void* stream);
int ganq_outlier_extract(float* W, int64_t m, int64_t n, const float* cut, const int32_t* rowptr, int32_t* cols, float* vals,
                         void* stream);
int ganq_outlier_matmul(const void* x, int dtype, int64_t M, int64_t m, int64_t n, const int32_t* rowptr, const int32_t* cols,
                        const void* vals, float* out, void* stream);

/* ---- developer / test switches.  They are read from the environment (variable == option name) once, when the library
 * is loaded; afterwards only these calls change them -- the compute entry points never call getenv().  Options:
 * GANQ_T_FULL, GANQ_T_INCR_THR, GANQ_T_JACOBI, GANQ_SOLVE_ALL_ROWS, GANQ_MUPDATE_LDS, GANQ_WH_F64, GANQ_KMEANS_WCAP,
 * GANQ_CHOL_LOOKAHEAD, GANQ_ACCUM_DEBUG, GANQ_LUT_INWG, GANQ_LUT_WGS, GANQ_LUT_KS, GANQ_LUT_NT, GANQ_LUT_DENSE_M, GANQ_LUT_GEMM_RM,
 * GANQ_LUT_GEMM_PIPE, GANQ_GEMM_H16_BM, GANQ_H_EXT, GANQ_SOLVE_VARIANT
 * (meanings: ganq_amd/csrc/runtime.hip).  None of them changes a result except where a test says so. */
int ganq_debug_set_option(const char* name, long long value);
int ganq_debug_get_option(const char* name, long long* value);
int ganq_debug_reset_option(const char* name);

/* ---- per-kernel device timing (HIP events recorded on the caller's stream around every kernel launch) ----
 * ganq_profile_enable(1) starts collecting, ganq_profile_get() sums what has completed: the caller must have
 * synchronised the stream.  kernel ids are 0 .. ganq_profile_num_kernels()-1.  Every instrumented launch puts two
 * event packets between dependent kernels (about 1 ms of idle time per 4096x4096 layer with all kernels instrumented):
 * ganq_profile_select(id) restricts the instrumentation to one kernel (-1: all, the default).                    */
int ganq_profile_enable(int on);
int ganq_profile_select(int kernel_id);
int ganq_profile_reset(void);
int ganq_profile_num_kernels(void);
const char* ganq_profile_kernel_name(int kernel_id);
int ganq_profile_get(int kernel_id, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* GANQ_HIP_H */
