/*
 * dpgp.h — C ABI of libdpgp_hip.so: the DP-GP-LVM variational-ELBO inner loop on AMD MI355X (gfx950), hand-written HIP.
 *
 * The reference (AndrewRLawrence/dp_gp_lvm) has no FFI: its boundary for this path is the Python operator API
 *   k_ard_rbf / Kernel.covariance_matrix | covariance_diag | psi_0 | psi_1 | psi_2   (src/kernels/rbf_kernel.py:26-203,
 *                                                                                     src/kernels/interfaces/kernel.py:204-280)
 *   dp_gp_lvm(...).objective                                                          (src/models/dp_gp_lvm.py:100-154)
 * which dispatches to TensorFlow 1.15 ops (tf.matmul / tf.exp / tf.cholesky / tf.matrix_triangular_solve ...).
 * These entry points are what a binding of that API would call instead of TensorFlow; dp_gp_lvm_amd/ binds them with
 * ctypes (dp_gp_lvm_amd/_lib.py), INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (e.g. torch's allocator); row-major, contiguous, leading batch
 *    dimension; the library keeps no global state and allocates nothing: scratch is a caller-provided workspace whose
 *    size comes from the matching *_workspace_bytes() query (a pure host function, callable without a GPU);
 *  - `stream` is a hipStream_t passed as void*; every call only ENQUEUES work on it and returns (graph-capturable);
 *  - return value: DPGP_OK (0), or -(1-based index of the first bad argument), or DPGP_ERR_LAUNCH (-100) if the HIP
 *    launch itself failed.  A non-positive-definite matrix is never an abort: it is reported LAPACK-style in the
 *    caller-provided device array info[B] (0 = ok, j>0 = leading minor j not positive; for the fused ELBO, M + j
 *    refers to the second factorisation);
 *  - suffix _f32 / _f64 is the arithmetic AND storage type of the call;  `s` is always the DIAGONAL [N,Q] of q(X)'s
 *    covariance (the reference API takes [N,Q,Q] and reads only its diagonal: rbf_kernel.py:151,182);
 *  - B = kernel batch (= D output dims in dp_gp_lvm), N observations, M inducing points, Q latent dims (Q <= 30).
 */
#ifndef DPGP_H
#define DPGP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DPGP_OK 0
#define DPGP_ERR_LAUNCH (-100)
#define DPGP_FLAG_NOISE 1  /* include_noise  (only honoured when x1 == NULL: rbf_kernel.py:80)  */
#define DPGP_FLAG_JITTER 2 /* include_jitter (only honoured when x1 == NULL: rbf_kernel.py:86)  */
#define DPGP_MAX_Q 30

/* algorithm selectors for the calls that have a matrix-core and a plain-VALU implementation */
#define DPGP_ALGO_AUTO 0     /* matrix-core kernels (the product path); fp32 psi2 = pair-tile GEMM, f16 hi/lo operands */
#define DPGP_ALGO_PLAIN 1    /* straightforward one-thread-per-element HIP kernels (cross-check)                  */
#define DPGP_ALGO_MFMA_F32 2 /* as AUTO, but fp32 psi2 on v_mfma_f32_16x16x4_f32 (exact fp32 products; slower)    */
#define DPGP_ALGO_PATCH_F16 3 /* as AUTO, but fp32 psi2 by the per-observation 64x64 patch kernel (round-1 form)    */

/* precision modes of the fused ELBO */
#define DPGP_PREC_F32 0   /* psi-statistics fp32, Cholesky chain fp32                          */
#define DPGP_PREC_MIXED 1 /* psi-statistics fp32 (MFMA), Cholesky chain + reductions fp64      */
#define DPGP_PREC_F64 2   /* everything fp64                                                   */
#define DPGP_PREC_MIXED_FAST 4  /* dpgp_elbo_grad_psi[_ex], dpgp_elbo_step only: as DPGP_PREC_MIXED, but the second products of the pair-tile
                                 * stage B take the exponentials as their f16 roundings alone (11 significant bits instead of 22; the pass
                                 * that also yields Psi2 keeps both halves).  The rounding errors are independent from element to element
                                 * and average over the observations / pairs a sum runs over: measured <= 3e-6 of the largest gradient
                                 * entry at N = 2000 (the default's 6e-7), beyond the 5e-4 gradient tolerance only for N of a few dozen
                                 * (tests/test_gpu_grad.py).  Opt-in; never the default. */
#define DPGP_PREC_MIXED_PATCH 3 /* dpgp_elbo_grad_psi[_ex] only: as DPGP_PREC_MIXED, the Psi2 term in the per-observation patch
                                 * form (psi2_grad_kernel) instead of the pair-tile form (psi2_pairs_grad.hip).  The pair-tile form
                                 * is faster (config 3: 6.7 vs 8.0 ms) but sums a' and b weighted exponentials SEPARATELY before
                                 * they cancel in 2 a s + b; where the adjoints themselves cancel heavily (K_uu nearly singular:
                                 * an fp64 forward pass with this stage in mixed precision) the patch form keeps 2e-3 of the
                                 * largest gradient entry, the pair form 7e-3 (tests/test_gpu_illcond.py) */

/* info[] codes besides the LAPACK-style positive ones (fused ELBO only; 0 = fine):
 *   DPGP_INFO_ILL_CONDITIONED: with an fp32 Psi2 (DPGP_PREC_MIXED / DPGP_PREC_F32) the rounding of Psi2, amplified by
 *   K_uu^-1, may move this output dim's terms by more than DPGP_GUARD_REL * N (bound written to the workspace's guard[d],
 *   see dpgp_elbo_workspace_layout): the terms are written but are not covered by the mixed-precision tolerance any more.
 *   Evaluate with DPGP_PREC_F64 (the reference's arithmetic, src/utils/types.py:13-14).
 *   Two paths use a LOOSER form of the bound (they flag earlier, never later): M > 128 with D >= 128 (chain_big.hip) takes
 *   tr K_uu^-1 for |K_uu^-1|_F (at most sqrt(M) larger); the over-T evaluation (dpgp_elbo_fhat_t) evaluates the guard of atom t with
 *   the data-fit factor of a stand-in column (column t of y) instead of the D columns the atom is solved against — there the flag
 *   says "this atom's K_uu / B is ill-conditioned for an fp32 Psi2", not a bound on a particular output dim's terms.
 * Operands outside the f16 range of the default fp32 psi kernels (|z - mean z| or |mu - mean z| beyond ~90 length scales)
 * are detected in the kernels: the affected Psi2 patch / Psi1^T y slab comes out as NaN, which the fused ELBO reports as a
 * failed factorisation (info > 0, NaN terms).  DPGP_ALGO_MFMA_F32 and fp64 have no such limit.
 * y in the pair-tile stage B and the training step (dpgp_elbo_step, dpgp_elbo_grad_psi[_ex] in mixed precision): the f16 features
 * of the Psi1 pass are y_nd times a power of two per output dim that brings max_n |y_nd| into [16, 32), undone exactly where the
 * pass's results are read — so any finite y whose every nonzero column has max_n |y_nd| in [2^-120, 2^120] is accepted with the
 * accuracy of unit-scale data (tests/test_gpu_scales.py sweeps 2^-20 ... 2^20 and columns of their own scale from 1e-4 to 1e5).
 * A non-finite y, or a column beyond 2^120, is refused as a range-guard hit: NaN gradients (and, in dpgp_elbo_step, NaN terms).
 * The observation features a'_q, b_q of the same passes are proportional to w = gamma_dq / (gamma_dq s_nq + 1); they carry a power
 * of two per (d, q) that lifts a gamma below 1/2 into [1/2, 1), so ARD-switched-off latent dims (gamma down to 1e-6 and below) keep
 * their d/dz to the mixed tolerance.  w above ~150 (gamma and 1/s both that large) overflows the features' f16 range: refused
 * in the same way (NaN plus the range flag), never a finite wrong number.
 * A large |y| still makes a mixed forward pass flag the output dim as DPGP_INFO_ILL_CONDITIONED: the conditioning-guard bound grows
 * with y^2 against an absolute threshold.                                                              */
#define DPGP_INFO_ILL_CONDITIONED (-2)
#define DPGP_GUARD_REL 2.0e-3

int dpgp_version(void);
/* text of the HIP error behind the last DPGP_ERR_LAUNCH returned to the calling thread (diagnostics) */
const char *dpgp_last_hip_error(void);

/* ---- Kernel.covariance_matrix (rbf_kernel.py:58-93): out[B,N0,N1] = alpha_b exp(-1/2 sum_q gamma_bq (x0_iq-x1_jq)^2)
 *      x1 == NULL means input_1 is None: N1 is ignored (= N0) and noise/jitter flags apply on the diagonal.          */
int dpgp_ard_rbf_gram_f32(int B, int N0, int N1, int Q, const float *x0, const float *x1, const float *gamma,
                          const float *alpha, const float *beta, int flags, double jitter, float *out, void *stream);
int dpgp_ard_rbf_gram_f64(int B, int N0, int N1, int Q, const double *x0, const double *x1, const double *gamma,
                          const double *alpha, const double *beta, int flags, double jitter, double *out, void *stream);

/* ---- gradient contraction of the ARD-RBF gram (gp_regression / gp_lvm backward pass, gaussian_process.py:22-129):
 *      G_ij = w_ij alpha exp(-1/2 sum_q gamma_q (x_iq - x_jq)^2)  (the noise-free gram; the diagonal counts, with exp = 1)
 *      r[i] = sum_j G_ij,  sx[i][q] = sum_j G_ij (x_iq - x_jq),  sq[i][q] = sum_j G_ij (x_iq - x_jq)^2
 *      x[N][Q], gamma[Q], alpha[1], w[N][ldw] (ldw >= N; any w, symmetry is not assumed), r[N], sx[N][Q], sq[N][Q].
 *      1 <= Q <= DPGP_GRAM_GRAD_MAX_Q (the LDS bound of the row / column strips).  N == 0 does nothing.  Partial sums go to
 *      ws and are added in a fixed order: no atomics, the same bits on every run.  dL/dK = w then gives
 *      dL/dalpha = sum r / alpha, dL/dgamma_q = -1/2 sum_i sq[i][q], dL/dx_iq = -2 gamma_q sx[i][q] (w symmetric). */
#define DPGP_GRAM_GRAD_MAX_Q 64
size_t dpgp_ard_rbf_gram_grad_workspace_bytes(int N, int Q);
int dpgp_ard_rbf_gram_grad_f64(int N, int Q, const double *x, const double *gamma, const double *alpha, const double *w, int ldw,
                               double *r, double *sx, double *sq, void *ws, size_t ws_bytes, void *stream);
/*   dpgp_ard_rbf_gram_grad_batched_f64: the same contraction for B kernels in one launch pair (the K_uu term of a masked
 *      multi-view bound: V kernels with their own inducing inputs).  x[B][N][Q], gamma[B][Q], alpha[B], kernel b's w at
 *      w + b * w_stride with leading dimension ldw (ldw >= N; w_stride >= (N - 1) ldw + N when B > 1), r[B][N], sx[B][N][Q],
 *      sq[B][N][Q]: for every b what dpgp_ard_rbf_gram_grad_f64 returns for b's own inputs (the bits may differ where the slab
 *      plans do: the batched plan divides its workgroup target by B).  B == 0 or N == 0 does nothing and reads no pointer.  The
 *      workspace query returns 0 for a shape out of range.  No atomics, the same bits on every run. */
size_t dpgp_ard_rbf_gram_grad_batched_workspace_bytes(int B, int N, int Q);
int dpgp_ard_rbf_gram_grad_batched_f64(int B, int N, int Q, const double *x, const double *gamma, const double *alpha,
                                       const double *w, int ldw, long long w_stride, double *r, double *sx, double *sq, void *ws,
                                       size_t ws_bytes, void *stream);

/* ---- Psi statistics of a test-point q(X*) for B kernels with their own inducing inputs, and their adjoint (the prediction
 *      paths of bayesian_gp_lvm / manifold_relevance_determination: gaussian_process.py:329-538 and :729-990 evaluate
 *      kernel.psi_1 / psi_2 of rbf_kernel.py:135-199 at q(X*) per view and differentiate the bound through them).
 *      z[B][M][Q] (kernel b's inducing inputs), mu[N][Q], s[N][Q] (q(X*) shared by the B kernels), gamma[B][Q], alpha[B].
 *      zfac: NULL, or [B][M][M] = alpha_b^2 exp(-1/4 sum_q gamma_bq (z_bmq - z_bm'q)^2), the pair factor of Psi2 that does not
 *      depend on q(X*) (precompute it once while Z is frozen, e.g. as the gram of z with gamma / 2 and alpha^2; NULL computes
 *      it in the kernels).  1 <= B, N, M;  1 <= Q <= DPGP_QX_PSI_MAX_Q.  Sums over pairs / test points are added in a fixed
 *      order through the workspace: no atomics, the same bits on every run.
 *   dpgp_qx_psi_stats_batched_f64:  psi1[B][N][M] (rbf_kernel.py:135-161), psi2[B][M][M] (:164-199, summed over the N test
 *      points, exactly symmetric).  ws: dpgp_qx_psi_stats_workspace_bytes(B,N,M,Q).
 *   dpgp_qx_psi_adjoint_f64:  with g1[B][N][M] = dF/dPsi1_b and g2[B][M][M] = dF/dPsi2_b (any matrix; symmetry not assumed)
 *      d_mu[N][Q] = sum_b sum_m g1_b[n,m] dPsi1_b[n,m]/dmu[n,q] + sum_b sum_{m,m'} g2_b[m,m'] dPsi2_b[m,m']/dmu[n,q],  d_s
 *      likewise (the derivatives with respect to the variances s, not their softplus parameters).  No z / gamma / alpha
 *      outputs.  ws: dpgp_qx_psi_adjoint_workspace_bytes(B,N,M,Q).
 *   dpgp_qx_psi_stats_weighted_f64 / dpgp_qx_psi_adjoint_weighted_f64:  the same with a weight per (kernel, test point),
 *      w[B][N] (any finite values; NULL = all ones, which runs the unweighted kernels and gives the unweighted bits):
 *      psi2[b] = sum_n w[b][n] (test point n's Psi2 term of kernel b), still exactly symmetric; psi1 is not weighted.  The
 *      adjoint multiplies the Psi2 part of test point n's (d_mu, d_s) from kernel b by w[b][n]; the Psi1 part is governed by
 *      g1 alone (zero the rows of g1 that must not count).  A weight of 0 contributes exactly 0.0 and costs no exponential
 *      in the stats kernel; in the adjoint a wave of 64 consecutive test points whose weights for kernel b are all 0 skips
 *      its pair loops.  w is nullable like zfac and follows it, so the negative bad-argument codes, the order of the checks
 *      and the workspace sizes are those of the unweighted functions.  (An output dim observed at a subset of the test
 *      points is a kernel b with w[b][n] = 1 where it was measured: per-entry missing-data masks.)
 *   dpgp_qx_psi_param_adjoint_weighted_f64:  the other half of the backward pass, for a model that trains its inducing inputs
 *      and hyper-parameters through the (weighted) statistics.  With L = sum_b <g1_b, Psi1_b> + <g2_b, sum_n w[b][n] psi2_bn>
 *      (g2 any matrix) the outputs are dL/dz_b  d_z[B][M][Q], dL/dgamma_b  d_gamma[B][Q] and dL/dalpha_b  d_alpha[B], PER KERNEL
 *      b (not summed over b: a model whose slots share one kernel adds them).  The derivative is of the complete Psi2, pair
 *      factor included; zfac is only a cached value of it (NULL computes it in the kernel), w == NULL means all ones.  With
 *      d1 = mu_n - z_m, d2 = mu_n - (z_m + z_m') / 2, D = z_m - z_m', A1 = g1 Psi1, A2 = g2[m,m'] w[b][n] psi2_bn[m,m']:
 *        d/dz_mq    = sum_n A1 iw1 d1 + sum_n sum_m' (A2[m,m'] + A2[m',m]) (-1/2 gamma_q D_q + iw2 d2_q)
 *        d/dgamma_q = sum A1 (-1/2 s/w1 - 1/2 d1^2/w1^2) + sum A2 (-1/4 D_q^2 - s/w2 - d2_q^2/w2^2)
 *        d/dalpha   = (<g1, Psi1> + 2 <g2, Psi2 weighted>) / alpha
 *      A pair is visited once; a weight of 0 contributes exactly 0.0 to the Psi2 part and costs no exponential; partial sums
 *      go through the workspace in a fixed order (no atomics: the same bits on every run).  Bad-argument codes -1 .. -12 are
 *      those of dpgp_qx_psi_adjoint_weighted_f64, then d_z -13, d_gamma -14, d_alpha -15, ws -16, ws_bytes too small -17.
 *      ws: dpgp_qx_psi_param_adjoint_workspace_bytes(B,N,M,Q).
 *   The workspace queries are host functions (0 for a shape out of range). */
#define DPGP_QX_PSI_MAX_Q 64
size_t dpgp_qx_psi_stats_workspace_bytes(int B, int N, int M, int Q);
int dpgp_qx_psi_stats_batched_f64(int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                                  const double *gamma, const double *alpha, const double *zfac, double *psi1, double *psi2,
                                  void *ws, size_t ws_bytes, void *stream);
size_t dpgp_qx_psi_adjoint_workspace_bytes(int B, int N, int M, int Q);
int dpgp_qx_psi_adjoint_f64(int B, int N, int M, int Q, const double *z, const double *mu, const double *s, const double *gamma,
                            const double *alpha, const double *zfac, const double *g1, const double *g2, double *d_mu, double *d_s,
                            void *ws, size_t ws_bytes, void *stream);
int dpgp_qx_psi_stats_weighted_f64(int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                                   const double *gamma, const double *alpha, const double *zfac, const double *w, double *psi1,
                                   double *psi2, void *ws, size_t ws_bytes, void *stream);
int dpgp_qx_psi_adjoint_weighted_f64(int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                                     const double *gamma, const double *alpha, const double *zfac, const double *w,
                                     const double *g1, const double *g2, double *d_mu, double *d_s, void *ws, size_t ws_bytes,
                                     void *stream);
size_t dpgp_qx_psi_param_adjoint_workspace_bytes(int B, int N, int M, int Q);
int dpgp_qx_psi_param_adjoint_weighted_f64(int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                                           const double *gamma, const double *alpha, const double *zfac, const double *w,
                                           const double *g1, const double *g2, double *d_z, double *d_gamma, double *d_alpha,
                                           void *ws, size_t ws_bytes, void *stream);

/* ---- Pattern-grouped forms of the three operators above: K kernels (z[K][M][Q], gamma[K][Q], alpha[K], zfac NULL or
 *      [K][M][M]) and P weight rows w[P][N] shared by all K kernels (any finite reals; 0 / 1 for row patterns of a missing-data
 *      mask; required, not nullable).  The semantics are those of the weighted operators called with B = K P slots, slot (k, p)
 *      carrying kernel k's replicated inputs and weight row p and g1 split in any way over the slots of a kernel; the grouped
 *      forms evaluate each (kernel, point, pair) exponential once per chunk of PC patterns instead of once per slot, and read
 *      Psi1 / g1 once per kernel.  1 <= K, P, N, M;  1 <= Q <= DPGP_QX_PSI_MAX_Q.  No atomics: partial sums go through the
 *      workspace in a fixed order, the same bits on every run.  A point whose weights are 0 for a whole chunk costs no
 *      exponential and contributes exactly 0.0.
 *   dpgp_qx_psi_stats_grouped_f64:  psi1[K][N][M] (once per kernel, not weighted), psi2[K][P][M][M] = sum_n w[p][n] psi2_kn,
 *      exactly symmetric.  PC = 8 / 4 / 2 / 1 for P >= 5 / 3 / 2 / 1.
 *   dpgp_qx_psi_adjoint_grouped_f64:  g1[K][N][M] (already summed over the patterns), g2[K][P][M][M] (any matrices);
 *      d_mu[N][Q], d_s[N][Q] = the derivative of sum_k <g1_k, Psi1_k> + sum_kp <g2_kp, Psi2_kp>.  PC as for the stats, halved
 *      until PC tiles [32][33] fit the 160 KiB of LDS beside one wave's points: 8 for Q <= 46, 4 for Q <= 63, 2 at Q = 64.
 *   dpgp_qx_psi_param_adjoint_grouped_f64:  the same inputs; d_z[K][M][Q], d_gamma[K][Q], d_alpha[K] of the same sum, per
 *      kernel, summed over that kernel's patterns; the derivative of the complete Psi2, pair factor included.  PC as for the
 *      stats.
 *   Bad arguments, checked in this order before anything is launched:  K -1, P -2, N -3, M -4, Q -5, z -6, mu -7, s -8,
 *      gamma -9, alpha -10, (zfac: nullable, no code), w -12; then stats: psi1 -13, psi2 -14, ws -15, ws_bytes too small -16;
 *      adjoint: g1 -13, g2 -14, d_mu -15, d_s -16, ws -17, ws_bytes too small -18;  parameter adjoint: g1 -13, g2 -14, d_z -15,
 *      d_gamma -16, d_alpha -17, ws -18, ws_bytes too small -19.
 *   ws: the ..._grouped_workspace_bytes(K,P,N,M,Q) of the operator (host functions; 0 for a shape out of range). */
size_t dpgp_qx_psi_stats_grouped_workspace_bytes(int K, int P, int N, int M, int Q);
int dpgp_qx_psi_stats_grouped_f64(int K, int P, int N, int M, int Q, const double *z, const double *mu, const double *s,
                                  const double *gamma, const double *alpha, const double *zfac, const double *w, double *psi1,
                                  double *psi2, void *ws, size_t ws_bytes, void *stream);
size_t dpgp_qx_psi_adjoint_grouped_workspace_bytes(int K, int P, int N, int M, int Q);
int dpgp_qx_psi_adjoint_grouped_f64(int K, int P, int N, int M, int Q, const double *z, const double *mu, const double *s,
                                    const double *gamma, const double *alpha, const double *zfac, const double *w,
                                    const double *g1, const double *g2, double *d_mu, double *d_s, void *ws, size_t ws_bytes,
                                    void *stream);
size_t dpgp_qx_psi_param_adjoint_grouped_workspace_bytes(int K, int P, int N, int M, int Q);
int dpgp_qx_psi_param_adjoint_grouped_f64(int K, int P, int N, int M, int Q, const double *z, const double *mu, const double *s,
                                          const double *gamma, const double *alpha, const double *zfac, const double *w,
                                          const double *g1, const double *g2, double *d_z, double *d_gamma, double *d_alpha,
                                          void *ws, size_t ws_bytes, void *stream);

/* ---- Per-point Psi2 contractions (csrc/qx_psi_point.hip): K kernels (z[K][M][Q], gamma[K][Q], alpha[K], zfac NULL or
 *      [K][M][M]) that share q(X) = (mu[N][Q], s[N][Q]), as in the grouped operators.  With psi2_kn[m,m'] test point n's own
 *      term of kernel k's Psi2 (pair factor included; sum_n psi2_kn is psi2 of dpgp_qx_psi_stats_batched_f64):
 *        tr[K][N][G]   = sum_{m,m'} c_kg[m,m'] psi2_kn[m,m']                  c[K][G][M][M], any matrices: symmetry not assumed
 *        quad[K][N][J] = sum_{m,m'} r_k[m,j] r_k[m',j] psi2_kn[m,m']          r[K][M][J]
 *      (the per-entry predictive variance of a sparse GP at an uncertain input needs both: c = K^-1 - P per row pattern, r the
 *      posterior weights per output column).  One product E[N x pairs] W[pairs x (G + J)] per kernel on the fp64 matrix pipe:
 *      E is made on the fly, one exponential per (k, n, pair) and per chunk of up to 128 columns (64 for Q > 32), and nothing of
 *      size N M M or pairs x J is written to memory.  The workspace holds partial sums of the two outputs only (the pair tiles
 *      are split over workgroups when N K is small); a second launch adds them in a fixed order: no atomics, the same bits on
 *      every run.  1 <= K, G, J, N, M;  1 <= Q <= DPGP_QX_PSI_MAX_Q.
 *   Bad arguments, checked in this order before anything is launched:  K -1, G -2, J -3, N -4, M -5, Q -6, z -7, mu -8, s -9,
 *      gamma -10, alpha -11, (zfac: nullable, no code), c -13, r -14, tr -15, quad -16, ws -17, ws_bytes too small -18.
 *   ws: dpgp_qx_psi_pointwise_workspace_bytes(K,G,J,N,M,Q) (a host function; 0 for a shape out of range). */
size_t dpgp_qx_psi_pointwise_workspace_bytes(int K, int G, int J, int N, int M, int Q);
int dpgp_qx_psi_pointwise_f64(int K, int G, int J, int N, int M, int Q, const double *z, const double *mu, const double *s,
                              const double *gamma, const double *alpha, const double *zfac, const double *c, const double *r,
                              double *tr, double *quad, void *ws, size_t ws_bytes, void *stream);

/* ---- Per-entry predictive moments on the same contractions (csrc/qx_psi_point.hip).  Inputs as above, plus gidx[K][J] (int32: the
 *      trace column of output column j; any value outside [0, G) means "no trace term", a column never observed in training) and
 *      beta[K].  With psi1_kn[m], psi2_kn[m,m'] test point n's own statistics of kernel k and tr_kn[g] = <c_kg, psi2_kn>:
 *        mean[K][N][J] = sum_m psi1_kn[m] r_k[m,j]
 *        var[K][N][J]  = alpha_k + 1/beta_k - tr_kn[gidx[k][j]] + r_kj^T psi2_kn r_kj - mean^2
 *      Two launches: the pair kernel of dpgp_qx_psi_pointwise_f64 (its partial sums go to the workspace as there), then one
 *      kernel that forms psi1's exponentials on the fly, multiplies them with r (on the fp64 matrix pipe for J >= 16, plain FMA
 *      below), adds the slab partials in slab order, gathers the trace term and combines.  Nothing of size K N M, N M M or
 *      pairs x J is written to memory; no atomics, the same bits on every run.  Ranges as above.
 *   Bad arguments, checked in this order before anything is launched:  K -1, G -2, J -3, N -4, M -5, Q -6, z -7, mu -8, s -9,
 *      gamma -10, alpha -11, (zfac: nullable, no code), c -13, r -14, gidx -15, beta -16, mean -17, var -18, ws -19,
 *      ws_bytes too small -20.
 *   ws: dpgp_qx_psi_point_moments_workspace_bytes(K,G,J,N,M,Q) (a host function; 0 for a shape out of range). */
size_t dpgp_qx_psi_point_moments_workspace_bytes(int K, int G, int J, int N, int M, int Q);
int dpgp_qx_psi_point_moments_f64(int K, int G, int J, int N, int M, int Q, const double *z, const double *mu, const double *s,
                                  const double *gamma, const double *alpha, const double *zfac, const double *c, const double *r,
                                  const int *gidx, const double *beta, double *mean, double *var, void *ws, size_t ws_bytes,
                                  void *stream);

/* ---- Latent adjoint of the per-point contractions (csrc/qx_psi_point_adjoint.hip).  Inputs as dpgp_qx_psi_pointwise_f64, plus the
 *      adjoints h[K][N][J], gq[K][N][J], gt[K][N][G].  With psi1_kn[m], psi2_kn[m,m'] test point n's own statistics of kernel k:
 *        L = sum_knj h (psi1_kn . r_kj) + sum_knj gq (r_kj^T psi2_kn r_kj) + sum_kng gt <c_kg, psi2_kn>
 *        d_mu[N][Q] = dL/dmu,   d_s[N][Q] = dL/ds        (s: variances; summed over the kernels; no z, gamma or alpha outputs)
 *      Per kernel the adjoint of psi2_kn is formed first, T[N x pairs] = gq [N x J] (r r')[J x pairs] + gt [N x G] c~[G x pairs]
 *      (a pair m <= m' visited once, c symmetrised), multiplied element-wise with the point's exponentials and contracted with
 *      the 1 + 2Q moment columns (1, zbar_q, zbar_q^2): both products on the fp64 matrix pipe, one exponential per (k, n, pair)
 *      and per chunk of up to 64 of the G + J columns (32 for Q > 32).  The Psi1 term is the
 *      same over single inducing points.  Nothing of size N M M, K N M, pairs x J or pairs x G is written to memory.  The
 *      workspace holds partial (d_mu, d_s) of slabs of kernels, pair tiles and column chunks only; a second launch adds them in
 *      slab order: no atomics, the same bits on every run.  A zero adjoint contributes exactly 0.0.
 *      1 <= K, G, J, N, M;  1 <= Q <= DPGP_QX_PSI_MAX_Q.
 *   Bad arguments, checked in this order before anything is launched:  K -1, G -2, J -3, N -4, M -5, Q -6, z -7, mu -8, s -9,
 *      gamma -10, alpha -11, (zfac: nullable, no code), c -13, r -14, h -15, gq -16, gt -17, d_mu -18, d_s -19, ws -20,
 *      ws_bytes too small -21.
 *   ws: dpgp_qx_psi_pointwise_adjoint_workspace_bytes(K,G,J,N,M,Q) (a host function; 0 for a shape out of range). */
size_t dpgp_qx_psi_pointwise_adjoint_workspace_bytes(int K, int G, int J, int N, int M, int Q);
int dpgp_qx_psi_pointwise_adjoint_f64(int K, int G, int J, int N, int M, int Q, const double *z, const double *mu, const double *s,
                                      const double *gamma, const double *alpha, const double *zfac, const double *c,
                                      const double *r, const double *h, const double *gq, const double *gt, double *d_mu,
                                      double *d_s, void *ws, size_t ws_bytes, void *stream);

/* ---- Latent-space metric and predictive Jacobian at deterministic latent points (csrc/ard_rbf_point_metric.hip).  K kernels with
 *      their own inducing inputs z[K][M][Q], gamma[K][Q], alpha[K]; points x[N][Q] (no variances).  With
 *        k_km(x_n)  = alpha_k exp(-1/2 sum_q gamma_kq (x_nq - z_kmq)^2)
 *        b_kmq(x_n) = d k_km / d x_q = -gamma_kq (x_nq - z_kmq) k_km(x_n)
 *      the operators are
 *        g[K][N][Q][Q]   = sum_{m,m'} p[k][m][m'] b_kmq(x_n) b_km'q'(x_n)       p[K][M][M], any matrices, used as given: a
 *                                                                               non-symmetric p gives a non-symmetric g
 *        jac[K][N][J][Q] = sum_m b_kmq(x_n) r[k][m][j]                          r[K][M][J]
 *      The alpha diag(gamma) term of the expected metric is the caller's.  One launch each: a workgroup owns a kernel and a tile
 *      of points, makes the features b on the fly (one exponential per (k, n, m) and per slab of 64 rows of p or columns of r)
 *      and runs both products of the metric, p B and B^T (p B), on the fp64 matrix pipe; p is streamed in 64 x 64 tiles.
 *      Nothing of size N M Q is written to memory; no atomics, the order of every sum is fixed by (M, Q): the same bits on
 *      every run, and a kernel's results do not depend on K.  Points far from every z give exact zeros.
 *      1 <= K, J, N, M;  1 <= Q <= DPGP_QX_PSI_MAX_Q.
 *   Bad arguments, checked in this order before anything is launched:
 *      metric:    K -1, N -2, M -3, Q -4, z -5, x -6, gamma -7, alpha -8, p -9, g -10, ws -11, ws_bytes too small -12
 *      jacobian:  K -1, J -2, N -3, M -4, Q -5, z -6, x -7, gamma -8, alpha -9, r -10, jac -11, ws -12, ws_bytes too small -13
 *   ws: the results are written from the accumulators, so the queries (host functions) return a token 256 bytes for a shape in
 *      range and 0 for one out of range; the pair (ws, ws_bytes) keeps the calling convention of the other point operators. */
size_t dpgp_ard_rbf_point_metric_workspace_bytes(int K, int N, int M, int Q);
int dpgp_ard_rbf_point_metric_f64(int K, int N, int M, int Q, const double *z, const double *x, const double *gamma,
                                  const double *alpha, const double *p, double *g, void *ws, size_t ws_bytes, void *stream);
size_t dpgp_ard_rbf_point_jacobian_workspace_bytes(int K, int J, int N, int M, int Q);
int dpgp_ard_rbf_point_jacobian_f64(int K, int J, int N, int M, int Q, const double *z, const double *x, const double *gamma,
                                    const double *alpha, const double *r, double *jac, void *ws, size_t ws_bytes, void *stream);

/* ---- Curve energy at deterministic latent points along directions, with both gradients (csrc/ard_rbf_point_energy.hip): what a
 *      geodesic under the expected metric needs at every segment.  Kernels, points x[N][Q] and p[K][M][M] as for the metric
 *      operator above; directions v[N][Q], shared by the kernels.  With k_km and b_kmq as above and
 *        d_knmq = x_nq - z_kmq,   a_knm = sum_q gamma_kq d_knmq v_nq,   c_knm = sum_q b_kmq(x_n) v_nq = -k_km(x_n) a_knm
 *        w_knm  = sum_m' (p[k][m][m'] + p[k][m'][m]) c_knm'
 *      the operator gives
 *        e[K][N]     = sum_{m,m'} p[k][m][m'] c_knm c_knm' = 1/2 sum_m w_knm c_knm       (= v_n^T g[k][n] v_n of the metric operator)
 *        dx[K][N][Q] = d e / d x_nq = gamma_kq sum_m w_knm k_km (a_knm d_knmq - v_nq)
 *        dv[K][N][Q] = d e / d v_nq = -gamma_kq sum_m w_knm k_km d_knmq
 *      p is any matrix; the results depend on its symmetric part only.  The alpha diag(gamma) term of the expected metric is the
 *      caller's.  One launch: a workgroup owns a kernel and a tile of 16 points, forms c on the fly (one exponential per
 *      (k, n, m) and per slab of 64 rows of p), runs W = (p + p^T) C on the fp64 matrix pipe with p streamed in symmetrised
 *      64 x 64 tiles (no limit on M from the LDS) and adds each finished slab's rows to the sums above with the differences d.
 *      Nothing of size N M is written to memory; no atomics, the order of every sum is fixed by (M, Q): the same bits on every
 *      run; a point's results depend neither on N, nor on its place in x, nor on K.  Points far from every z give exact zeros.
 *      1 <= K, N, M;  1 <= Q <= DPGP_QX_PSI_MAX_Q.
 *   Bad arguments, checked in this order before anything is launched:  K -1, N -2, M -3, Q -4, z -5, x -6, v -7, gamma -8,
 *      alpha -9, p -10, e -11, dx -12, dv -13, ws -14, ws_bytes too small -15.
 *   ws: the results are written from registers, so the query (a host function) returns a token 256 bytes for a shape in range and
 *      0 for one out of range; the pair (ws, ws_bytes) keeps the calling convention of the other point operators. */
size_t dpgp_ard_rbf_point_energy_workspace_bytes(int K, int N, int M, int Q);
int dpgp_ard_rbf_point_energy_f64(int K, int N, int M, int Q, const double *z, const double *x, const double *v,
                                  const double *gamma, const double *alpha, const double *p, double *e, double *dx, double *dv,
                                  void *ws, size_t ws_bytes, void *stream);

/* ---- The geodesic equation at deterministic latent points (csrc/ard_rbf_point_metric.hip, csrc/geodesic_accel.hip): what one
 *      stage of an integrator of x'' = -G(x)^-1 Gamma(x, x') needs.  Kernels, points x[N][Q] and p[K][M][M] as for the metric
 *      operator above; velocities v[N][Q], shared by the kernels.  With k_km and b_kmq as above and
 *        a_knm = sum_q gamma_kq (x_nq - z_kmq) v_nq,   d_knm = k_km(x_n) (a_knm^2 - sum_q gamma_kq v_nq^2) = v_n^T (d2 k_km / dx dx) v_n
 *      the first operator gives
 *        g[K][N][Q][Q] = sum_{m,m'} p[k][m][m'] b_kmq(x_n) b_km'q'(x_n)         (exactly the metric operator's quantity)
 *        gam[K][N][Q]  = sum_{m,m'} b_kmq(x_n) p[k][m][m'] d_knm'
 *      p is used as given; for a symmetric p, gam is the Christoffel symbol of the first kind of g contracted twice with v,
 *      (D_v g) v - 1/2 grad_x (v^T g v).  One launch: the metric kernel's two products on the fp64 matrix pipe with the feature
 *      block of a point widened to [b_.1 .. b_.Q, d] (W = Q + 1 columns, ceil(W / 16) column tiles); p is streamed in 64 x 64
 *      tiles.  Nothing of size N M is written to memory; no atomics, the order of every sum is fixed by (M, Q): the same bits on
 *      every run; a point's results depend neither on N, nor on its place in x, nor on K.  Points far from every z give exact
 *      zeros.  1 <= K, N, M;  1 <= Q <= 63.
 *   Bad arguments, checked in this order before anything is launched:  K -1, N -2, M -3, Q -4, z -5, x -6, v -7, gamma -8,
 *      alpha -9, p -10, g -11, gam -12, ws -13, ws_bytes too small -14.
 *   ws: the results are written from the accumulators, so the query (a host function) returns a token 256 bytes for a shape in
 *      range and 0 for one out of range; the pair (ws, ws_bytes) keeps the calling convention of the other point operators.
 *      The finishing operator takes g[K][N][Q][Q], gam[K][N][Q], prior[Q] (a constant diagonal metric) and v[N][Q] and gives, per
 *      point, with G = sum_k g[k][n] + diag(prior) (k ascending),
 *        speed[N] = v_n^T G v_n,     a[N][Q] = -G^-1 sum_k gam[k][n]            by a Cholesky factorisation of G (lower triangle read)
 *        info[N]  = 0, or the 1-based index of the first pivot that is not positive: a[n][:] is then NaN; other points are unaffected
 *      One launch, a workgroup per point; no atomics, no workspace, nothing read on the host, the same bits on every run.
 *      1 <= K, N;  1 <= Q <= DPGP_QX_PSI_MAX_Q.
 *   Bad arguments, in this order:  K -1, N -2, Q -3, g -4, gam -5, prior -6, v -7, a -8, speed -9, info -10. */
size_t dpgp_ard_rbf_point_christoffel_workspace_bytes(int K, int N, int M, int Q);
int dpgp_ard_rbf_point_christoffel_f64(int K, int N, int M, int Q, const double *z, const double *x, const double *v,
                                       const double *gamma, const double *alpha, const double *p, double *g, double *gam,
                                       void *ws, size_t ws_bytes, void *stream);
int dpgp_geodesic_accel_f64(int K, int N, int Q, const double *g, const double *gam, const double *prior, const double *v,
                            double *a, double *speed, int *info, void *stream);

/* ---- The tangent of the geodesic equation (csrc/ard_rbf_point_metric.hip, csrc/geodesic_accel.hip): what one stage of the
 *      tangent-linear (Jacobi field) integrator needs, the derivative of the pair (g, gam) above and of the acceleration along a
 *      direction (dx, dv)[N][Q] of the state (x, v).  With u_q = gamma_kq (x_nq - z_kmq), k = k_km(x_n), b_q = -k u_q,
 *      a = sum_q u_q v_q, s = sum_q gamma_kq v_nq^2, d = k (a^2 - s) as above and
 *        e = sum_q u_q dx_q,   f = sum_q u_q dv_q,   c1 = sum_q gamma_kq dx_q v_q,   c2 = sum_q gamma_kq v_q dv_q
 *        db_q = k (e u_q - gamma_kq dx_q),           dd = k (-e (a^2 - s) + 2 a (c1 + f) - 2 c2)
 *      the first operator gives g and gam, WITH THE BITS of dpgp_ard_rbf_point_christoffel_f64, and
 *        dg[K][N][Q][Q] = dB^T p B + B^T p dB,       dgam[K][N][Q] = dB^T p d + B^T p dd          (p used as given)
 *      One launch: the same kernel with the feature block F = [B | d | dB | dd], W = 2 Q + 2 columns, ceil(W / 16) column tiles;
 *      all four results are entries of the one product F^T p F (dg: rows 0 .. Q-1 x columns Q+1 .. 2Q plus rows Q+1 .. 2Q x
 *      columns 0 .. Q-1; dgam: rows Q+1 .. 2Q of column Q plus rows 0 .. Q-1 of column 2Q+1).  The rules of the operator above
 *      hold: nothing of size N M in memory, no atomics, sums ordered by (M, Q) alone, a point's bits independent of N, its place
 *      and K, exact zeros far from every z and for a zero direction.  1 <= K, N, M;  1 <= Q <= 31.
 *   Bad arguments, checked in this order before anything is launched:  K -1, N -2, M -3, Q -4, z -5, x -6, v -7, dx -8, dv -9,
 *      gamma -10, alpha -11, p -12, g -13, gam -14, dg -15, dgam -16, ws -17, ws_bytes too small -18.
 *   ws: as above, a token 256 bytes for a shape in range, 0 for one out of range.
 *      The finishing operator takes the four results, prior[Q] and v[N][Q] and gives a, speed and info WITH THE BITS of
 *      dpgp_geodesic_accel_f64 on (g, gam), and with the same factor of G (the constant prior has no share in the tangent of G)
 *        da[N][Q] = -G^-1 ( sum_k dgam[k][n] + (sum_k dg[k][n]) a )              (k ascending)
 *      A pivot that is not positive ends that point alone: info = its 1-based index, a[n][:] = da[n][:] = NaN.
 *      1 <= K, N;  1 <= Q <= DPGP_QX_PSI_MAX_Q.
 *   Bad arguments, in this order:  K -1, N -2, Q -3, g -4, gam -5, dg -6, dgam -7, prior -8, v -9, a -10, da -11, speed -12,
 *      info -13. */
size_t dpgp_ard_rbf_point_christoffel_tangent_workspace_bytes(int K, int N, int M, int Q);
int dpgp_ard_rbf_point_christoffel_tangent_f64(int K, int N, int M, int Q, const double *z, const double *x, const double *v,
                                               const double *dx, const double *dv, const double *gamma, const double *alpha,
                                               const double *p, double *g, double *gam, double *dg, double *dgam, void *ws,
                                               size_t ws_bytes, void *stream);
int dpgp_geodesic_accel_tangent_f64(int K, int N, int Q, const double *g, const double *gam, const double *dg,
                                    const double *dgam, const double *prior, const double *v, double *a, double *da,
                                    double *speed, int *info, void *stream);

/* ---- Parallel transport along a geodesic (csrc/ard_rbf_point_metric.hip, csrc/geodesic_accel.hip): what one stage of an
 *      integrator of the transport equation w' = -G^-1 Gamma(x; v, w) needs, for a frame of F vectors w[N][F][Q] at once.
 *      With u_q, k, b_q, a = a_v, d = d(v,v) as above and, per vector w_r of the frame,
 *        a_w = sum_q u_q w_q,     d(v,w) = v^T (d^2 k / dx dx) w = k (a_v a_w - sum_q gamma_kq v_q w_q)
 *      the first operator gives g and gam, WITH THE BITS of dpgp_ard_rbf_point_christoffel_f64, and
 *        tgam[K][N][F][Q] = B^T p d(v,w_r)                                                               (p used as given)
 *      which for a symmetric p is the Christoffel symbol of the first kind of g contracted with v and w_r.
 *      One launch: the same kernel with the feature block [B | d(v,v) | d(v,w_1) .. d(v,w_F)], W = Q + 1 + F columns,
 *      ceil(W / 16) column tiles; tgam[..][r][:] is rows 0 .. Q-1 of column Q + 1 + r of the one product.  Result tiles below
 *      row Q are not formed.  d(v,w) is made with the statements of d(v,v): for w_r = v, tgam[..][r][:] has the bits of gam; a
 *      vector's tgam depends neither on F, nor on r, nor on the other vectors.  The rules of the operators above hold: nothing of
 *      size N M in memory, no atomics, sums ordered by (M, Q) alone, a point's bits independent of N, its place and K, exact
 *      zeros far from every z and for w = 0.  1 <= K, N, M, Q, F;  Q + 1 + F <= 64.
 *   Bad arguments, checked in this order before anything is launched:  K -1, N -2, M -3, Q -4, F -5, z -6, x -7, v -8, w -9,
 *      gamma -10, alpha -11, p -12, g -13, gam -14, tgam -15, ws -16, ws_bytes too small -17.
 *   ws: as above, a token 256 bytes for a shape in range, 0 for one out of range.
 *      The finishing operator takes the three results, prior[Q] and v[N][Q] and gives a, speed and info WITH THE BITS of
 *      dpgp_geodesic_accel_f64 on (g, gam), and with the same factor of G (the constant prior has no Christoffel symbols)
 *        dw[N][F][Q] = -G^-1 sum_k tgam[k][n][r]                                  (k ascending)
 *      all 1 + F right-hand sides in one pair of substitutions, each with the statements of a's: where tgam[..][r][:] has the
 *      bits of gam, dw[n][r][:] has the bits of a[n][:].  A pivot that is not positive ends that point alone: info = its 1-based
 *      index, a[n][:] = dw[n][:][:] = NaN.  1 <= K, N;  1 <= Q <= DPGP_QX_PSI_MAX_Q;  1 <= F <= 63.
 *   Bad arguments, in this order:  K -1, N -2, Q -3, F -4, g -5, gam -6, tgam -7, prior -8, v -9, a -10, dw -11, speed -12,
 *      info -13. */
size_t dpgp_ard_rbf_point_transport_workspace_bytes(int K, int N, int M, int Q, int F);
int dpgp_ard_rbf_point_transport_f64(int K, int N, int M, int Q, int F, const double *z, const double *x, const double *v,
                                     const double *w, const double *gamma, const double *alpha, const double *p, double *g,
                                     double *gam, double *tgam, void *ws, size_t ws_bytes, void *stream);
int dpgp_geodesic_transport_f64(int K, int N, int Q, int F, const double *g, const double *gam, const double *tgam,
                                const double *prior, const double *v, double *a, double *dw, double *speed, int *info,
                                void *stream);

/* ---- The integrators of the geodesic equation on the device (csrc/geodesic_accel.hip): the classical Runge-Kutta solution of
 *      (x', v') = (v, -G(x)^-1 Gamma(x, v)) on t in [0, 1] at step h = 1 / S for C curves from x[C][Q] with velocities v[C][Q], and
 *      its tangent-linear solution (a discrete Jacobi field) from (dx, dv)[C][Q], all steps from ONE call.  The metric is given
 *      as `parts` parts, part i being the kernels z[i][K_i][M_i][Q], gamma[i][K_i][Q], alpha[i][K_i] and p[i][K_i][M_i][M_i] of the
 *      christoffel operators above (K, M: host arrays of `parts` ints; z, gamma, alpha, p: host arrays of `parts` device
 *      pointers), plus the constant diagonal prior[Q]:  G = sum_i sum_k g_ik + diag(prior), kernels in part order.
 *      Per stage the call enqueues dpgp_ard_rbf_point_christoffel[_tangent]_f64 once per part, each into its slice of one slab
 *      array [sum_i K_i][C][..] in the workspace, and then one stage kernel, a workgroup of one wave per curve, which does
 *      dpgp_geodesic_accel[_tangent]_f64's work on the slabs (the same code: slab sums in ascending k, Cholesky in LDS, the
 *      solves) and applies the stage's share of the step to a per-curve state in the workspace:
 *        next arguments  base + (h/2) k  (stage 3: base + h k),    running sums ((k1 + 2 k2) + 2 k3) + k4,
 *        stage 4:        row s+1 = base + (h/6) sums               (each product rounded before its add)
 *      with h, h/2 and h/6 formed in double on the host.  4 S (parts + 1) launches in order on `stream`; nothing is allocated
 *      and nothing is read on the host; no atomics, no cooperative launch; the same bits on every run, and a curve's bits depend
 *      neither on C nor on its place.  The results carry the bits of the host loop of models/geodesic.py on the two operators.
 *        curve, vel[, dcurve, dvel] [C][S+1][Q]   the states after every step; row 0 holds the bits of x, v[, dx, dv]
 *        bad[C]                                   the number of stages whose G failed to factor; such a stage leaves NaN in its
 *                                                 curve from there on, the other curves are unaffected
 *        speed0[C]  (tangent)                     v^T G(x) v at the start
 *      1 <= parts <= 64;  1 <= K_i, M_i, C, S;  1 <= Q <= 63, tangent 1 <= Q <= 31.
 *   Bad arguments, checked in this order before anything is launched:  parts -1, K (null, or an entry < 1) -2, M -3, Q -4, C -5,
 *      S -6, z (null, or a null entry) -7, gamma -8, alpha -9, p -10, prior -11, x -12, v -13, then
 *        shoot:          curve -14, vel -15, bad -16, ws -17, ws_bytes too small -18
 *        shoot_tangent:  dx -14, dv -15, curve -16, vel -17, dcurve -18, dvel -19, bad -20, speed0 -21, ws -22, ws_bytes too small -23
 *   ws: dpgp_geodesic_shoot_workspace_bytes (a host function; tangent != 0 for the tangent call) bytes: the slabs,
 *      sum_i K_i C (Q Q + Q) doubles (tangent: twice that), and 6 (tangent: 12) C Q doubles of state; 0 for a shape out of range. */
size_t dpgp_geodesic_shoot_workspace_bytes(int parts, const int *K, const int *M, int Q, int C, int tangent);
int dpgp_geodesic_shoot_f64(int parts, const int *K, const int *M, int Q, int C, int S, const double *const *z,
                            const double *const *gamma, const double *const *alpha, const double *const *p, const double *prior,
                            const double *x, const double *v, double *curve, double *vel, int *bad, void *ws, size_t ws_bytes,
                            void *stream);
int dpgp_geodesic_shoot_tangent_f64(int parts, const int *K, const int *M, int Q, int C, int S, const double *const *z,
                                    const double *const *gamma, const double *const *alpha, const double *const *p,
                                    const double *prior, const double *x, const double *v, const double *dx, const double *dv,
                                    double *curve, double *vel, double *dcurve, double *dvel, int *bad, double *speed0, void *ws,
                                    size_t ws_bytes, void *stream);

/* ---- Joint posterior covariance at deterministic latent points (csrc/ard_rbf_point_cov.hip): the off-diagonal that the per-point
 *      operators above leave out.  Kernels z[K][M][Q], gamma[K][Q], alpha[K] and points x[N][Q] as for the metric operator;
 *      c[K][G][M][M]: G matrices per kernel (one per training row pattern), any matrices.  With k_km as above,
 *        out[k][g][i][j] = alpha_k exp(-1/2 sum_q gamma_kq (x_iq - x_jq)^2) - sum_{m,m'} k_km(x_i) c[k][g][m][m'] k_km'(x_j)
 *      out[K][G][N][N].  Rules:
 *      - both products run on v_mfma_f64_16x16x4, the exponentials are dpgp_exp2;
 *      - c enters through its symmetric part (c + c^T) / 2 only, symmetrised as its 64 x 64 tiles are staged;
 *      - the result is EXACTLY symmetric: only tile pairs J <= I (tiles of 32 points) are evaluated, an entry (i, j) with
 *        i > j is computed once and stored to both places;
 *      - the G patterns of a kernel share the features: the number of exponentials does not depend on G (a workgroup makes
 *        the features of a block of 64 inducing points at its 64 points once per pair of blocks, for all patterns);
 *      - nothing of size N M, K N M or K G N M is written to memory; c is streamed in tiles and the features in blocks: no
 *        limit on M from the LDS;
 *      - no atomics, the order of every sum is fixed by (M, Q): the same bits on every run; kernel k's results do not depend
 *        on K, G or the other kernels and patterns; entry (i, j) depends neither on N, nor on the places of i and j in x,
 *        nor on which of the two comes first;
 *      - points far from every z give the prior term alone: every product with the exact zeros of dpgp_exp2 is 0, no NaN.
 *      1 <= K, G, M;  1 <= N <= 46340 (N N fits 31 bits);  1 <= Q <= DPGP_QX_PSI_MAX_Q.
 *   Bad arguments, checked in this order before anything is launched:  K -1, G -2, N -3, M -4, Q -5, z -6, x -7, gamma -8,
 *      alpha -9, c -10, out -11, ws -12, ws_bytes too small -13.
 *   ws: the results are written from registers, so the query (a host function) returns a token 256 bytes (never more) for a
 *      shape in range and 0 for one out of range; the pair (ws, ws_bytes) keeps the calling convention of the other point
 *      operators. */
size_t dpgp_ard_rbf_point_cov_workspace_bytes(int K, int G, int N, int M, int Q);
int dpgp_ard_rbf_point_cov_f64(int K, int G, int N, int M, int Q, const double *z, const double *x, const double *gamma,
                               const double *alpha, const double *c, double *out, void *ws, size_t ws_bytes, void *stream);

/* ---- Latent adjoint of B kernels that share inducing inputs AND q(X*) (csrc/psi_latent_adjoint.hip): the frozen over-D model at
 *      test time.  z[M][Q], q(X*) = (mu[N][Q], s[N][Q]: variances), gamma[B][Q], alpha[B]; y[N][ldy]: zero-filled data, column b
 *      for kernel b; w[B][N]: weights of the test points (NULL = all ones; any finite reals); stage-A adjoints g_v[B][M] and
 *      g_psi2[B][M][M] (any matrices: symmetry not assumed).  With psi1_bn[m], psi2_bn[m,m'] test point n's own terms of kernel b:
 *        L = sum_b <g_psi2_b, sum_n w[b][n] psi2_bn> + sum_b g_v_b . (Psi1_b^T y_b)
 *        d_mu[N][Q] = dL/dmu,   d_s[N][Q] = dL/ds           (no z, gamma or alpha outputs: the model is frozen)
 *      Per kernel one product E[N x pairs] W[pairs x (1 + 2Q)] on the fp64 matrix pipe: a pair m <= m' is visited once, E is
 *      made on the fly (one exponential per (b, n, pair); per chunk of 128 moment columns, i.e. twice at Q = 64), W is formed in
 *      LDS from g_psi2 and z; the Psi1 term is the same product over single inducing points.  Nothing of size B (1 + 2Q) M M,
 *      N M M or B N M is written to memory.  A workgroup owns 64 test points and a slab of kernels b, walked in ascending order;
 *      the workspace holds the slabs' partial (d_mu, d_s) only and a second launch adds them in slab order: no atomics, the
 *      same bits on every run.  A weight of 0 and a y of 0 contribute exactly 0.0.  1 <= B, N, M;  1 <= Q <= DPGP_QX_PSI_MAX_Q;
 *      ldy >= B.
 *   Bad arguments, checked in this order before anything is launched:  B -1, N -2, M -3, Q -4, z -5, mu -6, s -7, gamma -8,
 *      alpha -9, y -10, ldy -11, (w: nullable, no code), g_v -13, g_psi2 -14, d_mu -15, d_s -16, ws -17, ws_bytes too small -18.
 *   ws: dpgp_psi_latent_adjoint_workspace_bytes(B,N,M,Q) (a host function; 0 for a shape out of range). */
size_t dpgp_psi_latent_adjoint_workspace_bytes(int B, int N, int M, int Q);
int dpgp_psi_latent_adjoint_f64(int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                                const double *gamma, const double *alpha, const double *y, int ldy, const double *w,
                                const double *g_v, const double *g_psi2, double *d_mu, double *d_s, void *ws, size_t ws_bytes,
                                void *stream);

/* ---- Kernel.covariance_diag (rbf_kernel.py:96-116): out[B,N] = alpha_b (+1/beta_b) (+jitter) */
int dpgp_ard_rbf_diag_f32(int B, int N, const float *alpha, const float *beta, int flags, double jitter, float *out,
                          void *stream);
int dpgp_ard_rbf_diag_f64(int B, int N, const double *alpha, const double *beta, int flags, double jitter, double *out,
                          void *stream);

/* ---- Kernel.psi_0 (rbf_kernel.py:119-132): out[B] = alpha_b * N */
int dpgp_psi0_f32(int B, int N, const float *alpha, float *out, void *stream);
int dpgp_psi0_f64(int B, int N, const double *alpha, double *out, void *stream);

/* ---- Kernel.psi_1 (rbf_kernel.py:135-161): out[B,N,M] */
int dpgp_psi1_f32(int B, int N, int M, int Q, const float *z, const float *mu, const float *s, const float *gamma,
                  const float *alpha, float *out, void *stream);
int dpgp_psi1_f64(int B, int N, int M, int Q, const double *z, const double *mu, const double *s, const double *gamma,
                  const double *alpha, double *out, void *stream);

/* ---- Psi1_b^T y_b without materialising Psi1 (replaces the two [D,M,N] solves + [D,N,N] product of
 *      dp_gp_lvm.py:132-136,145): y is [N, ldy] with column b used for batch entry b; out[B,M].
 *      ws: dpgp_psi1T_y_workspace_bytes(B,N,M).                                                                   */
size_t dpgp_psi1T_y_workspace_bytes(int B, int N, int M);
int dpgp_psi1T_y_f32(int B, int N, int M, int Q, const float *z, const float *mu, const float *s, const float *gamma,
                     const float *alpha, const float *y, int ldy, float *out, void *ws, size_t ws_bytes, void *stream);
int dpgp_psi1T_y_f64(int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                     const double *gamma, const double *alpha, const double *y, int ldy, double *out, void *ws,
                     size_t ws_bytes, void *stream);

/* ---- Kernel.psi_2 (rbf_kernel.py:164-199): out[B,M,M], streamed over n (no [B,N,M,M,Q] temporary).
 *      ws: dpgp_psi2_workspace_bytes(B,N,M,Q,elem_size).                                                           */
size_t dpgp_psi2_workspace_bytes(int B, int N, int M, int Q, int elem_size);
int dpgp_psi2_f32(int B, int N, int M, int Q, const float *z, const float *mu, const float *s, const float *gamma,
                  const float *alpha, float *out, void *ws, size_t ws_bytes, int algo, void *stream);
int dpgp_psi2_f64(int B, int N, int M, int Q, const double *z, const double *mu, const double *s, const double *gamma,
                  const double *alpha, double *out, void *ws, size_t ws_bytes, int algo, void *stream);
/* ---- Psi2 with a weight per (batch entry, observation): out[b] = sum_n w[b][n] psi2_bn, where psi2_bn is row n's term of the
 *      sum dpgp_psi2_f64 forms; exactly symmetric.  fp64.  w[B][N] >= 0 and finite (behaviour for negative weights is
 *      unspecified); a weight of 0 contributes exactly 0.0 and a run of rows with weight 0 is not evaluated at all (missing
 *      entries of a data matrix: w = 0 / 1).  w == NULL: the unweighted kernels of dpgp_psi2_f64, bit for bit.  w adds no
 *      bad-argument code: codes, their order and ws (dpgp_psi2_workspace_bytes(B,N,M,Q,8)) are those of dpgp_psi2_f64.
 *      algo: DPGP_ALGO_AUTO (matrix cores) or DPGP_ALGO_PLAIN, anything else -13.  No atomics: the same bits on every run. */
int dpgp_psi2_weighted_f64(int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                           const double *gamma, const double *alpha, const double *w /* [B][N], nullable */, double *out,
                           void *ws, size_t ws_bytes, int algo, void *stream);

/* ---- tf.cholesky (dp_gp_lvm.py:116,127): in-place lower Cholesky of a[B,M,M] (upper triangle zeroed), info[B].
 *      ws: dpgp_potrf_workspace_bytes(B,M,elem_size).                                                              */
size_t dpgp_potrf_workspace_bytes(int B, int M, int elem_size);
int dpgp_potrf_batched_f32(int B, int M, float *a, int *info, void *ws, size_t ws_bytes, int algo, void *stream);
int dpgp_potrf_batched_f64(int B, int M, double *a, int *info, void *ws, size_t ws_bytes, int algo, void *stream);

/* ---- tf.matrix_triangular_solve(lower=True) (dp_gp_lvm.py:118-121,132-133): rhs[B,M,K] <- l[B,M,M]^-1 rhs.
 *      ws: dpgp_trsm_workspace_bytes(B,M,K,elem_size).                                                             */
size_t dpgp_trsm_workspace_bytes(int B, int M, int K, int elem_size);
int dpgp_trsm_batched_f32(int B, int M, int K, const float *l, float *rhs, void *ws, size_t ws_bytes, int algo,
                          void *stream);
int dpgp_trsm_batched_f64(int B, int M, int K, const double *l, double *rhs, void *ws, size_t ws_bytes, int algo,
                          void *stream);
/* L^-1 of B lower-triangular factors l[B][M][M] (M a multiple of 128; -2 otherwise): out[B][M][M] = L^-1, lower, zeros above the
 * diagonal — tf.matrix_triangular_solve(l, eye) (the composed stage A of the backward pass for M > 128 forms K_uu^-1 = W^T W and
 * B^-1 from it) as one persistent-workgroup launch per batch (potrf_persist.hip).  ws: B doubles. */
int dpgp_trtri_lower_batched_f64(int B, int M, const double *l, double *out, void *ws, size_t ws_bytes, void *stream);

/* ---- strided batched matrix product, fp64, on the matrix cores:  C[b] = alpha A[b] B[b] + beta C[b],
 *      A[b][i][k] = a[b a_sb + i a_si + k a_sk],  B[b][k][j] = b[b b_sb + k b_sk + j b_sj],  C likewise (element strides:
 *      a transposed, sliced or batch-broadcast (stride 0) operand is a choice of strides).  m x k times k x n, batch >= 1.
 *      Replaces the tf.matmul call sites of the composed models: Psi1^T Y of the over-T objective
 *      (/root/reference/src/models/dp_gp_lvm.py:657-658), the prediction bound (dp_gp_lvm.py:300-420) and the adjoint
 *      algebra of their backward passes.  beta == 0: C is not read.  Returns -(argument index) on a bad argument. */
int dpgp_gemm_strided_f64(int batch, int m, int n, int k, double alpha, const double *a, long long a_sb, long long a_si,
                          long long a_sk, const double *b, long long b_sb, long long b_sk, long long b_sj, double beta,
                          double *c, long long c_sb, long long c_si, long long c_sj, void *stream);

/* ---- calculate_kl_divergence_standard_prior (gp_expressions.py:10-24): out[1] (fp64) */
int dpgp_kl_qx_f32(int N, int Q, const float *mu, const float *s, double *out, void *stream);
int dpgp_kl_qx_f64(int N, int Q, const double *mu, const double *s, double *out, void *stream);

/* ---- the fused per-output ELBO reduction, dp_gp_lvm.py:108-145, for D output dims resident on this GPU.
 *   inputs (all fp64 device arrays; they are rounded to fp32 on the fly where `prec` says so):
 *     y[N,ldy] (column d = output d), z[M,Q], mu[N,Q], s[N,Q], gamma[D,Q], alpha[D], beta[D]
 *   outputs (fp64): terms[D,5] = { N/2 (log beta - log 2pi), -sum log diag L_A, beta/2 (tr(L^-1 Psi2 L^-T) - alpha N),
 *                                  -beta/2 y'y, beta^2/2 |L_A^-1 L^-1 Psi1' y|^2 }   (f_hat = sum of all entries)
 *                   sums[2]    = { f_hat, KL(q(X)||p(X)) }
 *                   info[D]    (see top of file)
 *   ws: dpgp_elbo_workspace_bytes(D,N,M,Q,prec).  algo: DPGP_ALGO_*.                                               */
size_t dpgp_elbo_workspace_bytes(int D, int N, int M, int Q, int prec);
/* where a finished dpgp_elbo_fhat call left its streaming results inside ws: out[10] = { byte offset of the Psi2 partial slabs
 * [ns2][D][Mp][Mp] (lower 64x64 patches; their sum over the slabs is Psi2), ns2, element size of the slabs (4 or 8), Mp,
 * byte offset of the Psi1^T y partial slabs [ns1][D][M] (fp64), ns1, byte offset of the y^T y partial slabs [nyy][D] (fp64), nyy,
 * byte offset of guard[D] (fp64: bound on the effect of an fp32 Psi2's rounding on each output dim's terms), D }.
 * Used by the host-side composition of the backward pass's stage A for M > 128 (ops.elbo_grad_chain). */
int dpgp_elbo_workspace_layout(int D, int N, int M, int Q, int prec, size_t *out);
/* what the front launch of a finished dpgp_elbo_fhat[_ex] call left inside ws: out[6] = { byte offset of K_uu + jitter I of output
 * dim 0 ([Mp][Mp], the square [0,M) x [0,M) written), byte stride between output dims, element size (4 or 8), Mp, byte offset of the
 * pair factors alpha_d^2 exp(-1/4 sum_q gamma_dq (z_mq - z_m'q)^2) of the pair-tile Psi2 kernel (fp32 [D][Ppad], pair (m, m'),
 * m' <= m, at m (m + 1) / 2 + m'; DPGP_ALGO_AUTO), Ppad -- 0 where that kernel does not run (fp64 Psi2, Q > 21) }. */
int dpgp_elbo_workspace_front_layout(int D, int N, int M, int Q, int prec, size_t *out);
int dpgp_elbo_fhat(int D, int N, int M, int Q, const double *y, int ldy, const double *z, const double *mu,
                   const double *s, const double *gamma, const double *alpha, const double *beta, double jitter,
                   int prec, int algo, double *terms, double *sums, int *info, void *ws, size_t ws_bytes,
                   void *stream);
/* same, with optional extras (exec may be NULL = dpgp_elbo_fhat):
 *   ev_psi2_begin / ev_psi2_end : caller-created hipEvent_t recorded on `stream` immediately before / after the psi2
 *       launch so that a harness can time the dominant kernel inside its timed region; either may be NULL.
 *   model_scal / model_pack / model_out : fold the model-level tail into the last launch.  model_scal = the scal array
 *       written by dpgp_model_prepare for the same D; then model_pack[2] (if given) receives what dpgp_model_pack would
 *       write and model_out[5] (if given; single-GPU case) what dpgp_model_finalize would write.  NULL: not done.     */
typedef struct dpgp_exec {
    void *ev_psi2_begin;
    void *ev_psi2_end;
    const double *model_scal;
    double *model_pack;
    double *model_out;
    /* parallel branch (all three set, or none): the Psi1^T y launch — independent of the psi2 launch, both feed the chain —
     * goes to `stream_aux` between `ev_fork` (recorded on `stream` after the front launch) and `ev_join` (waited for by
     * `stream` before the chain launch).  Caller-created: dpgp_stream_create / dpgp_event_create.  Graph-capturable. */
    void *stream_aux;
    void *ev_fork;
    void *ev_join;
} dpgp_exec_t;
int dpgp_elbo_fhat_ex(int D, int N, int M, int Q, const double *y, int ldy, const double *z, const double *mu,
                      const double *s, const double *gamma, const double *alpha, const double *beta, double jitter,
                      int prec, int algo, double *terms, double *sums, int *info, void *ws, size_t ws_bytes,
                      void *stream, const dpgp_exec_t *exec);
/* Backward pass of the fused ELBO, stage A (first version; reference: tf.gradients(objective) as used by every training
 * script, test/synthetic_data_hard_test.py:143-155; the forward it differentiates: src/models/dp_gp_lvm.py:108-145).
 * Adjoints of the per-output dense algebra, computed from the workspace `ws` of a FINISHED dpgp_elbo_fhat[_ex] call with
 * the same D, N, M, Q, prec (prec = DPGP_PREC_MIXED or DPGP_PREC_F64; M <= 128: B_d is kept in LDS; -30 otherwise — for larger
 * M the host side composes this stage from dpgp_potrf_batched / dpgp_trsm_batched and plain GEMMs, ops.py).  Mp = 16 * ceil(M / 16).
 *   g_psi2[D][Mp][Mp]  d f_hat / d Psi2_d   (lower triangle j <= i valid, symmetric)
 *   w_kuu [D][Mp][Mp]  (d f_hat / d K_uu,d) .* (K_uu,d - jitter I)   (lower triangle)
 *   g_v   [D][Mp]      d f_hat / d (Psi1_d^T y_d)
 *   d_alpha_beta[D][2] d f_hat / d alpha_d (complete: direct + through K_uu, Psi1, Psi2) and d f_hat / d beta_d
 *   info[D]            0 or the failing minor of B_d = K_uu,d + beta_d Psi2_d                                              */
int dpgp_elbo_grad_chain(int D, int N, int M, int Q, const double *alpha, const double *beta, double jitter, int prec,
                         void *ws, size_t ws_bytes, double *g_psi2, double *w_kuu, double *g_v, double *d_alpha_beta,
                         int *info, void *stream);
/* As dpgp_elbo_grad_chain, reading psi2_slabs Psi2 slabs of the workspace: 0 = the forward's own count (dpgp_elbo_grad_chain), 1 after
 * dpgp_elbo_fhat_step, which leaves one slab whatever dpgp_elbo_workspace_layout reports. */
int dpgp_elbo_grad_chain_ex(int D, int N, int M, int Q, const double *alpha, const double *beta, double jitter, int prec,
                            void *ws, size_t ws_bytes, int psi2_slabs, double *g_psi2, double *w_kuu, double *g_v,
                            double *d_alpha_beta, int *info, void *stream);
/* Stage A for M > 128, M a multiple of 128 (-3 otherwise: the host side composes it from dpgp_potrf_batched / dpgp_trsm_batched /
 * dpgp_gemm_strided_f64 then): the same adjoints from the forward evaluation's workspace, on [D][M][M] fp64 matrices in memory — the
 * persistent-workgroup Cholesky and solve (L^-1 with every block row stored), five strided MFMA products and three streaming kernels
 * (csrc/chain_grad_big.hip).  K_uu is rebuilt from z, gamma, alpha (rbf_kernel.py:58-93).  psi2_slabs: 0 = the forward's own count of
 * Psi2 slabs, 1 after dpgp_elbo_fhat_step.  ws: dpgp_elbo_grad_chain_big_workspace_bytes(D, M) (six [D][M][M] matrices).  Outputs as
 * dpgp_elbo_grad_chain with Mp = M, both triangles written. */
size_t dpgp_elbo_grad_chain_big_workspace_bytes(int D, int M);
int dpgp_elbo_grad_chain_big(int D, int N, int M, int Q, const double *z, const double *gamma, const double *alpha,
                             const double *beta, double jitter, int prec, void *fwd_ws, size_t fwd_ws_bytes, int psi2_slabs, void *ws,
                             size_t ws_bytes, double *g_psi2, double *w_kuu, double *g_v, double *d_alpha_beta, int *info,
                             void *stream);

/* Backward pass, stage B: second streaming pass over the observations — the derivatives of
 * <g_psi2, Psi2> + <g_v, Psi1^T y> + <d f_hat / d K_uu, K_uu> (reference forward: src/kernels/rbf_kernel.py:58-199) with
 * respect to mu[N,Q], the diagonal q(X) variances s[N,Q], z[M,Q] and gamma[D,Q], given the stage-A adjoints.  alpha is a
 * constant factor here (its derivative is complete in d_alpha_beta of stage A).
 *   DPGP_PREC_MIXED: fp32 arithmetic, fp64 sums of the per-workgroup partial results, any M: the Psi2 term on the matrix pipe
 *     (psi2_grad_kernel: the forward's f16-split exponent tiles, a second MFMA product for the z-weighted column sums), the
 *     Psi1 term by two reduction-free kernels, the K_uu term without a pass over the observations;
 *   DPGP_PREC_F64: one plain kernel, M <= 128, and at 113 <= M <= 128 Q <= 20: M x M adjoint and z in 160 KB of LDS (-30 otherwise).
 * M may exceed N (prediction evaluates few test points).  ws: dpgp_elbo_grad_psi_workspace_bytes_ex(D,N,M,Q,prec) — the
 * images and results of the pair-tile form (the bulk: ~1.6 GB at N=2000, D=512, M=128, Q=10) are only part of it for
 * DPGP_PREC_MIXED; dpgp_elbo_grad_psi_workspace_bytes(D,N,M,Q) = the largest of the three (works for every prec).            */
size_t dpgp_elbo_grad_psi_workspace_bytes(int D, int N, int M, int Q);
size_t dpgp_elbo_grad_psi_workspace_bytes_ex(int D, int N, int M, int Q, int prec);
int dpgp_elbo_grad_psi(int D, int N, int M, int Q, const double *y, int ldy, const double *z, const double *mu,
                       const double *s, const double *gamma, const double *alpha, const double *g_psi2,
                       const double *w_kuu, const double *g_v, int prec, void *ws, size_t ws_bytes, double *d_mu,
                       double *d_s, double *d_z, double *d_gamma, void *stream);
/* dpgp_elbo_grad_psi(prec = DPGP_PREC_F64) with a weight per (output dim, observation) on the Psi2 term: the derivatives, with
 * respect to mu, s, z and gamma_d, of  sum_d <g_psi2_d, sum_n w[d][n] psi2_dn> + <g_v_d, Psi1_d^T y_d> + the K_uu term.  The Psi1
 * term is governed by y alone (the caller zero-fills it where an entry is missing), the K_uu term is unweighted, alpha stays a
 * constant factor.  w[D][N] >= 0 and finite (behaviour for negative weights is unspecified); a weight of 0 contributes exactly 0.0,
 * and a pair of observations (2k, 2k+1 of an n-split) with w = 0 and y = 0 is not evaluated.  w == NULL: the unweighted kernel, bit
 * for bit.  w adds no bad-argument code: codes, their order and ws (dpgp_elbo_grad_psi_workspace_bytes_ex(D,N,M,Q,DPGP_PREC_F64))
 * are those of dpgp_elbo_grad_psi; M <= 128 (-30 otherwise).  No atomics: the same bits on every run. */
int dpgp_elbo_grad_psi_weighted_f64(int D, int N, int M, int Q, const double *y, int ldy, const double *z, const double *mu,
                                    const double *s, const double *gamma, const double *alpha,
                                    const double *w /* [D][N], nullable */, const double *g_psi2, const double *w_kuu,
                                    const double *g_v, void *ws, size_t ws_bytes, double *d_mu, double *d_s, double *d_z,
                                    double *d_gamma, void *stream);
/* as dpgp_elbo_grad_psi with a full adjoint g_psi1[D][N][Mp] of Psi1 (may be NULL) in place of the rank-1 form
 * g_v[d][a] y[n][d]: then y and g_v may be NULL.  Mixed precision only.  (The over-T model, reference dp_gp_lvm.py:513-676,
 * couples every atom with all columns of y.) */
int dpgp_elbo_grad_psi_ex(int D, int N, int M, int Q, const double *y, int ldy, const double *z, const double *mu,
                          const double *s, const double *gamma, const double *alpha, const double *g_psi2,
                          const double *w_kuu, const double *g_v, const double *g_psi1, int prec, void *ws,
                          size_t ws_bytes, double *d_mu, double *d_s, double *d_z, double *d_gamma, void *stream);

/* ---- Training step: the f_hat terms AND their gradients with respect to mu, s, z, gamma (stage B) and alpha, beta (stage A) in
 * one call — what one Adam iteration of every training script of the reference evaluates (objective + tf.gradients,
 * test/synthetic_data_hard_test.py:143-155; forward src/models/dp_gp_lvm.py:108-145, src/kernels/rbf_kernel.py:135-199).
 * Mixed precision (prec = DPGP_PREC_MIXED, as of the three calls it replaces: dpgp_elbo_fhat_ex + dpgp_elbo_grad_chain +
 * dpgp_elbo_grad_psi; or DPGP_PREC_MIXED_FAST for stage B), M <= 128 (-3), Q <= 21 (-4: the pair-tile form of stage B).  Same results as the three calls within the mixed-precision tolerance; the
 * Psi2 statistic comes out of the first pass of stage B (same exponentials, constant feature), so its exponentials are
 * evaluated twice per step instead of three times — the minimum: Psi2 is needed before the adjoints exist, the observation-side sums
 * after; Psi1^T y likewise comes out of the Psi1 term's adjoint-free pass (its y-weighted constant feature).  exec (may be NULL): with
 * stream_aux / ev_fork / ev_join set and D <= 256 the K_uu branch and stage A run on the second stream beside the image build and
 * chain_b (few output dims leave most of the chip idle); the streams are joined again on every way out.
 *   terms / sums / info / ws: as dpgp_elbo_fhat (ws: dpgp_elbo_workspace_bytes(D,N,M,Q,DPGP_PREC_MIXED));
 *   g_psi2 / w_kuu / g_v / d_alpha_beta / info_grad: as dpgp_elbo_grad_chain (outputs, caller-allocated);
 *   gws: dpgp_elbo_grad_psi_workspace_bytes_ex(D,N,M,Q,DPGP_PREC_MIXED);  d_mu / d_s / d_z / d_gamma: as dpgp_elbo_grad_psi.   */
int dpgp_elbo_step(int D, int N, int M, int Q, const double *y, int ldy, const double *z, const double *mu, const double *s,
                   const double *gamma, const double *alpha, const double *beta, double jitter, int prec, double *terms, double *sums,
                   int *info, void *ws, size_t ws_bytes, double *g_psi2, double *w_kuu, double *g_v, double *d_alpha_beta,
                   int *info_grad, void *gws, size_t gws_bytes, double *d_mu, double *d_s, double *d_z, double *d_gamma,
                   void *stream, const dpgp_exec_t *exec);

/* The two halves of dpgp_elbo_step as calls of their own, for M > 128 (stage A is then composed by the caller from dpgp_potrf_batched /
 * dpgp_trsm_batched / dpgp_gemm_strided_f64, as after dpgp_elbo_fhat_ex): dpgp_elbo_fhat_step = the forward evaluation with Psi2 out of
 * the first pass of stage B (any M; afterwards the forward workspace holds ONE Psi2 slab: slab count 1 instead of
 * dpgp_elbo_workspace_layout's), dpgp_elbo_grad_psi_step = the rest of stage B on the same two workspaces. */
int dpgp_elbo_fhat_step(int D, int N, int M, int Q, const double *y, int ldy, const double *z, const double *mu, const double *s,
                        const double *gamma, const double *alpha, const double *beta, double jitter, double *terms, double *sums,
                        int *info, void *ws, size_t ws_bytes, void *gws, size_t gws_bytes, void *stream, const dpgp_exec_t *exec);
int dpgp_elbo_grad_psi_step(int D, int N, int M, int Q, const double *y, int ldy, const double *z, const double *mu, const double *s,
                            const double *gamma, const double *alpha, const double *g_psi2, const double *w_kuu, const double *g_v,
                            int prec, void *ws, size_t ws_bytes, void *gws, size_t gws_bytes, double *d_mu, double *d_s, double *d_z,
                            double *d_gamma, void *stream);

/* ---- f_hat of the over-T model dp_gp_lvm_t (reference: src/models/dp_gp_lvm.py:608-676; the [T,M,N] x [N,D] contraction at
 * :657-658): T atoms with their own kernel hyper-parameters, every atom coupled to all D columns of y through phit[T,D].
 *   inputs (fp64 device arrays): y[N,ldy], yy[D] = column sums of y^2, z[M,Q], mu[N,Q], s[N,Q], gamma[T,Q], alpha[T], beta[T],
 *     phit: assignment probabilities phi_dt of the D output dims on this GPU, element strides below
 *   outputs: per_t[T] = N/2 log beta_t + beta_t/2 (tr(L^-1 Psi2 L^-T) - alpha_t N) - sum log diag L_A,t,
 *            quad[T,D] = beta_t^2 |L_A,t^-1 L^-1 Psi1_t^T y_d|^2,   sums[2] = { f_hat (of these D output dims), KL(q(X)||p(X)) },
 *            info[T] (as for dpgp_elbo_fhat; a failed atom makes f_hat NaN)
 *   prec: DPGP_PREC_MIXED (Psi2 on the fp32 matrix path) or DPGP_PREC_F64; Psi1, the contraction and the chain are fp64.
 *   M <= 128 and T <= D (-30 / -2 otherwise: the host composes the same value from the operators above).
 *   ws: dpgp_elbo_fhat_t_workspace_bytes(T,D,N,M,Q,prec).  Eleven launches, no host synchronisation.                     */
size_t dpgp_elbo_fhat_t_workspace_bytes(int T, int D, int N, int M, int Q, int prec);
int dpgp_elbo_fhat_t(int T, int D, int N, int M, int Q, const double *y, int ldy, const double *yy, const double *z,
                     const double *mu, const double *s, const double *gamma, const double *alpha, const double *beta,
                     const double *phit, long long phi_st, long long phi_sd, double jitter, int prec, double *per_t,
                     double *quad, double *sums, int *info, void *ws, size_t ws_bytes, void *stream,
                     const double *model_scal, double *model_pack, double *model_out, void *stream_aux, void *ev_fork,
                     void *ev_join);
/*   phit is read as phit[t * phi_st + d * phi_sd] (phi[D,T] of dpgp_model_prepare_t: phi_st = 1, phi_sd = T).
 *   model_scal / model_pack / model_out (each may be NULL): the model-level tail in the last launch, as dpgp_exec_t's fields
 *   of the same names — model_scal = scal of dpgp_model_prepare_t for the same D output dims.
 *   stream_aux / ev_fork / ev_join (all three or none; dpgp_stream_create / dpgp_event_create): Psi1 and the product Psi1^T Y run
 *   on stream_aux beside the fused reduction on the atoms — both are short latency-bound chains at small T.  Ignored while
 *   `stream` is being captured into a graph. */

/* hipEvent helpers for hosts without their own HIP binding */
void *dpgp_event_create(void);
void dpgp_event_destroy(void *event);
void *dpgp_stream_create(void);          /* a non-blocking hipStream_t (dpgp_exec_t.stream_aux) */
void dpgp_stream_destroy(void *stream);
float dpgp_event_elapsed_ms(void *begin, void *end);

/* ---- model-level glue of dp_gp_lvm(...).objective that is O(D T + N Q) (all fp64):
 *   dpgp_model_prepare : from the RAW variational parameters (softplus / softmax parameterisation of utils/types.py:40-57,
 *     dirichlet_process.py:39-59) of the D output dims resident on this GPU (global index d_offset + d; logits row
 *     (d_offset+d)/mask_size) compute  phi[D,T] (optional), gamma[D,Q] = phi gamma_atoms, alpha[D], beta[D]
 *     (dp_gp_lvm.py:100-102), s[N,Q] = softplus(s_raw), and scal[dpgp_model_scal_count(D)]:
 *       scal[0] = D-independent terms of the DP ELBO (dirichlet_process.py:68-77; 0 unless add_constants != 0, i.e. on
 *                 exactly one rank), scal[1] = hyper-prior log-likelihood of the atoms (dp_gp_lvm.py:96-98),
 *       scal[2..] = per-row-block partial sums of E[log p(Z|V)] + H[q(Z)] (dirichlet_process.py:64-66,75).
 *   dpgp_model_pack    : pack[0] = f_hat (from the fused ELBO's sums[0]), pack[1] = this GPU's share of the DP objective
 *                        (= -(sum of scal[0], scal[2..])): the 2-vector that is sum-all-reduced when D is sharded.
 *   dpgp_model_finalize: pack[2] (summed over GPUs), kl[1], hyper[1] ->
 *       out[5] = {objective (dp_gp_lvm.py:154), f_hat, KL, DP objective, hyper-prior}.                               */
int dpgp_model_scal_count(int D);
int dpgp_model_prepare(int D, int T, int Q, int N, int d_offset, int mask_size, const double *logits,
                       const double *gamma_atoms_raw, const double *alpha_atoms_raw, const double *beta_atoms_raw,
                       const double *s_raw, const double *g1_raw, const double *g2_raw, const double *w_raw, double s1,
                       double s2, int add_constants, double *gamma, double *alpha, double *beta, double *s, double *phi,
                       double *scal, void *stream);
/* dpgp_model_prepare for the over-T model: no mixing; outputs s[N,Q], phi[D,T], atoms[T*Q + 2 T] = softplus of the atoms
 * (gamma [T,Q] | alpha [T] | beta [T]) and scal as above. */
int dpgp_model_prepare_t(int D, int T, int Q, int N, int d_offset, int mask_size, const double *logits,
                         const double *gamma_atoms_raw, const double *alpha_atoms_raw, const double *beta_atoms_raw,
                         const double *s_raw, const double *g1_raw, const double *g2_raw, const double *w_raw, double s1,
                         double s2, int add_constants, double *s, double *phi, double *atoms, double *scal, void *stream);
/* The trouble flag of a gradient evaluation: out[0] = 1.0 if any info[0..d) != 0 (failed factorisation / conditioning guard of the
 * forward evaluation) or any of flat[0..n) is not finite, else 0.0 — the value the host-side optimiser loop branches on where the
 * reference's tf.cholesky raises (dp_gp_lvm.py:116,127), reduced over the ranks with the packed gradients.  One launch. */
int dpgp_trouble_flag(size_t n, const double *flat, int d, const int *info, double *out, void *stream);
/* Model-level backward pass (first version): d objective / d (the reference's eleven raw trainable variables,
 * dp_gp_lvm.py:63-94, dirichlet_process.py:40-59) from d f_hat / d (mu, S, z, gamma, alpha, beta) of dpgp_elbo_grad_chain +
 * dpgp_elbo_grad_psi, for the D output dims resident on this GPU.  phi[D,T]: as written by dpgp_model_prepare.  Outputs are
 * PARTIAL over this GPU's output dims, the D-independent terms being added iff add_constants (exactly one rank): a
 * sum-all-reduce of the outputs is the gradient.  d_logits[logits_rows][T] is zero outside the rows of the local dims.  */
int dpgp_model_backward(int D, int T, int Q, int N, int M, int d_offset, int mask_size, int logits_rows,
                        const double *logits, const double *gamma_atoms_raw, const double *alpha_atoms_raw,
                        const double *beta_atoms_raw, const double *s_raw, const double *g1_raw, const double *g2_raw,
                        const double *w_raw, const double *x_mean, const double *phi, double s1, double s2,
                        int add_constants, const double *df_dmu, const double *df_ds, const double *df_dz,
                        const double *df_dgamma, const double *df_dalpha_beta, double *d_x_mean, double *d_s_raw,
                        double *d_x_u, double *d_logits, double *d_g1_raw, double *d_g2_raw, double *d_w_raw,
                        double *d_gamma_atoms_raw, double *d_alpha_atoms_raw, double *d_beta_atoms_raw, void *stream);
/* the same for the over-T model dp_gp_lvm_t (reference src/models/dp_gp_lvm.py:513-676: the kernel batch is the T atoms, phi enters f_hat
 * directly): df_dgamma_atoms [T][Q] and df_dalpha_beta_atoms [T][2] are d f_hat / d (softplus'd atoms) themselves, df_dphi [D][T] is
 * d f_hat / d phi of the D output dims on this GPU.  Everything else as dpgp_model_backward. */
int dpgp_model_backward_t(int D, int T, int Q, int N, int M, int d_offset, int mask_size, int logits_rows, const double *logits,
                          const double *gamma_atoms_raw, const double *alpha_atoms_raw, const double *beta_atoms_raw,
                          const double *s_raw, const double *g1_raw, const double *g2_raw, const double *w_raw,
                          const double *x_mean, const double *phi, double s1, double s2, int add_constants, const double *df_dmu,
                          const double *df_ds, const double *df_dz, const double *df_dgamma_atoms,
                          const double *df_dalpha_beta_atoms, const double *df_dphi, double *d_x_mean, double *d_s_raw,
                          double *d_x_u, double *d_logits, double *d_g1_raw, double *d_g2_raw, double *d_w_raw,
                          double *d_gamma_atoms_raw, double *d_alpha_atoms_raw, double *d_beta_atoms_raw, void *stream);
int dpgp_model_pack(int D, const double *fhat, const double *scal, double *pack, void *stream);
int dpgp_model_finalize(const double *pack, const double *kl, const double *hyper, double *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DPGP_H */
