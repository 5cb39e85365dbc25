// Psi statistics of a test-point q(X*) and their adjoint, for B ARD-RBF kernels that each have their own inducing inputs
// (the prediction paths of bayesian_gp_lvm and manifold_relevance_determination; reference rbf_kernel.py:135-199).
// Kernel b: z_b [M][Q], gamma_b [Q], alpha_b; shared q(X*): mu [N][Q], s [N][Q] (diagonal variances).
//   w1_nq = gamma_q s_nq + 1,  w2_nq = 2 gamma_q s_nq + 1,  iw1 = gamma / w1,  iw2 = gamma / w2
//   Psi1[b,n,m]  = alpha prod_q w1^-1/2 exp(-1/2 sum_q iw1_q (mu_nq - z_mq)^2)
//   Psi2[b,m,m'] = sum_n F[b,m,m'] c2_n exp(-sum_q iw2_q (mu_nq - zbar_q)^2),   zbar = (z_m + z_m') / 2,
//                  F = alpha^2 exp(-1/4 sum_q gamma_q (z_mq - z_m'q)^2)  (the pair factor: constant while Z is frozen),
//                  c2_n = prod_q w2_nq^-1/2.
// The adjoint contracts G1 = dF/dPsi1 and G2 = dF/dPsi2 with the derivatives of Psi1 / Psi2 with respect to (mu, s):
//   per (n, q), with d = mu - z_m (Psi1) or mu - zbar (Psi2) and A = G2-weighted Psi2 term of test point n:
//   d_mu = -iw1 sum_m G1 Psi1 d - 2 iw2 sum_pairs A d
//   d_s  = 1/2 iw1^2 sum_m G1 Psi1 d^2 - 1/2 iw1 sum_m G1 Psi1 + 2 iw2^2 sum_pairs A d^2 - iw2 sum_pairs A
// d is formed directly (no mu^2 - 2 mu zbar + zbar^2 expansion, which cancels for points far from the inducing inputs).
//
// Layouts.  Pairs are visited as 32 x 32 tiles (I, J), I <= J, of the upper block triangle; a pair m < m' is visited once and
// weighted by G2[m,m'] + G2[m',m] (exact for any G2), the diagonal by G2[m,m].
//   stats:   workgroup (pair tile, n slab, b), 256 threads = 32 columns x 8 row groups, 4 rows each; the n of the slab are
//            staged 32 at a time; partial Psi2 tiles go to slab s of the workspace, a second launch adds the slabs in slab
//            order and writes both triangles.  Psi1: one thread per (b, n, m), its own launch.
//   adjoint: workgroup (64 test points, pair slab, (b, q chunk)), one wave: lane = test point.  LDS holds mu, iw1, iw2 of the
//            64 points [Q][64], the tile's z rows / columns [32][Q] and the weighted pair factor H [32][33] of the tile (G2 and
//            F, so the per-pair, per-point work is one exponential);  2048 Q + 8448 bytes (139.5 KiB at Q = 64, the bound).
//            A lane keeps the accumulators of one chunk of up to 8 latent dims in registers; the exponent runs over all Q.
//            The Psi1 term is evaluated by the workgroup whose slab holds the diagonal tile of the column block.  Partial
//            (d_mu, d_s) go to slab [slab][b]; a second launch adds them in b order, then slab order.
//   parameter adjoint (d/dz_b, d/dgamma_b, d/dalpha_b per kernel b; the closed forms are in include/dpgp.h): the outputs reduce
//            over n, so the Psi2 term has the stats kernel's layout: workgroup (pair tile, n slab, (b, chunk of 4 latent dims)),
//            256 threads = 32 columns x 8 row groups, 4 pairs each, the slab's points staged 32 at a time as [32][Q][4] =
//            (mu, gamma / w2, 1 / w2, s / w2).  Per (point, pair): one exponential over all Q, then for the chunk's dims
//            sum a d2 / w2 and sum a (s / w2 + d2^2 / w2^2) in registers (a = weighted pair factor x c2_n x exp).  At the end the
//            tile's pairs give, per dim, a row-side and a column-side d_z sum (through two [32][33] LDS tiles, added in index
//            order) and a block-wide d_gamma / d_alpha sum (a fixed binary tree), written to the cell (slab, b, tile) of the
//            workspace.  The Psi1 term is its own launch: workgroup (32 inducing points, n slab, b); per step a1 = g1 Psi1
//            [32][33] with one exponential per (n, m), then the items (m, q) add over the step's points into LDS accumulators.
//            A last launch adds the cells in a fixed order.  The z tiles have the odd row stride Q | 1 (lane = column reads).
// No atomics anywhere: the same inputs give the same bits.
//
// Weighted forms (per-entry observation masks): wt [B][N] multiplies test point n's Psi2 term of kernel b (c2_n in both
// kernels); Psi1 and its adjoint are not weighted.  The kernels are templated on WEIGHTED: the unweighted instantiations
// are the code of the unweighted entry points, and wt == NULL runs them.  A point of weight 0 costs no exponential: the
// stats kernel skips it in its staged-point loop (a workgroup-uniform branch on the staged weight), the adjoint skips a
// tile's pair loop when all 64 points of the wave have weight 0 for kernel b.  Either way its contribution is exactly 0.
// The parameter adjoint skips a point of weight 0 as the stats kernel does, on its staged weight; its Psi1 term is not weighted.
#include "internal.h"
#include "qx_tile.h"

#define QP_TILE 32
#define QP_HSTRIDE (QP_TILE + 1)
#define QP_NT 64           // test points per adjoint workgroup (one wave)
#define QP_SN 32           // test points staged per step of the stats kernel
#define QP_QCHUNK 8        // latent dims per adjoint accumulator chunk
#define QP_PCHUNK 4        // latent dims per parameter-adjoint accumulator chunk
#define QP_TARGET_WGS 1024

namespace {

int qp_tiles(int M) { const int t = dpgp_ceil_div(M, QP_TILE); return t * (t + 1) / 2; }

// pair factor F[m][m'] (alpha^2 exp(-1/4 sum gamma dz^2)), from zfac when given
__device__ __forceinline__ double qp_pair_factor(const double *zfac, size_t b, int M, int Q, int m, int mp, const double *zm,
                                                 const double *zmp, const double *gm, double al) {
    if (zfac) return zfac[(b * M + m) * M + mp];
    double e = 0.0;
    for (int q = 0; q < Q; ++q) {
        const double d = zm[q] - zmp[q];
        e = fma(gm[q] * d, d, e);
    }
    return al * al * exp(-0.25 * e);
}

// ---- Psi1: one thread per (n, m) of kernel b = blockIdx.y
__global__ __launch_bounds__(256) void qp_psi1_kernel(int N, int M, int Q, const double *__restrict__ z,
                                                      const double *__restrict__ mu, const double *__restrict__ s,
                                                      const double *__restrict__ gamma, const double *__restrict__ alpha,
                                                      double *__restrict__ psi1) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)N * M) return;
    const int b = blockIdx.y, n = (int)(e / M), m = (int)(e % M);
    const double *g = gamma + (size_t)b * Q, *zm = z + ((size_t)b * M + m) * Q, *mn = mu + (size_t)n * Q, *sn = s + (size_t)n * Q;
    double acc = 0.0;
    for (int q = 0; q < Q; ++q) {                                   // (rbf_kernel.py:155-159, the log form)
        const double den = fma(g[q], sn[q], 1.0), d = mn[q] - zm[q];
        acc += g[q] * d * d / den + log(den);
    }
    psi1[(size_t)b * N * M + e] = alpha[b] * exp(-0.5 * acc);
}

// ---- Psi2 partial tiles: (pair tile, n slab, b); WEIGHTED: sc2 carries wt[b][n] c2_n and a zero skips the point
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void qp_psi2_kernel(int N, int M, int Q, int T, int n_per_slab, const double *__restrict__ z,
                                                      const double *__restrict__ mu, const double *__restrict__ s,
                                                      const double *__restrict__ gamma, const double *__restrict__ alpha,
                                                      const double *__restrict__ zfac, const double *__restrict__ wt,
                                                      double *__restrict__ part) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *smu = reinterpret_cast<double *>(smem_raw);    // [QP_SN][Q]
    double *siw = smu + (size_t)QP_SN * Q;                  // [QP_SN][Q]
    double *sc2 = siw + (size_t)QP_SN * Q;                  // [QP_SN]
    double *zr = sc2 + QP_SN;                               // [32][Q] rows of block I
    double *zc = zr + (size_t)QP_TILE * Q;                  // [32][Q] columns of block J
    double *gm = zc + (size_t)QP_TILE * Q;                  // [Q]
    const int t = threadIdx.x, b = blockIdx.z, slab = blockIdx.y;
    int I, J;
    dpgp_tile_ij(blockIdx.x, T, I, J);
    const int m0 = I * QP_TILE, c0 = J * QP_TILE;
    const double *zb = z + (size_t)b * M * Q;
    for (int k = t; k < QP_TILE * Q; k += 256) {
        const int r = k / Q, q = k % Q;
        zr[k] = m0 + r < M ? zb[(size_t)(m0 + r) * Q + q] : 0.0;
        zc[k] = c0 + r < M ? zb[(size_t)(c0 + r) * Q + q] : 0.0;
    }
    for (int q = t; q < Q; q += 256) gm[q] = gamma[(size_t)b * Q + q];
    const double al = alpha[b];
    const int c = t & 31, rg = t >> 5;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int n_lo = slab * n_per_slab, n_hi = min(N, n_lo + n_per_slab);
    for (int nb = n_lo; nb < n_hi; nb += QP_SN) {
        const int nn = min(QP_SN, n_hi - nb);
        __syncthreads();                                       // (previous step done with smu / siw / sc2)
        for (int k = t; k < nn * Q; k += 256) {
            const int i = k / Q, q = k % Q;
            const double g = gamma[(size_t)b * Q + q], w2 = fma(2.0 * g, s[(size_t)(nb + i) * Q + q], 1.0);
            smu[k] = mu[(size_t)(nb + i) * Q + q];
            siw[k] = g / w2;
        }
        if (t < nn) {
            const double wn = WEIGHTED ? wt[(size_t)b * N + nb + t] : 1.0;
            if (WEIGHTED && wn == 0.0) {
                sc2[t] = 0.0;
            } else {
                double l = 0.0;
                for (int q = 0; q < Q; ++q) l += log(fma(2.0 * gamma[(size_t)b * Q + q], s[(size_t)(nb + t) * Q + q], 1.0));
                sc2[t] = WEIGHTED ? wn * exp(-0.5 * l) : exp(-0.5 * l);
            }
        }
        __syncthreads();
        for (int i = 0; i < nn; ++i) {
            if (WEIGHTED && sc2[i] == 0.0) continue;           // (the same LDS word for every thread: uniform)
            const double *mi = smu + (size_t)i * Q, *wi = siw + (size_t)i * Q;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = rg + 8 * k;
                double e = 0.0;
                for (int q = 0; q < Q; ++q) {
                    const double d = mi[q] - 0.5 * (zr[r * Q + q] + zc[c * Q + q]);
                    e = fma(wi[q] * d, d, e);
                }
                acc[k] = fma(sc2[i], exp(-e), acc[k]);
            }
        }
    }
    const int mp = c0 + c;
    if (mp >= M) return;
    double *pb = part + ((size_t)slab * gridDim.z + b) * M * M;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int m = m0 + rg + 8 * k;
        if (m < M) pb[(size_t)m * M + mp] = acc[k] * qp_pair_factor(zfac, b, M, Q, m, mp, zr + (size_t)(rg + 8 * k) * Q,
                                                                     zc + (size_t)c * Q, gm, al);
    }
}

// out[b][m][m'] = sum over slabs of the partial of (min, max): both triangles from the one visited pair
__global__ __launch_bounds__(256) void qp_psi2_reduce_kernel(int B, int M, int slabs, const double *__restrict__ part,
                                                             double *__restrict__ psi2) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)B * M * M) return;
    const int b = (int)(e / ((size_t)M * M));
    const int r = (int)(e % ((size_t)M * M)), m = r / M, mp = r % M;
    const size_t off = (size_t)b * M * M + (size_t)min(m, mp) * M + max(m, mp);
    double acc = 0.0;
    for (int k = 0; k < slabs; ++k) acc += part[(size_t)k * B * M * M + off];
    psi2[e] = acc;
}

// ---- adjoint partials: (64 test points, pair slab, b * qchunks + chunk); KQ: the chunk's register width
template <int KQ, bool WEIGHTED>
__global__ __launch_bounds__(64) void qp_adjoint_kernel(int B, int N, int M, int Q, int T, int tiles_per_slab,
                                                        const double *__restrict__ z, const double *__restrict__ mu,
                                                        const double *__restrict__ s, const double *__restrict__ gamma,
                                                        const double *__restrict__ alpha, const double *__restrict__ zfac,
                                                        const double *__restrict__ wt, const double *__restrict__ g1,
                                                        const double *__restrict__ g2, double *__restrict__ part) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *smu = reinterpret_cast<double *>(smem_raw);    // [Q][64]
    double *siw1 = smu + (size_t)Q * QP_NT;                 // [Q][64]
    double *siw2 = siw1 + (size_t)Q * QP_NT;                // [Q][64]
    double *zr = siw2 + (size_t)Q * QP_NT;                  // [32][Q]
    double *zc = zr + (size_t)QP_TILE * Q;                  // [32][Q]
    double *hs = zc + (size_t)QP_TILE * Q;                  // [32][33] weighted pair factor
    double *gm = hs + QP_TILE * QP_HSTRIDE;                 // [Q]
    const int lane = threadIdx.x, slab = blockIdx.y;
    const int qchunks = (Q + QP_QCHUNK - 1) / QP_QCHUNK;
    const int b = blockIdx.z / qchunks, q0 = (blockIdx.z % qchunks) * QP_QCHUNK;
    const int nq = min(QP_QCHUNK, Q - q0);
    const int n = blockIdx.x * QP_NT + lane;
    const bool live = n < N;
    const double al = alpha[b];
    const double *gb = gamma + (size_t)b * Q;
    const double *zb = z + (size_t)b * M * Q;
    for (int q = lane; q < Q; q += QP_NT) gm[q] = gb[q];
    double l1 = 0.0, l2 = 0.0;
    for (int q = 0; q < Q; ++q) {
        const double g = gb[q], sv = live ? s[(size_t)n * Q + q] : 1.0;
        const double w1 = fma(g, sv, 1.0), w2 = fma(2.0 * g, sv, 1.0);
        smu[q * QP_NT + lane] = live ? mu[(size_t)n * Q + q] : 0.0;
        siw1[q * QP_NT + lane] = g / w1;
        siw2[q * QP_NT + lane] = g / w2;
        l1 += log(w1);
        l2 += log(w2);
    }
    const double wn = WEIGHTED ? (live ? wt[(size_t)b * N + n] : 0.0) : 1.0;
    const double c1 = al * exp(-0.5 * l1), c2 = WEIGHTED ? wn * exp(-0.5 * l2) : exp(-0.5 * l2);
    const bool pairs = !WEIGHTED || __any(wn != 0.0);          // the workgroup is one wave: uniform
    double mk[KQ], i1[KQ], i2[KQ], s1[KQ], s2[KQ], t1[KQ], t2[KQ], dk[KQ];
    double s0 = 0.0, t0 = 0.0;
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
        const bool on = k < nq;
        mk[k] = on ? smu[(q0 + k) * QP_NT + lane] : 0.0;
        i1[k] = on ? siw1[(q0 + k) * QP_NT + lane] : 0.0;
        i2[k] = on ? siw2[(q0 + k) * QP_NT + lane] : 0.0;
        s1[k] = s2[k] = t1[k] = t2[k] = dk[k] = 0.0;
    }
    const bool one = nq == Q;                                  // the chunk is every latent dim: exponent from registers
    const int tile_lo = slab * tiles_per_slab, tile_hi = min(T * (T + 1) / 2, tile_lo + tiles_per_slab);
    for (int tile = tile_lo; tile < tile_hi; ++tile) {
        int I, J;
        dpgp_tile_ij(tile, T, I, J);
        if (WEIGHTED && !pairs && I != J) continue;            // every weight of the wave is 0 and no Psi1 term here
        const int m0 = I * QP_TILE, c0 = J * QP_TILE;
        const int nr = min(QP_TILE, M - m0), nc = min(QP_TILE, M - c0);
        __syncthreads();                                       // (previous tile done with zr / zc / hs)
        for (int k = lane; k < QP_TILE * Q; k += QP_NT) {
            const int r = k / Q, q = k % Q;
            zr[k] = r < nr ? zb[(size_t)(m0 + r) * Q + q] : 0.0;
            zc[k] = r < nc ? zb[(size_t)(c0 + r) * Q + q] : 0.0;
        }
        __syncthreads();
        const double *g2b = g2 + (size_t)b * M * M;
        for (int k = lane; k < QP_TILE * QP_TILE; k += QP_NT) {
            const int r = k / QP_TILE, cc = k % QP_TILE, m = m0 + r, mp = c0 + cc;
            double h = 0.0;
            if (r < nr && cc < nc && (I != J || cc >= r)) {
                const double w = m == mp ? g2b[(size_t)m * M + m] : g2b[(size_t)m * M + mp] + g2b[(size_t)mp * M + m];
                h = w * qp_pair_factor(zfac, b, M, Q, m, mp, zr + (size_t)r * Q, zc + (size_t)cc * Q, gm, al);
            }
            hs[r * QP_HSTRIDE + cc] = h;
        }
        __syncthreads();
        // Psi2 term over the tile's pairs (uniform over the wave: every lane visits the same pair)
        for (int r = 0; r < (pairs ? nr : 0); ++r) {
            const double *zrr = zr + (size_t)r * Q;
            for (int cc = (I == J ? r : 0); cc < nc; ++cc) {
                const double h = hs[r * QP_HSTRIDE + cc];
                const double *zcc = zc + (size_t)cc * Q;
                double e = 0.0;
                if (one) {
#pragma unroll
                    for (int k = 0; k < KQ; ++k)
                        if (k < nq) {
                            dk[k] = mk[k] - 0.5 * (zrr[k] + zcc[k]);
                            e = fma(i2[k] * dk[k], dk[k], e);
                        }
                } else {
                    for (int q = 0; q < Q; ++q) {
                        const double d = smu[q * QP_NT + lane] - 0.5 * (zrr[q] + zcc[q]);
                        e = fma(siw2[q * QP_NT + lane] * d, d, e);
                    }
#pragma unroll
                    for (int k = 0; k < KQ; ++k)
                        if (k < nq) dk[k] = mk[k] - 0.5 * (zrr[q0 + k] + zcc[q0 + k]);
                }
                const double a = h * c2 * exp(-e);
                s0 += a;
#pragma unroll
                for (int k = 0; k < KQ; ++k) {
                    const double ad = a * dk[k];
                    s1[k] += ad;
                    s2[k] = fma(ad, dk[k], s2[k]);
                }
            }
        }
        // Psi1 term of the column block: evaluated with the diagonal tile
        if (I == J && live) {
            const double *g1n = g1 + ((size_t)b * N + n) * M;
            for (int r = 0; r < nr; ++r) {
                const double *zrr = zr + (size_t)r * Q;
                double e = 0.0;
                if (one) {
#pragma unroll
                    for (int k = 0; k < KQ; ++k)
                        if (k < nq) {
                            dk[k] = mk[k] - zrr[k];
                            e = fma(i1[k] * dk[k], dk[k], e);
                        }
                } else {
                    for (int q = 0; q < Q; ++q) {
                        const double d = smu[q * QP_NT + lane] - zrr[q];
                        e = fma(siw1[q * QP_NT + lane] * d, d, e);
                    }
#pragma unroll
                    for (int k = 0; k < KQ; ++k)
                        if (k < nq) dk[k] = mk[k] - zrr[q0 + k];
                }
                const double a = g1n[m0 + r] * c1 * exp(-0.5 * e);
                t0 += a;
#pragma unroll
                for (int k = 0; k < KQ; ++k) {
                    const double ad = a * dk[k];
                    t1[k] += ad;
                    t2[k] = fma(ad, dk[k], t2[k]);
                }
            }
        }
    }
    if (!live) return;
    // part[((slab * B + b) * 2 + {0: d_mu, 1: d_s}) * Q + q][n]
    double *pb = part + ((size_t)slab * B + b) * 2 * Q * N;
#pragma unroll
    for (int k = 0; k < KQ; ++k)
        if (k < nq) {
            const int q = q0 + k;
            pb[(size_t)q * N + n] = -i1[k] * t1[k] - 2.0 * i2[k] * s1[k];
            pb[((size_t)Q + q) * N + n] = 0.5 * i1[k] * (i1[k] * t2[k] - t0) + i2[k] * (2.0 * i2[k] * s2[k] - s0);
        }
}

// d_mu[n][q], d_s[n][q]: the partials added in b order, then slab order
__global__ __launch_bounds__(256) void qp_adjoint_reduce_kernel(int B, int N, int Q, int slabs, const double *__restrict__ part,
                                                                double *__restrict__ d_mu, double *__restrict__ d_s) {
    const size_t per = (size_t)2 * Q * N;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    double acc = 0.0;
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < slabs; ++k) acc += part[((size_t)k * B + b) * per + e];
    const int kq = (int)(e / N), n = (int)(e % N);
    if (kq < Q) d_mu[(size_t)n * Q + kq] = acc;
    else d_s[(size_t)n * Q + (kq - Q)] = acc;
}

// ---- parameter adjoint, Psi2 term: (pair tile, n slab, b * qchunks + chunk); layout in the header comment
// sum of v over the 256 threads of the workgroup, added as a fixed binary tree in LDS (red [256])
__device__ __forceinline__ double qp_block_sum(double v, double *red, int t) {
    red[t] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

template <int KQ, bool WEIGHTED>
__global__ __launch_bounds__(256) void qp_param_kernel(int B, int N, int M, int Q, int T, int n_per_slab,
                                                       const double *__restrict__ z, const double *__restrict__ mu,
                                                       const double *__restrict__ s, const double *__restrict__ gamma,
                                                       const double *__restrict__ alpha, const double *__restrict__ zfac,
                                                       const double *__restrict__ wt, const double *__restrict__ g2,
                                                       double *__restrict__ part) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int ZS = Q | 1;                                   // odd row stride of the z tiles: lane = column reads hit 32 banks
    double *sp = reinterpret_cast<double *>(smem_raw);    // staged points [QP_SN][Q][4]: mu, gamma / w2, 1 / w2, s / w2
    double *sc = sp + (size_t)QP_SN * Q * 4;                // [QP_SN] wt c2_n
    double *zt = sc + QP_SN;                                // [64][ZS]: rows of block I, then columns of block J
    double *gm = zt + (size_t)2 * QP_TILE * ZS;             // [Q]
    double *buf = gm + Q;                                   // [2][32][33] row- and column-side d_z terms, then [256]
    const int t = threadIdx.x, slab = blockIdx.y;
    const int qchunks = (Q + QP_PCHUNK - 1) / QP_PCHUNK;
    const int b = blockIdx.z / qchunks, q0 = (blockIdx.z % qchunks) * QP_PCHUNK;
    const int nq = min(QP_PCHUNK, Q - q0);
    int I, J;
    dpgp_tile_ij(blockIdx.x, T, I, J);
    const bool diag = I == J;
    const int m0 = I * QP_TILE, c0 = J * QP_TILE;
    {
        const double *zb = z + (size_t)b * M * Q;
        for (int k = t; k < QP_TILE * Q; k += 256) {
            const int r = k / Q, q = k % Q;
            zt[r * ZS + q] = m0 + r < M ? zb[(size_t)(m0 + r) * Q + q] : 0.0;
            zt[(QP_TILE + r) * ZS + q] = c0 + r < M ? zb[(size_t)(c0 + r) * Q + q] : 0.0;
        }
        for (int q = t; q < Q; q += 256) gm[q] = gamma[(size_t)b * Q + q];
    }
    const int c = t & 31, rg = t >> 5;
    const double *zcc = zt + (size_t)(QP_TILE + c) * ZS;     // the thread's column
    const double *zr0 = zt + (size_t)rg * ZS;                // its rows: zr0 + 8 k ZS
    __syncthreads();
    // weighted pair factor of the thread's four pairs: (G2[m,m'] + G2[m',m]) F off the diagonal, G2[m,m] F on it, 0 for a
    // pair that is out of range or below the diagonal of a diagonal tile (such a pair then adds exact zeros everywhere)
    double h[4];
    {
        const double *g2b = g2 + (size_t)b * M * M;
        const double al = alpha[b];
        const int mp = c0 + c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = rg + 8 * k, m = m0 + r;
            h[k] = 0.0;
            if (m < M && mp < M && (!diag || c >= r)) {
                const double w = m == mp ? g2b[(size_t)m * M + m] : g2b[(size_t)m * M + mp] + g2b[(size_t)mp * M + m];
                h[k] = w * qp_pair_factor(zfac, b, M, Q, m, mp, zr0 + (size_t)8 * k * ZS, zcc, gm, al);
            }
        }
    }
    double p0[4], p1[4][KQ], p2[4][KQ];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        p0[k] = 0.0;
#pragma unroll
        for (int kk = 0; kk < KQ; ++kk) p1[k][kk] = p2[k][kk] = 0.0;
    }
    const int n_hi = min(N, (slab + 1) * n_per_slab);
    for (int nb = slab * n_per_slab; nb < n_hi; nb += QP_SN) {
        const int nn = min(QP_SN, n_hi - nb);
        __syncthreads();                                       // (previous step done with the staged points)
        for (int k = t; k < nn * Q; k += 256) {
            const int q = k % Q;
            const double g = gm[q], sv = s[(size_t)nb * Q + k];
            const double i2 = 1.0 / fma(2.0 * g, sv, 1.0);
            sp[4 * k] = mu[(size_t)nb * Q + k];
            sp[4 * k + 1] = g * i2;
            sp[4 * k + 2] = i2;
            sp[4 * k + 3] = sv * i2;
        }
        if (t < nn) {
            const double wn = WEIGHTED ? wt[(size_t)b * N + nb + t] : 1.0;
            const double *sn = s + (size_t)(nb + t) * Q;
            if (WEIGHTED && wn == 0.0) {
                sc[t] = 0.0;
            } else {
                double l = 0.0;
                for (int q = 0; q < Q; ++q) l += log(fma(2.0 * gm[q], sn[q], 1.0));
                sc[t] = WEIGHTED ? wn * exp(-0.5 * l) : exp(-0.5 * l);
            }
        }
        __syncthreads();
        // Psi2 term: one exponential per (point, pair), then the chunk's accumulators
        for (int i = 0; i < nn; ++i) {
            const double c2 = sc[i];
            if (WEIGHTED && c2 == 0.0) continue;               // (the same LDS word for every thread: uniform)
            const double *pi = sp + (size_t)i * Q * 4;
            double a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double *zrr = zr0 + (size_t)8 * k * ZS;
                double e = 0.0;
                for (int q = 0; q < Q; ++q) {
                    const double d = pi[4 * q] - 0.5 * (zrr[q] + zcc[q]);
                    e = fma(pi[4 * q + 1] * d, d, e);
                }
                a[k] = h[k] * c2 * exp(-e);
                p0[k] += a[k];
            }
#pragma unroll
            for (int kk = 0; kk < KQ; ++kk)
                if (kk < nq) {
                    const int q = q0 + kk;
                    const double mq = pi[4 * q], iv = pi[4 * q + 2], rs = pi[4 * q + 3], zcq = zcc[q];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const double di = (mq - 0.5 * (zr0[8 * k * ZS + q] + zcq)) * iv;
                        p1[k][kk] = fma(a[k], di, p1[k][kk]);
                        p2[k][kk] = fma(a[k], fma(di, di, rs), p2[k][kk]);
                    }
                }
        }
    }
    // tile-level sums in a fixed order, one latent dim at a time; cell of the workspace: [2][32][Q] d_z sides, [Q], [1]
    double *pz = part + (((size_t)slab * B + b) * gridDim.x + blockIdx.x) * ((size_t)2 * QP_TILE * Q + Q + 1);
    double *bufb = buf + QP_TILE * QP_HSTRIDE, *red = bufb + QP_TILE * QP_HSTRIDE;
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk)
        if (kk < nq) {                                         // (uniform)
            const int q = q0 + kk;
            const double gq = gm[q];
            double gv = 0.0;
            __syncthreads();                                   // (previous dim's sums read)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = rg + 8 * k;
                const double dz = zr0[8 * k * ZS + q] - zcc[q];
                const double u = gq * p1[k][kk], hd = 0.5 * gq * dz * p0[k];
                buf[r * QP_HSTRIDE + c] = u - hd;
                bufb[r * QP_HSTRIDE + c] = u + hd;
                gv -= fma(0.25 * dz * dz, p0[k], p2[k][kk]);
            }
            __syncthreads();
            if (t < 32) {
                double acc = 0.0;
                for (int cc = 0; cc < QP_TILE; ++cc) acc += buf[t * QP_HSTRIDE + cc];
                pz[(size_t)t * Q + q] = acc;
            } else if (t < 64) {
                double acc = 0.0;
                for (int r = 0; r < QP_TILE; ++r) acc += bufb[r * QP_HSTRIDE + (t - 32)];
                pz[(size_t)t * Q + q] = acc;
            }
            const double tot = qp_block_sum(gv, red, t);
            if (t == 0) pz[(size_t)2 * QP_TILE * Q + q] = tot;
        }
    if (q0 == 0) {                                             // alpha: 2 <g2, Psi2>, by the first chunk
        const double tot = qp_block_sum(2.0 * ((p0[0] + p0[1]) + (p0[2] + p0[3])), red, t);
        if (t == 0) pz[(size_t)2 * QP_TILE * Q + Q] = tot;
    }
}

// ---- parameter adjoint, Psi1 term: (block of 32 inducing points, n slab, b).  Per step of 32 staged points the threads
// (inducing point c, points rg + 8 j) form a1 = g1 Psi1 [32][33] with one exponential each, then the items (m, q) of the block
// (thread t owns t, t + 256, ..) add a1 d / w1 and a1 (s / w1 + d^2 / w1^2) over the step's points into their LDS accumulators
__global__ __launch_bounds__(256) void qp_param_psi1_kernel(int B, int N, int M, int Q, int n_per_slab, const double *__restrict__ z,
                                                            const double *__restrict__ mu, const double *__restrict__ s,
                                                            const double *__restrict__ gamma, const double *__restrict__ alpha,
                                                            const double *__restrict__ g1, double *__restrict__ part) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int ZS = Q | 1;
    double *sp = reinterpret_cast<double *>(smem_raw);    // staged points [QP_SN][Q][3]: mu, 1 / w1, s / w1
    double *sc = sp + (size_t)QP_SN * Q * 3;                // [QP_SN] alpha c1_n
    double *zt = sc + QP_SN;                                // [32][ZS]
    double *gm = zt + (size_t)QP_TILE * ZS;                 // [Q]
    double *sa = gm + Q;                                    // [QP_SN][33] a1 of the step
    double *acc1 = sa + QP_SN * QP_HSTRIDE;                 // [32][Q]
    double *acc2 = acc1 + (size_t)QP_TILE * Q;              // [32][Q]
    double *red = acc2 + (size_t)QP_TILE * Q;               // [256]
    const int t = threadIdx.x, slab = blockIdx.y, b = blockIdx.z, m0 = blockIdx.x * QP_TILE;
    const double *zb = z + (size_t)b * M * Q;
    for (int k = t; k < QP_TILE * Q; k += 256) {
        const int r = k / Q, q = k % Q;
        zt[r * ZS + q] = m0 + r < M ? zb[(size_t)(m0 + r) * Q + q] : 0.0;
        acc1[k] = acc2[k] = 0.0;
    }
    for (int q = t; q < Q; q += 256) gm[q] = gamma[(size_t)b * Q + q];
    const int c = t & 31, rg = t >> 5;
    const double *zcc = zt + (size_t)c * ZS;
    double t0 = 0.0;
    const int n_hi = min(N, (slab + 1) * n_per_slab);
    for (int nb = slab * n_per_slab; nb < n_hi; nb += QP_SN) {
        const int nn = min(QP_SN, n_hi - nb);
        __syncthreads();                                       // (previous step done with the staged points and a1)
        for (int k = t; k < nn * Q; k += 256) {
            const double sv = s[(size_t)nb * Q + k], i1 = 1.0 / fma(gm[k % Q], sv, 1.0);
            sp[3 * k] = mu[(size_t)nb * Q + k];
            sp[3 * k + 1] = i1;
            sp[3 * k + 2] = sv * i1;
        }
        if (t < nn) {
            const double *sn = s + (size_t)(nb + t) * Q;
            double l = 0.0;
            for (int q = 0; q < Q; ++q) l += log(fma(gm[q], sn[q], 1.0));
            sc[t] = alpha[b] * exp(-0.5 * l);
        }
        __syncthreads();
        for (int i = rg; i < nn; i += 8) {
            double a1 = 0.0;
            if (m0 + c < M) {
                const double *pi = sp + (size_t)i * Q * 3;
                double e = 0.0;
                for (int q = 0; q < Q; ++q) {
                    const double d = pi[3 * q] - zcc[q];
                    e = fma(gm[q] * pi[3 * q + 1] * d, d, e);
                }
                a1 = g1[((size_t)b * N + nb + i) * M + m0 + c] * sc[i] * exp(-0.5 * e);
            }
            sa[i * QP_HSTRIDE + c] = a1;
            t0 += a1;
        }
        __syncthreads();
        for (int k = t; k < QP_TILE * Q; k += 256) {
            const int r = k / Q, q = k % Q;
            const double zq = zt[r * ZS + q];
            double u1 = 0.0, u2 = 0.0;
            for (int i = 0; i < nn; ++i) {
                const double *pq = sp + ((size_t)i * Q + q) * 3;
                const double a1 = sa[i * QP_HSTRIDE + r], di = (pq[0] - zq) * pq[1];
                u1 = fma(a1, di, u1);
                u2 = fma(a1, fma(di, di, pq[2]), u2);
            }
            acc1[k] += u1;
            acc2[k] += u2;
        }
    }
    __syncthreads();
    // cell of the workspace: [32][Q] d_z, [Q] d_gamma, [1] <g1, Psi1>
    double *pz = part + (((size_t)slab * B + b) * gridDim.x + blockIdx.x) * ((size_t)QP_TILE * Q + Q + 1);
    for (int k = t; k < QP_TILE * Q; k += 256) pz[k] = gm[k % Q] * acc1[k];
    for (int q = t; q < Q; q += 256) {
        double a = 0.0;
        for (int r = 0; r < QP_TILE; ++r) a += acc2[r * Q + q];
        pz[(size_t)QP_TILE * Q + q] = -0.5 * a;
    }
    const double tot = qp_block_sum(t0, red, t);
    if (t == 0) pz[(size_t)QP_TILE * Q + Q] = tot;
}

// d_z[b][m][q]: over slabs, the column sides of the tiles (I, block of m), I ascending, then the row sides of the tiles
// (block of m, J), J ascending, then the Psi1 slabs; d_gamma[b][q] and d_alpha[b]: over slabs, then tiles, then the Psi1 cells
__global__ __launch_bounds__(256) void qp_param_reduce_kernel(int B, int M, int Q, int T, int slabs,
                                                              int slabs1, const double *__restrict__ alpha,
                                                              const double *__restrict__ part, const double *__restrict__ part1,
                                                              double *__restrict__ d_z, double *__restrict__ d_gamma,
                                                              double *__restrict__ d_alpha) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nz = (size_t)B * M * Q, ng = (size_t)B * Q;
    const size_t tiles = (size_t)T * (T + 1) / 2, side = (size_t)QP_TILE * Q, cell = 2 * side + Q + 1, cell1 = side + Q + 1;
    if (e < nz) {
        const int b = (int)(e / ((size_t)M * Q)), rem = (int)(e % ((size_t)M * Q)), m = rem / Q, q = rem % Q;
        const int bm = m / QP_TILE;
        const size_t off = (size_t)(m % QP_TILE) * Q + q;
        double acc = 0.0;
        for (int k = 0; k < slabs; ++k) {
            const size_t base = ((size_t)k * B + b) * tiles;
            for (int i = 0; i <= bm; ++i) {
                const size_t idx = (size_t)i * T - (size_t)(i * (i - 1) / 2) + (bm - i);
                acc += part[(base + idx) * cell + side + off];
            }
            const size_t row = (size_t)bm * T - (size_t)(bm * (bm - 1) / 2);
            for (int j = bm; j < T; ++j) acc += part[(base + row + (j - bm)) * cell + off];
        }
        for (int k = 0; k < slabs1; ++k) acc += part1[(((size_t)k * B + b) * T + bm) * cell1 + off];
        d_z[e] = acc;
    } else if (e < nz + ng + B) {                              // d_gamma[b][q], then d_alpha[b] (times alpha: the last entry)
        const bool isa = e >= nz + ng;
        const int b = isa ? (int)(e - nz - ng) : (int)((e - nz) / Q);
        const size_t off = 2 * side + (isa ? (size_t)Q : (e - nz) % Q);
        double acc = 0.0;
        for (int k = 0; k < slabs; ++k)
            for (size_t i = 0; i < tiles; ++i) acc += part[(((size_t)k * B + b) * tiles + i) * cell + off];
        for (int k = 0; k < slabs1; ++k)
            for (int i = 0; i < T; ++i) acc += part1[(((size_t)k * B + b) * T + i) * cell1 + off - side];
        if (isa) d_alpha[b] = acc / alpha[b];
        else d_gamma[e - nz] = acc;
    }
}

// Tests and experiments: a forced number of slabs, read on every plan so that the workspace queries and the launches agree.
// DPGP_QP_N_SLABS: the n slabs of the stats kernel and of both terms of the parameter adjoint (clamped to the staged steps);
// DPGP_QP_PAIR_SLABS: the pair-tile slabs of the adjoint (clamped to the tiles).  The grouped plans go through the same code.

struct QpStatsPlan { int T, tiles, slabs, n_per_slab; };
QpStatsPlan qp_stats_plan(int B, int N, int M) {
    QpStatsPlan p;
    p.T = dpgp_ceil_div(M, QP_TILE);
    p.tiles = qp_tiles(M);
    const int chunks = dpgp_ceil_div(N, QP_SN);
    int sl = dpgp_ceil_div(QP_TARGET_WGS / 2, p.tiles * B);
    if (const int v = dpgp_env_plan("DPGP_QP_N_SLABS", 1, chunks)) sl = v;
    sl = sl < 1 ? 1 : (sl > chunks ? chunks : sl);
    p.n_per_slab = dpgp_ceil_div(chunks, sl) * QP_SN;
    p.slabs = dpgp_ceil_div(N, p.n_per_slab);
    return p;
}

struct QpAdjPlan { int T, tiles, nt, qchunks, slabs, tiles_per_slab; };
QpAdjPlan qp_adj_plan(int B, int N, int M, int Q) {
    QpAdjPlan p;
    p.T = dpgp_ceil_div(M, QP_TILE);
    p.tiles = qp_tiles(M);
    p.nt = dpgp_ceil_div(N, QP_NT);
    p.qchunks = dpgp_ceil_div(Q, QP_QCHUNK);
    long base = (long)p.nt * B * p.qchunks;
    int sl = (int)((QP_TARGET_WGS + base - 1) / base);
    if (const int v = dpgp_env_plan("DPGP_QP_PAIR_SLABS", 1, p.tiles)) sl = v;
    sl = sl < 1 ? 1 : (sl > p.tiles ? p.tiles : sl);
    p.tiles_per_slab = dpgp_ceil_div(p.tiles, sl);
    p.slabs = dpgp_ceil_div(p.tiles, p.tiles_per_slab);
    return p;
}

// parameter adjoint: n slabs so that tiles x slabs x B x q chunks fills the GPU (256-thread workgroups, as the stats plan)
struct QpParamPlan { int T, tiles, qchunks, slabs, n_per_slab, slabs1, n_per_slab1; };
QpParamPlan qp_param_plan(int B, int N, int M, int Q) {
    QpParamPlan p;
    p.T = dpgp_ceil_div(M, QP_TILE);
    p.tiles = qp_tiles(M);
    p.qchunks = dpgp_ceil_div(Q, QP_PCHUNK);
    const int chunks = dpgp_ceil_div(N, QP_SN);
    const long base = (long)p.tiles * B * p.qchunks;
    int sl = (int)((QP_TARGET_WGS / 2 + base - 1) / base);
    const int forced = dpgp_env_plan("DPGP_QP_N_SLABS", 1, chunks);
    if (forced) sl = forced;
    sl = sl < 1 ? 1 : (sl > chunks ? chunks : sl);
    p.n_per_slab = dpgp_ceil_div(chunks, sl) * QP_SN;
    p.slabs = dpgp_ceil_div(N, p.n_per_slab);
    sl = dpgp_ceil_div(QP_TARGET_WGS / 2, p.T * B);             // (the Psi1 term: blocks of 32 inducing points x slabs x B)
    if (forced) sl = forced;
    sl = sl < 1 ? 1 : (sl > chunks ? chunks : sl);
    p.n_per_slab1 = dpgp_ceil_div(chunks, sl) * QP_SN;
    p.slabs1 = dpgp_ceil_div(N, p.n_per_slab1);
    return p;
}
// doubles per (slab, b, tile): the two d_z sides [2][32][Q], d_gamma [Q], d_alpha; per (Psi1 slab, b, block): one side
size_t qp_param_part_elems(int Q) { return (size_t)2 * QP_TILE * Q + Q + 1; }
size_t qp_param_part1_elems(int Q) { return (size_t)QP_TILE * Q + Q + 1; }
size_t qp_param_psi1_lds(int Q) {
    return sizeof(double) * ((size_t)3 * QP_SN * Q + QP_SN + (size_t)QP_TILE * (Q | 1) + Q + QP_SN * QP_HSTRIDE +
                             (size_t)2 * QP_TILE * Q + 256);
}
size_t qp_param_lds(int Q) {
    return sizeof(double) * ((size_t)4 * QP_SN * Q + QP_SN + (size_t)2 * QP_TILE * (Q | 1) + Q + 2 * QP_TILE * QP_HSTRIDE + 256);
}

size_t qp_stats_lds(int Q) { return sizeof(double) * ((size_t)2 * QP_SN * Q + QP_SN + (size_t)2 * QP_TILE * Q + Q); }
size_t qp_adj_lds(int Q) {
    return sizeof(double) * ((size_t)3 * Q * QP_NT + (size_t)2 * QP_TILE * Q + QP_TILE * QP_HSTRIDE + Q);
}

template <int KQ, bool WEIGHTED>
int qp_launch_adjoint(const QpAdjPlan &p, int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                      const double *gamma, const double *alpha, const double *zfac, const double *wt, const double *g1,
                      const double *g2, double *part, hipStream_t st) {
    const size_t lds = qp_adj_lds(Q);
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(qp_adjoint_kernel<KQ, WEIGHTED>), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL((qp_adjoint_kernel<KQ, WEIGHTED>), dim3(p.nt, p.slabs, B * p.qchunks), dim3(QP_NT), lds, st, B, N, M, Q,
                       p.T, p.tiles_per_slab, z, mu, s, gamma, alpha, zfac, wt, g1, g2, part);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

template <bool WEIGHTED>
int qp_launch_psi2(const QpStatsPlan &p, int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                   const double *gamma, const double *alpha, const double *zfac, const double *wt, double *part,
                   hipStream_t st) {
    const size_t lds = qp_stats_lds(Q);
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(qp_psi2_kernel<WEIGHTED>), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL((qp_psi2_kernel<WEIGHTED>), dim3(p.tiles, p.slabs, B), dim3(256), lds, st, N, M, Q, p.T, p.n_per_slab,
                       z, mu, s, gamma, alpha, zfac, wt, part);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

template <bool WEIGHTED>
int qp_dispatch_adjoint(const QpAdjPlan &p, int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                        const double *gamma, const double *alpha, const double *zfac, const double *wt, const double *g1,
                        const double *g2, double *part, hipStream_t st) {
    const int w = Q < QP_QCHUNK ? Q : QP_QCHUNK;
    return w <= 1   ? qp_launch_adjoint<1, WEIGHTED>(p, B, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g1, g2, part, st)
           : w <= 2 ? qp_launch_adjoint<2, WEIGHTED>(p, B, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g1, g2, part, st)
           : w <= 4 ? qp_launch_adjoint<4, WEIGHTED>(p, B, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g1, g2, part, st)
                    : qp_launch_adjoint<8, WEIGHTED>(p, B, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g1, g2, part, st);
}

template <int KQ, bool WEIGHTED>
int qp_launch_param(const QpParamPlan &p, int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                    const double *gamma, const double *alpha, const double *zfac, const double *wt, const double *g2,
                    double *part, hipStream_t st) {
    const size_t lds = qp_param_lds(Q);
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(qp_param_kernel<KQ, WEIGHTED>), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL((qp_param_kernel<KQ, WEIGHTED>), dim3(p.tiles, p.slabs, B * p.qchunks), dim3(256), lds, st, B, N, M, Q,
                       p.T, p.n_per_slab, z, mu, s, gamma, alpha, zfac, wt, g2, part);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

template <bool WEIGHTED>
int qp_dispatch_param(const QpParamPlan &p, int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                      const double *gamma, const double *alpha, const double *zfac, const double *wt, const double *g2,
                      double *part, hipStream_t st) {
    return Q <= 1   ? qp_launch_param<1, WEIGHTED>(p, B, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g2, part, st)
           : Q <= 2 ? qp_launch_param<2, WEIGHTED>(p, B, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g2, part, st)
                    : qp_launch_param<QP_PCHUNK, WEIGHTED>(p, B, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g2, part, st);
}

bool qp_shape_ok(int B, int N, int M, int Q) {
    return B >= 1 && N >= 1 && M >= 1 && Q >= 1 && Q <= DPGP_QX_PSI_MAX_Q;
}

}  // namespace

extern "C" size_t dpgp_qx_psi_stats_workspace_bytes(int B, int N, int M, int Q) {
    if (!qp_shape_ok(B, N, M, Q)) return 0;
    const QpStatsPlan p = qp_stats_plan(B, N, M);
    return sizeof(double) * (size_t)p.slabs * B * M * M;
}

// wt == NULL: the unweighted instantiations (dpgp_qx_psi_stats_batched_f64 is this with wt == NULL)
extern "C" int dpgp_qx_psi_stats_weighted_f64(int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                                              const double *gamma, const double *alpha, const double *zfac, const double *wt,
                                              double *psi1, double *psi2, void *ws, size_t ws_bytes, void *stream) {
    if (B < 1) return -1;
    if (N < 1) return -2;
    if (M < 1) return -3;
    if (Q < 1 || Q > DPGP_QX_PSI_MAX_Q) return -4;
    if (!z) return -5;
    if (!mu) return -6;
    if (!s) return -7;
    if (!gamma) return -8;
    if (!alpha) return -9;
    if (!psi1) return -11;
    if (!psi2) return -12;
    if (!ws) return -13;
    if (ws_bytes < dpgp_qx_psi_stats_workspace_bytes(B, N, M, Q)) return -14;
    hipStream_t st = (hipStream_t)stream;
    const QpStatsPlan p = qp_stats_plan(B, N, M);
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(qp_psi1_kernel, dim3((unsigned)(((size_t)N * M + 255) / 256), B), dim3(256), 0, st, N, M, Q, z, mu, s,
                       gamma, alpha, psi1);
    DPGP_LAUNCH_CHECK();
    double *part = static_cast<double *>(ws);
    const int rc = wt ? qp_launch_psi2<true>(p, B, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, part, st)
                      : qp_launch_psi2<false>(p, B, N, M, Q, z, mu, s, gamma, alpha, zfac, nullptr, part, st);
    if (rc) return rc;
    const size_t tot = (size_t)B * M * M;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(qp_psi2_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, B, M, p.slabs, part, psi2);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

extern "C" int dpgp_qx_psi_stats_batched_f64(int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                                             const double *gamma, const double *alpha, const double *zfac, double *psi1,
                                             double *psi2, void *ws, size_t ws_bytes, void *stream) {
    return dpgp_qx_psi_stats_weighted_f64(B, N, M, Q, z, mu, s, gamma, alpha, zfac, nullptr, psi1, psi2, ws, ws_bytes, stream);
}

extern "C" size_t dpgp_qx_psi_adjoint_workspace_bytes(int B, int N, int M, int Q) {
    if (!qp_shape_ok(B, N, M, Q)) return 0;
    const QpAdjPlan p = qp_adj_plan(B, N, M, Q);
    return sizeof(double) * (size_t)p.slabs * B * 2 * Q * N;
}

// wt == NULL: the unweighted instantiations (dpgp_qx_psi_adjoint_f64 is this with wt == NULL)
extern "C" int dpgp_qx_psi_adjoint_weighted_f64(int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                                                const double *gamma, const double *alpha, const double *zfac, const double *wt,
                                                const double *g1, const double *g2, double *d_mu, double *d_s, void *ws,
                                                size_t ws_bytes, void *stream) {
    if (B < 1) return -1;
    if (N < 1) return -2;
    if (M < 1) return -3;
    if (Q < 1 || Q > DPGP_QX_PSI_MAX_Q) return -4;
    if (!z) return -5;
    if (!mu) return -6;
    if (!s) return -7;
    if (!gamma) return -8;
    if (!alpha) return -9;
    if (!g1) return -11;
    if (!g2) return -12;
    if (!d_mu) return -13;
    if (!d_s) return -14;
    if (!ws) return -15;
    if (ws_bytes < dpgp_qx_psi_adjoint_workspace_bytes(B, N, M, Q)) return -16;
    hipStream_t st = (hipStream_t)stream;
    const QpAdjPlan p = qp_adj_plan(B, N, M, Q);
    double *part = static_cast<double *>(ws);
    const int rc = wt ? qp_dispatch_adjoint<true>(p, B, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g1, g2, part, st)
                      : qp_dispatch_adjoint<false>(p, B, N, M, Q, z, mu, s, gamma, alpha, zfac, nullptr, g1, g2, part, st);
    if (rc) return rc;
    const size_t tot = (size_t)2 * Q * N;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(qp_adjoint_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, B, N, Q, p.slabs, part,
                       d_mu, d_s);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

extern "C" int dpgp_qx_psi_adjoint_f64(int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                                       const double *gamma, const double *alpha, const double *zfac, const double *g1,
                                       const double *g2, double *d_mu, double *d_s, void *ws, size_t ws_bytes, void *stream) {
    return dpgp_qx_psi_adjoint_weighted_f64(B, N, M, Q, z, mu, s, gamma, alpha, zfac, nullptr, g1, g2, d_mu, d_s, ws, ws_bytes,
                                            stream);
}

extern "C" size_t dpgp_qx_psi_param_adjoint_workspace_bytes(int B, int N, int M, int Q) {
    if (!qp_shape_ok(B, N, M, Q)) return 0;
    const QpParamPlan p = qp_param_plan(B, N, M, Q);
    return sizeof(double) * ((size_t)p.slabs * B * p.tiles * qp_param_part_elems(Q) +
                             (size_t)p.slabs1 * B * p.T * qp_param_part1_elems(Q));
}

// the adjoint of the weighted Psi statistics with respect to the kernels' own parameters, per kernel b (not summed over b)
extern "C" int dpgp_qx_psi_param_adjoint_weighted_f64(int B, int N, int M, int Q, const double *z, const double *mu,
                                                      const double *s, const double *gamma, const double *alpha,
                                                      const double *zfac, const double *wt, const double *g1, const double *g2,
                                                      double *d_z, double *d_gamma, double *d_alpha, void *ws, size_t ws_bytes,
                                                      void *stream) {
    if (B < 1) return -1;
    if (N < 1) return -2;
    if (M < 1) return -3;
    if (Q < 1 || Q > DPGP_QX_PSI_MAX_Q) return -4;
    if (!z) return -5;
    if (!mu) return -6;
    if (!s) return -7;
    if (!gamma) return -8;
    if (!alpha) return -9;
    if (!g1) return -11;
    if (!g2) return -12;
    if (!d_z) return -13;
    if (!d_gamma) return -14;
    if (!d_alpha) return -15;
    if (!ws) return -16;
    if (ws_bytes < dpgp_qx_psi_param_adjoint_workspace_bytes(B, N, M, Q)) return -17;
    hipStream_t st = (hipStream_t)stream;
    const QpParamPlan p = qp_param_plan(B, N, M, Q);
    double *part = static_cast<double *>(ws), *part1 = part + (size_t)p.slabs * B * p.tiles * qp_param_part_elems(Q);
    const int rc = wt ? qp_dispatch_param<true>(p, B, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g2, part, st)
                      : qp_dispatch_param<false>(p, B, N, M, Q, z, mu, s, gamma, alpha, zfac, nullptr, g2, part, st);
    if (rc) return rc;
    const size_t lds1 = qp_param_psi1_lds(Q);
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(qp_param_psi1_kernel), lds1)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(qp_param_psi1_kernel, dim3(p.T, p.slabs1, B), dim3(256), lds1, st, B, N, M, Q, p.n_per_slab1, z, mu, s, gamma,
                       alpha, g1, part1);
    DPGP_LAUNCH_CHECK();
    const size_t tot = (size_t)B * M * Q + (size_t)B * Q + B;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(qp_param_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, B, M, Q, p.T, p.slabs, p.slabs1,
                       alpha, part, part1, d_z, d_gamma, d_alpha);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

// ---- Pattern-grouped forms: K kernels x P weight rows w[P][N] shared by the kernels (the masked over-T model: atom k, row
// pattern p).  The slot form of the weighted operators above would run B = K P slots and evaluate every (kernel, point, pair)
// exponential P times; here it is evaluated once per chunk of PC patterns.
//   stats:   qp_psi2_kernel with PC accumulators per pair: workgroup (pair tile, n slab, (k, pattern chunk)); the staged point
//            carries c2_n and its PC weights; psi2 partials land in slot k P + p of the slot form's workspace layout, so the
//            slot form's reduction adds them.  Psi1 is qp_psi1_kernel with B = K (not weighted, once per kernel).
//   adjoint: qp_adjoint_kernel with PC weighted pair-factor tiles H_p [32][33] and the lane's PC weights in registers; per pair
//            h = sum_p w_p(lane) H_p[r][c], then the one exponential.  A workgroup is NW waves (64 NW points) that share the
//            staged z rows and H tiles: 8 (3 Q 64 NW + 65 Q + 1056 PC) bytes of LDS, (PC, NW) picked per Q on the host
//            (qg_adj_plan) to stay inside 160 KiB.  Workgroup (64 NW points, pair slab, (k, q chunk, pattern chunk)); the
//            Psi1 term is done with pattern chunk 0 only (g1 is already summed over the patterns).  A wave whose points have
//            zero weight for the whole chunk skips its pair loops; a workgroup of such waves skips the off-diagonal tiles.
//   parameter adjoint: qp_param_kernel with the weighted pair factor of the chunk's PC patterns in registers; per (point,
//            pair) the effective weight sum_p w_pn h_p, then one exponential and ONE accumulator set for the whole chunk.
//            Workgroup (pair tile, n slab, (k, q chunk, pattern chunk)); the reduction adds the pattern chunks of a kernel
//            in chunk order.  The Psi1 term is qp_param_psi1_kernel with B = K.
// A staged point whose PC weights are all zero is skipped (a workgroup-uniform branch): no exponential, exact zeros.
#define QG_MAX_PC 8
#define QG_LDS_BUDGET (160 * 1024)

namespace {

int qg_pow2_width(int P) { return P >= 5 ? 8 : P >= 3 ? 4 : P >= 2 ? 2 : 1; }

template <int PC>
__global__ __launch_bounds__(256) void qg_psi2_kernel(int P, int N, int M, int Q, int T, int n_per_slab, int pchunks,
                                                      const double *__restrict__ z, const double *__restrict__ mu,
                                                      const double *__restrict__ s, const double *__restrict__ gamma,
                                                      const double *__restrict__ alpha, const double *__restrict__ zfac,
                                                      const double *__restrict__ wt, double *__restrict__ part) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *smu = reinterpret_cast<double *>(smem_raw);    // [QP_SN][Q]
    double *siw = smu + (size_t)QP_SN * Q;                  // [QP_SN][Q]
    double *sc2 = siw + (size_t)QP_SN * Q;                  // [QP_SN] c2_n, 0: every weight of the chunk is 0
    double *sw = sc2 + QP_SN;                               // [QP_SN][PC] the chunk's weights
    double *zr = sw + QP_SN * PC;                           // [32][Q] rows of block I
    double *zc = zr + (size_t)QP_TILE * Q;                  // [32][Q] columns of block J
    double *gm = zc + (size_t)QP_TILE * Q;                  // [Q]
    const int t = threadIdx.x, slab = blockIdx.y;
    const int kb = blockIdx.z / pchunks, p0 = (blockIdx.z % pchunks) * PC;
    const int np = min(PC, P - p0);
    int I, J;
    dpgp_tile_ij(blockIdx.x, T, I, J);
    const int m0 = I * QP_TILE, c0 = J * QP_TILE;
    const double *zb = z + (size_t)kb * M * Q;
    for (int k = t; k < QP_TILE * Q; k += 256) {
        const int r = k / Q, q = k % Q;
        zr[k] = m0 + r < M ? zb[(size_t)(m0 + r) * Q + q] : 0.0;
        zc[k] = c0 + r < M ? zb[(size_t)(c0 + r) * Q + q] : 0.0;
    }
    for (int q = t; q < Q; q += 256) gm[q] = gamma[(size_t)kb * Q + q];
    const double al = alpha[kb];
    const int c = t & 31, rg = t >> 5;
    double acc[PC][4];
#pragma unroll
    for (int p = 0; p < PC; ++p)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[p][k] = 0.0;
    const int n_lo = slab * n_per_slab, n_hi = min(N, n_lo + n_per_slab);
    for (int nb = n_lo; nb < n_hi; nb += QP_SN) {
        const int nn = min(QP_SN, n_hi - nb);
        __syncthreads();                                       // (previous step done with the staged points)
        for (int k = t; k < nn * Q; k += 256) {
            const int i = k / Q, q = k % Q;
            const double g = gamma[(size_t)kb * Q + q], w2 = fma(2.0 * g, s[(size_t)(nb + i) * Q + q], 1.0);
            smu[k] = mu[(size_t)(nb + i) * Q + q];
            siw[k] = g / w2;
        }
        if (t < nn) {
            bool any = false;
#pragma unroll
            for (int p = 0; p < PC; ++p) {
                const double wv = p < np ? wt[(size_t)(p0 + p) * N + nb + t] : 0.0;
                sw[t * PC + p] = wv;
                any = any || wv != 0.0;
            }
            double cv = 0.0;
            if (any) {
                double l = 0.0;
                for (int q = 0; q < Q; ++q) l += log(fma(2.0 * gamma[(size_t)kb * Q + q], s[(size_t)(nb + t) * Q + q], 1.0));
                cv = exp(-0.5 * l);
            }
            sc2[t] = cv;
        }
        __syncthreads();
        for (int i = 0; i < nn; ++i) {
            const double cv = sc2[i];
            if (cv == 0.0) continue;                           // (the same LDS word for every thread: uniform)
            const double *mi = smu + (size_t)i * Q, *wi = siw + (size_t)i * Q;
            double ex[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = rg + 8 * k;
                double e = 0.0;
                for (int q = 0; q < Q; ++q) {
                    const double d = mi[q] - 0.5 * (zr[r * Q + q] + zc[c * Q + q]);
                    e = fma(wi[q] * d, d, e);
                }
                ex[k] = cv * exp(-e);
            }
#pragma unroll
            for (int p = 0; p < PC; ++p) {
                const double wv = sw[i * PC + p];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[p][k] = fma(wv, ex[k], acc[p][k]);
            }
        }
    }
    const int mp = c0 + c;
    if (mp >= M) return;
    double f[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int m = m0 + rg + 8 * k;
        f[k] = m < M ? qp_pair_factor(zfac, kb, M, Q, m, mp, zr + (size_t)(rg + 8 * k) * Q, zc + (size_t)c * Q, gm, al) : 0.0;
    }
    const size_t B = (size_t)(gridDim.z / pchunks) * P;
#pragma unroll
    for (int p = 0; p < PC; ++p) {
        if (p >= np) break;
        double *pb = part + ((size_t)slab * B + (size_t)kb * P + p0 + p) * M * M;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int m = m0 + rg + 8 * k;
            if (m < M) pb[(size_t)m * M + mp] = acc[p][k] * f[k];
        }
    }
}

// adjoint partials: (64 NW points, pair slab, (k, q chunk, pattern chunk)); blockDim.x = 64 NW
template <int KQ, int PC>
__global__ __launch_bounds__(256) void qg_adjoint_kernel(int K, int P, int N, int M, int Q, int T, int tiles_per_slab,
                                                         int pchunks, const double *__restrict__ z,
                                                         const double *__restrict__ mu, const double *__restrict__ s,
                                                         const double *__restrict__ gamma, const double *__restrict__ alpha,
                                                         const double *__restrict__ zfac, const double *__restrict__ wt,
                                                         const double *__restrict__ g1, const double *__restrict__ g2,
                                                         double *__restrict__ part) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int NT = blockDim.x;                              // points of the workgroup
    double *smu = reinterpret_cast<double *>(smem_raw);    // [Q][NT]
    double *siw1 = smu + (size_t)Q * NT;                    // [Q][NT]
    double *siw2 = siw1 + (size_t)Q * NT;                   // [Q][NT]
    double *zr = siw2 + (size_t)Q * NT;                     // [32][Q]
    double *zc = zr + (size_t)QP_TILE * Q;                  // [32][Q]
    double *hs = zc + (size_t)QP_TILE * Q;                  // [PC][32][33] weighted pair factors of the chunk's patterns
    double *gm = hs + PC * QP_TILE * QP_HSTRIDE;            // [Q]
    const int lane = threadIdx.x, slab = blockIdx.y;
    const int qchunks = (Q + QP_QCHUNK - 1) / QP_QCHUNK;
    const int pcn = blockIdx.z % pchunks, qc = (blockIdx.z / pchunks) % qchunks, kb = blockIdx.z / (pchunks * qchunks);
    const int p0 = pcn * PC, np = min(PC, P - p0), q0 = qc * QP_QCHUNK;
    const int nq = min(QP_QCHUNK, Q - q0);
    const int n = blockIdx.x * NT + lane;
    const bool live = n < N;
    const double al = alpha[kb];
    const double *gb = gamma + (size_t)kb * Q;
    const double *zb = z + (size_t)kb * M * Q;
    for (int q = lane; q < Q; q += NT) gm[q] = gb[q];
    double l1 = 0.0, l2 = 0.0;
    for (int q = 0; q < Q; ++q) {
        const double g = gb[q], sv = live ? s[(size_t)n * Q + q] : 1.0;
        const double w1 = fma(g, sv, 1.0), w2 = fma(2.0 * g, sv, 1.0);
        smu[q * NT + lane] = live ? mu[(size_t)n * Q + q] : 0.0;
        siw1[q * NT + lane] = g / w1;
        siw2[q * NT + lane] = g / w2;
        l1 += log(w1);
        l2 += log(w2);
    }
    double wl[PC];
    bool mine = false;
#pragma unroll
    for (int p = 0; p < PC; ++p) {
        wl[p] = (live && p < np) ? wt[(size_t)(p0 + p) * N + n] : 0.0;
        mine = mine || wl[p] != 0.0;
    }
    const double c1 = al * exp(-0.5 * l1), c2 = exp(-0.5 * l2);
    const bool pairs = __any(mine);                            // uniform over the wave
    const bool wg_pairs = __syncthreads_or(mine);              // uniform over the workgroup
    const bool with_psi1 = pcn == 0;
    double mk[KQ], i1[KQ], i2[KQ], s1[KQ], s2[KQ], t1[KQ], t2[KQ], dk[KQ];
    double s0 = 0.0, t0 = 0.0;
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
        const bool on = k < nq;
        mk[k] = on ? smu[(q0 + k) * NT + lane] : 0.0;
        i1[k] = on ? siw1[(q0 + k) * NT + lane] : 0.0;
        i2[k] = on ? siw2[(q0 + k) * NT + lane] : 0.0;
        s1[k] = s2[k] = t1[k] = t2[k] = dk[k] = 0.0;
    }
    const bool one = nq == Q;                                  // the chunk is every latent dim: exponent from registers
    const int tile_lo = slab * tiles_per_slab, tile_hi = min(T * (T + 1) / 2, tile_lo + tiles_per_slab);
    for (int tile = tile_lo; tile < tile_hi; ++tile) {
        int I, J;
        dpgp_tile_ij(tile, T, I, J);
        if (!wg_pairs && (I != J || !with_psi1)) continue;     // (workgroup-uniform) nothing weighted and no Psi1 term here
        const int m0 = I * QP_TILE, c0 = J * QP_TILE;
        const int nr = min(QP_TILE, M - m0), nc = min(QP_TILE, M - c0);
        __syncthreads();                                       // (previous tile done with zr / zc / hs)
        for (int k = lane; k < QP_TILE * Q; k += NT) {
            const int r = k / Q, q = k % Q;
            zr[k] = r < nr ? zb[(size_t)(m0 + r) * Q + q] : 0.0;
            zc[k] = r < nc ? zb[(size_t)(c0 + r) * Q + q] : 0.0;
        }
        __syncthreads();
        if (wg_pairs)
            for (int k = lane; k < QP_TILE * QP_TILE; k += NT) {
                const int r = k / QP_TILE, cc = k % QP_TILE, m = m0 + r, mp = c0 + cc;
                const bool in = r < nr && cc < nc && (I != J || cc >= r);
                const double f = in ? qp_pair_factor(zfac, kb, M, Q, m, mp, zr + (size_t)r * Q, zc + (size_t)cc * Q, gm, al) : 0.0;
#pragma unroll
                for (int p = 0; p < PC; ++p) {
                    double h = 0.0;
                    if (in && p < np) {
                        const double *g2b = g2 + ((size_t)kb * P + p0 + p) * M * M;
                        const double w = m == mp ? g2b[(size_t)m * M + m] : g2b[(size_t)m * M + mp] + g2b[(size_t)mp * M + m];
                        h = w * f;
                    }
                    hs[(p * QP_TILE + r) * QP_HSTRIDE + cc] = h;
                }
            }
        __syncthreads();
        // Psi2 term over the tile's pairs (uniform over the wave: every lane visits the same pair)
        for (int r = 0; r < (pairs ? nr : 0); ++r) {
            const double *zrr = zr + (size_t)r * Q;
            for (int cc = (I == J ? r : 0); cc < nc; ++cc) {
                double h = 0.0;
#pragma unroll
                for (int p = 0; p < PC; ++p) h = fma(wl[p], hs[(p * QP_TILE + r) * QP_HSTRIDE + cc], h);
                const double *zcc = zc + (size_t)cc * Q;
                double e = 0.0;
                if (one) {
#pragma unroll
                    for (int k = 0; k < KQ; ++k)
                        if (k < nq) {
                            dk[k] = mk[k] - 0.5 * (zrr[k] + zcc[k]);
                            e = fma(i2[k] * dk[k], dk[k], e);
                        }
                } else {
                    for (int q = 0; q < Q; ++q) {
                        const double d = smu[q * NT + lane] - 0.5 * (zrr[q] + zcc[q]);
                        e = fma(siw2[q * NT + lane] * d, d, e);
                    }
#pragma unroll
                    for (int k = 0; k < KQ; ++k)
                        if (k < nq) dk[k] = mk[k] - 0.5 * (zrr[q0 + k] + zcc[q0 + k]);
                }
                const double a = h * c2 * exp(-e);
                s0 += a;
#pragma unroll
                for (int k = 0; k < KQ; ++k) {
                    const double ad = a * dk[k];
                    s1[k] += ad;
                    s2[k] = fma(ad, dk[k], s2[k]);
                }
            }
        }
        // Psi1 term of the column block: evaluated with the diagonal tile, by pattern chunk 0
        if (I == J && live && with_psi1) {
            const double *g1n = g1 + ((size_t)kb * N + n) * M;
            for (int r = 0; r < nr; ++r) {
                const double *zrr = zr + (size_t)r * Q;
                double e = 0.0;
                if (one) {
#pragma unroll
                    for (int k = 0; k < KQ; ++k)
                        if (k < nq) {
                            dk[k] = mk[k] - zrr[k];
                            e = fma(i1[k] * dk[k], dk[k], e);
                        }
                } else {
                    for (int q = 0; q < Q; ++q) {
                        const double d = smu[q * NT + lane] - zrr[q];
                        e = fma(siw1[q * NT + lane] * d, d, e);
                    }
#pragma unroll
                    for (int k = 0; k < KQ; ++k)
                        if (k < nq) dk[k] = mk[k] - zrr[q0 + k];
                }
                const double a = g1n[m0 + r] * c1 * exp(-0.5 * e);
                t0 += a;
#pragma unroll
                for (int k = 0; k < KQ; ++k) {
                    const double ad = a * dk[k];
                    t1[k] += ad;
                    t2[k] = fma(ad, dk[k], t2[k]);
                }
            }
        }
    }
    if (!live) return;
    // part[((slab * K pchunks + k pchunks + chunk) * 2 + {0: d_mu, 1: d_s}) * Q + q][n]: the slot form's layout with B = K pchunks
    double *pb = part + ((size_t)slab * K * pchunks + (size_t)kb * pchunks + pcn) * 2 * Q * N;
#pragma unroll
    for (int k = 0; k < KQ; ++k)
        if (k < nq) {
            const int q = q0 + k;
            pb[(size_t)q * N + n] = -i1[k] * t1[k] - 2.0 * i2[k] * s1[k];
            pb[((size_t)Q + q) * N + n] = 0.5 * i1[k] * (i1[k] * t2[k] - t0) + i2[k] * (2.0 * i2[k] * s2[k] - s0);
        }
}

// parameter adjoint, Psi2 term: (pair tile, n slab, (k, q chunk, pattern chunk)); cells as qp_param_kernel with B = K pchunks
template <int KQ, int PC>
__global__ __launch_bounds__(256) void qg_param_kernel(int K, int P, int N, int M, int Q, int T, int n_per_slab, int pchunks,
                                                       const double *__restrict__ z, const double *__restrict__ mu,
                                                       const double *__restrict__ s, const double *__restrict__ gamma,
                                                       const double *__restrict__ alpha, const double *__restrict__ zfac,
                                                       const double *__restrict__ wt, const double *__restrict__ g2,
                                                       double *__restrict__ part) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int ZS = Q | 1;                                   // odd row stride of the z tiles: lane = column reads hit 32 banks
    double *sp = reinterpret_cast<double *>(smem_raw);    // staged points [QP_SN][Q][4]: mu, gamma / w2, 1 / w2, s / w2
    double *sc = sp + (size_t)QP_SN * Q * 4;                // [QP_SN] c2_n, 0: every weight of the chunk is 0
    double *sw = sc + QP_SN;                                // [QP_SN][PC] the chunk's weights
    double *zt = sw + QP_SN * PC;                           // [64][ZS]: rows of block I, then columns of block J
    double *gm = zt + (size_t)2 * QP_TILE * ZS;             // [Q]
    double *buf = gm + Q;                                   // [2][32][33] row- and column-side d_z terms, then [256]
    const int t = threadIdx.x, slab = blockIdx.y;
    const int qchunks = (Q + QP_PCHUNK - 1) / QP_PCHUNK;
    const int pcn = blockIdx.z % pchunks, qc = (blockIdx.z / pchunks) % qchunks, kb = blockIdx.z / (pchunks * qchunks);
    const int pl = pcn * PC, np = min(PC, P - pl), q0 = qc * QP_PCHUNK;
    const int nq = min(QP_PCHUNK, Q - q0);
    int I, J;
    dpgp_tile_ij(blockIdx.x, T, I, J);
    const bool diag = I == J;
    const int m0 = I * QP_TILE, c0 = J * QP_TILE;
    {
        const double *zb = z + (size_t)kb * M * Q;
        for (int k = t; k < QP_TILE * Q; k += 256) {
            const int r = k / Q, q = k % Q;
            zt[r * ZS + q] = m0 + r < M ? zb[(size_t)(m0 + r) * Q + q] : 0.0;
            zt[(QP_TILE + r) * ZS + q] = c0 + r < M ? zb[(size_t)(c0 + r) * Q + q] : 0.0;
        }
        for (int q = t; q < Q; q += 256) gm[q] = gamma[(size_t)kb * Q + q];
    }
    const int c = t & 31, rg = t >> 5;
    const double *zcc = zt + (size_t)(QP_TILE + c) * ZS;     // the thread's column
    const double *zr0 = zt + (size_t)rg * ZS;                // its rows: zr0 + 8 k ZS
    __syncthreads();
    // weighted pair factor of the thread's four pairs, per pattern of the chunk (0: out of range, below the diagonal of a
    // diagonal tile, or no such pattern)
    double h[4][PC];
    {
        const double al = alpha[kb];
        const int mp = c0 + c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = rg + 8 * k, m = m0 + r;
            const bool in = m < M && mp < M && (!diag || c >= r);
            const double f = in ? qp_pair_factor(zfac, kb, M, Q, m, mp, zr0 + (size_t)8 * k * ZS, zcc, gm, al) : 0.0;
#pragma unroll
            for (int p = 0; p < PC; ++p) {
                h[k][p] = 0.0;
                if (in && p < np) {
                    const double *g2b = g2 + ((size_t)kb * P + pl + p) * M * M;
                    const double w = m == mp ? g2b[(size_t)m * M + m] : g2b[(size_t)m * M + mp] + g2b[(size_t)mp * M + m];
                    h[k][p] = w * f;
                }
            }
        }
    }
    double p0[4], p1[4][KQ], p2[4][KQ];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        p0[k] = 0.0;
#pragma unroll
        for (int kk = 0; kk < KQ; ++kk) p1[k][kk] = p2[k][kk] = 0.0;
    }
    const int n_hi = min(N, (slab + 1) * n_per_slab);
    for (int nb = slab * n_per_slab; nb < n_hi; nb += QP_SN) {
        const int nn = min(QP_SN, n_hi - nb);
        __syncthreads();                                       // (previous step done with the staged points)
        for (int k = t; k < nn * Q; k += 256) {
            const int q = k % Q;
            const double g = gm[q], sv = s[(size_t)nb * Q + k];
            const double i2 = 1.0 / fma(2.0 * g, sv, 1.0);
            sp[4 * k] = mu[(size_t)nb * Q + k];
            sp[4 * k + 1] = g * i2;
            sp[4 * k + 2] = i2;
            sp[4 * k + 3] = sv * i2;
        }
        if (t < nn) {
            bool any = false;
#pragma unroll
            for (int p = 0; p < PC; ++p) {
                const double wv = p < np ? wt[(size_t)(pl + p) * N + nb + t] : 0.0;
                sw[t * PC + p] = wv;
                any = any || wv != 0.0;
            }
            double cv = 0.0;
            if (any) {
                const double *sn = s + (size_t)(nb + t) * Q;
                double l = 0.0;
                for (int q = 0; q < Q; ++q) l += log(fma(2.0 * gm[q], sn[q], 1.0));
                cv = exp(-0.5 * l);
                if (PC == 1) cv *= sw[t];                      // (one pattern: the weight rides in c2_n, as in qp_param_kernel)
            }
            sc[t] = cv;
        }
        __syncthreads();
        // Psi2 term: one exponential per (point, pair) for the whole chunk of patterns, then the chunk's accumulators
        for (int i = 0; i < nn; ++i) {
            const double c2 = sc[i];
            if (c2 == 0.0) continue;                           // (the same LDS word for every thread: uniform)
            const double *pi = sp + (size_t)i * Q * 4;
            double a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                double he = h[k][0];
                if (PC > 1) {
                    he = 0.0;
#pragma unroll
                    for (int p = 0; p < PC; ++p) he = fma(sw[i * PC + p], h[k][p], he);
                }
                const double *zrr = zr0 + (size_t)8 * k * ZS;
                double e = 0.0;
                for (int q = 0; q < Q; ++q) {
                    const double d = pi[4 * q] - 0.5 * (zrr[q] + zcc[q]);
                    e = fma(pi[4 * q + 1] * d, d, e);
                }
                a[k] = he * c2 * exp(-e);
                p0[k] += a[k];
            }
#pragma unroll
            for (int kk = 0; kk < KQ; ++kk)
                if (kk < nq) {
                    const int q = q0 + kk;
                    const double mq = pi[4 * q], iv = pi[4 * q + 2], rs = pi[4 * q + 3], zcq = zcc[q];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const double di = (mq - 0.5 * (zr0[8 * k * ZS + q] + zcq)) * iv;
                        p1[k][kk] = fma(a[k], di, p1[k][kk]);
                        p2[k][kk] = fma(a[k], fma(di, di, rs), p2[k][kk]);
                    }
                }
        }
    }
    // tile-level sums in a fixed order, one latent dim at a time; cell of the workspace: [2][32][Q] d_z sides, [Q], [1]
    double *pz = part + ((((size_t)slab * K + kb) * pchunks + pcn) * gridDim.x + blockIdx.x) * ((size_t)2 * QP_TILE * Q + Q + 1);
    double *bufb = buf + QP_TILE * QP_HSTRIDE, *red = bufb + QP_TILE * QP_HSTRIDE;
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk)
        if (kk < nq) {                                         // (uniform)
            const int q = q0 + kk;
            const double gq = gm[q];
            double gv = 0.0;
            __syncthreads();                                   // (previous dim's sums read)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = rg + 8 * k;
                const double dz = zr0[8 * k * ZS + q] - zcc[q];
                const double u = gq * p1[k][kk], hd = 0.5 * gq * dz * p0[k];
                buf[r * QP_HSTRIDE + c] = u - hd;
                bufb[r * QP_HSTRIDE + c] = u + hd;
                gv -= fma(0.25 * dz * dz, p0[k], p2[k][kk]);
            }
            __syncthreads();
            if (t < 32) {
                double acc = 0.0;
                for (int cc = 0; cc < QP_TILE; ++cc) acc += buf[t * QP_HSTRIDE + cc];
                pz[(size_t)t * Q + q] = acc;
            } else if (t < 64) {
                double acc = 0.0;
                for (int r = 0; r < QP_TILE; ++r) acc += bufb[r * QP_HSTRIDE + (t - 32)];
                pz[(size_t)t * Q + q] = acc;
            }
            const double tot = qp_block_sum(gv, red, t);
            if (t == 0) pz[(size_t)2 * QP_TILE * Q + q] = tot;
        }
    if (q0 == 0) {                                             // alpha: 2 <g2, Psi2>, by the first q chunk
        const double tot = qp_block_sum(2.0 * ((p0[0] + p0[1]) + (p0[2] + p0[3])), red, t);
        if (t == 0) pz[(size_t)2 * QP_TILE * Q + Q] = tot;
    }
}

// qp_param_reduce_kernel with the cells of a kernel's pattern chunks added in chunk order (C = pchunks cells per (slab, k))
__global__ __launch_bounds__(256) void qg_param_reduce_kernel(int K, int M, int Q, int T, int slabs, int C, int slabs1,
                                                              const double *__restrict__ alpha, const double *__restrict__ part,
                                                              const double *__restrict__ part1, double *__restrict__ d_z,
                                                              double *__restrict__ d_gamma, double *__restrict__ d_alpha) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nz = (size_t)K * M * Q, ng = (size_t)K * Q;
    const size_t tiles = (size_t)T * (T + 1) / 2, side = (size_t)QP_TILE * Q, cell = 2 * side + Q + 1, cell1 = side + Q + 1;
    if (e < nz) {
        const int b = (int)(e / ((size_t)M * Q)), rem = (int)(e % ((size_t)M * Q)), m = rem / Q, q = rem % Q;
        const int bm = m / QP_TILE;
        const size_t off = (size_t)(m % QP_TILE) * Q + q;
        double acc = 0.0;
        for (int k = 0; k < slabs; ++k)
            for (int ch = 0; ch < C; ++ch) {
                const size_t base = (((size_t)k * K + b) * C + ch) * tiles;
                for (int i = 0; i <= bm; ++i) {
                    const size_t idx = (size_t)i * T - (size_t)(i * (i - 1) / 2) + (bm - i);
                    acc += part[(base + idx) * cell + side + off];
                }
                const size_t row = (size_t)bm * T - (size_t)(bm * (bm - 1) / 2);
                for (int j = bm; j < T; ++j) acc += part[(base + row + (j - bm)) * cell + off];
            }
        for (int k = 0; k < slabs1; ++k) acc += part1[(((size_t)k * K + b) * T + bm) * cell1 + off];
        d_z[e] = acc;
    } else if (e < nz + ng + K) {                              // d_gamma[k][q], then d_alpha[k] (times alpha: the last entry)
        const bool isa = e >= nz + ng;
        const int b = isa ? (int)(e - nz - ng) : (int)((e - nz) / Q);
        const size_t off = 2 * side + (isa ? (size_t)Q : (e - nz) % Q);
        double acc = 0.0;
        for (int k = 0; k < slabs; ++k)
            for (int ch = 0; ch < C; ++ch)
                for (size_t i = 0; i < tiles; ++i) acc += part[((((size_t)k * K + b) * C + ch) * tiles + i) * cell + off];
        for (int k = 0; k < slabs1; ++k)
            for (int i = 0; i < T; ++i) acc += part1[(((size_t)k * K + b) * T + i) * cell1 + off - side];
        if (isa) d_alpha[b] = acc / alpha[b];
        else d_gamma[e - nz] = acc;
    }
}

// stats: the slot form's plan with B = K ceil(P / PC) workgroup columns
struct QgStatsPlan { int pc, pchunks; QpStatsPlan s; };
QgStatsPlan qg_stats_plan(int K, int P, int N, int M) {
    QgStatsPlan p;
    p.pc = qg_pow2_width(P);
    p.pchunks = dpgp_ceil_div(P, p.pc);
    p.s = qp_stats_plan(K * p.pchunks, N, M);
    return p;
}
size_t qg_stats_lds(int Q, int pc) { return qp_stats_lds(Q) + sizeof(double) * QP_SN * pc; }

// adjoint: the widest pattern chunk of {8, 4, 2, 1} (not wider than P needs) whose H tiles fit beside one wave's points, then
// the most waves of {4, 2, 1} (not more than N needs) that still fit:  Q <= 46: PC 8;  Q <= 63: PC 4;  Q = 64: PC 2.
// With PC = 8: NW 4 for Q <= 14, 2 for Q <= 26, else 1.
size_t qg_adj_lds(int Q, int pc, int nw) {
    return sizeof(double) * ((size_t)3 * Q * QP_NT * nw + (size_t)2 * QP_TILE * Q + (size_t)pc * QP_TILE * QP_HSTRIDE + Q);
}
struct QgAdjPlan { int pc, pchunks, nw, T, tiles, nt, qchunks, slabs, tiles_per_slab; };
QgAdjPlan qg_adj_plan(int K, int P, int N, int M, int Q) {
    QgAdjPlan p;
    p.pc = qg_pow2_width(P);
    while (p.pc > 1 && qg_adj_lds(Q, p.pc, 1) > QG_LDS_BUDGET) p.pc /= 2;
    p.pchunks = dpgp_ceil_div(P, p.pc);
    p.nw = N > 2 * QP_NT ? 4 : N > QP_NT ? 2 : 1;
    while (p.nw > 1 && qg_adj_lds(Q, p.pc, p.nw) > QG_LDS_BUDGET) p.nw /= 2;
    p.T = dpgp_ceil_div(M, QP_TILE);
    p.tiles = qp_tiles(M);
    p.nt = dpgp_ceil_div(N, QP_NT * p.nw);
    p.qchunks = dpgp_ceil_div(Q, QP_QCHUNK);
    const long base = (long)p.nt * K * p.qchunks * p.pchunks;
    int sl = (int)((QP_TARGET_WGS + base - 1) / base);
    if (const int v = dpgp_env_plan("DPGP_QP_PAIR_SLABS", 1, p.tiles)) sl = v;
    sl = sl < 1 ? 1 : (sl > p.tiles ? p.tiles : sl);
    p.tiles_per_slab = dpgp_ceil_div(p.tiles, sl);
    p.slabs = dpgp_ceil_div(p.tiles, p.tiles_per_slab);
    return p;
}

struct QgParamPlan { int pc, pchunks; QpParamPlan s; };
QgParamPlan qg_param_plan(int K, int P, int N, int M, int Q) {
    QgParamPlan p;
    p.pc = qg_pow2_width(P);
    p.pchunks = dpgp_ceil_div(P, p.pc);
    p.s = qp_param_plan(K * p.pchunks, N, M, Q);                // (Psi2 term: K pchunks workgroup columns)
    const QpParamPlan k1 = qp_param_plan(K, N, M, Q);           // (Psi1 term: once per kernel)
    p.s.slabs1 = k1.slabs1;
    p.s.n_per_slab1 = k1.n_per_slab1;
    return p;
}
size_t qg_param_lds(int Q, int pc) { return qp_param_lds(Q) + sizeof(double) * QP_SN * pc; }

template <int PC>
int qg_launch_psi2(const QgStatsPlan &p, int K, int P, int N, int M, int Q, const double *z, const double *mu, const double *s,
                   const double *gamma, const double *alpha, const double *zfac, const double *wt, double *part, hipStream_t st) {
    const size_t lds = qg_stats_lds(Q, PC);
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(qg_psi2_kernel<PC>), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL((qg_psi2_kernel<PC>), dim3(p.s.tiles, p.s.slabs, K * p.pchunks), dim3(256), lds, st, P, N, M, Q, p.s.T,
                       p.s.n_per_slab, p.pchunks, z, mu, s, gamma, alpha, zfac, wt, part);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

template <int KQ, int PC>
int qg_launch_adjoint(const QgAdjPlan &p, int K, int P, int N, int M, int Q, const double *z, const double *mu, const double *s,
                      const double *gamma, const double *alpha, const double *zfac, const double *wt, const double *g1,
                      const double *g2, double *part, hipStream_t st) {
    const size_t lds = qg_adj_lds(Q, PC, p.nw);
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(qg_adjoint_kernel<KQ, PC>), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL((qg_adjoint_kernel<KQ, PC>), dim3(p.nt, p.slabs, K * p.qchunks * p.pchunks), dim3(QP_NT * p.nw), lds, st,
                       K, P, N, M, Q, p.T, p.tiles_per_slab, p.pchunks, z, mu, s, gamma, alpha, zfac, wt, g1, g2, part);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

template <int PC>
int qg_dispatch_adjoint(const QgAdjPlan &p, int K, int P, int N, int M, int Q, const double *z, const double *mu,
                        const double *s, const double *gamma, const double *alpha, const double *zfac, const double *wt,
                        const double *g1, const double *g2, double *part, hipStream_t st) {
    const int w = Q < QP_QCHUNK ? Q : QP_QCHUNK;
    return w <= 1   ? qg_launch_adjoint<1, PC>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g1, g2, part, st)
           : w <= 2 ? qg_launch_adjoint<2, PC>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g1, g2, part, st)
           : w <= 4 ? qg_launch_adjoint<4, PC>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g1, g2, part, st)
                    : qg_launch_adjoint<8, PC>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g1, g2, part, st);
}

template <int KQ, int PC>
int qg_launch_param(const QgParamPlan &p, int K, int P, int N, int M, int Q, const double *z, const double *mu, const double *s,
                    const double *gamma, const double *alpha, const double *zfac, const double *wt, const double *g2,
                    double *part, hipStream_t st) {
    const size_t lds = qg_param_lds(Q, PC);
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(qg_param_kernel<KQ, PC>), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL((qg_param_kernel<KQ, PC>), dim3(p.s.tiles, p.s.slabs, K * p.s.qchunks * p.pchunks), dim3(256), lds, st, K,
                       P, N, M, Q, p.s.T, p.s.n_per_slab, p.pchunks, z, mu, s, gamma, alpha, zfac, wt, g2, part);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

template <int PC>
int qg_dispatch_param(const QgParamPlan &p, int K, int P, int N, int M, int Q, const double *z, const double *mu, const double *s,
                      const double *gamma, const double *alpha, const double *zfac, const double *wt, const double *g2,
                      double *part, hipStream_t st) {
    return Q <= 1   ? qg_launch_param<1, PC>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g2, part, st)
           : Q <= 2 ? qg_launch_param<2, PC>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g2, part, st)
                    : qg_launch_param<QP_PCHUNK, PC>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, wt, g2, part, st);
}

bool qg_shape_ok(int K, int P, int N, int M, int Q) {
    return P >= 1 && qp_shape_ok(K, N, M, Q) && (long)K * P <= 0x7fffffffL / 2;
}

// the checks shared by the three grouped entry points: K -1, P -2, N -3, M -4, Q -5, z -6, mu -7, s -8, gamma -9, alpha -10,
// (zfac: nullable, no code), w -12
int qg_check_common(int K, int P, int N, int M, int Q, const double *z, const double *mu, const double *s, const double *gamma,
                    const double *alpha, const double *wt) {
    if (K < 1) return -1;
    if (P < 1 || (long)K * P > 0x7fffffffL / 2) return -2;
    if (N < 1) return -3;
    if (M < 1) return -4;
    if (Q < 1 || Q > DPGP_QX_PSI_MAX_Q) return -5;
    if (!z) return -6;
    if (!mu) return -7;
    if (!s) return -8;
    if (!gamma) return -9;
    if (!alpha) return -10;
    if (!wt) return -12;
    return 0;
}

}  // namespace

extern "C" size_t dpgp_qx_psi_stats_grouped_workspace_bytes(int K, int P, int N, int M, int Q) {
    if (!qg_shape_ok(K, P, N, M, Q)) return 0;
    const QgStatsPlan p = qg_stats_plan(K, P, N, M);
    return sizeof(double) * (size_t)p.s.slabs * K * P * M * M;
}

extern "C" int dpgp_qx_psi_stats_grouped_f64(int K, int P, int N, int M, int Q, const double *z, const double *mu,
                                             const double *s, const double *gamma, const double *alpha, const double *zfac,
                                             const double *w, double *psi1, double *psi2, void *ws, size_t ws_bytes,
                                             void *stream) {
    if (const int rc = qg_check_common(K, P, N, M, Q, z, mu, s, gamma, alpha, w)) return rc;
    if (!psi1) return -13;
    if (!psi2) return -14;
    if (!ws) return -15;
    if (ws_bytes < dpgp_qx_psi_stats_grouped_workspace_bytes(K, P, N, M, Q)) return -16;
    hipStream_t st = (hipStream_t)stream;
    const QgStatsPlan p = qg_stats_plan(K, P, N, M);
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(qp_psi1_kernel, dim3((unsigned)(((size_t)N * M + 255) / 256), K), dim3(256), 0, st, N, M, Q, z, mu, s,
                       gamma, alpha, psi1);
    DPGP_LAUNCH_CHECK();
    double *part = static_cast<double *>(ws);
    const int rc = p.pc == 1   ? qg_launch_psi2<1>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, w, part, st)
                   : p.pc == 2 ? qg_launch_psi2<2>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, w, part, st)
                   : p.pc == 4 ? qg_launch_psi2<4>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, w, part, st)
                               : qg_launch_psi2<8>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, w, part, st);
    if (rc) return rc;
    const size_t tot = (size_t)K * P * M * M;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(qp_psi2_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, K * P, M, p.s.slabs, part,
                       psi2);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

extern "C" size_t dpgp_qx_psi_adjoint_grouped_workspace_bytes(int K, int P, int N, int M, int Q) {
    if (!qg_shape_ok(K, P, N, M, Q)) return 0;
    const QgAdjPlan p = qg_adj_plan(K, P, N, M, Q);
    return sizeof(double) * (size_t)p.slabs * K * p.pchunks * 2 * Q * N;
}

extern "C" int dpgp_qx_psi_adjoint_grouped_f64(int K, int P, int N, int M, int Q, const double *z, const double *mu,
                                               const double *s, const double *gamma, const double *alpha, const double *zfac,
                                               const double *w, const double *g1, const double *g2, double *d_mu, double *d_s,
                                               void *ws, size_t ws_bytes, void *stream) {
    if (const int rc = qg_check_common(K, P, N, M, Q, z, mu, s, gamma, alpha, w)) return rc;
    if (!g1) return -13;
    if (!g2) return -14;
    if (!d_mu) return -15;
    if (!d_s) return -16;
    if (!ws) return -17;
    if (ws_bytes < dpgp_qx_psi_adjoint_grouped_workspace_bytes(K, P, N, M, Q)) return -18;
    hipStream_t st = (hipStream_t)stream;
    const QgAdjPlan p = qg_adj_plan(K, P, N, M, Q);
    double *part = static_cast<double *>(ws);
    const int rc = p.pc == 1   ? qg_dispatch_adjoint<1>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, w, g1, g2, part, st)
                   : p.pc == 2 ? qg_dispatch_adjoint<2>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, w, g1, g2, part, st)
                   : p.pc == 4 ? qg_dispatch_adjoint<4>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, w, g1, g2, part, st)
                               : qg_dispatch_adjoint<8>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, w, g1, g2, part, st);
    if (rc) return rc;
    const size_t tot = (size_t)2 * Q * N;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(qp_adjoint_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, K * p.pchunks, N, Q,
                       p.slabs, part, d_mu, d_s);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

extern "C" size_t dpgp_qx_psi_param_adjoint_grouped_workspace_bytes(int K, int P, int N, int M, int Q) {
    if (!qg_shape_ok(K, P, N, M, Q)) return 0;
    const QgParamPlan p = qg_param_plan(K, P, N, M, Q);
    return sizeof(double) * ((size_t)p.s.slabs * K * p.pchunks * p.s.tiles * qp_param_part_elems(Q) +
                             (size_t)p.s.slabs1 * K * p.s.T * qp_param_part1_elems(Q));
}

extern "C" int dpgp_qx_psi_param_adjoint_grouped_f64(int K, int P, int N, int M, int Q, const double *z, const double *mu,
                                                     const double *s, const double *gamma, const double *alpha,
                                                     const double *zfac, const double *w, const double *g1, const double *g2,
                                                     double *d_z, double *d_gamma, double *d_alpha, void *ws, size_t ws_bytes,
                                                     void *stream) {
    if (const int rc = qg_check_common(K, P, N, M, Q, z, mu, s, gamma, alpha, w)) return rc;
    if (!g1) return -13;
    if (!g2) return -14;
    if (!d_z) return -15;
    if (!d_gamma) return -16;
    if (!d_alpha) return -17;
    if (!ws) return -18;
    if (ws_bytes < dpgp_qx_psi_param_adjoint_grouped_workspace_bytes(K, P, N, M, Q)) return -19;
    hipStream_t st = (hipStream_t)stream;
    const QgParamPlan p = qg_param_plan(K, P, N, M, Q);
    double *part = static_cast<double *>(ws);
    double *part1 = part + (size_t)p.s.slabs * K * p.pchunks * p.s.tiles * qp_param_part_elems(Q);
    const int rc = p.pc == 1   ? qg_dispatch_param<1>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, w, g2, part, st)
                   : p.pc == 2 ? qg_dispatch_param<2>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, w, g2, part, st)
                   : p.pc == 4 ? qg_dispatch_param<4>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, w, g2, part, st)
                               : qg_dispatch_param<8>(p, K, P, N, M, Q, z, mu, s, gamma, alpha, zfac, w, g2, part, st);
    if (rc) return rc;
    const size_t lds1 = qp_param_psi1_lds(Q);
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(qp_param_psi1_kernel), lds1)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(qp_param_psi1_kernel, dim3(p.s.T, p.s.slabs1, K), dim3(256), lds1, st, K, N, M, Q, p.s.n_per_slab1, z, mu,
                       s, gamma, alpha, g1, part1);
    DPGP_LAUNCH_CHECK();
    const size_t tot = (size_t)K * M * Q + (size_t)K * Q + K;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(qg_param_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, K, M, Q, p.s.T, p.s.slabs,
                       p.pchunks, p.s.slabs1, alpha, part, part1, d_z, d_gamma, d_alpha);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}
