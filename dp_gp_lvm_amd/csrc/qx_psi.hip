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
// No atomics anywhere: the same inputs give the same bits.
//
// Weighted forms (per-entry observation masks): wt [B][N] multiplies test point n's Psi2 term of kernel b (c2_n in both
// kernels); Psi1 and its adjoint are not weighted.  The kernels are templated on WEIGHTED: the unweighted instantiations
// are the code of the unweighted entry points, and wt == NULL runs them.  A point of weight 0 costs no exponential: the
// stats kernel skips it in its staged-point loop (a workgroup-uniform branch on the staged weight), the adjoint skips a
// tile's pair loop when all 64 points of the wave have weight 0 for kernel b.  Either way its contribution is exactly 0.
#include "internal.h"

#define QP_TILE 32
#define QP_HSTRIDE (QP_TILE + 1)
#define QP_NT 64           // test points per adjoint workgroup (one wave)
#define QP_SN 32           // test points staged per step of the stats kernel
#define QP_QCHUNK 8        // latent dims per adjoint accumulator chunk
#define QP_TARGET_WGS 1024

namespace {

int qp_tiles(int M) { const int t = dpgp_ceil_div(M, QP_TILE); return t * (t + 1) / 2; }

// tile index -> (I, J), I <= J, row-major over the upper block triangle
__device__ __forceinline__ void qp_tile_ij(int idx, int T, int &I, int &J) {
    int i = 0;
    while (idx >= T - i) { idx -= T - i; ++i; }
    I = i;
    J = i + idx;
}

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
    qp_tile_ij(blockIdx.x, T, I, J);
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
        qp_tile_ij(tile, T, I, J);
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

struct QpStatsPlan { int T, tiles, slabs, n_per_slab; };
QpStatsPlan qp_stats_plan(int B, int N, int M) {
    QpStatsPlan p;
    p.T = dpgp_ceil_div(M, QP_TILE);
    p.tiles = qp_tiles(M);
    const int chunks = dpgp_ceil_div(N, QP_SN);
    int sl = dpgp_ceil_div(QP_TARGET_WGS / 2, p.tiles * B);
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
    sl = sl < 1 ? 1 : (sl > p.tiles ? p.tiles : sl);
    p.tiles_per_slab = dpgp_ceil_div(p.tiles, sl);
    p.slabs = dpgp_ceil_div(p.tiles, p.tiles_per_slab);
    return p;
}

size_t qp_stats_lds(int Q) { return sizeof(double) * ((size_t)2 * QP_SN * Q + QP_SN + (size_t)2 * QP_TILE * Q + Q); }
size_t qp_adj_lds(int Q) {
    return sizeof(double) * ((size_t)3 * Q * QP_NT + (size_t)2 * QP_TILE * Q + QP_TILE * QP_HSTRIDE + Q);
}

int qp_set_lds(const void *fn, size_t lds) {
    if (lds > 48 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return DPGP_ERR_LAUNCH;
    return DPGP_OK;
}

template <int KQ, bool WEIGHTED>
int qp_launch_adjoint(const QpAdjPlan &p, int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                      const double *gamma, const double *alpha, const double *zfac, const double *wt, const double *g1,
                      const double *g2, double *part, hipStream_t st) {
    const size_t lds = qp_adj_lds(Q);
    if (qp_set_lds(reinterpret_cast<const void *>(qp_adjoint_kernel<KQ, WEIGHTED>), lds)) return DPGP_ERR_LAUNCH;
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
    if (qp_set_lds(reinterpret_cast<const void *>(qp_psi2_kernel<WEIGHTED>), lds)) return DPGP_ERR_LAUNCH;
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
