// Per-point Psi2 contractions for K ARD-RBF kernels that each have their own inducing inputs (the predictive moments of the
// over-T model at a test-point q(X*)).  With psi2_kn[m,m'] test point n's own term of kernel k's Psi2 (what qp_psi2_kernel of
// qx_psi.hip sums over n, pair factor F included; symbols in that file's header):
//   tr[k][n][g]   = sum_{m,m'} c_kg[m,m'] psi2_kn[m,m']                 c[K][G][M][M], any matrices
//   quad[k][n][j] = sum_{m,m'} r_k[m,j] r_k[m',j] psi2_kn[m,m']         r[K][M][J]
// Both are one product E[N x pairs] W[pairs x (G + J)] per kernel.  A pair m <= m' is visited once:
//   E_n[pair] = c2_n exp(-sum_q iw2_nq (mu_nq - zbar_q)^2)      (d formed directly, no expansion of the square)
//   W[pair][g]     = F (c_g[m,m'] + c_g[m',m]),  on the diagonal F c_g[m,m]
//   W[pair][G + j] = 2 F r[m,j] r[m',j],          on the diagonal F r[m,j]^2
// E is never stored: it is made on the fly as the A operand of v_mfma_f64_16x16x4 (Mfma<double>).
//
// Layout.  Workgroup (block of 64 test points, column chunk, kernel k; slab of pair tiles), 256 threads = 4 waves; a wave owns 16
// points (the rows of the MFMA tile) and CT <= 8 column tiles of 16 as accumulators (8 x f64x4 = 64 VGPRs: the chunk is 128 columns
// wide, 64 wide for Q > 32 where the LDS does not hold more).  Pairs are visited as in qx_psi.hip: 32 x 32 tiles (I, J), I <= J, of
// the upper block triangle, and inside a tile one row m at a time (a block of 32 pairs (m, c0 .. c0 + 31)):
//   per tile:   the columns' z rows zc [32][Q], the columns' rows of r of the chunk rJ [32][16 CT] and the pair factor sF [32][33]
//               (from zfac when given; 0 for a pair out of range or below the diagonal of a diagonal tile) are staged in LDS;
//   per block:  all threads form zbar [32][Q] and W [32][16 CT] of the block's pairs in LDS (c is read from memory here, each
//               element once per workgroup); then every wave runs the block's 8 steps of 4 pairs: lane (point i = lane & 15,
//               pair kk = lane >> 4) evaluates ONE exponential (dpgp_exp2(double)) and feeds it to the CT MFMAs of the step, so an
//               exponential is evaluated once per (k, n, pair) and per chunk of 16 CT columns, never once per column.  Steps that
//               lie wholly below the diagonal or past M are not run.
// The points' mu and -log2(e) gamma / w2 live in registers for Q <= 16 and in LDS ([Q][64]) above.  A wave whose 16 points are
// all past N only helps to form W.
// LDS: 8 (128 Q + 64 + 64 Q + Q + 1056 + 32 (16 CT + 16) + 512 CT) bytes: 91.8 KiB at Q = 10, CT = 8;  125.0 KiB at Q = 32, CT = 8;
//      141.3 KiB at Q = 64, CT = 4 (the bound is 160 KiB; Q = 64 with CT = 8 would need 173.3 KiB).
// The accumulators go to slab [slab][K][N][G + J] of the workspace (partial sums of the two outputs and nothing else: the pair
// tiles are split over slabs only to fill the GPU when N K is small); a second launch adds the slabs in slab order and splits
// the columns into tr and quad.  No atomics: the same inputs give the same bits.
#include "internal.h"
#include "qx_tile.h"

#define PW_TILE 32
#define PW_NP 64            // test points per workgroup: 4 waves x 16 MFMA rows
#define PW_FSTRIDE (PW_TILE + 1)
#define PW_WPAD 16          // W row stride 16 CT + 16 doubles: the 4 rows of a B operand fall on disjoint halves of the banks
#define PW_QR 16            // Q <= PW_QR: the lane's point in registers
#define PW_TARGET_WGS 512   // (256-thread workgroups: QP_TARGET_WGS / 2 of qx_psi.hip)

namespace {

template <int CT, bool QREG>
__global__ __launch_bounds__(256) void pw_kernel(int K, int G, int J, int N, int M, int Q, int T, int nchunks, int nct_plan,
                                                 int ntn, int tiles_per_slab, const double *__restrict__ z,
                                                 const double *__restrict__ mu, const double *__restrict__ s,
                                                 const double *__restrict__ gamma, const double *__restrict__ alpha,
                                                 const double *__restrict__ zfac, const double *__restrict__ c,
                                                 const double *__restrict__ r, double *__restrict__ part) {
    constexpr int CW = 16 * CT, WS = CW + PW_WPAD, PSTEP = 256 / CW;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *smu = reinterpret_cast<double *>(smem_raw);    // [Q][64]
    double *siw = smu + (size_t)Q * PW_NP;                  // [Q][64]  -log2(e) gamma / w2
    double *sc2 = siw + (size_t)Q * PW_NP;                  // [64]     c2_n, 0 past N
    double *zc = sc2 + PW_NP;                               // [32][Q]  z rows of the tile's columns
    double *zb = zc + (size_t)PW_TILE * Q;                  // [32][Q]  zbar of the block's pairs
    double *gm = zb + (size_t)PW_TILE * Q;                  // [Q]
    double *sF = gm + Q;                                    // [32][33] pair factor of the tile
    double *sW = sF + PW_TILE * PW_FSTRIDE;                 // [32][WS]
    double *rJ = sW + PW_TILE * WS;                         // [32][CW] r rows of the tile's columns (quad columns of the chunk)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, slab = blockIdx.y;
    const int nt = blockIdx.x % ntn, rest = blockIdx.x / ntn, chunk = rest % nchunks, k = rest / nchunks;
    const int C = G + J, tiles16 = (C + 15) / 16;
    const int nct = min(nct_plan, tiles16 - chunk * nct_plan), col0 = 16 * chunk * nct_plan;
    const int n0 = nt * PW_NP;
    const double *zk = z + (size_t)k * M * Q, *gk = gamma + (size_t)k * Q;
    const double *rk = r + (size_t)k * M * J, *zf = zfac ? zfac + (size_t)k * M * M : nullptr;
    const double al = alpha[k];
    for (int e = t; e < PW_NP * Q; e += 256) {
        const int i = e / Q, q = e % Q;
        const bool live = n0 + i < N;
        const double g = gk[q], sv = live ? s[(size_t)n0 * Q + e] : 0.0;
        smu[q * PW_NP + i] = live ? mu[(size_t)n0 * Q + e] : 0.0;
        siw[q * PW_NP + i] = live ? -DPGP_LOG2E * g / fma(2.0 * g, sv, 1.0) : 0.0;
    }
    if (t < PW_NP) {
        double v = 0.0;
        if (n0 + t < N) {
            const double *sn = s + (size_t)(n0 + t) * Q;
            double l = 0.0;
            for (int q = 0; q < Q; ++q) l += log(fma(2.0 * gk[q], sn[q], 1.0));
            v = exp(-0.5 * l);
        }
        sc2[t] = v;
    }
    for (int q = t; q < Q; q += 256) gm[q] = gk[q];
    __syncthreads();
    const int pi = wave * 16 + (lane & 15), kk = lane >> 4;
    const bool wave_live = n0 + wave * 16 < N;
    const double c2 = sc2[pi];
    double pm[QREG ? PW_QR : 1], pw[QREG ? PW_QR : 1];
    if (QREG) {
#pragma unroll
        for (int q = 0; q < PW_QR; ++q) {
            pm[q] = q < Q ? smu[q * PW_NP + pi] : 0.0;
            pw[q] = q < Q ? siw[q * PW_NP + pi] : 0.0;
        }
    }
    f64x4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
    // the thread's element of W: column col_l of the chunk, pairs prow, prow + PSTEP, ..
    const int col_l = t % CW, prow = t / CW, gcol = col0 + col_l;
    const bool col_on = gcol < C && col_l < 16 * nct, col_tr = gcol < G;
    const double *cg = c + ((size_t)k * G + (col_tr ? gcol : 0)) * M * M;
    const int tile_lo = slab * tiles_per_slab, tile_hi = min(T * (T + 1) / 2, tile_lo + tiles_per_slab);
    for (int tile = tile_lo; tile < tile_hi; ++tile) {
        int I, Jt;
        dpgp_tile_ij(tile, T, I, Jt);
        const bool diag = I == Jt;
        const int m0 = I * PW_TILE, c0 = Jt * PW_TILE;
        const int nr = min(PW_TILE, M - m0), nc = min(PW_TILE, M - c0);
        __syncthreads();                                       // (previous tile done with zc / sF / rJ / sW / zb)
        for (int e = t; e < PW_TILE * Q; e += 256) zc[e] = e / Q < nc ? zk[(size_t)c0 * Q + e] : 0.0;
        for (int e = t; e < PW_TILE * CW; e += 256) {
            const int p = e / CW, cl = e % CW, gc = col0 + cl;
            rJ[e] = (p < nc && gc >= G && gc < C && cl < 16 * nct) ? rk[(size_t)(c0 + p) * J + (gc - G)] : 0.0;
        }
        for (int e = t; e < PW_TILE * PW_TILE; e += 256) {
            const int rr = e / PW_TILE, cc = e % PW_TILE, m = m0 + rr, mp = c0 + cc;
            double f = 0.0;
            if (rr < nr && cc < nc && (!diag || cc >= rr)) f = dpgp_pair_factor(zf, M, Q, m, mp, zk, gm, al);
            sF[rr * PW_FSTRIDE + cc] = f;
        }
        for (int rr = 0; rr < nr; ++rr) {
            const int m = m0 + rr;
            __syncthreads();                                   // (the tile's staging is visible; previous block's W / zbar consumed)
            for (int e = t; e < PW_TILE * Q; e += 256) zb[e] = 0.5 * (zk[(size_t)m * Q + e % Q] + zc[e]);
            {
                const double rm = (col_on && !col_tr) ? rk[(size_t)m * J + (gcol - G)] : 0.0;
                for (int p = prow; p < PW_TILE; p += PSTEP) {
                    const double f = sF[rr * PW_FSTRIDE + p];
                    double w = 0.0;
                    if (col_on && f != 0.0) {
                        const int mp = c0 + p;
                        if (col_tr) w = f * (m == mp ? cg[(size_t)m * M + m] : cg[(size_t)m * M + mp] + cg[(size_t)mp * M + m]);
                        else w = (m == mp ? f : 2.0 * f) * rm * rJ[p * CW + col_l];
                    }
                    sW[p * WS + col_l] = w;
                }
            }
            __syncthreads();
            if (!wave_live) continue;                          // (wave-uniform)
            const int s_lo = diag ? rr >> 2 : 0, s_hi = (nc + 3) >> 2;
            for (int st = s_lo; st < s_hi; ++st) {
                const int cc = 4 * st + kk;
                const double *zq = zb + (size_t)cc * Q;
                double e = 0.0;
                if (QREG) {
#pragma unroll
                    for (int q = 0; q < PW_QR; ++q)
                        if (q < Q) {
                            const double d = pm[q] - zq[q];
                            e = fma(pw[q] * d, d, e);
                        }
                } else {
                    for (int q = 0; q < Q; ++q) {
                        const double d = smu[q * PW_NP + pi] - zq[q];
                        e = fma(siw[q * PW_NP + pi] * d, d, e);
                    }
                }
                const double a = c2 * dpgp_exp2(e);
                const double *wrow = sW + cc * WS + (lane & 15);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
                    if (ct < nct) acc[ct] = Mfma<double>::mma(a, wrow[16 * ct], acc[ct]);
            }
        }
    }
    if (!wave_live) return;
    double *pb = part + ((size_t)slab * K + k) * N * C;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
        if (ct < nct) {
            const int col = col0 + 16 * ct + (lane & 15);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int n = n0 + wave * 16 + Mfma<double>::row(lane, rr);
                if (n < N && col < C) pb[(size_t)n * C + col] = acc[ct][rr];
            }
        }
}

// tr[k][n][g], quad[k][n][j]: the slabs added in slab order, the columns split
__global__ __launch_bounds__(256) void pw_reduce_kernel(int K, int G, int J, int N, int slabs, const double *__restrict__ part,
                                                        double *__restrict__ tr, double *__restrict__ quad) {
    const size_t C = (size_t)G + J, tot = (size_t)K * N * C;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= tot) return;
    double acc = 0.0;
    for (int sl = 0; sl < slabs; ++sl) acc += part[(size_t)sl * tot + e];
    const size_t kn = e / C;
    const int col = (int)(e % C);
    if (col < G) tr[kn * G + col] = acc;
    else quad[kn * J + (col - G)] = acc;
}

struct PwPlan { int T, tiles, ntn, nchunks, nct, ct, slabs, tiles_per_slab; };

// Tests and experiments: DPGP_PW_PAIR_SLABS forces the number of pair-tile slabs (clamped to the tiles; unset or < 1: the plan's own).
// It is read on every plan, so the workspace queries and the launches agree; the moments operator plans through the same function.

PwPlan pw_plan(int K, int G, int J, int N, int M, int Q) {
    PwPlan p;
    p.T = dpgp_ceil_div(M, PW_TILE);
    p.tiles = p.T * (p.T + 1) / 2;
    p.ntn = dpgp_ceil_div(N, PW_NP);
    const int tiles16 = (int)(((long)G + J + 15) / 16), ctmax = Q <= 32 ? 8 : 4;
    p.nct = dpgp_ceil_div(tiles16, dpgp_ceil_div(tiles16, ctmax));      // chunks of equal width
    p.nchunks = dpgp_ceil_div(tiles16, p.nct);
    p.ct = p.nct <= 1 ? 1 : p.nct <= 2 ? 2 : p.nct <= 4 ? 4 : 8;
    const long base = (long)p.ntn * K * p.nchunks;
    long sl = (PW_TARGET_WGS + base - 1) / base;
    if (const int v = dpgp_env_plan("DPGP_PW_PAIR_SLABS", 1, p.tiles)) sl = v;
    sl = sl < 1 ? 1 : (sl > p.tiles ? p.tiles : sl);
    p.tiles_per_slab = dpgp_ceil_div(p.tiles, (int)sl);
    p.slabs = dpgp_ceil_div(p.tiles, p.tiles_per_slab);
    return p;
}

size_t pw_lds(int Q, int ct) {
    return sizeof(double) * ((size_t)2 * Q * PW_NP + PW_NP + (size_t)2 * PW_TILE * Q + Q + PW_TILE * PW_FSTRIDE +
                             (size_t)PW_TILE * (16 * ct + PW_WPAD) + (size_t)PW_TILE * 16 * ct);
}

// K, G, J, N, M >= 1, 1 <= Q <= 64, and sizes that the 32-bit grid and the int indices of the plan hold
bool pw_shape_ok(int K, int G, int J, int N, int M, int Q) {
    if (K < 1 || G < 1 || J < 1 || N < 1 || M < 1 || Q < 1 || Q > DPGP_QX_PSI_MAX_Q) return false;
    if ((long)G + J > 0x7fffffffL / 2 || M > 46000) return false;
    const long wgs = (long)dpgp_ceil_div(N, PW_NP) * K * (((long)G + J + 15) / 16);
    return wgs <= 0x7fffffffL / 2;
}

template <int CT, bool QREG>
int pw_launch(const PwPlan &p, int K, int G, int J, int N, int M, int Q, const double *z, const double *mu, const double *s,
              const double *gamma, const double *alpha, const double *zfac, const double *c, const double *r, double *part,
              hipStream_t st) {
    const size_t lds = pw_lds(Q, CT);
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(pw_kernel<CT, QREG>), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL((pw_kernel<CT, QREG>), dim3((unsigned)((long)p.ntn * p.nchunks * K), p.slabs), dim3(256), lds, st, K, G, J, N,
                       M, Q, p.T, p.nchunks, p.nct, p.ntn, p.tiles_per_slab, z, mu, s, gamma, alpha, zfac, c, r, part);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

template <bool QREG>
int pw_dispatch(const PwPlan &p, int K, int G, int J, int N, int M, int Q, const double *z, const double *mu, const double *s,
                const double *gamma, const double *alpha, const double *zfac, const double *c, const double *r, double *part,
                hipStream_t st) {
    return p.ct == 1   ? pw_launch<1, QREG>(p, K, G, J, N, M, Q, z, mu, s, gamma, alpha, zfac, c, r, part, st)
           : p.ct == 2 ? pw_launch<2, QREG>(p, K, G, J, N, M, Q, z, mu, s, gamma, alpha, zfac, c, r, part, st)
           : p.ct == 4 ? pw_launch<4, QREG>(p, K, G, J, N, M, Q, z, mu, s, gamma, alpha, zfac, c, r, part, st)
                       : pw_launch<8, QREG>(p, K, G, J, N, M, Q, z, mu, s, gamma, alpha, zfac, c, r, part, st);
}

// ---- per-entry moments (dpgp_qx_psi_point_moments_f64): the second launch of the operator above replaced by one that also forms
// the psi1 . r term and finishes.  Workgroup (block of 64 points, chunk of columns j, kernel k), 256 threads; psi1's exponentials
// are made on the fly, 32 inducing points at a time (their z rows and rows of r staged in LDS), and never stored to memory:
//   mean[k][n][j] = sum_m psi1_kn[m] r_k[m,j],  psi1_kn[m] = alpha_k prod_q (gamma_q s_nq + 1)^-1/2 exp(-gamma_q (mu_nq - z_mq)^2 / (2 (gamma_q s_nq + 1)))
//   var[k][n][j]  = alpha_k + 1/beta_k - tr[gidx[k][j]] + quad[j] - mean^2,   tr / quad: pw_kernel's slab partials added in slab order
// J >= 16 (pm_finish_mfma_kernel): the [64 x 32] [32 x 16 FT] product runs on v_mfma_f64_16x16x4 as in pw_kernel: a wave owns 16
// points and FT <= 4 column tiles, lane (point i, m = 4 step + (lane >> 4)) evaluates one exponential per step as the A operand.
// J < 16 (pm_finish_fma_kernel): a tile of 16 columns would be mostly padding; the psi1 tile [64][32] goes through LDS and thread
// (point, column group) runs plain FMAs over its <= 4 columns.  Both sum over m in ascending order and use no atomics.
#define PM_MAXFT 4

// the points' mu, -log2(e) gamma / (2 (gamma s + 1)) and alpha prod_q (gamma s + 1)^-1/2 (0 past N) of the block into LDS
__device__ __forceinline__ void pm_stage_points(int t, int n0, int N, int Q, double al, const double *__restrict__ gk,
                                                const double *__restrict__ mu, const double *__restrict__ s, double *smu,
                                                double *siw, double *sc1) {
    for (int e = t; e < PW_NP * Q; e += 256) {
        const int i = e / Q, q = e % Q;
        const bool live = n0 + i < N;
        const double g = gk[q], sv = live ? s[(size_t)n0 * Q + e] : 0.0;
        smu[q * PW_NP + i] = live ? mu[(size_t)n0 * Q + e] : 0.0;
        siw[q * PW_NP + i] = live ? -0.5 * DPGP_LOG2E * g / fma(g, sv, 1.0) : 0.0;
    }
    if (t < PW_NP) {
        double v = 0.0;
        if (n0 + t < N) {
            const double *sn = s + (size_t)(n0 + t) * Q;
            double l = 0.0;
            for (int q = 0; q < Q; ++q) l += log(fma(gk[q], sn[q], 1.0));
            v = al * exp(-0.5 * l);
        }
        sc1[t] = v;
    }
}

// one entry: the slabs added in slab order, the trace term gathered (none for gidx outside [0, G)), the terms combined
__device__ __forceinline__ void pm_finish_entry(int G, int J, int N, int K, int slabs, int k, int n, int j, double base,
                                                double mean_v, const int *__restrict__ gidx, const double *__restrict__ part,
                                                double *__restrict__ mean, double *__restrict__ var) {
    const size_t C = (size_t)G + J, tot = (size_t)K * N * C, row = ((size_t)k * N + n) * C;
    const int g = gidx[(size_t)k * J + j];
    double quad = 0.0, tr = 0.0;
    for (int sl = 0; sl < slabs; ++sl) quad += part[(size_t)sl * tot + row + G + j];
    if ((unsigned)g < (unsigned)G)
        for (int sl = 0; sl < slabs; ++sl) tr += part[(size_t)sl * tot + row + g];
    const size_t o = ((size_t)k * N + n) * J + j;
    mean[o] = mean_v;
    var[o] = base - tr + quad - mean_v * mean_v;
}

template <int FT>
__global__ __launch_bounds__(256) void pm_finish_mfma_kernel(int K, int G, int J, int N, int M, int Q, int ntn, int nchunks,
                                                             int nft_plan, int slabs, const double *__restrict__ z,
                                                             const double *__restrict__ mu, const double *__restrict__ s,
                                                             const double *__restrict__ gamma, const double *__restrict__ alpha,
                                                             const double *__restrict__ r, const int *__restrict__ gidx,
                                                             const double *__restrict__ beta, const double *__restrict__ part,
                                                             double *__restrict__ mean, double *__restrict__ var) {
    constexpr int CW = 16 * FT, RS = CW + PW_WPAD;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *smu = reinterpret_cast<double *>(smem_raw);    // [Q][64]
    double *siw = smu + (size_t)Q * PW_NP;                  // [Q][64]
    double *sc1 = siw + (size_t)Q * PW_NP;                  // [64]
    double *zt = sc1 + PW_NP;                               // [32][Q]  z rows of the tile
    double *rT = zt + (size_t)PW_TILE * Q;                  // [32][RS] r rows of the tile, the chunk's columns
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nt = blockIdx.x % ntn, rest = blockIdx.x / ntn, chunk = rest % nchunks, k = rest / nchunks;
    const int tiles16 = (J + 15) / 16, nft = min(nft_plan, tiles16 - chunk * nft_plan), j0 = 16 * chunk * nft_plan;
    const int n0 = nt * PW_NP;
    const double *zk = z + (size_t)k * M * Q, *rk = r + (size_t)k * M * J;
    const double al = alpha[k];
    pm_stage_points(t, n0, N, Q, al, gamma + (size_t)k * Q, mu, s, smu, siw, sc1);
    __syncthreads();
    const int pi = wave * 16 + (lane & 15), kk = lane >> 4;
    const bool wave_live = n0 + wave * 16 < N;
    const double c1 = sc1[pi];
    f64x4 acc[FT];
#pragma unroll
    for (int ct = 0; ct < FT; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int m0 = 0; m0 < M; m0 += PW_TILE) {
        const int nr = min(PW_TILE, M - m0);
        __syncthreads();                                       // (previous tile consumed)
        for (int e = t; e < PW_TILE * Q; e += 256) zt[e] = e / Q < nr ? zk[(size_t)m0 * Q + e] : 0.0;
        for (int e = t; e < PW_TILE * CW; e += 256) {
            const int p = e / CW, cl = e % CW, j = j0 + cl;
            rT[p * RS + cl] = (p < nr && j < J && cl < 16 * nft) ? rk[(size_t)(m0 + p) * J + j] : 0.0;
        }
        __syncthreads();
        if (!wave_live) continue;                              // (wave-uniform)
        for (int st = 0; st < (nr + 3) >> 2; ++st) {
            const int mm = 4 * st + kk;                        // (a row past M: z = 0 gives a finite a, its r row is 0)
            const double *zq = zt + (size_t)mm * Q;
            double e = 0.0;
            for (int q = 0; q < Q; ++q) {
                const double d = smu[q * PW_NP + pi] - zq[q];
                e = fma(siw[q * PW_NP + pi] * d, d, e);
            }
            const double a = c1 * dpgp_exp2(e);
            const double *rrow = rT + mm * RS + (lane & 15);
#pragma unroll
            for (int ct = 0; ct < FT; ++ct)
                if (ct < nft) acc[ct] = Mfma<double>::mma(a, rrow[16 * ct], acc[ct]);
        }
    }
    if (!wave_live) return;
    const double base = al + 1.0 / beta[k];
#pragma unroll
    for (int ct = 0; ct < FT; ++ct)
        if (ct < nft) {
            const int j = j0 + 16 * ct + (lane & 15);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int n = n0 + wave * 16 + Mfma<double>::row(lane, rr);
                if (n < N && j < J) pm_finish_entry(G, J, N, K, slabs, k, n, j, base, acc[ct][rr], gidx, part, mean, var);
            }
        }
}

__global__ __launch_bounds__(256) void pm_finish_fma_kernel(int K, int G, int J, int N, int M, int Q, int ntn, int slabs,
                                                            const double *__restrict__ z, const double *__restrict__ mu,
                                                            const double *__restrict__ s, const double *__restrict__ gamma,
                                                            const double *__restrict__ alpha, const double *__restrict__ r,
                                                            const int *__restrict__ gidx, const double *__restrict__ beta,
                                                            const double *__restrict__ part, double *__restrict__ mean,
                                                            double *__restrict__ var) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *smu = reinterpret_cast<double *>(smem_raw);    // [Q][64]
    double *siw = smu + (size_t)Q * PW_NP;                  // [Q][64]
    double *sc1 = siw + (size_t)Q * PW_NP;                  // [64]
    double *zt = sc1 + PW_NP;                               // [32][Q]
    double *rT = zt + (size_t)PW_TILE * Q;                  // [32][16]  (J < 16)
    double *sP = rT + PW_TILE * 16;                         // [64][33]  psi1 of the tile
    const int t = threadIdx.x, nt = blockIdx.x % ntn, k = blockIdx.x / ntn, n0 = nt * PW_NP;
    const int pt = t & 63, jg = t >> 6;                     // the thread's point and its columns jg, jg + 4, jg + 8, jg + 12
    const double *zk = z + (size_t)k * M * Q, *rk = r + (size_t)k * M * J;
    const double al = alpha[k];
    pm_stage_points(t, n0, N, Q, al, gamma + (size_t)k * Q, mu, s, smu, siw, sc1);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int m0 = 0; m0 < M; m0 += PW_TILE) {
        const int nr = min(PW_TILE, M - m0);
        __syncthreads();                                       // (the points are staged; previous tile consumed)
        for (int e = t; e < PW_TILE * Q; e += 256) zt[e] = e / Q < nr ? zk[(size_t)m0 * Q + e] : 0.0;
        for (int e = t; e < PW_TILE * 16; e += 256) {
            const int p = e >> 4, j = e & 15;
            rT[e] = (p < nr && j < J) ? rk[(size_t)(m0 + p) * J + j] : 0.0;
        }
        __syncthreads();
        for (int e = t; e < PW_NP * PW_TILE; e += 256) {
            const int i = e & 63, p = e >> 6;
            double v = 0.0;
            if (p < nr) {
                const double *zq = zt + (size_t)p * Q;
                double x = 0.0;
                for (int q = 0; q < Q; ++q) {
                    const double d = smu[q * PW_NP + i] - zq[q];
                    x = fma(siw[q * PW_NP + i] * d, d, x);
                }
                v = sc1[i] * dpgp_exp2(x);
            }
            sP[i * PW_FSTRIDE + p] = v;
        }
        __syncthreads();
        for (int p = 0; p < nr; ++p) {
            const double a = sP[pt * PW_FSTRIDE + p];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = fma(a, rT[p * 16 + jg + 4 * i], acc[i]);
        }
    }
    const int n = n0 + pt;
    if (n >= N) return;
    const double base = al + 1.0 / beta[k];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = jg + 4 * i;
        if (j < J) pm_finish_entry(G, J, N, K, slabs, k, n, j, base, acc[i], gidx, part, mean, var);
    }
}

struct PmPlan { int mfma, nft, nchunks, ft; };
PmPlan pm_plan(int J) {
    PmPlan p;
    p.mfma = J >= 16;
    const int tiles16 = dpgp_ceil_div(J, 16);
    p.nft = dpgp_ceil_div(tiles16, dpgp_ceil_div(tiles16, PM_MAXFT));   // chunks of equal width
    p.nchunks = dpgp_ceil_div(tiles16, p.nft);
    p.ft = p.nft <= 1 ? 1 : p.nft <= 2 ? 2 : 4;
    return p;
}

size_t pm_lds(int Q, const PmPlan &p) {
    const size_t pts = (size_t)2 * Q * PW_NP + PW_NP + (size_t)PW_TILE * Q;
    return sizeof(double) * (pts + (p.mfma ? (size_t)PW_TILE * (16 * p.ft + PW_WPAD) : (size_t)PW_TILE * 16 + PW_NP * PW_FSTRIDE));
}

template <typename KERNEL, typename... ARGS>
int pm_launch(KERNEL kernel, unsigned grid, size_t lds, hipStream_t st, ARGS... args) {
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(kernel), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, st, args...);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

}  // namespace

extern "C" size_t dpgp_qx_psi_point_moments_workspace_bytes(int K, int G, int J, int N, int M, int Q) {
    return dpgp_qx_psi_pointwise_workspace_bytes(K, G, J, N, M, Q);     // pw_kernel's slab partials and nothing else
}

extern "C" int dpgp_qx_psi_point_moments_f64(int K, int G, int J, int N, int M, int Q, const double *z, const double *mu,
                                             const double *s, const double *gamma, const double *alpha, const double *zfac,
                                             const double *c, const double *r, const int *gidx, const double *beta, double *mean,
                                             double *var, void *ws, size_t ws_bytes, void *stream) {
    if (K < 1) return -1;
    if (G < 1) return -2;
    if (J < 1) return -3;
    if (N < 1) return -4;
    if (M < 1) return -5;
    if (Q < 1 || Q > DPGP_QX_PSI_MAX_Q) return -6;
    if (!z) return -7;
    if (!mu) return -8;
    if (!s) return -9;
    if (!gamma) return -10;
    if (!alpha) return -11;
    if (!c) return -13;
    if (!r) return -14;
    if (!gidx) return -15;
    if (!beta) return -16;
    if (!mean) return -17;
    if (!var) return -18;
    if (!ws) return -19;
    const size_t need = dpgp_qx_psi_point_moments_workspace_bytes(K, G, J, N, M, Q);
    if (need == 0 || ws_bytes < need) return -20;
    hipStream_t st = (hipStream_t)stream;
    const PwPlan p = pw_plan(K, G, J, N, M, Q);
    double *part = static_cast<double *>(ws);
    const int rc = Q <= PW_QR ? pw_dispatch<true>(p, K, G, J, N, M, Q, z, mu, s, gamma, alpha, zfac, c, r, part, st)
                              : pw_dispatch<false>(p, K, G, J, N, M, Q, z, mu, s, gamma, alpha, zfac, c, r, part, st);
    if (rc) return rc;
    const PmPlan f = pm_plan(J);
    const size_t lds = pm_lds(Q, f);
    if (!f.mfma)
        return pm_launch(pm_finish_fma_kernel, (unsigned)((long)p.ntn * K), lds, st, K, G, J, N, M, Q, p.ntn, p.slabs, z, mu, s, gamma,
                         alpha, r, gidx, beta, (const double *)part, mean, var);
    const unsigned grid = (unsigned)((long)p.ntn * f.nchunks * K);
#define PM_MFMA(FT)                                                                                                               \
    pm_launch(pm_finish_mfma_kernel<FT>, grid, lds, st, K, G, J, N, M, Q, p.ntn, f.nchunks, f.nft, p.slabs, z, mu, s, gamma, alpha, r, \
              gidx, beta, (const double *)part, mean, var)
    return f.ft == 1 ? PM_MFMA(1) : f.ft == 2 ? PM_MFMA(2) : PM_MFMA(4);
#undef PM_MFMA
}

extern "C" size_t dpgp_qx_psi_pointwise_workspace_bytes(int K, int G, int J, int N, int M, int Q) {
    if (!pw_shape_ok(K, G, J, N, M, Q)) return 0;
    const PwPlan p = pw_plan(K, G, J, N, M, Q);
    return sizeof(double) * (size_t)p.slabs * K * N * ((size_t)G + J);
}

extern "C" int dpgp_qx_psi_pointwise_f64(int K, int G, int J, int N, int M, int Q, const double *z, const double *mu,
                                         const double *s, const double *gamma, const double *alpha, const double *zfac,
                                         const double *c, const double *r, double *tr, double *quad, void *ws, size_t ws_bytes,
                                         void *stream) {
    if (K < 1) return -1;
    if (G < 1) return -2;
    if (J < 1) return -3;
    if (N < 1) return -4;
    if (M < 1) return -5;
    if (Q < 1 || Q > DPGP_QX_PSI_MAX_Q) return -6;
    if (!z) return -7;
    if (!mu) return -8;
    if (!s) return -9;
    if (!gamma) return -10;
    if (!alpha) return -11;
    if (!c) return -13;
    if (!r) return -14;
    if (!tr) return -15;
    if (!quad) return -16;
    if (!ws) return -17;
    const size_t need = dpgp_qx_psi_pointwise_workspace_bytes(K, G, J, N, M, Q);
    if (need == 0 || ws_bytes < need) return -18;              // (need == 0: a shape past what the launch grid holds)
    hipStream_t st = (hipStream_t)stream;
    const PwPlan p = pw_plan(K, G, J, N, M, Q);
    double *part = static_cast<double *>(ws);
    const int rc = Q <= PW_QR ? pw_dispatch<true>(p, K, G, J, N, M, Q, z, mu, s, gamma, alpha, zfac, c, r, part, st)
                              : pw_dispatch<false>(p, K, G, J, N, M, Q, z, mu, s, gamma, alpha, zfac, c, r, part, st);
    if (rc) return rc;
    const size_t tot = (size_t)K * N * ((size_t)G + J);
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(pw_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, K, G, J, N, p.slabs, part, tr, quad);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}
