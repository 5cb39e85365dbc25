// (d_mu, d_s) of a frozen over-D model's test bound: B ARD-RBF kernels that SHARE the inducing inputs z [M][Q] and q(X*) = (mu, s)
// [N][Q] and differ in (gamma_b, alpha_b), in their zero-filled data column y[:, b] and in the weights w[b][:] of their test points.
// With psi1_bn[m], psi2_bn[m,m'] test point n's own terms of kernel b (rbf_kernel.py:135-199, pair factor included):
//   L = sum_b <g_psi2_b, sum_n w[b][n] psi2_bn> + sum_b g_v_b . (Psi1_b^T y_b),      d_mu = dL/dmu,  d_s = dL/ds  (s: variances)
// Per (b, n) everything is a contraction of the point's exponentials with 1 + 2Q moment columns.  Psi2 part, a pair m <= m' visited
// once, zbar = (z_m + z_m') / 2, g~ = g[m,m'] + g[m',m] (g[m,m] on the diagonal), F = alpha^2 exp(-1/4 sum_q gamma_q (z_mq - z_m'q)^2):
//   E_n[pair] = c2_n exp(-sum_q gr_q (mu_nq - zbar_q)^2),   gr_q = gamma_q / (2 gamma_q s_nq + 1),  c2_n = prod_q (2 gamma_q s_nq + 1)^-1/2
//   W[pair][0] = F g~,   W[pair][1 + q] = F g~ zbar_q,   W[pair][1 + Q + q] = F g~ zbar_q^2          (S0, S1_q, S2_q = E W)
//   d_mu_nq += -2 w gr_q (mu S0 - S1_q),     d_s_nq += w (-gr_q S0 + 2 gr_q^2 (mu^2 S0 - 2 mu S1_q + S2_q))
// Psi1 part, the same product over single inducing points with gr1_q = gamma_q / (gamma_q s_nq + 1), exponent -1/2 sum_q gr1_q
// (mu - z_mq)^2, prefactor alpha prod_q (gamma_q s_nq + 1)^-1/2 and W[m] = g_v[m] (1, z_mq, z_mq^2)  (T0, T1_q, T2_q):
//   d_mu_nq += -y gr1_q (mu T0 - T1_q),      d_s_nq += y/2 (-gr1_q T0 + gr1_q^2 (mu^2 T0 - 2 mu T1_q + T2_q))
// mu and z are taken relative to the workgroup's first test point (the forms above only see mu - z), so the expanded squares lose
// no digits to an offset of the latent space.  For Q <= 16 the exponent itself is expanded the same way, -log2(e) sum_q gr_q
// (mu_q - zbar_q)^2 = e0 + sum_q zbar_q (a_q zbar_q + b_q) with a, b, e0 in registers per (point, column): two FMAs per q and step.
// The exponential is dpgp_exp2_tab (its 64-entry table in LDS).
//
// Layout (that of pw_kernel, qx_psi_point.hip).  Workgroup (block of 64 test points, chunk of moment columns, slab of columns b;
// slab of pair tiles), 256 threads = 4 waves; a wave owns 16 points (the rows of the MFMA tile) and CT <= 8 tiles of 16 moment
// columns as accumulators; 1 + 2Q > 128 (Q = 64) goes in two chunks.  The workgroup walks its columns b in ascending order; per column:
//   the points' gr, prefactor and scale (w, or y/2) are staged in LDS;
//   Psi2: its pair tiles (32 x 32, I <= J, one row m = a block of 32 pairs at a time): F g~ of the tile is staged, all threads
//         form zbar [32][Q] and W [32][16 CT] in LDS, then every wave runs the block's 8 steps of 4 pairs: lane (point lane & 15,
//         pair lane >> 4) evaluates ONE exponential as the A operand of the CT v_mfma_f64_16x16x4 of the step;
//   Psi1 (pair slab 0 only): the same with blocks of 32 inducing points;
//   after either, the wave's moments go through LDS ([64][16 CT + 1], over the staging area) and lane (point, q = lane >> 4 + 4 j)
//   adds the column's contribution to its register accumulators of (d_mu, d_s).
// A wave whose points all have scale 0 for a column (w = 0, or y = 0) skips the column's steps and its contribution behind one
// wave-uniform branch; a scale of 0 that is not skipped multiplies finite moments: exactly 0.0 either way.
// The accumulators go to part[slab][2][N][Q]; a second launch adds the slabs in slab order.  No atomics: the same bits on every run.
#include "internal.h"
#include "qx_tile.h"

#define PL_TILE 32
#define PL_NP 64            // test points per workgroup: 4 waves x 16 MFMA rows
#define PL_FSTRIDE (PL_TILE + 1)
#define PL_WPAD 16          // W row stride 16 CT + 16 doubles (as PW_WPAD)
#define PL_QR 16            // Q <= PL_QR: the lane's point in registers, 4 (d_mu, d_s) accumulators per lane; above: LDS, 16
#define PL_MAXCT 8
#define PL_TARGET_WGS 512

namespace {

struct PlArgs {
    int B, N, M, Q, T, ntn, nchunks, nct, cslabs, cols_per_slab, pslabs, tiles_per_slab, ldy, region;
    const double *z, *mu, *s, *gamma, *alpha, *y, *w, *gv, *g2;
    double *part;
};

template <int CT, bool QREG>
__global__ __launch_bounds__(256) void pl_kernel(const PlArgs a) {
    constexpr int CW = 16 * CT, WS = CW + PL_WPAD, PSTEP = 256 / CW, MS = CW + 1, NQ = QREG ? PL_QR / 4 : DPGP_QX_PSI_MAX_Q / 4;
    const int N = a.N, M = a.M, Q = a.Q;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *smu = reinterpret_cast<double *>(smem_raw);    // [Q][64]  mu - centre
    double *sg = smu + (size_t)Q * PL_NP;                   // [Q][64]  gr (Psi2) / gr1 (Psi1) of the column, 0 past N
    double *sc = sg + (size_t)Q * PL_NP;                    // [64]     prefactor c2_n / alpha c1_n, 0 past N
    double *ssc = sc + PL_NP;                               // [64]     scale: w (Psi2) / y/2 (Psi1), 0 past N
    double *cen = ssc + PL_NP;                              // [Q]      the workgroup's centre: mu of its first point
    double *gm = cen + Q;                                   // [Q]      gamma of the column
    double *zc = gm + Q;                                    // [32][Q]  z rows of the tile's columns, centred
    double *zb = zc + (size_t)PL_TILE * Q;                  // [32][Q]  zbar of the block's pairs, centred
    double *sF = zb + (size_t)PL_TILE * Q;                  // [32][33] F g~ of the tile
    double *sW = sF + PL_TILE * PL_FSTRIDE;                 // [32][WS]
    double *sM = zc;                                        // [64][MS] the waves' moments (over zc .. sW, between the phases)
    double *tab = sM + (size_t)a.region;                    // [64]     2^(j/64) (dpgp_exp2_tab)
    dpgp_exp2_tab_init(tab);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, pslab = blockIdx.y;
    const int nt = blockIdx.x % a.ntn, rest = blockIdx.x / a.ntn, chunk = rest % a.nchunks, cslab = rest / a.nchunks;
    const int C = 1 + 2 * Q, tiles16 = (C + 15) / 16;
    const int nct = min(a.nct, tiles16 - chunk * a.nct), col0 = 16 * chunk * a.nct;
    const int n0 = nt * PL_NP;
    const double *z = a.z;
    for (int q = t; q < Q; q += 256) cen[q] = a.mu[(size_t)n0 * Q + q];
    __syncthreads();
    for (int e = t; e < PL_NP * Q; e += 256) {
        const int i = e / Q, q = e % Q;
        smu[q * PL_NP + i] = n0 + i < N ? a.mu[(size_t)n0 * Q + e] - cen[q] : 0.0;
    }
    const int pi = wave * 16 + (lane & 15), kk = lane >> 4;
    const bool wave_live = n0 + wave * 16 < N;
    double dmu[NQ], dsv[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) dmu[j] = dsv[j] = 0.0;
    // the thread's element of W: moment column col_l of the chunk, pairs prow, prow + PSTEP, ..
    const int col_l = t % CW, prow = t / CW, gcol = col0 + col_l;
    const bool col_on = gcol < C && col_l < 16 * nct;
    const int ctype = gcol == 0 ? 0 : (gcol <= Q ? 1 : 2), cq = gcol == 0 ? 0 : (gcol <= Q ? gcol - 1 : min(gcol - 1 - Q, Q - 1));
    const int b_lo = cslab * a.cols_per_slab, b_hi = min(a.B, b_lo + a.cols_per_slab);
    const int ntile2 = a.T * (a.T + 1) / 2;
    const int tile_lo = pslab * a.tiles_per_slab, tile_hi = min(ntile2, tile_lo + a.tiles_per_slab);
    for (int b = b_lo; b < b_hi; ++b) {
        const double *gk = a.gamma + (size_t)b * Q, *g2b = a.g2 + (size_t)b * M * M, *gvb = a.gv + (size_t)b * M;
        const double al = a.alpha[b];
        for (int ph = 0; ph < (pslab == 0 ? 2 : 1); ++ph) {
            const bool p2 = ph == 0;
            const double k2 = p2 ? 2.0 : 1.0, kexp = p2 ? -DPGP_LOG2E : -0.5 * DPGP_LOG2E;
            __syncthreads();                                   // (previous phase done with sg / sc / ssc / gm and with sM)
            for (int e = t; e < PL_NP * Q; e += 256) {
                const int i = e / Q, q = e % Q;
                const double g = gk[q];
                sg[q * PL_NP + i] = n0 + i < N ? g / fma(k2 * g, a.s[(size_t)n0 * Q + e], 1.0) : 0.0;
            }
            if (t < PL_NP) {
                double sc_ = 0.0;
                const int n = n0 + t;
                if (n < N) sc_ = p2 ? (a.w ? a.w[(size_t)b * N + n] : 1.0) : 0.5 * a.y[(size_t)n * a.ldy + b];
                sc[t] = dpgp_point_prefactor(n, N, Q, gk, a.s, k2, p2 ? 1.0 : al);
                ssc[t] = sc_;
            }
            for (int q = t; q < Q; q += 256) gm[q] = gk[q];
            __syncthreads();
            const double scale = ssc[pi];
            const bool on = wave_live && __any(scale != 0.0);  // (wave-uniform)
            if (!__syncthreads_or(on)) continue;               // (workgroup-uniform: nothing of this column counts here)
            const double c2 = sc[pi];
            DpgpPointExponent<QREG ? PL_QR : 1> ex;            // (Q <= 16: the expanded exponent, two FMAs per q and step)
            if constexpr (QREG) ex.setup(Q, kexp, smu, sg, PL_NP, pi);
            f64x4 acc[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
            const int t_lo = p2 ? tile_lo : 0, t_hi = p2 ? tile_hi : a.T;
            for (int tile = t_lo; tile < t_hi; ++tile) {
                int I = tile, Jt = tile;
                if (p2) dpgp_tile_ij(tile, a.T, I, Jt);
                const bool diag = I == Jt;
                const int m0 = I * PL_TILE, c0 = Jt * PL_TILE;
                const int nr = min(PL_TILE, M - m0), nc = min(PL_TILE, M - c0);
                __syncthreads();                               // (previous tile done with zc / sF / sW / zb)
                for (int e = t; e < PL_TILE * Q; e += 256) zc[e] = e / Q < nc ? z[(size_t)c0 * Q + e] - cen[e % Q] : 0.0;
                if (p2)
                    for (int e = t; e < PL_TILE * PL_TILE; e += 256) {
                        const int rr = e / PL_TILE, cc = e % PL_TILE, m = m0 + rr, mp = c0 + cc;
                        double f = 0.0;
                        if (rr < nr && cc < nc && (!diag || cc >= rr)) {
                            double d2 = 0.0;
                            for (int q = 0; q < Q; ++q) {
                                const double d = z[(size_t)m * Q + q] - z[(size_t)mp * Q + q];
                                d2 = fma(gm[q] * d, d, d2);
                            }
                            f = al * al * exp(-0.25 * d2) * (m == mp ? g2b[(size_t)m * M + m] : g2b[(size_t)m * M + mp] + g2b[(size_t)mp * M + m]);
                        }
                        sF[rr * PL_FSTRIDE + cc] = f;
                    }
                const int nrows = p2 ? nr : 1;
                for (int rr = 0; rr < nrows; ++rr) {
                    const int m = m0 + rr;
                    __syncthreads();                           // (the tile's staging is visible; previous block's W / zbar consumed)
                    if (p2) {
                        for (int e = t; e < PL_TILE * Q; e += 256) zb[e] = 0.5 * ((z[(size_t)m * Q + e % Q] - cen[e % Q]) + zc[e]);
                        const double zm = z[(size_t)m * Q + cq] - cen[cq];
                        for (int p = prow; p < PL_TILE; p += PSTEP) {
                            const double f = sF[rr * PL_FSTRIDE + p], zv = 0.5 * (zm + zc[p * Q + cq]);
                            sW[p * WS + col_l] = col_on ? (ctype == 0 ? f : ctype == 1 ? f * zv : f * zv * zv) : 0.0;
                        }
                    } else {
                        for (int p = prow; p < PL_TILE; p += PSTEP) {
                            const double f = p < nc ? gvb[c0 + p] : 0.0, zv = zc[p * Q + cq];
                            sW[p * WS + col_l] = col_on ? (ctype == 0 ? f : ctype == 1 ? f * zv : f * zv * zv) : 0.0;
                        }
                    }
                    __syncthreads();
                    if (!on) continue;                         // (wave-uniform)
                    const double *zz = p2 ? zb : zc;
                    const int s_lo = (p2 && diag) ? rr >> 2 : 0, s_hi = (nc + 3) >> 2;
                    for (int st = s_lo; st < s_hi; ++st) {
                        const int cc = 4 * st + kk;
                        const double *zq = zz + (size_t)cc * Q;
                        double e = 0.0;
                        if constexpr (QREG) {
                            e = ex.at(Q, zq);
                        } else {
                            for (int q = 0; q < Q; ++q) {
                                const double d = smu[q * PL_NP + pi] - zq[q];
                                e = fma(kexp * sg[q * PL_NP + pi] * d, d, e);
                            }
                        }
                        const double av = c2 * dpgp_exp2_tab(e, tab);
                        const double *wrow = sW + cc * WS + (lane & 15);
#pragma unroll
                        for (int ct = 0; ct < CT; ++ct)
                            if (ct < nct) acc[ct] = Mfma<double>::mma(av, wrow[16 * ct], acc[ct]);
                    }
                }
            }
            // the column's moments -> its contribution to (d_mu, d_s)
            __syncthreads();                                   // (every wave is done with zc / zb / sF / sW: sM lies over them)
            if (on) dpgp_spill_moment_tiles(acc, nct, sM, MS, wave, lane);
            __syncthreads();
            if (on) {
                const int cw = 16 * nct;
                const double *mrow = sM + pi * MS;
                const double s0 = col0 == 0 ? mrow[0] : 0.0, cf = p2 ? 2.0 : 1.0;
#pragma unroll
                for (int j = 0; j < NQ; ++j) {
                    const int q = kk + 4 * j;
                    if (q < Q) {
                        const int i1 = 1 + q - col0, i2 = 1 + Q + q - col0;
                        const double s1 = (i1 >= 0 && i1 < cw) ? mrow[i1] : 0.0, s2 = (i2 >= 0 && i2 < cw) ? mrow[i2] : 0.0;
                        const double g = sg[q * PL_NP + pi], mq = smu[q * PL_NP + pi], sgv = scale * g;
                        dmu[j] += -2.0 * sgv * (mq * s0 - s1);
                        dsv[j] += -sgv * s0 + cf * sgv * g * (mq * mq * s0 - 2.0 * mq * s1 + s2);
                    }
                }
            }
        }
    }
    if (!wave_live) return;
    const int n = n0 + pi;
    if (n >= N) return;
    const size_t slab = ((size_t)cslab * a.pslabs + pslab) * a.nchunks + chunk;
    dpgp_write_point_partials(a.part + slab * 2 * (size_t)N * Q, n, N, Q, kk, dmu, dsv);
}

// d_mu[n][q], d_s[n][q]: the slabs added in slab order (launch_point_adjoint_slab_sum, also qx_psi_point_adjoint.hip's)
__global__ __launch_bounds__(256) void point_adjoint_slab_sum_kernel(size_t nq, int slabs, const double *__restrict__ part,
                                                                     double *__restrict__ d_mu, double *__restrict__ d_s) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= 2 * nq) return;
    double acc = 0.0;
    for (int sl = 0; sl < slabs; ++sl) acc += part[(size_t)sl * 2 * nq + e];
    if (e < nq) d_mu[e] = acc;
    else d_s[e - nq] = acc;
}

struct PlPlan { int T, tiles, ntn, nchunks, nct, ct, cslabs, cols_per_slab, pslabs, tiles_per_slab; };


PlPlan pl_plan(int B, int N, int M, int Q) {
    PlPlan p;
    p.T = dpgp_ceil_div(M, PL_TILE);
    p.tiles = p.T * (p.T + 1) / 2;
    p.ntn = dpgp_ceil_div(N, PL_NP);
    const int tiles16 = dpgp_ceil_div(1 + 2 * Q, 16);
    p.nct = dpgp_ceil_div(tiles16, dpgp_ceil_div(tiles16, PL_MAXCT));   // chunks of equal width
    p.nchunks = dpgp_ceil_div(tiles16, p.nct);
    p.ct = p.nct <= 1 ? 1 : p.nct <= 2 ? 2 : p.nct <= 4 ? 4 : 8;
    // slabs of columns b, then of pair tiles; DPGP_PLA_COL_SLABS / DPGP_PLA_PAIR_SLABS force the two counts
    const DpgpSlabSplit sp = dpgp_slab_split((long)p.ntn * p.nchunks, PL_TARGET_WGS, B, p.tiles, "DPGP_PLA_COL_SLABS", "DPGP_PLA_PAIR_SLABS");
    p.cslabs = sp.outer_slabs; p.cols_per_slab = sp.outer_per_slab; p.pslabs = sp.pair_slabs; p.tiles_per_slab = sp.tiles_per_slab;
    return p;
}

size_t pl_lds(int Q, int ct) {
    const size_t stage = (size_t)2 * PL_TILE * Q + PL_TILE * PL_FSTRIDE + (size_t)PL_TILE * (16 * ct + PL_WPAD);
    const size_t mom = (size_t)PL_NP * (16 * ct + 1);
    return sizeof(double) * ((size_t)2 * Q * PL_NP + 2 * PL_NP + 2 * Q + (stage > mom ? stage : mom) + DPGP_EXP2_TAB_ELEMS);
}
int pl_region(int Q, int ct) {                                // doubles of the staging area / the moments that lie over it
    return (int)(pl_lds(Q, ct) / sizeof(double) - ((size_t)2 * Q * PL_NP + 2 * PL_NP + 2 * Q + DPGP_EXP2_TAB_ELEMS));
}

// B, N, M >= 1, 1 <= Q <= 64, and sizes that the 32-bit grid and the int indices of the plan hold
bool pl_shape_ok(int B, int N, int M, int Q) {
    if (B < 1 || N < 1 || M < 1 || Q < 1 || Q > DPGP_QX_PSI_MAX_Q) return false;
    if (M > 46000) return false;
    return (long)dpgp_ceil_div(N, PL_NP) * 2 * B <= 0x7fffffffL / 2;
}

template <int CT, bool QREG> int pl_launch(const PlPlan &p, PlArgs a, hipStream_t st) {
    const size_t lds = pl_lds(a.Q, CT);
    a.region = pl_region(a.Q, CT);
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(pl_kernel<CT, QREG>), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL((pl_kernel<CT, QREG>), dim3((unsigned)((long)p.ntn * p.nchunks * p.cslabs), p.pslabs), dim3(256), lds, st, a);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

template <bool QREG> int pl_dispatch(const PlPlan &p, const PlArgs &a, hipStream_t st) {
    return p.ct == 1 ? pl_launch<1, QREG>(p, a, st) : p.ct == 2 ? pl_launch<2, QREG>(p, a, st)
         : p.ct == 4 ? pl_launch<4, QREG>(p, a, st) : pl_launch<8, QREG>(p, a, st);
}

}  // namespace

int launch_point_adjoint_slab_sum(size_t nq, int slabs, const double *part, double *d_mu, double *d_s, hipStream_t st) {
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(point_adjoint_slab_sum_kernel, dim3((unsigned)((2 * nq + 255) / 256)), dim3(256), 0, st, nq, slabs, part, d_mu,
                       d_s);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

extern "C" size_t dpgp_psi_latent_adjoint_workspace_bytes(int B, int N, int M, int Q) {
    if (!pl_shape_ok(B, N, M, Q)) return 0;
    const PlPlan p = pl_plan(B, N, M, Q);
    return sizeof(double) * (size_t)p.cslabs * p.pslabs * p.nchunks * 2 * N * Q;
}

extern "C" int dpgp_psi_latent_adjoint_f64(int B, int N, int M, int Q, const double *z, const double *mu, const double *s,
                                           const double *gamma, const double *alpha, const double *y, int ldy, const double *w,
                                           const double *g_v, const double *g_psi2, double *d_mu, double *d_s, void *ws,
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
    if (!y) return -10;
    if (ldy < B) return -11;
    if (!g_v) return -13;
    if (!g_psi2) return -14;
    if (!d_mu) return -15;
    if (!d_s) return -16;
    if (!ws) return -17;
    const size_t need = dpgp_psi_latent_adjoint_workspace_bytes(B, N, M, Q);
    if (need == 0 || ws_bytes < need) return -18;              // (need == 0: a shape past what the launch grid holds)
    hipStream_t st = (hipStream_t)stream;
    const PlPlan p = pl_plan(B, N, M, Q);
    PlArgs a;
    a.B = B; a.N = N; a.M = M; a.Q = Q; a.T = p.T; a.ntn = p.ntn; a.nchunks = p.nchunks; a.nct = p.nct; a.cslabs = p.cslabs;
    a.cols_per_slab = p.cols_per_slab; a.pslabs = p.pslabs; a.tiles_per_slab = p.tiles_per_slab; a.ldy = ldy;
    a.z = z; a.mu = mu; a.s = s; a.gamma = gamma; a.alpha = alpha; a.y = y; a.w = w; a.gv = g_v; a.g2 = g_psi2;
    a.part = static_cast<double *>(ws);
    const int rc = Q <= PL_QR ? pl_dispatch<true>(p, a, st) : pl_dispatch<false>(p, a, st);
    if (rc) return rc;
    return launch_point_adjoint_slab_sum((size_t)N * Q, p.cslabs * p.pslabs * p.nchunks, a.part, d_mu, d_s, st);
}
