// (d_mu, d_s) of the per-point Psi contractions of qx_psi_point.hip: K ARD-RBF kernels with their own inducing inputs z[K][M][Q]
// that share q(X*) = (mu, s) [N][Q], c[K][G][M][M] (any matrices), r[K][M][J], and the adjoints h[K][N][J], gq[K][N][J], gt[K][N][G] of
//   L = sum_knj h (psi1_kn . r_kj) + sum_knj gq (r_kj^T psi2_kn r_kj) + sum_kng gt <c_kg, psi2_kn>,     d_mu = dL/dmu, d_s = dL/ds
// (s: variances).  Per (k, n) the adjoint of psi2_kn is formed FIRST and then multiplied with the point's exponentials, so an
// exponential is evaluated once per (k, n, pair) however many columns J + G there are.  Psi2 part, a pair m <= m' visited once,
// zbar = (z_m + z_m') / 2, F = alpha^2 exp(-1/4 sum_q gamma_q (z_mq - z_m'q)^2) (or zfac), F' = F on the diagonal and 2 F off it:
//   T[n][pair] = sum_j gq[n,j] r[m,j] r[m',j] + sum_g gt[n,g] (c_g[m,m'] + c_g[m',m]) / 2                      (GEMM 1, inner size J + G)
//   E[n][pair] = c2_n exp(-sum_q gr_q (mu_nq - zbar_q)^2),  gr_q = gamma_q / (2 gamma_q s_nq + 1),  c2_n = prod_q (2 gamma_q s_nq + 1)^-1/2
//   D = T . E . F',     (S0, S1_q, S2_q) = D [N x pairs] (1, zbar_q, zbar_q^2) [pairs x (1 + 2Q)]               (GEMM 2)
//   d_mu_nq += -2 gr_q (mu S0 - S1_q),     d_s_nq += -gr_q S0 + 2 gr_q^2 (mu^2 S0 - 2 mu S1_q + S2_q)
// Psi1 part, the same over single inducing points: a1[n][m] = sum_j h[n,j] r[m,j] (GEMM 1), gr1_q = gamma_q / (gamma_q s_nq + 1),
// E1 = alpha prod_q (gamma_q s_nq + 1)^-1/2 exp(-1/2 sum_q gr1_q (mu_nq - z_mq)^2), (T0, T1_q, T2_q) = (a1 . E1) (1, z_mq, z_mq^2):
//   d_mu_nq += -gr1_q (mu T0 - T1_q),      d_s_nq += 1/2 (-gr1_q T0 + gr1_q^2 (mu^2 T0 - 2 mu T1_q + T2_q))
// mu and z are taken relative to the workgroup's first test point (only mu - z enters), the exponential is dpgp_exp2_tab, and for
// Q <= 16 the exponent is expanded per (point, phase) (DpgpPointExponent, qx_tile.h): two FMAs per q and pair.
//
// Layout (that of pw_kernel and pl_kernel; the pieces common to pl_kernel and this kernel are the helpers of qx_tile.h).  Workgroup (block of 64 test points, chunk of <= 16 CT of the G + J columns [gt | gq],
// slab of kernels k; slab of pair tiles), 256 threads = 4 waves; a wave owns 16 points.  The lane (point i = lane & 15, kk = lane >> 4)
// keeps its point's adjoints of the chunk, columns kk + 4 st, in registers: they are the B operand of GEMM 1, which is run
// TRANSPOSED, T^T [16 pairs x 16 points] = A [16 pairs x columns] B [columns x 16 points] on v_mfma_f64_16x16x4, A read from LDS.
// Its result leaves lane (i, kk) with T of point i at pairs kk + 4 rr, which is exactly the A operand of GEMM 2's step rr: the lane
// evaluates ONE exponential per such pair, multiplies, and feeds the MT <= 9 moment tiles of v_mfma_f64_16x16x4.  No transposition
// through LDS and nothing of size N M M, pairs x J or pairs x G anywhere.  Pairs are walked as in pw_kernel: 32 x 32 tiles (I, J),
// I <= J, one row m (a block of 32 pairs) at a time; per block all threads form zbar [32][Q], A [32][16 CT] and the moment
// columns [32][16 MT] in LDS.  A column chunk beyond 16 CT columns is another workgroup (its exponentials are evaluated again, as in
// the forward operator); L is linear in the adjoints, so the chunks' partial (d_mu, d_s) simply add.
// A wave whose 16 points have all-zero adjoints in the chunk skips the phase behind one wave-uniform branch; a zero adjoint that is
// not skipped gives T = 0 and multiplies finite numbers: exactly 0.0 either way.
// The accumulators go to part[slab][2][N][Q]; a second launch (launch_point_adjoint_slab_sum) adds the slabs in slab order.  No atomics: the same bits on every run.
#include "internal.h"
#include "qx_tile.h"

#define PA_TILE 32
#define PA_NP 64            // test points per workgroup: 4 waves x 16 MFMA rows
#define PA_FSTRIDE (PA_TILE + 1)
#define PA_APAD 4           // A row stride 16 CT + 4 doubles: the 16 rows x 4 columns of an A operand fall on distinct banks
#define PA_WPAD 16          // moment row stride 16 MT + 16 doubles (as PW_WPAD)
#define PA_QR 16            // Q <= PA_QR: the lane's point in registers, 4 (d_mu, d_s) accumulators per lane; above: LDS, 16
#define PA_TARGET_WGS 512

namespace {

struct PaArgs {
    int K, G, J, N, M, Q, T, ntn, nchunks, nct, kslabs, k_per_slab, pslabs, tiles_per_slab, region;
    const double *z, *mu, *s, *gamma, *alpha, *zfac, *c, *r, *h, *gq, *gt;
    double *part;
};

template <int CT, int MT, bool QREG>
__global__ __launch_bounds__(256) void pa_kernel(const PaArgs a) {
    constexpr int CW = 16 * CT, AS = CW + PA_APAD, PSTEP = 256 / CW, NB = CW / 4;
    constexpr int MW = 16 * MT, WS = MW + PA_WPAD, MS = MW + 1, NQ = QREG ? PA_QR / 4 : DPGP_QX_PSI_MAX_Q / 4;
    const int G = a.G, J = a.J, N = a.N, M = a.M, Q = a.Q;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *smu = reinterpret_cast<double *>(smem_raw);    // [Q][64]  mu - centre
    double *sg = smu + (size_t)Q * PA_NP;                   // [Q][64]  gr (Psi2) / gr1 (Psi1) of the kernel, 0 past N
    double *sc = sg + (size_t)Q * PA_NP;                    // [64]     prefactor c2_n / alpha c1_n, 0 past N
    double *cen = sc + PA_NP;                               // [Q]      the workgroup's centre: mu of its first point
    double *gm = cen + Q;                                   // [Q]      gamma of the kernel
    double *zc = gm + Q;                                    // [32][Q]  z rows of the tile's columns, centred
    double *zb = zc + (size_t)PA_TILE * Q;                  // [32][Q]  zbar of the block's pairs, centred
    double *sF = zb + (size_t)PA_TILE * Q;                  // [32][33] F' of the tile
    double *sW = sF + PA_TILE * PA_FSTRIDE;                 // [32][WS] moment columns of the block's pairs
    double *sA = sW + PA_TILE * WS;                         // [32][AS] A of GEMM 1: r[m,j] r[m',j] | symmetrised c_g[m,m']  (Psi1: r rows)
    double *sM = zc;                                        // [64][MS] the waves' moments (over zc .. sA, between the phases)
    double *tab = sM + (size_t)a.region;                    // [64]     2^(j/64) (dpgp_exp2_tab)
    dpgp_exp2_tab_init(tab);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, pslab = blockIdx.y;
    const int nt = blockIdx.x % a.ntn, rest = blockIdx.x / a.ntn, chunk = rest % a.nchunks, kslab = rest / a.nchunks;
    const int C = G + J, tiles16 = (C + 15) / 16;
    const int nct = min(a.nct, tiles16 - chunk * a.nct), col0 = 16 * chunk * a.nct, nst = 4 * nct;
    const int n0 = nt * PA_NP;
    for (int q = t; q < Q; q += 256) cen[q] = a.mu[(size_t)n0 * Q + q];
    __syncthreads();
#pragma unroll 1
    for (int e = t; e < PA_NP * Q; e += 256) {
        const int i = e / Q, q = e % Q;
        smu[q * PA_NP + i] = n0 + i < N ? a.mu[(size_t)n0 * Q + e] - cen[q] : 0.0;
    }
    const int pi = wave * 16 + (lane & 15), kk = lane >> 4;
    const bool wave_live = n0 + wave * 16 < N, pt_live = n0 + pi < N;
    double dmu[NQ], dsv[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) dmu[j] = dsv[j] = 0.0;
    // the thread's element of A: column col_l of the chunk, pairs prow, prow + PSTEP, ..
    const int col_l = t % CW, prow = t / CW, gcol = col0 + col_l;
    const bool col_on = gcol < C && col_l < 16 * nct, col_tr = gcol < G;
    const int k_lo = kslab * a.k_per_slab, k_hi = min(a.K, k_lo + a.k_per_slab);
    const int ntile2 = a.T * (a.T + 1) / 2;
    const int tile_lo = pslab * a.tiles_per_slab, tile_hi = min(ntile2, tile_lo + a.tiles_per_slab);
    for (int k = k_lo; k < k_hi; ++k) {
        const double *zk = a.z + (size_t)k * M * Q, *gk = a.gamma + (size_t)k * Q, *rk = a.r + (size_t)k * M * J;
        const double *cg = a.c + ((size_t)k * G + (col_tr ? gcol : 0)) * M * M;
        const double *rcol = rk + (col_on && !col_tr ? gcol - G : 0);
        const double *zf = a.zfac ? a.zfac + (size_t)k * M * M : nullptr;
        const double al = a.alpha[k];
        for (int ph = 0; ph < (pslab == 0 ? 2 : 1); ++ph) {
            const bool p2 = ph == 0;
            const double k2 = p2 ? 2.0 : 1.0, kexp = p2 ? -DPGP_LOG2E : -0.5 * DPGP_LOG2E;
            __syncthreads();                                   // (previous phase done with sg / sc / gm and with sM)
#pragma unroll 1
            for (int e = t; e < PA_NP * Q; e += 256) {
                const int i = e / Q, q = e % Q;
                const double g = gk[q];
                sg[q * PA_NP + i] = n0 + i < N ? g / fma(k2 * g, a.s[(size_t)n0 * Q + e], 1.0) : 0.0;
            }
            if (t < PA_NP) sc[t] = dpgp_point_prefactor(n0 + t, N, Q, gk, a.s, k2, p2 ? 1.0 : al);
            for (int q = t; q < Q; q += 256) gm[q] = gk[q];
            // the lane's adjoints of the chunk: column col0 + kk + 4 st (the B operand of GEMM 1)
            double breg[NB];
            bool nz = false;
            {
                const size_t kn = (size_t)k * N + (pt_live ? n0 + pi : 0);
#pragma unroll
                for (int st = 0; st < NB; ++st) {
                    const int col = col0 + 4 * st + kk;
                    double v = 0.0;
                    if (pt_live && st < nst && col < C) {
                        if (p2) v = col < G ? a.gt[kn * G + col] : a.gq[kn * J + (col - G)];
                        else if (col >= G) v = a.h[kn * J + (col - G)];
                    }
                    breg[st] = v;
                    nz = nz || v != 0.0;
                }
            }
            const bool on = wave_live && __any(nz);            // (wave-uniform)
            if (!__syncthreads_or(on)) continue;               // (a barrier: sg / sc / gm are visible.  Workgroup-uniform)
            const double c2 = sc[pi];
            DpgpPointExponent<QREG ? PA_QR : 1> ex;            // (Q <= 16: the expanded exponent, two FMAs per q and pair)
            if constexpr (QREG) ex.setup(Q, kexp, smu, sg, PA_NP, pi);
            f64x4 acc[MT];
#pragma unroll
            for (int ct = 0; ct < MT; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
            const int t_lo = p2 ? tile_lo : 0, t_hi = p2 ? tile_hi : a.T;
            for (int tile = t_lo; tile < t_hi; ++tile) {
                int I = tile, Jt = tile;
                if (p2) dpgp_tile_ij(tile, a.T, I, Jt);
                const bool diag = I == Jt;
                const int m0 = I * PA_TILE, c0 = Jt * PA_TILE;
                const int nr = min(PA_TILE, M - m0), nc = min(PA_TILE, M - c0);
                __syncthreads();                               // (previous tile done with zc / sF / sW / zb / sA)
#pragma unroll 1
                for (int e = t; e < PA_TILE * Q; e += 256) zc[e] = e / Q < nc ? zk[(size_t)c0 * Q + e] - cen[e % Q] : 0.0;
                if (p2)
#pragma unroll 1
                    for (int e = t; e < PA_TILE * PA_TILE; e += 256) {
                        const int rr = e / PA_TILE, cc = e % PA_TILE, m = m0 + rr, mp = c0 + cc;
                        double f = 0.0;
                        if (rr < nr && cc < nc && (!diag || cc >= rr)) {
                            f = dpgp_pair_factor(zf, M, Q, m, mp, zk, gm, al);
                            if (m != mp) f *= 2.0;
                        }
                        sF[rr * PA_FSTRIDE + cc] = f;
                    }
                const int nrows = p2 ? nr : 1;
                for (int rr = 0; rr < nrows; ++rr) {
                    const int m = m0 + rr;
                    __syncthreads();                           // (the tile's staging is visible; previous block's A / W / zbar consumed)
                    if (p2) {
#pragma unroll 1
                        for (int e = t; e < PA_TILE * Q; e += 256) zb[e] = 0.5 * ((zk[(size_t)m * Q + e % Q] - cen[e % Q]) + zc[e]);
                        const double rm = (col_on && !col_tr) ? rcol[(size_t)m * J] : 0.0;
#pragma unroll 1
                        for (int p = prow; p < PA_TILE; p += PSTEP) {
                            const int mp = c0 + p;
                            double v = 0.0;
                            if (col_on && p < nc && (!diag || p >= rr)) {
                                if (col_tr) v = m == mp ? cg[(size_t)m * M + m] : 0.5 * (cg[(size_t)m * M + mp] + cg[(size_t)mp * M + m]);
                                else v = rm * rcol[(size_t)mp * J];
                            }
                            sA[p * AS + col_l] = v;
                        }
                    } else {
#pragma unroll 1
                        for (int p = prow; p < PA_TILE; p += PSTEP)
                            sA[p * AS + col_l] = (col_on && !col_tr && p < nc) ? rcol[(size_t)(c0 + p) * J] : 0.0;
                    }
                    __syncthreads();                           // (zbar / the tile's z rows are visible: the moment columns read them)
                    {
                        const double *zz = p2 ? zb : zc;
#pragma unroll 1
                        for (int e = t; e < PA_TILE * MW; e += 256) {
                            const int p = e / MW, ml = e % MW;
                            double v = 0.0;
                            if (p < nc && ml <= 2 * Q) {
                                const double zv = ml == 0 ? 1.0 : zz[p * Q + (ml <= Q ? ml - 1 : ml - 1 - Q)];
                                v = ml <= Q ? zv : zv * zv;
                            }
                            sW[p * WS + ml] = v;
                        }
                    }
                    __syncthreads();
                    if (!on) continue;                         // (wave-uniform)
                    const double *zz = p2 ? zb : zc;
                    const int s_lo = (p2 && diag) ? rr >> 2 : 0, s_hi = (nc + 3) >> 2;
#pragma unroll 1
                    for (int pt = 0; pt < 2; ++pt) {
                        if (4 * pt >= s_hi || 4 * pt + 3 < s_lo) continue;     // (wave-uniform: no pair of these 16 counts)
                        // GEMM 1, transposed: lane (i, kk) gets T of point i at pairs 16 pt + kk + 4 r4
                        f64x4 tacc = f64x4{0.0, 0.0, 0.0, 0.0};
                        const double *arow = sA + (16 * pt + (lane & 15)) * AS + kk;
#pragma unroll
                        for (int ct = 0; ct < CT; ++ct)
                            if (ct < nct) {
#pragma unroll
                                for (int st = 4 * ct; st < 4 * ct + 4; ++st) tacc = Mfma<double>::mma(arow[4 * st], breg[st], tacc);
                            }
#pragma unroll 1
                        for (int r4 = 0; r4 < 4; ++r4) {
                            const int st2 = 4 * pt + r4;
                            if (st2 < s_lo || st2 >= s_hi) continue;           // (wave-uniform)
                            const int cc = 4 * st2 + kk;
                            const double *zq = zz + (size_t)cc * Q;
                            double e = 0.0;
                            if constexpr (QREG) {
                                e = ex.at(Q, zq);
                            } else {
                                for (int q = 0; q < Q; ++q) {
                                    const double d = smu[q * PA_NP + pi] - zq[q];
                                    e = fma(kexp * sg[q * PA_NP + pi] * d, d, e);
                                }
                            }
                            const double tv = r4 == 0 ? tacc[0] : r4 == 1 ? tacc[1] : r4 == 2 ? tacc[2] : tacc[3];
                            double av = tv * (c2 * dpgp_exp2_tab(e, tab));
                            if (p2) av *= sF[rr * PA_FSTRIDE + cc];
                            const double *wrow = sW + cc * WS + (lane & 15);
#pragma unroll
                            for (int ct = 0; ct < MT; ++ct) acc[ct] = Mfma<double>::mma(av, wrow[16 * ct], acc[ct]);
                        }
                    }
                }
            }
            // the phase's moments -> its contribution to (d_mu, d_s)
            __syncthreads();                                   // (every wave is done with zc / zb / sF / sW / sA: sM lies over them)
            if (on) dpgp_spill_moment_tiles(acc, MT, sM, MS, wave, lane);
            __syncthreads();
            if (on) {
                const double *mrow = sM + pi * MS;
                const double s0 = mrow[0], cf = p2 ? 2.0 : 1.0, scale = p2 ? 1.0 : 0.5;
#pragma unroll
                for (int j = 0; j < NQ; ++j) {
                    const int q = kk + 4 * j;
                    if (q < Q) {
                        const double s1 = mrow[1 + q], s2 = mrow[1 + Q + q];
                        const double g = sg[q * PA_NP + pi], mq = smu[q * PA_NP + pi], sgv = scale * g;
                        dmu[j] += -2.0 * sgv * (mq * s0 - s1);
                        dsv[j] += -sgv * s0 + cf * sgv * g * (mq * mq * s0 - 2.0 * mq * s1 + s2);
                    }
                }
            }
        }
    }
    if (!pt_live) return;
    const int n = n0 + pi;
    const size_t slab = ((size_t)kslab * a.pslabs + pslab) * a.nchunks + chunk;
    dpgp_write_point_partials(a.part + slab * 2 * (size_t)N * Q, n, N, Q, kk, dmu, dsv);
}

struct PaPlan { int T, tiles, ntn, nchunks, nct, ct, mt, kslabs, k_per_slab, pslabs, tiles_per_slab; };

// Tests and experiments: a forced number of slabs, read on every plan so that the workspace query and the launch agree.
// DPGP_PA_K_SLABS: the slabs of kernels k (clamped to K);  DPGP_PA_PAIR_SLABS: the pair-tile slabs (clamped to the tiles).
// Unset or < 1: the plan's own.

PaPlan pa_plan(int K, int G, int J, int N, int M, int Q) {
    PaPlan p;
    p.T = dpgp_ceil_div(M, PA_TILE);
    p.tiles = p.T * (p.T + 1) / 2;
    p.ntn = dpgp_ceil_div(N, PA_NP);
    // column chunks of equal width, at most 64 columns (the lane's 16 adjoints; 32 for Q > 32, where the LDS does not hold more)
    const int tiles16 = (int)(((long)G + J + 15) / 16), ctmax = Q <= 32 ? 4 : 2;
    p.nct = dpgp_ceil_div(tiles16, dpgp_ceil_div(tiles16, ctmax));
    p.nchunks = dpgp_ceil_div(tiles16, p.nct);
    p.ct = p.nct <= 2 ? 2 : 4;
    const int mt = dpgp_ceil_div(1 + 2 * Q, 16);               // all 1 + 2Q moment columns in one pass: 2, 3, 5 or 9 tiles
    p.mt = mt <= 2 ? 2 : mt <= 3 ? 3 : mt <= 5 ? 5 : 9;
    // slabs of kernels k, then of pair tiles
    const DpgpSlabSplit sp = dpgp_slab_split((long)p.ntn * p.nchunks, PA_TARGET_WGS, K, p.tiles, "DPGP_PA_K_SLABS", "DPGP_PA_PAIR_SLABS");
    p.kslabs = sp.outer_slabs; p.k_per_slab = sp.outer_per_slab; p.pslabs = sp.pair_slabs; p.tiles_per_slab = sp.tiles_per_slab;
    return p;
}

size_t pa_fixed(int Q) { return (size_t)2 * Q * PA_NP + PA_NP + 2 * Q + DPGP_EXP2_TAB_ELEMS; }
size_t pa_lds(int Q, int ct, int mt) {
    const size_t stage = (size_t)2 * PA_TILE * Q + PA_TILE * PA_FSTRIDE + (size_t)PA_TILE * (16 * mt + PA_WPAD) +
                         (size_t)PA_TILE * (16 * ct + PA_APAD);
    const size_t mom = (size_t)PA_NP * (16 * mt + 1);
    return sizeof(double) * (pa_fixed(Q) + (stage > mom ? stage : mom));
}

// K, G, J, N, M >= 1, 1 <= Q <= 64, and sizes that the 32-bit grid and the int indices of the plan hold
bool pa_shape_ok(int K, int G, int J, int N, int M, int Q) {
    if (K < 1 || G < 1 || J < 1 || N < 1 || M < 1 || Q < 1 || Q > DPGP_QX_PSI_MAX_Q) return false;
    if ((long)G + J > 0x7fffffffL / 2 || M > 46000) return false;
    const long wgs = (long)dpgp_ceil_div(N, PA_NP) * K * (((long)G + J + 15) / 16);
    return wgs <= 0x7fffffffL / 2;
}

template <int CT, int MT, bool QREG> int pa_launch(const PaPlan &p, PaArgs a, hipStream_t st) {
    const size_t lds = pa_lds(a.Q, CT, MT);
    a.region = (int)(lds / sizeof(double) - pa_fixed(a.Q));
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(pa_kernel<CT, MT, QREG>), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL((pa_kernel<CT, MT, QREG>), dim3((unsigned)((long)p.ntn * p.nchunks * p.kslabs), p.pslabs), dim3(256), lds, st, a);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

template <int CT> int pa_dispatch(const PaPlan &p, const PaArgs &a, hipStream_t st) {
    if (a.Q <= PA_QR) return p.mt == 2 ? pa_launch<CT, 2, true>(p, a, st) : pa_launch<CT, 3, true>(p, a, st);
    if (p.mt == 3) return pa_launch<CT, 3, false>(p, a, st);
    if (p.mt == 5) return pa_launch<CT, 5, false>(p, a, st);
    if constexpr (CT == 2) return pa_launch<2, 9, false>(p, a, st);    // (9 moment tiles: Q >= 40, where a chunk has 2 column tiles)
    return DPGP_ERR_LAUNCH;
}

}  // namespace

extern "C" size_t dpgp_qx_psi_pointwise_adjoint_workspace_bytes(int K, int G, int J, int N, int M, int Q) {
    if (!pa_shape_ok(K, G, J, N, M, Q)) return 0;
    const PaPlan p = pa_plan(K, G, J, N, M, Q);
    return sizeof(double) * (size_t)p.kslabs * p.pslabs * p.nchunks * 2 * N * Q;
}

extern "C" int dpgp_qx_psi_pointwise_adjoint_f64(int K, int G, int J, int N, int M, int Q, const double *z, const double *mu,
                                                 const double *s, const double *gamma, const double *alpha, const double *zfac,
                                                 const double *c, const double *r, const double *h, const double *gq,
                                                 const double *gt, double *d_mu, double *d_s, void *ws, size_t ws_bytes,
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
    if (!h) return -15;
    if (!gq) return -16;
    if (!gt) return -17;
    if (!d_mu) return -18;
    if (!d_s) return -19;
    if (!ws) return -20;
    const size_t need = dpgp_qx_psi_pointwise_adjoint_workspace_bytes(K, G, J, N, M, Q);
    if (need == 0 || ws_bytes < need) return -21;              // (need == 0: a shape past what the launch grid holds)
    hipStream_t st = (hipStream_t)stream;
    const PaPlan p = pa_plan(K, G, J, N, M, Q);
    PaArgs a;
    a.K = K; a.G = G; a.J = J; a.N = N; a.M = M; a.Q = Q; a.T = p.T; a.ntn = p.ntn; a.nchunks = p.nchunks; a.nct = p.nct;
    a.kslabs = p.kslabs; a.k_per_slab = p.k_per_slab; a.pslabs = p.pslabs; a.tiles_per_slab = p.tiles_per_slab; a.region = 0;
    a.z = z; a.mu = mu; a.s = s; a.gamma = gamma; a.alpha = alpha; a.zfac = zfac; a.c = c; a.r = r; a.h = h; a.gq = gq; a.gt = gt;
    a.part = static_cast<double *>(ws);
    const int rc = p.ct == 2 ? pa_dispatch<2>(p, a, st) : pa_dispatch<4>(p, a, st);
    if (rc) return rc;
    return launch_point_adjoint_slab_sum((size_t)N * Q, p.kslabs * p.pslabs * p.nchunks, a.part, d_mu, d_s, st);
}
