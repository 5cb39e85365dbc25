// Latent-space metric, predictive Jacobian, contracted Christoffel symbol and its tangent of K ARD-RBF kernels at DETERMINISTIC
// latent points x [N][Q].  With
//   k_km(x_n)  = alpha_k exp(-1/2 sum_q gamma_kq (x_nq - z_kmq)^2)
//   b_kmq(x_n) = d k_km / d x_q = -gamma_kq (x_nq - z_kmq) k_km(x_n)                    the derivative features [M x Q] of point n
// the four operators are
//   metric:      g[k][n][q][q']  = sum_{m,m'} p[k][m][m'] b_kmq(x_n) b_km'q'(x_n)         p [K][M][M], used as given (not symmetrised)
//   jacobian:    jac[k][n][j][q] = sum_m b_kmq(x_n) r[k][m][j]                           r [K][M][J]
//   christoffel: g as the metric's, and with velocities v [N][Q],
//                  a_knm = sum_q gamma_kq (x_nq - z_kmq) v_nq
//                  d_knm = v_n^T (d^2 k_km / dx dx)(x_n) v_n = k_km(x_n) (a_knm^2 - sum_q gamma_kq v_nq^2)
//                gam[k][n][q]    = sum_{m,m'} b_kmq(x_n) p[k][m][m'] d_knm'
//                For symmetric p, gam is the Christoffel symbol of the first kind of g contracted twice with v,
//                  gam = (D_v g) v - 1/2 grad_x (v^T g v):    the (Hv)^T p c terms of the two parts cancel, H the Hessian features.
//   tangent:     g and gam as christoffel's (the same bits), and their derivatives along a direction (dx, dv) [N][Q] of (x, v):
//                with u_q = gamma_kq (x_nq - z_kmq), s = sum_q gamma_kq v_nq^2,
//                  e = sum_q u_q dx_q,   f = sum_q u_q dv_q,   c1 = sum_q gamma_kq dx_q v_q,   c2 = sum_q gamma_kq v_q dv_q
//                  db_q = k (e u_q - gamma_kq dx_q),           dd = k (-e (a^2 - s) + 2 a (c1 + f) - 2 c2)
//                dg[k][n][q][q'] = (dB^T p B + B^T p dB)_qq',    dgam[k][n][q] = (dB^T p d + B^T p dd)_q
// ONE kernel, mt_kernel<QT, MODE>, does all five (transport: below); what exists in one mode only sits behind `if constexpr`.
// The features B [M x (points, q)] are never stored to memory: a workgroup makes them on the fly, 64 inducing points at a time,
// into LDS, one exponential per (k, n, m) and per slab of 64 rows of the left operand.
//
// Layout.  Workgroup (kernel k, tile of NP points), 256 threads = 4 waves.  A point's feature block is W columns wide: W = Q, and
// W = Q + 1 for christoffel, whose block is F = [b_.1 .. b_.Q, d].  With QT = ceil(W / 16) a point owns QT column tiles of 16
// (its columns padded to 16 QT), NP = 8, 2, 1, 1 points for QT = 1 .. 4, CT = NP QT column tiles in all; for Q <= 15 the d column
// sits in the padding that the metric carries anyway.  All three operators are the product
//   U [R x (point, q)] = A [R x M] B [M x (point, q)]          metric, christoffel: A = p_k, R = M;   jacobian: A = r_k^T, R = J
// on v_mfma_f64_16x16x4 (Mfma<double>): the rows of A go in slabs of 64, wave w owns rows 16 w .. 16 w + 15 of the slab and the CT
// accumulators of its row tile; the inner index m' goes in chunks of 64: per chunk the z rows [64][Q], the exponentials
// [64][NP], the features sB [64][16 CT (+ pad)] and the A tile sP [64][64 (+ pad)] are staged in LDS, then every wave runs the
// chunk's 16 steps of 4 inner indices (A operand from sP, B operands from sB).  A is streamed through LDS in these tiles and is
// never resident: no size limit on M from the LDS.
//   jacobian: U is the result; it is stored from the accumulators.
//   metric:   g_n = B_n^T U_n is a second product on the matrix pipe.  The accumulator layout of v_mfma_f64_16x16x4 (row
//             (lane >> 4) + 4 r in register r) IS the B-operand layout of step r over the wave's 16 rows, so U never leaves the
//             registers: step r multiplies the features of rows 16 w + 4 r .. + 3 (A operand, from sB) with acc[.][r].  For that
//             the chunks of a slab are walked in the rotated order slab + 1, .., nch - 1, 0, .., slab: the slab's own chunk comes
//             last and its features are the ones in LDS when U is complete.  Each wave keeps NP QT^2 result tiles over all slabs;
//             at the end the four waves' tiles are added in wave order through LDS and stored.
//   christoffel: the same with F in the place of B: F^T p F holds g in its leading Q x Q block and gam in the first Q rows of its
//             last column.  An entry of g is summed in the metric's order whether or not the d column costs a tile: the same bits.
//   tangent:  the same with F = [B | d | dB | dd], W = 2 Q + 2: all four results are entries of F^T p F, g and gam where
//             christoffel has them, dg = (rows 0 .. Q-1, columns Q+1 .. 2Q) + (rows Q+1 .. 2Q, columns 0 .. Q-1), dgam = (rows
//             Q+1 .. 2Q, column Q) + (rows 0 .. Q-1, column 2Q+1).  The result tiles inside the (dB | dd)^T p (dB | dd) block are
//             read by nothing and are not formed (QT = 2: one of four, QT = 3: one of nine, QT = 4: four of sixteen).  Q <= 31.
//   transport: christoffel's block and one more column per vector of a frame w [N][F][Q] (MtTrn): F = [B | d(v,v) | d(v,w_1) ..
//             d(v,w_F)], W = Q + 1 + F, with d(v,w) = v^T (d^2 k / dx dx) w = k (a_v a_w - sum_q gamma_q v_q w_q),
//             a_w = sum_q gamma_q (x_q - z_q) w_q.  g and gam are where christoffel has them (the same bits), and
//             tgam[k][n][r] = B^T p d(v,w_r) is rows 0 .. Q-1 of column Q + 1 + r: for symmetric p the Christoffel symbol of the
//             first kind contracted with v and w_r, so that w' = -G^-1 sum_k tgam is parallel transport along a geodesic with
//             velocity v.  d(v,w_r) is made with the statements of d(v,v) (w_r = v: the bits of gam) by the thread that makes
//             d(v,v), straight into its column of sB; a column's bits depend on neither F, r nor the other vectors.  Only result
//             rows 0 .. Q-1 are read, so a result tile whose row tile starts at or past Q is not formed.  Q + 1 + F <= 64.
// The order of every sum is fixed by (M, Q) alone: no atomics, no workspace, the same bits on every run; a point's results depend
// neither on N, nor on its place in x, nor on K or the other kernels.  Far-away points: dpgp_exp2 gives exact zeros, every product
// with them is 0.  1 <= Q <= 64; christoffel 1 <= Q <= 63, tangent 1 <= Q <= 31, transport 1 <= Q, F with
// Q + 1 + F <= 64 (W <= 64).
// LDS: 8 (NP Q + Q + 64 Q + 64 NP + 64 66 + 64 BS) bytes, BS = 16 CT + 16 (+ 16 for odd CT): 120.4 KiB at Q = 16, 109.5 KiB at Q = 64;
// christoffel 8 (2 NP Q + Q + 64 Q + 128 NP + 64 66 + 64 BS): 122.5 KiB at Q = 15, 107.0 KiB at Q = 63;
// tangent 8 (4 NP Q + Q + 64 Q + 256 NP + 64 66 + 64 BS): 126.3 KiB at Q = 7, 85.6 KiB at Q = 15, 87.4 KiB at Q = 23, 91.7 KiB at Q = 31;
// transport: christoffel's + 8 NP F Q for the frame: 122.5 KiB at (Q, F) = (10, 5), 122.9 KiB at (13, 2), 82.0 KiB at (10, 10), 98.0 KiB at (31, 32), 106.9 KiB at (62, 1).
#include "point_tile.h"

#define MT_MS DPGP_POINT_MS
#define MT_PS DPGP_POINT_PS
#define MT_CHRISTOFFEL_MAX_Q 63

#define MT_TANGENT_MAX_Q 31
#define MT_TRANSPORT_MAX_W 64       // Q + 1 + F

namespace {

enum MtMode { MT_METRIC, MT_JACOBIAN, MT_CHRISTOFFEL, MT_TANGENT, MT_TRANSPORT };

// what the tangent mode takes beyond the family's arguments: the direction (dx, dv) [N][Q] of the state (x, v) and the two results
struct MtTan {
    const double *dx, *dv;
    double *dg, *dgam;
};

// what the transport mode takes beyond christoffel's arguments: the frame w [N][F][Q] and its result tgam [K][N][F][Q]
struct MtTrn {
    const double *w;
    double *tgam;
    int F;
};

template <int QT> struct MtCfg {
    static constexpr int NP = QT == 1 ? 8 : QT == 2 ? 2 : 1;   // points per workgroup
    static constexpr int CT = NP * QT;                         // column tiles of 16
    static constexpr int NG = NP * QT * QT;                    // result tiles of the second product per wave
    static constexpr int BS = 16 * CT + (CT % 2 ? 32 : 16);    // row stride of sB: the 2 rows of a half wave on disjoint bank halves
};

__device__ __forceinline__ const MtTan &mt_only(const MtTan &a) { return a; }
__device__ __forceinline__ const MtTrn &mt_only(const MtTrn &a) { return a; }

// tangent: result tile (qi, qj) of a point's product lies in the (db | dd)^T p (db | dd) block, which no output reads:
// Q + 1 <= 8 QT, so it does as soon as both tile indices reach QT / 2 (QT = 2: the lower-right tile, QT = 4: the lower-right four)
__device__ __forceinline__ constexpr bool mt_tan_unread(int qt, int qi, int qj) { return 2 * qi >= qt && 2 * qj >= qt; }

// transport: only rows 0 .. Q - 1 of a point's product are read (g, gam and tgam are all there), so every result tile of a row
// tile qi that starts at or past Q is neither multiplied nor added (wave-uniform: Q is a kernel argument)
__device__ __forceinline__ constexpr bool mt_trn_unread(int Q, int qi) { return 16 * qi >= Q; }

// a: p [K][M][M] (R = M) or r [K][M][R];  out: g or jac;  vel, out2: the velocities and gam of christoffel and tangent, unused
// otherwise;  tan: ONE MtTan in the tangent mode, ONE MtTrn in the transport mode, nothing in the others (their kernel arguments
// are the ones they always had)
template <int QT, MtMode MODE, class... TAN_ARGS>
__global__ __launch_bounds__(256) void mt_kernel(int N, int M, int Q, int R, int ntn, const double *__restrict__ z,
                                                 const double *__restrict__ x, const double *__restrict__ gamma,
                                                 const double *__restrict__ alpha, const double *__restrict__ a,
                                                 double *__restrict__ out, const double *__restrict__ vel,
                                                 double *__restrict__ out2, TAN_ARGS... tan) {
    constexpr bool JAC = MODE == MT_JACOBIAN, TAN = MODE == MT_TANGENT, TRN = MODE == MT_TRANSPORT;
    constexpr bool CHR = MODE == MT_CHRISTOFFEL || TAN || TRN;
    static_assert(sizeof...(TAN_ARGS) == (TAN || TRN ? 1 : 0), "MtTan goes with the tangent mode alone, MtTrn with transport");
    constexpr int NP = MtCfg<QT>::NP, CT = MtCfg<QT>::CT, NG = MtCfg<QT>::NG, BS = MtCfg<QT>::BS;
    static_assert(NG * 256 <= MT_MS * BS, "the waves' result tiles are added in the feature buffer");
    // sv and sd exist for christoffel, tangent and transport only, sdx, sdv, se and sdd for tangent only, sw for transport only;
    // elsewhere they take no room and are never touched
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *sx = reinterpret_cast<double *>(smem_raw);      // [NP][Q]   the points, 0 past N
    double *sv = sx + (CHR ? (size_t)NP * Q : 0);            // [NP][Q]   the velocities, 0 past N
    double *sdx = sv + (TAN ? (size_t)NP * Q : 0);           // [NP][Q]   the direction's dx, 0 past N
    double *sdv = sdx + (TAN ? (size_t)NP * Q : 0);          // [NP][Q]   the direction's dv, 0 past N
    MtTrn tr{};
    if constexpr (TRN) tr = mt_only(tan...);
    const int F = tr.F;                                      // (0 but in the transport mode)
    double *sw = sdv + (TRN ? (size_t)NP * Q : 0);           // [NP][F][Q] the frame, 0 past N
    double *sg = sw + (TRN ? (size_t)NP * F * Q : (size_t)NP * Q);   // [Q]       gamma_k
    double *sz = sg + Q;                                     // [64][Q]   z rows of the chunk, 0 past M
    double *sk = sz + (size_t)MT_MS * Q;                     // [64][NP]  k_km'(x_n), 0 past M or N
    double *sd = sk + (CHR ? MT_MS * NP : 0);                // [64][NP]  d_knm', 0 past M or N
    double *se = sd + (TAN ? MT_MS * NP : 0);                // [64][NP]  e_knm' = sum_q gamma_kq (x_nq - z_km'q) dx_nq
    double *sdd = se + (TAN ? MT_MS * NP : 0);               // [64][NP]  the tangent of d_knm', 0 past M or N
    double *sP = sdd + MT_MS * NP;                           // [64][PS]  A tile (slab rows x chunk indices), 0 out of range
    double *sB = sP + MT_MS * MT_PS;                         // [64][BS]  features [b (| d (| db | dd))] of the chunk, 0 in the padding
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kk = lane >> 4;
    const int nt = blockIdx.x % ntn, k = blockIdx.x / ntn, n0 = nt * NP;
    const double *zk = z + (size_t)k * M * Q, *gk = gamma + (size_t)k * Q;
    const double *ak = a + (size_t)k * M * R;
    const double al = alpha[k];
    MtTan ta{};
    if constexpr (TAN) ta = mt_only(tan...);
    for (int e = t; e < NP * Q; e += 256) {
        const bool in = n0 + e / Q < N;
        sx[e] = in ? x[(size_t)n0 * Q + e] : 0.0;
        if constexpr (CHR) sv[e] = in ? vel[(size_t)n0 * Q + e] : 0.0;
        if constexpr (TAN) {
            sdx[e] = in ? ta.dx[(size_t)n0 * Q + e] : 0.0;
            sdv[e] = in ? ta.dv[(size_t)n0 * Q + e] : 0.0;
        }
    }
    if constexpr (TRN)
        for (int e = t; e < NP * F * Q; e += 256) sw[e] = n0 + e / (F * Q) < N ? tr.w[(size_t)n0 * F * Q + e] : 0.0;
    for (int q = t; q < Q; q += 256) sg[q] = gk[q];
    const int nch = (M + MT_MS - 1) / MT_MS, nrs = (R + MT_MS - 1) / MT_MS;
    f64x4 G[JAC ? 1 : NG];
#pragma unroll
    for (int g = 0; g < (JAC ? 1 : NG); ++g) G[g] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int rs = 0; rs < nrs; ++rs) {
        const int r0 = rs * MT_MS;
        const bool wave_live = r0 + 16 * wave < R;             // (wave-uniform)
        f64x4 acc[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int ci = 0; ci < nch; ++ci) {
            const int mc = JAC ? ci : (rs + 1 + ci) % nch;     // second product: the slab's own chunk last (R = M: nrs = nch)
            const int c0 = mc * MT_MS, nc = min(MT_MS, M - c0);
            __syncthreads();                                   // (the points are staged; the previous chunk is consumed)
            for (int e = t; e < MT_MS * Q; e += 256) sz[e] = e / Q < nc ? zk[(size_t)c0 * Q + e] : 0.0;
            for (int e = t; e < MT_MS * MT_MS; e += 256) {
                // coalesced along A's contiguous index: the chunk index m' of p[m][m'], the row j of r[m'][j]
                const int rr = JAC ? e & 63 : e >> 6, cc = JAC ? e >> 6 : e & 63, row = r0 + rr, col = c0 + cc;
                double v = 0.0;
                if (row < R && col < M) v = JAC ? ak[(size_t)col * R + row] : ak[(size_t)row * M + col];
                sP[rr * MT_PS + cc] = v;
            }
            __syncthreads();
            for (int e = t; e < MT_MS * NP; e += 256) {
                const int rr = e / NP, i = e % NP;
                double v = 0.0, dv = 0.0, ev = 0.0, ddv = 0.0;
                [[maybe_unused]] double avt = 0.0;                  // transport: av, for the d(v, w_r) below
                if (rr < nc && n0 + i < N) {
                    double ex = 0.0, av = 0.0, s2 = 0.0, fv = 0.0, c1 = 0.0, c2 = 0.0;
                    for (int q = 0; q < Q; ++q) {
                        const double d = sx[i * Q + q] - sz[rr * Q + q];
                        ex = fma(-0.5 * DPGP_LOG2E * sg[q] * d, d, ex);
                        if constexpr (CHR) {
                            const double gv = sg[q] * sv[i * Q + q];
                            av = fma(gv, d, av);
                            s2 = fma(gv, sv[i * Q + q], s2);
                            if constexpr (TAN) {
                                const double u = sg[q] * d;
                                ev = fma(u, sdx[i * Q + q], ev);
                                fv = fma(u, sdv[i * Q + q], fv);
                                c1 = fma(gv, sdx[i * Q + q], c1);
                                c2 = fma(gv, sdv[i * Q + q], c2);
                            }
                        }
                    }
                    v = al * dpgp_exp2(ex);
                    if constexpr (CHR) dv = v * (av * av - s2);
                    if constexpr (TAN) ddv = v * (2.0 * av * (c1 + fv) - ev * (av * av - s2) - 2.0 * c2);
                    if constexpr (TRN) avt = av;
                }
                sk[e] = v;
                if constexpr (CHR) sd[e] = dv;
                if constexpr (TRN) {
                    // d(v, w_r) into column Q + 1 + r of the point's block, four vectors at a time (past F: the last one again,
                    // not stored): a_w by the fma sequence of av, sum_q gamma v w beside s2, the last line as dv's
                    double *bcol = sB + rr * BS + 16 * QT * i + Q + 1;
                    const bool live = rr < nc && n0 + i < N;
                    for (int f0 = 0; f0 < F; f0 += 4) {
                        double aw[4] = {0.0, 0.0, 0.0, 0.0}, cw[4] = {0.0, 0.0, 0.0, 0.0};
                        if (live)
                            for (int q = 0; q < Q; ++q) {
                                const double d = sx[i * Q + q] - sz[rr * Q + q], gv = sg[q] * sv[i * Q + q];
#pragma unroll
                                for (int u = 0; u < 4; ++u) {
                                    const double wq = sw[(i * F + min(f0 + u, F - 1)) * Q + q];
                                    aw[u] = fma(sg[q] * wq, d, aw[u]);
                                    cw[u] = fma(gv, wq, cw[u]);
                                }
                            }
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (f0 + u < F) bcol[f0 + u] = live ? v * (avt * aw[u] - cw[u]) : 0.0;
                    }
                }
                if constexpr (TAN) se[e] = ev, sdd[e] = ddv;
            }
            __syncthreads();
            for (int e = t; e < MT_MS * BS; e += 256) {
                const int rr = e / BS, col = e % BS, ct = col >> 4, i = ct / QT, q = ((ct % QT) << 4) + (col & 15);
                if constexpr (TRN)
                    if (ct < CT && q > Q && q <= Q + F) continue;   // (the d(v, w_r) columns are in place)
                double v = 0.0;
                if (ct < CT && q < Q) v = -sg[q] * (sx[i * Q + q] - sz[rr * Q + q]) * sk[rr * NP + i];
                if constexpr (CHR)
                    if (ct < CT && q == Q) v = sd[rr * NP + i];
                if constexpr (TAN) {
                    // db_q = k (e u_q - gamma_q dx_q) in columns Q + 1 .. 2 Q, dd in column 2 Q + 1
                    if (ct < CT && q > Q && q <= 2 * Q) {
                        const int r = q - Q - 1;
                        v = sk[rr * NP + i] * (se[rr * NP + i] * (sg[r] * (sx[i * Q + r] - sz[rr * Q + r])) - sg[r] * sdx[i * Q + r]);
                    }
                    if (ct < CT && q == 2 * Q + 1) v = sdd[rr * NP + i];
                }
                sB[e] = v;
            }
            __syncthreads();
            if (!wave_live) continue;
            const double *prow = sP + (16 * wave + li) * MT_PS + kk;
            for (int st = 0; st < (nc + 3) >> 2; ++st) {
                const double av = prow[4 * st];
                const double *brow = sB + (4 * st + kk) * BS + li;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[ct] = Mfma<double>::mma(av, brow[16 * ct], acc[ct]);
            }
        }
        if (!wave_live) continue;
        if constexpr (JAC) {
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const int n = n0 + ct / QT, q = ((ct % QT) << 4) + li;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = r0 + 16 * wave + Mfma<double>::row(lane, r);
                    if (n < N && q < Q && j < R) out[(((size_t)k * N + n) * R + j) * Q + q] = acc[ct][r];
                }
            }
        } else {
            // G_n += B_n^T U_n over the wave's 16 rows: sB holds the slab's own features (the chunk walked last)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double *brow = sB + (16 * wave + 4 * r + kk) * BS + li;
#pragma unroll
                for (int i = 0; i < NP; ++i)
#pragma unroll
                    for (int qi = 0; qi < QT; ++qi) {
                        const double bv = brow[16 * (i * QT + qi)];
#pragma unroll
                        for (int qj = 0; qj < QT; ++qj) {
                            if constexpr (TAN)
                                if (mt_tan_unread(QT, qi, qj)) continue;
                            if constexpr (TRN)
                                if (mt_trn_unread(Q, qi)) continue;
                            const int g = (i * QT + qi) * QT + qj;
                            G[g] = Mfma<double>::mma(bv, acc[i * QT + qj][r], G[g]);
                        }
                    }
            }
        }
    }
    if constexpr (!JAC) {
        double *sG = sB;                                           // [NG][4][64]: the waves' tiles added in wave order
        for (int w = 0; w < 4; ++w) {
            __syncthreads();                                       // (w = 0: every wave is done with the features)
            if (wave != w) continue;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if constexpr (TAN)
                    if (mt_tan_unread(QT, (g / QT) % QT, g % QT)) continue;
                if constexpr (TRN)
                    if (mt_trn_unread(Q, (g / QT) % QT)) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int o = (g * 4 + r) * 64 + lane;
                    sG[o] = w == 0 ? G[g][r] : sG[o] + G[g][r];
                }
            }
        }
        __syncthreads();
        // entry (row q, column c) of a point's product: tile (q >> 4, c >> 4), register (q & 15) >> 2, lane ((q & 3) << 4) | (c & 15).
        // A point's Q Q entries of g; christoffel: then its gam, the first Q rows of column Q
        const int qq = Q * Q, per = TAN ? 2 * (qq + Q) : TRN ? qq + Q + F * Q : CHR ? qq + Q : qq;
        if constexpr (TAN) {
            // then dg = (rows 0 .. Q - 1, columns Q + 1 .. 2 Q) + (rows Q + 1 .. 2 Q, columns 0 .. Q - 1) and
            // dgam = (rows Q + 1 .. 2 Q, column Q) + (rows 0 .. Q - 1, column 2 Q + 1)
            for (int e = t; e < NP * per; e += 256) {
                const int i = e / per, rem = e % per;
                if (n0 + i >= N) continue;
                const auto entry = [&](int q, int c) {
                    const int g = (i * QT + (q >> 4)) * QT + (c >> 4), row = q & 15, col = c & 15;
                    return sG[(g * 4 + (row >> 2)) * 64 + (((row & 3) << 4) | col)];
                };
                const size_t pt = (size_t)k * N + n0 + i;
                if (rem < qq) out[pt * qq + rem] = entry(rem / Q, rem % Q);
                else if (rem < qq + Q) out2[pt * Q + rem - qq] = entry(rem - qq, Q);
                else if (rem < 2 * qq + Q) {
                    const int r = rem - qq - Q, q = r / Q, c = r % Q;
                    ta.dg[pt * qq + r] = entry(q, Q + 1 + c) + entry(Q + 1 + q, c);
                } else {
                    const int q = rem - 2 * qq - Q;
                    ta.dgam[pt * Q + q] = entry(Q + 1 + q, Q) + entry(q, 2 * Q + 1);
                }
            }
        } else {
            for (int e = t; e < NP * per; e += 256) {
                const int i = e / per, rem = e % per;
                int q = rem / Q, c = rem % Q;
                if constexpr (CHR)
                    if (rem >= qq) q = rem - qq, c = Q;
                if constexpr (TRN)
                    if (rem >= qq + Q) q = (rem - qq - Q) % Q, c = Q + 1 + (rem - qq - Q) / Q;   // tgam[r][q]: row q of column Q + 1 + r
                if (n0 + i >= N) continue;
                const int g = (i * QT + (q >> 4)) * QT + (c >> 4), row = q & 15, col = c & 15;
                const double val = sG[(g * 4 + (row >> 2)) * 64 + (((row & 3) << 4) | col)];
                if (TRN && rem >= qq + Q) tr.tgam[((size_t)k * N + n0 + i) * F * Q + rem - qq - Q] = val;
                else if (CHR && rem >= qq) out2[((size_t)k * N + n0 + i) * Q + q] = val;
                else out[((size_t)k * N + n0 + i) * qq + rem] = val;
            }
        }
    }
}

// the tile count of a point's columns, and what follows from it: W = Q, Q + 1 (christoffel), 2 Q + 2 (tangent),
// Q + 1 + F (transport; F = 0 elsewhere)
template <MtMode MODE> int mt_qt(int Q, int F = 0) {
    return dpgp_ceil_div(MODE == MT_TANGENT ? 2 * Q + 2 : Q + (MODE == MT_CHRISTOFFEL || MODE == MT_TRANSPORT) + F, 16);
}

template <MtMode MODE> size_t mt_lds(int Q, int np, int bs, int F = 0) {
    // (x | v | dx | dv) and (k | d | e | dd); transport: christoffel's and the frame
    constexpr int V = MODE == MT_TANGENT ? 4 : MODE == MT_CHRISTOFFEL || MODE == MT_TRANSPORT ? 2 : 1;
    return sizeof(double) * ((size_t)V * np * Q + (size_t)np * F * Q + Q + (size_t)MT_MS * Q + V * MT_MS * np + MT_MS * MT_PS +
                             (size_t)MT_MS * bs);
}

inline int mt_frame() { return 0; }
inline int mt_frame(const MtTan &) { return 0; }
inline int mt_frame(const MtTrn &a) { return a.F; }

// K, N, M, R >= 1, 1 <= Q <= 64 (christoffel: 63, tangent: 31; transport: F >= 1 and Q + 1 + F <= 64), and sizes that the 32-bit
// grid and the int indices of the kernel hold
template <MtMode MODE> bool mt_shape_ok(int K, int N, int M, int Q, int R, int F = 0) {
    constexpr int max_q = MODE == MT_TANGENT ? MT_TANGENT_MAX_Q : MODE == MT_CHRISTOFFEL ? MT_CHRISTOFFEL_MAX_Q : DPGP_QX_PSI_MAX_Q;
    if (Q < 1 || Q > max_q) return false;                      // (before Q goes into a tile count)
    if (MODE == MT_TRANSPORT && (F < 1 || F > MT_TRANSPORT_MAX_W - 1 - Q)) return false;
    const int np = dpgp_dispatch_qt(mt_qt<MODE>(Q, F), [](auto qt) { return MtCfg<decltype(qt)::value>::NP; });
    // (transport: N F Q, the frame's size, is held by the size_t indices of the kernel)
    return dpgp_point_shape_ok(K, N, M, Q, R, max_q, np);
}

// tan: the tangent mode's MtTan, the transport mode's MtTrn, nothing otherwise
template <MtMode MODE, class... TAN_ARGS>
int mt_launch(int K, int N, int M, int Q, int R, const double *z, const double *x, const double *gamma, const double *alpha,
              const double *a, double *out, const double *vel, double *out2, hipStream_t st, TAN_ARGS... tan) {
    const int F = mt_frame(tan...);
    return dpgp_dispatch_qt(mt_qt<MODE>(Q, F), [&](auto qt) {
        using Cfg = MtCfg<decltype(qt)::value>;
        void (*const kernel)(int, int, int, int, int, const double *, const double *, const double *, const double *,
                             const double *, double *, const double *, double *, TAN_ARGS...) =
            mt_kernel<decltype(qt)::value, MODE, TAN_ARGS...>;
        const int ntn = dpgp_ceil_div(N, Cfg::NP);
        const size_t lds = mt_lds<MODE>(Q, Cfg::NP, Cfg::BS, F);
        if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(kernel), lds)) return DPGP_ERR_LAUNCH;
        DPGP_PRELAUNCH();
        hipLaunchKernelGGL(kernel, dim3((unsigned)((long)K * ntn)), dim3(256), lds, st, N, M, Q, R, ntn, z, x, gamma, alpha, a, out,
                           vel, out2, tan...);
        DPGP_LAUNCH_CHECK();
        return DPGP_OK;
    });
}

}  // namespace

extern "C" size_t dpgp_ard_rbf_point_metric_workspace_bytes(int K, int N, int M, int Q) {
    return mt_shape_ok<MT_METRIC>(K, N, M, Q, M) ? DPGP_POINT_WS : 0;
}

extern "C" int dpgp_ard_rbf_point_metric_f64(int K, int N, int M, int Q, const double *z, const double *x, const double *gamma,
                                             const double *alpha, const double *p, double *g, void *ws, size_t ws_bytes,
                                             void *stream) {
    if (K < 1) return -1;
    if (N < 1) return -2;
    if (M < 1) return -3;
    if (Q < 1 || Q > DPGP_QX_PSI_MAX_Q) return -4;
    if (!z) return -5;
    if (!x) return -6;
    if (!gamma) return -7;
    if (!alpha) return -8;
    if (!p) return -9;
    if (!g) return -10;
    if (!ws) return -11;
    const size_t need = dpgp_ard_rbf_point_metric_workspace_bytes(K, N, M, Q);
    if (need == 0 || ws_bytes < need) return -12;              // (need == 0: a shape past what the launch grid holds)
    return mt_launch<MT_METRIC>(K, N, M, Q, M, z, x, gamma, alpha, p, g, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" size_t dpgp_ard_rbf_point_jacobian_workspace_bytes(int K, int J, int N, int M, int Q) {
    return mt_shape_ok<MT_JACOBIAN>(K, N, M, Q, J) ? DPGP_POINT_WS : 0;
}

extern "C" int dpgp_ard_rbf_point_jacobian_f64(int K, int J, int N, int M, int Q, const double *z, const double *x,
                                               const double *gamma, const double *alpha, const double *r, double *jac, void *ws,
                                               size_t ws_bytes, void *stream) {
    if (K < 1) return -1;
    if (J < 1) return -2;
    if (N < 1) return -3;
    if (M < 1) return -4;
    if (Q < 1 || Q > DPGP_QX_PSI_MAX_Q) return -5;
    if (!z) return -6;
    if (!x) return -7;
    if (!gamma) return -8;
    if (!alpha) return -9;
    if (!r) return -10;
    if (!jac) return -11;
    if (!ws) return -12;
    const size_t need = dpgp_ard_rbf_point_jacobian_workspace_bytes(K, J, N, M, Q);
    if (need == 0 || ws_bytes < need) return -13;
    return mt_launch<MT_JACOBIAN>(K, N, M, Q, J, z, x, gamma, alpha, r, jac, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" size_t dpgp_ard_rbf_point_christoffel_workspace_bytes(int K, int N, int M, int Q) {
    return mt_shape_ok<MT_CHRISTOFFEL>(K, N, M, Q, M) ? DPGP_POINT_WS : 0;
}

extern "C" int dpgp_ard_rbf_point_christoffel_f64(int K, int N, int M, int Q, const double *z, const double *x, const double *v,
                                                  const double *gamma, const double *alpha, const double *p, double *g,
                                                  double *gam, void *ws, size_t ws_bytes, void *stream) {
    if (K < 1) return -1;
    if (N < 1) return -2;
    if (M < 1) return -3;
    if (Q < 1 || Q > MT_CHRISTOFFEL_MAX_Q) return -4;
    if (!z) return -5;
    if (!x) return -6;
    if (!v) return -7;
    if (!gamma) return -8;
    if (!alpha) return -9;
    if (!p) return -10;
    if (!g) return -11;
    if (!gam) return -12;
    if (!ws) return -13;
    const size_t need = dpgp_ard_rbf_point_christoffel_workspace_bytes(K, N, M, Q);
    if (need == 0 || ws_bytes < need) return -14;              // (need == 0: a shape past what the launch grid holds)
    return mt_launch<MT_CHRISTOFFEL>(K, N, M, Q, M, z, x, gamma, alpha, p, g, v, gam, (hipStream_t)stream);
}

extern "C" size_t dpgp_ard_rbf_point_christoffel_tangent_workspace_bytes(int K, int N, int M, int Q) {
    return mt_shape_ok<MT_TANGENT>(K, N, M, Q, M) ? DPGP_POINT_WS : 0;
}

extern "C" int dpgp_ard_rbf_point_christoffel_tangent_f64(int K, int N, int M, int Q, const double *z, const double *x,
                                                          const double *v, const double *dx, const double *dv,
                                                          const double *gamma, const double *alpha, const double *p, double *g,
                                                          double *gam, double *dg, double *dgam, void *ws, size_t ws_bytes,
                                                          void *stream) {
    if (K < 1) return -1;
    if (N < 1) return -2;
    if (M < 1) return -3;
    if (Q < 1 || Q > MT_TANGENT_MAX_Q) return -4;
    if (!z) return -5;
    if (!x) return -6;
    if (!v) return -7;
    if (!dx) return -8;
    if (!dv) return -9;
    if (!gamma) return -10;
    if (!alpha) return -11;
    if (!p) return -12;
    if (!g) return -13;
    if (!gam) return -14;
    if (!dg) return -15;
    if (!dgam) return -16;
    if (!ws) return -17;
    const size_t need = dpgp_ard_rbf_point_christoffel_tangent_workspace_bytes(K, N, M, Q);
    if (need == 0 || ws_bytes < need) return -18;              // (need == 0: a shape past what the launch grid holds)
    return mt_launch<MT_TANGENT>(K, N, M, Q, M, z, x, gamma, alpha, p, g, v, gam, (hipStream_t)stream, MtTan{dx, dv, dg, dgam});
}

extern "C" size_t dpgp_ard_rbf_point_transport_workspace_bytes(int K, int N, int M, int Q, int F) {
    return mt_shape_ok<MT_TRANSPORT>(K, N, M, Q, M, F) ? DPGP_POINT_WS : 0;
}

extern "C" int dpgp_ard_rbf_point_transport_f64(int K, int N, int M, int Q, int F, const double *z, const double *x, const double *v,
                                                const double *w, const double *gamma, const double *alpha, const double *p,
                                                double *g, double *gam, double *tgam, void *ws, size_t ws_bytes, void *stream) {
    if (K < 1) return -1;
    if (N < 1) return -2;
    if (M < 1) return -3;
    if (Q < 1 || Q > MT_TRANSPORT_MAX_W - 2) return -4;
    if (F < 1 || F > MT_TRANSPORT_MAX_W - 1 - Q) return -5;
    if (!z) return -6;
    if (!x) return -7;
    if (!v) return -8;
    if (!w) return -9;
    if (!gamma) return -10;
    if (!alpha) return -11;
    if (!p) return -12;
    if (!g) return -13;
    if (!gam) return -14;
    if (!tgam) return -15;
    if (!ws) return -16;
    const size_t need = dpgp_ard_rbf_point_transport_workspace_bytes(K, N, M, Q, F);
    if (need == 0 || ws_bytes < need) return -17;              // (need == 0: a shape past what the launch grid holds)
    return mt_launch<MT_TRANSPORT>(K, N, M, Q, M, z, x, gamma, alpha, p, g, v, gam, (hipStream_t)stream, MtTrn{w, tgam, F});
}
