// Latent-space metric and predictive Jacobian of K ARD-RBF kernels at DETERMINISTIC latent points x [N][Q].  With
//   k_km(x_n)  = alpha_k exp(-1/2 sum_q gamma_kq (x_nq - z_kmq)^2)
//   b_kmq(x_n) = d k_km / d x_q = -gamma_kq (x_nq - z_kmq) k_km(x_n)                    the derivative features [M x Q] of point n
// the two operators are
//   metric:    g[k][n][q][q']  = sum_{m,m'} p[k][m][m'] b_kmq(x_n) b_km'q'(x_n)           p [K][M][M], used as given (not symmetrised)
//   jacobian:  jac[k][n][j][q] = sum_m b_kmq(x_n) r[k][m][j]                             r [K][M][J]
// The features B [M x (points, q)] are never stored to memory: a workgroup makes them on the fly, 64 inducing points at a time,
// into LDS, one exponential per (k, n, m) and per slab of 64 rows of the left operand.
//
// Layout.  Workgroup (kernel k, tile of NP points), 256 threads = 4 waves.  With QT = ceil(Q / 16) a point owns QT column tiles of 16
// (its q padded to 16 QT), NP = 8, 2, 1, 1 points for QT = 1 .. 4, CT = NP QT column tiles in all.  Both operators are the product
//   U [R x (point, q)] = A [R x M] B [M x (point, q)]          metric: A = p_k, R = M;   jacobian: A = r_k^T, R = J
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
// The order of every sum is fixed by (M, Q) alone: no atomics, no workspace, the same bits on every run, and a kernel's results
// do not depend on K or on the other kernels.  Far-away points: dpgp_exp2 gives exact zeros, every product with them is 0.
// LDS: 8 (NP Q + Q + 64 Q + 64 NP + 64 66 + 64 BS) bytes, BS = 16 CT + 16 (+ 16 for odd CT): 120.4 KiB at Q = 16, 109.5 KiB at Q = 64.
#include "internal.h"

#define MT_MS 64            // rows of A per slab = inner indices per chunk
#define MT_PS 66            // row stride of the A tile in LDS: lanes (i, kk) of a half wave fall on 32 distinct bank pairs
#define MT_MAX_N 0x3fffffff

namespace {

template <int QT> struct MtCfg {
    static constexpr int NP = QT == 1 ? 8 : QT == 2 ? 2 : 1;   // points per workgroup
    static constexpr int CT = NP * QT;                         // column tiles of 16
    static constexpr int NG = NP * QT * QT;                    // result tiles of the metric per wave
    static constexpr int BS = 16 * CT + (CT % 2 ? 32 : 16);    // row stride of sB: the 2 rows of a half wave on disjoint bank halves
};

template <int QT, bool JAC>
__global__ __launch_bounds__(256) void mt_kernel(int N, int M, int Q, int R, int ntn, const double *__restrict__ z,
                                                 const double *__restrict__ x, const double *__restrict__ gamma,
                                                 const double *__restrict__ alpha, const double *__restrict__ a,
                                                 double *__restrict__ out) {
    constexpr int NP = MtCfg<QT>::NP, CT = MtCfg<QT>::CT, NG = MtCfg<QT>::NG, BS = MtCfg<QT>::BS;
    static_assert(NG * 256 <= MT_MS * BS, "the waves' result tiles are added in the feature buffer");
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *sx = reinterpret_cast<double *>(smem_raw);      // [NP][Q]   the points, 0 past N
    double *sg = sx + (size_t)NP * Q;                        // [Q]       gamma_k
    double *sz = sg + Q;                                     // [64][Q]   z rows of the chunk, 0 past M
    double *sk = sz + (size_t)MT_MS * Q;                     // [64][NP]  k_km'(x_n), 0 past M or N
    double *sP = sk + MT_MS * NP;                            // [64][PS]  A tile (slab rows x chunk indices), 0 out of range
    double *sB = sP + MT_MS * MT_PS;                         // [64][BS]  features of the chunk, 0 in the padding
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kk = lane >> 4;
    const int nt = blockIdx.x % ntn, k = blockIdx.x / ntn, n0 = nt * NP;
    const double *zk = z + (size_t)k * M * Q, *gk = gamma + (size_t)k * Q;
    const double *ak = a + (size_t)k * M * R;
    const double al = alpha[k];
    for (int e = t; e < NP * Q; e += 256) sx[e] = n0 + e / Q < N ? x[(size_t)n0 * Q + e] : 0.0;
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
            const int mc = JAC ? ci : (rs + 1 + ci) % nch;     // metric: the slab's own chunk last (R = M: nrs = nch)
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
                double v = 0.0;
                if (rr < nc && n0 + i < N) {
                    double ex = 0.0;
                    for (int q = 0; q < Q; ++q) {
                        const double d = sx[i * Q + q] - sz[rr * Q + q];
                        ex = fma(-0.5 * DPGP_LOG2E * sg[q] * d, d, ex);
                    }
                    v = al * dpgp_exp2(ex);
                }
                sk[e] = v;
            }
            __syncthreads();
            for (int e = t; e < MT_MS * BS; e += 256) {
                const int rr = e / BS, col = e % BS, ct = col >> 4, i = ct / QT, q = ((ct % QT) << 4) + (col & 15);
                double v = 0.0;
                if (ct < CT && q < Q) v = -sg[q] * (sx[i * Q + q] - sz[rr * Q + q]) * sk[rr * NP + i];
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
            // g_n += B_n^T U_n over the wave's 16 rows: sB holds the slab's own features (the chunk walked last)
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
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int o = (g * 4 + r) * 64 + lane;
                    sG[o] = w == 0 ? G[g][r] : sG[o] + G[g][r];
                }
        }
        __syncthreads();
        const int qq = Q * Q;
        for (int e = t; e < NP * qq; e += 256) {
            const int i = e / qq, rem = e % qq, q = rem / Q, qp = rem % Q;
            if (n0 + i >= N) continue;
            const int g = (i * QT + (q >> 4)) * QT + (qp >> 4), row = q & 15, col = qp & 15;
            out[((size_t)k * N + n0 + i) * qq + rem] = sG[(g * 4 + (row >> 2)) * 64 + (((row & 3) << 4) | col)];
        }
    }
}

size_t mt_lds(int Q, int np, int bs) {
    return sizeof(double) * ((size_t)np * Q + Q + (size_t)MT_MS * Q + MT_MS * np + MT_MS * MT_PS + (size_t)MT_MS * bs);
}

int mt_points(int Q) { const int qt = dpgp_ceil_div(Q, 16); return qt == 1 ? 8 : qt == 2 ? 2 : 1; }

// K, N, M, R >= 1, 1 <= Q <= 64, and sizes that the 32-bit grid and the int indices of the kernel hold
bool mt_shape_ok(int K, int N, int M, int Q, int R) {
    if (K < 1 || N < 1 || M < 1 || R < 1 || Q < 1 || Q > DPGP_QX_PSI_MAX_Q) return false;
    if (N > MT_MAX_N || M > MT_MAX_N || R > MT_MAX_N) return false;
    return (long)K * dpgp_ceil_div(N, mt_points(Q)) <= 0x7fffffffL;
}

template <int QT, bool JAC>
int mt_launch(int K, int N, int M, int Q, int R, const double *z, const double *x, const double *gamma, const double *alpha,
              const double *a, double *out, hipStream_t st) {
    const int ntn = dpgp_ceil_div(N, MtCfg<QT>::NP);
    const size_t lds = mt_lds(Q, MtCfg<QT>::NP, MtCfg<QT>::BS);
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(mt_kernel<QT, JAC>), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL((mt_kernel<QT, JAC>), dim3((unsigned)((long)K * ntn)), dim3(256), lds, st, N, M, Q, R, ntn, z, x, gamma,
                       alpha, a, out);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

template <bool JAC>
int mt_dispatch(int K, int N, int M, int Q, int R, const double *z, const double *x, const double *gamma, const double *alpha,
                const double *a, double *out, hipStream_t st) {
    const int qt = dpgp_ceil_div(Q, 16);
    return qt == 1   ? mt_launch<1, JAC>(K, N, M, Q, R, z, x, gamma, alpha, a, out, st)
           : qt == 2 ? mt_launch<2, JAC>(K, N, M, Q, R, z, x, gamma, alpha, a, out, st)
           : qt == 3 ? mt_launch<3, JAC>(K, N, M, Q, R, z, x, gamma, alpha, a, out, st)
                     : mt_launch<4, JAC>(K, N, M, Q, R, z, x, gamma, alpha, a, out, st);
}

}  // namespace

// The operators write their results from the accumulators and need no scratch memory; the query and the (ws, ws_bytes) pair
// are there so that every point operator is called the same way.  DPGP_POINT_METRIC_WS bytes for a shape in range, 0 outside.
#define DPGP_POINT_METRIC_WS 256

extern "C" size_t dpgp_ard_rbf_point_metric_workspace_bytes(int K, int N, int M, int Q) {
    return mt_shape_ok(K, N, M, Q, M) ? DPGP_POINT_METRIC_WS : 0;
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
    return mt_dispatch<false>(K, N, M, Q, M, z, x, gamma, alpha, p, g, (hipStream_t)stream);
}

extern "C" size_t dpgp_ard_rbf_point_jacobian_workspace_bytes(int K, int J, int N, int M, int Q) {
    return mt_shape_ok(K, N, M, Q, J) ? DPGP_POINT_METRIC_WS : 0;
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
    return mt_dispatch<true>(K, N, M, Q, J, z, x, gamma, alpha, r, jac, (hipStream_t)stream);
}
