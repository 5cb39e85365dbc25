// The geodesic equation of the expected metric at DETERMINISTIC latent points x [N][Q] with velocities v [N][Q]: two operators.
//
// (1) christoffel.  With k_km and the derivative features b_kmq of ard_rbf_point_metric.hip and
//   a_knm = sum_q gamma_kq (x_nq - z_kmq) v_nq
//   d_knm = v_n^T (d^2 k_km / dx dx)(x_n) v_n = k_km(x_n) (a_knm^2 - sum_q gamma_kq v_nq^2)
// the operator gives, for p [K][M][M] used as given,
//   g[k][n][q][q'] = sum_{m,m'} p[k][m][m'] b_kmq(x_n) b_km'q'(x_n)                      (what the metric operator returns)
//   gam[k][n][q]   = sum_{m,m'} b_kmq(x_n) p[k][m][m'] d_knm'
// For symmetric p, gam is the Christoffel symbol of the first kind of g contracted twice with v,
//   gam = (D_v g) v - 1/2 grad_x (v^T g v):      the (Hv)^T p c terms of the two parts cancel, H the Hessian features.
// Both come out of ONE product U = p [B | d]: the feature block of a point is [b_.1 .. b_.Q, d], W = Q + 1 columns wide, and
//   F^T p F,   F = [B | d] [M x W]
// holds g in its leading Q x Q block and gam in the first Q rows of its last column.  The layout is the metric kernel's with W in
// the place of Q: QT = ceil(W / 16), a point owns QT column tiles of 16, NP = 8, 2, 1, 1 points per workgroup for QT = 1 .. 4;
// for Q <= 15 the d column sits in the padding that the metric kernel carries anyway.  U = p F on v_mfma_f64_16x16x4 with p
// streamed in 64 x 64 tiles, the chunks of a slab walked in rotated order so that the slab's own features are in LDS when U
// is complete, then F^T U from the accumulators (the accumulator layout is the B-operand layout); the four waves' result tiles are
// added in wave order through LDS.  No atomics, no workspace, the order of every sum fixed by (M, Q): the same bits on every run;
// a point's results depend neither on N, nor on its place in x, nor on K.  Far-away points: dpgp_exp2 gives exact zeros and every
// product with them is 0.  1 <= Q <= 63 (W <= 64).
// LDS: 8 (2 NP Q + Q + 64 Q + 128 NP + 64 66 + 64 BS) bytes: 122.5 KiB at Q = 15, 107.0 KiB at Q = 63.
//
// (2) geodesic_accel.  Per point: G = sum_k g[k][n] (ascending k) + diag(prior), speed = v^T G v, G = L L^T,
//   a = -G^-1 sum_k gam[k][n].  One workgroup of one wave per point, the matrix in LDS, thread i owns row i of the right-looking
// factorisation (the lower triangle of G is read) and of the two substitutions.  A pivot that is not positive ends the point:
// info = its 1-based index, a = NaN; the other points never see it.  1 <= Q <= 64.
#include "internal.h"

#define CH_MS 64            // rows of p per slab = inner indices per chunk
#define CH_PS 66            // row stride of the p tile in LDS (the metric kernel's)
#define CH_MAX_N 0x3fffffff
#define CH_MAX_Q 63

namespace {

template <int QT> struct ChCfg {
    static constexpr int NP = QT == 1 ? 8 : QT == 2 ? 2 : 1;   // points per workgroup
    static constexpr int CT = NP * QT;                         // column tiles of 16
    static constexpr int NG = NP * QT * QT;                    // result tiles per wave
    static constexpr int BS = 16 * CT + (CT % 2 ? 32 : 16);    // row stride of sB: the 2 rows of a half wave on disjoint bank halves
};

template <int QT>
__global__ __launch_bounds__(256) void ch_kernel(int N, int M, int Q, int ntn, const double *__restrict__ z,
                                                 const double *__restrict__ x, const double *__restrict__ vel,
                                                 const double *__restrict__ gamma, const double *__restrict__ alpha,
                                                 const double *__restrict__ p, double *__restrict__ g, double *__restrict__ gam) {
    constexpr int NP = ChCfg<QT>::NP, CT = ChCfg<QT>::CT, NG = ChCfg<QT>::NG, BS = ChCfg<QT>::BS;
    static_assert(NG * 256 <= CH_MS * BS, "the waves' result tiles are added in the feature buffer");
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *sx = reinterpret_cast<double *>(smem_raw);      // [NP][Q]   the points, 0 past N
    double *sv = sx + (size_t)NP * Q;                        // [NP][Q]   the velocities, 0 past N
    double *sg = sv + (size_t)NP * Q;                        // [Q]       gamma_k
    double *sz = sg + Q;                                     // [64][Q]   z rows of the chunk, 0 past M
    double *sk = sz + (size_t)CH_MS * Q;                     // [64][NP]  k_km'(x_n), 0 past M or N
    double *sd = sk + CH_MS * NP;                            // [64][NP]  d_knm', 0 past M or N
    double *sP = sd + CH_MS * NP;                            // [64][PS]  p tile (slab rows x chunk indices), 0 out of range
    double *sB = sP + CH_MS * CH_PS;                         // [64][BS]  features [b | d] of the chunk, 0 in the padding
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kk = lane >> 4;
    const int nt = blockIdx.x % ntn, k = blockIdx.x / ntn, n0 = nt * NP;
    const double *zk = z + (size_t)k * M * Q, *gk = gamma + (size_t)k * Q;
    const double *pk = p + (size_t)k * M * M;
    const double al = alpha[k];
    for (int e = t; e < NP * Q; e += 256) {
        const bool in = n0 + e / Q < N;
        sx[e] = in ? x[(size_t)n0 * Q + e] : 0.0;
        sv[e] = in ? vel[(size_t)n0 * Q + e] : 0.0;
    }
    for (int q = t; q < Q; q += 256) sg[q] = gk[q];
    const int nch = (M + CH_MS - 1) / CH_MS;
    f64x4 G[NG];
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) G[gi] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int rs = 0; rs < nch; ++rs) {
        const int r0 = rs * CH_MS;
        const bool wave_live = r0 + 16 * wave < M;             // (wave-uniform)
        f64x4 acc[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int ci = 0; ci < nch; ++ci) {
            const int mc = (rs + 1 + ci) % nch;                // the slab's own chunk last
            const int c0 = mc * CH_MS, nc = min(CH_MS, M - c0);
            __syncthreads();                                   // (the points are staged; the previous chunk is consumed)
            for (int e = t; e < CH_MS * Q; e += 256) sz[e] = e / Q < nc ? zk[(size_t)c0 * Q + e] : 0.0;
            for (int e = t; e < CH_MS * CH_MS; e += 256) {
                const int rr = e >> 6, cc = e & 63, row = r0 + rr, col = c0 + cc;
                sP[rr * CH_PS + cc] = row < M && col < M ? pk[(size_t)row * M + col] : 0.0;
            }
            __syncthreads();
            for (int e = t; e < CH_MS * NP; e += 256) {
                const int rr = e / NP, i = e % NP;
                double kv = 0.0, dv = 0.0;
                if (rr < nc && n0 + i < N) {
                    double ex = 0.0, a = 0.0, s2 = 0.0;
                    for (int q = 0; q < Q; ++q) {
                        const double d = sx[i * Q + q] - sz[rr * Q + q], gv = sg[q] * sv[i * Q + q];
                        ex = fma(-0.5 * DPGP_LOG2E * sg[q] * d, d, ex);
                        a = fma(gv, d, a);
                        s2 = fma(gv, sv[i * Q + q], s2);
                    }
                    kv = al * dpgp_exp2(ex);
                    dv = kv * (a * a - s2);
                }
                sk[e] = kv;
                sd[e] = dv;
            }
            __syncthreads();
            for (int e = t; e < CH_MS * BS; e += 256) {
                const int rr = e / BS, col = e % BS, ct = col >> 4, i = ct / QT, q = ((ct % QT) << 4) + (col & 15);
                double v = 0.0;
                if (ct < CT) {
                    if (q < Q) v = -sg[q] * (sx[i * Q + q] - sz[rr * Q + q]) * sk[rr * NP + i];
                    else if (q == Q) v = sd[rr * NP + i];
                }
                sB[e] = v;
            }
            __syncthreads();
            if (!wave_live) continue;
            const double *prow = sP + (16 * wave + li) * CH_PS + kk;
            for (int st = 0; st < (nc + 3) >> 2; ++st) {
                const double av = prow[4 * st];
                const double *brow = sB + (4 * st + kk) * BS + li;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[ct] = Mfma<double>::mma(av, brow[16 * ct], acc[ct]);
            }
        }
        if (!wave_live) continue;
        // F_n^T U_n over the wave's 16 rows: sB holds the slab's own features (the chunk walked last)
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
                        const int gi = (i * QT + qi) * QT + qj;
                        G[gi] = Mfma<double>::mma(bv, acc[i * QT + qj][r], G[gi]);
                    }
                }
        }
    }
    double *sG = sB;                                           // [NG][4][64]: the waves' tiles added in wave order
    for (int w = 0; w < 4; ++w) {
        __syncthreads();                                       // (w = 0: every wave is done with the features)
        if (wave != w) continue;
#pragma unroll
        for (int gi = 0; gi < NG; ++gi)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = (gi * 4 + r) * 64 + lane;
                sG[o] = w == 0 ? G[gi][r] : sG[o] + G[gi][r];
            }
    }
    __syncthreads();
    // entry (row q, column c) of F^T p F: tile (q >> 4, c >> 4) of the point, register (q & 15) >> 2, lane ((q & 3) << 4) | (c & 15)
    const int qq = Q * Q, per = qq + Q;
    for (int e = t; e < NP * per; e += 256) {
        const int i = e / per, rem = e % per;
        if (n0 + i >= N) continue;
        const int q = rem < qq ? rem / Q : rem - qq, c = rem < qq ? rem % Q : Q;
        const int gi = (i * QT + (q >> 4)) * QT + (c >> 4), row = q & 15, col = c & 15;
        const double val = sG[(gi * 4 + (row >> 2)) * 64 + (((row & 3) << 4) | col)];
        if (rem < qq) g[((size_t)k * N + n0 + i) * qq + rem] = val;
        else gam[((size_t)k * N + n0 + i) * Q + q] = val;
    }
}

size_t ch_lds(int Q, int np, int bs) {
    return sizeof(double) * ((size_t)2 * np * Q + Q + (size_t)CH_MS * Q + 2 * CH_MS * np + CH_MS * CH_PS + (size_t)CH_MS * bs);
}

int ch_points(int Q) { const int qt = dpgp_ceil_div(Q + 1, 16); return qt == 1 ? 8 : qt == 2 ? 2 : 1; }

// K, N, M >= 1, 1 <= Q <= 63, and sizes that the 32-bit grid and the int indices of the kernel hold
bool ch_shape_ok(int K, int N, int M, int Q) {
    if (K < 1 || N < 1 || M < 1 || Q < 1 || Q > CH_MAX_Q) return false;
    if (N > CH_MAX_N || M > CH_MAX_N) return false;
    return (long)K * dpgp_ceil_div(N, ch_points(Q)) <= 0x7fffffffL;
}

template <int QT>
int ch_launch(int K, int N, int M, int Q, const double *z, const double *x, const double *v, const double *gamma,
              const double *alpha, const double *p, double *g, double *gam, hipStream_t st) {
    const int ntn = dpgp_ceil_div(N, ChCfg<QT>::NP);
    const size_t lds = ch_lds(Q, ChCfg<QT>::NP, ChCfg<QT>::BS);
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(ch_kernel<QT>), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL((ch_kernel<QT>), dim3((unsigned)((long)K * ntn)), dim3(256), lds, st, N, M, Q, ntn, z, x, v, gamma, alpha,
                       p, g, gam);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

// ---- the finishing kernel ---------------------------------------------------------------------------------------------------------
#define GA_MAX_Q 64

// sum_k p[k stride] in ascending k; the loads go eight at a time, the adds stay in order
__device__ __forceinline__ double ga_slab_sum(const double *__restrict__ p, int K, size_t stride) {
    double s = p[0];
    int k = 1;
    for (; k + 8 <= K; k += 8) {
        double part[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) part[u] = p[(size_t)(k + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += part[u];
    }
    for (; k < K; ++k) s += p[(size_t)k * stride];
    return s;
}

__global__ __launch_bounds__(64) void ga_kernel(int K, int N, int Q, const double *__restrict__ g, const double *__restrict__ gam,
                                                const double *__restrict__ prior, const double *__restrict__ vel,
                                                double *__restrict__ acc, double *__restrict__ speed, int *__restrict__ info) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int LD = Q + 1;
    double *sA = reinterpret_cast<double *>(smem_raw);      // [Q][Q + 1]  G, then L in its lower triangle
    double *sb = sA + (size_t)Q * LD;                        // [Q]         the right-hand side, then y
    double *sv = sb + Q;                                     // [Q]         v_n
    double *sr = sv + Q;                                     // [Q]         the rows' shares of v^T G v
    const int t = threadIdx.x, n = blockIdx.x, qq = Q * Q;
    const bool row_live = t < Q;
    for (int e = t; e < qq; e += 64) {
        const double s = ga_slab_sum(g + (size_t)n * qq + e, K, (size_t)N * qq);
        const int r = e / Q, c = e % Q;
        sA[r * LD + c] = r == c ? s + prior[r] : s;
    }
    if (row_live) {
        sb[t] = -ga_slab_sum(gam + (size_t)n * Q + t, K, (size_t)N * Q);
        sv[t] = vel[(size_t)n * Q + t];
    }
    __syncthreads();
    if (row_live) {
        double s = 0.0;
        for (int c = 0; c < Q; ++c) s = fma(sA[t * LD + c], sv[c], s);
        sr[t] = sv[t] * s;
    }
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int r = 0; r < Q; ++r) s += sr[r];
        speed[n] = s;
    }
    // right-looking Cholesky on the lower triangle: thread i owns row i
    int fail = 0;
    for (int j = 0; j < Q; ++j) {
        __syncthreads();
        const double d = sA[j * LD + j];                       // (every thread reads the same value: the exit is uniform)
        if (!(d > 0.0)) { fail = j + 1; break; }
        const double l = sqrt(d);
        const bool below = t > j && row_live;
        const double lij = below ? sA[t * LD + j] / l : 0.0;
        __syncthreads();
        if (t == j) sA[j * LD + j] = l;
        if (below) sA[t * LD + j] = lij;
        __syncthreads();
        if (below)
            for (int c = j + 1; c <= t; ++c) sA[t * LD + c] = fma(-lij, sA[c * LD + j], sA[t * LD + c]);
    }
    if (fail) {
        if (row_live) acc[(size_t)n * Q + t] = __builtin_nan("");
        if (t == 0) info[n] = fail;
        return;
    }
    // L y = rhs, column by column
    double y = 0.0;
    for (int j = 0; j < Q; ++j) {
        __syncthreads();
        const double yj = sb[j] / sA[j * LD + j];
        if (t == j) y = yj;
        if (t > j && row_live) sb[t] = fma(-sA[t * LD + j], yj, sb[t]);
    }
    __syncthreads();
    if (row_live) sb[t] = y;
    // L^T a = y, from the last row up
    double res = 0.0;
    for (int j = Q - 1; j >= 0; --j) {
        __syncthreads();
        const double aj = sb[j] / sA[j * LD + j];
        if (t == j) res = aj;
        if (t < j) sb[t] = fma(-sA[j * LD + t], aj, sb[t]);
    }
    if (row_live) acc[(size_t)n * Q + t] = res;
    if (t == 0) info[n] = 0;
}

}  // namespace

// The operator writes its results from the accumulators and needs no scratch memory; the query and the (ws, ws_bytes) pair are
// there so that every point operator is called the same way.  DPGP_POINT_CHRISTOFFEL_WS bytes for a shape in range, 0 outside.
#define DPGP_POINT_CHRISTOFFEL_WS 256

extern "C" size_t dpgp_ard_rbf_point_christoffel_workspace_bytes(int K, int N, int M, int Q) {
    return ch_shape_ok(K, N, M, Q) ? DPGP_POINT_CHRISTOFFEL_WS : 0;
}

extern "C" int dpgp_ard_rbf_point_christoffel_f64(int K, int N, int M, int Q, const double *z, const double *x, const double *v,
                                                  const double *gamma, const double *alpha, const double *p, double *g,
                                                  double *gam, void *ws, size_t ws_bytes, void *stream) {
    if (K < 1) return -1;
    if (N < 1) return -2;
    if (M < 1) return -3;
    if (Q < 1 || Q > CH_MAX_Q) return -4;
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
    hipStream_t st = (hipStream_t)stream;
    const int qt = dpgp_ceil_div(Q + 1, 16);
    return qt == 1   ? ch_launch<1>(K, N, M, Q, z, x, v, gamma, alpha, p, g, gam, st)
           : qt == 2 ? ch_launch<2>(K, N, M, Q, z, x, v, gamma, alpha, p, g, gam, st)
           : qt == 3 ? ch_launch<3>(K, N, M, Q, z, x, v, gamma, alpha, p, g, gam, st)
                     : ch_launch<4>(K, N, M, Q, z, x, v, gamma, alpha, p, g, gam, st);
}

extern "C" int dpgp_geodesic_accel_f64(int K, int N, int Q, const double *g, const double *gam, const double *prior,
                                       const double *v, double *a, double *speed, int *info, void *stream) {
    if (K < 1 || K > CH_MAX_N) return -1;
    if (N < 1 || N > CH_MAX_N) return -2;
    if (Q < 1 || Q > GA_MAX_Q) return -3;
    if (!g) return -4;
    if (!gam) return -5;
    if (!prior) return -6;
    if (!v) return -7;
    if (!a) return -8;
    if (!speed) return -9;
    if (!info) return -10;
    const size_t lds = sizeof(double) * ((size_t)Q * (Q + 1) + 3 * Q);
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(ga_kernel, dim3((unsigned)N), dim3(64), lds, (hipStream_t)stream, K, N, Q, g, gam, prior, v, a, speed, info);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}
