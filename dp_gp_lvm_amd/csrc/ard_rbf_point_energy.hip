// Curve energy of K ARD-RBF kernels at DETERMINISTIC latent points x [N][Q] along directions v [N][Q], with both gradients.  With
//   k_km(x_n)  = alpha_k exp(-1/2 sum_q gamma_kq (x_nq - z_kmq)^2),      d_knmq = x_nq - z_kmq
//   a_knm = sum_q gamma_kq d_knmq v_nq,     c_knm = sum_q b_kmq(x_n) v_nq = -k_km(x_n) a_knm       (b: ard_rbf_point_metric.hip)
//   w_knm = sum_m' (p[k][m][m'] + p[k][m'][m]) c_knm'                                              p [K][M][M], any matrices
// the operator gives
//   e  [K][N]    = sum_{m,m'} p[k][m][m'] c_knm c_knm' = 1/2 sum_m w_knm c_knm           (= v_n^T g[k][n] v_n of the metric operator)
//   dx [K][N][Q] = d e / d x_nq = gamma_kq sum_m w_knm k_km (a_knm d_knmq - v_nq)
//   dv [K][N][Q] = d e / d v_nq = -gamma_kq sum_m w_knm k_km d_knmq
// One M x M product per (kernel, point) where the metric needs Q of them.  Nothing of size N M is written to memory.
//
// Layout.  Workgroup (kernel k, tile of 16 points = ONE column tile of v_mfma_f64_16x16x4), 256 threads = 4 waves.  The product
//   W [M x 16] = (p_k + p_k^T) C [M x 16]
// runs as in mt_kernel: the rows of W go in slabs of 64, wave w owns rows 16 w .. 16 w + 15 of the slab and one accumulator; the
// inner index m' goes in chunks of 64.  Per chunk the z rows [64][Q], the triples (c, k, a) [64][16] each and the SYMMETRISED tile
// sP [64][64 (+ pad)] are staged in LDS: the transposed tile p[m'][m] is read along ITS contiguous index m and written transposed,
// then p[m][m'] is added along m' (both global reads coalesce); one exponential per (k, n, m') and per slab.  The global values
// of a step pass through registers, loaded one step ahead under the previous step's matrix work.  p is streamed in
// these tiles and never resident: no size limit on M from the LDS.  The chunks of a slab are walked in the rotated order
// slab + 1, .., nch - 1, 0, .., slab, so the slab's own chunk comes last and ITS (c, k, a) and z rows are the ones in LDS when W is
// complete.  Then every lane turns the triples of its 4 rows in place into (w c, w k, w k a) with W from its accumulator, and the
// block adds the slab's rows to the finishing sums: thread (point n, column j) keeps
//   j < Q:  sum_m (w k) d_mj,   sum_m (w k a) d_mj,   sum_m w k        j = Q:  sum_m w c
// over all slabs in registers, with the differences d = x - z formed on the fly: ascending m, one thread per sum, nothing to
// reduce across waves.  At the end  e = 1/2 sum w c,  dx_j = gamma_j (sum (w k a) d_j - v_j sum w k),  dv_j = -gamma_j sum (w k) d_j.
// The order of every sum is fixed by (M, Q) alone: no atomics, no workspace, the same bits on every run; a point is one column of
// every matrix step, so its bits depend neither on N, nor on its place in the tile, nor on K or the other kernels.  Far-away
// points: dpgp_exp2 gives k = 0 exactly, then c = w = 0 and every product with them is 0.
// LDS: 8 (16 Q + 16 Q + Q + 64 Q + 64 48 + 64 66) = 776 Q + 58368 bytes: 64.6 KiB at Q = 10 (two workgroups per CU), 105.5 KiB at Q = 64.
#include "point_tile.h"

#define PE_MS DPGP_POINT_MS // rows of W per slab = inner indices per chunk
#define PE_PS DPGP_POINT_PS // row stride of the p tile in LDS
#define PE_NP 16            // points per workgroup
#define PE_CS 48            // row stride of the (c | k | a) rows: the 2 rows of a half wave's B operand on disjoint bank halves

namespace {

template <int QT>
__global__ __launch_bounds__(256) void pe_kernel(int N, int M, int Q, int ntn, const double *__restrict__ z,
                                                 const double *__restrict__ x, const double *__restrict__ v,
                                                 const double *__restrict__ gamma, const double *__restrict__ alpha,
                                                 const double *__restrict__ p, double *__restrict__ e_out,
                                                 double *__restrict__ dx, double *__restrict__ dv) {
    constexpr int NPR = QT + 1;                              // (point, column) sums per thread: 16 (Q + 1) <= 256 NPR
    constexpr int NZ = 4 * QT;                               // z values of a chunk per thread: 64 Q <= 256 NZ
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *sx = reinterpret_cast<double *>(smem_raw);      // [Q][16]   the points, transposed, 0 past N
    double *sv = sx + (size_t)PE_NP * Q;                     // [Q][16]   the directions, transposed, 0 past N
    double *sg = sv + (size_t)PE_NP * Q;                     // [Q]       gamma_k
    double *sz = sg + Q;                                     // [64][Q]   z rows of the chunk, 0 past M
    double *sC = sz + (size_t)PE_MS * Q;                     // [64][CS]  (c | k | a) [16] each of the chunk, 0 past M or N
    double *sP = sC + PE_MS * PE_CS;                         // [64][PS]  p + p^T tile (slab rows x chunk indices), 0 out of range
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kk = lane >> 4;
    const int nt = blockIdx.x % ntn, k = blockIdx.x / ntn, n0 = nt * PE_NP;
    const double *zk = z + (size_t)k * M * Q, *gk = gamma + (size_t)k * Q;
    const double *pk = p + (size_t)k * M * M;
    const double al = alpha[k];
    for (int e = t; e < PE_NP * Q; e += 256) {
        const int i = e / Q, q = e % Q;
        const bool in = n0 + i < N;
        sx[q * PE_NP + i] = in ? x[(size_t)n0 * Q + e] : 0.0;
        sv[q * PE_NP + i] = in ? v[(size_t)n0 * Q + e] : 0.0;
    }
    for (int q = t; q < Q; q += 256) sg[q] = gk[q];
    const int nch = (M + PE_MS - 1) / PE_MS;
    double s0[NPR], s1[NPR], s2[NPR];                         // sum (w k) d | sum w c;   sum (w k a) d;   sum w k
#pragma unroll
    for (int i = 0; i < NPR; ++i) s0[i] = s1[i] = s2[i] = 0.0;
    // The p and z values of a step (slab, chunk) go through registers: all of a thread's loads are issued together, unconditionally
    // (out-of-range indices clamped, the values then replaced by 0), one step ahead, so they fly under the previous step's work.
    const int tl = t & 63, th = t >> 6;
    double pa[16], pb[16], zr[NZ];                            // p[m'][m] at (m = tl, m' = th + 4 i), p[m][m'] at (m = th + 4 i, m' = tl)
    auto fetch = [&](int frs, int fci) {
        const int fr0 = frs * PE_MS, fc0 = ((frs + 1 + fci) % nch) * PE_MS;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int a = th + 4 * i, rowa = fr0 + tl, cola = fc0 + a, rowb = fr0 + a, colb = fc0 + tl;
            const double ga = pk[(size_t)min(cola, M - 1) * M + min(rowa, M - 1)];
            const double gb = pk[(size_t)min(rowb, M - 1) * M + min(colb, M - 1)];
            pa[i] = rowa < M && cola < M ? ga : 0.0;
            pb[i] = rowb < M && colb < M ? gb : 0.0;
        }
        const long zend = (long)M * Q - 1;
#pragma unroll
        for (int i = 0; i < NZ; ++i) {
            const long at = (long)fc0 * Q + t + 256 * i;
            const double g = zk[at < zend ? at : zend];
            zr[i] = at <= zend ? g : 0.0;
        }
    };
    fetch(0, 0);
    for (int rs = 0; rs < nch; ++rs) {
        const int r0 = rs * PE_MS, nr = min(PE_MS, M - r0);
        const bool wave_live = r0 + 16 * wave < M;             // (wave-uniform)
        f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int ci = 0; ci < nch; ++ci) {
            const int mc = (rs + 1 + ci) % nch;                // the slab's own chunk last
            const int c0 = mc * PE_MS, nc = min(PE_MS, M - c0);
            __syncthreads();                                   // (the points are staged; the previous chunk and slab are consumed)
#pragma unroll
            for (int i = 0; i < NZ; ++i)
                if (t + 256 * i < PE_MS * Q) sz[t + 256 * i] = zr[i];
#pragma unroll
            for (int i = 0; i < 16; ++i) sP[tl * PE_PS + th + 4 * i] = pa[i];       // p[m'][m], read along m, written transposed
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 16; ++i) sP[(th + 4 * i) * PE_PS + tl] += pb[i];    // + p[m][m'], read along m'
            if (ci + 1 < nch) fetch(rs, ci + 1);
            else if (rs + 1 < nch) fetch(rs + 1, 0);
            for (int e = t; e < PE_MS * PE_NP; e += 256) {
                const int rr = e >> 4, i = e & 15;
                double kv = 0.0, av = 0.0;
                if (rr < nc && n0 + i < N) {
                    double ex = 0.0;
                    for (int q = 0; q < Q; ++q) {
                        const double g = sg[q], d = sx[q * PE_NP + i] - sz[rr * Q + q];
                        ex = fma(-0.5 * DPGP_LOG2E * g * d, d, ex);
                        av = fma(g * d, sv[q * PE_NP + i], av);
                    }
                    kv = al * dpgp_exp2(ex);
                }
                double *row = sC + rr * PE_CS + i;
                row[0] = -kv * av;
                row[16] = kv;
                row[32] = av;
            }
            __syncthreads();
            if (wave_live) {
                const double *prow = sP + (16 * wave + li) * PE_PS + kk;
                const double *brow = sC + kk * PE_CS + li;
                for (int st = 0; st < (nc + 3) >> 2; ++st) acc = Mfma<double>::mma(prow[4 * st], brow[4 * st * PE_CS], acc);
            }
        }
        __syncthreads();                                       // every wave is done with the B operands of the slab's own chunk
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            // (c, k, a) -> (w c, w k, w k a) of row 16 wave + kk + 4 r, point li: the accumulator layout of v_mfma_f64_16x16x4
            double *row = sC + (16 * wave + Mfma<double>::row(lane, r)) * PE_CS + li;
            const double w = acc[r], u = w * row[16];
            row[0] = w * row[0];
            row[16] = u;
            row[32] = u * row[32];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NPR; ++i) {
            const int e = t + 256 * i, n = e & 15, j = e >> 4;
            if (j < Q) {
                const double xq = sx[j * PE_NP + n];
                for (int m = 0; m < nr; ++m) {
                    const double u = sC[m * PE_CS + 16 + n], d = xq - sz[m * Q + j];
                    s0[i] = fma(u, d, s0[i]);
                    s1[i] = fma(sC[m * PE_CS + 32 + n], d, s1[i]);
                    s2[i] += u;
                }
            } else if (j == Q) {
                for (int m = 0; m < nr; ++m) s0[i] += sC[m * PE_CS + n];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NPR; ++i) {
        const int e = t + 256 * i, n = e & 15, j = e >> 4;
        if (n0 + n >= N || j > Q) continue;
        const size_t pt = (size_t)k * N + n0 + n;
        if (j == Q) {
            e_out[pt] = 0.5 * s0[i];
        } else {
            dx[pt * Q + j] = sg[j] * (s1[i] - sv[j * PE_NP + n] * s2[i]);
            dv[pt * Q + j] = -sg[j] * s0[i];
        }
    }
}

size_t pe_lds(int Q) {
    return sizeof(double) * ((size_t)2 * PE_NP * Q + Q + (size_t)PE_MS * Q + PE_MS * PE_CS + PE_MS * PE_PS);
}

template <int QT>
int pe_launch(int K, int N, int M, int Q, const double *z, const double *x, const double *v, const double *gamma,
              const double *alpha, const double *p, double *e, double *dx, double *dv, hipStream_t st) {
    const int ntn = dpgp_ceil_div(N, PE_NP);
    const size_t lds = pe_lds(Q);
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(pe_kernel<QT>), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL((pe_kernel<QT>), dim3((unsigned)((long)K * ntn)), dim3(256), lds, st, N, M, Q, ntn, z, x, v, gamma, alpha,
                       p, e, dx, dv);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

}  // namespace

extern "C" size_t dpgp_ard_rbf_point_energy_workspace_bytes(int K, int N, int M, int Q) {
    return dpgp_point_shape_ok(K, N, M, Q, M, DPGP_QX_PSI_MAX_Q, PE_NP) ? DPGP_POINT_WS : 0;
}

extern "C" int dpgp_ard_rbf_point_energy_f64(int K, int N, int M, int Q, const double *z, const double *x, const double *v,
                                             const double *gamma, const double *alpha, const double *p, double *e, double *dx,
                                             double *dv, void *ws, size_t ws_bytes, void *stream) {
    if (K < 1) return -1;
    if (N < 1) return -2;
    if (M < 1) return -3;
    if (Q < 1 || Q > DPGP_QX_PSI_MAX_Q) return -4;
    if (!z) return -5;
    if (!x) return -6;
    if (!v) return -7;
    if (!gamma) return -8;
    if (!alpha) return -9;
    if (!p) return -10;
    if (!e) return -11;
    if (!dx) return -12;
    if (!dv) return -13;
    if (!ws) return -14;
    const size_t need = dpgp_ard_rbf_point_energy_workspace_bytes(K, N, M, Q);
    if (need == 0 || ws_bytes < need) return -15;              // (need == 0: a shape past what the launch grid holds)
    const hipStream_t st = (hipStream_t)stream;
    return dpgp_dispatch_qt(dpgp_ceil_div(Q, 16), [&](auto qt) {
        return pe_launch<decltype(qt)::value>(K, N, M, Q, z, x, v, gamma, alpha, p, e, dx, dv, st);
    });
}
