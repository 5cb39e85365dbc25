// The finishing step of the geodesic equation of the expected metric at DETERMINISTIC latent points x [N][Q] with velocities
// v [N][Q], from the pair (g, gam) of the christoffel operator (ard_rbf_point_metric.hip).  Per point:
//   G = sum_k g[k][n] (ascending k) + diag(prior),   speed = v^T G v,   G = L L^T,   a = -G^-1 sum_k gam[k][n].
// One workgroup of one wave per point, the matrix in LDS, thread i owns row i of the right-looking factorisation (the lower
// triangle of G is read) and of the two substitutions.  A pivot that is not positive ends the point: info = its 1-based index,
// a = NaN; the other points never see it.  1 <= Q <= 64.
// The tangent operator (gat_kernel) takes the tangent mode's (dg, dgam) as well and solves a second time with the same factor:
//   da = -G^-1 (sum_k dgam[k][n] + (sum_k dg[k][n]) a);     a, speed and info carry ga_kernel's bits.
#include "point_tile.h"

#define GA_MAX_Q 64

namespace {

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

// L y = sb then L^T r = y in place on sb, thread t owning row t; returns r_t.  Every thread of the workgroup calls it.
__device__ __forceinline__ double gat_solve(const double *sA, double *sb, int Q, int LD, int t, bool row_live) {
    double y = 0.0;
    for (int j = 0; j < Q; ++j) {
        __syncthreads();
        const double yj = sb[j] / sA[j * LD + j];
        if (t == j) y = yj;
        if (t > j && row_live) sb[t] = fma(-sA[t * LD + j], yj, sb[t]);
    }
    __syncthreads();
    if (row_live) sb[t] = y;
    double res = 0.0;
    for (int j = Q - 1; j >= 0; --j) {
        __syncthreads();
        const double rj = sb[j] / sA[j * LD + j];
        if (t == j) res = rj;
        if (t < j) sb[t] = fma(-sA[j * LD + t], rj, sb[t]);
    }
    return res;
}

// ga_kernel's work, statement for statement (a, speed and info come out with its bits), and then with the same factor
//   da = -G^-1 (sum_k dgam[k][n] + (sum_k dg[k][n]) a):     the tangent of a along the direction that dg, dgam were taken in
// (the prior is constant and has no share in the tangent of G).  A failing pivot ends the point: a = da = NaN.
__global__ __launch_bounds__(64) void gat_kernel(int K, int N, int Q, const double *__restrict__ g, const double *__restrict__ gam,
                                                 const double *__restrict__ dg, const double *__restrict__ dgam,
                                                 const double *__restrict__ prior, const double *__restrict__ vel,
                                                 double *__restrict__ acc, double *__restrict__ dacc, double *__restrict__ speed,
                                                 int *__restrict__ info) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int LD = Q + 1;
    double *sA = reinterpret_cast<double *>(smem_raw);      // [Q][Q + 1]  G, then L in its lower triangle
    double *sb = sA + (size_t)Q * LD;                        // [Q]         the right-hand side, then y
    double *sv = sb + Q;                                     // [Q]         v_n
    double *sr = sv + Q;                                     // [Q]         the rows' shares of v^T G v
    double *sD = sr + Q;                                     // [Q][Q + 1]  sum_k dg
    double *sc = sD + (size_t)Q * LD;                        // [Q]         sum_k dgam
    double *sa = sc + Q;                                     // [Q]         a_n
    const int t = threadIdx.x, n = blockIdx.x, qq = Q * Q;
    const bool row_live = t < Q;
    for (int e = t; e < qq; e += 64) {
        const double s = ga_slab_sum(g + (size_t)n * qq + e, K, (size_t)N * qq);
        const int r = e / Q, c = e % Q;
        sA[r * LD + c] = r == c ? s + prior[r] : s;
        sD[r * LD + c] = ga_slab_sum(dg + (size_t)n * qq + e, K, (size_t)N * qq);
    }
    if (row_live) {
        sb[t] = -ga_slab_sum(gam + (size_t)n * Q + t, K, (size_t)N * Q);
        sv[t] = vel[(size_t)n * Q + t];
        sc[t] = ga_slab_sum(dgam + (size_t)n * Q + t, K, (size_t)N * Q);
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
        if (row_live) acc[(size_t)n * Q + t] = dacc[(size_t)n * Q + t] = __builtin_nan("");
        if (t == 0) info[n] = fail;
        return;
    }
    const double res = gat_solve(sA, sb, Q, LD, t, row_live);
    if (row_live) acc[(size_t)n * Q + t] = sa[t] = res;
    if (t == 0) info[n] = 0;
    __syncthreads();
    if (row_live) {
        double s = sc[t];
        for (int c = 0; c < Q; ++c) s = fma(sD[t * LD + c], sa[c], s);
        sb[t] = -s;
    }
    const double dres = gat_solve(sA, sb, Q, LD, t, row_live);
    if (row_live) dacc[(size_t)n * Q + t] = dres;
}

}  // namespace

extern "C" int dpgp_geodesic_accel_tangent_f64(int K, int N, int Q, const double *g, const double *gam, const double *dg,
                                               const double *dgam, const double *prior, const double *v, double *a, double *da,
                                               double *speed, int *info, void *stream) {
    if (K < 1 || K > DPGP_POINT_MAX_N) return -1;
    if (N < 1 || N > DPGP_POINT_MAX_N) return -2;
    if (Q < 1 || Q > GA_MAX_Q) return -3;
    if (!g) return -4;
    if (!gam) return -5;
    if (!dg) return -6;
    if (!dgam) return -7;
    if (!prior) return -8;
    if (!v) return -9;
    if (!a) return -10;
    if (!da) return -11;
    if (!speed) return -12;
    if (!info) return -13;
    const size_t lds = sizeof(double) * (2 * (size_t)Q * (Q + 1) + 5 * Q);       // 67.5 KiB at Q = 64
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(gat_kernel), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(gat_kernel, dim3((unsigned)N), dim3(64), lds, (hipStream_t)stream, K, N, Q, g, gam, dg, dgam, prior, v, a, da,
                       speed, info);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

extern "C" int dpgp_geodesic_accel_f64(int K, int N, int Q, const double *g, const double *gam, const double *prior,
                                       const double *v, double *a, double *speed, int *info, void *stream) {
    if (K < 1 || K > DPGP_POINT_MAX_N) return -1;
    if (N < 1 || N > DPGP_POINT_MAX_N) return -2;
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
