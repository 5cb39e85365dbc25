// The finishing step of the geodesic equation of the expected metric at DETERMINISTIC latent points x [N][Q] with velocities
// v [N][Q], from the pair (g, gam) of the christoffel operator (ard_rbf_point_metric.hip).  Per point:
//   G = sum_k g[k][n] (ascending k) + diag(prior),   speed = v^T G v,   G = L L^T,   a = -G^-1 sum_k gam[k][n].
// One workgroup of one wave per point, the matrix in LDS, thread i owns row i of the right-looking factorisation (the lower
// triangle of G is read) and of the two substitutions.  A pivot that is not positive ends the point: info = its 1-based index,
// a = NaN; the other points never see it.  1 <= Q <= 64.
// The tangent operator (gat_kernel) takes the tangent mode's (dg, dgam) as well and solves a second time with the same factor:
//   da = -G^-1 (sum_k dgam[k][n] + (sum_k dg[k][n]) a);     a, speed and info carry ga_kernel's bits.
// The transport operator (gt_kernel) takes the transport mode's tgam [K][N][F][Q] as well and solves for 1 + F right-hand sides in
// ONE pair of substitutions on the same factor:
//   dw_r = -G^-1 sum_k tgam[k][n][r]:     the rate of a vector w_r in parallel transport along the geodesic;  a, speed, info: ga_kernel's bits.
// The integrators on the device (gs_kernel, dpgp_geodesic_shoot[_tangent]_f64): the same solve (ga_point, shared by all four
// kernels) as one launch per Runge-Kutta stage, which also applies the stage's share of the classical RK4 step to a per-curve
// state in the workspace; all C curves over all S steps from one C call, with the bits of the host loop of models/geodesic.py.
#include "point_tile.h"

#define GA_MAX_Q 64
#define GT_MAX_F 63                 // the transport operator's right-hand sides beside a's

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

// The solve of ga_kernel / gat_kernel for point n of N, shared with the stage kernels of the integrator below (TAN: the tangent's
// second solve as well).  Every thread of the workgroup calls it; smem: the kernel's dynamic LDS.  Returns 0, or the 1-based index
// of the failing pivot (uniform over the workgroup): nothing is solved then.  On success thread t < Q returns row t of a in res
// (and of da in dres).  speed (this point's entry, or nullptr: not formed) receives v^T G v; sv, LDS, keeps v_n for the caller.
__device__ __forceinline__ double gat_solve(const double *sA, double *sb, int Q, int LD, int t, bool row_live);
__device__ __forceinline__ void gt_solve(const double *sA, double *sb, double *sy, int Q, int LD, int NR, int t, bool row_live);

// TRN (gt_kernel): dgam is tgam [K][N][F][Q]; the 1 + F right-hand sides -sum_k gam, -sum_k tgam[.][r] are solved together and
// the solutions are left in LDS, [1 + F][Q] from smem + Q (Q + 1) doubles on: thread t < Q reads row t of each, which it wrote.
template <bool TAN, bool TRN = false>
__device__ __forceinline__ int ga_point(unsigned char *smem, int K, int N, int Q, int n, const double *__restrict__ g,
                                        const double *__restrict__ gam, const double *__restrict__ dg,
                                        const double *__restrict__ dgam, const double *__restrict__ prior,
                                        const double *__restrict__ vel, double *__restrict__ speed, double &res, double &dres,
                                        const double *&v_lds, int F = 0) {
    const int LD = Q + 1;
    double *sA = reinterpret_cast<double *>(smem);          // [Q][Q + 1]  G, then L in its lower triangle
    double *sb = sA + (size_t)Q * LD;                        // [Q]         the right-hand side, then y    (TRN: [1 + F][Q])
    double *sv = sb + (TRN ? (size_t)(1 + F) * Q : (size_t)Q);   // [Q]     v_n
    double *sr = sv + Q;                                     // [Q]         the rows' shares of v^T G v
    double *sy = sr + Q;                                     // [1 + F][Q]  the forward substitutions' results          (TRN only)
    double *sD = sr + Q;                                     // [Q][Q + 1]  sum_k dg                       (TAN only, as the next two)
    double *sc = sD + (size_t)Q * LD;                        // [Q]         sum_k dgam
    double *sa = sc + Q;                                     // [Q]         a_n
    const int t = threadIdx.x, qq = Q * Q;
    const bool row_live = t < Q;
    v_lds = sv;
    for (int e = t; e < qq; e += 64) {
        const double s = ga_slab_sum(g + (size_t)n * qq + e, K, (size_t)N * qq);
        const int r = e / Q, c = e % Q;
        sA[r * LD + c] = r == c ? s + prior[r] : s;
        if (TAN) sD[r * LD + c] = ga_slab_sum(dg + (size_t)n * qq + e, K, (size_t)N * qq);
    }
    if (row_live) {
        sb[t] = -ga_slab_sum(gam + (size_t)n * Q + t, K, (size_t)N * Q);
        sv[t] = vel[(size_t)n * Q + t];
        if (TAN) sc[t] = ga_slab_sum(dgam + (size_t)n * Q + t, K, (size_t)N * Q);
        if constexpr (TRN)
            for (int r = 0; r < F; ++r) sb[(1 + r) * Q + t] = -ga_slab_sum(dgam + ((size_t)n * F + r) * Q + t, K, (size_t)N * F * Q);
    }
    __syncthreads();
    if (speed) {                                              // (uniform)
        if (row_live) {
            double s = 0.0;
            for (int c = 0; c < Q; ++c) s = fma(sA[t * LD + c], sv[c], s);
            sr[t] = sv[t] * s;
        }
        __syncthreads();
        if (t == 0) {
            double s = 0.0;
            for (int r = 0; r < Q; ++r) s += sr[r];
            *speed = s;
        }
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
    if (fail) return fail;
    if constexpr (TRN) {
        gt_solve(sA, sb, sy, Q, LD, 1 + F, t, row_live);
        return 0;
    }
    res = gat_solve(sA, sb, Q, LD, t, row_live);
    if (TAN) {
        if (row_live) sa[t] = res;
        __syncthreads();
        if (row_live) {
            double s = sc[t];
            for (int c = 0; c < Q; ++c) s = fma(sD[t * LD + c], sa[c], s);
            sb[t] = -s;
        }
        dres = gat_solve(sA, sb, Q, LD, t, row_live);
    }
    return 0;
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

// gat_solve for NR right-hand sides sb [NR][Q] at once, each with gat_solve's statements on its own column (the same bits as NR
// calls), the barriers paid once: thread t owns row t of every right-hand side.  sy [NR][Q]: y, which gat_solve keeps in a
// register.  The solutions come back in sb; thread t wrote row t of each.
__device__ __forceinline__ void gt_solve(const double *sA, double *sb, double *sy, int Q, int LD, int NR, int t, bool row_live) {
    for (int j = 0; j < Q; ++j) {
        __syncthreads();
        const double ljj = sA[j * LD + j], ltj = t > j && row_live ? sA[t * LD + j] : 0.0;
        for (int r = 0; r < NR; ++r) {
            const double yj = sb[r * Q + j] / ljj;
            if (t == j) sy[r * Q + j] = yj;
            if (t > j && row_live) sb[r * Q + t] = fma(-ltj, yj, sb[r * Q + t]);
        }
    }
    for (int j = Q - 1; j >= 0; --j) {
        __syncthreads();
        const double ljj = sA[j * LD + j], ljt = t < j ? sA[j * LD + t] : 0.0;
        for (int r = 0; r < NR; ++r) {
            const double rj = sy[r * Q + j] / ljj;
            if (t == j) sb[r * Q + j] = rj;
            if (t < j) sy[r * Q + t] = fma(-ljt, rj, sy[r * Q + t]);
        }
    }
}

__global__ __launch_bounds__(64) void ga_kernel(int K, int N, int Q, const double *__restrict__ g, const double *__restrict__ gam,
                                                const double *__restrict__ prior, const double *__restrict__ vel,
                                                double *__restrict__ acc, double *__restrict__ speed, int *__restrict__ info) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int t = threadIdx.x, n = blockIdx.x;
    const bool row_live = t < Q;
    double res = 0.0, dres = 0.0;
    const double *sv;
    const int fail = ga_point<false>(smem_raw, K, N, Q, n, g, gam, nullptr, nullptr, prior, vel, speed + n, res, dres, sv);
    if (row_live) acc[(size_t)n * Q + t] = fail ? __builtin_nan("") : res;
    if (t == 0) info[n] = fail;
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
    const int t = threadIdx.x, n = blockIdx.x;
    const bool row_live = t < Q;
    double res = 0.0, dres = 0.0;
    const double *sv;
    const int fail = ga_point<true>(smem_raw, K, N, Q, n, g, gam, dg, dgam, prior, vel, speed + n, res, dres, sv);
    if (row_live) {
        acc[(size_t)n * Q + t] = fail ? __builtin_nan("") : res;
        dacc[(size_t)n * Q + t] = fail ? __builtin_nan("") : dres;
    }
    if (t == 0) info[n] = fail;
}

// ga_kernel's work, statement for statement (a, speed and info come out with its bits), with the F right-hand sides of the
// transport equation solved beside a's on the same factor (the prior is constant: it has no Christoffel symbols and enters G
// only).  A failing pivot ends the point: a = dw = NaN.
__global__ __launch_bounds__(64) void gt_kernel(int K, int N, int Q, int F, const double *__restrict__ g, const double *__restrict__ gam,
                                                const double *__restrict__ tgam, const double *__restrict__ prior,
                                                const double *__restrict__ vel, double *__restrict__ acc, double *__restrict__ dw,
                                                double *__restrict__ speed, int *__restrict__ info) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int t = threadIdx.x, n = blockIdx.x;
    const bool row_live = t < Q;
    double res = 0.0, dres = 0.0;
    const double *sv;
    const int fail = ga_point<false, true>(smem_raw, K, N, Q, n, g, gam, nullptr, tgam, prior, vel, speed + n, res, dres, sv, F);
    const double *sol = reinterpret_cast<const double *>(smem_raw) + (size_t)Q * (Q + 1);
    if (row_live) {
        acc[(size_t)n * Q + t] = fail ? __builtin_nan("") : sol[t];
        for (int r = 0; r < F; ++r) dw[((size_t)n * F + r) * Q + t] = fail ? __builtin_nan("") : sol[(1 + r) * Q + t];
    }
    if (t == 0) info[n] = fail;
}

// ---- the integrators on the device: one launch per Runge-Kutta stage ---------------------------------------------------------------
// What a stage of models/geodesic.exp_map (TAN: _rk4_tangent) does after its christoffel calls, for curve c = blockIdx.x of C:
// ga_point on the stage's slabs, then the stage's share of the classical RK4 step on a per-curve state in memory.  With the
// stage's velocity argument k_x (k_1x = v of the step's base) and k_v = a just solved, in the host integrator's order
//   stage 1, 2:  next x_arg = x + (h/2) k_x,  next v_arg = v + (h/2) k_v;      stage 3: the same with h
//   sums:        k_1, then + 2 k_2, + 2 k_3, + k_4   (left to right)
//   stage 4:     row s + 1 = base + (h/6) sums, which is also the next step's base and arguments
// every product rounded before its add (gs_mul: the library is built with contraction on).  The tangent's state
// (dx, dv) goes the same way with k_x = dv_arg, k_v = da.  The very first stage reads the caller's (x, v[, dx, dv]) and copies
// them to row 0.  A stage that fails to factor counts in bad[c] and leaves NaN in its curve alone, as the host loop does.
struct GsState {                 // one of the states x, v, dx, dv: thread t of curve c works on component t
    const double *start;         // [C][Q]       the caller's value: row 0
    double *rows;                // [C][S+1][Q]  curve / vel / dcurve / dvel
    const double *arg_in;        // [C][Q]       this stage's argument (read for v and dv only)
    double *arg_out;             // [C][Q]       the next stage's
    double *sum;                 // [C][Q]       the running sum of the step's k
};
struct GsStage {
    GsState x, v, dx, dv;
    const double *g, *gam, *dg, *dgam, *prior;
    int *bad;
    double *speed0;
    double c_arg, c_row;         // (h/2 or h), h/6: formed in double on the host
    int K, C, Q, S, step, stage;
};

// a * b rounded to double before anything is added to it.  Under -ffp-contract=fast the backend fuses a product with the add that
// follows whatever the source says (__dmul_rn / __dadd_rn are plain * and + to it, and `#pragma clang fp contract(off)` only
// governs the front end); a value that has passed through an (empty) asm statement is no product to it any more.
__device__ __forceinline__ double gs_mul(double a, double b) {
    double r = a * b;
    asm volatile("" : "+v"(r));
    return r;
}

// the share of one state (kk: its k of this stage) in the stage's epilogue
__device__ __forceinline__ void gs_advance(const GsState &st, const GsStage &p, size_t i, size_t row, bool first, double kk) {
    const double base = first ? st.start[i] : st.rows[row];
    if (first) st.rows[row] = base;
    const double sum = p.stage == 1 ? kk : p.stage == 4 ? st.sum[i] + kk : st.sum[i] + gs_mul(2.0, kk);
    if (p.stage < 4) {
        st.sum[i] = sum;
        st.arg_out[i] = base + gs_mul(p.c_arg, kk);
    } else {
        const double next = base + gs_mul(p.c_row, sum);
        st.rows[row + p.Q] = next;
        st.arg_out[i] = next;
    }
}

template <bool TAN> __global__ __launch_bounds__(64) void gs_kernel(GsStage p) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int t = threadIdx.x, c = blockIdx.x, Q = p.Q;
    const bool first = p.step == 0 && p.stage == 1;
    double a = 0.0, da = 0.0;
    const double *sv;
    const int fail = ga_point<TAN>(smem_raw, p.K, p.C, Q, c, p.g, p.gam, p.dg, p.dgam, p.prior, first ? p.v.start : p.v.arg_in,
                                   TAN && first ? p.speed0 + c : nullptr, a, da, sv);
    if (t == 0) p.bad[c] = (first ? 0 : p.bad[c]) + (fail != 0);
    if (t >= Q) return;
    if (fail) a = da = __builtin_nan("");
    const size_t i = (size_t)c * Q + t, row = ((size_t)c * (p.S + 1) + p.step) * Q + t;
    gs_advance(p.x, p, i, row, first, sv[t]);                // k_x = the stage's velocity argument
    gs_advance(p.v, p, i, row, first, a);
    if (TAN) {
        gs_advance(p.dx, p, i, row, first, (first ? p.dv.start : p.dv.arg_in)[i]);
        gs_advance(p.dv, p, i, row, first, da);
    }
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

extern "C" int dpgp_geodesic_transport_f64(int K, int N, int Q, int F, const double *g, const double *gam, const double *tgam,
                                           const double *prior, const double *v, double *a, double *dw, double *speed, int *info,
                                           void *stream) {
    if (K < 1 || K > DPGP_POINT_MAX_N) return -1;
    if (N < 1 || N > DPGP_POINT_MAX_N) return -2;
    if (Q < 1 || Q > GA_MAX_Q) return -3;
    if (F < 1 || F > GT_MAX_F) return -4;
    if (!g) return -5;
    if (!gam) return -6;
    if (!tgam) return -7;
    if (!prior) return -8;
    if (!v) return -9;
    if (!a) return -10;
    if (!dw) return -11;
    if (!speed) return -12;
    if (!info) return -13;
    const size_t lds = sizeof(double) * ((size_t)Q * (Q + 1) + 2 * (size_t)(1 + F) * Q + 2 * Q);       // 97.5 KiB at Q = 64, F = 63
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(gt_kernel), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(gt_kernel, dim3((unsigned)N), dim3(64), lds, (hipStream_t)stream, K, N, Q, F, g, gam, tgam, prior, v, a, dw,
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

// ---- the shooting calls: all C curves over all S steps from one call ---------------------------------------------------------------
#define GS_MAX_PARTS 64

namespace {

// The workspace: a token for the christoffel operator, the two argument buffers that the stages alternate between, the running
// sums, and ONE slab array per result of the christoffel operator, [sum_i K_i][C][..], the parts' slices in part order.
struct GsPlan {
    size_t token, args, sums, g, gam, dg, dgam, bytes;        // byte offsets; args: [2][states][C][Q], sums: [states][C][Q]
    long ktot;
};

// false for a shape out of range; parts, K, M, Q, C are taken as checked by the caller (non-null, parts in range)
bool gs_plan(int parts, const int *K, const int *M, int Q, int C, int tangent, GsPlan &pl) {
    if (Q < 1 || Q > (tangent ? 31 : 63) || C < 1 || C > DPGP_POINT_MAX_N) return false;
    long ktot = 0;
    for (int i = 0; i < parts; ++i) {
        if (K[i] < 1 || M[i] < 1) return false;
        const size_t ok = tangent ? dpgp_ard_rbf_point_christoffel_tangent_workspace_bytes(K[i], C, M[i], Q)
                                  : dpgp_ard_rbf_point_christoffel_workspace_bytes(K[i], C, M[i], Q);
        if (ok == 0 || ok > DPGP_POINT_WS) return false;
        ktot += K[i];
    }
    if (ktot > DPGP_POINT_MAX_N) return false;
    const size_t states = tangent ? 4 : 2, cq = sizeof(double) * (size_t)C * Q;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += dpgp_align256(bytes); return at; };
    pl.ktot = ktot;
    pl.token = take(DPGP_POINT_WS);
    pl.args = take(2 * states * cq);
    pl.sums = take(states * cq);
    pl.g = take((size_t)ktot * cq * Q);
    pl.gam = take((size_t)ktot * cq);
    pl.dg = tangent ? take((size_t)ktot * cq * Q) : 0;
    pl.dgam = tangent ? take((size_t)ktot * cq) : 0;
    pl.bytes = off;
    return true;
}

struct GsParts { int parts; const int *K, *M; const double *const *z, *const *gamma, *const *alpha, *const *p; };

// the checks that the two entry points share, codes from -1 down; 0: all well
int gs_check_parts(const GsParts &a, int Q, int C, int S, int max_q) {
    if (a.parts < 1 || a.parts > GS_MAX_PARTS) return -1;
    if (!a.K) return -2;
    for (int i = 0; i < a.parts; ++i)
        if (a.K[i] < 1 || a.K[i] > DPGP_POINT_MAX_N) return -2;
    if (!a.M) return -3;
    for (int i = 0; i < a.parts; ++i)
        if (a.M[i] < 1 || a.M[i] > DPGP_POINT_MAX_N) return -3;
    if (Q < 1 || Q > max_q) return -4;
    if (C < 1 || C > DPGP_POINT_MAX_N) return -5;
    if (S < 1 || S > DPGP_POINT_MAX_N) return -6;
    const double *const *lists[4] = {a.z, a.gamma, a.alpha, a.p};
    for (int l = 0; l < 4; ++l) {
        if (!lists[l]) return -7 - l;
        for (int i = 0; i < a.parts; ++i)
            if (!lists[l][i]) return -7 - l;
    }
    return 0;
}

// 4 S (parts + 1) launches in order on st: per stage the christoffel operator of every part into its slice of the slabs, then
// the stage kernel.  io: the states x, v[, dx, dv] with start and rows set.
template <bool TAN>
int gs_run(const GsParts &a, int Q, int C, int S, const double *prior, GsState *io, int *bad, double *speed0, unsigned char *ws,
           const GsPlan &pl, hipStream_t st) {
    constexpr int STATES = TAN ? 4 : 2;
    const size_t cq = (size_t)C * Q;
    double *args = reinterpret_cast<double *>(ws + pl.args), *sums = reinterpret_cast<double *>(ws + pl.sums);
    double *g = reinterpret_cast<double *>(ws + pl.g), *gam = reinterpret_cast<double *>(ws + pl.gam);
    double *dg = TAN ? reinterpret_cast<double *>(ws + pl.dg) : nullptr, *dgam = TAN ? reinterpret_cast<double *>(ws + pl.dgam) : nullptr;
    const double h = 1.0 / S, c_half = 0.5 * h, c_row = h / 6.0;
    const size_t lds = sizeof(double) * ((TAN ? 2 : 1) * (size_t)Q * (Q + 1) + (TAN ? 5 : 3) * Q);      // 33.0 KiB at Q = 63; 16.7 at 31
    GsStage p{};
    p.g = g, p.gam = gam, p.dg = dg, p.dgam = dgam, p.prior = prior, p.bad = bad, p.speed0 = speed0;
    p.c_row = c_row, p.K = (int)pl.ktot, p.C = C, p.Q = Q, p.S = S;
    GsState *states[4] = {&p.x, &p.v, &p.dx, &p.dv};
    for (int j = 0; j < STATES; ++j) {
        *states[j] = io[j];
        states[j]->sum = sums + j * cq;
    }
    for (int launch = 0; launch < 4 * S; ++launch) {
        p.step = launch / 4, p.stage = launch % 4 + 1;
        p.c_arg = p.stage == 3 ? h : c_half;
        const double *in[4];
        for (int j = 0; j < STATES; ++j) {
            in[j] = launch == 0 ? io[j].start : args + ((size_t)((launch - 1) & 1) * STATES + j) * cq;
            states[j]->arg_in = in[j];
            states[j]->arg_out = args + ((size_t)(launch & 1) * STATES + j) * cq;
        }
        size_t koff = 0;
        for (int i = 0; i < a.parts; ++i) {
            const int rc = TAN ? dpgp_ard_rbf_point_christoffel_tangent_f64(a.K[i], C, a.M[i], Q, a.z[i], in[0], in[1], in[2], in[3],
                                                                            a.gamma[i], a.alpha[i], a.p[i], g + koff * cq * Q,
                                                                            gam + koff * cq, dg + koff * cq * Q, dgam + koff * cq,
                                                                            ws + pl.token, DPGP_POINT_WS, st)
                               : dpgp_ard_rbf_point_christoffel_f64(a.K[i], C, a.M[i], Q, a.z[i], in[0], in[1], a.gamma[i], a.alpha[i],
                                                                    a.p[i], g + koff * cq * Q, gam + koff * cq, ws + pl.token,
                                                                    DPGP_POINT_WS, st);
            if (rc != DPGP_OK) return DPGP_ERR_LAUNCH;
            koff += a.K[i];
        }
        DPGP_PRELAUNCH();
        hipLaunchKernelGGL(gs_kernel<TAN>, dim3((unsigned)C), dim3(64), lds, st, p);
        DPGP_LAUNCH_CHECK();
    }
    return DPGP_OK;
}

}  // namespace

extern "C" size_t dpgp_geodesic_shoot_workspace_bytes(int parts, const int *K, const int *M, int Q, int C, int tangent) {
    GsPlan pl;
    if (parts < 1 || parts > GS_MAX_PARTS || !K || !M) return 0;
    return gs_plan(parts, K, M, Q, C, tangent != 0, pl) ? pl.bytes : 0;
}

extern "C" int dpgp_geodesic_shoot_f64(int parts, const int *K, const int *M, int Q, int C, int S, const double *const *z,
                                       const double *const *gamma, const double *const *alpha, const double *const *p,
                                       const double *prior, const double *x, const double *v, double *curve, double *vel, int *bad,
                                       void *ws, size_t ws_bytes, void *stream) {
    const GsParts a{parts, K, M, z, gamma, alpha, p};
    if (const int rc = gs_check_parts(a, Q, C, S, 63)) return rc;
    if (!prior) return -11;
    if (!x) return -12;
    if (!v) return -13;
    if (!curve) return -14;
    if (!vel) return -15;
    if (!bad) return -16;
    if (!ws) return -17;
    GsPlan pl;
    if (!gs_plan(parts, K, M, Q, C, 0, pl) || ws_bytes < pl.bytes) return -18;      // (no plan: a shape past what a launch grid holds)
    GsState io[2] = {{x, curve, nullptr, nullptr, nullptr}, {v, vel, nullptr, nullptr, nullptr}};
    return gs_run<false>(a, Q, C, S, prior, io, bad, nullptr, static_cast<unsigned char *>(ws), pl, (hipStream_t)stream);
}

extern "C" int dpgp_geodesic_shoot_tangent_f64(int parts, const int *K, const int *M, int Q, int C, int S, const double *const *z,
                                               const double *const *gamma, const double *const *alpha, const double *const *p,
                                               const double *prior, const double *x, const double *v, const double *dx,
                                               const double *dv, double *curve, double *vel, double *dcurve, double *dvel, int *bad,
                                               double *speed0, void *ws, size_t ws_bytes, void *stream) {
    const GsParts a{parts, K, M, z, gamma, alpha, p};
    if (const int rc = gs_check_parts(a, Q, C, S, 31)) return rc;
    if (!prior) return -11;
    if (!x) return -12;
    if (!v) return -13;
    if (!dx) return -14;
    if (!dv) return -15;
    if (!curve) return -16;
    if (!vel) return -17;
    if (!dcurve) return -18;
    if (!dvel) return -19;
    if (!bad) return -20;
    if (!speed0) return -21;
    if (!ws) return -22;
    GsPlan pl;
    if (!gs_plan(parts, K, M, Q, C, 1, pl) || ws_bytes < pl.bytes) return -23;
    GsState io[4] = {{x, curve, nullptr, nullptr, nullptr}, {v, vel, nullptr, nullptr, nullptr},
                     {dx, dcurve, nullptr, nullptr, nullptr}, {dv, dvel, nullptr, nullptr, nullptr}};
    return gs_run<true>(a, Q, C, S, prior, io, bad, speed0, static_cast<unsigned char *>(ws), pl, (hipStream_t)stream);
}
