// Device helpers shared by the q(X) Psi operators that walk the pairs (m, m') of inducing points by 32 x 32 tiles of the upper
// block triangle: qx_psi.hip, qx_psi_point.hip, qx_psi_point_adjoint.hip, psi_latent_adjoint.hip.
#pragma once
#include "common.h"

// tile index -> (I, J), I <= J, row-major over the upper block triangle of T x T tiles
__device__ __forceinline__ void dpgp_tile_ij(int idx, int T, int &I, int &J) {
    int i = 0;
    while (idx >= T - i) { idx -= T - i; ++i; }
    I = i;
    J = i + idx;
}

// pair factor F[m][m'] = alpha^2 exp(-1/4 sum_q gamma_q (z_mq - z_m'q)^2) of one kernel: read from zf [M][M] when given
__device__ __forceinline__ double dpgp_pair_factor(const double *zf, int M, int Q, int m, int mp, const double *z, const double *gm,
                                                   double al) {
    if (zf) return zf[(size_t)m * M + mp];
    double d2 = 0.0;
    for (int q = 0; q < Q; ++q) {
        const double d = z[(size_t)m * Q + q] - z[(size_t)mp * Q + q];
        d2 = fma(gm[q] * d, d, d2);
    }
    return al * al * exp(-0.25 * d2);
}

// ---- the pieces that the per-point adjoint kernels share (pl_kernel of psi_latent_adjoint.hip, pa_kernel of
// qx_psi_point_adjoint.hip): a workgroup of 4 waves x 16 points, lane = (point pi, kk = lane >> 4), LDS arrays [Q][NP]

// the prefactor of point n for one kernel and phase: lead prod_q (k2 gamma_q s_nq + 1)^-1/2, 0 past N
__device__ __forceinline__ double dpgp_point_prefactor(int n, int N, int Q, const double *gk, const double *s, double k2, double lead) {
    if (n >= N) return 0.0;
    const double *sn = s + (size_t)n * Q;
    double l = 0.0;
    for (int q = 0; q < Q; ++q) l += log(fma(k2 * gk[q], sn[q], 1.0));
    return lead * exp(-0.5 * l);
}

// Q <= QR: the exponent kexp sum_q g_q (mu_q - z_q)^2 of the lane's point as  e0 + sum_q z_q (pw_q z_q + pl_q), the point's
// coefficients in registers: two FMAs per q and evaluation
template <int QR> struct DpgpPointExponent {
    double pl[QR], pw[QR], e0;
    __device__ __forceinline__ void setup(int Q, double kexp, const double *smu, const double *sg, int NP, int pi) {
        e0 = 0.0;
#pragma unroll
        for (int q = 0; q < QR; ++q) {
            const double mq = q < Q ? smu[q * NP + pi] : 0.0;
            pw[q] = q < Q ? kexp * sg[q * NP + pi] : 0.0;
            pl[q] = -2.0 * pw[q] * mq;
            e0 = fma(pw[q] * mq, mq, e0);
        }
    }
    __device__ __forceinline__ double at(int Q, const double *zq) const {
        double e = e0;
#pragma unroll
        for (int q = 0; q < QR; ++q)
            if (q < Q) e = fma(zq[q], fma(pw[q], zq[q], pl[q]), e);
        return e;
    }
};

// the wave's first nct moment tiles -> rows wave 16 .. wave 16 + 15 of sM [NP][MS]
template <int CT>
__device__ __forceinline__ void dpgp_spill_moment_tiles(const f64x4 (&acc)[CT], int nct, double *sM, int MS, int wave, int lane) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
        if (ct < nct) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) sM[(wave * 16 + Mfma<double>::row(lane, rr)) * MS + 16 * ct + (lane & 15)] = acc[ct][rr];
        }
}

// the lane's accumulators (latent dims kk + 4 j) of point n -> pb [2][N][Q] = (d_mu, d_s) of one slab
template <int NQ>
__device__ __forceinline__ void dpgp_write_point_partials(double *pb, int n, int N, int Q, int kk, const double (&dmu)[NQ],
                                                          const double (&dsv)[NQ]) {
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int q = kk + 4 * j;
        if (q < Q) {
            pb[(size_t)n * Q + q] = dmu[j];
            pb[((size_t)N + n) * Q + q] = dsv[j];
        }
    }
}
