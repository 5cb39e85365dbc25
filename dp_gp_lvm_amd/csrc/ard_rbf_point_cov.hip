// Joint posterior covariance of K ARD-RBF kernels with G training patterns each at DETERMINISTIC latent points x [N][Q].  With
//   k_km(x) = alpha_k exp(-1/2 sum_q gamma_kq (x_q - z_kmq)^2)
// the operator gives
//   out[k][g][i][j] = alpha_k exp(-1/2 sum_q gamma_kq (x_iq - x_jq)^2) - sum_{m,m'} k_km(x_i) ct[k][g][m][m'] k_km'(x_j)
// with ct = (c + c^T) / 2 the symmetric part of c [K][G][M][M] (any matrices).  The features k [N x M] are never stored to memory.
//
// Layout.  Workgroup (kernel k, tile I of 32 points, tile J <= I of 32 points), 256 threads = 4 waves; the 64 columns of every
// matrix step are the points of I (columns 0 .. 31) and of J (32 .. 63).  The inducing points go in blocks of 64; the workgroup
// walks the block pairs (rs, mc) in row-major order and, inside a pair, the patterns g:
//   sFr [64][FS]  features of block rs at the 64 points, made once per rs;   sFc: the same of block mc, made once per (rs, mc),
//                 mc != rs (mc == rs reads sFr).  The patterns share them: the number of exponentials does not depend on G.
//   sP  [64][PS]  the tile (c + c^T)[rs][mc] of pattern g: c^T's tile is read along ITS contiguous index and written transposed,
//                 then c's tile is added along its own (both global reads coalesce; a + b = b + a, so the tile (mc, rs) holds the
//                 transposed bits).
//   first product   U [64 x 64] = sP sFc on v_mfma_f64_16x16x4 (wave w owns rows 16 w .. 16 w + 15, four column tiles), to sU.
//   second product  wave w owns the 16 x 16 block (ti, tj) = (w >> 1, w & 1) of the pair's 32 x 32 results and forms BOTH
//                     q1[i][j] = sum_m sFr[m][i] sU[m][32 + j]        (features of i, U of j)
//                     q2[i][j] = sum_m sU[m][i]  sFr[m][32 + j]       (U of i, features of j)
//                   over the 64 rows m in ascending order.  Mathematically q1 = q2; their roundings differ, and the entry takes
//                   q1 + q2: a sum that does not change when i and j trade places.  So the bits of entry (i, j) do not depend
//                   on which of the two points comes first in x, nor on N, nor on the points' places in their tiles (a point is
//                   one column / one row of every matrix step).
//   The thread that holds entry (i, j) keeps its running value in out itself: the prior term at the first block pair, then
//   value -= (q1 + q2) / 4 per block pair, read and written by the same thread in the fixed order of the pairs; at the last
//   pair it also stores the value to (j, i).  Only tile pairs J <= I exist, and in a diagonal tile only entries i >= j are
//   touched: an entry with i > j is computed once and stored to both places, the result is exactly symmetric.
// No atomics, no workspace, nothing of size N M in memory; the order of every sum is fixed by (M, Q): the same bits on every
// run, a kernel's results do not depend on K, G or the other kernels and patterns.  Far-away points: dpgp_exp2 gives k = 0
// exactly, U and both products are exact zeros and the prior term stands alone.  c is streamed in 64 x 64 tiles and the features
// in blocks of 64: no limit on M from the LDS.
// LDS: 8 (3 64 FS + 64 PS + Q) = 156672 + 8 Q bytes (one workgroup per CU).  FS = 80: the two rows (kk, kk + 1) that a half
// wave reads for an A or B operand lie 80 doubles = 160 banks apart, i.e. on disjoint halves of the 64 banks; PS = 66 as
// the sibling operators' tile of p (lanes (i, kk) of a half wave on 32 distinct bank pairs).
#include "point_tile.h"

#define PC_MS DPGP_POINT_MS // inducing points per block
#define PC_PS DPGP_POINT_PS // row stride of the c tile
#define PC_FS 80            // row stride of the feature and U arrays
#define PC_NP 32            // points per tile
#define PC_MAX_N 46340      // N N fits 31 bits

namespace {

__global__ __launch_bounds__(256) void pc_kernel(int G, int N, int M, int Q, int npairs, const double *__restrict__ z,
                                                 const double *__restrict__ x, const double *__restrict__ gamma,
                                                 const double *__restrict__ alpha, const double *__restrict__ c,
                                                 double *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *sFr = reinterpret_cast<double *>(smem_raw);     // [64][FS]  features of block rs, 0 past M or N
    double *sFc = sFr + PC_MS * PC_FS;                       // [64][FS]  features of block mc != rs
    double *sU = sFc + PC_MS * PC_FS;                        // [64][FS]  U = (c + c^T) tile x features of block mc
    double *sP = sU + PC_MS * PC_FS;                         // [64][PS]  (c + c^T) tile, 0 out of range
    double *sg = sP + PC_MS * PC_PS;                         // [Q]       -1/2 log2(e) gamma_k
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 15, kk = lane >> 4;
    const int pair = blockIdx.x % npairs, k = blockIdx.x / npairs;
    int I = (int)((sqrt(8.0 * pair + 1.0) - 1.0) * 0.5);
    while (I * (I + 1) / 2 > pair) --I;
    while ((I + 1) * (I + 2) / 2 <= pair) ++I;
    const int J = pair - I * (I + 1) / 2;                    // J <= I
    const double *zk = z + (size_t)k * M * Q, *gk = gamma + (size_t)k * Q;
    const double al = alpha[k];
    for (int q = t; q < Q; q += 256) sg[q] = -0.5 * DPGP_LOG2E * gk[q];
    __syncthreads();

    // the thread's four entries: rows 16 ti + kk + 4 r, column 16 tj + li of the pair's 32 x 32 block
    const int ti = wave >> 1, tj = wave & 1;
    const bool wave_live = I != J || ti >= tj;               // (wave-uniform: a diagonal tile's upper block is never stored)
    const int gj = J * PC_NP + 16 * tj + li;
    double val[4];
    bool mine[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int gi = I * PC_NP + 16 * ti + Mfma<double>::row(lane, r);
        mine[r] = gi < N && gj < N && gi >= gj;
        double ex = 0.0;
        if (mine[r])
            for (int q = 0; q < Q; ++q) {
                const double d = x[(size_t)gi * Q + q] - x[(size_t)gj * Q + q];
                ex = fma(sg[q] * d, d, ex);
            }
        val[r] = mine[r] ? al * dpgp_exp2(ex) : 0.0;
    }

    auto features = [&](double *sF, int m0) {
        for (int e = t; e < PC_MS * 64; e += 256) {
            const int rr = e >> 6, col = e & 63, m = m0 + rr;
            const int n = (col < PC_NP ? I * PC_NP : J * PC_NP - PC_NP) + col;
            double v = 0.0;
            if (m < M && n < N) {
                const double *xn = x + (size_t)n * Q, *zm = zk + (size_t)m * Q;
                double ex = 0.0;
                for (int q = 0; q < Q; ++q) {
                    const double d = xn[q] - zm[q];
                    ex = fma(sg[q] * d, d, ex);
                }
                v = al * dpgp_exp2(ex);
            }
            sF[rr * PC_FS + col] = v;
        }
    };

    const int nch = (M + PC_MS - 1) / PC_MS;
    const int tl = t & 63, th = t >> 6;
    for (int rs = 0; rs < nch; ++rs) {
        const int r0 = rs * PC_MS;
        __syncthreads();                                       // the previous block pair's second product is done with sFr
        features(sFr, r0);
        for (int mc = 0; mc < nch; ++mc) {
            const int c0 = mc * PC_MS;
            const double *sF = mc == rs ? sFr : sFc;
            if (mc != rs) features(sFc, c0);                   // (its last reader, a first product, lies before a barrier)
            const bool first = rs == 0 && mc == 0, last = rs == nch - 1 && mc == nch - 1;
            for (int g = 0; g < G; ++g) {
                const double *cg = c + ((size_t)k * G + g) * M * M;
                double pa[16], pb[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int a = th + 4 * i, rowa = r0 + tl, cola = c0 + a, rowb = r0 + a, colb = c0 + tl;
                    const double ga = cg[(size_t)min(cola, M - 1) * M + min(rowa, M - 1)];
                    const double gb = cg[(size_t)min(rowb, M - 1) * M + min(colb, M - 1)];
                    pa[i] = rowa < M && cola < M ? ga : 0.0;
                    pb[i] = rowb < M && colb < M ? gb : 0.0;
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) sP[tl * PC_PS + th + 4 * i] = pa[i];      // c[m'][m], read along m, written transposed
                __syncthreads();                               // (also: the features are staged)
#pragma unroll
                for (int i = 0; i < 16; ++i) sP[(th + 4 * i) * PC_PS + tl] += pb[i];   // + c[m][m'], read along m'
                __syncthreads();
                {
                    f64x4 acc[4];
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
                    const double *prow = sP + (16 * wave + li) * PC_PS + kk;
                    const double *brow = sF + kk * PC_FS + li;
#pragma unroll 4
                    for (int st = 0; st < PC_MS / 4; ++st) {
                        const double av = prow[4 * st];
#pragma unroll
                        for (int ct = 0; ct < 4; ++ct) acc[ct] = Mfma<double>::mma(av, brow[4 * st * PC_FS + 16 * ct], acc[ct]);
                    }
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                        for (int r = 0; r < 4; ++r) sU[(16 * wave + Mfma<double>::row(lane, r)) * PC_FS + 16 * ct + li] = acc[ct][r];
                }
                __syncthreads();
                if (wave_live) {
                    f64x4 q1 = f64x4{0.0, 0.0, 0.0, 0.0}, q2 = f64x4{0.0, 0.0, 0.0, 0.0};
                    const double *fa = sFr + kk * PC_FS + 16 * ti + li, *ub = sU + kk * PC_FS + PC_NP + 16 * tj + li;
                    const double *ua = sU + kk * PC_FS + 16 * ti + li, *fb = sFr + kk * PC_FS + PC_NP + 16 * tj + li;
#pragma unroll 4
                    for (int st = 0; st < PC_MS / 4; ++st) {
                        q1 = Mfma<double>::mma(fa[4 * st * PC_FS], ub[4 * st * PC_FS], q1);
                        q2 = Mfma<double>::mma(ua[4 * st * PC_FS], fb[4 * st * PC_FS], q2);
                    }
                    double *og = out + ((size_t)k * G + g) * N * N;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (!mine[r]) continue;
                        const int gi = I * PC_NP + 16 * ti + Mfma<double>::row(lane, r);
                        const size_t at = (size_t)gi * N + gj;
                        const double v = (first ? val[r] : og[at]) - 0.25 * (q1[r] + q2[r]);
                        og[at] = v;
                        if (last && gi != gj) og[(size_t)gj * N + gi] = v;
                    }
                }
                // the next pattern's first barrier lies between this second product and the next write of sU; sP's last reader
                // (the first product) lies before the barrier above
            }
        }
    }
}

size_t pc_lds(int Q) { return sizeof(double) * ((size_t)3 * PC_MS * PC_FS + PC_MS * PC_PS + Q); }

long pc_pairs(int N) {
    const long T = dpgp_ceil_div(N, PC_NP);
    return T * (T + 1) / 2;
}

// K, G, N, M >= 1, 1 <= Q <= 64, N N within 31 bits, and sizes that the 32-bit grid and the int indices of the kernel hold
bool pc_shape_ok(int K, int G, int N, int M, int Q) {
    if (K < 1 || G < 1 || N < 1 || M < 1 || Q < 1 || Q > DPGP_QX_PSI_MAX_Q) return false;
    if (N > PC_MAX_N || M > DPGP_POINT_MAX_N) return false;
    return (long)K * pc_pairs(N) <= 0x7fffffffL;
}

}  // namespace

extern "C" size_t dpgp_ard_rbf_point_cov_workspace_bytes(int K, int G, int N, int M, int Q) {
    return pc_shape_ok(K, G, N, M, Q) ? DPGP_POINT_WS : 0;
}

extern "C" int dpgp_ard_rbf_point_cov_f64(int K, int G, int N, int M, int Q, const double *z, const double *x,
                                          const double *gamma, const double *alpha, const double *c, double *out, void *ws,
                                          size_t ws_bytes, void *stream) {
    if (K < 1) return -1;
    if (G < 1) return -2;
    if (N < 1 || N > PC_MAX_N) return -3;
    if (M < 1) return -4;
    if (Q < 1 || Q > DPGP_QX_PSI_MAX_Q) return -5;
    if (!z) return -6;
    if (!x) return -7;
    if (!gamma) return -8;
    if (!alpha) return -9;
    if (!c) return -10;
    if (!out) return -11;
    if (!ws) return -12;
    const size_t need = dpgp_ard_rbf_point_cov_workspace_bytes(K, G, N, M, Q);
    if (need == 0 || ws_bytes < need) return -13;              // (need == 0: a shape past what the launch grid holds)
    const long npairs = pc_pairs(N);
    const size_t lds = pc_lds(Q);
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(pc_kernel), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(pc_kernel, dim3((unsigned)((long)K * npairs)), dim3(256), lds, (hipStream_t)stream, G, N, M, Q, (int)npairs,
                       z, x, gamma, alpha, c, out);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}
