// ARD-RBF gram gradient contraction (the one new operator of gp_regression / gp_lvm's backward pass), for B kernels with their
// own x_b [N][Q], gamma_b, alpha_b and w_b (w_stride doubles apart) in ONE launch pair; the single operator is the case B = 1:
//   G_ij = w_ij alpha exp(-1/2 sum_q gamma_q d_ijq^2),  d_ijq = x_iq - x_jq   (noise-free gram, diagonal e_ii = 1)
//   r[i] = sum_j G_ij,   sx[i,q] = sum_j G_ij d_ijq,   sq[i,q] = sum_j G_ij d_ijq^2
// for any (not necessarily symmetric) w of leading dimension ldw.
//
// Layout: workgroup (kernel b, slab s; row tile) = 64 rows i x the j of slab s, in chunks of 64 j; the batch is part of the grid
// (blockIdx.x = b * slabs + slab).  The slab plan aims at 512 workgroups: slabs = ceil(512 / (row tiles * B)) clipped to the
// chunk count, so B small grams (N = M inducing points) get one slab each and a workspace of B (1 + 2Q) N doubles.
// The row strip x_b[i0:i0+64, :] is staged in LDS once, the column strip of each chunk per chunk, both transposed [Q][64] as
// gram_tile does; differences are taken directly in fp64 (no |x|^2 - 2 x^T x expansion, which cancels for points far from
// the origin).
//   phase 1: 256 threads = 8 rows x 32 column pairs per pass, 8 passes; w is read once, 16 bytes per lane (contiguous
//            along j within a row); the 64 x 64 G tile goes to LDS.
//   phase 2: thread = (row i = t & 63, latent dims q = wave, wave + 4, ...): the three sums over the chunk's j, the column
//            strip read as an LDS broadcast (the wave's lanes share q and j).  d_ijq is formed again here (one subtraction):
//            keeping phase 1's d in registers would need Q registers per element.
// Each workgroup writes its (1 + 2Q) x 64 partial sums to slab (b, s) of the workspace; a second launch adds kernel b's slabs
// in slab order.  No atomics: the same inputs give the same bits.
#include "internal.h"

#define GG_ROWS 64
#define GG_COLS 64
#define GG_GSTRIDE (GG_COLS + 1)
#define GG_TARGET_WGS 512

namespace {

struct GgPlan {
    int row_tiles, slabs, chunks_per_slab;
};

size_t gg_lds_bytes(int Q) { return sizeof(double) * ((size_t)2 * Q * GG_ROWS + (size_t)GG_ROWS * GG_GSTRIDE + DPGP_GRAM_GRAD_MAX_Q); }

// slabs = ceil(512 / (row tiles * B)), clipped to [1, chunks]
GgPlan gg_plan_batched(int B, int N) {
    GgPlan p;
    p.row_tiles = dpgp_ceil_div(N, GG_ROWS);
    const int chunks = dpgp_ceil_div(N, GG_COLS);
    const long long wgs = (long long)p.row_tiles * B;
    int s = wgs >= GG_TARGET_WGS ? 1 : (int)((GG_TARGET_WGS + wgs - 1) / wgs);
    s = s > chunks ? chunks : s;
    p.chunks_per_slab = dpgp_ceil_div(chunks, s);
    p.slabs = dpgp_ceil_div(chunks, p.chunks_per_slab);
    return p;
}

// KQ = ceil(Q / 4) rounded up to a power of two: the per-thread accumulators stay in registers
template <int KQ>
__global__ __launch_bounds__(256) void gram_grad_batched_kernel(int N, int Q, int slabs, int chunks_per_slab,
                                                                const double *__restrict__ x, const double *__restrict__ gamma,
                                                                const double *__restrict__ alpha, const double *__restrict__ w,
                                                                int ldw, long long w_stride, double *__restrict__ part) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    double *xi = reinterpret_cast<double *>(smem_raw);        // [Q][64] rows of the tile
    double *xj = xi + (size_t)Q * GG_ROWS;                     // [Q][64] columns of the chunk
    double *gs = xj + (size_t)Q * GG_COLS;                     // [64][65] G of the chunk
    double *gm = gs + GG_ROWS * GG_GSTRIDE;                    // [Q] gamma
    const int t = threadIdx.x;
    const int b = blockIdx.x / slabs, slab = blockIdx.x - b * slabs;
    const int i0 = blockIdx.y * GG_ROWS;
    const int c = t & 63;
    // kernel b's rows of x are reached through one 32-bit row offset (B N < 2^31 is part of the range check) and the vector
    // load of w is decided by one integer: with these the batch costs the kernel no scalar registers over a single-gram form
    const int bn = b * N;
    for (int q = t >> 6; q < Q; q += 4) xi[q * GG_ROWS + c] = i0 + c < N ? x[(size_t)(bn + i0 + c) * Q + q] : 0.0;
    for (int q = t; q < Q; q += 256) gm[q] = gamma[(size_t)b * Q + q];
    const double al = alpha[b];

    // phase-2 role: row il, latent dims q = qg + 4 k
    const int il = t & 63, qg = t >> 6;
    double acc_r = 0.0, acc_x[KQ], acc_q[KQ], xr[KQ];
#pragma unroll
    for (int k = 0; k < KQ; ++k) acc_x[k] = acc_q[k] = xr[k] = 0.0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KQ; ++k)
        if (qg + 4 * k < Q) xr[k] = xi[(qg + 4 * k) * GG_ROWS + il];

    // phase-1 role: column pair jp, rows rp + 8 p
    const int jp = (t & 31) * 2, rp = t >> 5;
    w += (size_t)b * w_stride;
    // 16-byte loads of kernel b's own w where ldw and its address allow them: for columns ja + 1 < nv
    const int nv = ((ldw & 1) == 0) && ((reinterpret_cast<uintptr_t>(w) & 15) == 0) ? N : 0;
    const int chunk0 = slab * chunks_per_slab;
    for (int ch = chunk0; ch < chunk0 + chunks_per_slab; ++ch) {
        const int j0 = ch * GG_COLS;
        if (j0 >= N) break;                                        // (uniform over the workgroup)
        __syncthreads();                                           // the previous chunk's phase 2 is done with xj / gs
        for (int q = t >> 6; q < Q; q += 4) xj[q * GG_COLS + c] = j0 + c < N ? x[(size_t)(bn + j0 + c) * Q + q] : 0.0;
        __syncthreads();
        const int ja = j0 + jp;
        for (int p = 0; p < GG_ROWS / 8; ++p) {
            const int r = rp + 8 * p, i = i0 + r;
            double w0 = 0.0, w1 = 0.0;
            if (i < N) {
                const double *wr = w + (size_t)i * ldw + ja;
                if (ja + 1 < nv) {
                    const double2 v = *reinterpret_cast<const double2 *>(wr);
                    w0 = v.x; w1 = v.y;
                } else {
                    if (ja < N) w0 = wr[0];
                    if (ja + 1 < N) w1 = wr[1];
                }
            }
            double e0 = 0.0, e1 = 0.0;
            for (int q = 0; q < Q; ++q) {
                const double a = xi[q * GG_ROWS + r], g = gm[q];
                const double d0 = a - xj[q * GG_COLS + jp], d1 = a - xj[q * GG_COLS + jp + 1];
                e0 = fma(g * d0, d0, e0);
                e1 = fma(g * d1, d1, e1);
            }
            // (w is 0 outside the matrix, so the padded rows / columns add nothing)
            gs[r * GG_GSTRIDE + jp] = w0 * (al * exp(-0.5 * e0));
            gs[r * GG_GSTRIDE + jp + 1] = w1 * (al * exp(-0.5 * e1));
        }
        __syncthreads();
        const int nj = N - j0 < GG_COLS ? N - j0 : GG_COLS;
        for (int jj = 0; jj < nj; ++jj) {
            const double g = gs[il * GG_GSTRIDE + jj];
            acc_r += g;
#pragma unroll
            for (int k = 0; k < KQ; ++k) {
                const int q = qg + 4 * k;
                if (q < Q) {
                    const double d = xr[k] - xj[q * GG_COLS + jj];
                    const double gd = g * d;
                    acc_x[k] += gd;
                    acc_q[k] = fma(gd, d, acc_q[k]);
                }
            }
        }
    }
    // partial sums of (b, slab): part[((b * slabs + slab) * (1 + 2Q) + k) * N + i], k = 0 (r), 1 + q (sx), 1 + Q + q (sq)
    const int i = i0 + il;
    if (i >= N) return;
    const size_t slab_base = (size_t)blockIdx.x * (1 + 2 * Q);
    if (qg == 0) part[slab_base * N + i] = acc_r;
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
        const int q = qg + 4 * k;
        if (q < Q) {
            part[(slab_base + 1 + q) * N + i] = acc_x[k];
            part[(slab_base + 1 + Q + q) * N + i] = acc_q[k];
        }
    }
}

// out element (b, k, i): kernel b's slabs added in slab order
__global__ __launch_bounds__(256) void gram_grad_batched_reduce_kernel(int B, int N, int Q, int slabs,
                                                                       const double *__restrict__ part, double *__restrict__ r,
                                                                       double *__restrict__ sx, double *__restrict__ sq) {
    const size_t per_slab = (size_t)(1 + 2 * Q) * N;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= per_slab * B) return;
    const size_t b = e / per_slab, eb = e - b * per_slab;
    const double *pb = part + b * slabs * per_slab + eb;
    double s = 0.0;
    for (int k = 0; k < slabs; ++k) s += pb[(size_t)k * per_slab];
    const int kk = (int)(eb / N), i = (int)(eb % N);
    if (kk == 0) r[b * N + i] = s;
    else if (kk <= Q) sx[(b * N + i) * Q + (kk - 1)] = s;
    else sq[(b * N + i) * Q + (kk - 1 - Q)] = s;
}

template <int KQ>
int launch_gram_grad_batched_kq(int B, int N, int Q, const GgPlan &p, const double *x, const double *gamma,
                                const double *alpha, const double *w, int ldw, long long w_stride, double *part,
                                hipStream_t st) {
    const size_t lds = gg_lds_bytes(Q);
    if (dpgp_set_dyn_lds(reinterpret_cast<const void *>(gram_grad_batched_kernel<KQ>), lds)) return DPGP_ERR_LAUNCH;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL((gram_grad_batched_kernel<KQ>), dim3((unsigned)((size_t)B * p.slabs), p.row_tiles), dim3(256), lds, st,
                       N, Q, p.slabs, p.chunks_per_slab, x, gamma, alpha, w, ldw, w_stride, part);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

// both launches of a checked call: the partial sums into part, then the slabs added into (r, sx, sq)
int launch_gram_grad_batched(int B, int N, int Q, const double *x, const double *gamma, const double *alpha, const double *w,
                             int ldw, long long w_stride, double *r, double *sx, double *sq, double *part, hipStream_t st) {
    const GgPlan p = gg_plan_batched(B, N);
    const int kq = dpgp_ceil_div(Q, 4);
    int rc = kq <= 1   ? launch_gram_grad_batched_kq<1>(B, N, Q, p, x, gamma, alpha, w, ldw, w_stride, part, st)
             : kq <= 2 ? launch_gram_grad_batched_kq<2>(B, N, Q, p, x, gamma, alpha, w, ldw, w_stride, part, st)
             : kq <= 4 ? launch_gram_grad_batched_kq<4>(B, N, Q, p, x, gamma, alpha, w, ldw, w_stride, part, st)
             : kq <= 8 ? launch_gram_grad_batched_kq<8>(B, N, Q, p, x, gamma, alpha, w, ldw, w_stride, part, st)
                       : launch_gram_grad_batched_kq<16>(B, N, Q, p, x, gamma, alpha, w, ldw, w_stride, part, st);
    if (rc) return rc;
    const size_t tot = (size_t)B * (1 + 2 * Q) * N;
    DPGP_PRELAUNCH();
    hipLaunchKernelGGL(gram_grad_batched_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, B, N, Q, p.slabs,
                       part, r, sx, sq);
    DPGP_LAUNCH_CHECK();
    return DPGP_OK;
}

// the kernels' 32-bit row offset b N, the grid's x extent and the reduction's block count stay below 2^31
bool gg_batched_in_range(int B, int N, int Q) {
    if (B <= 0 || N <= 0 || Q <= 0 || Q > DPGP_GRAM_GRAD_MAX_Q) return false;
    const GgPlan p = gg_plan_batched(B, N);
    const unsigned long long lim = 0x7fffffffull;
    return (unsigned long long)B * N <= lim && (unsigned long long)B * p.slabs <= lim && ((unsigned long long)B * (1 + 2 * Q) * N + 255) / 256 <= lim;
}

}  // namespace

extern "C" size_t dpgp_ard_rbf_gram_grad_batched_workspace_bytes(int B, int N, int Q) {
    if (!gg_batched_in_range(B, N, Q)) return 0;
    const GgPlan p = gg_plan_batched(B, N);
    return sizeof(double) * (size_t)B * p.slabs * (1 + 2 * Q) * N;
}

// (B = 1: every int N >= 1 is in range, so this is 0 only for N <= 0 or Q outside [1, DPGP_GRAM_GRAD_MAX_Q])
extern "C" size_t dpgp_ard_rbf_gram_grad_workspace_bytes(int N, int Q) {
    return dpgp_ard_rbf_gram_grad_batched_workspace_bytes(1, N, Q);
}

extern "C" int dpgp_ard_rbf_gram_grad_f64(int N, int Q, const double *x, const double *gamma, const double *alpha,
                                          const double *w, int ldw, double *r, double *sx, double *sq, void *ws,
                                          size_t ws_bytes, void *stream) {
    if (N < 0) return -1;
    if (Q <= 0 || Q > DPGP_GRAM_GRAD_MAX_Q) return -2;
    if (N == 0) return DPGP_OK;
    if (!x) return -3;
    if (!gamma) return -4;
    if (!alpha) return -5;
    if (!w) return -6;
    if (ldw < N) return -7;
    if (!r) return -8;
    if (!sx) return -9;
    if (!sq) return -10;
    if (!ws) return -11;
    if (ws_bytes < dpgp_ard_rbf_gram_grad_workspace_bytes(N, Q)) return -12;
    return launch_gram_grad_batched(1, N, Q, x, gamma, alpha, w, ldw, 0, r, sx, sq, static_cast<double *>(ws), (hipStream_t)stream);
}

extern "C" int dpgp_ard_rbf_gram_grad_batched_f64(int B, int N, int Q, const double *x, const double *gamma,
                                                  const double *alpha, const double *w, int ldw, long long w_stride, double *r,
                                                  double *sx, double *sq, void *ws, size_t ws_bytes, void *stream) {
    if (B < 0) return -1;
    if (N < 0) return -2;
    if (Q <= 0 || Q > DPGP_GRAM_GRAD_MAX_Q) return -3;
    if (B == 0 || N == 0) return DPGP_OK;
    if (!gg_batched_in_range(B, N, Q)) return -1;
    if (!x) return -4;
    if (!gamma) return -5;
    if (!alpha) return -6;
    if (!w) return -7;
    if (ldw < N) return -8;
    if (B > 1 && w_stride < (long long)(N - 1) * ldw + N) return -9;
    if (!r) return -10;
    if (!sx) return -11;
    if (!sq) return -12;
    if (!ws) return -13;
    if (ws_bytes < dpgp_ard_rbf_gram_grad_batched_workspace_bytes(B, N, Q)) return -14;
    return launch_gram_grad_batched(B, N, Q, x, gamma, alpha, w, ldw, w_stride, r, sx, sq, static_cast<double *>(ws),
                                    (hipStream_t)stream);
}
