// Pieces shared by the fp64 operators over deterministic latent points: ard_rbf_point_metric.hip (metric, Jacobian, Christoffel),
// ard_rbf_point_energy.hip, ard_rbf_point_cov.hip and geodesic_accel.hip.  No helper knows its caller.
//
// Left in the files, because the copies differ and a parameter would only make unlike things look alike:
//   the point staging      pe_kernel keeps x and v TRANSPOSED, [Q][16] (a point is a lane of its exponent and finishing loops),
//                          mt_kernel [NP][Q] (a point is a column tile), pc_kernel reads x from memory;
//   gamma in LDS           pc_kernel stores sg PRE-SCALED by -1/2 log2(e), the others store gamma itself (they need it again
//                          for the derivative features);
//   the z rows             pe_kernel prefetches them through registers one step ahead with its tile, mt_kernel stages them
//                          directly, pc_kernel reads them from memory;
//   the exponent loops     each reads those differently laid-out arrays, and sums different things next to the exponent;
//   the symmetrised tile   (p + p^T) of pe_kernel and pc_kernel: the registers pa / pb, the clamped unconditional fetch, the
//                          transposed store and the add are the same lines in both, and were tried here as one force-inlined
//                          helper.  The compiler simplifies a helper on its own before it inlines it, without the callers'
//                          facts about t and sP, and both kernels came out with other address arithmetic and register use
//                          (same occupancy, no scratch); ard_rbf_point_cov ran 0.4 - 1.9 % slower than before.
//                          The lines stay in the kernels until a form is found that compiles to what they compile to there.
#pragma once
#include <type_traits>
#include "internal.h"

#define DPGP_POINT_MS 64            // rows of the left operand per slab = inner indices per chunk = edge of its tile in LDS
#define DPGP_POINT_PS 66            // row stride of that tile in LDS: lanes (i, kk) of a half wave fall on 32 distinct bank pairs
#define DPGP_POINT_MAX_N 0x3fffffff // bound on N, M (and J): the int indices of the kernels hold them
// The point operators write their results from registers and need no scratch memory; the query and the (ws, ws_bytes) pair
// are there so that every point operator is called the same way.  DPGP_POINT_WS bytes for a shape in range, 0 outside.
#define DPGP_POINT_WS 256

// K, N, M, R >= 1, 1 <= Q <= max_q, and sizes that the 32-bit grid (np points per workgroup) and the int indices of the kernel
// hold.  R: the rows of the left operand (M where it is p [M][M])
static inline bool dpgp_point_shape_ok(int K, int N, int M, int Q, int R, int max_q, int np) {
    if (K < 1 || N < 1 || M < 1 || R < 1 || Q < 1 || Q > max_q) return false;
    if (N > DPGP_POINT_MAX_N || M > DPGP_POINT_MAX_N || R > DPGP_POINT_MAX_N) return false;
    return (long)K * dpgp_ceil_div(N, np) <= 0x7fffffffL;
}

// f(std::integral_constant<int, QT>) for the tile count qt = QT of a point's columns, 1 .. 4 (4 for anything else)
template <class F> static inline int dpgp_dispatch_qt(int qt, F &&f) {
    return qt == 1   ? f(std::integral_constant<int, 1>{})
           : qt == 2 ? f(std::integral_constant<int, 2>{})
           : qt == 3 ? f(std::integral_constant<int, 3>{})
                     : f(std::integral_constant<int, 4>{});
}
