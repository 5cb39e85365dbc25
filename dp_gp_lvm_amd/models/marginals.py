"""
Per-entry predictive moments of the sparse GP models at a test-point q(X*) = (mu, s), on ONE operator call
(ops.qx_psi_point_moments, csrc/qx_psi_point.hip).  With p(d) the training row pattern of output column d (the rows at which d was
observed; one pattern for complete training data), P_p = (K_uu + beta Psi2_p)^-1 and r_d = beta P_p(d) Psi1^T y_d over those rows,

    mean(n,d) = psi1*(n) . r_d
    var(n,d)  = alpha + 1/beta - tr((K_uu^-1 - P_p(d)) Psi2*(n)) + r_d^T Psi2*(n) r_d - mean(n,d)^2

psi1*(n), Psi2*(n) test point n's own statistics.  Observation noise 1/beta is included; a column never observed in training has
r_d = 0 and no trace term: mean 0, variance alpha + 1/beta.  The training side (the chain of models/masked_bound.py) is formed once
per _Marginals; summed over the test points the variance is the reference-shaped array's entry,
    sum_n var(n,d) = covar[d,0,0] + (N* - 1)/beta                            (gaussian_process._predictive_moments).

The same training side gives the geometry of the map from latent space to data at a DETERMINISTIC latent point x (Tosi et al.,
"Metrics for probabilistic geometries", UAI 2014): with b_mq(x) = d k_m(x) / d x_q the Jacobian row of column d is Gaussian,
    mean m_d(x) = b(x)^T r_d [Q],     covariance Sigma_d(x) = alpha diag(gamma) - b(x)^T (K_uu^-1 - P_p(d)) b(x) [Q x Q]
(d^2 k(x, x') / dx_q dx'_q' = alpha gamma_q delta_qq' at x' = x; the noise-free function: no 1/beta), and the expected metric over
a set of columns is G(x) = sum_d (m_d m_d^T + Sigma_d); sqrt(det G) is the magnification factor.  _Marginals.jacobian / .metric.

And the JOINT posterior of column d's noise-free function at several deterministic latent points: mean k(x)^T r_d and
    cov_d(x, x') = alpha exp(-1/2 sum_q gamma_q (x_q - x'_q)^2) - k(x)^T (K_uu^-1 - P_p(d)) k(x')
whose diagonal is var(n,d) at s = 0 less 1/beta: _Marginals.pattern_covariance / .covariance (ops.ard_rbf_point_cov, or the composed
form where it is faster) and .sample (one batched Cholesky over the (kernel, pattern) pairs, one batched product).

Every model's metric is the same object, a sum over parts b_k(x)^T P_k b_k(x) plus constant diagonal terms: Metric, built once per
public call from the models' (_Marginals, P, prior) parts, gives the curve terms, the geodesic acceleration and its tangent that
models/geodesic.py works on (the shared methods are in models/latent_geometry.py).
"""
import numpy as np
import torch

from .. import ops
from ..utils.types import TORCH_DTYPE
from . import collapsed
from .geodesic import _rk4, _rk4_tangent, prior_terms


class _Marginals:
    """K kernels' training side: z [K,M,Q], gamma [K,Q], alpha [K], beta [K], zfac [K,M,M] or None, c [K,G,M,M] = K_uu^-1 - P per
    pattern, r [K,M,D] the posterior weights per output column and gidx [K,D] (int32) each column's pattern, -1: never observed."""

    def __init__(self, z, gamma, alpha, beta, zfac, c, r, gidx, all_seen=False, gidx_host=None):
        """all_seen: the caller knows (on the host) that no column has gidx < 0; pattern_covariance then adds no prior pattern.
        gidx_host: gidx as a NumPy array, where the builder has it: pattern_covariance then runs only the patterns that the chosen
        columns touch, planned on the host without reading the device."""
        self.z, self.gamma, self.alpha, self.beta = z.contiguous(), gamma.contiguous(), alpha.contiguous(), beta.contiguous()
        self.all_seen = bool(all_seen)
        self.gidx_host = None if gidx_host is None else np.asarray(gidx_host, dtype=np.int64).reshape(tuple(gidx.shape))
        self.zfac = None if zfac is None else zfac.contiguous()
        self.c, self.r, self.gidx = c.contiguous(), r.contiguous(), gidx.contiguous()

    def at(self, mu, s, cols=None):
        """(mean, var) [K, N*, len(cols)] at q(X*) = (mu, s); cols: a long tensor of output columns on the device (default all)."""
        r, gidx = self.r, self.gidx
        if cols is not None:
            r, gidx = r.index_select(2, cols).contiguous(), gidx.index_select(1, cols).contiguous()
        return ops.qx_psi_point_moments(self.z, mu.contiguous(), s.contiguous(), self.gamma, self.alpha, self.c, r, gidx, self.beta,
                                        zfac=self.zfac)

    def jacobian(self, x, cols=None):
        """[K, N*, len(cols), Q]: the mean of the Jacobian row of every column at the deterministic latent points x [N*,Q],
        m_d(x) = b(x)^T r_d with b_mq = d k_m / d x_q (ops.ard_rbf_point_jacobian; the module's text for r)."""
        r = self.r if cols is None else self.r.index_select(2, cols).contiguous()
        return ops.ard_rbf_point_jacobian(self.z, x.contiguous(), self.gamma, self.alpha, r)

    def metric(self, x, cols=None, weights=None):
        """[K, N*, Q, Q]: every kernel's share of the expected metric of the noise-free map at x [N*,Q] over the columns `cols`,
            G_k(x) = sum_d w_kd (m_d m_d^T + Sigma_d) = n_k alpha_k diag(gamma_k) + b_k(x)^T P_k b_k(x)
            Sigma_d = alpha_k diag(gamma_k) - b^T c_p(d) b,   P_k = sum_d w_kd (r_d r_d^T - c_p(d)),   n_k = sum_d w_kd
        weights [K, D] (default: ones; the over-T model passes phi).  P_k is R diag(w) R^T and a pattern-count-weighted sum of c,
        both by ops.matmul; the quadratic form is ONE call of ops.ard_rbf_point_metric.  A column never observed in training
        (gidx < 0, r = 0) has no c term: it contributes w alpha diag(gamma).  1/beta does not enter."""
        p, prior = self._metric_operands(cols, weights)
        return ops.ard_rbf_point_metric(self.z, x.contiguous(), self.gamma, self.alpha, p) + prior[:, None]

    def metric_total(self, x, cols=None, weights=None):
        """[N*, Q, Q]: metric summed over the K kernels.  The operator's [K, n, Q, Q] result is taken over blocks of n points of at
        most 2^25 entries, so K = D kernels on a large grid need no array of size K N* Q^2 (a point's bits do not depend on its
        block)."""
        p, prior = self._metric_operands(cols, weights)
        x = x.contiguous()
        k, q = self.z.shape[0], self.z.shape[2]
        step = max(1, (1 << 25) // (k * q * q))
        out = [torch.sum(ops.ard_rbf_point_metric(self.z, x[i:i + step], self.gamma, self.alpha, p), dim=0)
               for i in range(0, x.shape[0], step)]
        return torch.cat(out) + torch.sum(prior, dim=0)

    def _patterns(self, cols):
        """(c [K, G', M, M], slot [K, J] long): the patterns to evaluate and, per kernel and column, its place among them.  With
        gidx_host (and host columns: columns_arg's .host) G' counts only the patterns that `cols` touch, in ascending order, plus
        one with c = 0, whose covariance is the prior gram, if a chosen column was never observed in training (gidx < 0); planned
        on the host, the places go to the device by a copy that nothing waits for.  Without it: all G patterns, plus the prior
        pattern unless all_seen."""
        k, g, m = self.c.shape[0], self.c.shape[1], self.c.shape[2]
        zero = lambda: torch.zeros((k, 1, m, m), dtype=TORCH_DTYPE, device=self.c.device)
        host = None if self.gidx_host is None else \
            (self.gidx_host if cols is None else (None if getattr(cols, 'host', None) is None else self.gidx_host[:, cols.host]))
        if host is not None:
            used = np.unique(host[host >= 0])
            prior = bool((host < 0).any()) or used.size == 0
            place = np.full(g + 1, used.size, dtype=np.int64)                # (never observed: the prior pattern, last)
            place[used] = np.arange(used.size)
            c = self.c if used.size == g else self.c.index_select(1, torch.as_tensor(used, device=self.c.device))
            c = torch.cat([c, zero()], dim=1) if prior else c
            return c.contiguous(), torch.as_tensor(place[np.where(host < 0, g, host)], device=self.c.device)
        gidx = self.gidx if cols is None else self.gidx.index_select(1, cols)
        slot = gidx.to(torch.long)
        if self.all_seen:
            return self.c, slot
        return torch.cat([self.c, zero()], dim=1), torch.where(slot < 0, torch.full_like(slot, g), slot)

    def pattern_covariance(self, x, cols=None):
        """(cov [K, G', N*, N*], slot [K, J]): the joint posterior covariance of the noise-free functions of every (kernel,
        pattern that `cols` touch: _patterns) at the deterministic latent points x [N*, Q],
            cov_kg(x, x') = alpha_k exp(-1/2 sum_q gamma_kq (x_q - x'_q)^2) - k_k(x)^T c[k, g] k_k(x'),
        by ONE call of ops.ard_rbf_point_cov over the K kernels and their patterns (at many points by composed_covariance where
        composed_is_faster's cost model says so); the last pattern may be the prior gram (c = 0: the operator's
        quadratic form is then an exact 0).  Column cols[j] of kernel k has the matrix cov[k, slot[k, j]]; columns of
        one (kernel, pattern) share it.  Exactly symmetric matrices; 1/beta does not enter."""
        c, slot = self._patterns(cols)
        if composed_is_faster(c.shape[0], c.shape[1], x.shape[0], c.shape[2]):
            return composed_covariance(self.z, x.contiguous(), self.gamma, self.alpha, c), slot
        return ops.ard_rbf_point_cov(self.z, x.contiguous(), self.gamma, self.alpha, c), slot

    def covariance(self, x, cols=None):
        """[K, J, N*, N*]: pattern_covariance's matrices laid out per column, cov[k, j] = the joint posterior covariance of
        column cols[j] under kernel k at the points x (K J N*^2 doubles: columns of one pattern repeat the same matrix)."""
        cov, slot = self.pattern_covariance(x, cols)
        return cov[torch.arange(cov.shape[0], device=cov.device)[:, None], slot]

    def sample(self, x, xi, cols=None, noise=False, jitter=1e-6):
        """(f [K, S, N*, J], info): joint draws of the columns `cols` at the points x [N*, Q] from standard normal draws xi
        [S, N*, J] (shared by the kernels) or [K, S, N*, J],
            f[k, s, :, j] = mean_kj + L_k,g(j) xi[s, :, j],     L L^T = cov_kg + (jitter alpha_k (+ 1/beta_k with noise)) I
        pattern_covariance's matrices are factorised by ONE ops.potrf_batched call over the K G' (kernel, pattern)
        pairs, and ONE ops.matmul, batched over the pairs, applies every factor to all S J draw columns; a gather then keeps,
        for column j, the product with its own pattern's factor.  This costs G' times the flops of a product grouped by
        pattern and needs no knowledge of the groups on the host: the number of launches does not depend on the number of
        columns, and nothing here synchronises.  info [K G'] is potrf's (non-zero: that matrix is not positive definite
        at this jitter); reading it is the caller's."""
        cov, slot = self.pattern_covariance(x, cols)
        k, g1, n = cov.shape[0], cov.shape[1], cov.shape[2]
        shift = jitter * self.alpha + (1.0 / self.beta.reshape(-1) if noise else 0.0)                 # [K]
        cov = cov + shift[:, None, None, None] * torch.eye(n, dtype=TORCH_DTYPE, device=cov.device)
        l, info = ops.potrf_batched(cov.reshape(k * g1, n, n))
        s, j = xi.shape[-3], xi.shape[-1]
        # the draws as [N*, S J] (one matrix for every pair) or [K G', N*, S J] against the factors l [K G', N*, N*]
        rhs = xi.transpose(-3, -2).reshape(xi.shape[:-3] + (n, s * j))
        if xi.dim() == 4:
            rhs = rhs[:, None].expand(k, g1, n, s * j).reshape(k * g1, n, s * j)
        prod = ops.matmul(torch.tril(l), rhs).reshape(k, g1, n, s, j)
        pick = slot[:, None, None, None, :].expand(k, 1, n, s, j)
        dev = torch.gather(prod, 1, pick)[:, 0]                                                       # [K, N*, S, J]
        mean, _ = self.at(x, torch.zeros_like(x), cols)                                               # [K, N*, J]
        return (mean[:, :, None, :] + dev).permute(0, 2, 1, 3).contiguous(), info

    def _metric_operands(self, cols, weights):
        """(P [K, M, M], n_k alpha_k diag(gamma_k) [K, Q, Q]) of metric's text."""
        r, gidx = self.r, self.gidx
        if cols is not None:
            r, gidx = r.index_select(2, cols).contiguous(), gidx.index_select(1, cols)
        k, m, g = r.shape[0], r.shape[1], self.c.shape[1]
        w = torch.ones(gidx.shape, dtype=TORCH_DTYPE, device=r.device) if weights is None else \
            (weights if cols is None else weights.index_select(1, cols))
        p = ops.matmul(r * w[:, None, :], r.transpose(1, 2))                                       # [K, M, M]
        hit = gidx[:, :, None] == torch.arange(g, dtype=gidx.dtype, device=r.device)               # [K, J, G]
        counts = torch.sum(hit.to(TORCH_DTYPE) * w[:, :, None], dim=1)                              # [K, G]
        ops.matmul(counts[:, None, :].contiguous(), self.c.reshape(k, g, m * m), out=p.view(k, 1, m * m), alpha=-1.0, beta=1.0)
        return p, (torch.sum(w, dim=1) * self.alpha)[:, None, None] * torch.diag_embed(self.gamma)


# ---- the metric a latent-geometry call runs under: what models/latent_geometry.py hands to models/geodesic.py -------------------
def _diagonal_sum(prior, q):
    """w [Q]: the summed diagonals of the constant metrics prior [*, Q, Q]."""
    return torch.sum(torch.diagonal(prior, dim1=-2, dim2=-1).reshape(-1, q), dim=0).contiguous()


class Metric:
    """The metric that ONE public call runs under, G(x) = sum over parts and their kernels of b_k(x)^T P_k b_k(x), plus constant
    diagonal metrics.  parts: a list of (marg: _Marginals, P [K, M, M], prior [K, Q, Q]), _metric_operands' pair behind its
    _Marginals (one part per model; MRD's summed metric has one per view); extra: further constant diagonal metrics [*, Q, Q] or
    None (only the diagonals of prior and extra are read).  No part and an extra is the prior-only metric (dp_gp_lvm with no
    chosen column observed in training).  Several parts with an extra occur nowhere and are refused.  Its four methods are the
    callables of models/geodesic.py; every one runs in blocks of points of at most 2^25 result entries, and a point's bits do not
    depend on its block.  shoot and shoot_tangent are the integrators on the device over accel and accel_tangent: whole
    Runge-Kutta solutions with the bits of geodesic.py's loops, blocked over the curves in the same way.

    A part carries its own prior because the sums differ: the energy of several parts is formed part by part, each with its own
    prior share, and summed over the stacked parts; the acceleration hands ONE w, over all priors, to one factorisation."""

    def __init__(self, parts, extra=None):
        assert len(parts) <= 1 or extra is None, 'several parts with an extra prior are not defined'
        assert parts or extra is not None, 'a metric needs a part or a prior'
        self.parts = [(marg, p) for marg, p, _ in parts]
        self.q = q = parts[0][0].z.shape[2] if parts else extra.shape[-1]
        self.block = (1 << 25) // max(1, sum(marg.z.shape[0] for marg, _ in self.parts) * (q * q + q))   # accel's points per block
        priors = [prior for _, _, prior in parts] + ([] if extra is None else [extra])
        self.w = _diagonal_sum(priors[0] if len(priors) == 1 else torch.cat(priors), q)        # over all priors: accel's
        self.ws = [self.w] if len(parts) <= 1 else [_diagonal_sum(prior, q) for prior in priors]  # per part: curve_terms'

    def curve_terms(self, x, v):
        """(e [N], dx [N, Q], dv [N, Q]): e_n = v_n^T G(x_n) v_n along the directions v [N, Q] at the points x [N, Q], and its
        gradients with respect to x_n and v_n: what a curve's energy and its gradient are made of.  Per part ONE call of
        ops.ard_rbf_point_energy per block of points, summed over the part's K kernels, plus its prior's share sum_q w_q v_q^2
        in e and 2 w_q v_q in dv; several parts' terms are stacked and summed."""
        if not self.parts:
            return prior_terms(v, self.w)
        x, v, q = x.contiguous(), v.contiguous(), self.q
        each = []
        for (marg, p), w in zip(self.parts, self.ws):
            k = marg.z.shape[0]
            step = max(1, (1 << 25) // (k * (2 * q + 1)))
            blocks = []
            for i in range(0, x.shape[0], step):
                out = ops.ard_rbf_point_energy(marg.z, x[i:i + step], v[i:i + step], marg.gamma, marg.alpha, p)
                blocks.append([o[0] if k == 1 else torch.sum(o, dim=0) for o in out])
            e, dx, dv = (bs[0] if len(bs) == 1 else torch.cat(bs) for bs in zip(*blocks))
            each.append((e + torch.sum(v * v * w, dim=1), dx, dv + 2.0 * v * w))
        return each[0] if len(each) == 1 else tuple(torch.sum(torch.stack(ts), dim=0) for ts in zip(*each))

    def accel(self, x, v):
        """(a [N, Q], speed [N], info [N] int32): the acceleration x'' = -G(x)^-1 Gamma(x, v) of the geodesic through the points
        x with the velocities v, speed = v^T G v, and the factorisation's info (0, or the failing pivot: a is then NaN at that
        point).  With G = G0 + sum_k b_k^T P_k b_k the geodesic obeys G x'' = -sum_k Gamma_k: one call of
        ops.ard_rbf_point_christoffel per part gives the slabs (g_k, Gamma_k), one call of ops.geodesic_accel sums the
        concatenated slabs, adds G0 = diag(w), factorises and solves.  The prior-only metric has straight lines: (0, w . v^2, 0)."""
        if not self.parts:
            return torch.zeros_like(v), torch.sum(v * v * self.w, dim=1), torch.zeros(v.shape[0], dtype=torch.int32, device=v.device)
        return self._solve(ops.ard_rbf_point_christoffel, ops.geodesic_accel, 1, (x.contiguous(), v.contiguous()))

    def accel_tangent(self, x, v, dx, dv):
        """(a, da [N, Q], speed [N], info [N] int32): accel's triple with its bits, and da, the derivative of the acceleration
        along the direction (dx, dv) of the state (x, v).  One call of ops.ard_rbf_point_christoffel_tangent per part gives the
        slabs (g_k, Gamma_k, dg_k, dGamma_k), one call of ops.geodesic_accel_tangent sums them and solves twice with one
        factor.  Twice accel's entries per point, so half its points per block.  The prior-only metric: da = 0."""
        if not self.parts:
            a, speed, info = self.accel(x, v)
            return a, torch.zeros_like(v), speed, info
        return self._solve(ops.ard_rbf_point_christoffel_tangent, ops.geodesic_accel_tangent, 2,
                           (x.contiguous(), v.contiguous(), dx.contiguous(), dv.contiguous()))

    def transport(self, x, v, w):
        """(a [N, Q], dw [N, F, Q], speed [N], info [N] int32): accel's triple with its bits, and the rates
        dw_r = -G(x)^-1 Gamma(x; v, w_r) of the vectors w [N, F, Q] in parallel transport along the geodesics through x with the
        velocities v.  One call of ops.ard_rbf_point_transport per part gives the slabs (g_k, Gamma_k, Gamma_k(v, w_r)), one
        call of ops.geodesic_transport sums them and solves for all 1 + F right-hand sides with one factor.  K (Q^2 + Q + F Q)
        entries per point go into the 2^25-entry blocks.  Q + 1 + F <= 64.  The prior-only metric has no symbols: dw = 0."""
        if not self.parts:
            a, speed, info = self.accel(x, v)
            return a, torch.zeros_like(w), speed, info
        q, f = self.q, w.shape[1]
        step = self.block * (q * q + q) // (q * q + q + f * q)          # accel's points per block, scaled to this call's entries
        return self._solve(ops.ard_rbf_point_transport, ops.geodesic_transport, 1, (x.contiguous(), v.contiguous(), w.contiguous()),
                           step=step)

    def shoot(self, x, v, num_steps):
        """(curve, vel [C, S+1, Q], bad [C] int32): geodesic._rk4 on accel from the states x, v [C, Q], with its bits, by the
        integrator on the device: ONE call of ops.geodesic_shoot per block of curves (accel's points per block) runs every
        stage of every step.  The prior-only metric takes the host loop: straight lines."""
        if not self.parts:
            return _rk4(self.accel, x, v, num_steps)
        return self._shoot(ops.geodesic_shoot, 1, (x.contiguous(), v.contiguous()), num_steps)

    def shoot_tangent(self, x, v, dx, dv, num_steps):
        """(curve, vel, dcurve, dvel [C, S+1, Q], bad [C] int32, speed0 [C]): geodesic._rk4_tangent on accel_tangent, with its
        bits, by ops.geodesic_shoot_tangent, as shoot (accel_tangent's points per block)."""
        if not self.parts:
            return _rk4_tangent(self.accel_tangent, x, v, dx, dv, num_steps)
        return self._shoot(ops.geodesic_shoot_tangent, 2, (x.contiguous(), v.contiguous(), dx.contiguous(), dv.contiguous()),
                           num_steps)

    def _shoot(self, run, width, state, num_steps):
        """run(the parts' operands, w, *state, num_steps) per block of the curves of state, blocked as _solve blocks a stage."""
        parts = [(marg.z, marg.gamma, marg.alpha, p) for marg, p in self.parts]
        n, step = state[0].shape[0], max(1, self.block // width)
        blocks = [run(parts, self.w, *(state if step >= n else [t[i:i + step] for t in state]), num_steps)
                  for i in range(0, n, step)]
        return blocks[0] if len(blocks) == 1 else tuple(torch.cat(bs) for bs in zip(*blocks))

    def _solve(self, slabs_of, solve, width, state, step=None):
        """solve(the parts' concatenated slabs_of(state), w, v) per block of the points of state = (x, v[, dx, dv | w]), `width`
        times accel's entries per point (or `step` points per block, where the caller counts them itself).  A stage of an
        integrator comes here: one block (the usual case) is neither sliced nor concatenated."""
        parts, w, n = self.parts, self.w, state[0].shape[0]
        step = max(1, self.block // width if step is None else step)
        blocks = []
        for i in range(0, n, step):
            sb = state if step >= n else [t[i:i + step] for t in state]
            slabs = [slabs_of(marg.z, *sb, marg.gamma, marg.alpha, p) for marg, p in parts]
            blocks.append(solve(*(slabs[0] if len(slabs) == 1 else [torch.cat(ss) for ss in zip(*slabs)]), w, sb[1]))
        return blocks[0] if len(blocks) == 1 else tuple(torch.cat(bs) for bs in zip(*blocks))


# ---- the joint posterior at latent points: what the models' predictive_covariance / sample_functions share ---------------------
DEFAULT_SAMPLE_JITTER = 1e-6
"""sample_functions' default jitter, in units of the kernel's alpha.  A choice, not a measurement: the gram of nearby points has
its smallest eigenvalue below rounding, and the Cholesky factorisation needs a shift well above eps N* lambda_max ~ 1e-12 alpha;
1e-6 alpha is far above that and far below any 1/beta the models train to."""


def composed_is_faster(k, g, n, m):
    """The route of _Marginals.pattern_covariance: a cost model of the two forms in microseconds, fitted to the timings of
    tools/time_point_cov.py on one MI355X, where it picks the faster form, or one within 20 % of it, at every
    measured layout.
      fused:     a workgroup per (kernel, pair of 32-point tiles), 256 at a time; each makes its features (about 18 us per block of
                 64 inducing points) and runs one step per (pair of blocks, pattern) (about 9 us): the first product is repeated
                 for every PAIR of point tiles, so the time grows with N*^2 M^2.
      composed:  about 80 us of launches plus 18 us per kernel (one gram launch each), then 6.5 passes over the K G N*^2 doubles of
                 the result at 3 TB/s."""
    tiles, blocks = (n + 31) // 32, (m + 63) // 64
    rounds = (k * tiles * (tiles + 1) // 2 + 255) // 256
    fused = rounds * (18.0 * blocks + 9.0 * blocks * blocks * g)
    composed = 80.0 + 18.0 * k + 6.5 * 8.0 * k * g * n * n / 3.0e6
    return composed < fused


def composed_covariance(z, x, gamma, alpha, c):
    """ops.ard_rbf_point_cov's result [K, G, N, N] composed of the other operators: ops.ard_rbf_gram per kernel for the features
    [K, N, M], two ops.matmul with the symmetric parts of c, ops.ard_rbf_gram for the prior term; the difference is symmetrised at
    the end, (a + a^T) / 2, so that this route's result is exactly symmetric too.  Memory: K N M + 2 K G N^2 + K G N M doubles."""
    k, g, m = c.shape[0], c.shape[1], c.shape[2]
    n = x.shape[0]
    feat = torch.stack([ops.ard_rbf_gram(x, z[i], gamma[i:i + 1], alpha[i:i + 1], alpha[i:i + 1])[0] for i in range(k)])
    ct = (0.5 * (c + c.transpose(2, 3))).reshape(k * g, m, m)
    fg = feat[:, None].expand(k, g, n, m).reshape(k * g, n, m) if g > 1 else feat
    quad = ops.matmul(ops.matmul(fg, ct), fg.transpose(1, 2))                                     # [K G, N, N]
    out = ops.ard_rbf_gram(x, None, gamma, alpha, alpha)[:, None] - quad.reshape(k, g, n, n)
    return 0.5 * (out + out.transpose(2, 3))


def with_noise(cov, inv_beta):
    """cov [J, N*, N*] with inv_beta (one element, or [J]) added on the diagonals."""
    eye = torch.eye(cov.shape[-1], dtype=TORCH_DTYPE, device=cov.device)
    return cov + inv_beta.reshape(-1, 1, 1) * eye


def draw_generator(seed, device):
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
    return gen


def standard_draws(draws, num_samples, n, j, gen, device):
    """xi [S, N*, J]: standard normal draws from the device generator `gen`, or the caller's `draws` (numpy or torch)."""
    if draws is None:
        assert int(num_samples) >= 1, 'num_samples must be at least 1'
        return torch.randn((int(num_samples), n, j), generator=gen, dtype=TORCH_DTYPE, device=device)
    xi = draws.detach() if torch.is_tensor(draws) else torch.as_tensor(np.asarray(draws, dtype=np.float64))
    xi = xi.to(device=device, dtype=TORCH_DTYPE).contiguous()
    assert xi.dim() == 3 and xi.shape[0] >= 1 and tuple(xi.shape[1:]) == (n, j), 'draws must be [S x N* x len(columns)]'
    return xi


def raise_if_not_factorised(info):
    """The one host read of sample_functions: potrf's info over every factorised matrix."""
    bad = int(torch.count_nonzero(info))
    if bad:
        raise FloatingPointError('sample_functions: %d of %d covariance matrices are not positive definite in fp64 at this jitter; '
                                 'raise `jitter` or set noise=True' % (bad, info.numel()))


def covariance_of(marg, x, cols, noise):
    """predictive_covariance of a one-kernel _Marginals: [J, N*, N*]."""
    cov = marg.covariance(x, cols)[0]
    return with_noise(cov, 1.0 / marg.beta) if noise else cov


def samples_of(marg, x, cols, num_samples, noise, jitter, seed, draws, infos=None):
    """sample_functions of a one-kernel _Marginals: [S, N*, J].  infos: a list that takes potrf's info in place of the host read
    (the caller then reads them all at once with raise_if_not_factorised)."""
    j = marg.gidx.shape[1] if cols is None else cols.numel()
    xi = standard_draws(draws, num_samples, x.shape[0], j, draw_generator(seed, x.device), x.device)
    f, info = marg.sample(x, xi, cols, noise, jitter)
    if infos is None:
        raise_if_not_factorised(info)
    else:
        infos.append(info)
    return f[0]


def columns_arg(columns, d, device):
    """The output dims as a long tensor on the device; it carries its host copy as .host (a NumPy array), so that a caller can
    plan on the host without reading the device (_Marginals._patterns)."""
    cols = np.arange(d) if columns is None else np.asarray(columns, dtype=np.int64).reshape(-1)
    assert cols.size >= 1 and cols.min() >= 0 and cols.max() < d, 'columns must be output dims in [0, D)'
    out = torch.as_tensor(cols, dtype=torch.long, device=device)
    out.host = cols
    return out


def points_arg(x, q, device):
    """x [N* x Q] (numpy array or torch tensor) as a contiguous fp64 tensor on the device."""
    x = x.detach() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float64))
    x = x.to(device=device, dtype=TORCH_DTYPE).contiguous()
    assert x.dim() == 2 and x.shape[0] >= 1 and x.shape[1] == q, 'x must be [N* x Q]'
    return x


def magnification(g):
    """sqrt(det G) [N*] of the metrics g [N*, Q, Q], as exp(1/2 logdet) from their Cholesky factors (ops.potrf_batched)."""
    l, _ = ops.potrf_batched(g.contiguous())
    return torch.exp(torch.sum(torch.log(torch.diagonal(l, dim1=-2, dim2=-1)), dim=-1))


def one_kernel(c, y, beta, slots, columns, d):
    """The _Marginals (K = 1) of the kernel that the slots `slots` (indices into the chain's batch) share: c the dict of
    _MaskedBound.chain / _MaskedViewsBound.chain, y [B,N,Dmax] the bound's zero-filled outputs, beta the kernel's noise precision
    (one element), columns[i] the output columns of slot slots[i] (their places in y), d the number of output columns."""
    device, m = y.device, c['r0'].shape[1]
    sel = torch.as_tensor(slots, dtype=torch.long, device=device)
    take = lambda t: t.index_select(0, sel).contiguous()
    v = ops.matmul(take(c['psi_1']).transpose(1, 2).contiguous(), take(y))                      # Psi1^T Y_p [P, M, Dmax]
    be = beta.reshape(1)
    rb, cm = collapsed.posterior(take(c['r0']), take(c['kinv']), be, v)                      # per pattern [P, ...]
    r = torch.zeros((m, d), dtype=TORCH_DTYPE, device=device)
    gidx = torch.full((d,), -1, dtype=torch.int32, device=device)
    gidx_host = np.full(d, -1, dtype=np.int64)
    for p, cols in enumerate(columns):
        ct = torch.as_tensor(np.asarray(cols), dtype=torch.long, device=device)
        r[:, ct] = rb[p, :, :len(cols)]
        gidx[ct] = p
        gidx_host[np.asarray(cols, dtype=np.int64)] = p
    i0 = slots[0]
    return _Marginals(c['z'][i0:i0 + 1], c['gamma'][i0:i0 + 1], c['alpha'][i0:i0 + 1].reshape(1), be, c['zfac'][i0:i0 + 1],
                      cm[None], r[None], gidx[None], all_seen=bool((gidx_host >= 0).all()), gidx_host=gidx_host[None])


def of_masked_bound(bound, z, mu, s, gamma, alpha, beta, d):
    """bayesian_gp_lvm: bound a masked_bound._MaskedBound (an all-True mask for complete training data)."""
    c = bound.chain(z, mu, s, gamma, alpha, beta)
    return one_kernel(c, bound.y, beta, list(range(bound.b)), [cols for cols, _ in bound.groups], d)


def of_masked_views_bound(bound, z, mu, s, gamma, alpha, beta, dims):
    """MRD: bound a masked_bound._MaskedViewsBound, z [V,M,Q], gamma [V,Q], alpha [V], beta [V]; one _Marginals per view."""
    c = bound.chain(z, mu, s, gamma, alpha, beta)
    out = []
    for v, d in enumerate(dims):
        slots = [i for i, (vv, _, _) in enumerate(bound.slots) if vv == v]
        out.append(one_kernel(c, bound.y, beta[v], slots, [bound.slots[i][1] for i in slots], d))
    return out


def unobserved_variance(var, observed):
    """var [N x D] at the unobserved entries, 0 at the observed ones."""
    return torch.where(torch.as_tensor(observed, device=var.device), torch.zeros_like(var), var)
