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
"""
import numpy as np
import torch

from .. import ops
from ..utils.types import TORCH_DTYPE
from . import collapsed


class _Marginals:
    """K kernels' training side: z [K,M,Q], gamma [K,Q], alpha [K], beta [K], zfac [K,M,M] or None, c [K,G,M,M] = K_uu^-1 - P per
    pattern, r [K,M,D] the posterior weights per output column and gidx [K,D] (int32) each column's pattern, -1: never observed."""

    def __init__(self, z, gamma, alpha, beta, zfac, c, r, gidx):
        self.z, self.gamma, self.alpha, self.beta = z.contiguous(), gamma.contiguous(), alpha.contiguous(), beta.contiguous()
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

    def curve_terms(self, x, v, p, prior):
        """(e [N*], dx [N*, Q], dv [N*, Q]): e_n = v_n^T G(x_n) v_n of metric_total's G along the directions v [N*, Q] at the
        points x [N*, Q], and its gradients with respect to x_n and v_n: what a curve's energy and its gradient are made of
        (models/geodesic.py).  (p, prior) are _metric_operands' pair, formed once by the caller; prior may hold further
        constant diagonal metrics [*, Q, Q] (only the diagonals are read).  ONE call of ops.ard_rbf_point_energy per block of
        points, summed over the K kernels, plus the prior's share sum_q w_q v_q^2 in e and 2 w_q v_q in dv,
        w_q = sum_k n_k alpha_k gamma_kq.  Blocks of at most 2^25 result entries, as metric_total."""
        x, v = x.contiguous(), v.contiguous()
        k, q = self.z.shape[0], self.z.shape[2]
        step = max(1, (1 << 25) // (k * (2 * q + 1)))
        parts = []
        for i in range(0, x.shape[0], step):
            out = ops.ard_rbf_point_energy(self.z, x[i:i + step], v[i:i + step], self.gamma, self.alpha, p)
            parts.append([o[0] if k == 1 else torch.sum(o, dim=0) for o in out])
        e, dx, dv = (ps[0] if len(ps) == 1 else torch.cat(ps) for ps in zip(*parts))
        w = torch.sum(torch.diagonal(prior, dim1=-2, dim2=-1).reshape(-1, q), dim=0)
        return e + torch.sum(v * v * w, dim=1), dx, dv + 2.0 * v * w

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


def columns_arg(columns, d, device):
    cols = np.arange(d) if columns is None else np.asarray(columns, dtype=np.int64).reshape(-1)
    assert cols.size >= 1 and cols.min() >= 0 and cols.max() < d, 'columns must be output dims in [0, D)'
    return torch.as_tensor(cols, dtype=torch.long, device=device)


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
    for p, cols in enumerate(columns):
        ct = torch.as_tensor(np.asarray(cols), dtype=torch.long, device=device)
        r[:, ct] = rb[p, :, :len(cols)]
        gidx[ct] = p
    i0 = slots[0]
    return _Marginals(c['z'][i0:i0 + 1], c['gamma'][i0:i0 + 1], c['alpha'][i0:i0 + 1].reshape(1), be, c['zfac'][i0:i0 + 1],
                      cm[None], r[None], gidx[None])


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
