"""
The frozen test bound of dp_gp_lvm (the over-D model) under per-entry observation masks, without slots.  The columns of the
over-D model share Z and q(X*) and differ only in their mixed (gamma_d, alpha_d, beta_d) and in the test points at which they
were measured (models/masked_bound_d.py says the same of the training side): Psi2*_b is ops.psi2(weights=), Psi1*_b enters
only as v_b = Psi1*_b^T y_b (ops.psi1T_y on the zero-filled data), and the (mu*, S*) adjoint of both is ONE call of
ops.psi_latent_adjoint.  No replicated Z, no Psi1* [B,N*,M] and no adjoint of that size.
"""
import math

import torch

from .. import ops
from ..utils.constants import GP_DEFAULT_JITTER
from ..utils.types import TORCH_DTYPE
from . import collapsed


class _TestBoundD:
    """B columns (those with at least one observed test entry) over one set of inducing inputs z [M,Q]: gamma [B,Q], alpha [B],
    beta [B], y [N*,B] zero where unobserved, weights [B,N*] (1 where column b was measured at test point n).  fp64 on the device.

    Once per object (the trained model is frozen): K_b = K_uu(gamma_b, alpha_b) + jitter I = L L^T, L^-1, K_b^-1 on [B,M,M].
    Per evaluation, with N_b = sum_n w_bn:  Psi2*_b = sum_n w_bn psi2_bn,  v_b = Psi1*_b^T y_b, then models/collapsed.py with D = 1,
    N_w = N_b, J = 1:
        f_hat*_b = 1/2 N_b (log beta - log 2 pi) - log|L_A| + 1/2 beta (tr T - alpha N_b) + 1/2 beta^2 |u|^2 - 1/2 beta |y_b|^2
    (the five terms of _TestBound.evaluate with D_b = 1 and N* -> N_b, in that order in self.terms [B x 5]) and, for the gradient,
    G2 in the difference form and g_v = beta^2 r, contracted with dPsi/d(mu, s) by ops.psi_latent_adjoint.  No host
    synchronisation.  self.info: failed factorisations of A."""

    def __init__(self, z, gamma, alpha, beta, y, weights, device):
        f64 = TORCH_DTYPE
        put = lambda v: v.detach().to(device=device, dtype=f64).contiguous()
        self.z = put(z)
        m, q = self.z.shape
        self.gamma = put(gamma).reshape(-1, q)
        b = self.gamma.shape[0]
        self.alpha, self.beta = put(alpha).reshape(-1), put(beta).reshape(-1)
        self.y, self.weights = put(y), put(weights)
        self.n_t = self.y.shape[0]
        assert self.alpha.numel() == b and self.beta.numel() == b, 'alpha and beta must be [B]'
        assert tuple(self.y.shape) == (self.n_t, b) and tuple(self.weights.shape) == (b, self.n_t), 'y must be [N* x B], weights [B x N*]'
        self.m, self.device = m, device
        self.n_w = torch.sum(self.weights, dim=1)
        self.yy = torch.sum(self.y * self.y, dim=0)
        ones = torch.ones(b, dtype=f64, device=device)
        self.li, self.info_uu = collapsed.factors(ops.ard_rbf_gram(self.z, None, self.gamma, self.alpha, ones, include_noise=False,
                                                                   include_jitter=True, jitter=GP_DEFAULT_JITTER))
        self.kinv = collapsed.k_inverse(self.li)
        self.eye = torch.eye(m, dtype=f64, device=device)
        self.terms = self.info = None

    def evaluate(self, mu, s, grad=False):
        """f_hat* summed over the B columns (0-d tensor) with (v [B,M], Psi2* [B,M,M]); with grad: (f_hat*, d_mu, d_s)."""
        be, n_w = self.beta, self.n_w
        mu, s = mu.contiguous(), s.contiguous()
        psi_2 = ops.psi2(self.z, mu, s, self.gamma, self.alpha, weights=self.weights)
        v = ops.psi1T_y(self.z, mu, s, self.gamma, self.alpha, self.y)                       # [B, M]
        ch = collapsed.Chain(self.li, psi_2, be, self.eye).project(v[:, :, None])             # u [B, M, 1]
        self.info = ch.info
        self.terms = torch.stack([0.5 * n_w * (torch.log(be) - math.log(2.0 * math.pi)), -ch.logdet, 0.5 * be * (ch.tr - self.alpha * n_w),
                                  0.5 * be * be * torch.sum(ch.u * ch.u, dim=(1, 2)), -0.5 * be * self.yy], dim=1)
        f = torch.sum(self.terms)
        if not grad:
            return f, v, psi_2
        adj = collapsed.Adjoint(ch)
        g_v = (be * be)[:, None] * adj.r[:, :, 0]
        d_mu, d_s = ops.psi_latent_adjoint(self.z, mu, s, self.gamma, self.alpha, self.y, g_v.contiguous(),
                                           adj.g2_difference(self.kinv).contiguous(), weights=self.weights)
        return f, d_mu, d_s


class _ShardedTestBoundD:
    """The test bound of a D-sharded model: `local` is the _TestBoundD of this rank's columns that have an observed test entry, or
    None where there is none (the rank then contributes zeros and still joins).  The bound is a sum over columns of terms on the
    replicated (Z, q(X*)), so one evaluation is the local one followed by ONE sum all-reduce of a packed fp64 buffer: f_hat* and,
    with grad, d_mu and d_s (1 + 2 N* Q values).  process_group None: the local partial values, no exchange.  KL(q(X*)) is not in
    here: the caller adds it once, after the exchange, identically on every rank."""

    def __init__(self, local, n_t, q, device, process_group=None):
        self.local, self.n_t, self.q, self.device, self.group = local, n_t, q, device, process_group
        self.terms = torch.zeros((0, 5), dtype=TORCH_DTYPE, device=device)
        self.info = torch.zeros(0, dtype=torch.int32, device=device)

    def evaluate(self, mu, s, grad=False):
        """(f_hat*, None, None), or with grad (f_hat*, d_mu, d_s): the values summed over the ranks."""
        nq = self.n_t * self.q
        flat = torch.zeros(1 + (2 * nq if grad else 0), dtype=TORCH_DTYPE, device=self.device)
        if self.local is not None:
            res = self.local.evaluate(mu, s, grad=grad)
            flat[0] = res[0]
            if grad:
                flat[1:1 + nq] = res[1].reshape(-1)
                flat[1 + nq:] = res[2].reshape(-1)
            self.terms, self.info = self.local.terms, self.local.info
        if self.group is not None:
            import torch.distributed as dist
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)
        if not grad:
            return flat[0], None, None
        return flat[0], flat[1:1 + nq].reshape(self.n_t, self.q), flat[1 + nq:].reshape(self.n_t, self.q)
