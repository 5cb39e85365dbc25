"""
The q(X*) part of the prediction bounds (shared by bayesian_gp_lvm, manifold_relevance_determination and the per-entry
missing-data path of dp_gp_lvm): B frozen ARD-RBF kernels sharing one q(X*), evaluated in fp64 by the library's operators.
"""
import math

import numpy as np
import torch

from .. import ops
from ..utils.constants import GP_DEFAULT_JITTER
from ..utils.types import TORCH_DTYPE


def _as_device(v, device, shape=None):
    t = torch.as_tensor(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float64), dtype=TORCH_DTYPE)
    return (t if shape is None else t.reshape(shape)).to(device).contiguous()


class _TestBound:
    """The q(X*) part of the prediction bounds of bayesian_gp_lvm / manifold_relevance_determination (gaussian_process.py:365-394,
    :776-831, :880-919): B frozen ARD-RBF kernels (inducing inputs z [B,M,Q], gamma [B,Q], alpha [B], beta [B]) sharing q(X*), each
    with its own test outputs y_b [N*, D_b].  Everything runs in fp64 on the device, whatever precision the model trains in.

    Once per object (the trained model is frozen): K_uu_b, its Cholesky factor L_b, L_b^-1, K_uu_b^-1 (ard_rbf_gram / potrf_batched /
    tril_inverse_batched / matmul) and the q(X*)-independent pair factor of Psi2 (ops.qx_pair_factor).
    Per evaluation: Psi1*, Psi2* of the B kernels (one qx_psi_stats_batched), then on [B, M, M] arrays
        T = L^-1 Psi2* L^-T,  A = beta T + I = L_A L_A^T,  R0 = L_A^-1 L^-1,  U = R0 Psi1*^T Y,
        f_hat*_b = 1/2 N* D_b (log beta - log 2 pi) - D_b log|L_A| + 1/2 D_b beta (tr T - alpha N*) + 1/2 beta^2 |U|^2 - 1/2 beta |Y|^2
    and, for the gradient, the adjoints  (P = R0^T R0 = (K_uu + beta Psi2*)^-1,  R = R0^T U)
        G2 = 1/2 D_b beta (K_uu^-1 - P) - 1/2 beta^3 R R^T,    G1 = beta^2 Y R^T
    contracted with dPsi/d(mu, s) by one qx_psi_adjoint.  No host synchronisation.

    Per-entry observation masks (_TestBound.slots): kernel ("slot") b has weights w_b [N*] (1 where its output dims were measured
    at test point n) and y_b zero-filled where they were not.  With N_b = sum_n w_b[n]: Psi2* is the weighted sum (the weighted
    stats operator), N* becomes N_b in the first and third term, G2 keeps its formula and goes to the weighted adjoint; U, |Y|^2
    and G1 need no change because the zero rows of Y carry the mask.  weights None is the arithmetic above, bit for bit."""

    def __init__(self, z, gamma, alpha, beta, ys, device):
        f64 = TORCH_DTYPE
        self.z = torch.stack([_as_device(v, device) for v in z]).contiguous()                       # [B, M, Q]
        self.gamma = torch.stack([_as_device(v, device).reshape(-1) for v in gamma]).contiguous()   # [B, Q]
        self.alpha = torch.cat([_as_device(v, device).reshape(-1) for v in alpha]).contiguous()     # [B]
        self.beta = torch.cat([_as_device(v, device).reshape(-1) for v in beta]).contiguous()       # [B]
        b, m = self.z.shape[0], self.z.shape[1]
        self.m, self.device = m, device
        self.dims = torch.tensor([y.shape[1] for y in ys], dtype=f64, device=device)
        n_t, dmax = ys[0].shape[0], max(y.shape[1] for y in ys)
        self.n_t = n_t
        self.y = torch.zeros((b, n_t, dmax), dtype=f64, device=device)                          # zero-padded columns
        for i, y in enumerate(ys):
            self.y[i, :, :y.shape[1]] = y
        self.yy = torch.sum(self.y * self.y, dim=(1, 2))
        one = torch.ones(1, 1, dtype=f64, device=device)
        k_uu = torch.stack([ops.ard_rbf_gram(self.z[i], None, self.gamma[i:i + 1], self.alpha[i].reshape(1, 1), one,
                                             include_noise=False, include_jitter=True, jitter=GP_DEFAULT_JITTER)[0]
                            for i in range(b)])
        self.l_uu, self.info_uu = ops.potrf_batched(k_uu)
        self.li = ops.tril_inverse_batched(self.l_uu)
        self.kinv = ops.matmul(self.li.transpose(1, 2), self.li)
        self.zfac = ops.qx_pair_factor(self.z, self.gamma, self.alpha)
        self.eye = torch.eye(m, dtype=f64, device=device)
        self.terms = None
        self.weights = self.n_w = None

    @classmethod
    def slots(cls, z, gamma, alpha, beta, y, dims, weights, device):
        """B slots over ONE set of inducing inputs z [M,Q]: y [B,N*,Dmax] (zero where unobserved and in the padding columns),
        dims [B] (the slots' numbers of output dims), weights [B,N*].  gamma [K,Q], alpha [K], beta [K] with K = B (a kernel per
        slot) or K = 1 (one kernel for every slot: K_uu, L, L^-1, K_uu^-1 and the pair factor are formed once and expanded)."""
        f64 = TORCH_DTYPE
        self = cls.__new__(cls)
        b, m = y.shape[0], z.shape[0]
        put = lambda v: v.detach().to(device=device, dtype=f64).contiguous() if torch.is_tensor(v) else _as_device(v, device)
        z = put(z)
        gamma = put(gamma).reshape(-1, z.shape[1])
        alpha, beta = put(alpha).reshape(-1), put(beta).reshape(-1)
        k = gamma.shape[0]
        assert k in (1, b) and alpha.numel() == k and beta.numel() == k, 'one kernel, or one per slot'
        ones = torch.ones(k, dtype=f64, device=device)
        k_uu = ops.ard_rbf_gram(z, None, gamma, alpha, ones, include_noise=False, include_jitter=True, jitter=GP_DEFAULT_JITTER)
        l_uu, info_uu = ops.potrf_batched(k_uu)
        li = ops.tril_inverse_batched(l_uu)
        kinv = ops.matmul(li.transpose(1, 2), li)
        zfac = ops.ard_rbf_gram(z, None, 0.5 * gamma, alpha * alpha, ones)
        rep_ = (lambda t: t.expand(b, *t.shape[1:]).contiguous()) if k != b else (lambda t: t.contiguous())
        self.z = z[None].expand(b, *z.shape).contiguous()
        self.gamma, self.alpha, self.beta = rep_(gamma), rep_(alpha), rep_(beta)
        self.l_uu, self.info_uu, self.li, self.kinv, self.zfac = rep_(l_uu), rep_(info_uu), rep_(li), rep_(kinv), rep_(zfac)
        self.m, self.device, self.n_t = m, device, y.shape[1]
        self.dims = torch.as_tensor(np.asarray(dims, dtype=np.float64), dtype=f64, device=device)
        self.y = put(y)
        self.yy = torch.sum(self.y * self.y, dim=(1, 2))
        self.eye = torch.eye(m, dtype=f64, device=device)
        self.terms = None
        self.weights = put(weights)
        self.n_w = torch.sum(self.weights, dim=1)
        return self

    def psi(self, mu, s):
        """Unweighted Psi1*, Psi2* of the kernels (every test point counts)."""
        return ops.qx_psi_stats_batched(self.z, mu, s, self.gamma, self.alpha, self.zfac)

    def evaluate(self, mu, s, grad=False):
        """f_hat* summed over the B kernels (0-d tensor); with grad, also d f_hat* / d(mu, s).  self.terms: [B x 5] per-kernel
        terms (the five summands above), self.info: failed factorisations of A (0 = fine)."""
        be, dd = self.beta, self.dims
        n_t = self.n_t if self.weights is None else self.n_w                                 # N*, or N_b [B]
        psi_1, psi_2 = ops.qx_psi_stats_batched(self.z, mu, s, self.gamma, self.alpha, self.zfac, weights=self.weights)
        tm = ops.matmul(ops.matmul(self.li, psi_2), self.li.transpose(1, 2))
        l_a, self.info = ops.potrf_batched(be[:, None, None] * tm + self.eye)
        r0 = ops.matmul(ops.tril_inverse_batched(l_a), self.li)
        u = ops.matmul(r0, ops.matmul(psi_1.transpose(1, 2), self.y))                       # [B, M, Dmax]
        logdet = torch.sum(torch.log(torch.diagonal(l_a, dim1=-2, dim2=-1)), dim=-1)
        tr = torch.diagonal(tm, dim1=-2, dim2=-1).sum(-1)
        self.terms = torch.stack([0.5 * n_t * dd * (torch.log(be) - math.log(2.0 * math.pi)), -dd * logdet,
                                  0.5 * dd * be * (tr - self.alpha * n_t), 0.5 * be * be * torch.sum(u * u, dim=(1, 2)),
                                  -0.5 * be * self.yy], dim=1)
        f = torch.sum(self.terms)
        if not grad:
            return f, psi_1, psi_2
        r = ops.matmul(r0.transpose(1, 2), u)                                                  # [B, M, Dmax]
        p = ops.matmul(r0.transpose(1, 2), r0)
        g2 = (0.5 * dd * be)[:, None, None] * (self.kinv - p) - (0.5 * be ** 3)[:, None, None] * ops.matmul(r, r.transpose(1, 2))
        g1 = (be * be)[:, None, None] * ops.matmul(self.y, r.transpose(1, 2))                # [B, N*, M]
        d_mu, d_s = ops.qx_psi_adjoint(self.z, mu, s, self.gamma, self.alpha, g1, g2, self.zfac, weights=self.weights)
        return f, d_mu, d_s
