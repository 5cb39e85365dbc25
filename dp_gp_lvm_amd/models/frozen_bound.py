"""
The q(X*) part of the prediction bounds (shared by bayesian_gp_lvm, manifold_relevance_determination and the per-entry
missing-data path of dp_gp_lvm): B frozen ARD-RBF kernels sharing one q(X*), evaluated in fp64 by the library's operators.
"""
import math

import numpy as np
import torch

from .. import ops
from ..utils.types import TORCH_DTYPE
from . import collapsed


def _as_device(v, device, shape=None):
    t = torch.as_tensor(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float64), dtype=TORCH_DTYPE)
    return (t if shape is None else t.reshape(shape)).to(device).contiguous()


def _put(v, device):
    return v.detach().to(device=device, dtype=TORCH_DTYPE).contiguous() if torch.is_tensor(v) else _as_device(v, device)


def _own_z(z, gamma, alpha, beta, device):
    """Lists of K kernels' values (z [M,Q] each) -> stacked (z [K,M,Q], gamma [K,Q], alpha [K], beta [K]) and their factors."""
    z = torch.stack([_as_device(v, device) for v in z]).contiguous()
    gamma = torch.stack([_as_device(v, device).reshape(-1) for v in gamma]).contiguous()
    alpha = torch.cat([_as_device(v, device).reshape(-1) for v in alpha]).contiguous()
    beta = torch.cat([_as_device(v, device).reshape(-1) for v in beta]).contiguous()
    return (z, gamma, alpha, beta), collapsed.own_z_kernels(z, gamma, alpha)


class _TestBound:
    """The q(X*) part of the prediction bounds of bayesian_gp_lvm / manifold_relevance_determination (gaussian_process.py:365-394,
    :776-831, :880-919): B frozen ARD-RBF kernels ("slots": inducing inputs z [B,M,Q], gamma [B,Q], alpha [B], beta [B]) sharing
    q(X*), each with its own test outputs y_b [N*, D_b].  Everything runs in fp64 on the device, whatever precision the model
    trains in.

    Once per object (the trained model is frozen): K_uu_b, L_b^-1, K_uu_b^-1 and the q(X*)-independent pair factor of Psi2, formed
    by one of the three entry points below.  Per evaluation: Psi1*, Psi2* of the B kernels (one qx_psi_stats_batched), then
    models/collapsed.py with D = D_b and N_w = N*:
        f_hat*_b = 1/2 N* D_b (log beta - log 2 pi) - D_b log|L_A| + 1/2 D_b beta (tr T - alpha N*) + 1/2 beta^2 |U|^2 - 1/2 beta |Y|^2
    and, for the gradient, G2 in the difference form and G1 = beta^2 Y R^T contracted with dPsi/d(mu, s) by one qx_psi_adjoint.
    No host synchronisation.

    Per-entry observation masks: slot b has weights w_b [N*] (1 where its output dims were measured at test point n) and y_b
    zero-filled where they were not.  With N_b = sum_n w_b[n]: Psi2* is the weighted sum (the weighted stats operator), N* becomes
    N_b in the first and third term, G2 keeps its formula and goes to the weighted adjoint; U, |Y|^2 and G1 need no change because
    the zero rows of Y carry the mask.  weights None is the arithmetic above, bit for bit."""

    def __init__(self, z, gamma, alpha, beta, factors, y, dims, weights, device):
        """z [B,M,Q], gamma [B,Q], alpha [B], beta [B] and factors = (L^-1, K_uu^-1, potrf info, pair factor) of the slots'
        kernels, all at the slots; y [B,N*,Dmax] (zero where unobserved and in the padding columns), dims [B] (the slots' numbers
        of output dims), weights [B,N*] or None."""
        self.z, self.gamma, self.alpha, self.beta = z, gamma, alpha, beta
        self.li, self.kinv, self.info_uu, self.zfac = factors
        self.m, self.device, self.n_t = z.shape[1], device, y.shape[1]
        self.dims = torch.as_tensor(np.asarray(dims, dtype=np.float64), dtype=TORCH_DTYPE, device=device)
        self.y = _put(y, device)
        self.yy = torch.sum(self.y * self.y, dim=(1, 2))
        self.eye = torch.eye(self.m, dtype=TORCH_DTYPE, device=device)
        self.weights = None if weights is None else _put(weights, device)
        self.n_w = None if weights is None else torch.sum(self.weights, dim=1)
        self.terms = self.info = None

    @classmethod
    def kernels(cls, z, gamma, alpha, beta, ys, device):
        """B kernels with their own inducing inputs (lists of B) and their own complete outputs ys[b] [N*, D_b]; no weights."""
        hyp, factors = _own_z(z, gamma, alpha, beta, device)
        y = torch.zeros((len(ys), ys[0].shape[0], max(v.shape[1] for v in ys)), dtype=TORCH_DTYPE, device=device)
        for i, v in enumerate(ys):
            y[i, :, :v.shape[1]] = v                                                            # zero-padded columns
        return cls(*hyp, factors, y, [v.shape[1] for v in ys], None, device)

    @classmethod
    def slots(cls, z, gamma, alpha, beta, y, dims, weights, device):
        """B slots over ONE set of inducing inputs z [M,Q].  gamma [K,Q], alpha [K], beta [K] with K = B (a kernel per slot) or
        K = 1 (one kernel for every slot: K_uu, L^-1, K_uu^-1 and the pair factor are formed once and expanded)."""
        b = y.shape[0]
        z = _put(z, device)
        gamma = _put(gamma, device).reshape(-1, z.shape[1])
        alpha, beta = _put(alpha, device).reshape(-1), _put(beta, device).reshape(-1)
        k = gamma.shape[0]
        assert k in (1, b) and alpha.numel() == k and beta.numel() == k, 'one kernel, or one per slot'
        rep = (lambda t: t.expand(b, *t.shape[1:]).contiguous()) if k != b else (lambda t: t.contiguous())
        factors = tuple(rep(t) for t in collapsed.shared_z_kernels(z, gamma, alpha))
        return cls(z[None].expand(b, *z.shape).contiguous(), rep(gamma), rep(alpha), rep(beta), factors, y, dims, weights, device)

    def psi(self, mu, s):
        """Unweighted Psi1*, Psi2* of the kernels (every test point counts)."""
        return ops.qx_psi_stats_batched(self.z, mu, s, self.gamma, self.alpha, self.zfac)

    def evaluate(self, mu, s, grad=False):
        """f_hat* summed over the B kernels (0-d tensor); with grad, also d f_hat* / d(mu, s).  self.terms: [B x 5] per-kernel
        terms (the five summands above), self.info: failed factorisations of A (0 = fine)."""
        be, dd = self.beta, self.dims
        n_t = self.n_t if self.weights is None else self.n_w                                 # N*, or N_b [B]
        psi_1, psi_2 = ops.qx_psi_stats_batched(self.z, mu, s, self.gamma, self.alpha, self.zfac, weights=self.weights)
        ch = collapsed.Chain(self.li, psi_2, be, self.eye).project(ops.matmul(psi_1.transpose(1, 2), self.y))   # u [B, M, Dmax]
        self.info = ch.info
        self.terms = torch.stack([0.5 * n_t * dd * (torch.log(be) - math.log(2.0 * math.pi)), -dd * ch.logdet,
                                  0.5 * dd * be * (ch.tr - self.alpha * n_t), 0.5 * be * be * torch.sum(ch.u * ch.u, dim=(1, 2)),
                                  -0.5 * be * self.yy], dim=1)
        f = torch.sum(self.terms)
        if not grad:
            return f, psi_1, psi_2
        adj = collapsed.Adjoint(ch, dd)
        g1 = (be * be)[:, None, None] * ops.matmul(self.y, adj.r.transpose(1, 2))            # [B, N*, M]
        d_mu, d_s = ops.qx_psi_adjoint(self.z, mu, s, self.gamma, self.alpha, g1, adj.g2_difference(self.kinv), self.zfac,
                                       weights=self.weights)
        return f, d_mu, d_s


def kernel_slots(z, gamma, alpha, beta, kern, y, dims, weights, device):
    """B slots over K kernels that each have their own inducing inputs (lists of K, as _TestBound.kernels takes them; the per-entry
    masks of manifold_relevance_determination at test time); kern [B]: slot b's kernel.  The factors are formed once per
    kernel and gathered to the slots."""
    hyp, factors = _own_z(z, gamma, alpha, beta, device)
    idx = torch.as_tensor(np.asarray(kern, dtype=np.int64), device=device)
    take = lambda t: t.index_select(0, idx).contiguous()
    return _TestBound(*(take(t) for t in hyp), tuple(take(t) for t in factors), y, dims, weights, device)
