"""
f_hat of dp_gp_lvm (the over-D model) for TRAINING data with missing entries (observed=...), and its derivatives, in fp64 on
the device.  The columns of the over-D model share Z and q(X) and differ only in their mixed (gamma_d, alpha_d, beta_d) and in
the rows R_d at which they were measured: that is the batch layout of the fp64 operators of the unmasked precision='f64' model
with ONE addition, a 0 / 1 weight per (column, row) on the Psi2 sum and on its adjoint (ops.psi2(weights=),
ops.elbo_grad_psi(prec='f64', weights=): dpgp_psi2_weighted_f64, dpgp_elbo_grad_psi_weighted_f64).  Psi1 enters only as
v_d = Psi1_d^T y_d, and a zero-filled y carries the mask there.  No replicated Z, no Psi1 [D,N,M] and no slot machinery.

    f_hat = sum over the columns d observed somewhere of the five terms of the unmasked model
            (oracle/dpgp_oracle_torch.py:fhat_from_pieces) with N -> N_d = sum_n w_dn, Psi2_d = sum_n w_dn psi2_dn,
            v_d = Psi1_d^T y_d, y_d^T y_d over the observed rows.

A column never observed is left out of the operator batch (it contributes nothing to f_hat and its derivative rows are zero).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from ..utils import missing as _missing
from ..utils.constants import GP_DEFAULT_JITTER
from ..utils.types import TORCH_DTYPE
from . import collapsed


class _MaskedBoundD:
    """One slot per column d observed somewhere, in the symbols of models/collapsed.py with K_d = K_uu(gamma_d, alpha_d) +
    jitter I, D = 1, N_w = N_d, J = 1 and no phi:
        terms[d] = 1/2 N_d (log beta_d - log 2 pi), -log|L_A|, 1/2 beta_d (tr T_d - alpha_d N_d), -1/2 beta_d y_d^T y_d,
                   1/2 beta_d^2 |u_d|^2
    Adjoints: g_psi2_d = G2 in the product form, g_v_d = beta_d^2 r_d, w_kuu_d = GK_d .* (K_d - jitter I),
        d alpha_d = -1/2 beta_d N_d + (sum w_kuu_d + 2 <g_psi2_d, Psi2_d> + g_v_d . v_d) / alpha_d
    d beta_d the core's summand, and (mu, S, z, gamma_d) by the weighted stage B on the adjoints padded to Mp.  No host
    synchronisation."""

    def __init__(self, y0, observed, device):
        f64 = TORCH_DTYPE
        observed = np.asarray(observed)
        # (the columns of one rank of a D-sharded model may hold no observed entry: an empty batch, on which no operator is launched;
        #  "at least one True" is the model's check on the global mask)
        cols = _missing.observed_columns(observed)
        self.n, self.d = observed.shape
        self.device = device
        self.cols_np = cols
        self.all_columns = cols.size == self.d
        self.cols = torch.as_tensor(cols, dtype=torch.long, device=device)
        self.y = torch.as_tensor(np.ascontiguousarray(y0[:, cols]), dtype=f64, device=device).contiguous()      # [N, Dc], zero-filled
        self.weights = torch.as_tensor(np.ascontiguousarray(observed[:, cols].T), dtype=f64, device=device).contiguous()   # [Dc, N]
        self.n_d = torch.sum(self.weights, dim=1)
        self.yy = torch.sum(self.y * self.y, dim=0)
        self.terms = None                                   # [Dc x 5] of the last evaluation
        self.info = torch.zeros(cols.size, dtype=torch.int32, device=device)

    def take(self, t):
        """Rows of a per-column array [D, ...] that belong to the operator batch."""
        return t if self.all_columns else t.index_select(0, self.cols)

    def scatter(self, t):
        """[Dc, ...] -> [D, ...], zero rows for the columns never observed."""
        if self.all_columns:
            return t.contiguous()
        return torch.zeros((self.d,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device).index_copy_(0, self.cols, t)

    def chain(self, z, mu, s, gamma, alpha, beta, sel=None):
        """gamma [Dc,Q], alpha [Dc], beta [Dc] of the batch columns: statistics and factors shared by the bound, its backward
        pass, the imputation and the predictive moments.  sel (long tensor): only these columns of the batch (gamma, alpha, beta
        are then theirs)."""
        y = self.y if sel is None else self.y.index_select(1, sel).contiguous()
        w = self.weights if sel is None else self.weights.index_select(0, sel).contiguous()
        c = dict(k_uu=ops.ard_rbf_gram(z, None, gamma, alpha, beta, include_noise=False, include_jitter=True, jitter=GP_DEFAULT_JITTER))
        c['li'], info_k = collapsed.factors(c['k_uu'])
        psi_2 = ops.psi2(z, mu, s, gamma, alpha, weights=w)
        c['v'] = ops.psi1T_y(z, mu, s, gamma, alpha, y)                                     # [Dc, M]
        c['chain'] = collapsed.Chain(c['li'], psi_2, beta)
        if sel is None:
            self.info = torch.maximum(info_k.abs(), c['chain'].info.abs()).to(torch.int32)
        return c

    def evaluate(self, z, mu, s, gamma, alpha, beta, grad=False):
        """f_hat as a 1-element tensor; with grad also (d_mu [N,Q], d_s [N,Q], d_z [M,Q], d_gamma [Dc,Q], d_alpha_beta [Dc,2]).
        self.terms: [Dc x 5]; self.info [Dc]: 0 where K_d and A_d factorised."""
        n_d = self.n_d
        if self.cols_np.size == 0:                          # no column of this share was observed: f_hat = 0, zero derivatives
            zeros = lambda *shape: torch.zeros(shape, dtype=TORCH_DTYPE, device=self.device)
            self.terms = zeros(0, 5)
            return (zeros(1), (zeros(*mu.shape), zeros(*s.shape), zeros(*z.shape), zeros(0, z.shape[1]), zeros(0, 2))) if grad \
                else zeros(1)
        c = self.chain(z, mu, s, gamma, alpha, beta)
        v, ch = c['v'], c['chain'].project(c['v'][:, :, None])                                    # u [Dc, M, 1]
        uu = torch.sum(ch.u * ch.u, dim=(1, 2))
        self.terms = torch.stack([0.5 * n_d * (torch.log(beta) - math.log(2.0 * math.pi)), -ch.logdet,
                                  0.5 * beta * (ch.tr - alpha * n_d), -0.5 * beta * self.yy, 0.5 * beta * beta * uu], dim=1)
        f = torch.sum(self.terms).reshape(1)
        if not grad:
            return f
        m = z.shape[0]
        mp = 16 * ((m + 15) // 16)
        adj = collapsed.Adjoint(ch, outer=torch.mul)
        g2 = adj.g2_product(collapsed.k_inverse(c['li']))
        wk = adj.gk() * (c['k_uu'] - GP_DEFAULT_JITTER * torch.eye(m, dtype=TORCH_DTYPE, device=self.device))
        gv = beta[:, None] ** 2 * adj.r[:, :, 0]
        d_alpha = -0.5 * beta * n_d + (wk.sum(dim=(1, 2)) + 2.0 * (g2 * ch.psi_2).sum(dim=(1, 2)) + torch.sum(gv * v, dim=1)) / alpha
        d_beta = adj.d_beta(n_d, alpha, uu, self.yy)
        pad2 = (0, mp - m, 0, mp - m)
        d_mu, d_s, d_z, d_gamma = ops.elbo_grad_psi(self.y, z, mu, s, gamma, alpha, F.pad(g2, pad2).contiguous(),
                                                    F.pad(wk, pad2).contiguous(), F.pad(gv, (0, mp - m)).contiguous(), prec='f64',
                                                    weights=self.weights)
        return f, (d_mu, d_s, d_z, d_gamma, torch.stack([d_alpha, d_beta], dim=1).contiguous())

    def posterior(self, z, mu, s, gamma, alpha, beta, sel=None):
        """(c_d = K_d^-1 - P_d [K,M,M], rhs_d = beta_d P_d v_d [K,M]): what the predictive moments of the batch columns `sel` need."""
        c = self.chain(z, mu, s, gamma, alpha, beta, sel=sel)
        rhs, cm = collapsed.posterior(c['chain'].r0, collapsed.k_inverse(c['li']), beta, c['v'][:, :, None])
        return cm, rhs[:, :, 0]
