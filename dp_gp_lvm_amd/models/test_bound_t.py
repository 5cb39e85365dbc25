"""
The frozen test bound of dp_gp_lvm_t and the mixture's predictive moments: the over-T model's prediction paths, in fp64 on the
device.  The bound is masked_bound_t._MaskedBoundT on (y*, observed*) with everything trained held fixed, so only q(X*) moves;
the moments come from the per-point Psi2 contractions of ops.qx_psi_pointwise.
"""
import math

import torch

from .. import ops
from ..utils.constants import GP_DEFAULT_JITTER
from ..utils.types import TORCH_DTYPE
from .masked_bound_t import _MaskedBoundT


def mixture_moments(phit, mean_t, var_t):
    """Mean and variance [N, J] of the mixture sum_t phi_td N(mean_t(n,d), var_t(n,d)) per entry: phit [T, J] (columns sum to 1),
    mean_t, var_t [T, N, J].  mean = sum_t phi mean_t, var = sum_t phi (var_t + mean_t^2) - mean^2 (pure torch, any device)."""
    w = phit[:, None, :]
    mean = torch.sum(w * mean_t, dim=0)
    return mean, torch.sum(w * (var_t + mean_t * mean_t), dim=0) - mean * mean


class _TestBoundT(_MaskedBoundT):
    """f_hat* = sum_{d observed somewhere} ( -1/2 N_p(d) log 2 pi + sum_t phi_td F_t(y*_d on its rows) ), the symbols of
    _MaskedBoundT, with z [M,Q], the atoms (gamma [T,Q], alpha [T], beta [T]) and phit [T,D] frozen.
    Once per object: K_t, its factor, L_t^-1, K_t^-1, the pair factor zfac, the pattern grouping of observed* (P test patterns;
    P = 1 for complete test data), phi and |y*_d|^2 at the slots' places.
    Per evaluation: one ops.qx_psi_stats_grouped (K = T), the T P factorisations of A_tp, and with grad=True
        G2_tp = 1/2 D_tp beta_t^2 sym(K_t^-1 Psi2*_tp P_tp) - 1/2 beta_t^3 RR,    G1_t = beta_t^2 Y* diag(phi_t) R_t^T
    through one ops.qx_psi_adjoint_grouped for (d_mu, d_s) only: no parameter adjoint, no gram gradient, no host
    synchronisation.  The grouped operators are used whatever DPGP_GROUPED_PSI says (that switch is a training cross-check).
    self.terms: F_t(d) [T P, Dmax]; self.info: 0 when every K_t and every A_tp factorised."""

    def __init__(self, z, gat, aat, bat, phit, y0, observed, device):
        t = gat.shape[0]
        super().__init__(y0, observed, t, device)
        f64 = TORCH_DTYPE
        put = lambda a: a.detach().to(device=device, dtype=f64).contiguous()
        z, gat, aat, bat, phit = put(z), put(gat), put(aat).reshape(-1), put(bat).reshape(-1), put(phit)
        assert tuple(phit.shape) == (t, self.d), 'phit must be [T x D]'
        self.grouped = True
        self.m = z.shape[0]
        self.gat, self.aat, self.bat = gat, aat, bat
        k_uu = ops.ard_rbf_gram(z, None, gat, aat, self.ones_t, include_noise=False, include_jitter=True, jitter=GP_DEFAULT_JITTER)
        l_uu, info_uu = ops.potrf_batched(k_uu)
        li = ops.tril_inverse_batched(l_uu)
        self.info_uu = info_uu.abs().max()
        self.kinv_t = ops.matmul(li.transpose(1, 2), li)                                           # [T, M, M]
        self.zfac = ops.ard_rbf_gram(z, None, 0.5 * gat, aat * aat, self.ones_t)
        self.z_t = z[None].expand(t, *z.shape).contiguous()
        self.li, self.kinv, self.be, self.al = self._rep(li), self._rep(self.kinv_t), self._rep(bat), self._rep(aat)
        self.phis = self.to_slots(phit[:, None, :]).reshape(t * self.p, self.dmax)               # phi_td at the slots' places
        self.dd = torch.sum(self.phis, dim=1)                                                      # D_tp
        self.nw = self.n_w.repeat(t)
        self.yy_s, self.valid_s = self.yy.repeat(t, 1), self.valid.repeat(t, 1)
        self.const = -0.5 * math.log(2.0 * math.pi) * torch.sum(self.n_w * self.n_cols)
        self.eye = torch.eye(self.m, dtype=f64, device=device)

    def evaluate(self, mu, s, grad=False):
        """(f_hat* (0-d), d f_hat* / d mu, d f_hat* / d s); the derivatives are None without grad."""
        t, p, m = self.t, self.p, self.m
        be = self.be
        psi_1, psi_2 = ops.qx_psi_stats_grouped(self.z_t, mu, s, self.gat, self.aat, self.weights, zfac=self.zfac)
        psi_2 = psi_2.reshape(t * p, m, m)
        tm = ops.matmul(ops.matmul(self.li, psi_2), self.li.transpose(1, 2))
        l_a, info_a = ops.potrf_batched(be[:, None, None] * tm + self.eye)
        self.info = torch.maximum(self.info_uu, info_a.abs().max())
        r0 = ops.matmul(ops.tril_inverse_batched(l_a), self.li)
        u = ops.matmul(r0, self._columns(dict(psi_1=psi_1)))                                       # [T P, M, Dmax]
        logdet = torch.sum(torch.log(torch.diagonal(l_a, dim1=-2, dim2=-1)), dim=-1)
        tr = torch.diagonal(tm, dim1=-2, dim2=-1).sum(-1)
        uu = torch.sum(u * u, dim=1)
        per = 0.5 * self.nw * torch.log(be) + 0.5 * be * (tr - self.al * self.nw) - logdet
        fm = (per[:, None] - 0.5 * be[:, None] * self.yy_s + 0.5 * (be * be)[:, None] * uu) * self.valid_s
        f = torch.sum(self.phis * fm) + self.const
        self.terms = fm
        if not grad:
            return f, None, None
        d3, b3 = self.dd[:, None, None], be[:, None, None]
        r = ops.matmul(r0.transpose(1, 2), u)
        rphi = r * self.phis[:, None, :]
        pm = ops.matmul(r0.transpose(1, 2), r0)
        kpp = ops.matmul(ops.matmul(self.kinv, psi_2), pm)
        g2 = (0.25 * b3 * b3) * d3 * (kpp + kpp.transpose(1, 2)) - (0.5 * b3 ** 3) * ops.matmul(rphi, r.transpose(1, 2))
        r_all = self.to_columns(rphi.reshape(t, p, m, self.dmax))                                  # [T, M, D]: phi_td r_d
        g1 = (self.bat * self.bat)[:, None, None] * ops.matmul(self.y, r_all.transpose(1, 2))     # [T, N*, M]
        d_mu, d_s = ops.qx_psi_adjoint_grouped(self.z_t, mu, s, self.gat, self.aat, g1, g2.reshape(t, p, m, m), self.weights,
                                               zfac=self.zfac)
        return f, d_mu, d_s


class _MomentsT:
    """The training side of the over-T model's predictive moments, formed once: with p the training row pattern of column d,
    P_tp = (K_t + beta_t Psi2_tp)^-1 and r_td = beta_t P_tp Psi1_t^T y_d (0 for a column never observed in training),
        mean_t(n,d) = psi1*_t(n) . r_td
        var_t(n,d)  = alpha_t - tr((K_t^-1 - P_tp) Psi2*_t(n)) + r_td^T Psi2*_t(n) r_td - mean_t(n,d)^2 + 1/beta_t
    then mixture_moments over the atoms.  `train` is the model's _MaskedBoundT (an all-True mask for complete training data)."""

    def __init__(self, train, z, mu, s, gat, aat, bat, phit):
        t, p, m = train.t, train.p, z.shape[0]
        c = train.chain(z, mu, s, gat, aat, bat)
        self.info = train.info
        pm = ops.matmul(c['r0'].transpose(1, 2), c['r0'])                                          # P_tp [T P, M, M]
        r = c['be'][:, None, None] * ops.matmul(pm, train._columns(c))                             # [T P, M, Dmax]
        self.r = train.to_columns(r.reshape(t, p, m, train.dmax))                                  # [T, M, D]
        self.c = (c['kinv'] - pm).reshape(t, p, m, m).contiguous()
        pattern = torch.full((train.d,), -1, dtype=torch.long, device=train.device)
        for i, (cols, _) in enumerate(train.groups):
            pattern[torch.as_tensor(cols, device=train.device)] = i
        self.pattern = pattern                                                                     # [D]: p(d), -1 never observed
        self.z_t, self.zfac = c['z'], c['zfac']
        self.z, self.gat, self.aat, self.bat, self.phit = z, gat, aat, bat, phit

    def at(self, mu, s, cols):
        """(mean, var) [N* x len(cols)] at q(X*) = (mu, s); cols: a long tensor of output dims on the device."""
        r = self.r.index_select(2, cols).contiguous()                                              # [T, M, J]
        tr, quad = ops.qx_psi_pointwise(self.z_t, mu, s, self.gat, self.aat, self.c, r, zfac=self.zfac)
        psi_1 = ops.psi1(self.z, mu, s, self.gat, self.aat)                                        # [T, N*, M]
        mean_t = ops.matmul(psi_1, r)                                                              # [T, N*, J]
        pat = self.pattern.index_select(0, cols)
        seen = (pat >= 0).to(TORCH_DTYPE)
        tr_d = tr.index_select(2, pat.clamp(min=0)) * seen                                         # [T, N*, J]
        var_t = (self.aat + 1.0 / self.bat)[:, None, None] - tr_d + quad - mean_t * mean_t
        return mixture_moments(self.phit.index_select(1, cols), mean_t, var_t)
