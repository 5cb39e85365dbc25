"""
The collapsed bound of dp_gp_lvm_t for TRAINING data with missing entries (observed=...), and its backward pass, in fp64 on the
device.  The over-T bound is linear in phi: f_hat = sum_d sum_t phi_td F_t(y_d), F_t(y_d) the collapsed per-column bound under
atom t's kernel; under a mask column d sees only its rows R_d, so the columns of one row pattern p share Psi2_{t,p} and one
factorisation.  The model is T x P slots (t, p) of the algebra of masked_bound._MaskedBound with the real weights
D_tp = sum_{d in p} phi_td in place of the integer column count, and Y diag(sqrt(phi_t)) where Y enters quadratically.
"""
import math
import os

import numpy as np
import torch

from .. import ops
from ..utils import missing as _missing
from ..utils.constants import GP_DEFAULT_JITTER
from ..utils.types import TORCH_DTYPE


def grouped_psi_enabled():
    """DPGP_GROUPED_PSI=0: the slot form on the weighted operators with B = T P (cross-checks only); default: the
    pattern-grouped operators with K = T."""
    return os.environ.get('DPGP_GROUPED_PSI', '1') != '0'


class _MaskedBoundT:
    """Per slot (t, p), with N_p = sum_n w_pn, T_tp = L_t^-1 Psi2_tp L_t^-T, A_tp = beta_t T_tp + I = L_A L_A^T, R0 = L_A^-1 L_t^-1
    and u_d = R0 Psi1_t^T y_d (y_d zero where unobserved, so Psi1_t^T y_d runs over R_d on its own):
        F_t(d) = 1/2 N_p log beta_t + 1/2 beta_t (tr T_tp - alpha_t N_p) - log|L_A,tp| - 1/2 beta_t |y_d|^2 + 1/2 beta_t^2 |u_d|^2
        f_hat  = sum_{d observed somewhere} ( -1/2 N_p(d) log 2 pi + sum_t phi_td F_t(d) ),        d f_hat / d phi_td = F_t(d).
    Backward pass (P = R0^T R0 = (K_t + beta_t Psi2_tp)^-1, r_d = P Psi1_t^T y_d, KP = K_t^-1 Psi2_tp, RR = sum_d phi_td r_d r_d^T):
        G2_tp = 1/2 D_tp beta_t^2 sym(KP P) - 1/2 beta_t^3 RR
        GK_t  = sum_p ( -1/2 D_tp beta_t^2 sym(KP P KP^T) - 1/2 beta_t^2 RR )
        G1_t  = beta_t^2 Y diag(phi_t) R_t^T          one batched product over all columns: already summed over the patterns
    (mu, S) and (Z, gamma_t, alpha_t) through Psi by the pattern-grouped operators with K = T (ops.qx_psi_*_grouped), or by
    the weighted operators with B = T P slots (DPGP_GROUPED_PSI=0); K_uu terms through ONE ops.ard_rbf_gram_grad_batched with
    the shared Z replicated to the atoms.  Slot b = t P + p in every [T P, ...] array.  No host synchronisation."""

    def __init__(self, y0, observed, truncation_level, device):
        f64 = TORCH_DTYPE
        groups = _missing.group_columns_by_pattern(observed)
        assert groups, 'observed must hold at least one True entry'
        n, d = y0.shape
        dmax = max(len(c) for c, _ in groups)
        self.groups, self.t, self.p, self.n, self.d, self.dmax, self.device = groups, truncation_level, len(groups), n, d, dmax, device
        idx = np.zeros((self.p, dmax), dtype=np.int64)                    # column of (pattern, place); padded places: column 0
        valid = np.zeros((self.p, dmax), dtype=bool)
        for i, (cols, _) in enumerate(groups):
            idx[i, :len(cols)] = cols
            valid[i, :len(cols)] = True
        lt = lambda a: torch.as_tensor(a, dtype=torch.long, device=device)
        self.idx = lt(idx.reshape(-1))                                     # [P Dmax]
        self.valid = torch.as_tensor(valid.astype(np.float64), dtype=f64, device=device)           # [P, Dmax]
        self.places = lt(np.flatnonzero(valid.reshape(-1)))               # the places that hold a column, and their columns
        self.cols = lt(idx.reshape(-1)[valid.reshape(-1)])
        self.y = torch.as_tensor(y0, dtype=f64, device=device).contiguous()                         # [N, D], zero where unobserved
        self.yy = (torch.sum(self.y * self.y, dim=0).index_select(0, self.idx).reshape(self.p, dmax) * self.valid)   # [P, Dmax]
        self.weights = torch.as_tensor(np.stack([w for _, w in groups]), dtype=f64, device=device).contiguous()     # [P, N]
        self.n_w = torch.sum(self.weights, dim=1)                                                                   # [P]
        self.n_cols = torch.tensor([float(len(c)) for c, _ in groups], dtype=f64, device=device)
        self.ones_t = torch.ones(truncation_level, dtype=f64, device=device)
        self.grouped = grouped_psi_enabled()
        self.terms = self.info = None

    # ---- between the [T, D] column layout and the [T, P, Dmax] slot layout
    def to_slots(self, a):
        """[T, X, D] -> [T, P, X, Dmax] (zero at the padded places)."""
        t, x = a.shape[0], a.shape[1]
        g = a.index_select(2, self.idx).reshape(t, x, self.p, self.dmax) * self.valid
        return g.permute(0, 2, 1, 3).contiguous()

    def to_columns(self, a):
        """[T, P, X, Dmax] -> [T, X, D] (zero at the columns never observed)."""
        t, x = a.shape[0], a.shape[2]
        flat = a.permute(0, 2, 1, 3).reshape(t, x, self.p * self.dmax).index_select(2, self.places)
        return torch.zeros((t, x, self.d), dtype=a.dtype, device=a.device).index_copy_(2, self.cols, flat)

    def _rep(self, a):
        """[T, ...] -> [T P, ...]: atom t's array at its P slots."""
        return a.repeat_interleave(self.p, dim=0).contiguous()

    def chain(self, z, mu, s, gat, aat, bat):
        """Everything up to the factor of A_tp (shared by evaluate and the imputation)."""
        t, p, m = self.t, self.p, z.shape[0]
        k_uu = ops.ard_rbf_gram(z, None, gat, aat, self.ones_t, include_noise=False, include_jitter=True, jitter=GP_DEFAULT_JITTER)
        l_uu, info_uu = ops.potrf_batched(k_uu)
        li = ops.tril_inverse_batched(l_uu)
        kinv = ops.matmul(li.transpose(1, 2), li)
        zfac = ops.ard_rbf_gram(z, None, 0.5 * gat, aat * aat, self.ones_t)
        c = dict(z=z[None].expand(t, *z.shape).contiguous(), zfac=zfac, li=self._rep(li), kinv=self._rep(kinv), be=self._rep(bat),
                 al=self._rep(aat))
        if self.grouped:
            c['psi_1'], psi_2 = ops.qx_psi_stats_grouped(c['z'], mu, s, gat, aat, self.weights, zfac=zfac)
            c['psi_2'] = psi_2.reshape(t * p, m, m)
        else:
            c['slot'] = (self._rep(c['z']), self._rep(gat), self._rep(aat), self._rep(zfac), self.weights.repeat(t, 1).contiguous())
            zs, gs, als, zfs, ws = c['slot']
            psi_1, c['psi_2'] = ops.qx_psi_stats_batched(zs, mu, s, gs, als, zfs, weights=ws)
            c['psi_1'] = psi_1.reshape(t, p, self.n, m)[:, 0].contiguous()
        c['tm'] = ops.matmul(ops.matmul(c['li'], c['psi_2']), c['li'].transpose(1, 2))
        eye = torch.eye(m, dtype=TORCH_DTYPE, device=self.device)
        c['l_a'], info_a = ops.potrf_batched(c['be'][:, None, None] * c['tm'] + eye)
        c['r0'] = ops.matmul(ops.tril_inverse_batched(c['l_a']), c['li'])
        self.info = torch.maximum(info_uu.abs().max(), info_a.abs().max())
        return c

    def _columns(self, c):
        """V_s [T P, M, Dmax] = Psi1_t^T y_d at the slots' places, from one batched product over all columns."""
        v = ops.matmul(c['psi_1'].transpose(1, 2), self.y)                                        # [T, M, D]
        return self.to_slots(v).reshape(self.t * self.p, -1, self.dmax)

    def evaluate(self, z, mu, s, gat, aat, bat, phit, grad=False):
        """f_hat (0-d); with grad also a dict of d f_hat / d (mu, s, z, gamma [T,Q], alpha [T], beta [T], phit [T,D]) (the values,
        not the raw variables).  self.info: 0 when every K_uu,t and every A_tp factorised."""
        t, p, dmax, n_w = self.t, self.p, self.dmax, self.n_w
        c = self.chain(z, mu, s, gat, aat, bat)
        be, al = c['be'], c['al']                                                                  # [T P]
        psi_2, tm, r0 = c['psi_2'], c['tm'], c['r0']
        phis = self.to_slots(phit[:, None, :]).reshape(t * p, dmax)                                # phi_td at the slots' places
        dd = torch.sum(phis, dim=1)                                                                # D_tp
        nw = n_w.repeat(t)
        u = ops.matmul(r0, self._columns(c))                                                       # [T P, M, Dmax]
        logdet = torch.sum(torch.log(torch.diagonal(c['l_a'], dim1=-2, dim2=-1)), dim=-1)
        tr = torch.diagonal(tm, dim1=-2, dim2=-1).sum(-1)
        uu = torch.sum(u * u, dim=1)                                                               # [T P, Dmax]
        yy = self.yy.repeat(t, 1)
        per = 0.5 * nw * torch.log(be) + 0.5 * be * (tr - al * nw) - logdet                        # [T P]
        fm = (per[:, None] - 0.5 * be[:, None] * yy + 0.5 * (be * be)[:, None] * uu) * self.valid.repeat(t, 1)   # F_t(d)
        f = torch.sum(phis * fm) - 0.5 * math.log(2.0 * math.pi) * torch.sum(n_w * self.n_cols)
        self.terms = fm
        if not grad:
            return f
        sym = lambda a: 0.5 * (a + a.transpose(1, 2))
        d3, b3 = dd[:, None, None], be[:, None, None]
        r = ops.matmul(r0.transpose(1, 2), u)                                                      # [T P, M, Dmax]
        rphi = r * phis[:, None, :]
        pm = ops.matmul(r0.transpose(1, 2), r0)
        rrt = ops.matmul(rphi, r.transpose(1, 2))
        kp = ops.matmul(c['kinv'], psi_2)                                                          # K_t^-1 Psi2_tp
        kpp = ops.matmul(kp, pm)
        g2 = (0.5 * b3 * b3) * d3 * sym(kpp) - (0.5 * b3 ** 3) * rrt
        m = z.shape[0]
        gk = ((-0.5 * b3 * b3) * d3 * sym(ops.matmul(kpp, kp.transpose(1, 2))) - (0.5 * b3 * b3) * rrt).reshape(t, p, m, m).sum(dim=1)
        r_all = self.to_columns(rphi.reshape(t, p, m, dmax))                                       # [T, M, D]: phi_td r_d
        g1 = (bat * bat)[:, None, None] * ops.matmul(self.y, r_all.transpose(1, 2))               # [T, N, M]
        if self.grouped:
            args = (c['z'], mu, s, gat, aat, g1, g2.reshape(t, p, m, m), self.weights)
            d_mu, d_s = ops.qx_psi_adjoint_grouped(*args, zfac=c['zfac'])
            dz_t, dg_t, da_t = ops.qx_psi_param_adjoint_grouped(*args, zfac=c['zfac'])
        else:
            zs, gs, als, zfs, ws = c['slot']
            g1s = torch.zeros((t, p, self.n, m), dtype=TORCH_DTYPE, device=self.device)
            g1s[:, 0] = g1                                                                         # (g1 rides in a kernel's first slot)
            args = (zs, mu, s, gs, als, g1s.reshape(t * p, self.n, m), g2, zfs)
            d_mu, d_s = ops.qx_psi_adjoint(*args, weights=ws)
            per_t = lambda a: a.reshape((t, p) + tuple(a.shape[1:])).sum(dim=1)
            dz_t, dg_t, da_t = (per_t(a) for a in ops.qx_psi_param_adjoint(*args, weights=ws))
        rk, sx, sq = ops.ard_rbf_gram_grad_batched(c['z'], gat, aat, gk)                           # [T,M], [T,M,Q], [T,M,Q]
        per_t = lambda a: a.reshape(t, p).sum(dim=1)
        uuphi, yyphi = torch.sum(phis * uu, dim=1), torch.sum(phis * yy, dim=1)
        d_z = torch.sum(dz_t - 2.0 * gat[:, None, :] * sx, dim=0)
        d_gamma = dg_t - 0.5 * torch.sum(sq, dim=1)
        d_alpha = da_t.reshape(-1) + torch.sum(rk, dim=1) / aat - 0.5 * bat * per_t(dd * nw)
        d_beta = per_t(0.5 * nw * dd / be - 0.5 * dd * torch.sum(pm * psi_2, dim=(1, 2)) + 0.5 * dd * (tr - al * nw)
                       + be * uuphi - (0.5 * be * be) * torch.sum(rrt * psi_2, dim=(1, 2)) - 0.5 * yyphi)
        d_phit = self.to_columns(fm.reshape(t, p, 1, dmax))[:, 0, :]
        return f, dict(mu=d_mu, s=d_s, z=d_z, gamma=d_gamma, alpha=d_alpha, beta=d_beta, phit=d_phit)

    def posterior_means(self, z, mu, s, gat, aat, bat, phit):
        """[N, D]: sum_t phi_td beta_t Psi1_t (K_t + beta_t Psi2_{t,p(d)})^-1 Psi1_t^T y_d at every row (Psi1 is not weighted); 0
        for a column never observed."""
        t, p, m = self.t, self.p, z.shape[0]
        c = self.chain(z, mu, s, gat, aat, bat)
        phis = self.to_slots(phit[:, None, :]).reshape(t * p, self.dmax)
        pm = ops.matmul(c['r0'].transpose(1, 2), c['r0'])
        r = ops.matmul(pm, self._columns(c)) * phis[:, None, :]
        r_all = self.to_columns(r.reshape(t, p, m, self.dmax)) * bat[:, None, None]
        return torch.sum(ops.matmul(c['psi_1'], r_all), dim=0)
