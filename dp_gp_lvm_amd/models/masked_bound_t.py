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
from ..utils.types import TORCH_DTYPE
from . import collapsed


def grouped_psi_enabled():
    """DPGP_GROUPED_PSI=0: the slot form on the weighted operators with B = T P (cross-checks only); default: the
    pattern-grouped operators with K = T."""
    return os.environ.get('DPGP_GROUPED_PSI', '1') != '0'


class _PatternLayout:
    """The row patterns of a mask [N x D] and the moves between the [T, D] column layout and the [T, P, Dmax] slot layout:
    groups (columns, row weights) per pattern, idx / valid [P, Dmax] the column of each (pattern, place) and whether it holds
    one, places / cols the places that hold a column and their columns, y [N, D] zero where unobserved, yy = |y_d|^2 at the
    places, weights [P, N], n_w = N_p, n_cols the patterns' column counts.  Slot b = t P + p in every [T P, ...] array."""

    def __init__(self, y0, observed, device):
        f64 = TORCH_DTYPE
        groups = _missing.group_columns_by_pattern(observed)
        assert groups, 'observed must hold at least one True entry'
        n, d = y0.shape
        dmax = max(len(c) for c, _ in groups)
        self.groups, self.p, self.n, self.d, self.dmax, self.device = groups, len(groups), n, d, dmax, device
        idx = np.zeros((self.p, dmax), dtype=np.int64)                    # column of (pattern, place); padded places: column 0
        valid = np.zeros((self.p, dmax), dtype=bool)
        for i, (cols, _) in enumerate(groups):
            idx[i, :len(cols)] = cols
            valid[i, :len(cols)] = True
        lt = lambda a: torch.as_tensor(a, dtype=torch.long, device=device)
        self.idx = lt(idx.reshape(-1))                                     # [P Dmax]
        self.valid = torch.as_tensor(valid.astype(np.float64), dtype=f64, device=device)           # [P, Dmax]
        self.places = lt(np.flatnonzero(valid.reshape(-1)))
        self.cols = lt(idx.reshape(-1)[valid.reshape(-1)])
        self.y = torch.as_tensor(y0, dtype=f64, device=device).contiguous()                         # [N, D], zero where unobserved
        self.yy = (torch.sum(self.y * self.y, dim=0).index_select(0, self.idx).reshape(self.p, dmax) * self.valid)   # [P, Dmax]
        self.weights = torch.as_tensor(np.stack([w for _, w in groups]), dtype=f64, device=device).contiguous()     # [P, N]
        self.n_w = torch.sum(self.weights, dim=1)                                                                   # [P]
        self.n_cols = torch.tensor([float(len(c)) for c, _ in groups], dtype=f64, device=device)

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

    def rep(self, a):
        """[T, ...] -> [T P, ...]: atom t's array at its P slots."""
        return a.repeat_interleave(self.p, dim=0).contiguous()

    def phi_slots(self, phit):
        """phit [T, D] -> phi_td at the slots' places [T P, Dmax]."""
        return self.to_slots(phit[:, None, :]).reshape(-1, self.dmax)

    def psi1T_y(self, psi_1):
        """V_s [T P, M, Dmax] = Psi1_t^T y_d at the slots' places, from one batched product over all columns (psi_1 [T, N, M])."""
        v = ops.matmul(psi_1.transpose(1, 2), self.y)                                             # [T, M, D]
        return self.to_slots(v).reshape(-1, v.shape[1], self.dmax)

    def g1(self, rphi, bat):
        """G1_t [T, N, M] = beta_t^2 Y diag(phi_t) R_t^T from phi_td r_d at the slots' places, rphi [T P, M, Dmax]."""
        r_all = self.to_columns(rphi.reshape(bat.shape[0], self.p, -1, self.dmax))                 # [T, M, D]: phi_td r_d
        return (bat * bat)[:, None, None] * ops.matmul(self.y, r_all.transpose(1, 2))


def slot_column_values(ch, al, nw, yy, uu, valid):
    """F_t(d) at the slots' places [T P, Dmax] from the projected chain of the T P slots; al, nw [T P] and yy, uu, valid
    [T P, Dmax] at the slots."""
    be = ch.beta
    per = 0.5 * nw * torch.log(be) + 0.5 * be * (ch.tr - al * nw) - ch.logdet                      # [T P]
    return (per[:, None] - 0.5 * be[:, None] * yy + 0.5 * (be * be)[:, None] * uu) * valid


class _MaskedBoundT:
    """T P slots (t, p) of models/collapsed.py on a _PatternLayout, with D = D_tp = sum_{d in p} phi_td, N_w = N_p and phi the
    slot's phi_td: with u_d = R0 Psi1_t^T y_d (y_d zero where unobserved, so Psi1_t^T y_d runs over R_d on its own)
        F_t(d) = 1/2 N_p log beta_t + 1/2 beta_t (tr T_tp - alpha_t N_p) - log|L_A,tp| - 1/2 beta_t |y_d|^2 + 1/2 beta_t^2 |u_d|^2
        f_hat  = sum_{d observed somewhere} ( -1/2 N_p(d) log 2 pi + sum_t phi_td F_t(d) ),        d f_hat / d phi_td = F_t(d).
    |u_d|^2 is reduced over M per column and then phi-weighted.  Backward pass: G2_tp in the product form,
        GK_t  = sum_p GK_tp,      G1_t  = beta_t^2 Y diag(phi_t) R_t^T    one batched product over all columns: already summed
    over the patterns; (mu, S) and (Z, gamma_t, alpha_t) through Psi by the pattern-grouped operators with K = T
    (ops.qx_psi_*_grouped), or by the weighted operators with B = T P slots (DPGP_GROUPED_PSI=0); K_uu terms through ONE
    ops.ard_rbf_gram_grad_batched with the shared Z replicated to the atoms.  No host synchronisation."""

    def __init__(self, y0, observed, truncation_level, device):
        self.layout = _PatternLayout(y0, observed, device)
        self.groups, self.t, self.device = self.layout.groups, truncation_level, device
        self.grouped = grouped_psi_enabled()
        self.terms = self.info = None

    def chain(self, z, mu, s, gat, aat, bat):
        """Everything up to the factor of A_tp (shared by evaluate, the imputation and _MomentsT)."""
        lay, t, m = self.layout, self.t, z.shape[0]
        li, kinv, info_uu, zfac = collapsed.shared_z_kernels(z, gat, aat)
        c = dict(z=z[None].expand(t, *z.shape).contiguous(), zfac=zfac, kinv=lay.rep(kinv), al=lay.rep(aat))
        if self.grouped:
            c['psi_1'], psi_2 = ops.qx_psi_stats_grouped(c['z'], mu, s, gat, aat, lay.weights, zfac=zfac)
            psi_2 = psi_2.reshape(t * lay.p, m, m)
        else:
            c['slot'] = (lay.rep(c['z']), lay.rep(gat), lay.rep(aat), lay.rep(zfac), lay.weights.repeat(t, 1).contiguous())
            zs, gs, als, zfs, ws = c['slot']
            psi_1, psi_2 = ops.qx_psi_stats_batched(zs, mu, s, gs, als, zfs, weights=ws)
            c['psi_1'] = psi_1.reshape(t, lay.p, lay.n, m)[:, 0].contiguous()
        c['chain'] = collapsed.Chain(lay.rep(li), psi_2, lay.rep(bat))
        self.info = torch.maximum(info_uu.abs().max(), c['chain'].info.abs().max())
        return c

    def evaluate(self, z, mu, s, gat, aat, bat, phit, grad=False):
        """f_hat (0-d); with grad also a dict of d f_hat / d (mu, s, z, gamma [T,Q], alpha [T], beta [T], phit [T,D]) (the values,
        not the raw variables).  self.terms: F_t(d) [T P, Dmax]; self.info: 0 when every K_uu,t and every A_tp factorised."""
        lay, t, m = self.layout, self.t, z.shape[0]
        p, dmax, n_w = lay.p, lay.dmax, lay.n_w
        c = self.chain(z, mu, s, gat, aat, bat)
        al, phis, nw, yy = c['al'], lay.phi_slots(phit), n_w.repeat(t), lay.yy.repeat(t, 1)
        ch = c['chain'].project(lay.psi1T_y(c['psi_1']))                                           # u [T P, M, Dmax]
        be = ch.beta                                                                               # [T P]
        uu = torch.sum(ch.u * ch.u, dim=1)                                                         # [T P, Dmax]
        fm = slot_column_values(ch, al, nw, yy, uu, lay.valid.repeat(t, 1))
        f = torch.sum(phis * fm) - 0.5 * math.log(2.0 * math.pi) * torch.sum(n_w * lay.n_cols)
        self.terms = fm
        if not grad:
            return f
        dd = torch.sum(phis, dim=1)                                                                # D_tp
        adj = collapsed.Adjoint(ch, dd, phis)
        g2 = adj.g2_product(c['kinv'])
        gk = adj.gk().reshape(t, p, m, m).sum(dim=1)
        g1 = lay.g1(adj.rphi, bat)                                                                 # [T, N, M]
        if self.grouped:
            args = (c['z'], mu, s, gat, aat, g1, g2.reshape(t, p, m, m), lay.weights)
            d_mu, d_s = ops.qx_psi_adjoint_grouped(*args, zfac=c['zfac'])
            dz_t, dg_t, da_t = ops.qx_psi_param_adjoint_grouped(*args, zfac=c['zfac'])
        else:
            zs, gs, als, zfs, ws = c['slot']
            g1s = torch.zeros((t, p, lay.n, m), dtype=TORCH_DTYPE, device=self.device)
            g1s[:, 0] = g1                                                                         # (g1 rides in a kernel's first slot)
            args = (zs, mu, s, gs, als, g1s.reshape(t * p, lay.n, m), g2, zfs)
            d_mu, d_s = ops.qx_psi_adjoint(*args, weights=ws)
            per_t = lambda a: a.reshape((t, p) + tuple(a.shape[1:])).sum(dim=1)
            dz_t, dg_t, da_t = (per_t(a) for a in ops.qx_psi_param_adjoint(*args, weights=ws))
        rk, sx, sq = ops.ard_rbf_gram_grad_batched(c['z'], gat, aat, gk)                           # [T,M], [T,M,Q], [T,M,Q]
        per_t = lambda a: a.reshape(t, p).sum(dim=1)
        d_z = torch.sum(dz_t - 2.0 * gat[:, None, :] * sx, dim=0)
        d_gamma = dg_t - 0.5 * torch.sum(sq, dim=1)
        d_alpha = da_t.reshape(-1) + torch.sum(rk, dim=1) / aat - 0.5 * bat * per_t(dd * nw)
        d_beta = per_t(adj.d_beta(nw, al, torch.sum(phis * uu, dim=1), torch.sum(phis * yy, dim=1)))
        d_phit = lay.to_columns(fm.reshape(t, p, 1, dmax))[:, 0, :]
        return f, dict(mu=d_mu, s=d_s, z=d_z, gamma=d_gamma, alpha=d_alpha, beta=d_beta, phit=d_phit)

    def posterior_means(self, z, mu, s, gat, aat, bat, phit):
        """[N, D]: sum_t phi_td beta_t Psi1_t (K_t + beta_t Psi2_{t,p(d)})^-1 Psi1_t^T y_d at every row (Psi1 is not weighted); 0
        for a column never observed."""
        lay, t, m = self.layout, self.t, z.shape[0]
        c = self.chain(z, mu, s, gat, aat, bat)
        phis = lay.phi_slots(phit)
        pm = collapsed.precision(c['chain'].r0)
        r = ops.matmul(pm, lay.psi1T_y(c['psi_1'])) * phis[:, None, :]
        r_all = lay.to_columns(r.reshape(t, lay.p, m, lay.dmax)) * bat[:, None, None]
        return torch.sum(ops.matmul(c['psi_1'], r_all), dim=0)
