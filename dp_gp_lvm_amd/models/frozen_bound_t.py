"""
The frozen test bound of dp_gp_lvm_t and the mixture's predictive moments: the over-T model's prediction paths, in fp64 on the
device.  The bound is the forward pass of masked_bound_t._MaskedBoundT on (y*, observed*) with everything trained held fixed, so
only q(X*) moves; the moments come from the per-point Psi2 contractions of ops.qx_psi_pointwise.
"""
import math

import numpy as np
import torch

from .. import ops
from ..utils.types import TORCH_DTYPE
from . import collapsed
from .marginals import _Marginals
from .masked_bound_t import _PatternLayout, slot_column_values


def mixture_moments(phit, mean_t, var_t):
    """Mean and variance [N, J] of the mixture sum_t phi_td N(mean_t(n,d), var_t(n,d)) per entry: phit [T, J] (columns sum to 1),
    mean_t, var_t [T, N, J].  mean = sum_t phi mean_t, var = sum_t phi (var_t + mean_t^2) - mean^2 (pure torch, any device)."""
    w = phit[:, None, :]
    mean = torch.sum(w * mean_t, dim=0)
    return mean, torch.sum(w * (var_t + mean_t * mean_t), dim=0) - mean * mean


class _TestBoundT:
    """f_hat* = sum_{d observed somewhere} ( -1/2 N_p(d) log 2 pi + sum_t phi_td F_t(y*_d on its rows) ), the symbols of
    _MaskedBoundT, with z [M,Q], the atoms (gamma [T,Q], alpha [T], beta [T]) and phit [T,D] frozen.
    Once per object: K_t, its factor, L_t^-1, K_t^-1, the pair factor zfac, the _PatternLayout of observed* (P test patterns;
    P = 1 for complete test data), phi and |y*_d|^2 at the slots' places.
    Per evaluation: one ops.qx_psi_stats_grouped (K = T), the T P factorisations of A_tp, and with grad=True G2_tp in the product
    form and G1_t through one ops.qx_psi_adjoint_grouped for (d_mu, d_s) only: no parameter adjoint, no gram gradient, no host
    synchronisation.  The grouped operators are used whatever DPGP_GROUPED_PSI says (that switch is a training cross-check).
    self.terms: F_t(d) [T P, Dmax]; self.info: 0 when every K_t and every A_tp factorised."""

    def __init__(self, z, gat, aat, bat, phit, y0, observed, device):
        lay = self.layout = _PatternLayout(y0, observed, device)
        t = self.t = gat.shape[0]
        put = lambda a: a.detach().to(device=device, dtype=TORCH_DTYPE).contiguous()
        z, gat, aat, bat, phit = put(z), put(gat), put(aat).reshape(-1), put(bat).reshape(-1), put(phit)
        assert tuple(phit.shape) == (t, lay.d), 'phit must be [T x D]'
        self.m = z.shape[0]
        self.gat, self.aat, self.bat = gat, aat, bat
        li, kinv, info_uu, self.zfac = collapsed.shared_z_kernels(z, gat, aat)
        self.info_uu = info_uu.abs().max()
        self.z_t = z[None].expand(t, *z.shape).contiguous()
        self.li, self.kinv, self.be, self.al = lay.rep(li), lay.rep(kinv), lay.rep(bat), lay.rep(aat)
        self.phis = lay.phi_slots(phit)                                                            # phi_td at the slots' places
        self.dd = torch.sum(self.phis, dim=1)                                                      # D_tp
        self.nw = lay.n_w.repeat(t)
        self.yy_s, self.valid_s = lay.yy.repeat(t, 1), lay.valid.repeat(t, 1)
        self.const = -0.5 * math.log(2.0 * math.pi) * torch.sum(lay.n_w * lay.n_cols)
        self.eye = torch.eye(self.m, dtype=TORCH_DTYPE, device=device)
        self.terms = self.info = None

    def evaluate(self, mu, s, grad=False):
        """(f_hat* (0-d), d f_hat* / d mu, d f_hat* / d s); the derivatives are None without grad."""
        lay, t, m = self.layout, self.t, self.m
        psi_1, psi_2 = ops.qx_psi_stats_grouped(self.z_t, mu, s, self.gat, self.aat, lay.weights, zfac=self.zfac)
        ch = collapsed.Chain(self.li, psi_2.reshape(t * lay.p, m, m), self.be, self.eye)
        self.info = torch.maximum(self.info_uu, ch.info.abs().max())
        ch.project(lay.psi1T_y(psi_1))                                                             # u [T P, M, Dmax]
        uu = torch.sum(ch.u * ch.u, dim=1)
        fm = slot_column_values(ch, self.al, self.nw, self.yy_s, uu, self.valid_s)
        f = torch.sum(self.phis * fm) + self.const
        self.terms = fm
        if not grad:
            return f, None, None
        adj = collapsed.Adjoint(ch, self.dd, self.phis)
        g2 = adj.g2_product(self.kinv)
        d_mu, d_s = ops.qx_psi_adjoint_grouped(self.z_t, mu, s, self.gat, self.aat, lay.g1(adj.rphi, self.bat),
                                               g2.reshape(t, lay.p, m, m), lay.weights, zfac=self.zfac)
        return f, d_mu, d_s


class _MomentsT:
    """The training side of the over-T model's predictive moments, formed once: with p the training row pattern of column d,
    P_tp = (K_t + beta_t Psi2_tp)^-1 and r_td = beta_t P_tp Psi1_t^T y_d (0 for a column never observed in training),
        mean_t(n,d) = psi1*_t(n) . r_td
        var_t(n,d)  = alpha_t - tr((K_t^-1 - P_tp) Psi2*_t(n)) + r_td^T Psi2*_t(n) r_td - mean_t(n,d)^2 + 1/beta_t
    then mixture_moments over the atoms.  `train` is the model's _MaskedBoundT (an all-True mask for complete training data)."""

    def __init__(self, train, z, mu, s, gat, aat, bat, phit):
        lay, t, m = train.layout, train.t, z.shape[0]
        c = train.chain(z, mu, s, gat, aat, bat)
        self.info = train.info
        r, cm = collapsed.posterior(c['chain'].r0, c['kinv'], c['chain'].beta, lay.psi1T_y(c['psi_1']))     # per slot [T P, ...]
        self.r = lay.to_columns(r.reshape(t, lay.p, m, lay.dmax))                                  # [T, M, D]
        self.c = cm.reshape(t, lay.p, m, m).contiguous()
        pattern = torch.full((lay.d,), -1, dtype=torch.long, device=train.device)
        self.pattern_host = np.full(lay.d, -1, dtype=np.int64)
        for i, (cols, _) in enumerate(lay.groups):
            pattern[torch.as_tensor(cols, device=train.device)] = i
            self.pattern_host[np.asarray(cols, dtype=np.int64)] = i
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

    def _atoms(self):
        """The T atoms as the kernels of a marginals._Marginals: every atom sees all D columns, column d on its pattern p(d)."""
        gidx = self.pattern.to(torch.int32)[None].expand(self.r.shape[0], -1)
        return _Marginals(self.z_t, self.gat, self.aat, self.bat, self.zfac, self.c, self.r, gidx,
                          gidx_host=np.broadcast_to(self.pattern_host, (self.r.shape[0], self.pattern_host.size)))

    def covariance(self, x, cols, noise=False):
        """[len(cols) x N* x N*]: the covariance of the mixture over the atoms of the columns' functions at the deterministic
        latent points x,
            sum_t phi_td (cov_t,p(d) + m_td m_td^T) - m_d m_d^T,     m_td = k_t(x)^T r_td [N*],   m_d = sum_t phi_td m_td
        cov_t,p the joint posterior covariance under atom t and pattern p (marginals._Marginals.covariance on the T atoms: one
        call of ops.ard_rbf_point_cov), with 1/beta_t on its diagonal when `noise`: mixture_moments' variance on the diagonal."""
        atoms = self._atoms()
        cov_t = atoms.covariance(x, cols)                                                          # [T, J, N*, N*]
        if noise:
            cov_t = cov_t + (1.0 / self.bat).reshape(-1, 1, 1, 1) * torch.eye(x.shape[0], dtype=TORCH_DTYPE, device=x.device)
        mean_t = atoms.at(x, torch.zeros_like(x), cols)[0].transpose(1, 2)                         # [T, J, N*]
        phi = self.phit.index_select(1, cols)                                                      # [T, J]
        mean = torch.sum(phi[:, :, None] * mean_t, dim=0)                                          # [J, N*]
        second = cov_t + mean_t[:, :, :, None] * mean_t[:, :, None, :]
        return torch.sum(phi[:, :, None, None] * second, dim=0) - mean[:, :, None] * mean[:, None, :]

    def sample(self, x, xi, cols, atoms, noise, jitter):
        """(f [S x N* x J], info): f[s, :, j] = m_tj + L_t,p(j) xi[s, :, j] with t = atoms[s, j] [S x J] (long), the atom of
        (sample, column).  The draws of every atom come from ONE marginals._Marginals.sample on the T atoms (one potrf_batched
        over the (atom, pattern) pairs, one matmul); a gather keeps each (sample, column)'s own atom."""
        f_t, info = self._atoms().sample(x, xi, cols, noise, jitter)                               # [T, S, N*, J]
        s, n, j = f_t.shape[1], f_t.shape[2], f_t.shape[3]
        return torch.gather(f_t, 0, atoms[None, :, None, :].expand(1, s, n, j))[0], info

    def jacobian(self, x, cols):
        """[N* x len(cols) x Q]: the mean of the mixture's Jacobian rows at the deterministic latent points x,
        sum_t phi_td b_t(x)^T r_td (ops.ard_rbf_point_jacobian on the T atoms)."""
        jac_t = self._atoms().jacobian(x, cols)                                                    # [T, N*, J, Q]
        return torch.sum(self.phit.index_select(1, cols)[:, None, :, None] * jac_t, dim=0)

    def metric(self, x, cols):
        """[N* x Q x Q]: the expected metric over the columns `cols`, the second moment of the mixture over the atoms as
        mixture_moments takes it for the variance: sum_t ( n_t alpha_t diag(gamma_t) + b_t^T P_t b_t ), n_t = sum_d phi_td,
        P_t = sum_d phi_td (r_td r_td^T - C_t,p(d))  (marginals._Marginals.metric_total with phi as the columns' weights)."""
        return self._atoms().metric_total(x, cols, weights=self.phit)

    def metric_part(self, cols):
        """(atoms, P [T, M, M], prior [T, Q, Q]): the part of a marginals.Metric under metric's G over the columns `cols`, the T
        atoms with marginals._Marginals._metric_operands' pair, phi as the columns' weights; formed once per call."""
        atoms = self._atoms()
        return (atoms,) + atoms._metric_operands(cols, self.phit)
