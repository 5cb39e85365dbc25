"""
The collapsed bound of bayesian_gp_lvm for TRAINING data with missing entries (observed=...), and its whole backward pass, in
fp64 on the device.  With a boolean mask [N x D] the bound is a sum over output dims, dim d seeing only the rows R_d at which
it was measured; columns that share one row pattern share a "slot" b (D_b columns, 0 / 1 row weights w_b, N_b = sum_n w_b[n]),
and all slots share the one kernel (Z, gamma, alpha, beta).  The forward pass is the sum _TestBound.slots(...).evaluate computes
(frozen_bound.py), evaluated at the training q(X); here Z and the hyper-parameters move, so K_uu and its factors are formed per
evaluation and the bound is also differentiated with respect to them.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from ..utils import missing as _missing
from ..utils.types import TORCH_DTYPE
from . import collapsed


class _SlotBound:
    """What _MaskedBound and _MaskedViewsBound share: B slots (column groups of one row pattern) as ONE batch of the weighted
    operators.  slots: a list of (columns' data [N, D_b], row weights w_b [N]).  Per slot, in the symbols of models/collapsed.py
    (D = D_b the slot's column count, N_w = N_b = sum_n w_b[n], no phi):
        terms[b] = 1/2 N_b D_b (log beta - log 2 pi), -D_b log|L_A|, 1/2 D_b beta (tr T_b - alpha N_b), 1/2 beta^2 |U|^2, -1/2 beta |Y_b|^2
    Psi2_b the weighted sum over the rows of slot b (ops.qx_psi_stats_batched(weights=)), Y_b zero where unobserved; G2 in the
    product form and G1_b = beta^2 Y_b R^T go to ops.qx_psi_adjoint(weights=) for (mu, S) and to ops.qx_psi_param_adjoint for the
    Psi part of (Z, gamma, alpha), per slot.  A subclass forms the kernels of the slots (chain) and adds the slots' parameter
    adjoints and GK_b within their kernel (evaluate).  No host synchronisation."""

    def __init__(self, slots, device):
        f64 = TORCH_DTYPE
        n, dmax = slots[0][0].shape[0], max(y.shape[1] for y, _ in slots)
        y = np.zeros((len(slots), n, dmax))
        for i, (ys, _) in enumerate(slots):
            y[i, :, :ys.shape[1]] = ys
        self.b, self.n, self.device = len(slots), n, device
        self.y = torch.as_tensor(y, dtype=f64, device=device).contiguous()                           # [B, N, Dmax]
        self.yy = torch.sum(self.y * self.y, dim=(1, 2))
        self.dims = torch.tensor([float(ys.shape[1]) for ys, _ in slots], dtype=f64, device=device)
        self.weights = torch.as_tensor(np.stack([w for _, w in slots]), dtype=f64, device=device).contiguous()
        self.n_w = torch.sum(self.weights, dim=1)
        self.terms = self.info = None

    def _chain(self, c, mu, s, info_uu):
        """c: the kernels gathered to the slots (z, gamma, alpha, beta, zfac, li, kinv); adds the statistics and the factors of
        A_b (psi_1, psi_2, chain, and tm, l_a, r0 of it: what marginals.py reads)."""
        c['psi_1'], c['psi_2'] = ops.qx_psi_stats_batched(c['z'], mu, s, c['gamma'], c['alpha'], c['zfac'], weights=self.weights)
        ch = c['chain'] = collapsed.Chain(c['li'], c['psi_2'], c['beta'])
        c['tm'], c['l_a'], c['r0'] = ch.tm, ch.l_a, ch.r0
        self.info = torch.maximum(info_uu.abs().max(), ch.info.abs().max())
        return c

    def _forward(self, c):
        """f, the projected chain and |U|^2 per slot; sets self.terms [B x 5]."""
        be, al, dd, n_w = c['beta'], c['alpha'], self.dims, self.n_w
        ch = c['chain'].project(ops.matmul(c['psi_1'].transpose(1, 2), self.y))                  # u [B, M, Dmax]
        uu = torch.sum(ch.u * ch.u, dim=(1, 2))
        self.terms = torch.stack([0.5 * n_w * dd * (torch.log(be) - math.log(2.0 * math.pi)), -dd * ch.logdet,
                                  0.5 * dd * be * (ch.tr - al * n_w), 0.5 * be * be * uu, -0.5 * be * self.yy], dim=1)
        return torch.sum(self.terms), ch, uu

    def _backward(self, c, ch, uu, mu, s):
        """(d_mu, d_s, the per-slot (d_z, d_gamma, d_alpha) through Psi, GK_b [B,M,M], the beta summand [B])."""
        adj = collapsed.Adjoint(ch, self.dims)
        g2 = adj.g2_product(c['kinv'])
        g1 = (adj.b3 * adj.b3) * ops.matmul(self.y, adj.r.transpose(1, 2))                       # [B, N, M]
        gk = adj.gk()
        args = (c['z'], mu, s, c['gamma'], c['alpha'], g1, g2, c['zfac'])
        d_mu, d_s = ops.qx_psi_adjoint(*args, weights=self.weights)
        return d_mu, d_s, ops.qx_psi_param_adjoint(*args, weights=self.weights), gk, adj.d_beta(self.n_w, c['alpha'], uu, self.yy)

    def posterior_means(self, z, mu, s, gamma, alpha, beta):
        """[B, N, Dmax]: beta Psi1 (K_uu + beta Psi2_b)^-1 Psi1^T Y_b at every row, per slot, with the slot's kernel (Psi1 is not
        weighted)."""
        c = self.chain(z, mu, s, gamma, alpha, beta)
        v = ops.matmul(c['psi_1'].transpose(1, 2), self.y)
        return c['chain'].beta[:, None, None] * ops.matmul(c['psi_1'], ops.matmul(collapsed.precision(c['r0']), v))


class _MaskedBound(_SlotBound):
    """f = sum_b f_b over the column groups of ONE kernel (z [M,Q], gamma, alpha, beta): K_uu, its factors and the pair factor
    are formed once and expanded to the slots; the slots' (Z, gamma, alpha, beta) adjoints are added with torch.sum, the K_uu
    term is ONE ops.ard_rbf_gram_grad with GK = sum_b GK_b; alpha's explicit part is -1/2 beta sum_b D_b N_b."""

    def __init__(self, y0, observed, device):
        self.groups = _missing.group_columns_by_pattern(observed)
        assert self.groups, 'observed must hold at least one True entry'
        super().__init__([(y0[:, cols], w) for cols, w in self.groups], device)

    def chain(self, z, mu, s, gamma, alpha, beta):
        """Everything up to the factor of A_b (shared by evaluate, the imputation and marginals.py)."""
        gamma, alpha = gamma.reshape(1, -1), alpha.reshape(1)
        li, kinv, info_uu, zfac = collapsed.shared_z_kernels(z, gamma, alpha)
        rep = lambda t: t.expand(self.b, *t.shape[1:]).contiguous()
        c = dict(z=rep(z[None]), gamma=rep(gamma), alpha=rep(alpha), zfac=rep(zfac), li=rep(li), kinv=rep(kinv), beta=beta.reshape(1))
        return self._chain(c, mu, s, info_uu)

    def evaluate(self, z, mu, s, gamma, alpha, beta, grad=False):
        """f (0-d); with grad also a dict of df/d(mu, s, z, gamma [Q], alpha, beta) (the values, not the raw variables).
        self.terms: [B x 5], self.info: 0 when K_uu and every A_b factorised."""
        c = self.chain(z, mu, s, gamma, alpha, beta)
        f, ch, uu = self._forward(c)
        if not grad:
            return f
        d_mu, d_s, (dz_b, dg_b, da_b), gk, db_b = self._backward(c, ch, uu, mu, s)
        rk, sx, sq = ops.ard_rbf_gram_grad(z, gamma.reshape(1, -1), alpha.reshape(1), torch.sum(gk, dim=0))
        d_z = torch.sum(dz_b, dim=0) - 2.0 * gamma.reshape(1, -1) * sx
        d_gamma = torch.sum(dg_b, dim=0) - 0.5 * torch.sum(sq, dim=0)
        d_alpha = torch.sum(da_b) + torch.sum(rk) / alpha.reshape(()) - 0.5 * beta.reshape(()) * torch.sum(self.dims * self.n_w)
        return f, dict(mu=d_mu, s=d_s, z=d_z, gamma=d_gamma, alpha=d_alpha, beta=torch.sum(db_b))


def _log_normal_prior(x):
    """sum of the log-normal(0, 1) log-density over x (distributions/log_normal.py) and its derivative."""
    lx = torch.log(x)
    return torch.sum(-lx - 0.5 * (math.log(2.0 * math.pi) + lx * lx)), -(1.0 + lx) / x


class MaskedBayesianGPLVM:
    """The masked fp64 model behind bayesian_gp_lvm(..., observed=...): six raw variables (the names and shapes of the unmasked
    model's), objective = -(sum_slots f_b - KL(q(X)) over all N rows + hyper-prior), its gradients and the training-data
    imputation.  The interface is the part of dp_gp_lvm_t's that bayesian_gp_lvm uses: raw, gradients(), objective_terms
    (objective, f_hat, KL, 0, hyper-prior), cholesky_info."""

    def __init__(self, y0, observed, raw, device):
        self.bound = _MaskedBound(y0, observed, device)
        self.raw = raw
        self.y0, self.observed, self.device = y0, observed, device
        self.cholesky_info = torch.zeros((), dtype=torch.int32, device=device)

    def _values(self):
        r = self.raw
        return (r['x_u'].detach(), r['x_mean'].detach(), F.softplus(r['x_var'].detach()), F.softplus(r['gamma_atoms'].detach()),
                F.softplus(r['alpha_atoms'].detach()), F.softplus(r['beta_atoms'].detach()))

    def _rest(self, mu, s, gam, al, be):
        kl = 0.5 * (torch.sum(mu * mu) + torch.sum(s - torch.log(s)) - mu.shape[0] * mu.shape[1])
        priors = [_log_normal_prior(a) for a in (gam, al, be)]
        return kl, priors[0][0] + priors[1][0] + priors[2][0], [p[1] for p in priors]

    @property
    def objective_terms(self):
        with torch.no_grad():
            z, mu, s, gam, al, be = self._values()
            f = self.bound.evaluate(z, mu, s, gam, al, be)
            self.cholesky_info = self.bound.info
            kl, hyper, _ = self._rest(mu, s, gam, al, be)
            return torch.stack([-(f - kl) - hyper, f, kl, torch.zeros_like(f), hyper])

    def gradients(self):
        """d objective / d raw variable for the six raw variables."""
        with torch.no_grad():
            r = self.raw
            z, mu, s, gam, al, be = self._values()
            _, g = self.bound.evaluate(z, mu, s, gam, al, be, grad=True)
            self.cholesky_info = self.bound.info
            _, _, dp = self._rest(mu, s, gam, al, be)
            sg = lambda k: torch.sigmoid(r[k].detach())
            return dict(x_mean=-(g['mu'] - mu), x_var=-(g['s'] - 0.5 * (1.0 - 1.0 / s)) * sg('x_var'), x_u=-g['z'],
                        gamma_atoms=-(g['gamma'].reshape(gam.shape) + dp[0]) * sg('gamma_atoms'),
                        alpha_atoms=-(g['alpha'].reshape(al.shape) + dp[1]) * sg('alpha_atoms'),
                        beta_atoms=-(g['beta'].reshape(be.shape) + dp[2]) * sg('beta_atoms'))

    def impute(self):
        """[N x D]: the observed entries as given; an unobserved entry (n, d) gets beta Psi1[n,:] (K_uu + beta Psi2_d)^-1 Psi1^T y_d
        with Psi2_d and y_d over the rows at which d was observed; a never-observed column gets 0."""
        with torch.no_grad():
            means = self.bound.posterior_means(*self._values())
            obs = torch.as_tensor(self.observed, device=self.device)
            out = torch.zeros(self.y0.shape, dtype=TORCH_DTYPE, device=self.device)
            for i, (cols, _) in enumerate(self.bound.groups):
                out[:, torch.as_tensor(cols, device=self.device)] = means[i, :, :len(cols)]
            return torch.where(obs, torch.as_tensor(self.y0, dtype=TORCH_DTYPE, device=self.device), out)


class _MaskedViewsBound(_SlotBound):
    """_MaskedBound for V views with their own kernels (Z_v, gamma_v, alpha_v, beta_v) sharing q(X): the slots of view v use
    kernel v, kern[b] = v.  The slots of all views are ONE batch, ordered by view and then by first column; K_uu_v, its factors
    and the pair factor are formed once per kernel per evaluation and gathered to the slots; the per-slot d_z, d_gamma,
    d_alpha, d_beta and GK_b are added within their view (index_add), and the K_uu term of all V kernels is ONE
    ops.ard_rbf_gram_grad_batched with GK_v = sum_{b in v} GK_b."""

    def __init__(self, y0s, observeds, device):
        self.view_groups = [_missing.group_columns_by_pattern(o) for o in observeds]
        assert all(self.view_groups), 'every view must hold at least one True entry'
        self.slots = [(v, cols, w) for v, gs in enumerate(self.view_groups) for cols, w in gs]
        super().__init__([(y0s[v][:, cols], w) for v, cols, w in self.slots], device)
        self.v = len(y0s)
        self.kern = torch.tensor([v for v, _, _ in self.slots], dtype=torch.long, device=device)

    def per_view(self, t):
        """[B, ...] per slot -> [V, ...]: the slots of a view added."""
        return torch.zeros((self.v,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device).index_add_(0, self.kern, t)

    def chain(self, z, mu, s, gamma, alpha, beta):
        """z [V,M,Q], gamma [V,Q], alpha [V], beta [V]: everything up to the factor of A_b."""
        li, kinv, info_uu, zfac = collapsed.own_z_kernels(z, gamma, alpha)
        take = lambda t: t.index_select(0, self.kern).contiguous()
        c = dict(z=take(z), gamma=take(gamma), alpha=take(alpha), beta=take(beta), zfac=take(zfac), li=take(li), kinv=take(kinv))
        return self._chain(c, mu, s, info_uu)

    def evaluate(self, z, mu, s, gamma, alpha, beta, grad=False):
        """f (0-d); with grad also a dict of df/d(mu, s, z [V,M,Q], gamma [V,Q], alpha [V], beta [V]) (the values, not the raw
        variables).  self.terms: [B x 5], self.info: 0 when every K_uu_v and every A_b factorised."""
        c = self.chain(z, mu, s, gamma, alpha, beta)
        f, ch, uu = self._forward(c)
        if not grad:
            return f
        d_mu, d_s, (dz_b, dg_b, da_b), gk, db_b = self._backward(c, ch, uu, mu, s)
        rk, sx, sq = ops.ard_rbf_gram_grad_batched(z, gamma, alpha, self.per_view(gk))            # [V,M], [V,M,Q], [V,M,Q]
        d_z = self.per_view(dz_b) - 2.0 * gamma[:, None, :] * sx
        d_gamma = self.per_view(dg_b) - 0.5 * torch.sum(sq, dim=1)
        d_alpha = self.per_view(da_b.reshape(-1) - 0.5 * c['beta'] * self.dims * self.n_w) + torch.sum(rk, dim=1) / alpha
        return f, dict(mu=d_mu, s=d_s, z=d_z, gamma=d_gamma, alpha=d_alpha, beta=self.per_view(db_b))


class MaskedMRD:
    """The masked fp64 model behind manifold_relevance_determination(..., observed=...): raw variables x_mean, x_var and, per
    view v, x_u_v, gamma_atoms_v, alpha_atoms_v, beta_atoms_v (the names, shapes and order of the unmasked model's);
    objective = -(sum_v sum_{b in v} f_b - KL(q(X)) over all N rows + sum_v hyper-prior_v), its gradients and the imputation."""
    PER_VIEW = ('x_u', 'gamma_atoms', 'alpha_atoms', 'beta_atoms')

    def __init__(self, y0s, observeds, raw, device):
        self.bound = _MaskedViewsBound(y0s, observeds, device)
        self.raw, self.v = raw, len(y0s)
        self.y0s, self.observeds, self.device = y0s, observeds, device
        self.cholesky_info = torch.zeros((), dtype=torch.int32, device=device)

    def _values(self):
        r = self.raw
        stack = lambda k, pos: torch.stack([F.softplus(r['%s_%d' % (k, v)].detach()).reshape(-1) if pos else
                                            r['%s_%d' % (k, v)].detach() for v in range(self.v)]).contiguous()
        return (stack('x_u', False), r['x_mean'].detach(), F.softplus(r['x_var'].detach()), stack('gamma_atoms', True),
                stack('alpha_atoms', True).reshape(-1), stack('beta_atoms', True).reshape(-1))

    @staticmethod
    def _kl(mu, s):
        return 0.5 * (torch.sum(mu * mu) + torch.sum(s - torch.log(s)) - mu.shape[0] * mu.shape[1])

    def terms(self):
        """(objective, f_hat summed over the slots, KL(q(X)), hyper-prior summed over the views), 0-d each."""
        with torch.no_grad():
            z, mu, s, gam, al, be = self._values()
            f = self.bound.evaluate(z, mu, s, gam, al, be)
            self.cholesky_info = self.bound.info
            kl = self._kl(mu, s)
            hyper = sum(_log_normal_prior(a)[0] for a in (gam, al, be))
            return -(f - kl) - hyper, f, kl, hyper

    def gradients(self):
        """d objective / d raw variable, in the order of the raw variables."""
        with torch.no_grad():
            r = self.raw
            z, mu, s, gam, al, be = self._values()
            _, g = self.bound.evaluate(z, mu, s, gam, al, be, grad=True)
            self.cholesky_info = self.bound.info
            dp = [_log_normal_prior(a)[1] for a in (gam, al, be)]
            out = dict(x_mean=-(g['mu'] - mu), x_var=-(g['s'] - 0.5 * (1.0 - 1.0 / s)) * torch.sigmoid(r['x_var'].detach()))
            for v in range(self.v):
                raw_of = lambda k: r['%s_%d' % (k, v)].detach()
                out['x_u_%d' % v] = -g['z'][v]
                for k, gk, d in (('gamma_atoms', g['gamma'], dp[0]), ('alpha_atoms', g['alpha'], dp[1]),
                                 ('beta_atoms', g['beta'], dp[2])):
                    out['%s_%d' % (k, v)] = -((gk[v] + d[v]).reshape(raw_of(k).shape)) * torch.sigmoid(raw_of(k))
            return out

    def impute(self):
        """A list of V tensors [N x D_v]: the observed entries as given; an unobserved entry (n, d) of view v gets
        beta_v Psi1_v[n,:] (K_uu_v + beta_v Psi2_d)^-1 Psi1_v^T y_d with Psi2_d and y_d over the rows at which d was observed; a
        never-observed column gets 0."""
        with torch.no_grad():
            means = self.bound.posterior_means(*self._values())
            outs = [torch.zeros(y.shape, dtype=TORCH_DTYPE, device=self.device) for y in self.y0s]
            for i, (v, cols, _) in enumerate(self.bound.slots):
                outs[v][:, torch.as_tensor(cols, device=self.device)] = means[i, :, :len(cols)]
            return [torch.where(torch.as_tensor(o, device=self.device), torch.as_tensor(y, dtype=TORCH_DTYPE, device=self.device),
                                out) for o, y, out in zip(self.observeds, self.y0s, outs)]
