"""
The collapsed bound of bayesian_gp_lvm for TRAINING data with missing entries (observed=...), and its whole backward pass, in
fp64 on the device.  With a boolean mask [N x D] the bound is a sum over output dims, dim d seeing only the rows R_d at which
it was measured; columns that share one row pattern share a "slot" b (D_b columns, 0 / 1 row weights w_b, N_b = sum_n w_b[n]),
and all slots share the one kernel (Z, gamma, alpha, beta).  The forward pass is the sum _TestBound.slots(...).evaluate computes
(test_bound.py), evaluated at the training q(X); here Z and the hyper-parameters move, so K_uu and its factors are formed per
evaluation and the bound is also differentiated with respect to them.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from ..utils import missing as _missing
from ..utils.constants import GP_DEFAULT_JITTER
from ..utils.types import TORCH_DTYPE


class _MaskedBound:
    """f = sum_b f_b with (T_b = L^-1 Psi2_b L^-T, A_b = beta T_b + I = L_A L_A^T, R0 = L_A^-1 L^-1, U = R0 Psi1^T Y_b)
        f_b = 1/2 N_b D_b (log beta - log 2 pi) - D_b log|L_A| + 1/2 D_b beta (tr T_b - alpha N_b) + 1/2 beta^2 |U|^2 - 1/2 beta |Y_b|^2
    Psi2_b the weighted sum over the rows of slot b (ops.qx_psi_stats_batched(weights=)), Y_b zero where unobserved.

    Backward pass (P = (K_uu + beta Psi2_b)^-1 = R0^T R0, R = P Psi1^T Y_b, KP = K_uu^-1 Psi2_b):
        G2_b = 1/2 D_b beta^2 sym(KP P) - 1/2 beta^3 R R^T         (= 1/2 D_b beta (K_uu^-1 - P) - .., written as a product:
        G1_b = beta^2 Y_b R^T                                         the difference cancels for a small beta |Psi2| / |K_uu|)
        GK_b = -1/2 D_b beta^2 KP P KP^T - 1/2 beta^2 R R^T         (= 1/2 D_b (K_uu^-1 - P) - 1/2 D_b beta K_uu^-1 Psi2_b K_uu^-1 - ..)
    (mu, S) through ops.qx_psi_adjoint(weights=), (Z, gamma, alpha) through Psi by ops.qx_psi_param_adjoint with the same G1, G2
    (per slot, added here: the slots share the kernel), through K_uu by ONE ops.ard_rbf_gram_grad with GK = sum_b GK_b; beta and
    alpha's explicit -1/2 D_b beta N_b are closed forms on the [B, M, M] arrays.  No host synchronisation."""

    def __init__(self, y0, observed, device):
        f64 = TORCH_DTYPE
        groups = _missing.group_columns_by_pattern(observed)
        assert groups, 'observed must hold at least one True entry'
        n, dmax = y0.shape[0], max(len(c) for c, _ in groups)
        y = np.zeros((len(groups), n, dmax))
        for i, (cols, _) in enumerate(groups):
            y[i, :, :len(cols)] = y0[:, cols]
        self.groups = groups
        self.b, self.n, self.device = len(groups), n, device
        self.y = torch.as_tensor(y, dtype=f64, device=device).contiguous()                           # [B, N, Dmax]
        self.yy = torch.sum(self.y * self.y, dim=(1, 2))
        self.dims = torch.tensor([float(len(c)) for c, _ in groups], dtype=f64, device=device)
        self.weights = torch.as_tensor(np.stack([w for _, w in groups]), dtype=f64, device=device).contiguous()
        self.n_w = torch.sum(self.weights, dim=1)
        self.one = torch.ones(1, dtype=f64, device=device)
        self.terms = self.info = None

    def chain(self, z, mu, s, gamma, alpha, beta):
        """Everything up to the factor of A_b (shared by evaluate and the imputation)."""
        b, m = self.b, z.shape[0]
        gamma, alpha = gamma.reshape(1, -1), alpha.reshape(1)
        k_uu = ops.ard_rbf_gram(z, None, gamma, alpha, self.one, include_noise=False, include_jitter=True,
                                jitter=GP_DEFAULT_JITTER)
        l_uu, info_uu = ops.potrf_batched(k_uu)
        li = ops.tril_inverse_batched(l_uu)
        kinv = ops.matmul(li.transpose(1, 2), li)
        zfac = ops.ard_rbf_gram(z, None, 0.5 * gamma, alpha * alpha, self.one)
        rep = lambda t: t.expand(b, *t.shape[1:]).contiguous()
        c = dict(z=rep(z[None]), gamma=rep(gamma), alpha=rep(alpha), zfac=rep(zfac), li=rep(li), kinv=rep(kinv))
        c['psi_1'], c['psi_2'] = ops.qx_psi_stats_batched(c['z'], mu, s, c['gamma'], c['alpha'], c['zfac'], weights=self.weights)
        c['tm'] = ops.matmul(ops.matmul(c['li'], c['psi_2']), c['li'].transpose(1, 2))
        eye = torch.eye(m, dtype=TORCH_DTYPE, device=self.device)
        c['l_a'], info_a = ops.potrf_batched(beta.reshape(1, 1, 1) * c['tm'] + eye)
        c['r0'] = ops.matmul(ops.tril_inverse_batched(c['l_a']), c['li'])
        self.info = torch.maximum(info_uu.abs().max(), info_a.abs().max())
        return c

    def evaluate(self, z, mu, s, gamma, alpha, beta, grad=False):
        """f (0-d); with grad also a dict of df/d(mu, s, z, gamma [Q], alpha, beta) (the values, not the raw variables).
        self.terms: [B x 5], self.info: 0 when K_uu and every A_b factorised."""
        be, al, dd, n_w = beta.reshape(()), alpha.reshape(()), self.dims, self.n_w
        c = self.chain(z, mu, s, gamma, alpha, beta)
        psi_1, psi_2, tm, r0 = c['psi_1'], c['psi_2'], c['tm'], c['r0']
        u = ops.matmul(r0, ops.matmul(psi_1.transpose(1, 2), self.y))                            # [B, M, Dmax]
        logdet = torch.sum(torch.log(torch.diagonal(c['l_a'], dim1=-2, dim2=-1)), dim=-1)
        tr = torch.diagonal(tm, dim1=-2, dim2=-1).sum(-1)
        uu = torch.sum(u * u, dim=(1, 2))
        self.terms = torch.stack([0.5 * n_w * dd * (torch.log(be) - math.log(2.0 * math.pi)), -dd * logdet,
                                  0.5 * dd * be * (tr - al * n_w), 0.5 * be * be * uu, -0.5 * be * self.yy], dim=1)
        f = torch.sum(self.terms)
        if not grad:
            return f
        sym = lambda a: 0.5 * (a + a.transpose(1, 2))
        d3 = dd[:, None, None]
        r = ops.matmul(r0.transpose(1, 2), u)                                                     # [B, M, Dmax]
        p = ops.matmul(r0.transpose(1, 2), r0)
        rrt = ops.matmul(r, r.transpose(1, 2))
        kp = ops.matmul(c['kinv'], psi_2)                                                         # K_uu^-1 Psi2_b
        kpp = ops.matmul(kp, p)
        g2 = (0.5 * be * be) * d3 * sym(kpp) - (0.5 * be ** 3) * rrt
        g1 = (be * be) * ops.matmul(self.y, r.transpose(1, 2))                                   # [B, N, M]
        gk = torch.sum((-0.5 * be * be) * d3 * sym(ops.matmul(kpp, kp.transpose(1, 2))) - (0.5 * be * be) * rrt, dim=0)
        args = (c['z'], mu, s, c['gamma'], c['alpha'], g1, g2, c['zfac'])
        d_mu, d_s = ops.qx_psi_adjoint(*args, weights=self.weights)
        dz_b, dg_b, da_b = ops.qx_psi_param_adjoint(*args, weights=self.weights)
        rk, sx, sq = ops.ard_rbf_gram_grad(z, gamma.reshape(1, -1), alpha.reshape(1), gk)
        d_z = torch.sum(dz_b, dim=0) - 2.0 * gamma.reshape(1, -1) * sx
        d_gamma = torch.sum(dg_b, dim=0) - 0.5 * torch.sum(sq, dim=0)
        d_alpha = torch.sum(da_b) + torch.sum(rk) / al - 0.5 * be * torch.sum(dd * n_w)
        d_beta = torch.sum(0.5 * n_w * dd / be - 0.5 * dd * torch.sum(p * psi_2, dim=(1, 2)) + 0.5 * dd * (tr - al * n_w)
                           + be * uu - (0.5 * be * be) * torch.sum(rrt * psi_2, dim=(1, 2)) - 0.5 * self.yy)
        return f, dict(mu=d_mu, s=d_s, z=d_z, gamma=d_gamma, alpha=d_alpha, beta=d_beta)

    def posterior_means(self, z, mu, s, gamma, alpha, beta):
        """[B, N, Dmax]: beta Psi1 (K_uu + beta Psi2_b)^-1 Psi1^T Y_b at every row, per slot (Psi1 is not weighted)."""
        c = self.chain(z, mu, s, gamma, alpha, beta)
        p = ops.matmul(c['r0'].transpose(1, 2), c['r0'])
        v = ops.matmul(c['psi_1'].transpose(1, 2), self.y)
        return beta.reshape(()) * ops.matmul(c['psi_1'], ops.matmul(p, v))


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


class _MaskedViewsBound:
    """_MaskedBound for V views with their own kernels (Z_v, gamma_v, alpha_v, beta_v) sharing q(X): the slots of view v (the
    column groups of its mask that share one row pattern) use kernel v, kern[b] = v.  The slots of all views are ONE batch,
    ordered by view and then by first column: one weighted stats call, one adjoint and one parameter adjoint serve them all,
    and the per-slot d_z, d_gamma, d_alpha, d_beta and GK_b are added within their view (index_add).  K_uu_v, L_v, L_v^-1,
    K_uu_v^-1 and the pair factor are formed once per kernel per evaluation and gathered to the slots; the K_uu term of all V
    kernels is ONE ops.ard_rbf_gram_grad_batched with GK_v = sum_{b in v} GK_b.  The formulas per slot are _MaskedBound's with
    (alpha, beta) of the slot's kernel.  No host synchronisation."""

    def __init__(self, y0s, observeds, device):
        f64 = TORCH_DTYPE
        self.view_groups = [_missing.group_columns_by_pattern(o) for o in observeds]
        assert all(self.view_groups), 'every view must hold at least one True entry'
        slots = [(v, cols, w) for v, gs in enumerate(self.view_groups) for cols, w in gs]
        n, dmax = y0s[0].shape[0], max(len(c) for _, c, _ in slots)
        y = np.zeros((len(slots), n, dmax))
        for i, (v, cols, _) in enumerate(slots):
            y[i, :, :len(cols)] = y0s[v][:, cols]
        self.slots = slots
        self.b, self.v, self.n, self.device = len(slots), len(y0s), n, device
        self.kern = torch.tensor([v for v, _, _ in slots], dtype=torch.long, device=device)
        self.y = torch.as_tensor(y, dtype=f64, device=device).contiguous()                           # [B, N, Dmax]
        self.yy = torch.sum(self.y * self.y, dim=(1, 2))
        self.dims = torch.tensor([float(len(c)) for _, c, _ in slots], dtype=f64, device=device)
        self.weights = torch.as_tensor(np.stack([w for _, _, w in slots]), dtype=f64, device=device).contiguous()
        self.n_w = torch.sum(self.weights, dim=1)
        self.one = torch.ones(1, dtype=f64, device=device)
        self.terms = self.info = None

    def per_view(self, t):
        """[B, ...] per slot -> [V, ...]: the slots of a view added."""
        return torch.zeros((self.v,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device).index_add_(0, self.kern, t)

    def chain(self, z, mu, s, gamma, alpha, beta):
        """z [V,M,Q], gamma [V,Q], alpha [V], beta [V]: everything up to the factor of A_b."""
        m = z.shape[1]
        k_uu = torch.cat([ops.ard_rbf_gram(z[v], None, gamma[v:v + 1], alpha[v:v + 1], self.one, include_noise=False,
                                           include_jitter=True, jitter=GP_DEFAULT_JITTER) for v in range(self.v)])
        l_uu, info_uu = ops.potrf_batched(k_uu)
        li = ops.tril_inverse_batched(l_uu)
        kinv = ops.matmul(li.transpose(1, 2), li)
        zfac = ops.qx_pair_factor(z, gamma, alpha)
        take = lambda t: t.index_select(0, self.kern).contiguous()
        c = dict(z=take(z), gamma=take(gamma), alpha=take(alpha), beta=take(beta), zfac=take(zfac), li=take(li), kinv=take(kinv))
        c['psi_1'], c['psi_2'] = ops.qx_psi_stats_batched(c['z'], mu, s, c['gamma'], c['alpha'], c['zfac'], weights=self.weights)
        c['tm'] = ops.matmul(ops.matmul(c['li'], c['psi_2']), c['li'].transpose(1, 2))
        eye = torch.eye(m, dtype=TORCH_DTYPE, device=self.device)
        c['l_a'], info_a = ops.potrf_batched(c['beta'][:, None, None] * c['tm'] + eye)
        c['r0'] = ops.matmul(ops.tril_inverse_batched(c['l_a']), c['li'])
        self.info = torch.maximum(info_uu.abs().max(), info_a.abs().max())
        return c

    def evaluate(self, z, mu, s, gamma, alpha, beta, grad=False):
        """f (0-d); with grad also a dict of df/d(mu, s, z [V,M,Q], gamma [V,Q], alpha [V], beta [V]) (the values, not the raw
        variables).  self.terms: [B x 5], self.info: 0 when every K_uu_v and every A_b factorised."""
        dd, n_w = self.dims, self.n_w
        c = self.chain(z, mu, s, gamma, alpha, beta)
        be, al = c['beta'], c['alpha']                                                            # [B]: the slots' kernels'
        psi_1, psi_2, tm, r0 = c['psi_1'], c['psi_2'], c['tm'], c['r0']
        u = ops.matmul(r0, ops.matmul(psi_1.transpose(1, 2), self.y))                            # [B, M, Dmax]
        logdet = torch.sum(torch.log(torch.diagonal(c['l_a'], dim1=-2, dim2=-1)), dim=-1)
        tr = torch.diagonal(tm, dim1=-2, dim2=-1).sum(-1)
        uu = torch.sum(u * u, dim=(1, 2))
        self.terms = torch.stack([0.5 * n_w * dd * (torch.log(be) - math.log(2.0 * math.pi)), -dd * logdet,
                                  0.5 * dd * be * (tr - al * n_w), 0.5 * be * be * uu, -0.5 * be * self.yy], dim=1)
        f = torch.sum(self.terms)
        if not grad:
            return f
        sym = lambda a: 0.5 * (a + a.transpose(1, 2))
        d3, b3 = dd[:, None, None], be[:, None, None]
        r = ops.matmul(r0.transpose(1, 2), u)                                                     # [B, M, Dmax]
        p = ops.matmul(r0.transpose(1, 2), r0)
        rrt = ops.matmul(r, r.transpose(1, 2))
        kp = ops.matmul(c['kinv'], psi_2)                                                         # K_uu^-1 Psi2_b
        kpp = ops.matmul(kp, p)
        g2 = (0.5 * b3 * b3) * d3 * sym(kpp) - (0.5 * b3 ** 3) * rrt
        g1 = (b3 * b3) * ops.matmul(self.y, r.transpose(1, 2))                                   # [B, N, M]
        gk = self.per_view((-0.5 * b3 * b3) * d3 * sym(ops.matmul(kpp, kp.transpose(1, 2))) - (0.5 * b3 * b3) * rrt)
        args = (c['z'], mu, s, c['gamma'], c['alpha'], g1, g2, c['zfac'])
        d_mu, d_s = ops.qx_psi_adjoint(*args, weights=self.weights)
        dz_b, dg_b, da_b = ops.qx_psi_param_adjoint(*args, weights=self.weights)
        rk, sx, sq = ops.ard_rbf_gram_grad_batched(z, gamma, alpha, gk)                           # [V,M], [V,M,Q], [V,M,Q]
        d_z = self.per_view(dz_b) - 2.0 * gamma[:, None, :] * sx
        d_gamma = self.per_view(dg_b) - 0.5 * torch.sum(sq, dim=1)
        d_alpha = self.per_view(da_b.reshape(-1) - 0.5 * be * dd * n_w) + torch.sum(rk, dim=1) / alpha
        d_beta = self.per_view(0.5 * n_w * dd / be - 0.5 * dd * torch.sum(p * psi_2, dim=(1, 2)) + 0.5 * dd * (tr - al * n_w)
                               + be * uu - (0.5 * be * be) * torch.sum(rrt * psi_2, dim=(1, 2)) - 0.5 * self.yy)
        return f, dict(mu=d_mu, s=d_s, z=d_z, gamma=d_gamma, alpha=d_alpha, beta=d_beta)

    def posterior_means(self, z, mu, s, gamma, alpha, beta):
        """[B, N, Dmax]: beta_v Psi1_v (K_uu_v + beta_v Psi2_b)^-1 Psi1_v^T Y_b at every row, per slot (Psi1 is not weighted)."""
        c = self.chain(z, mu, s, gamma, alpha, beta)
        p = ops.matmul(c['r0'].transpose(1, 2), c['r0'])
        v = ops.matmul(c['psi_1'].transpose(1, 2), self.y)
        return c['beta'][:, None, None] * ops.matmul(c['psi_1'], ops.matmul(p, v))


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
