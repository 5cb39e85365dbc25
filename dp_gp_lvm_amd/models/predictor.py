"""
Frozen predictors: the per-entry predictive moments of a trained model as a differentiable function of q(X*) = (x_mean, x_var).

A predictor holds the training side of the moments (factorisations, c = K^-1 - P, posterior weights r), built ONCE at the model's
parameters of the moment it was made; it is stale after further training: make a new one.  Calling it costs what the test side
costs, so a loop over q(X*) (fitting q(X*) to a predictive density, walking the latent space) does not redo the training side.

    p = model.frozen_predictor(columns)
    mean, var = p(x_mean, x_var)                         each [N* x len(columns)]; the bits of model.predictive_marginals
    d_mean, d_var = p.vjp(x_mean, x_var, g_mean, g_var)  [N* x Q] each; derivatives with respect to the VARIANCES x_var

With inputs that require grad the outputs carry a grad_fn (one torch.autograd.Function whose backward is the VJP; once
differentiable).  The VJPs run on the fp64 HIP adjoint operators:
    bayesian_gp_lvm, MRD views   ops.qx_psi_point_moments_adjoint           (one kernel, J columns, G row patterns)
    dp_gp_lvm_t                  mixture_moments_vjp on the host, then the same operator on the T atoms
    dp_gp_lvm                    ops.psi_latent_adjoint: K = len(columns) kernels share Z and q(X*); with c_b, r_b of column b,
                                 w[b][n] = g_var[n,b], g_psi2_b = r_b r_b^T - c_b, y[n,b] = g_mean[n,b] - 2 mean[n,b] g_var[n,b],
                                 g_v_b = r_b; a column never observed in training is left out: exact zeros.
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .. import ops
from ..utils.types import TORCH_DTYPE


def mixture_moments_vjp(phit, mean_t, mean, g_mean, g_var):
    """The adjoints (g_mean_t, g_var_t) [T,N,J] of frozen_bound_t.mixture_moments' inputs: phit [T,J], mean_t [T,N,J] the atoms'
    means, mean [N,J] the mixture's, (g_mean, g_var) [N,J] the adjoints of its outputs (pure torch, any device)."""
    w = phit[:, None, :]
    return w * (g_mean[None] + 2.0 * g_var[None] * (mean_t - mean[None])), w * g_var[None].expand_as(mean_t)


def negative_log_density(mean, var, y, given):
    """-sum over the entries with given = True of log N(y | mean, var): the held-out predictive density that q(X*) can be fitted to
    through a predictor (y, given [N* x J] on mean's device; entries not given are ignored and may be NaN)."""
    y = torch.where(given, y, mean.detach())
    terms = 0.5 * (torch.log(2.0 * np.pi * var) + (y - mean) ** 2 / var)
    return torch.sum(torch.where(given, terms, torch.zeros_like(terms)))


class _MomentsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, predictor, mu, s):
        mean, var = predictor._forward(mu, s)
        ctx.predictor = predictor
        ctx.save_for_backward(mu, s, mean)
        return mean, var

    @staticmethod
    @once_differentiable
    def backward(ctx, g_mean, g_var):
        mu, s, mean = ctx.saved_tensors
        d_mu, d_s = ctx.predictor._vjp(mu, s, _adjoint(g_mean, mean), _adjoint(g_var, mean), mean)
        return None, d_mu, d_s


def _adjoint(g, like):
    if g is None:
        return torch.zeros_like(like)
    assert g.shape == like.shape, 'the adjoints must be [N* x len(columns)]'
    return g.detach().to(device=like.device, dtype=TORCH_DTYPE).contiguous()


class FrozenPredictor:
    """See the module's text.  forward(mu, s) -> (mean, var); vjp(mu, s, g_mean, g_var, mean) -> (d_mu, d_s); `mean` is the
    forward's first output at the same (mu, s)."""

    def __init__(self, device, num_columns, forward, vjp):
        self.device, self.num_columns = device, num_columns
        self._forward, self._vjp = forward, vjp

    def _arg(self, v):
        if torch.is_tensor(v):
            return v.to(device=self.device, dtype=TORCH_DTYPE).contiguous()
        return torch.as_tensor(np.asarray(v, dtype=np.float64), dtype=TORCH_DTYPE).to(self.device).contiguous()

    def _args(self, x_mean, x_var):
        mu, s = self._arg(x_mean), self._arg(x_var)
        assert mu.dim() == 2 and mu.shape == s.shape, 'x_mean and x_var must be [N* x Q]'
        return mu, s

    def __call__(self, x_mean, x_var):
        mu, s = self._args(x_mean, x_var)
        if torch.is_grad_enabled() and (mu.requires_grad or s.requires_grad):
            return _MomentsFn.apply(self, mu, s)
        with torch.no_grad():
            return self._forward(mu, s)

    def vjp(self, x_mean, x_var, grad_mean, grad_var):
        """(d_x_mean, d_x_var) [N* x Q] of sum grad_mean . mean + sum grad_var . var at q(X*) = (x_mean, x_var)."""
        with torch.no_grad():
            mu, s = self._args(x_mean, x_var)
            mean, _ = self._forward(mu, s)
            return self._vjp(mu, s, _adjoint(grad_mean, mean), _adjoint(grad_var, mean), mean)


def of_marginals(marg, cols, device):
    """One kernel's predictor on a marginals._Marginals (K = 1): bayesian_gp_lvm and a view of MRD."""
    r, gidx = marg.r.index_select(2, cols).contiguous(), marg.gidx.index_select(1, cols).contiguous()

    def forward(mu, s):
        mean, var = marg.at(mu, s, cols)
        return mean[0], var[0]

    def vjp(mu, s, g_mean, g_var, mean):
        return ops.qx_psi_point_moments_adjoint(marg.z, mu, s, marg.gamma, marg.alpha, marg.c, r, gidx, marg.beta, mean[None].contiguous(),
                                                g_mean[None].contiguous(), g_var[None].contiguous(), zfac=marg.zfac)
    return FrozenPredictor(device, int(cols.numel()), forward, vjp)


def of_mixture(mom, cols, device):
    """dp_gp_lvm_t's predictor on a frozen_bound_t._MomentsT: the VJP of the mixture on the host, then the T atoms' operator."""
    r = mom.r.index_select(2, cols).contiguous()                                                   # [T, M, J]
    phit = mom.phit.index_select(1, cols)
    gidx = mom.pattern.index_select(0, cols).to(torch.int32)[None].expand(r.shape[0], -1).contiguous()

    def forward(mu, s):
        return mom.at(mu, s, cols)

    def vjp(mu, s, g_mean, g_var, mean):
        mean_t = ops.matmul(ops.psi1(mom.z, mu, s, mom.gat, mom.aat), r)                           # [T, N*, J], as _MomentsT.at
        g_mean_t, g_var_t = mixture_moments_vjp(phit, mean_t, mean, g_mean, g_var)
        return ops.qx_psi_point_moments_adjoint(mom.z_t, mu, s, mom.gat, mom.aat, mom.c, r, gidx, mom.bat, mean_t,
                                                g_mean_t.contiguous(), g_var_t.contiguous(), zfac=mom.zfac)
    return FrozenPredictor(device, int(cols.numel()), forward, vjp)


def of_columns(z, gamma, alpha, beta, c, r, here, prior_var, scatter, device):
    """dp_gp_lvm's predictor: every output column its own kernel on the shared Z [M,Q].  gamma [K,Q], alpha, beta [K], c [K,M,M]
    and r [K,M] belong to the K columns at the places `here` (a long tensor) of the predictor's columns; prior_var [J]: alpha_d +
    1/beta_d of every column, the variance of those never observed in training (their mean is 0).  scatter: the outputs are
    written into (0, prior_var) at `here`, as the mask-trained model's predictive_marginals does; without it K = J."""
    k, width = int(here.numel()), int(prior_var.numel())
    if k:
        z_k = z[None].expand(k, -1, -1).contiguous()
        c4, r3 = c[:, None].contiguous(), r[:, :, None].contiguous()
        gidx = torch.zeros((k, 1), dtype=torch.int32, device=device)
        g_psi2 = (ops.matmul(r3, r3.transpose(1, 2).contiguous()) - c).contiguous()
    assert scatter or k == width

    def forward(mu, s):
        n = mu.shape[0]
        if not scatter:
            mean, var = ops.qx_psi_point_moments(z_k, mu, s, gamma, alpha, c4, r3, gidx, beta)
            return mean[:, :, 0].transpose(0, 1).contiguous(), var[:, :, 0].transpose(0, 1).contiguous()
        mean = torch.zeros((n, width), dtype=TORCH_DTYPE, device=device)
        var = prior_var[None, :].expand(n, -1).clone()
        if k:
            mn, vr = ops.qx_psi_point_moments(z_k, mu, s, gamma, alpha, c4, r3, gidx, beta)
            mean[:, here], var[:, here] = mn[:, :, 0].transpose(0, 1), vr[:, :, 0].transpose(0, 1)
        return mean, var

    def vjp(mu, s, g_mean, g_var, mean):
        if not k:
            return torch.zeros_like(mu), torch.zeros_like(s)
        y = (g_mean - 2.0 * mean * g_var).index_select(1, here).contiguous()                       # [N*, K]
        w = g_var.index_select(1, here).transpose(0, 1).contiguous()                               # [K, N*]
        return ops.psi_latent_adjoint(z, mu, s, gamma, alpha, y, r, g_psi2, weights=w)
    return FrozenPredictor(device, width, forward, vjp)
