"""
GP regression and the GP-LVM (reference src/models/gaussian_process.py:22-129): exact GP on one ARD-RBF kernel shared by
the D outputs; the gradient of the marginal likelihood with respect to the kernel's inputs and hyper-parameters reduces to
one contraction of dL/dK with the gram (dpgp_ard_rbf_gram_grad_f64), the rest to the library's gram / Cholesky / inverse /
product operators.

Bayesian GP-LVM — mirror of the reference's ``bayesian_gp_lvm`` factory (src/models/gaussian_process.py:132-270; SURVEY.md
§8(f) row 4: the B = 1 model, which needs no new kernels).  One ARD-RBF kernel (gamma [1 x Q], alpha, beta [1 x 1]) serves
all D output dims, so the f_hat of gaussian_process.py:236-258 is the over-T f_hat of ``dp_gp_lvm_t`` with a single atom and
phi = 1; the objective is  -(f_hat - KL(q(X)||p(X)) + kernel.prior_log_likelihood)  (:263-269).  This wrapper therefore
builds a one-atom ``dp_gp_lvm_t`` (library operators for the forward, its autograd.Function for the backward) and drops the
(constant) DP terms.  The reference's stochastic variant (``num_latent_samples > 0``: Monte-Carlo psi statistics through
tensorflow_probability) is not built.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from ..distributions.normal import mvn_conditional_mean_covar

from ..kernels.interfaces.kernel import KernelHyperparameters
from ..kernels.rbf_kernel import k_ard_rbf
from ..utils.constants import GP_LVM_DEFAULT_LATENT_DIMENSIONS, GP_LVM_DEFAULT_NUM_INDUCING_POINTS, GP_INIT_GAMMA, \
    GP_INIT_ALPHA, GP_INIT_BETA, GP_DEFAULT_JITTER
from ..utils.expressions import principal_component_analysis as pca
from ..utils import missing as _missing
from .dp_gp_lvm import dp_gp_lvm_t
from ..utils.types import TORCH_DTYPE, default_device, inverse_softplus
from .interfaces.trainable import Trainable
from .frozen_bound import _TestBound, _as_device, kernel_slots
from .masked_bound import MaskedBayesianGPLVM, MaskedMRD, _MaskedBound, _MaskedViewsBound
from . import collapsed, marginals as _marginals, predictor as _predictor, test_latents as _latents
from .latent_geometry import LatentGeometry, ViewsLatentGeometry


def _gp_forward(x, y, gamma, alpha, beta):
    """log N(y_d | 0, K) for every output dim d [D] (gaussian_process.py:50-55 without the hyper-prior), K = gram(x) +
    (1/beta + jitter) I, plus what the gradient needs: (ll, info, K^-1, A = K^-1 Y).  No host synchronisation."""
    n = y.shape[0]
    k = ops.ard_rbf_gram(x, None, gamma, alpha, beta, include_noise=True, include_jitter=True, jitter=GP_DEFAULT_JITTER)
    l_, info = ops.potrf_batched(k)
    li = ops.tril_inverse_batched(l_)[0]
    kinv = ops.matmul(li.transpose(0, 1), li)
    a = ops.matmul(kinv, y)
    logdet = 2.0 * torch.sum(torch.log(torch.diagonal(l_[0])))
    ll = -0.5 * torch.sum(y * a, dim=0) - 0.5 * logdet - 0.5 * n * math.log(2.0 * math.pi)
    ll = torch.where(info[0] == 0, ll, torch.full_like(ll, float('nan')))
    return ll, info, kinv, a


def _gp_backward(x, gamma, alpha, beta, kinv, a, weights=None):
    """Derivatives of sum_d weights_d ll_d with respect to (x, gamma, alpha, beta) — the softplus'd values.
    W = dL/dK = 1/2 A diag(weights) A^T - (sum weights)/2 K^-1 overwrites kinv; weights None means all ones."""
    d = a.shape[1]
    if weights is None:
        w = ops.matmul(a, a.transpose(0, 1), out=kinv, alpha=0.5, beta=-0.5 * d)
    else:
        kinv.mul_(-0.5 * torch.sum(weights))
        w = ops.matmul(a * weights[None, :], a.transpose(0, 1), out=kinv, alpha=0.5, beta=1.0)
    r, sx, sq = ops.ard_rbf_gram_grad(x, gamma, alpha, w)
    d_x = -2.0 * gamma.reshape(1, -1) * sx
    d_gamma = (-0.5 * torch.sum(sq, dim=0)).reshape(gamma.shape)
    d_alpha = (torch.sum(r) / alpha.reshape(-1)[0]).reshape(alpha.shape)
    d_beta = (-torch.sum(torch.diagonal(w)) / beta.reshape(-1)[0] ** 2).reshape(beta.shape)
    return d_x, d_gamma, d_alpha, d_beta


class _GPLogLikelihood(torch.autograd.Function):
    """ll [D] of _gp_forward, differentiable with respect to x, gamma, alpha, beta through _gp_backward (no tape)."""

    @staticmethod
    def forward(ctx, x, gamma, alpha, beta, y):
        ll, _, kinv, a = _gp_forward(x, y, gamma, alpha, beta)
        ctx.save_for_backward(x, gamma, alpha, beta, kinv, a)
        return ll

    @staticmethod
    def backward(ctx, g):
        x, gamma, alpha, beta, kinv, a = ctx.saved_tensors
        d_x, d_gamma, d_alpha, d_beta = _gp_backward(x, gamma, alpha, beta, kinv.clone(), a, weights=g)
        return d_x, d_gamma, d_alpha, d_beta, None


def _gaussian_process(x_raw, y, raw, x_name, device):
    """The model object behind gp_regression / gp_lvm.  raw: ordered dict of leaf tensors (x_name among them when the input
    is trainable); x_raw: the input tensor (the same storage as raw[x_name] then)."""
    n, d = y.shape

    def hyper():
        return F.softplus(raw['gamma_raw']), F.softplus(raw['alpha_raw']), F.softplus(raw['beta_raw'])

    def kernel():
        gamma, alpha, beta = hyper()
        return k_ard_rbf(gamma=gamma, alpha=alpha, beta=beta)

    def log_likelihood():
        gamma, alpha, beta = hyper()
        kern = k_ard_rbf(gamma=gamma, alpha=alpha, beta=beta)
        return _GPLogLikelihood.apply(x_raw, gamma, alpha, beta, y) + kern.prior_log_likelihood

    def gradients_and_info():
        with torch.no_grad():
            gamma, alpha, beta = hyper()
            ll, info, kinv, a = _gp_forward(x_raw.detach(), y, gamma, alpha, beta)
            d_x, d_gamma, d_alpha, d_beta = _gp_backward(x_raw.detach(), gamma, alpha, beta, kinv, a)
        # softplus chain rule and the D copies of the hyper-prior: autograd on the three small raw tensors
        hr = [raw[k].detach().requires_grad_() for k in ('gamma_raw', 'alpha_raw', 'beta_raw')]
        with torch.enable_grad():
            vals = [F.softplus(t) for t in hr]
            prior = k_ard_rbf(gamma=vals[0], alpha=vals[1], beta=vals[2]).prior_log_likelihood
            surrogate = -(torch.sum(d_gamma * vals[0]) + torch.sum(d_alpha * vals[1]) + torch.sum(d_beta * vals[2])) - d * prior
            gh = torch.autograd.grad(surrogate, hr)
        out = {}
        for k in raw:
            out[k] = -d_x if k == x_name else gh[('gamma_raw', 'alpha_raw', 'beta_raw').index(k)]
        return out, info

    def _gradients():
        return gradients_and_info()[0]

    def _optimise(num_iterations, learning_rate=0.01, callback=None):
        opt = torch.optim.Adam(list(raw.values()), lr=learning_rate)
        for it in range(num_iterations):
            g, info = gradients_and_info()
            if int(info[0]) != 0:                                          # (one read of the Cholesky info per iteration)
                raise FloatingPointError('iteration %d: the Cholesky factorisation of K failed at minor %d'
                                         % (it, int(info[0])))
            for k, p_ in raw.items():
                p_.grad = g[k].reshape(p_.shape)
            opt.step()
            if callback is not None:
                callback(it)

    def _predict_mean_covar(x_test, reference_compat=True):
        with torch.no_grad():
            xs = _as_device(x_test, device)
            assert xs.dim() == 2 and xs.shape[1] == x_raw.shape[1], 'x_test must be [N* x Q]'
            kern = kernel()
            k_ss = kern.covariance_matrix(xs, None, include_noise=False, include_jitter=True)
            k_xs = kern.covariance_matrix(x_raw.detach(), xs, include_noise=False, include_jitter=False)
            k_xx = kern.covariance_matrix(x_raw.detach(), None, include_noise=True, include_jitter=True)
            zeros_s = torch.zeros((xs.shape[0], 1), dtype=TORCH_DTYPE, device=device)
            zeros_x = torch.zeros((n, 1), dtype=TORCH_DTYPE, device=device)
            return mvn_conditional_mean_covar(b=y, mean_a=zeros_s, mean_b=zeros_x, covar_aa=k_ss, covar_bb=k_xx, covar_ab=k_xs,
                                              reference_compat=reference_compat)

    class GaussianProcess(Trainable):
        """Accessors as in the reference (gaussian_process.py:57-104), plus raw_variables / gradients / optimise."""
        raw_variables = raw

        @property
        def kernel(self):
            return kernel()

        @property
        def log_likelihood(self):
            """[D]: log N(y_d | 0, K_xx) + kernel.prior_log_likelihood for every output dim (the prior in EVERY entry,
            as the reference's broadcast does: gaussian_process.py:50-53)."""
            return log_likelihood()

        @property
        def objective(self):
            """-sum(log_likelihood) = -sum_d log N(y_d | 0, K_xx) - D * prior (gaussian_process.py:54): 0-d fp64 device
            tensor; .backward() fills the raw variables' .grad."""
            return -torch.sum(log_likelihood())

        @staticmethod
        def predict_mean_covar(x_test, reference_compat=True):
            """Predictive mean [N* x D] and covariance [N* x N*] at x_test [N* x Q] (gaussian_process.py:73-94): K_ss with
            jitter, K_xs with neither noise nor jitter, K_xx with both.  N* = 1 works (the reference fails there: it
            squeezes K_xs to a vector).  reference_compat: see distributions.normal.mvn_conditional_mean_covar — True
            gives the reference's mean K_xs^T diag(L)^-1 L^-1 Y, False the textbook K_xs^T K_xx^-1 Y."""
            return _predict_mean_covar(x_test, reference_compat)

        gradients = staticmethod(_gradients)
        optimise = staticmethod(_optimise)

    if x_name is not None:
        class GPLVM(GaussianProcess):
            @property
            def latent_input(self):
                return raw[x_name]
        return GPLVM()
    return GaussianProcess()


def _predictive_moments(bound_u, c_index, x_mean, s_train, y_train_u, xt, st_):
    """Predictive means [N* x D_b] and covariances [D_b x N* x N*] of the kernels of bound_u (the unobserved views / dims) at
    q(X*) (gaussian_process.py:495-536, :920-988), from the training q(X) = (x_mean, s_train) and training outputs y_train_u
    [N x D_b] of each kernel.  Training Psi statistics and factors are formed once per call, in fp64.  c_index[b]: the kernel
    whose training C = L_A^-1 L^-1 Psi1^T enters kernel b's mean (b itself; the reference's MRD uses the last training view's C
    for every view, gaussian_process.py:938)."""
    psi_1, psi_2 = bound_u.psi(x_mean, s_train)
    r0 = collapsed.Chain(bound_u.li, psi_2, bound_u.beta, bound_u.eye).r0                      # L_A^-1 L^-1 (training)
    psi_1t, psi_2t = bound_u.psi(xt, st_)
    n_t = xt.shape[0]
    c_tr = ops.matmul(r0, psi_1.transpose(1, 2))                                             # [B, M, N]
    c_pred = ops.matmul(r0, psi_1t.transpose(1, 2))                                          # [B, M, N*]
    means, covars = [], []
    p = collapsed.precision(r0)                                                              # (K_uu + beta Psi2)^-1
    gmat = psi_2t - ops.matmul(psi_1t.transpose(1, 2), psi_1t)
    tr = torch.diagonal(ops.matmul(bound_u.kinv - p, psi_2t), dim1=-2, dim2=-1).sum(-1)
    for b, y_u in enumerate(y_train_u):
        be, al = bound_u.beta[b], bound_u.alpha[b]
        cy = ops.matmul(c_tr[c_index[b]], y_u)                                               # [M, D_b]
        means.append(be * ops.matmul(c_pred[b].transpose(0, 1), cy))
        scale = ops.matmul(p[b], ops.matmul(psi_1[b].transpose(0, 1), y_u))                 # [M, D_b]
        var = be * be * torch.sum(scale * ops.matmul(gmat[b], scale), dim=0)                 # diag(scale^T g scale)
        eye = torch.eye(n_t, dtype=TORCH_DTYPE, device=xt.device)
        covars.append(var[:, None, None] + (al * n_t + 1.0 / be - tr[b]) * eye)
    return means, covars


def _hyper_raw(q, kernel, iv, device):
    if kernel is not None:
        hp = kernel.hyperparameters
        iv.setdefault('gamma', hp[KernelHyperparameters.ARD_WEIGHTS].detach().cpu().numpy())
        iv.setdefault('alpha', hp[KernelHyperparameters.SIGNAL_VARIANCE].detach().cpu().numpy())
        iv.setdefault('beta', hp[KernelHyperparameters.NOISE_PRECISION].detach().cpu().numpy())
    pick = lambda key, default, shape: np.asarray(iv.get(key, default), dtype=np.float64).reshape(shape)
    vals = dict(gamma_raw=pick('gamma', np.full((1, q), GP_INIT_GAMMA), (1, q)), alpha_raw=pick('alpha', GP_INIT_ALPHA, (1, 1)),
                beta_raw=pick('beta', GP_INIT_BETA, (1, 1)))
    for k, v in vals.items():
        assert np.all(v > 0), 'Initial value must be positive.'
    return {k: _as_device(inverse_softplus(v), device).requires_grad_() for k, v in vals.items()}


def gp_regression(x_train, y_train, kernel=None, device=None, initial_values=None):
    """
    Exact GP regression (reference src/models/gaussian_process.py:22-107): one ARD-RBF kernel (gamma [1 x Q], alpha,
    beta [1 x 1], softplus of raw variables) shared by the D outputs;
        log_likelihood_d = log N(y_d | 0, K_xx) + kernel.prior_log_likelihood,   objective = -sum_d log_likelihood_d.
    :param x_train: [N x Q] inputs (fixed).  :param y_train: [N x D] outputs.  :param kernel: optional k_ard_rbf with batch
    size 1 whose hyper-parameter VALUES initialise the model's own trainable ones.
    Extensions: device, initial_values (gamma, alpha, beta: values).  Everything is fp64; Q <= 30 (the gram's bound).
    """
    device = torch.device(device) if device is not None else default_device()
    x = _as_device(x_train, device)
    y = _as_device(y_train, device)
    assert x.dim() == 2 and y.dim() == 2 and x.shape[0] == y.shape[0], 'x_train must be [N x Q] and y_train [N x D]'
    raw = _hyper_raw(x.shape[1], kernel, dict(initial_values or {}), device)
    return _gaussian_process(x, y, raw, None, device)


def gp_lvm(y_train, kernel=None, num_latent_dims=GP_LVM_DEFAULT_LATENT_DIMENSIONS, device=None, initial_values=None):
    """
    Point-estimate GP-LVM (reference src/models/gaussian_process.py:110-129): gp_regression on a trainable latent input X
    [N x Q] that starts from the PCA of y_train.  No prior or KL term on X (as the reference).
    Extensions: device, initial_values (x_latent [N x Q]; gamma, alpha, beta: values); latent_input is X.
    """
    d = np.shape(y_train)[1]
    assert 0 < num_latent_dims < d, \
        'Number of latent dimensions must be postive and less than the dimensionality of the observed data.'
    device = torch.device(device) if device is not None else default_device()
    iv = dict(initial_values or {})
    y = _as_device(y_train, device)
    x0 = iv['x_latent'] if 'x_latent' in iv else pca(y.cpu().numpy(), num_latent_dimensions=num_latent_dims)
    x = _as_device(x0, device, (y.shape[0], num_latent_dims)).requires_grad_()
    raw = dict(x_latent=x)
    raw.update(_hyper_raw(num_latent_dims, kernel, iv, device))
    return _gaussian_process(x, y, raw, 'x_latent', device)


def bayesian_gp_lvm(y_train, kernel=None, num_latent_dims=GP_LVM_DEFAULT_LATENT_DIMENSIONS,
                    num_inducing_points=GP_LVM_DEFAULT_NUM_INDUCING_POINTS, num_latent_samples=0,
                    device=None, precision=None, initial_values=None, observed=None):
    """
    :param y_train: [N x D] numpy array.  :param kernel: optional k_ard_rbf with batch size 1 whose hyper-parameter VALUES
    initialise the model's own trainable ones.  :param num_latent_dims: Q.  :param num_inducing_points: M (< N).
    :param num_latent_samples: must be 0 (closed-form psi statistics).
    Extensions: device, precision ('mixed' | 'f64'), initial_values (x_mean, x_var, x_u, gamma, alpha, beta: values).

    observed (extension): a boolean [N x D] mask of the entries of y_train that were measured, any pattern with at least one
    True (utils.missing.observed_mask(y) makes it; entries where it is False are ignored and may be NaN).  The model is then
    the masked fp64 model (precision None or 'f64'): output dim d enters the bound with the rows at which it was measured,
    columns of one row pattern share a slot of the weighted operators (models/masked_bound.py), a column never observed is
    left out, a row never observed contributes only its KL.  The objective is -(sum_slots f_b - KL(q(X)) over all N rows +
    hyper-prior); gradients() returns the same six raw variables.  x_mean defaults to the PCA of y_train with its gaps filled
    by the columns' observed means.  impute_training_data() fills the gaps with the posterior mean; the test-point methods
    work with the masked model's own training-side terms, except predict_missing_data (NotImplementedError).
    """
    num_samples, num_dimensions = np.shape(y_train)
    assert isinstance(num_latent_dims, int), 'Number of latent dimensions must be an integer.'
    assert 0 < num_latent_dims < num_dimensions, \
        'Number of latent dimensions must be postive and less than the dimensionality of the observed data.'
    assert isinstance(num_inducing_points, int), 'Number of inducing points must be an integer.'
    assert 0 < num_inducing_points < num_samples, \
        'Number of inducing points must be positive and less than the number of observations in the observed data.'
    assert isinstance(num_latent_samples, int), 'Number of latent space samples must be an integer.'
    if num_latent_samples:
        raise NotImplementedError('stochastic psi statistics (gaussian_process.py:189-214) are not built')
    iv = dict(initial_values or {})
    if kernel is not None:
        hp = kernel.hyperparameters
        iv.setdefault('gamma', hp[KernelHyperparameters.ARD_WEIGHTS].detach().cpu().numpy())
        iv.setdefault('alpha', hp[KernelHyperparameters.SIGNAL_VARIANCE].detach().cpu().numpy())
        iv.setdefault('beta', hp[KernelHyperparameters.NOISE_PRECISION].detach().cpu().numpy())
    q = num_latent_dims
    train_obs = None
    if observed is not None:
        assert precision in (None, 'f64'), "with observed, precision must be None or 'f64' (the masked model is fp64)"
        train_obs = _missing.check_observed(observed, (num_samples, num_dimensions))
        assert train_obs.any(), 'observed must hold at least one True entry'
    inner_iv = dict(gamma_atoms=np.asarray(iv.get('gamma', np.full((1, q), GP_INIT_GAMMA)), dtype=np.float64).reshape(1, q),
                    alpha_atoms=np.asarray(iv.get('alpha', GP_INIT_ALPHA), dtype=np.float64).reshape(1, 1),
                    beta_atoms=np.asarray(iv.get('beta', GP_INIT_BETA), dtype=np.float64).reshape(1, 1),
                    x_var=np.asarray(iv.get('x_var', np.full((num_samples, q), 0.5)), dtype=np.float64),   # (:218: 0.5, not 1)
                    phi_logits=np.zeros((num_dimensions, 1)))
    for k in ('x_mean', 'x_u'):
        if k in iv:
            inner_iv[k] = iv[k]
    names = ('x_mean', 'x_var', 'x_u', 'gamma_atoms', 'alpha_atoms', 'beta_atoms')
    if train_obs is None:
        inner = dp_gp_lvm_t(y_train, num_latent_dims=num_latent_dims, num_inducing_points=num_inducing_points,
                            truncation_level=1, device=device, precision=precision, initial_values=inner_iv)
    else:
        # the same defaults as dp_gp_lvm_t's, from the PCA of the column-mean-filled data
        dev_m = torch.device(device) if device is not None else default_device()
        np.random.seed(seed=0)
        x_init = np.asarray(inner_iv['x_mean'], dtype=np.float64) if 'x_mean' in inner_iv else \
            pca(_missing.column_mean_filled(y_train, train_obs), num_latent_dimensions=q)
        x_u0 = inner_iv['x_u'] if 'x_u' in inner_iv else np.random.permutation(x_init)[:num_inducing_points] + \
            np.random.normal(loc=0.0, scale=0.01, size=(num_inducing_points, q))
        pos = lambda key, shape: _as_device(inverse_softplus(np.asarray(inner_iv[key], dtype=np.float64).reshape(shape)), dev_m)
        for k in ('gamma_atoms', 'alpha_atoms', 'beta_atoms', 'x_var'):
            assert np.all(np.asarray(inner_iv[k]) > 0), 'Initial value must be positive.'
        inner = MaskedBayesianGPLVM(_missing.zero_filled(y_train, train_obs), train_obs,
                                    dict(x_mean=_as_device(x_init, dev_m, (num_samples, q)), x_var=pos('x_var', (num_samples, q)),
                                         x_u=_as_device(x_u0, dev_m, (num_inducing_points, q)), gamma_atoms=pos('gamma_atoms', (1, q)),
                                         alpha_atoms=pos('alpha_atoms', (1, 1)), beta_atoms=pos('beta_atoms', (1, 1))), dev_m)
    raw = {k: inner.raw[k] for k in names}

    def _gradients():
        g = inner.gradients()                                 # (the DP terms of the one-atom model do not touch these six)
        return {k: g[k] for k in names}

    def _optimise(num_iterations, learning_rate=0.01, callback=None):
        opt = torch.optim.Adam(list(raw.values()), lr=learning_rate)
        for it in range(num_iterations):
            g = _gradients()
            # a failed factorisation or a non-finite gradient raises before Adam steps on it (as dp_gp_lvm_t and MRD do)
            bad = ~torch.stack([torch.isfinite(v).all() for v in g.values()]).all() | (inner.cholesky_info != 0)
            if bool(bad):
                eff = precision or 'f64'
                raise FloatingPointError('iteration %d: failed Cholesky factorisation or non-finite gradient (precision=%r)%s'
                                         % (it, eff, '' if eff == 'f64' else '; use precision="f64"'))
            for k, p_ in raw.items():
                p_.grad = g[k].reshape(p_.shape)
            opt.step()
            if callback is not None:
                callback(it)

    y_np = np.asarray(y_train, dtype=np.float64) if train_obs is None else inner.y0       # (zero where unobserved)
    dev_ = inner.raw['x_mean'].device
    pred_state = {}

    def _init_latents(do, y_test, use_pca, x_test_mean, x_test_var):
        """q(X*) for test points observed in their first `do` output dims; on a mask-trained model the nearest neighbour
        compares over the columns that the training row observed too."""
        def neighbour():
            xm = raw['x_mean'].detach().cpu().numpy()
            if train_obs is None:
                return _latents.l2_neighbour(y_np[:, :do], y_test, xm)
            return _latents.masked_neighbour(y_np[:, :do], train_obs[:, :do], y_test, np.ones(y_test.shape, dtype=bool), xm)
        return _latents.start(y_test.shape[0], num_latent_dims, dev_, x_test_mean, x_test_var, use_pca, y_test, neighbour)

    def _frozen():
        """The trained kernel as a B = 1 test bound's parameters (fp64 values of the raw variables)."""
        with torch.no_grad():
            return ([raw['x_u'].detach()], [F.softplus(raw['gamma_atoms']).detach()], [F.softplus(raw['alpha_atoms']).detach()],
                    [F.softplus(raw['beta_atoms']).detach()])

    def _test_bound(y_test):
        z, g, a, b = _frozen()
        bound = _TestBound.kernels(z, g, a, b, [_as_device(y_test, dev_)], dev_)
        pred_state['bound'] = bound
        return bound

    def _masked(y_test, observed, predict=False, reference_compat=False):
        return _missing.masked_arguments(y_test, observed, num_dimensions, predict, reference_compat)

    def _masked_bound(y0, obs):
        """The test bound whose slots are the column groups of the mask that share one row pattern; all share the one kernel."""
        groups = _missing.group_columns_by_pattern(obs)
        dmax = max(len(c) for c, _ in groups)
        y = np.zeros((len(groups), y0.shape[0], dmax))
        for i, (cols, _) in enumerate(groups):
            y[i, :, :len(cols)] = y0[:, cols]
        z, g, a, b = _frozen()
        bound = _TestBound.slots(z[0], g[0], a[0], b[0], _as_device(y, dev_), [len(c) for c, _ in groups],
                                 _as_device(np.stack([w for _, w in groups]), dev_), dev_)
        pred_state['bound'] = bound
        pred_state['missing_columns'] = _missing.missing_columns(obs)
        return bound

    def _masked_init(y0, obs, use_pca, x_test_mean, x_test_var):
        return _latents.start(
            y0.shape[0], num_latent_dims, dev_, x_test_mean, x_test_var, use_pca, y0,
            lambda: _latents.masked_neighbour(y_np, train_obs, y0, obs, raw['x_mean'].detach().cpu().numpy()))

    def _check_observed(y_test, full):
        y_test = np.asarray(y_test, dtype=np.float64)
        assert y_test.ndim == 2 and y_test.shape[0] >= 1, 'y_test must be [N* x D]'
        if full:
            assert y_test.shape[1] == num_dimensions, \
                'Observed dimensionality for prediction must be equal to the dimensionality of the training data.'
        else:
            assert y_test.shape[1] < num_dimensions, \
                'Observed dimensionality for missing data scenario must be less than the total ' \
                'dimensionality of the training data.'
        return y_test

    def _train_terms():
        t_ = inner.objective_terms                          # (objective_t, f_hat, KL, DP objective, hyper-prior)
        return t_[1], t_[2]

    def _bound_at(y_test, xt, st_):
        f_test, kl_t = _latents.bound_at(_test_bound(y_test), xt, st_)
        with torch.no_grad():
            f_hat, kl = _train_terms()
        return f_hat, kl, f_test, kl_t

    def _test_latent_gradients(y_test, x_test_mean, x_test_var, observed=None):
        if observed is not None:
            bound = _masked_bound(*_masked(y_test, observed))
        else:
            y_test = np.asarray(y_test, dtype=np.float64)
            assert y_test.ndim == 2 and y_test.shape[1] <= num_dimensions, 'y_test must be [N* x Do], Do <= D'
            bound = _test_bound(y_test)
        with torch.no_grad():
            return _latents.ascent_gradient(bound, _latents.latent_values(x_test_mean, dev_, num_latent_dims, bound.n_t),
                                            _latents.latent_values(x_test_var, dev_, num_latent_dims, bound.n_t))

    def _optimise_test_latents(y_test, num_iterations=200, learning_rate=0.01, use_pca=False, x_test_mean=None, x_test_var=None,
                               observed=None):
        if observed is not None:
            y0, obs = _masked(y_test, observed)
            xt, st_ = _masked_init(y0, obs, use_pca, x_test_mean, x_test_var)
            bound = _masked_bound(y0, obs)
        else:
            y_test = np.asarray(y_test, dtype=np.float64)
            assert y_test.ndim == 2 and y_test.shape[1] <= num_dimensions, 'y_test must be [N* x Do], Do <= D'
            xt, st_ = _init_latents(y_test.shape[1], y_test, use_pca, x_test_mean, x_test_var)
            bound = _test_bound(y_test)
        with torch.no_grad():
            return _latents.fit(functools.partial(_latents.ascent_gradient, bound), xt.clone(), st_, num_iterations, learning_rate)

    def _train_marginals():
        """The training side of the per-entry moments (models/marginals.py), formed once per call: the model's own masked bound,
        or the same bound with an all-True mask on a model trained on complete data."""
        z, g, a, b = _frozen()
        bound = inner.bound if train_obs is not None else \
            _MaskedBound(y_np, np.ones((num_samples, num_dimensions), dtype=bool), dev_)
        return _marginals.of_masked_bound(bound, z[0], raw['x_mean'].detach(), F.softplus(raw['x_var']).detach(), g[0], a[0], b[0],
                                          num_dimensions)

    def _marginals_at(xt, st_, columns):
        with torch.no_grad():
            mean, var = _train_marginals().at(xt, st_, _marginals.columns_arg(columns, num_dimensions, dev_))
        return mean[0], var[0]

    def _metric_under(columns, name):
        """latent_geometry's hook: the marginals.Metric under latent_metric(., columns), the training side and (P, prior)
        formed once."""
        cols = _marginals.columns_arg(columns, num_dimensions, dev_)
        with torch.no_grad():
            marg = _train_marginals()
            return _marginals.Metric([(marg,) + marg._metric_operands(cols, None)])

    class BayesianGPLVM(LatentGeometry, Trainable):
        """Accessors as in the reference (gaussian_process.py:276-340), and its two prediction methods (:329-538) with the same
        keywords and return tuples as dp_gp_lvm's, plus test_latent_gradients / optimise_test_latents / prediction_terms.
        Prediction runs in fp64 (the reference's dtype) whatever `precision` the model trains in; the training-side f_hat and
        KL(q(X)) of the bounds are those of the model's own evaluation (mixed Psi statistics when precision='mixed').
        The latent-geometry methods are models/latent_geometry.LatentGeometry's, over the model's one kernel."""
        raw_variables = raw
        _latent_dims, _device, _metric_of = num_latent_dims, dev_, staticmethod(_metric_under)

        @staticmethod
        def predict_new_latent_variables(y_test, use_pca=False, x_test_mean=None, x_test_var=None, reference_compat=False):
            """q(X*) for fully observed test data y_test [N* x D] (gaussian_process.py:329-402).  Returns
                (prediction_lower_bound = f_hat + f_hat* - KL(q(X)) - KL(q(X*)), x_test_mean [N* x Q], x_test_covar [N* x Q x Q],
                 test_log_likelihood = f_hat* - f_hat)
            — the test log-likelihood exactly as the reference defines it (:400, "equation 36"): the training f_hat is
            subtracted and KL(q(X*)) is not.  q(X*) starts at the nearest training neighbour + N(0, 0.01^2) noise, or the PCA of
            y_test (use_pca), or the given x_test_mean / x_test_var (values; variances 1 by default).  reference_compat: accepted
            for symmetry with dp_gp_lvm; the reference's B = 1 bound has no defect to reproduce, so both settings agree."""
            y_test = _check_observed(y_test, True)
            xt, st_ = _init_latents(num_dimensions, y_test, use_pca, x_test_mean, x_test_var)
            f_hat, kl, f_test, kl_t = _bound_at(y_test, xt, st_)
            return f_hat + f_test - kl - kl_t, xt, torch.diag_embed(st_), f_test - f_hat

        @staticmethod
        def predictive_marginals(x_test_mean, x_test_var, columns=None):
            """(mean, var), each [N* x len(columns)]: the per-entry predictive moments of the output dims `columns` (default: all
            D) at q(X*) = (x_test_mean, x_test_var [N* x Q]), observation noise 1/beta included (formulas in models/marginals.py;
            one call of ops.qx_psi_point_moments).  Works on a model trained on complete data and on one trained with
            observed= (column d then sees the training rows at which it was observed; a column never observed in training has
            mean 0 and variance alpha + 1/beta): optimise_test_latents(..., observed=) followed by this is how a mask-trained
            model predicts at test points.  fp64, torch.no_grad."""
            return _marginals_at(_as_device(x_test_mean, dev_), _as_device(x_test_var, dev_), columns)

        @staticmethod
        def frozen_predictor(columns=None):
            """A models/predictor.FrozenPredictor of the output dims `columns` (default: all D): p(x_mean, x_var) gives the bits of
            predictive_marginals, differentiably in q(X*); p.vjp is its vector-Jacobian product (ops.qx_psi_point_moments_adjoint).
            The training side is built once, here, at the model's current parameters: stale after further training."""
            cols = _marginals.columns_arg(columns, num_dimensions, dev_)
            with torch.no_grad():
                return _predictor.of_marginals(_train_marginals(), cols, dev_)

        @staticmethod
        def predictive_jacobian(x, columns=None):
            """[N* x len(columns) x Q]: the mean of the Jacobian d f_d / d x of the noise-free map of the output dims `columns`
            (default: all D) at the DETERMINISTIC latent points x [N* x Q] (numpy or torch): the derivative of
            predictive_marginals' mean at x_test_var = 0 (models/marginals.py; one call of ops.ard_rbf_point_jacobian).
            The training side is built once per call.  fp64, torch.no_grad."""
            cols = _marginals.columns_arg(columns, num_dimensions, dev_)
            with torch.no_grad():
                return _train_marginals().jacobian(_marginals.points_arg(x, num_latent_dims, dev_), cols)[0]

        @staticmethod
        def latent_metric(x, columns=None):
            """[N* x Q x Q]: the expected Riemannian metric G(x) = sum_d E[J_d J_d^T] of the map from latent space to the output
            dims `columns` (default: all D) at the latent points x [N* x Q] (Tosi et al., UAI 2014; formulas in
            models/marginals.py; one call of ops.ard_rbf_point_metric).  Works on a model trained on complete data and on one
            trained with observed= (a column never observed in training contributes its prior alpha diag(gamma)).  fp64."""
            cols = _marginals.columns_arg(columns, num_dimensions, dev_)
            with torch.no_grad():
                return _train_marginals().metric(_marginals.points_arg(x, num_latent_dims, dev_), cols)[0]

        @staticmethod
        def predictive_covariance(x, columns=None, noise=False):
            """[len(columns) x N* x N*]: the joint posterior covariance of the noise-free functions of the output dims `columns`
            (default: all D) at the DETERMINISTIC latent points x [N* x Q] (numpy or torch),
                cov_d(x, x') = alpha exp(-1/2 sum_q gamma_q (x_q - x'_q)^2) - k(x)^T (K_uu^-1 - P_p(d)) k(x')
            (models/marginals.py; one call of ops.ard_rbf_point_cov): the off-diagonal that predictive_marginals leaves out.  Its
            diagonal plus 1/beta is predictive_marginals(x, 0)'s variance; noise=True adds 1/beta on the diagonal.  A column never
            observed in training gets the prior gram.  Exactly symmetric.  The array is J N*^2 doubles, and columns of one training
            row pattern repeat the same matrix.  Works on a model trained on complete data and on one trained with observed=.
            fp64, torch.no_grad."""
            cols = _marginals.columns_arg(columns, num_dimensions, dev_)
            with torch.no_grad():
                return _marginals.covariance_of(_train_marginals(), _marginals.points_arg(x, num_latent_dims, dev_), cols, noise)

        @staticmethod
        def sample_functions(x, num_samples=1, columns=None, noise=False, jitter=_marginals.DEFAULT_SAMPLE_JITTER, seed=0,
                             draws=None):
            """[S x N* x len(columns)]: S joint draws of the output dims `columns` (default: all D) at the latent points x
            [N* x Q]: mean + L xi with L L^T = predictive_covariance + jitter alpha I (+ 1/beta I with noise), xi standard normal
            from a device torch.Generator seeded with `seed`, or given as `draws` [S x N* x len(columns)].  One
            ops.potrf_batched call over the training row patterns and one ops.matmul, whatever the number of columns; one host
            read, potrf's info at the end: FloatingPointError if a factorisation failed (raise `jitter` or set noise=True).
            The default jitter, 1e-6 alpha, is a choice, not a measurement: the gram of nearby points has its smallest eigenvalue
            below rounding and the factorisation needs a shift well above eps N* lambda_max ~ 1e-12 alpha; 1e-6 alpha is far
            above that and far below any 1/beta the models train to.  fp64, torch.no_grad."""
            cols = _marginals.columns_arg(columns, num_dimensions, dev_)
            with torch.no_grad():
                return _marginals.samples_of(_train_marginals(), _marginals.points_arg(x, num_latent_dims, dev_), cols, num_samples,
                                             noise, jitter, seed, draws)

        @staticmethod
        def predict_missing_data(y_test, use_pca=False, x_test_mean=None, x_test_var=None, reference_compat=False,
                                 observed=None, marginal_variance=False):
            """y_test [N* x Do] holds the FIRST Do < D output dims of the test points (gaussian_process.py:405-538).  Returns
                (missing_data_lower_bound, x_test_mean, x_test_covar, predicted_mean [N* x Du], predicted_covar [Du x N* x N*])
            for the remaining Du = D - Do dims, at the initial q(X*) of predict_new_latent_variables (nearest neighbour over
            the observed dims).  The predictive moments are the reference's (:495-536), composed of the library's operators;
            reference_compat: as predict_new_latent_variables (no effect).

            observed (extension): a boolean [N* x D] mask of the entries of y_test [N* x D] that were measured, any pattern
            (entries where it is False are ignored and may be NaN).  The bound is f_hat + f_hat*(masked) - KL(q(X)) - KL(q(X*)):
            output dim d enters f_hat* with the test points at which it was measured (columns of one row pattern share a slot
            of the weighted test-point operators); KL(q(X*)) runs over all N* rows.  The Du predicted dims are then the columns
            with at least one unobserved entry, ascending (property missing_columns); their moments are the same formulas and
            depend on the mask only through q(X*), which starts at the masked nearest neighbour (smallest mean squared
            difference over each row's observed columns; a row with nothing observed starts at 0).  AssertionError for a
            non-boolean mask, a shape mismatch, a mask that is True everywhere, or reference_compat=True.

            marginal_variance=True (extension): the last entry is the per-entry variance [N* x Du] of predictive_marginals on
            the predicted dims in place of the [Du x N* x N*] array (one scalar per dim plus a diagonal, the same for every
            test point).

            On a model trained with observed= this method is not built: NotImplementedError (predictive_marginals gives the
            moments at test points, impute_training_data fills the training data's own gaps)."""
            if train_obs is not None:
                raise NotImplementedError('predict_missing_data is not built for a model trained with observed=: use '
                                          'impute_training_data for the gaps of the training data')
            if observed is not None:
                y0, obs = _masked(y_test, observed, predict=True, reference_compat=reference_compat)
                xt, st_ = _masked_init(y0, obs, use_pca, x_test_mean, x_test_var)
                bound = _masked_bound(y0, obs)
                mc = pred_state['missing_columns']
                f_test, kl_t = _latents.bound_at(bound, xt, st_)
                with torch.no_grad():
                    f_hat, kl = _train_terms()
                    z, g, a, b = _frozen()
                    plain = _TestBound.kernels(z, g, a, b, [torch.zeros((y0.shape[0], 1), dtype=TORCH_DTYPE, device=dev_)], dev_)
                    means, covars = _predictive_moments(plain, [0], raw['x_mean'].detach(), F.softplus(raw['x_var']).detach(),
                                                        [_as_device(y_np[:, mc], dev_)], xt, st_)
                covar = _marginals_at(xt, st_, mc)[1] if marginal_variance else covars[0]
                return f_hat + f_test - kl - kl_t, xt, torch.diag_embed(st_), means[0], covar
            y_test = _check_observed(y_test, False)
            do = y_test.shape[1]
            pred_state['missing_columns'] = np.arange(do, num_dimensions)
            xt, st_ = _init_latents(do, y_test, use_pca, x_test_mean, x_test_var)
            f_hat, kl, f_test, kl_t = _bound_at(y_test, xt, st_)
            bound = pred_state['bound']
            with torch.no_grad():
                means, covars = _predictive_moments(bound, [0], raw['x_mean'].detach(), F.softplus(raw['x_var']).detach(),
                                                    [_as_device(y_np[:, do:], dev_)], xt, st_)
            covar = _marginals_at(xt, st_, pred_state['missing_columns'])[1] if marginal_variance else covars[0]
            return f_hat + f_test - kl - kl_t, xt, torch.diag_embed(st_), means[0], covar

        @staticmethod
        def test_latent_gradients(y_test, x_test_mean, x_test_var, observed=None):
            """d(f_hat* - KL(q(X*))) / d(x_test_mean, x_test_var) [N* x Q] each — the gradient of either prediction bound with
            respect to q(X*) (mean and diagonal variances), the trained model fixed; y_test [N* x Do], Do <= D (the first Do
            output dims).  One qx_psi_stats_batched + dense chain + qx_psi_adjoint, fp64.  observed: as predict_missing_data
            (y_test [N* x D]; True everywhere is allowed here)."""
            return _test_latent_gradients(y_test, x_test_mean, x_test_var, observed)

        @staticmethod
        def optimise_test_latents(y_test, num_iterations=200, learning_rate=0.01, use_pca=False, x_test_mean=None,
                                  x_test_var=None, observed=None):
            """Adam on q(X*) (the mean and softplus-parametrised variances) maximising f_hat* - KL(q(X*)) for test points
            observed in their first Do output dims; returns (x_test_mean, x_test_var) to hand to predict_*.  K_uu and its factor
            are formed once; no host synchronisation inside the loop.  observed: as predict_missing_data."""
            return _optimise_test_latents(y_test, num_iterations, learning_rate, use_pca, x_test_mean, x_test_var, observed)

        @property
        def missing_columns(self):
            """The output dims whose moments the last predict_missing_data returned (ascending), or None."""
            return pred_state.get('missing_columns')

        @property
        def prediction_terms(self):
            """[slots x 5] terms of f_hat* in the last prediction evaluation: 1/2 N* D (log beta - log 2 pi), -D log|L_A|,
            1/2 D beta (tr(K_uu^-1 Psi2*) - alpha N*), 1/2 beta^2 |C* Y*|^2, -1/2 beta |Y*|^2."""
            b = pred_state.get('bound')
            return None if b is None else b.terms

        @staticmethod
        def impute_training_data(return_variance=False):
            """A model trained with observed=: y_train [N x D] with every unobserved entry (n, d) replaced by the posterior mean
            beta Psi1[n,:] (K_uu + beta Psi2_d)^-1 Psi1^T y_d (Psi2_d and y_d over the rows at which d was observed); observed
            entries as given, a never-observed column 0.  fp64 device tensor.  return_variance=True: (filled, var), var
            [N x D] the per-entry predictive variance of predictive_marginals at the training q(X) at the unobserved entries
            and 0 at the observed ones; filled is the same tensor either way."""
            assert train_obs is not None, 'impute_training_data needs a model trained with observed='
            filled = inner.impute()
            if not return_variance:
                return filled
            var = _marginals_at(raw['x_mean'].detach(), F.softplus(raw['x_var']).detach(), None)[1]
            return filled, _marginals.unobserved_variance(var, train_obs)

        @property
        def objective_terms(self):
            """A model trained with observed=: the [slots x 5] terms of sum_slots f_b in the last evaluation (as prediction_terms,
            with N_b for N*); None for a model trained on complete data."""
            return None if train_obs is None else inner.bound.terms

        @property
        def kernel(self):
            return k_ard_rbf(gamma=F.softplus(raw['gamma_atoms']), alpha=F.softplus(raw['alpha_atoms']),
                             beta=F.softplus(raw['beta_atoms']))

        @property
        def ard_weights(self):
            return F.softplus(raw['gamma_atoms'])

        @property
        def signal_variance(self):
            return F.softplus(raw['alpha_atoms'])

        @property
        def noise_precision(self):
            return F.softplus(raw['beta_atoms'])

        @property
        def inducing_input(self):
            return raw['x_u']

        @property
        def q_x(self):
            return raw['x_mean'], torch.diag_embed(F.softplus(raw['x_var']))

        @property
        def objective(self):
            """-(f_hat - KL + hyper-prior) (gaussian_process.py:263-269): 0-d fp64 device tensor."""
            t = inner.objective_terms                           # (objective_t, f_hat, KL, DP objective, hyper-prior)
            return t[0] - t[3]

        gradients = staticmethod(_gradients)
        optimise = staticmethod(_optimise)

    return BayesianGPLVM()


class _MaskedView:
    """One view of a mask-trained MRD as the accessors and the test bounds see it: the view's four raw variables."""

    def __init__(self, raw):
        self.raw = raw

    @property
    def kernel(self):
        return k_ard_rbf(gamma=F.softplus(self.raw['gamma_atoms']), alpha=F.softplus(self.raw['alpha_atoms']),
                         beta=F.softplus(self.raw['beta_atoms']))


def manifold_relevance_determination(views_train, num_latent_dims=GP_LVM_DEFAULT_LATENT_DIMENSIONS,
                                     num_inducing_points=GP_LVM_DEFAULT_NUM_INDUCING_POINTS,
                                     device=None, precision=None, initial_values=None, observed=None):
    """
    Manifold relevance determination — mirror of the reference's factory (src/models/gaussian_process.py:551-664): V views
    [N x D_v] share q(X); every view has its own B = 1 ARD-RBF kernel and its own M inducing inputs, and
        objective = -( sum_v f_hat_v - KL(q(X)||p(X)) + sum_v kernel_v.prior_log_likelihood )                      (:653-664)
    with f_hat_v the Bayesian GP-LVM's f_hat of view v (:619-651 = :236-258).  Like ``bayesian_gp_lvm`` it needs no new kernels:
    every view is a one-atom ``dp_gp_lvm_t`` (library operators forward, its streaming stage B backward) whose q(X) tensors
    are the SAME storage; the shared KL is counted once.
    Extensions: device, precision ('mixed' | 'f64'), initial_values (x_mean, x_var [N x Q]; gamma, alpha, beta, x_u: lists
    with one entry per view).

    observed (extension): a list of V entries, each None (the view is complete) or a boolean [N x D_v] mask of the entries of
    view v that were measured (entries where it is False are ignored and may be NaN); every view needs at least one True.
    The model is then the masked fp64 model (precision None or 'f64', models/masked_bound.py): within a view the columns of
    one row pattern share a slot of the weighted operators, the slots of view v use kernel v, a column never observed is left
    out and a row observed in no view keeps only its KL.  The objective is -(sum_v sum_{b in v} f_b - KL(q(X)) over all N rows
    + sum_v hyper-prior_v); raw_variables and gradients() keep the unmasked model's names, shapes and order.  x_mean defaults
    to the PCA of the stacked views with their gaps filled by the columns' observed means.  impute_training_data() fills the
    gaps with the posterior mean; the test-point methods work with the masked model's own training-side terms, except
    predict_missing_data (NotImplementedError).
    """
    num_views = len(views_train)
    shapes = np.array([np.shape(v) for v in views_train])
    num_samples = [shapes[v][0] for v in range(num_views)]
    num_dimensions = [int(shapes[v][1]) for v in range(num_views)]
    assert np.size(np.unique(num_samples)) == 1, 'Each view must have the same number of observations.'
    num_samples = int(num_samples[0])
    assert 0 < num_latent_dims < np.sum(num_dimensions), \
        'Number of latent dimensions must be postive and less than the dimensionality of the observed data.'
    assert 0 < num_inducing_points < num_samples, \
        'Number of inducing points must be positive and less than the number of observations in the observed data.'
    iv = dict(initial_values or {})
    q, m = num_latent_dims, num_inducing_points
    train_obs = None
    if observed is not None:
        assert precision in (None, 'f64'), "with observed, precision must be None or 'f64' (the masked model is fp64)"
        assert isinstance(observed, (list, tuple)) and len(observed) == num_views, 'observed must be a list with one entry per view'
        train_obs = [np.ones((num_samples, num_dimensions[v]), dtype=bool) if o is None else
                     _missing.check_observed(o, (num_samples, num_dimensions[v])) for v, o in enumerate(observed)]
        assert all(o.any() for o in train_obs), 'every view must hold at least one True entry'
    x_init = np.asarray(iv['x_mean'], dtype=np.float64) if 'x_mean' in iv else \
        pca(np.hstack([np.asarray(v) for v in views_train] if train_obs is None else
                      [_missing.column_mean_filled(v, o) for v, o in zip(views_train, train_obs)]),
            num_latent_dimensions=q)                                                                            # (:591)
    x_var = np.asarray(iv.get('x_var', np.ones((num_samples, q))), dtype=np.float64)                            # (:593: 1.0)
    inner = []
    dev_m = torch.device(device) if device is not None else default_device()
    masked_raw = {}
    if train_obs is not None:
        assert np.all(x_var > 0), 'Initial value must be positive.'
        masked_raw = dict(x_mean=_as_device(x_init, dev_m, (num_samples, q)),
                          x_var=_as_device(inverse_softplus(x_var), dev_m, (num_samples, q)))
    for v in range(num_views):
        x_u = np.asarray(iv['x_u'][v], dtype=np.float64) if 'x_u' in iv else \
            np.random.permutation(x_init)[:m] + np.random.normal(loc=0.0, scale=0.01, size=(m, q))              # (:599-601)
        pick = lambda key, default, shape: np.asarray(iv[key][v] if key in iv else default, dtype=np.float64).reshape(shape)
        if train_obs is not None:
            masked_raw['x_u_%d' % v] = _as_device(x_u, dev_m, (m, q))
            for k, key, default, shape in (('gamma_atoms', 'gamma', np.full((1, q), GP_INIT_GAMMA), (1, q)),
                                           ('alpha_atoms', 'alpha', GP_INIT_ALPHA, (1, 1)), ('beta_atoms', 'beta', GP_INIT_BETA, (1, 1))):
                val = pick(key, default, shape)
                assert np.all(val > 0), 'Initial value must be positive.'
                masked_raw['%s_%d' % (k, v)] = _as_device(inverse_softplus(val), dev_m)
            continue
        inner.append(dp_gp_lvm_t(np.asarray(views_train[v]), num_latent_dims=q, num_inducing_points=m, truncation_level=1,
                                 device=device, precision=precision, _view_of_many=True,
                                 initial_values=dict(x_mean=x_init, x_var=x_var, x_u=x_u,
                                                     gamma_atoms=pick('gamma', np.full((1, q), GP_INIT_GAMMA), (1, q)),
                                                     alpha_atoms=pick('alpha', GP_INIT_ALPHA, (1, 1)),
                                                     beta_atoms=pick('beta', GP_INIT_BETA, (1, 1)),
                                                     phi_logits=np.zeros((num_dimensions[v], 1)))))
    per_view = ('x_u', 'gamma_atoms', 'alpha_atoms', 'beta_atoms')
    masked = None
    if train_obs is not None:
        views_zero = [_missing.zero_filled(v, o) for v, o in zip(views_train, train_obs)]
        masked = MaskedMRD(views_zero, train_obs, masked_raw, dev_m)
        inner = [_MaskedView({k: masked_raw['%s_%d' % (k, v)] for k in per_view}) for v in range(num_views)]
        x_mean_t, x_var_raw = masked_raw['x_mean'], masked_raw['x_var']
    else:
        x_mean_t, x_var_raw = inner[0].raw['x_mean'], inner[0].raw['x_var']
        for mv in inner[1:]:                                 # one q(X): same storage in every view's model
            mv.raw['x_mean'].data = x_mean_t.data
            mv.raw['x_var'].data = x_var_raw.data
    raw = dict(x_mean=x_mean_t, x_var=x_var_raw)
    for v, mv in enumerate(inner):
        for k in per_view:
            raw['%s_%d' % (k, v)] = mv.raw[k]

    def _train_terms():
        """(sum_v f_hat_v, KL(q(X))) of the model's own evaluation."""
        if masked is not None:
            _, f_hat, kl, _ = masked.terms()
            return f_hat, kl
        terms = [mv.objective_terms for mv in inner]        # (objective_t, f_hat, KL, DP objective, hyper-prior) per view
        return sum(t_[1] for t_ in terms), terms[0][2]

    def _objective():
        if masked is not None:
            return masked.terms()[0]
        terms = [mv.objective_terms for mv in inner]          # (objective_t, f_hat, KL, DP objective, hyper-prior) per view
        return sum(t[0] - t[3] for t in terms) - (num_views - 1) * terms[0][2]

    def _gradients():
        if masked is not None:
            return masked.gradients()
        g = [mv.gradients() for mv in inner]
        s_ = F.softplus(x_var_raw)
        out = dict(x_mean=sum(gv['x_mean'] for gv in g) - (num_views - 1) * x_mean_t,          # KL counted once:
                   x_var=sum(gv['x_var'] for gv in g) -                                           # gp_expressions.py:10-24
                   (num_views - 1) * 0.5 * (1.0 - 1.0 / s_) * torch.sigmoid(x_var_raw))
        for v, gv in enumerate(g):
            for k in per_view:
                out['%s_%d' % (k, v)] = gv[k]
        return out

    def _optimise(num_iterations, learning_rate=0.01, callback=None):
        opt = torch.optim.Adam(list(raw.values()), lr=learning_rate)
        for it in range(num_iterations):
            g = _gradients()
            bad = ~torch.stack([torch.isfinite(v).all() for v in g.values()]).all()
            for mv in inner if masked is None else [masked]:
                bad = bad | (mv.cholesky_info != 0)
            if bool(bad):
                eff = precision or 'f64'                        # (None resolves to the reference's fp64 in the models it builds)
                raise FloatingPointError('iteration %d: failed Cholesky factorisation or non-finite gradient (precision=%r)%s'
                                         % (it, eff, '' if eff == 'f64' else '; use precision="f64"'))
            for k, p_ in raw.items():
                p_.grad = g[k].reshape(p_.shape)
            opt.step()
            if callback is not None:
                callback(it)

    views_np = [np.asarray(v, dtype=np.float64) for v in views_train] if masked is None else views_zero
    dev_ = x_mean_t.device
    pred_state = {}

    def _frozen(ks):
        return ([mv.raw['x_u'].detach() for mv in ks], [F.softplus(mv.raw['gamma_atoms']).detach() for mv in ks],
                [F.softplus(mv.raw['alpha_atoms']).detach() for mv in ks], [F.softplus(mv.raw['beta_atoms']).detach() for mv in ks])

    def _test_bound(views_test):
        """Test bound of the first len(views_test) kernels (the observed views)."""
        with torch.no_grad():
            bound = _TestBound.kernels(*_frozen(inner[:len(views_test)]), [_as_device(v, dev_) for v in views_test], dev_)
        pred_state['bound'] = bound
        return bound

    def _check_views(views_test, missing):
        vo = len(views_test)
        if missing:
            assert 0 < vo < num_views, \
                'The number of test views for the missing data scenario must be less than the number of training views.'
        else:
            assert vo == num_views, 'The number of test views must be the same as the number of training views.'
        views_test = [np.asarray(v, dtype=np.float64) for v in views_test]
        assert all(v.ndim == 2 for v in views_test), 'Each test view must be [N* x D_v].'
        assert np.size(np.unique([v.shape[0] for v in views_test])) == 1 and views_test[0].shape[0] >= 1, \
            'Each view must have the same number of test points.'
        assert [v.shape[1] for v in views_test] == num_dimensions[:vo], \
            'Observed dimensionality for prediction must be equal to the dimensionality of the training data for each ' \
            'observed view.'
        return views_test

    def _bound_at(views_test, xt, st_):
        f_test, kl_t = _latents.bound_at(_test_bound(views_test), xt, st_)
        with torch.no_grad():
            f_hat, kl = _train_terms()
        return f_hat + f_test - kl - kl_t

    def _init(views_test, use_pca, x_test_mean, x_test_var):
        vo, y_t = len(views_test), np.hstack(views_test)

        def neighbour():
            xm = x_mean_t.detach().cpu().numpy()
            if masked is None:
                return _latents.l2_neighbour(np.hstack(views_np[:vo]), y_t, xm)
            return _latents.masked_neighbour(np.hstack(views_np[:vo]), np.hstack(train_obs[:vo]), y_t,
                                             np.ones(y_t.shape, dtype=bool), xm)
        return _latents.start(y_t.shape[0], q, dev_, x_test_mean, x_test_var, use_pca, y_t, neighbour)

    def _masked(views_test, observed, predict=False, reference_compat=False):
        """The argument checks of the observed= paths; returns (the V test views zero-filled where unobserved, the V masks)."""
        assert not reference_compat, 'reference_compat has no meaning with observed: the reference has no per-entry masks'
        assert isinstance(observed, (list, tuple)) and len(observed) == num_views and len(views_test) == num_views, \
            'with observed, views_test and observed must be lists with one entry per training view'
        views_test = [np.asarray(v, dtype=np.float64) for v in views_test]
        assert all(v.ndim == 2 for v in views_test) and views_test[0].shape[0] >= 1 and \
            [v.shape for v in views_test] == [(views_test[0].shape[0], d) for d in num_dimensions], \
            'with observed, each test view must be [N* x D_v]'
        obs = [np.ones(y.shape, dtype=bool) if o is None else _missing.check_observed(o, y.shape)
               for y, o in zip(views_test, observed)]
        assert any(o.any() for o in obs), 'observed must hold at least one True entry'
        if predict:
            assert not all(o.all() for o in obs), \
                'observed is True everywhere: nothing is missing (use predict_new_latent_variables)'
        return [_missing.zero_filled(y, o) for y, o in zip(views_test, obs)], obs

    def _masked_bound(y0s, obs):
        """The test bound whose slots are, per view, the column groups of its mask that share one row pattern (a view whose mask
        is all False has none); the slots of view v use kernel v."""
        slots = [(v, cols, w) for v in range(num_views) for cols, w in _missing.group_columns_by_pattern(obs[v])]
        dmax = max(len(c) for _, c, _ in slots)
        y = np.zeros((len(slots), y0s[0].shape[0], dmax))
        for i, (v, cols, _) in enumerate(slots):
            y[i, :, :len(cols)] = y0s[v][:, cols]
        with torch.no_grad():
            bound = kernel_slots(*_frozen(inner), [v for v, _, _ in slots], _as_device(y, dev_), [len(c) for _, c, _ in slots],
                                 _as_device(np.stack([w for _, _, w in slots]), dev_), dev_)
        pred_state['bound'] = bound
        pred_state['missing_views'] = [v for v in range(num_views) if not obs[v].all()]
        pred_state['missing_columns'] = [_missing.missing_columns(obs[v]) for v in pred_state['missing_views']]
        return bound

    def _masked_init(y0s, obs, use_pca, x_test_mean, x_test_var):
        y_t, o_t = np.hstack(y0s), np.hstack(obs)
        return _latents.start(
            y_t.shape[0], q, dev_, x_test_mean, x_test_var, use_pca, y_t,
            lambda: _latents.masked_neighbour(np.hstack(views_np), None if masked is None else np.hstack(train_obs), y_t, o_t,
                                              x_mean_t.detach().cpu().numpy()))

    def _test_latent_gradients(views_test, x_test_mean, x_test_var, observed=None):
        if observed is not None:
            bound = _masked_bound(*_masked(views_test, observed))
        else:
            views_test = [np.asarray(v, dtype=np.float64) for v in views_test]
            assert 0 < len(views_test) <= num_views and [v.shape[1] for v in views_test] == num_dimensions[:len(views_test)], \
                'views_test must be the first Vo <= V views, each [N* x D_v]'
            bound = _test_bound(views_test)
        with torch.no_grad():
            return _latents.ascent_gradient(bound, _latents.latent_values(x_test_mean, dev_, q, bound.n_t),
                                            _latents.latent_values(x_test_var, dev_, q, bound.n_t))

    def _optimise_test_latents(views_test, num_iterations=200, learning_rate=0.01, use_pca=False, x_test_mean=None,
                               x_test_var=None, observed=None):
        if observed is not None:
            y0s, obs = _masked(views_test, observed)
            xt, st_ = _masked_init(y0s, obs, use_pca, x_test_mean, x_test_var)
            bound = _masked_bound(y0s, obs)
        else:
            views_test = [np.asarray(v, dtype=np.float64) for v in views_test]
            assert 0 < len(views_test) <= num_views and [v.shape[1] for v in views_test] == num_dimensions[:len(views_test)], \
                'views_test must be the first Vo <= V views, each [N* x D_v]'
            xt, st_ = _init(views_test, use_pca, x_test_mean, x_test_var)
            bound = _test_bound(views_test)
        with torch.no_grad():
            return _latents.fit(functools.partial(_latents.ascent_gradient, bound), xt.clone(), st_, num_iterations, learning_rate)

    def _train_marginals():
        """The training side of the per-entry moments of every view (models/marginals.py), formed once per call: the model's own
        masked bound, or the same bound with all-True masks on a model trained on complete views."""
        z, g, a, b = _frozen(inner)
        bound = masked.bound if masked is not None else \
            _MaskedViewsBound(views_np, [np.ones(v.shape, dtype=bool) for v in views_np], dev_)
        flat = lambda ts: torch.stack([t.reshape(-1) for t in ts]).contiguous()
        return _marginals.of_masked_views_bound(bound, torch.stack(z).contiguous(), x_mean_t.detach(),
                                                F.softplus(x_var_raw).detach(), flat(g), flat(a).reshape(-1), flat(b).reshape(-1),
                                                num_dimensions)

    def _marginals_at(xt, st_, views, columns=None):
        """Two lists (means, variances) over `views`; columns[i]: the columns of views[i] (default all)."""
        with torch.no_grad():
            train = _train_marginals()
            out = [train[v].at(xt, st_, _marginals.columns_arg(None if columns is None else columns[i], num_dimensions[v], dev_))
                   for i, v in enumerate(views)]
        return [o[0][0] for o in out], [o[1][0] for o in out]

    def _views_arg(views):
        vs = list(range(num_views)) if views is None else [int(v) for v in views]
        assert vs and all(0 <= v < num_views for v in vs), 'views must be view indices in [0, V)'
        return vs

    def _metrics_under(views, total):
        """latent_geometry's hook: the marginals.Metric of every view of `views`, or with total the one of their sum (one part
        per view), the training side and every view's (P, prior) formed once."""
        vs = _views_arg(views)
        with torch.no_grad():
            train = _train_marginals()
            parts = [(train[v],) + train[v]._metric_operands(None, None) for v in vs]
            return [_marginals.Metric(parts)] if total else [_marginals.Metric([part]) for part in parts]

    class ManifoldRelevanceDetermination(ViewsLatentGeometry, Trainable):
        """Accessors as in the reference (gaussian_process.py:667-727), its two prediction methods (:729-990) and
        test_latent_gradients / optimise_test_latents / prediction_terms as bayesian_gp_lvm's, with lists of views in place of
        y_test: the first Vo views are observed.  Prediction runs in fp64 (the reference's dtype) whatever `precision` the
        model trains in; the training-side f_hat and KL(q(X)) are those of the model's own evaluation.
        The latent-geometry methods are models/latent_geometry.ViewsLatentGeometry's, every view under its own kernel."""
        raw_variables = raw
        _latent_dims, _device, _metrics_of = num_latent_dims, dev_, staticmethod(_metrics_under)

        @staticmethod
        def predict_new_latent_variables(views_test, use_pca=False, x_test_mean=None, x_test_var=None, reference_compat=False):
            """q(X*) for test points observed in every view, views_test: V arrays [N* x D_v] (gaussian_process.py:729-832).
            Returns (prediction_lower_bound = sum_v f_hat_v + sum_v f_hat*_v - KL(q(X)) - KL(q(X*)), x_test_mean [N* x Q],
            x_test_covar [N* x Q x Q]) — the reference's 3-tuple.  q(X*) starts as in bayesian_gp_lvm (nearest neighbour over
            all views' columns).  reference_compat: no defect in this bound (both settings agree)."""
            views_test = _check_views(views_test, False)
            xt, st_ = _init(views_test, use_pca, x_test_mean, x_test_var)
            return _bound_at(views_test, xt, st_), xt, torch.diag_embed(st_)

        @staticmethod
        def predictive_marginals(x_test_mean, x_test_var, views=None):
            """(means, variances): two lists with one tensor [N* x D_v] per view of `views` (default: all V, in order): the
            per-entry predictive moments at q(X*) = (x_test_mean, x_test_var [N* x Q]), observation noise 1/beta_v included
            (formulas in models/marginals.py; one call of ops.qx_psi_point_moments per view).  Works on a model trained on
            complete views and on one trained with observed= (column d of view v then sees the training rows at which it was
            observed; a column never observed in training has mean 0 and variance alpha_v + 1/beta_v):
            optimise_test_latents(..., observed=) followed by this is how a mask-trained model predicts at test points.
            fp64, torch.no_grad."""
            vs = _views_arg(views)
            return _marginals_at(_as_device(x_test_mean, dev_), _as_device(x_test_var, dev_), vs)

        @staticmethod
        def frozen_predictor(views=None):
            """One models/predictor.FrozenPredictor per view of `views` (default: all V, in order), each over all D_v columns of its
            view: p(x_mean, x_var) gives the bits of that view's predictive_marginals, differentiably in q(X*); p.vjp is its
            vector-Jacobian product.  The training side of all views is built once, here, at the model's current parameters: stale
            after further training."""
            vs = _views_arg(views)
            with torch.no_grad():
                train = _train_marginals()
                return [_predictor.of_marginals(train[v], _marginals.columns_arg(None, num_dimensions[v], dev_), dev_) for v in vs]

        @staticmethod
        def predictive_jacobian(x, views=None):
            """One tensor [N* x D_v x Q] per view of `views` (default: all V, in order): the mean of the Jacobian of the view's
            noise-free map at the deterministic latent points x [N* x Q], as bayesian_gp_lvm.predictive_jacobian."""
            vs = _views_arg(views)
            with torch.no_grad():
                train, xp = _train_marginals(), _marginals.points_arg(x, num_latent_dims, dev_)
                return [train[v].jacobian(xp)[0] for v in vs]

        @staticmethod
        def latent_metric(x, views=None, total=False):
            """One expected metric [N* x Q x Q] per view of `views` (default: all V, in order) at the latent points x [N* x Q],
            as bayesian_gp_lvm.latent_metric with the view's own kernel: which latent directions each view stretches.
            total=True: their sum, one tensor, the metric of the map to the chosen views' stacked columns."""
            vs = _views_arg(views)
            with torch.no_grad():
                train, xp = _train_marginals(), _marginals.points_arg(x, num_latent_dims, dev_)
                out = [train[v].metric(xp)[0] for v in vs]
            return torch.sum(torch.stack(out), dim=0) if total else out

        @staticmethod
        def predictive_covariance(x, views=None, columns=None, noise=False):
            """One array [len(columns[i]) x N* x N*] per view of `views` (default: all V, in order): the joint posterior covariance
            of the view's noise-free functions at the deterministic latent points x [N* x Q], as
            bayesian_gp_lvm.predictive_covariance with the view's own kernel.  columns: one list of the view's columns per entry
            of `views` (default: all D_v).  noise=True adds 1/beta_v on the diagonal.  Each array is J N*^2 doubles, and columns
            of one training row pattern repeat the same matrix."""
            vs = _views_arg(views)
            assert columns is None or len(columns) == len(vs), 'columns must hold one list per view of `views`'
            with torch.no_grad():
                train, xp = _train_marginals(), _marginals.points_arg(x, num_latent_dims, dev_)
                return [_marginals.covariance_of(
                    train[v], xp, _marginals.columns_arg(None if columns is None else columns[i], num_dimensions[v], dev_), noise)
                    for i, v in enumerate(vs)]

        @staticmethod
        def sample_functions(x, num_samples=1, views=None, columns=None, noise=False, jitter=_marginals.DEFAULT_SAMPLE_JITTER,
                             seed=0, draws=None):
            """One array [S x N* x len(columns[i])] per view of `views` (default: all V, in order): joint draws of the view's output
            dims at the latent points x, as bayesian_gp_lvm.sample_functions (the default jitter and its reasons there).  Every
            view draws from a generator seeded with `seed`; draws: one array [S x N* x len(columns[i])] per view.  The views are
            independent given x."""
            vs = _views_arg(views)
            assert columns is None or len(columns) == len(vs), 'columns must hold one list per view of `views`'
            assert draws is None or len(draws) == len(vs), 'draws must hold one array per view of `views`'
            with torch.no_grad():
                train, xp, infos = _train_marginals(), _marginals.points_arg(x, num_latent_dims, dev_), []
                out = [_marginals.samples_of(
                    train[v], xp, _marginals.columns_arg(None if columns is None else columns[i], num_dimensions[v], dev_),
                    num_samples, noise, jitter, seed, None if draws is None else draws[i], infos) for i, v in enumerate(vs)]
                _marginals.raise_if_not_factorised(torch.cat(infos))
            return out

        @staticmethod
        def predict_missing_data(views_test, use_pca=False, x_test_mean=None, x_test_var=None, reference_compat=False,
                                 observed=None, marginal_variance=False):
            """views_test: the FIRST Vo < V views of the test points (gaussian_process.py:834-990).  Returns
                (missing_data_lower_bound, x_test_mean, x_test_covar, predicted_means, predicted_covars)
            with one entry per unobserved view v = Vo .. V-1: mean [N* x D_v], covariance [D_v x N* x N*].
            reference_compat=True reproduces the reference's predicted means, which use the LAST training view's
            C = L_A^-1 L_uu^-1 Psi1^T for every unobserved view (a variable leaked from the training loop, :938); the default
            uses view v's own C.  The bound and the covariances are the same either way.

            observed (extension): a list of V entries, each None (the view is complete) or a boolean [N* x D_v] mask of the
            measured entries of views_test[v] (an all-False mask: the view is absent); views_test then holds all V arrays,
            whose unobserved entries are ignored and may be NaN.  The bound is sum_v f_hat_v + sum_slots f_hat*_b - KL(q(X)) -
            KL(q(X*)), the slots of view v being the column groups of its mask that share one row pattern, with kernel v.  The
            moments are returned for every view with at least one unobserved entry, in view order (property missing_views),
            over that view's columns with at least one unobserved entry (property missing_columns, aligned), always with the
            view's own C.  q(X*) starts at the masked nearest neighbour over the stacked views (a row with nothing observed
            starts at 0).  AssertionError for lists of the wrong length, non-boolean masks, shape mismatches, masks that are
            True everywhere, no True entry anywhere, or reference_compat=True.

            marginal_variance=True (extension): predicted_covars holds, per returned view, the per-entry variance [N* x Du] of
            predictive_marginals on the predicted columns in place of the [Du x N* x N*] array.

            On a model trained with observed= this method is not built: NotImplementedError (predictive_marginals gives the
            moments at test points, impute_training_data fills the training data's own gaps)."""
            if masked is not None:
                raise NotImplementedError('predict_missing_data is not built for a model trained with observed=: use '
                                          'impute_training_data for the gaps of the training data')
            if observed is not None:
                y0s, obs = _masked(views_test, observed, predict=True, reference_compat=reference_compat)
                xt, st_ = _masked_init(y0s, obs, use_pca, x_test_mean, x_test_var)
                bound = _masked_bound(y0s, obs)
                mv_, mc = pred_state['missing_views'], pred_state['missing_columns']
                f_test, kl_t = _latents.bound_at(bound, xt, st_)
                with torch.no_grad():
                    f_hat, kl = _train_terms()
                    bound_u = _TestBound.kernels(*_frozen([inner[v] for v in mv_]),
                                                 [torch.zeros((1, 1), dtype=TORCH_DTYPE, device=dev_)] * len(mv_), dev_)
                    means, covars = _predictive_moments(bound_u, list(range(len(mv_))), x_mean_t.detach(),
                                                        F.softplus(x_var_raw).detach(),
                                                        [_as_device(views_np[v][:, c], dev_) for v, c in zip(mv_, mc)], xt, st_)
                if marginal_variance:
                    covars = _marginals_at(xt, st_, mv_, mc)[1]
                return f_hat + f_test - kl - kl_t, xt, torch.diag_embed(st_), means, covars
            views_test = _check_views(views_test, True)
            vo = len(views_test)
            pred_state['missing_views'] = list(range(vo, num_views))
            pred_state['missing_columns'] = [np.arange(num_dimensions[v]) for v in range(vo, num_views)]
            xt, st_ = _init(views_test, use_pca, x_test_mean, x_test_var)
            lb = _bound_at(views_test, xt, st_)
            ku = inner[vo:]
            with torch.no_grad():
                bound_u = _TestBound.kernels(*_frozen(ku), [torch.zeros((1, 1), dtype=TORCH_DTYPE, device=dev_)] * len(ku), dev_)
                c_index = [len(ku) - 1] * len(ku) if reference_compat else list(range(len(ku)))
                means, covars = _predictive_moments(bound_u, c_index, x_mean_t.detach(), F.softplus(x_var_raw).detach(),
                                                    [_as_device(v, dev_) for v in views_np[vo:]], xt, st_)
            if marginal_variance:
                covars = _marginals_at(xt, st_, pred_state['missing_views'])[1]
            return lb, xt, torch.diag_embed(st_), means, covars

        @staticmethod
        def test_latent_gradients(views_test, x_test_mean, x_test_var, observed=None):
            """d(sum_v f_hat*_v - KL(q(X*))) / d(x_test_mean, x_test_var) over the given first Vo <= V views (one batched
            qx_psi_stats_batched / qx_psi_adjoint over the Vo kernels).  observed: as predict_missing_data (all V views; True
            everywhere is allowed here)."""
            return _test_latent_gradients(views_test, x_test_mean, x_test_var, observed)

        @staticmethod
        def optimise_test_latents(views_test, num_iterations=200, learning_rate=0.01, use_pca=False, x_test_mean=None,
                                  x_test_var=None, observed=None):
            """Adam on q(X*) maximising sum_v f_hat*_v - KL(q(X*)) over the given first Vo views; returns (x_test_mean,
            x_test_var).  No host synchronisation inside the loop.  observed: as predict_missing_data."""
            return _optimise_test_latents(views_test, num_iterations, learning_rate, use_pca, x_test_mean, x_test_var, observed)

        @property
        def missing_views(self):
            """The views whose moments the last predict_missing_data returned (ascending), or None."""
            return pred_state.get('missing_views')

        @property
        def missing_columns(self):
            """Aligned with missing_views: the columns of each such view whose moments were returned (ascending), or None."""
            return pred_state.get('missing_columns')

        @staticmethod
        def impute_training_data(return_variance=False):
            """A model trained with observed=: a list of V fp64 device tensors [N x D_v], view v with every unobserved entry
            (n, d) replaced by the posterior mean beta_v Psi1_v[n,:] (K_uu_v + beta_v Psi2_d)^-1 Psi1_v^T y_d (Psi2_d and y_d
            over the rows at which d was observed); observed entries as given, a never-observed column 0.
            return_variance=True: (filled, variances), variances a list of V tensors [N x D_v]: the per-entry predictive
            variance of predictive_marginals at the training q(X) at the unobserved entries and 0 at the observed ones; filled
            is the same list either way."""
            assert masked is not None, 'impute_training_data needs a model trained with observed='
            filled = masked.impute()
            if not return_variance:
                return filled
            _, variances = _marginals_at(x_mean_t.detach(), F.softplus(x_var_raw).detach(), list(range(num_views)))
            return filled, [_marginals.unobserved_variance(v, o) for v, o in zip(variances, train_obs)]

        @property
        def objective_terms(self):
            """A model trained with observed=: the [slots x 5] terms of sum_slots f_b in the last evaluation, ordered by view
            and then by first column; None for a model trained on complete views."""
            return None if masked is None else masked.bound.terms

        @property
        def prediction_terms(self):
            """[Vo x 5] terms of f_hat*_v of the last prediction evaluation (as bayesian_gp_lvm.prediction_terms, per view);
            [slots x 5] after an evaluation with observed=."""
            b = pred_state.get('bound')
            return None if b is None else b.terms

        @property
        def number_of_views(self):
            return num_views

        @property
        def kernels(self):
            return [mv.kernel for mv in inner]

        @property
        def ard_weights(self):
            return [F.softplus(mv.raw['gamma_atoms']) for mv in inner]

        @property
        def signal_variance(self):
            return [F.softplus(mv.raw['alpha_atoms']) for mv in inner]

        @property
        def noise_precision(self):
            return [F.softplus(mv.raw['beta_atoms']) for mv in inner]

        @property
        def inducing_input(self):
            return [mv.raw['x_u'] for mv in inner]

        @property
        def q_x(self):
            return x_mean_t, torch.diag_embed(F.softplus(x_var_raw))

        @property
        def objective(self):
            return _objective()

        gradients = staticmethod(_gradients)
        optimise = staticmethod(_optimise)

    return ManifoldRelevanceDetermination()
