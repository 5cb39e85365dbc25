"""
The test-time fit of q(X*) = N(mean, diag(variances)) that bayesian_gp_lvm, manifold_relevance_determination, dp_gp_lvm and
dp_gp_lvm_t share: the coercion of supplied values, the start, the gradient of the bound a model holds frozen, the Adam loop on
(mean, softplus-raw variances) and the evaluation of that bound at a point, each written once.  Plain functions: a model builds
its bound (any object with evaluate(mu, s, grad=) -> (f_hat*, d f_hat* / d mu, d f_hat* / d s): frozen_bound._TestBound,
frozen_bound_t._TestBoundT, frozen_bound_d._TestBoundD / _ShardedTestBoundD), checks its own arguments, keeps its own sum of the
bound's parts and decides whether the fit updates the start in place (the DP models) or a copy (the B = 1 models).
"""
import numpy as np
import torch
import torch.nn.functional as F

from .. import ops
from ..utils import missing as _missing
from ..utils.expressions import principal_component_analysis as pca
from .frozen_bound import _as_device


def latent_values(v, device, num_latent_dims, num_points=-1):
    """v (numpy or torch, any shape of num_points x Q values) as a contiguous fp64 tensor [N* x Q] on the device."""
    return _as_device(v, device, (num_points, num_latent_dims))


def l2_neighbour(y_ref, y_test, x_train_mean):
    """The training latent mean (numpy [N x Q]) of every test row's nearest training row, L2 over the given columns (the SUM of
    squares, utils/expressions.py:28-44; the masked forms below compare means), plus one N(0, 0.01^2) draw [N* x Q] from NumPy's
    global generator."""
    d2 = ((y_ref[:, None, :] - y_test[None, :, :]) ** 2).sum(-1)                    # [N x N*]
    return x_train_mean[np.argmin(d2, axis=0)] + np.random.normal(scale=0.01, size=(y_test.shape[0], x_train_mean.shape[1]))


def masked_neighbour(y_train, train_observed, y_test, observed, x_train_mean):
    """The start under a per-entry test mask, noise drawn (utils/missing.py): over each test row's observed columns on a model
    trained on complete data (train_observed None), over the jointly observed columns on a mask-trained one."""
    if train_observed is None:
        return _missing.masked_nearest_neighbour_init(y_train, y_test, observed, x_train_mean)
    return _missing.jointly_observed_nearest_neighbour_init(y_train, train_observed, y_test, observed, x_train_mean)


def start(num_points, num_latent_dims, device, x_test_mean, x_test_var, use_pca, y_pca, neighbour):
    """(mean, variances) [N* x Q] of q(X*) before any fit (gaussian_process.py:346-360, dp_gp_lvm.py:246-262): the mean is the given
    x_test_mean, else (use_pca) the PCA of y_pca, else neighbour(), a numpy [N* x Q] with its noise already drawn; the variances
    are the given x_test_var, else 1.  Only neighbour() draws random numbers."""
    if x_test_mean is not None:
        init = x_test_mean
    elif use_pca:
        init = pca(y_pca, num_latent_dimensions=num_latent_dims)
    else:
        init = neighbour()
    var = x_test_var if x_test_var is not None else np.ones((num_points, num_latent_dims))
    return latent_values(init, device, num_latent_dims, num_points), latent_values(var, device, num_latent_dims, num_points)


def kl_gradient(mu, s):
    """d KL(q(X*) || N(0, I)) / d (mu, s) (gp_expressions.py:10-24)."""
    return mu, 0.5 * (1.0 - 1.0 / s)


def ascent_gradient(bound, mu, s):
    """d (f_hat* - KL(q(X*))) / d (mu, s) of a frozen bound."""
    _, d_mu, d_s = bound.evaluate(mu, s, grad=True)
    k_mu, k_s = kl_gradient(mu, s)
    return d_mu - k_mu, d_s - k_s


def fit(grad_fn, xt, st, num_iterations, learning_rate):
    """Adam on q(X*) (mean xt, softplus-parametrised variances from st) ascending the bound whose gradient grad_fn(mu, s) returns;
    torch.optim.Adam only applies the update.  xt is updated IN PLACE and returned with the fitted variances: a caller that keeps
    its start passes a clone.  No host read, no collective and no autograd state of its own."""
    raw = torch.log(torch.expm1(st))
    opt = torch.optim.Adam([xt, raw], lr=learning_rate)
    for _ in range(num_iterations):
        g_mu, g_s = grad_fn(xt, F.softplus(raw))
        xt.grad, raw.grad = -g_mu, -g_s * torch.sigmoid(raw)
        opt.step()
    return xt, F.softplus(raw)


def bound_at(bound, mu, s):
    """(f_hat*, KL(q(X*))) of a frozen bound at q(X*) = (mu, s); the caller adds the training side in its own order."""
    with torch.no_grad():
        f_test, _, _ = bound.evaluate(mu, s)
        return f_test, ops.kl_qx(mu, s)
