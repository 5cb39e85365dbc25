"""
CPU tests (no GPU): the gp_regression / gp_lvm fixtures (tests/golden/gpr_ref_*.npz, gplvm_ref_*.npz, written by
tools/gen_golden_gp.py from the reference's own models, src/models/gaussian_process.py:22-129) against a short torch fp64
restatement.  This pins what the HIP models must reproduce:
  * log_likelihood_d = log N(y_d | 0, K_xx) + P for every d, so objective = -sum_d log N(y_d | 0, K_xx) - D * P;
  * K_xx = alpha exp(-1/2 sum_q gamma_q d^2) + (1/beta + 1e-8) I; K_ss has the jitter only, K_xs neither;
  * the predictive mean is K_xs^T diag(L)^-1 L^-1 Y (the reference's second triangular solve reads only the diagonal of L^T).
"""
import glob
import math
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FILES = sorted(glob.glob(os.path.join(GOLDEN, 'gpr_ref_*.npz')) + glob.glob(os.path.join(GOLDEN, 'gplvm_ref_*.npz')))
JITTER = 1e-8


def softplus(t):
    return torch.log1p(torch.exp(t))


def gram(x0, x1, gamma, alpha):
    d = x0[:, None, :] - x1[None, :, :]
    return alpha * torch.exp(-0.5 * torch.sum(gamma * d * d, dim=-1))


def log_normal(v):
    return -torch.log(v) - 0.5 * (math.log(2.0 * math.pi) + torch.log(v) ** 2)


def restated(f, raw):
    """(objective, log_likelihood [D], prediction mean, prediction covariance) from the raw variables (torch leaves)."""
    y = torch.as_tensor(f['y'])
    x = raw['x_latent'] if 'x_latent' in raw else torch.as_tensor(f['x'])
    gamma, alpha, beta = softplus(raw['gamma_raw']), softplus(raw['alpha_raw'])[0, 0], softplus(raw['beta_raw'])[0, 0]
    n, d = y.shape
    k = gram(x, x, gamma, alpha) + (1.0 / beta + JITTER) * torch.eye(n, dtype=torch.float64)
    l_ = torch.linalg.cholesky(k)
    z = torch.linalg.solve_triangular(l_, y, upper=False)
    ll = -0.5 * torch.sum(z * z, dim=0) - torch.sum(torch.log(torch.diagonal(l_))) - 0.5 * n * math.log(2.0 * math.pi)
    prior = torch.sum(log_normal(gamma)) + log_normal(alpha) + log_normal(beta)
    ll = ll + prior
    xs = torch.as_tensor(f['x_test'])
    ns = xs.shape[0]
    k_ss = gram(xs, xs, gamma, alpha) + JITTER * torch.eye(ns, dtype=torch.float64)
    k_xs = gram(x, xs, gamma, alpha)
    mean = k_xs.T @ (z / torch.diagonal(l_)[:, None])
    v = torch.linalg.solve_triangular(l_, k_xs, upper=False)
    return -torch.sum(ll), ll, mean, k_ss - v.T @ v


@pytest.mark.parametrize('path', FILES, ids=[os.path.basename(p)[:-4] for p in FILES])
def test_restatement_reproduces_the_reference_fixture(path):
    f = np.load(path)
    names = [k for k in ('x_latent', 'gamma_raw', 'alpha_raw', 'beta_raw') if k in f.files]
    raw = {k: torch.tensor(f[k], dtype=torch.float64, requires_grad=True) for k in names}
    obj, ll, mean, covar = restated(f, raw)
    np.testing.assert_allclose(float(obj.detach()), float(f['objective']), rtol=1e-12)
    np.testing.assert_allclose(ll.detach().numpy(), f['log_likelihood'], rtol=1e-12)
    grads = torch.autograd.grad(obj, [raw[k] for k in names])
    for k, g in zip(names, grads):
        ref = f['grad_' + k]
        np.testing.assert_allclose(g.numpy(), ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max(), err_msg=k)
    np.testing.assert_allclose(mean.detach().numpy(), f['pred_mean'], rtol=1e-10, atol=1e-10 * np.abs(f['pred_mean']).max())
    np.testing.assert_allclose(covar.detach().numpy(), f['pred_covar'], rtol=1e-10, atol=1e-10 * np.abs(f['pred_covar']).max())


def test_fixtures_cover_the_three_cholesky_paths():
    ns = sorted({int(np.load(p)['y'].shape[0]) for p in FILES})
    assert any(n <= 128 for n in ns)
    assert any(n > 128 and n % 128 for n in ns)
    assert any(n % 128 == 0 and n > 128 for n in ns)
    assert {str(np.load(p)['kind']) for p in FILES} == {'gpr', 'gplvm'}


def test_models_are_importable():
    from dp_gp_lvm_amd.models.gaussian_process import gp_lvm, gp_regression   # noqa: F401
    from dp_gp_lvm_amd.distributions.normal import mvn_conditional_mean_covar   # noqa: F401
    from dp_gp_lvm_amd import ops
    assert callable(ops.ard_rbf_gram_grad)


def test_gram_grad_workspace_query_is_host_only():
    from dp_gp_lvm_amd import _lib
    l = _lib.lib()
    for n, q in ((1, 1), (65, 3), (2048, 10), (4096, 8), (777, 64)):
        b = l.dpgp_ard_rbf_gram_grad_workspace_bytes(n, q)
        assert b >= 8 * (2 * q + 1) * n and b % 8 == 0, (n, q, b)
    assert l.dpgp_ard_rbf_gram_grad_workspace_bytes(0, 3) == 0
    assert l.dpgp_ard_rbf_gram_grad_workspace_bytes(10, 0) == 0
    assert l.dpgp_ard_rbf_gram_grad_workspace_bytes(10, 65) == 0
