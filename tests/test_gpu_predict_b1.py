"""GPU tests of test-point prediction for bayesian_gp_lvm and manifold_relevance_determination (reference
src/models/gaussian_process.py:329-538, :729-990) and of its two operators, dpgp_qx_psi_stats_batched_f64 and
dpgp_qx_psi_adjoint_f64 (csrc/qx_psi.hip).  Fixtures: tools/gen_golden_predict_b1.py -> tests/golden/predb1_*.npz."""
import itertools

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu
BGPLVM = ['predb1_bgplvm_40_6_12_3', 'predb1_bgplvm_70_9_20_4', 'predb1_bgplvm_150_12_136_8']
MRD = ['predb1_mrd_50_2views_12_3', 'predb1_mrd_60_4views_15_4']


def softplus(x):
    return np.logaddexp(0.0, x)


def close(have, want, rtol, err_msg=''):
    have = have.detach().cpu().numpy() if torch.is_tensor(have) else np.asarray(have)
    want = np.asarray(want)
    np.testing.assert_allclose(have.reshape(want.shape), want, rtol=rtol, atol=rtol * max(1.0, np.abs(want).max()),
                               err_msg=err_msg)


def build_bgplvm(g, dev, prec='f64', y=None, x_u=None, hyper=''):
    from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm
    y = g['y'] if y is None else y
    x_u = g['x_u'] if x_u is None else x_u
    return bayesian_gp_lvm(y, num_latent_dims=g['x_mean'].shape[1], num_inducing_points=x_u.shape[0], device=dev, precision=prec,
                           initial_values=dict(x_mean=g['x_mean'], x_var=softplus(g['x_var_raw']), x_u=x_u,
                                               gamma=softplus(g['gamma_raw' + hyper]), alpha=softplus(g['alpha_raw' + hyper]),
                                               beta=softplus(g['beta_raw' + hyper])))


def build_mrd(g, dev, prec='f64'):
    from dp_gp_lvm_amd.models.gaussian_process import manifold_relevance_determination
    nv = int(g['num_views'])
    views = [g['view_%d' % i] for i in range(nv)]
    iv = dict(x_mean=g['x_mean'], x_var=softplus(g['x_var_raw']), x_u=[g['x_u_%d' % i] for i in range(nv)],
              gamma=[softplus(g['gamma_raw_%d' % i]) for i in range(nv)], alpha=[softplus(g['alpha_raw_%d' % i]) for i in range(nv)],
              beta=[softplus(g['beta_raw_%d' % i]) for i in range(nv)])
    return manifold_relevance_determination(views, num_latent_dims=g['x_mean'].shape[1], num_inducing_points=g['x_u_0'].shape[0],
                                            device=dev, precision=prec, initial_values=iv)


# ---------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize('fixture', BGPLVM)
@pytest.mark.parametrize('compat', [False, True])
def test_bgplvm_prediction_matches_the_reference(dev, fixture, compat):
    g = golden(fixture)
    model = build_bgplvm(g, dev)
    xm, xv, y_test, do = g['x_test_mean'], g['x_test_var'], g['y_test'], int(g['n_observed'])
    lb, mean, covar, ll = model.predict_new_latent_variables(y_test, x_test_mean=xm, x_test_var=xv, reference_compat=compat)
    close(lb, g['new_lower_bound'], 1e-10, 'new bound')
    close(ll, g['new_test_log_likelihood'], 1e-10, 'test log-likelihood')
    close(mean, xm, 1e-15)
    close(torch.diagonal(covar, dim1=-2, dim2=-1), xv, 1e-15)
    assert tuple(model.prediction_terms.shape) == (1, 5)
    mlb, _, _, pmean, pcovar = model.predict_missing_data(y_test[:, :do], x_test_mean=xm, x_test_var=xv, reference_compat=compat)
    close(mlb, g['missing_lower_bound'], 1e-10, 'missing-data bound')
    close(pmean, g['predicted_mean'], 1e-10, 'predicted mean')
    close(pcovar, g['predicted_covar'], 1e-10, 'predicted covariance')
    for tag, yt in (('new', y_test), ('missing', y_test[:, :do])):
        g_mu, g_s = model.test_latent_gradients(yt, xm, xv)
        close(g_mu, g[tag + '_grad_mean'], 1e-8, tag + ' d/dmean')
        close(g_s, g[tag + '_grad_var'], 1e-8, tag + ' d/dvar')


@pytest.mark.parametrize('fixture', MRD)
@pytest.mark.parametrize('compat', [False, True])
def test_mrd_prediction_matches_the_reference(dev, fixture, compat):
    g = golden(fixture)
    model = build_mrd(g, dev)
    nv, vo = int(g['num_views']), int(g['n_observed'])
    views_test = [g['test_view_%d' % i] for i in range(nv)]
    xm, xv = g['x_test_mean'], g['x_test_var']
    out = model.predict_new_latent_variables(views_test, x_test_mean=xm, x_test_var=xv, reference_compat=compat)
    assert len(out) == 3
    close(out[0], g['new_lower_bound'], 1e-10, 'new bound')
    assert tuple(model.prediction_terms.shape) == (nv, 5)
    mlb, _, _, means, covars = model.predict_missing_data(views_test[:vo], x_test_mean=xm, x_test_var=xv,
                                                          reference_compat=compat)
    close(mlb, g['missing_lower_bound'], 1e-10, 'missing-data bound')
    assert len(means) == len(covars) == nv - vo
    for i in range(nv - vo):
        close(means[i], g[('predicted_mean_compat_%d' if compat else 'predicted_mean_%d') % i], 1e-10, 'mean %d' % i)
        close(covars[i], g['predicted_covar_%d' % i], 1e-10, 'covariance %d' % i)
    for tag, vt in (('new', views_test), ('missing', views_test[:vo])):
        g_mu, g_s = model.test_latent_gradients(vt, xm, xv)
        close(g_mu, g[tag + '_grad_mean'], 1e-8, tag + ' d/dmean')
        close(g_s, g[tag + '_grad_var'], 1e-8, tag + ' d/dvar')


def test_mrd_defect_fixture_differs():
    # the 4-view fixture has two unobserved views: the reference's leaked C changes the first one's mean
    g = golden(MRD[1])
    assert np.abs(g['predicted_mean_0'] - g['predicted_mean_compat_0']).max() > 1e-3
    np.testing.assert_allclose(g['predicted_mean_1'], g['predicted_mean_compat_1'], rtol=1e-12, atol=1e-12)


# --------------------------------------------------------------------------------------------------------------- operators
def restated(z, mu, s, gamma, alpha, g1, g2):
    """sum_b <g1_b, Psi1_b> + <g2_b, Psi2_b> and its gradient with respect to (mu, s), by torch autograd of a plain
    restatement of rbf_kernel.py:135-199 (Psi2 in chunks of test points; its terms are separable over them)."""
    mu = mu.detach().clone().requires_grad_()
    s = s.detach().clone().requires_grad_()
    ga, al = gamma[:, None, None, :], alpha[:, None, None]
    den1 = ga * s[None, :, None, :] + 1.0                                                  # [B,N,1,Q]
    num1 = ga * (mu[None, :, None, :] - z[:, None, :, :]) ** 2                             # [B,N,M,Q]
    psi1 = torch.exp(torch.log(al) - 0.5 * torch.sum(num1 / den1 + torch.log(den1), dim=-1))
    f = torch.sum(g1 * psi1)
    b_, m_, q_ = z.shape
    step = max(1, int(2e7 // max(1, b_ * m_ * m_ * q_)))
    psi2 = torch.zeros_like(g2)
    zbar = 0.5 * (z[:, :, None, :] + z[:, None, :, :])                                    # [B,M,M,Q]
    t1 = 0.25 * gamma[:, None, None, :] * (z[:, :, None, :] - z[:, None, :, :]) ** 2
    for n0 in range(0, mu.shape[0], step):
        mc, sc = mu[n0:n0 + step], s[n0:n0 + step]
        gq = gamma[:, None, None, None, :]
        den2 = 2.0 * gq * sc[None, :, None, None, :] + 1.0                                  # [B,n,1,1,Q]
        num2 = gq * (mc[None, :, None, None, :] - zbar[:, None]) ** 2                       # [B,n,M,M,Q]
        lg = 2.0 * torch.log(alpha)[:, None, None, None] - torch.sum(0.5 * torch.log(den2) + t1[:, None] + num2 / den2, dim=-1)
        p2 = torch.exp(lg).sum(dim=1)
        psi2 = psi2 + p2.detach()
        f = f + torch.sum(g2 * p2)
    d_mu, d_s = torch.autograd.grad(f, [mu, s])
    return psi1.detach(), psi2, d_mu, d_s


def random_case(dev, b, n, m, q, seed):
    rs = np.random.default_rng(seed)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)
    z = t(rs.standard_normal((b, m, q)))
    mu = t(rs.standard_normal((n, q)))
    s = t(rs.uniform(0.1, 1.5, (n, q)))
    gamma = t(rs.uniform(0.2, 2.0, (b, q)))
    alpha = t(rs.uniform(0.5, 2.0, b))
    g1 = t(rs.standard_normal((b, n, m)))
    g2 = t(rs.standard_normal((b, m, m)))
    return z, mu, s, gamma, alpha, g1, g2


@pytest.mark.parametrize('b,m,q,n', list(itertools.product([1, 5], [1, 17, 64, 128, 200], [1, 10, 23], [1, 300])))
def test_operators_match_autograd_of_the_restatement(dev, b, m, q, n):
    from dp_gp_lvm_amd import ops
    z, mu, s, gamma, alpha, g1, g2 = random_case(dev, b, n, m, q, 1000 * b + 10 * m + q + n)
    psi1_r, psi2_r, dmu_r, ds_r = restated(z, mu, s, gamma, alpha, g1, g2)
    zfac = ops.qx_pair_factor(z, gamma, alpha)
    for zf in (None, zfac):
        psi1, psi2 = ops.qx_psi_stats_batched(z, mu, s, gamma, alpha, zfac=zf)
        close(psi1, psi1_r.cpu().numpy(), 1e-12, 'psi1')
        close(psi2, psi2_r.cpu().numpy(), 1e-12, 'psi2')
        assert torch.equal(psi2, psi2.transpose(1, 2))
        d_mu, d_s = ops.qx_psi_adjoint(z, mu, s, gamma, alpha, g1, g2, zfac=zf)
        close(d_mu, dmu_r.cpu().numpy(), 1e-12, 'd_mu')
        close(d_s, ds_r.cpu().numpy(), 1e-12, 'd_s')


def test_adjoint_is_bitwise_reproducible(dev):
    from dp_gp_lvm_amd import ops
    z, mu, s, gamma, alpha, g1, g2 = random_case(dev, 5, 300, 200, 23, 7)
    a = ops.qx_psi_adjoint(z, mu, s, gamma, alpha, g1, g2)
    b = ops.qx_psi_adjoint(z, mu, s, gamma, alpha, g1, g2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    p = ops.qx_psi_stats_batched(z, mu, s, gamma, alpha)
    r = ops.qx_psi_stats_batched(z, mu, s, gamma, alpha)
    assert torch.equal(p[0], r[0]) and torch.equal(p[1], r[1])


# ------------------------------------------------------------------------------------------------------------------ models
def test_optimise_test_latents_raises_the_bound(dev):
    g = golden(BGPLVM[1])
    model = build_bgplvm(g, dev)
    model.optimise(20, learning_rate=0.01)
    y_test = g['y_test']
    xm0, xv0 = g['x_test_mean'], g['x_test_var']
    before = float(model.predict_new_latent_variables(y_test, x_test_mean=xm0, x_test_var=xv0)[0])
    xm, xv = model.optimise_test_latents(y_test, 50, learning_rate=0.05, x_test_mean=xm0, x_test_var=xv0)
    after = float(model.predict_new_latent_variables(y_test, x_test_mean=xm, x_test_var=xv)[0])
    assert np.isfinite(after) and after > before + 1.0, (before, after)


def test_mrd_with_one_observed_view_agrees_with_bgplvm(dev):
    g = golden(MRD[0])
    mrd = build_mrd(g, dev)
    gb = dict(g)
    for k in ('gamma_raw', 'alpha_raw', 'beta_raw'):
        gb[k] = g[k + '_0']
    bg = build_bgplvm(gb, dev, y=g['view_0'], x_u=g['x_u_0'])
    vt, xm, xv = g['test_view_0'], g['x_test_mean'], g['x_test_var']
    a_mu, a_s = mrd.test_latent_gradients([vt], xm, xv)
    ta = mrd.prediction_terms.clone()
    b_mu, b_s = bg.test_latent_gradients(vt, xm, xv)
    tb = bg.prediction_terms.clone()
    close(ta, tb.cpu().numpy(), 1e-13, 'terms')
    close(a_mu, b_mu.cpu().numpy(), 1e-13, 'd/dmean')
    close(a_s, b_s.cpu().numpy(), 1e-13, 'd/dvar')


def test_argument_checks(dev):
    g = golden(BGPLVM[0])
    model = build_bgplvm(g, dev)
    y_test = g['y_test']
    with pytest.raises(AssertionError):
        model.predict_missing_data(y_test)                                  # Do >= D
    with pytest.raises(AssertionError):
        model.predict_new_latent_variables(y_test[:, :-1])
    m = golden(MRD[1])
    mrd = build_mrd(m, dev)
    views_test = [m['test_view_%d' % i] for i in range(int(m['num_views']))]
    with pytest.raises(AssertionError):
        mrd.predict_new_latent_variables(views_test[:-1])                    # view count
    with pytest.raises(AssertionError):
        mrd.predict_missing_data(views_test)                                 # Vo = V
    with pytest.raises(AssertionError):
        mrd.predict_missing_data([views_test[0], views_test[1][:-1]])        # N* differs
    with pytest.raises(AssertionError):
        mrd.predict_missing_data([views_test[0][:, :-1]])                    # D_v differs


def test_reference_workflow_end_to_end(dev):
    """Train, predict_missing_data, optimise q(X*) for 1000 iterations, score the held-out dims with mvn_log_pdf
    (test/horse_mocap_missing_data_test.py's steps), for both models."""
    from dp_gp_lvm_amd.distributions.normal import mvn_log_pdf
    g = golden(BGPLVM[1])
    model = build_bgplvm(g, dev, prec='mixed')
    model.optimise(10, learning_rate=0.01)
    y_test, do = g['y_test'], int(g['n_observed'])
    np.random.seed(0)
    _, xm, xc, _, _ = model.predict_missing_data(y_test[:, :do])
    xm, xv = model.optimise_test_latents(y_test[:, :do], 1000, learning_rate=0.01, x_test_mean=xm,
                                         x_test_var=torch.diagonal(xc, dim1=-2, dim2=-1))
    lb, _, _, pmean, pcovar = model.predict_missing_data(y_test[:, :do], x_test_mean=xm, x_test_var=xv)
    score = sum(float(mvn_log_pdf(torch.as_tensor(y_test[None, :, do + j], device=dev), pmean[None, :, j], pcovar[j])[0])
                for j in range(y_test.shape[1] - do))
    assert np.isfinite(float(lb)) and np.isfinite(score)
    m = golden(MRD[1])
    mrd = build_mrd(m, dev, prec='mixed')
    mrd.optimise(10, learning_rate=0.01)
    vo = int(m['n_observed'])
    views_test = [m['test_view_%d' % i] for i in range(int(m['num_views']))]
    _, xm, xc, _, _ = mrd.predict_missing_data(views_test[:vo])
    xm, xv = mrd.optimise_test_latents(views_test[:vo], 1000, learning_rate=0.01, x_test_mean=xm,
                                       x_test_var=torch.diagonal(xc, dim1=-2, dim2=-1))
    lb, _, _, means, covars = mrd.predict_missing_data(views_test[:vo], x_test_mean=xm, x_test_var=xv)
    for i, (pm, pc) in enumerate(zip(means, covars)):
        yv = views_test[vo + i]
        score = sum(float(mvn_log_pdf(torch.as_tensor(yv[None, :, j], device=dev), pm[None, :, j], pc[j])[0])
                    for j in range(yv.shape[1]))
        assert np.isfinite(score)
    assert np.isfinite(float(lb))
