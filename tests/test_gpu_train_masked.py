"""GPU tests of training bayesian_gp_lvm on data with missing entries (observed=...): the parameter adjoint of the weighted
Psi statistics (dpgp_qx_psi_param_adjoint_weighted_f64, csrc/qx_psi.hip) against fp64 torch autograd of a plain restatement,
the masked model's objective and six raw gradients against the reference's fixtures (all-True mask) and the committed fp64
oracle evaluated per output dim on the rows at which that dim was observed (general masks), training + imputation on
synthetic data, and prediction on a mask-trained model.  Tolerances: 1e-12 for the operator (the project's operator
tolerance), rtol 1e-10 for objectives and 1e-7 of each variable's largest entry for gradients (the fp64 tolerances of the
README)."""
import itertools

import numpy as np
import pytest
import torch

from conftest import golden
from test_gpu_predict_b1 import close, random_case
from test_gpu_predict_masked import masks_of, weights_of

pytestmark = pytest.mark.gpu
FIXTURES = ['bgplvm_ref_40_6_12_3', 'bgplvm_ref_70_9_20_4']
REF2RAW = dict(gamma_raw='gamma_atoms', alpha_raw='alpha_atoms', beta_raw='beta_atoms', x_mean='x_mean', x_u='x_u',
               x_var_raw='x_var')


def softplus(x):
    return np.logaddexp(0.0, x)


# ---------------------------------------------------------------------------------------------------------------- operator
def restated_param(z, mu, s, gamma, alpha, g1, g2, w):
    """d/d(z, gamma, alpha) of sum_b <g1_b, Psi1_b> + <g2_b, sum_n w[b,n] psi2_bn> by torch autograd of the plain restatement of
    rbf_kernel.py:135-199 used by test_gpu_predict_masked.restated (weights on the Psi2 sum; Psi2 in chunks of points)."""
    z, gamma, alpha = (a.detach().clone().requires_grad_() for a in (z, gamma, alpha))
    ga, al = gamma[:, None, None, :], alpha[:, None, None]
    den1 = ga * s[None, :, None, :] + 1.0                                                  # [B,N,1,Q]
    num1 = ga * (mu[None, :, None, :] - z[:, None, :, :]) ** 2                             # [B,N,M,Q]
    psi1 = torch.exp(torch.log(al) - 0.5 * torch.sum(num1 / den1 + torch.log(den1), dim=-1))
    f = torch.sum(g1 * psi1)
    b_, m_, q_ = z.shape
    step = max(1, int(2e7 // max(1, b_ * m_ * m_ * q_)))
    zbar = 0.5 * (z[:, :, None, :] + z[:, None, :, :])                                    # [B,M,M,Q]
    t1 = 0.25 * gamma[:, None, None, :] * (z[:, :, None, :] - z[:, None, :, :]) ** 2
    grads = None
    for n0 in range(0, mu.shape[0], step):
        mc, sc = mu[n0:n0 + step], s[n0:n0 + step]
        gq = gamma[:, None, None, None, :]
        den2 = 2.0 * gq * sc[None, :, None, None, :] + 1.0                                  # [B,n,1,1,Q]
        num2 = gq * (mc[None, :, None, None, :] - zbar[:, None]) ** 2                       # [B,n,M,M,Q]
        lg = 2.0 * torch.log(alpha)[:, None, None, None] - torch.sum(0.5 * torch.log(den2) + t1[:, None] + num2 / den2, dim=-1)
        p2 = (w[:, n0:n0 + step, None, None] * torch.exp(lg)).sum(dim=1)
        gr = torch.autograd.grad(torch.sum(g2 * p2), [z, gamma, alpha], retain_graph=True)   # (chunk by chunk: memory)
        grads = gr if grads is None else tuple(a + c for a, c in zip(grads, gr))
    gr = torch.autograd.grad(f, [z, gamma, alpha])
    return tuple(a + c for a, c in zip(grads, gr))


GRID = list(itertools.product([1, 5], [1, 17, 64, 128, 200], [1, 10, 23], [1, 300])) + [(2, 40, 64, 70)]


@pytest.mark.parametrize('kind', ['binary', 'kernel_off', 'normal', 'none'])
@pytest.mark.parametrize('b,m,q,n', GRID)
def test_param_adjoint_matches_autograd_of_the_restatement(dev, b, m, q, n, kind):
    from dp_gp_lvm_amd import ops
    seed = 1000 * b + 10 * m + q + n
    z, mu, s, gamma, alpha, g1, g2 = random_case(dev, b, n, m, q, seed)
    ones = torch.ones((b, n), dtype=torch.float64, device=dev)
    w = None if kind == 'none' else weights_of(kind, b, n, seed + 1, dev)
    want = restated_param(z, mu, s, gamma, alpha, g1, g2, ones if w is None else w)
    if q <= 30:
        zfac = ops.qx_pair_factor(z, gamma, alpha)
    else:                                                        # (beyond the gram operator's Q: the same factor in torch)
        dz = z[:, :, None, :] - z[:, None, :, :]
        zfac = (alpha * alpha)[:, None, None] * torch.exp(-0.25 * torch.sum(gamma[:, None, None, :] * dz * dz, dim=-1))
    for zf in (None, zfac):
        have = ops.qx_psi_param_adjoint(z, mu, s, gamma, alpha, g1, g2, zfac=zf, weights=w)
        again = ops.qx_psi_param_adjoint(z, mu, s, gamma, alpha, g1, g2, zfac=zf, weights=w)
        for name, h, a, r in zip(('d_z', 'd_gamma', 'd_alpha'), have, again, want):
            print('%s %s zfac=%s: max |err| %.3e of %.3e' % (kind, name, zf is not None, float((h - r.reshape(h.shape)).abs().max()),
                                                              float(r.abs().max())))
            close(h, r.cpu().numpy(), 1e-12, name)
            assert torch.equal(h, a), name + ': two calls differ'
        if w is None:                                            # weights=None equals all-ones weights
            for name, h, o in zip(('d_z', 'd_gamma', 'd_alpha'), have,
                                  ops.qx_psi_param_adjoint(z, mu, s, gamma, alpha, g1, g2, zfac=zf, weights=ones)):
                close(h, o.cpu().numpy(), 1e-14, name + ' (None against ones)')
        if kind == 'kernel_off':                                 # a kernel with every weight 0 and g1 = 0: exactly nothing
            off = int(np.flatnonzero((w == 0.0).all(dim=1).cpu().numpy())[0])
            g1z = g1.clone()
            g1z[off] = 0.0
            d_z, d_gamma, d_alpha = ops.qx_psi_param_adjoint(z, mu, s, gamma, alpha, g1z, g2, zfac=zf, weights=w)
            assert bool((d_z[off] == 0.0).all()) and bool((d_gamma[off] == 0.0).all()) and bool(d_alpha[off] == 0.0)


# ------------------------------------------------------------------------------------------------------------------- model
def build_masked(g, dev, obs, y=None, prec=None):
    from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm
    y = g['y'] if y is None else y
    return bayesian_gp_lvm(y, num_latent_dims=g['x_mean'].shape[1], num_inducing_points=g['x_u'].shape[0], device=dev,
                           precision=prec, observed=obs,
                           initial_values=dict(x_mean=g['x_mean'], x_var=softplus(g['x_var_raw']), x_u=g['x_u'],
                                               gamma=softplus(g['gamma_raw']), alpha=softplus(g['alpha_raw']),
                                               beta=softplus(g['beta_raw'])))


def oracle_masked_fhat(y, obs, z, mu, s, gam, al, be):
    """sum over output dims d of the oracle's f_hat of column d on the rows R_d at which d was observed (torch, differentiable)."""
    from oracle import dpgp_oracle_torch as ot
    one = torch.ones((1, 1), dtype=torch.float64)
    f = torch.zeros((), dtype=torch.float64)
    for d in range(obs.shape[1]):
        r = np.flatnonzero(obs[:, d])
        if r.size:
            f = f + ot.fhat_t(y[r, d:d + 1], z, mu[r], s[r], one, gam, al, be)
    return f


def oracle_masked_objective(y, obs, g):
    """-(sum_d f_hat_d over R_d - KL over all rows + hyper-prior) at the fixture's raw variables and its six raw gradients."""
    from oracle import dpgp_oracle_torch as ot
    raw = {k: torch.tensor(np.asarray(g[k], dtype=np.float64), dtype=torch.float64, requires_grad=True) for k in ot.BGPLVM_NAMES}
    yt = torch.as_tensor(np.where(obs, y, 0.0), dtype=torch.float64)
    mu, s = raw['x_mean'], ot._softplus(raw['x_var_raw'])
    gam, al, be = ot._softplus(raw['gamma_raw']), ot._softplus(raw['alpha_raw']), ot._softplus(raw['beta_raw'])
    f = oracle_masked_fhat(yt, obs, raw['x_u'], mu, s, gam, al[:, 0], be[:, 0])
    kl = 0.5 * (torch.sum(mu * mu) + torch.sum(s - torch.log(s)) - mu.shape[0] * mu.shape[1])
    hyper = sum(torch.sum(ot._log_normal_log_pdf(a)) for a in (gam, al, be))
    obj = -(f - kl + hyper)
    grads = torch.autograd.grad(obj, [raw[k] for k in ot.BGPLVM_NAMES])
    return float(obj.detach()), {k: v.numpy() for k, v in zip(ot.BGPLVM_NAMES, grads)}, float(f.detach()), float(kl.detach())


def check_gradients(got, want_of):
    for ref_name, raw_name in REF2RAW.items():
        want = np.asarray(want_of(ref_name))
        have = got[raw_name].cpu().numpy().reshape(want.shape)
        scale = np.abs(want).max()
        print('%s: max |err| %.3e of %.3e' % (ref_name, np.abs(have - want).max(), scale))
        np.testing.assert_allclose(have, want, rtol=0, atol=1e-7 * scale, err_msg=ref_name)


@pytest.mark.parametrize('fixture', FIXTURES)
def test_all_true_mask_equals_the_reference(dev, fixture):
    g = golden(fixture)
    model = build_masked(g, dev, np.ones(g['y'].shape, dtype=bool))
    print('objective %.15g (fixture %.15g)' % (float(model.objective), float(g['objective'])))
    np.testing.assert_allclose(float(model.objective), float(g['objective']), rtol=1e-10)
    assert tuple(model.objective_terms.shape) == (1, 5)
    got = model.gradients()
    assert list(got) == ['x_mean', 'x_var', 'x_u', 'gamma_atoms', 'alpha_atoms', 'beta_atoms']
    for k, v in got.items():
        assert v.shape == model.raw_variables[k].shape, k
    check_gradients(got, lambda name: g['grad_' + name])


@pytest.mark.parametrize('kind', ['random30', 'block', 'odd'])
@pytest.mark.parametrize('fixture', FIXTURES)
def test_general_masks_match_the_oracle(dev, fixture, kind):
    g = golden(fixture)
    y = g['y']
    obs = masks_of(*y.shape, 23)[kind]
    want, grads, _, _ = oracle_masked_objective(y, obs, g)
    model = build_masked(g, dev, obs, y=np.where(obs, y, np.nan))          # unobserved entries are NaN: they are ignored
    have = model.objective
    assert have.dim() == 0 and have.dtype == torch.float64 and have.is_cuda
    print('%s %s: objective %.15g (oracle %.15g)' % (fixture, kind, float(have), want))
    np.testing.assert_allclose(float(have), want, rtol=1e-10)
    slots = len({obs[:, d].tobytes() for d in range(obs.shape[1]) if obs[:, d].any()})
    assert tuple(model.objective_terms.shape) == (slots, 5)
    check_gradients(model.gradients(), lambda name: grads[name])


def synthetic(seed):
    rs = np.random.default_rng(seed)
    t = np.sort(rs.uniform(-2.5, 2.5, 60))
    y = np.sin(1.3 * t[:, None] + np.pi * np.arange(8)[None, :] / 8.0) + 0.05 * rs.standard_normal((60, 8))
    mask = rs.random((60, 8)) >= 0.3
    return y, mask


@pytest.mark.parametrize('seed', [5, 6, 7])
def test_training_and_imputation(dev, seed):
    """x_mean: the PCA (utils.expressions) of the column-mean-filled data with its columns standardised (zero mean, unit
    standard deviation).  Reference figures (CPU oracle + torch Adam, the same formulation): imputation RMSE 0.126 / 0.142 /
    0.130 against 0.713 / 0.745 / 0.722 for column means; the objective falls from about 500 to about 217."""
    from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm
    from dp_gp_lvm_amd.utils import missing
    from dp_gp_lvm_amd.utils.expressions import principal_component_analysis as pca
    y, mask = synthetic(seed)
    filled = missing.column_mean_filled(y, mask)
    x0 = pca(filled, num_latent_dimensions=2)
    x0 = (x0 - x0.mean(axis=0)) / x0.std(axis=0)
    x_u = x0[np.random.default_rng(seed + 100).permutation(60)[:10]]
    model = bayesian_gp_lvm(np.where(mask, y, np.nan), num_latent_dims=2, num_inducing_points=10, device=dev, observed=mask,
                            initial_values=dict(x_mean=x0, x_var=np.full((60, 2), 0.5), x_u=x_u, gamma=np.ones((1, 2)), alpha=1.0,
                                                beta=1.0))
    before = float(model.objective)
    model.optimise(300, learning_rate=0.05)
    after = float(model.objective)
    imputed = model.impute_training_data()
    assert tuple(imputed.shape) == y.shape and imputed.dtype == torch.float64
    imp = imputed.cpu().numpy()
    np.testing.assert_array_equal(imp[mask], y[mask])
    rmse = np.sqrt(np.mean((imp[~mask] - y[~mask]) ** 2))
    rmse_mean = np.sqrt(np.mean((filled[~mask] - y[~mask]) ** 2))
    print('seed %d: objective %.6f -> %.6f; imputation RMSE %.4f, column means %.4f' % (seed, before, after, rmse, rmse_mean))
    assert np.isfinite(after) and after < before
    assert rmse < 0.5 * rmse_mean
    # the posterior-mean formula per column, in NumPy fp64 at the model's final parameters
    from oracle import dpgp_oracle_torch as ot
    z = model.inducing_input.detach().cpu()
    mu = model.q_x[0].detach().cpu()
    s = torch.diagonal(model.q_x[1], dim1=-2, dim2=-1).detach().cpu()
    gam, al, be = (a.detach().cpu() for a in (model.ard_weights, model.signal_variance, model.noise_precision))
    want = np.where(mask, y, 0.0)
    for d in range(8):
        r = np.flatnonzero(mask[:, d])
        yd = torch.as_tensor(y[r, d:d + 1])
        k_uu, p2, _ = ot.psi_pieces_t(yd, z, mu[r], s[r], gam, al[:, 0])
        _, _, v_all = ot.psi_pieces_t(torch.eye(60, dtype=torch.float64), z, mu, s, gam, al[:, 0])     # Psi1^T of every row [1,M,N]
        psi1 = v_all[0].numpy().T                                                                      # [N, M]
        a = k_uu[0].numpy() + float(be) * p2[0].numpy()
        col = float(be) * psi1 @ np.linalg.solve(a, psi1[r].T @ y[r, d])
        want[~mask[:, d], d] = col[~mask[:, d]]
    close(imputed, want, 1e-9, 'imputation')


def test_prediction_on_a_mask_trained_model(dev):
    from oracle import dpgp_oracle as orc
    from oracle import dpgp_oracle_torch as ot
    g = golden(FIXTURES[1])
    p = golden('predb1_bgplvm_70_9_20_4')                                  # its test points, for a model of the same shape
    y = g['y']
    obs = masks_of(*y.shape, 23)['random30']
    model = build_masked(g, dev, obs, y=np.where(obs, y, np.nan))
    _, _, f_train, kl_train = oracle_masked_objective(y, obs, g)
    y_test, xm, xv = p['y_test'], p['x_test_mean'], p['x_test_var']
    assert y_test.shape[1] == y.shape[1] and xm.shape[1] == g['x_mean'].shape[1]
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    gam, al, be = (t(softplus(g[k])) for k in ('gamma_raw', 'alpha_raw', 'beta_raw'))
    # fully observed test points
    f_test = float(oracle_masked_fhat(t(y_test), np.ones(y_test.shape, dtype=bool), t(g['x_u']), t(xm), t(xv), gam, al[:, 0], be[:, 0]))
    kl_t = orc.kl_qx(xm, xv)
    lb, mean, covar, ll = model.predict_new_latent_variables(y_test, x_test_mean=xm, x_test_var=xv)
    print('bound %.15g (want %.15g)' % (float(lb), f_train + f_test - kl_train - kl_t))
    close(model.prediction_terms.sum(), f_test, 1e-10, 'f_hat*')
    close(lb, f_train + f_test - kl_train - kl_t, 1e-10, 'bound')
    close(ll, f_test - f_train, 1e-10, 'test log-likelihood')
    close(mean, xm, 1e-15)
    # test points with their own mask: the gradient's bound pieces against the oracle per column
    obs_t = masks_of(*y_test.shape, 29)['random30']
    mu_t, s_t = t(xm).requires_grad_(), t(xv).requires_grad_()
    f_m = oracle_masked_fhat(t(np.where(obs_t, y_test, 0.0)), obs_t, t(g['x_u']), mu_t, s_t, gam, al[:, 0], be[:, 0])
    d_mu, d_s = torch.autograd.grad(f_m, [mu_t, s_t])
    g_mu, g_s = model.test_latent_gradients(np.where(obs_t, y_test, np.nan), xm, xv, observed=obs_t)
    close(model.prediction_terms.sum(), float(f_m), 1e-10, 'masked f_hat*')
    close(g_mu, d_mu.numpy() - xm, 1e-8, 'd/dmean')
    close(g_s, d_s.numpy() - 0.5 * (1.0 - 1.0 / xv), 1e-8, 'd/dvar')
    g_mu, _ = model.test_latent_gradients(y_test, xm, xv)
    assert bool(torch.isfinite(g_mu).all())
    # default starts: the jointly observed nearest neighbour, with and without a test mask
    np.random.seed(0)
    rows = y[[3, 17, 8]]
    out = model.predict_new_latent_variables(np.where(obs[[3, 17, 8]], rows, 0.0) + 0.0)
    assert bool(torch.isfinite(out[0]))
    xm2, xv2 = model.optimise_test_latents(np.where(obs_t, y_test, np.nan), 5, learning_rate=0.01, observed=obs_t)
    assert tuple(xm2.shape) == xm.shape and bool(torch.isfinite(xm2).all()) and bool((xv2 > 0).all())
    xm3, _ = model.optimise_test_latents(y_test, 3)
    assert bool(torch.isfinite(xm3).all())
    with pytest.raises(NotImplementedError, match='impute_training_data'):
        model.predict_missing_data(np.where(obs_t, y_test, np.nan), observed=obs_t)
    with pytest.raises(NotImplementedError, match='impute_training_data'):
        model.predict_missing_data(y_test[:, :5])


def test_argument_checks(dev):
    g = golden(FIXTURES[0])
    y = g['y']
    obs = masks_of(*y.shape, 23)['random30']
    build_masked(g, dev, obs, prec='f64')                                   # fine
    with pytest.raises(AssertionError):
        build_masked(g, dev, obs, prec='mixed')
    with pytest.raises(AssertionError):
        build_masked(g, dev, obs.astype(np.float64))                        # not boolean
    with pytest.raises(AssertionError):
        build_masked(g, dev, obs[:-1])                                      # shape mismatch
    with pytest.raises(AssertionError):
        build_masked(g, dev, np.zeros(y.shape, dtype=bool))                 # nothing observed
    from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm
    plain = bayesian_gp_lvm(y, num_latent_dims=3, num_inducing_points=12, device=dev)
    with pytest.raises(AssertionError):
        plain.impute_training_data()
    assert plain.objective_terms is None


def test_default_initial_values_with_a_mask(dev):
    from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm
    y, mask = synthetic(5)
    model = bayesian_gp_lvm(np.where(mask, y, np.nan), num_latent_dims=2, num_inducing_points=10, device=dev, observed=mask)
    assert tuple(model.inducing_input.shape) == (10, 2) and tuple(model.q_x[0].shape) == (60, 2)
    np.testing.assert_allclose(torch.diagonal(model.q_x[1], dim1=-2, dim2=-1).cpu().numpy(), 0.5, rtol=1e-12)
    before = float(model.objective)
    model.optimise(20, learning_rate=0.01)
    assert float(model.objective) < before
