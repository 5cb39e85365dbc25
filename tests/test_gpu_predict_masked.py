"""GPU tests of prediction with per-entry observation masks (predict_missing_data / test_latent_gradients /
optimise_test_latents with observed=...) for bayesian_gp_lvm and dp_gp_lvm, and of the two weighted operators under them,
dpgp_qx_psi_stats_weighted_f64 and dpgp_qx_psi_adjoint_weighted_f64 (csrc/qx_psi.hip).

References: fp64 torch autograd of a plain restatement (operators); the reference's own fixtures for masks that are its
"first Do columns" case; the committed fp64 oracle, evaluated per output dim on the test points at which that dim was
observed, for general masks; the existing suffix interface on a model with permuted columns for non-suffix column sets.
Tolerances are those of test_gpu_predict_b1.py / test_gpu_predict.py for the same quantities."""
import itertools

import numpy as np
import pytest
import torch

from conftest import golden
from test_gpu_model_t import build as build_dp
from test_gpu_predict_b1 import build_bgplvm, close, random_case

pytestmark = pytest.mark.gpu
BGPLVM = ['predb1_bgplvm_40_6_12_3', 'predb1_bgplvm_70_9_20_4', 'predb1_bgplvm_150_12_136_8']
DP = ['predict_ref_40_6_12_3_T4', 'predict_ref_60_10_15_4_T5']


# --------------------------------------------------------------------------------------------------------------- operators
def restated(z, mu, s, gamma, alpha, g1, g2, w):
    """sum_b <g1_b, Psi1_b> + <g2_b, Psi2_b> with Psi2_b = sum_n w[b,n] (test point n's term), and its gradient with respect
    to (mu, s), by torch autograd of a plain restatement of rbf_kernel.py:135-199 (the restated() of test_gpu_predict_b1.py
    with the weights on the Psi2 sum; Psi2 in chunks of test points)."""
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
        p2 = (w[:, n0:n0 + step, None, None] * torch.exp(lg)).sum(dim=1)
        psi2 = psi2 + p2.detach()
        f = f + torch.sum(g2 * p2)
    d_mu, d_s = torch.autograd.grad(f, [mu, s])
    return psi1.detach(), psi2, d_mu, d_s


def weights_of(kind, b, n, seed, dev):
    rs = np.random.default_rng(seed)
    if kind == 'binary':                                     # 0 / 1, about 40 % zeros
        w = (rs.random((b, n)) >= 0.4).astype(np.float64)
    elif kind == 'kernel_off':                               # one kernel with every weight 0, the others 0 / 1
        w = (rs.random((b, n)) >= 0.4).astype(np.float64)
        w[rs.integers(0, b)] = 0.0
    else:                                                    # any finite reals
        w = rs.standard_normal((b, n))
    return torch.as_tensor(w, dtype=torch.float64, device=dev).contiguous()


@pytest.mark.parametrize('kind', ['binary', 'kernel_off', 'normal'])
@pytest.mark.parametrize('b,m,q,n', list(itertools.product([1, 5], [1, 17, 64, 128, 200], [1, 10, 23], [1, 300])))
def test_weighted_operators_match_autograd_of_the_restatement(dev, b, m, q, n, kind):
    from dp_gp_lvm_amd import ops
    seed = 1000 * b + 10 * m + q + n
    z, mu, s, gamma, alpha, g1, g2 = random_case(dev, b, n, m, q, seed)
    w = weights_of(kind, b, n, seed + 1, dev)
    psi1_r, psi2_r, dmu_r, ds_r = restated(z, mu, s, gamma, alpha, g1, g2, w)
    zfac = ops.qx_pair_factor(z, gamma, alpha)
    for zf in (None, zfac):
        psi1, psi2 = ops.qx_psi_stats_batched(z, mu, s, gamma, alpha, zfac=zf, weights=w)
        close(psi1, psi1_r.cpu().numpy(), 1e-12, 'psi1')
        close(psi2, psi2_r.cpu().numpy(), 1e-12, 'psi2')
        assert torch.equal(psi2, psi2.transpose(1, 2))
        d_mu, d_s = ops.qx_psi_adjoint(z, mu, s, gamma, alpha, g1, g2, zfac=zf, weights=w)
        close(d_mu, dmu_r.cpu().numpy(), 1e-12, 'd_mu')
        close(d_s, ds_r.cpu().numpy(), 1e-12, 'd_s')


@pytest.mark.parametrize('b,n,m,q', [(5, 300, 200, 23), (1, 100, 50, 10)])
def test_unit_and_absent_weights_give_the_unweighted_bits(dev, b, n, m, q):
    """weights=None (the old entry points), the new entry points with w = NULL, and weights all 1.0 agree bit for bit; two runs
    with the same weights too."""
    from dp_gp_lvm_amd import _lib, ops
    z, mu, s, gamma, alpha, g1, g2 = random_case(dev, b, n, m, q, 7)
    ones = torch.ones((b, n), dtype=torch.float64, device=dev)
    l = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    for zf in (None, ops.qx_pair_factor(z, gamma, alpha)):
        zp = None if zf is None else zf.data_ptr()
        p_old = ops.qx_psi_stats_batched(z, mu, s, gamma, alpha, zfac=zf)
        p_one = ops.qx_psi_stats_batched(z, mu, s, gamma, alpha, zfac=zf, weights=ones)
        a_old = ops.qx_psi_adjoint(z, mu, s, gamma, alpha, g1, g2, zfac=zf)
        a_one = ops.qx_psi_adjoint(z, mu, s, gamma, alpha, g1, g2, zfac=zf, weights=ones)
        # the weighted entry points with a NULL weight pointer
        p_null = (torch.empty_like(p_old[0]), torch.empty_like(p_old[1]))
        wsb = l.dpgp_qx_psi_stats_workspace_bytes(b, n, m, q)
        ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
        assert l.dpgp_qx_psi_stats_weighted_f64(b, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                                alpha.data_ptr(), zp, None, p_null[0].data_ptr(), p_null[1].data_ptr(),
                                                ws.data_ptr(), wsb, st) == 0
        a_null = (torch.empty_like(a_old[0]), torch.empty_like(a_old[1]))
        wsb2 = l.dpgp_qx_psi_adjoint_workspace_bytes(b, n, m, q)
        ws2 = torch.empty(max(wsb2, 256), dtype=torch.uint8, device=dev)
        assert l.dpgp_qx_psi_adjoint_weighted_f64(b, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                                  alpha.data_ptr(), zp, None, g1.data_ptr(), g2.data_ptr(), a_null[0].data_ptr(),
                                                  a_null[1].data_ptr(), ws2.data_ptr(), wsb2, st) == 0
        torch.cuda.synchronize()
        for have in (p_one, p_null):
            assert torch.equal(have[0], p_old[0]) and torch.equal(have[1], p_old[1])
        for have in (a_one, a_null):
            assert torch.equal(have[0], a_old[0]) and torch.equal(have[1], a_old[1])
    w = weights_of('normal', b, n, 11, dev)
    p, r = (ops.qx_psi_stats_batched(z, mu, s, gamma, alpha, weights=w) for _ in range(2))
    assert torch.equal(p[0], r[0]) and torch.equal(p[1], r[1])
    a, c = (ops.qx_psi_adjoint(z, mu, s, gamma, alpha, g1, g2, weights=w) for _ in range(2))
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


@pytest.mark.parametrize('b,n,m,q', [(5, 300, 200, 23), (3, 130, 40, 10)])
def test_zero_weight_rows_have_exactly_zero_gradient(dev, b, n, m, q):
    from dp_gp_lvm_amd import ops
    z, mu, s, gamma, alpha, g1, g2 = random_case(dev, b, n, m, q, 13)
    rs = np.random.default_rng(17)
    rows = np.unique(np.concatenate([rs.integers(0, n, 20), np.arange(64, min(n, 128))]))    # scattered rows and a whole wave
    w = weights_of('normal', b, n, 19, dev)
    w[:, rows] = 0.0
    d_mu, d_s = ops.qx_psi_adjoint(z, mu, s, gamma, alpha, torch.zeros_like(g1), g2, weights=w)
    assert bool((d_mu[rows] == 0.0).all()) and bool((d_s[rows] == 0.0).all())
    keep = np.setdiff1d(np.arange(n), rows)
    assert bool((d_mu[keep] != 0.0).any())
    # a kernel with every weight 0 contributes an exactly zero Psi2
    w[1] = 0.0
    assert bool((ops.qx_psi_stats_batched(z, mu, s, gamma, alpha, weights=w)[1][1] == 0.0).all())


# ------------------------------------------------------------------------------------------- suffix masks: the reference's case
def suffix_mask(y_test, do):
    obs = np.zeros(y_test.shape, dtype=bool)
    obs[:, :do] = True
    return np.where(obs, y_test, np.nan), obs


@pytest.mark.parametrize('fixture', BGPLVM)
def test_bgplvm_suffix_mask_matches_the_reference(dev, fixture):
    g = golden(fixture)
    model = build_bgplvm(g, dev)
    xm, xv, do = g['x_test_mean'], g['x_test_var'], int(g['n_observed'])
    y_nan, obs = suffix_mask(g['y_test'], do)
    mlb, mean, covar, pmean, pcovar = model.predict_missing_data(y_nan, x_test_mean=xm, x_test_var=xv, observed=obs)
    close(mlb, g['missing_lower_bound'], 1e-10, 'missing-data bound')
    close(pmean, g['predicted_mean'], 1e-10, 'predicted mean')
    close(pcovar, g['predicted_covar'], 1e-10, 'predicted covariance')
    close(mean, xm, 1e-15)
    close(torch.diagonal(covar, dim1=-2, dim2=-1), xv, 1e-15)
    np.testing.assert_array_equal(model.missing_columns, np.arange(do, g['y_test'].shape[1]))
    assert tuple(model.prediction_terms.shape) == (1, 5)
    g_mu, g_s = model.test_latent_gradients(y_nan, xm, xv, observed=obs)
    close(g_mu, g['missing_grad_mean'], 1e-8, 'd/dmean')
    close(g_s, g['missing_grad_var'], 1e-8, 'd/dvar')


@pytest.mark.parametrize('fixture', DP)
def test_dp_gp_lvm_suffix_mask_matches_the_reference(dev, fixture):
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
    g = golden(fixture)
    model = build_dp(dp_gp_lvm, g, dev, 'f64')
    do, xm = int(g['n_observed']), g['missing_x_test_mean']
    y_nan, obs = suffix_mask(g['y_test'], do)
    lb, _, _, mean, covar = model.predict_missing_data(y_nan, x_test_mean=xm, observed=obs)
    np.testing.assert_allclose(float(lb), float(g['missing_lower_bound_clean']), rtol=1e-9)
    assert mean.shape == g['predicted_mean'].shape and covar.shape == g['predicted_covar'].shape
    np.testing.assert_allclose(mean.cpu().numpy(), g['predicted_mean'], rtol=0, atol=1e-8 * np.abs(g['predicted_mean']).max())
    np.testing.assert_allclose(covar.cpu().numpy(), g['predicted_covar'], rtol=0, atol=1e-8 * np.abs(g['predicted_covar']).max())
    np.testing.assert_array_equal(model.missing_columns, np.arange(do, g['y_test'].shape[1]))
    assert tuple(model.prediction_terms.shape) == (do, 5)
    xv = 0.5 + np.random.default_rng(0).random(xm.shape)
    want = model.test_latent_gradients(g['y_test'][:, :do], xm, xv)
    have = model.test_latent_gradients(y_nan, xm, xv, observed=obs)
    close(have[0], want[0].cpu().numpy(), 1e-8, 'd/dmean')
    close(have[1], want[1].cpu().numpy(), 1e-8, 'd/dvar')


# ------------------------------------------------------------------------------------------------ general masks: the oracle
def masks_of(n_t, d, seed):
    rs = np.random.default_rng(seed)
    random30 = rs.random((n_t, d)) >= 0.3
    block = np.ones((n_t, d), dtype=bool)
    block[n_t // 4:3 * n_t // 4 + 1, d // 3:2 * d // 3 + 1] = False
    odd = rs.random((n_t, d)) >= 0.2
    odd[:, 2] = False                                        # a column never observed
    odd[:, d - 2] = False
    odd[1, d - 2] = True                                     # a column observed in exactly one row
    odd[n_t // 2, :] = False                                 # a row never observed
    assert odd[:, d - 2].sum() == 1 and n_t // 2 != 1
    return dict(random30=random30, block=block, odd=odd)


def oracle_masked(y_test, obs, z, mu, s, gamma, alpha, beta):
    """f_hat* = sum over output dims d of the oracle's f_hat of column d on the test points R_d at which d was observed
    (gamma [D,Q], alpha [D], beta [D]: that dim's kernel), and its gradient with respect to (mu, s) scattered into rows R_d."""
    from oracle import dpgp_oracle as orc
    from oracle import dpgp_oracle_torch as orct
    f, d_mu, d_s = 0.0, np.zeros_like(mu), np.zeros_like(s)
    for d in range(obs.shape[1]):
        r = np.flatnonzero(obs[:, d])
        if r.size == 0:
            continue
        args = (y_test[r, d:d + 1], z, mu[r], s[r], gamma[d:d + 1], alpha[d:d + 1], beta[d:d + 1])
        f += orc.fhat_terms(*args).sum()
        gr = orct.fhat_input_gradients(*args)
        d_mu[r] += gr['d_mu']
        d_s[r] += gr['d_s']
    return f, d_mu, d_s


@pytest.mark.parametrize('kind', ['random30', 'block', 'odd'])
@pytest.mark.parametrize('fixture', ['predb1_bgplvm_70_9_20_4', 'predb1_bgplvm_150_12_136_8'])
def test_bgplvm_general_masks_match_the_oracle(dev, fixture, kind):
    from oracle import dpgp_oracle as orc
    from test_gpu_predict_b1 import softplus
    g = golden(fixture)
    model = build_bgplvm(g, dev)
    y_test, xm, xv = g['y_test'], g['x_test_mean'], g['x_test_var']
    n_t, dd = y_test.shape
    obs = masks_of(n_t, dd, 23)[kind]
    y_nan = np.where(obs, y_test, np.nan)
    rep = lambda a: np.repeat(softplus(a).reshape(1, -1), dd, axis=0)
    f_want, dmu_want, ds_want = oracle_masked(y_test, obs, g['x_u'], xm, xv, rep(g['gamma_raw']), rep(g['alpha_raw'])[:, 0],
                                              rep(g['beta_raw'])[:, 0])
    kl_t = orc.kl_qx(xm, xv)
    # the training side f_hat - KL(q(X)) from an unmasked call: bound = f_hat + f_hat*(full) - KL - KL*
    lb_full = float(model.predict_new_latent_variables(y_test, x_test_mean=xm, x_test_var=xv)[0])
    train = lb_full - float(model.prediction_terms.sum()) + kl_t
    lb, _, _, pmean, pcovar = model.predict_missing_data(y_nan, x_test_mean=xm, x_test_var=xv, observed=obs)
    f_have = float(model.prediction_terms.sum())
    print('%s %s: f_hat* %.15g (oracle %.15g), bound %.15g (want %.15g)' % (fixture, kind, f_have, f_want, float(lb),
                                                                            train + f_want - kl_t))
    close(f_have, f_want, 1e-10, 'f_hat*')
    close(lb, train + f_want - kl_t, 1e-10, 'bound')
    mc = np.flatnonzero(~obs.all(axis=0))
    np.testing.assert_array_equal(model.missing_columns, mc)
    assert tuple(pmean.shape) == (n_t, mc.size) and tuple(pcovar.shape) == (mc.size, n_t, n_t)
    g_mu, g_s = model.test_latent_gradients(y_nan, xm, xv, observed=obs)
    close(g_mu, dmu_want - xm, 1e-8, 'd/dmean')
    close(g_s, ds_want - 0.5 * (1.0 - 1.0 / xv), 1e-8, 'd/dvar')


@pytest.mark.parametrize('kind', ['random30', 'block', 'odd'])
def test_dp_gp_lvm_general_masks_match_the_oracle(dev, kind):
    from oracle import dpgp_oracle as orc
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
    g = golden('predict_ref_60_10_15_4_T5')
    model = build_dp(dp_gp_lvm, g, dev, 'f64')
    y_test, xm = g['y_test'], g['new_x_test_mean']
    xv = 0.5 + np.random.default_rng(0).random(xm.shape)
    n_t, dd = y_test.shape
    obs = masks_of(n_t, dd, 29)[kind]
    y_nan = np.where(obs, y_test, np.nan)
    gam, al, be = (a.detach().cpu().numpy() for a in (model.ard_weights, model.signal_variance, model.noise_precision))
    f_want, dmu_want, ds_want = oracle_masked(y_test, obs, g['x_u'], xm, xv, gam, al.reshape(-1), be.reshape(-1))
    terms = model.objective_terms.cpu().numpy()                          # (objective, f_hat, KL, DP objective, hyper-prior)
    want = terms[1] + f_want - terms[2] - orc.kl_qx(xm, xv)
    lb, _, _, pmean, pcovar = model.predict_missing_data(y_nan, x_test_mean=xm, x_test_var=xv, observed=obs)
    f_have = float(model.prediction_terms.sum())
    print('%s: f_hat* %.15g (oracle %.15g), bound %.15g (want %.15g)' % (kind, f_have, f_want, float(lb), want))
    np.testing.assert_allclose(f_have, f_want, rtol=1e-9)
    np.testing.assert_allclose(float(lb), want, rtol=1e-9)
    mc = np.flatnonzero(~obs.all(axis=0))
    np.testing.assert_array_equal(model.missing_columns, mc)
    assert tuple(model.prediction_terms.shape) == (int(obs.any(axis=0).sum()), 5)
    assert tuple(pmean.shape) == (n_t, mc.size) and tuple(pcovar.shape) == (mc.size, n_t, n_t)
    g_mu, g_s = model.test_latent_gradients(y_nan, xm, xv, observed=obs)
    close(g_mu, dmu_want - xm, 1e-8, 'd/dmean')
    close(g_s, ds_want - 0.5 * (1.0 - 1.0 / xv), 1e-8, 'd/dvar')


# ------------------------------------------------------------------------- non-suffix column sets through the existing interface
def column_mask(n_t, d, missing_cols):
    obs = np.ones((n_t, d), dtype=bool)
    obs[:, missing_cols] = False
    perm = np.concatenate([np.setdiff1d(np.arange(d), missing_cols), np.sort(missing_cols)])
    return obs, perm


@pytest.mark.parametrize('fixture', BGPLVM)
def test_bgplvm_column_mask_equals_the_suffix_interface_on_permuted_columns(dev, fixture):
    g = golden(fixture)
    y_test, xm, xv = g['y_test'], g['x_test_mean'], g['x_test_var']
    miss = np.array([1, 4])
    obs, perm = column_mask(*y_test.shape, miss)
    model = build_bgplvm(g, dev)
    lb, _, _, pmean, pcovar = model.predict_missing_data(np.where(obs, y_test, np.nan), x_test_mean=xm, x_test_var=xv,
                                                         observed=obs)
    np.testing.assert_array_equal(model.missing_columns, miss)
    permuted = build_bgplvm(g, dev, y=g['y'][:, perm])
    lb_p, _, _, pmean_p, pcovar_p = permuted.predict_missing_data(y_test[:, perm][:, :perm.size - miss.size], x_test_mean=xm,
                                                                  x_test_var=xv)
    close(lb, lb_p.cpu().numpy(), 1e-10, 'bound')
    close(pmean, pmean_p.cpu().numpy(), 1e-10, 'predicted mean')
    close(pcovar, pcovar_p.cpu().numpy(), 1e-10, 'predicted covariance')


@pytest.mark.parametrize('fixture', DP)
def test_dp_gp_lvm_column_mask_equals_the_suffix_interface_on_permuted_columns(dev, fixture):
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
    g = golden(fixture)
    y_test, xm = g['y_test'], g['missing_x_test_mean']
    miss = np.array([1, 4])
    obs, perm = column_mask(*y_test.shape, miss)
    model = build_dp(dp_gp_lvm, g, dev, 'f64')
    lb, _, _, pmean, pcovar = model.predict_missing_data(np.where(obs, y_test, np.nan), x_test_mean=xm, observed=obs)
    np.testing.assert_array_equal(model.missing_columns, miss)
    gp = dict(g)
    gp['y'], gp['dp_logits'] = g['y'][:, perm], g['dp_logits'][perm]
    permuted = build_dp(dp_gp_lvm, gp, dev, 'f64')
    lb_p, _, _, pmean_p, pcovar_p = permuted.predict_missing_data(y_test[:, perm][:, :perm.size - miss.size], x_test_mean=xm)
    np.testing.assert_allclose(float(lb), float(lb_p), rtol=1e-9)
    pmean_p, pcovar_p = pmean_p.cpu().numpy(), pcovar_p.cpu().numpy()
    np.testing.assert_allclose(pmean.cpu().numpy(), pmean_p, rtol=0, atol=1e-8 * np.abs(pmean_p).max())
    np.testing.assert_allclose(pcovar.cpu().numpy(), pcovar_p, rtol=0, atol=1e-8 * np.abs(pcovar_p).max())


# ------------------------------------------------------------------------------------------------------------ other checks
def test_an_all_true_mask_gives_the_unmasked_gradient(dev):
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
    g = golden(BGPLVM[1])
    model = build_bgplvm(g, dev)
    y_test, xm, xv = g['y_test'], g['x_test_mean'], g['x_test_var']
    obs = np.ones(y_test.shape, dtype=bool)
    want = model.test_latent_gradients(y_test, xm, xv)
    have = model.test_latent_gradients(y_test, xm, xv, observed=obs)
    close(have[0], want[0].cpu().numpy(), 1e-12, 'B-GPLVM d/dmean')
    close(have[1], want[1].cpu().numpy(), 1e-12, 'B-GPLVM d/dvar')
    g = golden(DP[1])
    model = build_dp(dp_gp_lvm, g, dev, 'f64')
    y_test, xm = g['y_test'], g['new_x_test_mean']
    xv = 0.5 + np.random.default_rng(0).random(xm.shape)
    want = model.test_latent_gradients(y_test, xm, xv)
    have = model.test_latent_gradients(y_test, xm, xv, observed=np.ones(y_test.shape, dtype=bool))
    close(have[0], want[0].cpu().numpy(), 1e-8, 'dp_gp_lvm d/dmean')
    close(have[1], want[1].cpu().numpy(), 1e-8, 'dp_gp_lvm d/dvar')


def test_optimise_test_latents_raises_the_masked_bound(dev):
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
    g = golden(BGPLVM[1])
    gd = golden(DP[1])
    cases = [(build_bgplvm(g, dev), g['y_test'], g['x_test_mean'], g['x_test_var']),
             (build_dp(dp_gp_lvm, gd, dev, 'mixed'), gd['y_test'], gd['new_x_test_mean'], np.ones_like(gd['new_x_test_mean']))]
    for model, y_test, xm0, xv0 in cases:
        obs = np.random.default_rng(31).random(y_test.shape) >= 0.3
        assert not obs.all() and obs.any()
        y_nan = np.where(obs, y_test, np.nan)
        before = float(model.predict_missing_data(y_nan, x_test_mean=xm0, x_test_var=xv0, observed=obs)[0])
        xm, xv = model.optimise_test_latents(y_nan, 50, learning_rate=0.05, x_test_mean=xm0, x_test_var=xv0, observed=obs)
        after = float(model.predict_missing_data(y_nan, x_test_mean=xm, x_test_var=xv, observed=obs)[0])
        print('masked bound before %.9g after %.9g' % (before, after))
        assert np.isfinite(after) and after > before, (before, after)


def test_default_initialisation_with_a_mask(dev):
    """No x_test_mean: the masked nearest neighbour + N(0, 0.01^2); a row with nothing observed starts at 0."""
    g = golden(BGPLVM[1])
    model = build_bgplvm(g, dev)
    y_test = g['y'][[3, 17, 5, 8]] + 1e-3
    obs = np.random.default_rng(37).random(y_test.shape) >= 0.3
    obs[2] = False
    np.random.seed(0)
    lb, xm, _, _, _ = model.predict_missing_data(np.where(obs, y_test, np.nan), observed=obs)
    assert bool(torch.isfinite(lb))
    xm = xm.cpu().numpy()
    assert np.abs(xm[[0, 1, 3]] - g['x_mean'][[3, 17, 8]]).max() < 0.06 and np.abs(xm[2]).max() < 0.06


def test_argument_checks(dev):
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
    g, gd = golden(BGPLVM[0]), golden(DP[0])
    for model, y_test, xm in ((build_bgplvm(g, dev), g['y_test'], g['x_test_mean']),
                              (build_dp(dp_gp_lvm, gd, dev, 'f64'), gd['y_test'], gd['missing_x_test_mean'])):
        xv = np.ones_like(xm)
        obs = np.random.default_rng(41).random(y_test.shape) >= 0.3
        kw = dict(x_test_mean=xm, x_test_var=xv)
        model.predict_missing_data(y_test, observed=obs, **kw)                                      # fine
        with pytest.raises(AssertionError):
            model.predict_missing_data(y_test[:, :-1], observed=obs[:, :-1], **kw)                  # y_test must be [N* x D]
        with pytest.raises(AssertionError):
            model.predict_missing_data(y_test, observed=obs[:-1], **kw)                             # shape mismatch
        with pytest.raises(AssertionError):
            model.predict_missing_data(y_test, observed=obs.astype(np.float64), **kw)               # not boolean
        with pytest.raises(AssertionError):
            model.predict_missing_data(y_test, observed=np.ones(y_test.shape, dtype=bool), **kw)    # nothing missing
        with pytest.raises(AssertionError):
            model.predict_missing_data(y_test, observed=obs, reference_compat=True, **kw)
        with pytest.raises(AssertionError):
            model.test_latent_gradients(y_test, xm, xv, observed=obs.astype(np.int64))
        with pytest.raises(AssertionError):
            model.optimise_test_latents(y_test, 1, observed=obs[:, :-1], **kw)
        # observed=None: the existing paths and their assertions
        with pytest.raises(AssertionError):
            model.predict_missing_data(y_test, **kw)                                                # width D
        do = y_test.shape[1] - 2
        out = model.predict_missing_data(y_test[:, :do], **kw)
        assert tuple(out[3].shape) == (y_test.shape[0], 2)
        np.testing.assert_array_equal(model.missing_columns, [do, do + 1])


def test_ops_refuse_bad_weights(dev):
    from dp_gp_lvm_amd import ops
    z, mu, s, gamma, alpha, g1, g2 = random_case(dev, 2, 9, 5, 3, 1)
    w = torch.ones((2, 9), dtype=torch.float64, device=dev)
    with pytest.raises(AssertionError):
        ops.qx_psi_stats_batched(z, mu, s, gamma, alpha, weights=w[:, :-1].contiguous())
    with pytest.raises(TypeError):
        ops.qx_psi_stats_batched(z, mu, s, gamma, alpha, weights=w.float())
    with pytest.raises(TypeError):
        ops.qx_psi_adjoint(z, mu, s, gamma, alpha, g1, g2, weights=w.t().contiguous().t())
    with pytest.raises(RuntimeError):
        ops.qx_psi_adjoint(z, mu, s, gamma, alpha, g1, g2, weights=w.cpu())
