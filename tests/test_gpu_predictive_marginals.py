"""GPU tests of the per-entry predictive moments of bayesian_gp_lvm, manifold_relevance_determination and dp_gp_lvm (over-D):
predictive_marginals, predict_missing_data(marginal_variance=True) (models/marginals.py on ops.qx_psi_point_moments).  Moments
against the NumPy restatement of test_gpu_predict_t.moments_numpy (one atom: per-point Psi statistics from the oracle,
np.linalg.solve) at 1e-9, the moments tolerance of the over-T model; means against predict_missing_data's at 1e-10; the sum of
the variances over the test points against the reference-pinned [Du x N* x N*] array."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_gpu_model_t import build as build_dp
from test_gpu_mrd_masked import build as build_mrd_masked
from test_gpu_predict_b1 import build_bgplvm, build_mrd, close, softplus
from test_gpu_predict_t import build_t, moments_numpy
from test_gpu_train_masked import build_masked

pytestmark = pytest.mark.gpu
BGPLVM, MRD, OVER_D = 'predb1_bgplvm_40_6_12_3', 'predb1_mrd_50_2views_12_3', 'predict_ref_40_6_12_3_T4'
N_T = 7
_WANT = {}


def scalar(a):
    return float(np.asarray(a).reshape(-1)[0])


def t64(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def one_atom(z, gamma, alpha, beta, mu, s, d):
    """The values of a one-kernel model in the layout of test_gpu_predict_t.values_of (T = 1)."""
    return dict(z=t64(z), gat=t64(gamma).reshape(1, -1), aat=t64(alpha).reshape(1), bat=t64(beta).reshape(1), phi=torch.ones((d, 1),
                dtype=torch.float64), mu=t64(mu), s=t64(s))


def values_b(g):
    return one_atom(g['x_u'], softplus(g['gamma_raw']), softplus(g['alpha_raw']), softplus(g['beta_raw']), g['x_mean'],
                    softplus(g['x_var_raw']), g['y'].shape[1])


def values_view(g, v):
    return one_atom(g['x_u_%d' % v], softplus(g['gamma_raw_%d' % v]), softplus(g['alpha_raw_%d' % v]), softplus(g['beta_raw_%d' % v]),
                    g['x_mean'], softplus(g['x_var_raw']), g['view_%d' % v].shape[1])


def points(x_mean, n_t, seed):
    """A q(X*) near permuted training latent points."""
    rs = np.random.default_rng(seed)
    idx = np.resize(rs.permutation(x_mean.shape[0]), n_t)
    xm = x_mean[idx] + 0.05 * rs.standard_normal((n_t, x_mean.shape[1]))
    return idx, xm, rs.uniform(0.3, 1.0, xm.shape)


def mask(n, d, seed):
    """30 % missing at random, a column never observed (1) and a row never observed (n // 3)."""
    obs = np.random.default_rng(seed).random((n, d)) >= 0.3
    obs[:, 1] = False
    obs[n // 3, :] = False
    return obs


def want_of(key, v, y, obs, xm, xv):
    """The NumPy restatement, once per case."""
    if key not in _WANT:
        _WANT[key] = moments_numpy(v, np.where(obs, y, 0.0), obs, xm, xv, list(range(y.shape[1])))
    return _WANT[key]


def check(tag, mean, var, want):
    for name, have, w in (('mean', mean, want[0]), ('var', var, want[1])):
        print('%s %s: max |err| %.3e of %.3e (bound 1e-9)' % (tag, name, np.abs(have.cpu().numpy() - w).max(), np.abs(w).max()))
        close(have, w, 1e-9, '%s %s' % (tag, name))


# ------------------------------------------------------------------------------------------------------------ bayesian_gp_lvm
def test_bgplvm_moments_match_the_numpy_restatement(dev):
    g = golden(BGPLVM)
    model = build_bgplvm(g, dev)
    n, d = g['y'].shape
    _, xm, xv = points(g['x_mean'], N_T, 3)
    want = want_of('b', values_b(g), g['y'], np.ones((n, d), dtype=bool), xm, xv)
    mean, var = model.predictive_marginals(xm, xv)
    assert tuple(mean.shape) == (N_T, d) == tuple(var.shape)
    check('complete', mean, var, want)
    some = [d - 1, 0, 2]
    mean_s, var_s = model.predictive_marginals(xm, xv, columns=some)
    check('chosen columns', mean_s, var_s, (want[0][:, some], want[1][:, some]))
    assert float(var.min()) > 1.0 / scalar(softplus(g['beta_raw']))
    with pytest.raises(AssertionError):
        model.predictive_marginals(xm, xv, columns=[d])


def test_bgplvm_means_identity_and_marginal_variance(dev):
    g = golden(BGPLVM)
    model = build_bgplvm(g, dev)
    do, beta = int(g['n_observed']), scalar(softplus(g['beta_raw']))
    d = g['y'].shape[1]
    idx, xm7, xv7 = points(g['x_mean'], N_T, 3)
    for tag, y_test, xm, xv in (('fixture', g['y_test'], g['x_test_mean'], g['x_test_var']), ('7 points', g['y'][idx], xm7, xv7)):
        n_t = xm.shape[0]
        out = model.predict_missing_data(y_test[:, :do], x_test_mean=xm, x_test_var=xv)
        mean, var = model.predictive_marginals(xm, xv, columns=np.arange(do, d))
        close(mean, out[3].cpu().numpy(), 1e-10, tag + ': mean against predicted_mean')
        # sum_n var(n,d) = covar[d,0,0] + (N* - 1)/beta: the reference-pinned array
        close(var.sum(dim=0), (out[4][:, 0, 0] + (n_t - 1) / beta).cpu().numpy(), 1e-9, tag + ': sum of variances')
        assert tuple(out[4].shape) == (d - do, n_t, n_t)
        out_v = model.predict_missing_data(y_test[:, :do], x_test_mean=xm, x_test_var=xv, marginal_variance=True)
        assert tuple(out_v[4].shape) == (n_t, d - do) and torch.equal(out_v[4], var) and torch.equal(out_v[3], out[3])
        assert float(out_v[0]) == float(out[0])
    # the default output is what it was: the reference's array
    out = model.predict_missing_data(g['y_test'][:, :do], x_test_mean=g['x_test_mean'], x_test_var=g['x_test_var'])
    close(out[4], g['predicted_covar'], 1e-10, 'predicted covariance (default)')
    # with a test mask: the columns with an unobserved entry
    obs_t = np.random.default_rng(11).random((N_T, d)) >= 0.3
    obs_t[:, 0] = True
    y_nan = np.where(obs_t, g['y'][idx], np.nan)
    out = model.predict_missing_data(y_nan, x_test_mean=xm7, x_test_var=xv7, observed=obs_t)
    out_v = model.predict_missing_data(y_nan, x_test_mean=xm7, x_test_var=xv7, observed=obs_t, marginal_variance=True)
    cols = list(model.missing_columns)
    mean, var = model.predictive_marginals(xm7, xv7, columns=cols)
    assert tuple(out[4].shape) == (len(cols), N_T, N_T) and torch.equal(out_v[4], var)
    close(mean, out[3].cpu().numpy(), 1e-10, 'masked test points: mean against predicted_mean')
    close(var.sum(dim=0), (out[4][:, 0, 0] + (N_T - 1) / beta).cpu().numpy(), 1e-9, 'masked test points: sum of variances')


def gp_variance_at_points(dev, z, mu, s, gamma, alpha, beta, xt, weights=None):
    """alpha - k*^T (K^-1 - P) k* + 1/beta at the points xt [N* x Q] (no input uncertainty), P = (K + beta Psi2)^-1 with Psi2 of the
    training q(X) = (mu, s) over the rows of `weights` (default all); K and k* from ops.ard_rbf_gram."""
    from dp_gp_lvm_amd import ops
    dv = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=dev)
    z, mu, s, xt = dv(z), dv(mu), dv(s), dv(xt)
    gamma, alpha, beta = dv(gamma).reshape(1, -1), dv(alpha).reshape(1), dv(beta).reshape(1)
    k_uu = ops.ard_rbf_gram(z, None, gamma, alpha, beta, include_noise=False, include_jitter=True, jitter=1e-8)[0]
    k_s = ops.ard_rbf_gram(z, xt, gamma, alpha, beta)[0]                                      # [M, N*]
    w = None if weights is None else dv(weights).reshape(1, -1).contiguous()
    _, psi_2 = ops.qx_psi_stats_batched(z[None].contiguous(), mu, s, gamma, alpha, weights=w)
    diff = torch.linalg.inv(k_uu) - torch.linalg.inv(k_uu + beta * psi_2[0])
    return (alpha + 1.0 / beta - torch.sum(k_s * (diff @ k_s), dim=0)).cpu().numpy()


def test_bgplvm_zero_test_variance(dev):
    g = golden(BGPLVM)
    model = build_bgplvm(g, dev)
    _, xm, _ = points(g['x_mean'], N_T, 3)
    mean, var = model.predictive_marginals(xm, np.zeros_like(xm))
    want = gp_variance_at_points(dev, g['x_u'], g['x_mean'], softplus(g['x_var_raw']), softplus(g['gamma_raw']),
                                 softplus(g['alpha_raw']), softplus(g['beta_raw']), xm)
    print('zero test variance: max |err| %.3e of %.3e (bound 1e-9)' % (np.abs(var.cpu().numpy() - want[:, None]).max(), want.max()))
    close(var, np.repeat(want[:, None], var.shape[1], axis=1), 1e-9, 'variance of a GP at a point')


def test_bgplvm_trained_with_a_mask(dev):
    g = golden(BGPLVM)
    y = g['y']
    n, d = y.shape
    obs = mask(n, d, 17)
    model = build_masked(g, dev, obs, y=np.where(obs, y, np.nan))
    _, xm, xv = points(g['x_mean'], N_T, 3)
    want = want_of(('b', 'masked'), values_b(g), y, obs, xm, xv)
    mean, var = model.predictive_marginals(xm, xv)
    check('masked', mean, var, want)
    be = scalar(softplus(g['beta_raw']))
    base = (model.signal_variance.detach() + 1.0 / model.noise_precision.detach()).reshape(1)
    assert torch.equal(mean[:, 1], torch.zeros_like(mean[:, 1])) and torch.equal(var[:, 1], base.expand(N_T))
    with pytest.raises(NotImplementedError):
        model.predict_missing_data(y[:N_T, :2], x_test_mean=xm, x_test_var=xv, marginal_variance=True)
    # after fitting q(X*) to masked test rows: the moments at the fitted q(X*) are finite and positive
    obs_t = np.random.default_rng(11).random((N_T, d)) >= 0.3
    xf, sf = model.optimise_test_latents(np.where(obs_t, y[:N_T], np.nan), num_iterations=3, x_test_mean=xm, x_test_var=xv,
                                         observed=obs_t)
    mean_f, var_f = model.predictive_marginals(xf, sf)
    assert bool(torch.isfinite(mean_f).all()) and float(var_f.min()) > 1.0 / be
    # an all-True mask is the model trained on complete data
    full = build_masked(g, dev, np.ones((n, d), dtype=bool))
    plain = build_bgplvm(g, dev)
    have, ref = full.predictive_marginals(xm, xv), plain.predictive_marginals(xm, xv)
    close(have[0], ref[0].cpu().numpy(), 1e-9, 'all-True mask: mean')
    close(have[1], ref[1].cpu().numpy(), 1e-9, 'all-True mask: var')


# ------------------------------------------------------------------------------------------------------------------------ MRD
def test_mrd_moments_means_identity_and_marginal_variance(dev):
    g = golden(MRD)
    model = build_mrd(g, dev)
    nv, vo = int(g['num_views']), int(g['n_observed'])
    views = [g['view_%d' % v] for v in range(nv)]
    idx, xm, xv = points(g['x_mean'], N_T, 3)
    means, variances = model.predictive_marginals(xm, xv)
    assert len(means) == len(variances) == nv
    for v in range(nv):
        want = want_of(('mrd', v), values_view(g, v), views[v], np.ones(views[v].shape, dtype=bool), xm, xv)
        check('view %d' % v, means[v], variances[v], want)
    one = model.predictive_marginals(xm, xv, views=[nv - 1])
    assert len(one[0]) == 1 and torch.equal(one[0][0], means[nv - 1]) and torch.equal(one[1][0], variances[nv - 1])
    for tag, vt, pm, pv in (('fixture', [g['test_view_%d' % v] for v in range(vo)], g['x_test_mean'], g['x_test_var']),
                            ('7 points', [y[idx] for y in views[:vo]], xm, xv)):
        n_t = pm.shape[0]
        out = model.predict_missing_data(vt, x_test_mean=pm, x_test_var=pv)
        out_v = model.predict_missing_data(vt, x_test_mean=pm, x_test_var=pv, marginal_variance=True)
        m_, v_ = model.predictive_marginals(pm, pv, views=list(range(vo, nv)))
        for i, v in enumerate(range(vo, nv)):
            beta = scalar(softplus(g['beta_raw_%d' % v]))
            close(m_[i], out[3][i].cpu().numpy(), 1e-10, '%s view %d: mean against predicted_mean' % (tag, v))
            close(v_[i].sum(dim=0), (out[4][i][:, 0, 0] + (n_t - 1) / beta).cpu().numpy(), 1e-9, '%s view %d: sum of variances' % (tag, v))
            assert tuple(out[4][i].shape) == (views[v].shape[1], n_t, n_t)
            assert tuple(out_v[4][i].shape) == (n_t, views[v].shape[1]) and torch.equal(out_v[4][i], v_[i])
    out = model.predict_missing_data([g['test_view_%d' % v] for v in range(vo)], x_test_mean=g['x_test_mean'],
                                     x_test_var=g['x_test_var'])
    close(out[4][0], g['predicted_covar_0'], 1e-10, 'predicted covariance (default)')


def test_mrd_zero_test_variance(dev):
    g = golden(MRD)
    model = build_mrd(g, dev)
    _, xm, _ = points(g['x_mean'], N_T, 3)
    _, variances = model.predictive_marginals(xm, np.zeros_like(xm))
    for v in range(int(g['num_views'])):
        want = gp_variance_at_points(dev, g['x_u_%d' % v], g['x_mean'], softplus(g['x_var_raw']), softplus(g['gamma_raw_%d' % v]),
                                     softplus(g['alpha_raw_%d' % v]), softplus(g['beta_raw_%d' % v]), xm)
        close(variances[v], np.repeat(want[:, None], variances[v].shape[1], axis=1), 1e-9, 'view %d' % v)


def test_mrd_trained_with_masks(dev):
    g = golden(MRD)
    nv = int(g['num_views'])
    views = [g['view_%d' % v] for v in range(nv)]
    obs = [mask(*views[v].shape, 17 + v) for v in range(nv)]
    model = build_mrd_masked(g, dev, obs, views=[np.where(o, y, np.nan) for o, y in zip(obs, views)])
    _, xm, xv = points(g['x_mean'], N_T, 3)
    means, variances = model.predictive_marginals(xm, xv)
    for v in range(nv):
        want = want_of(('mrd', v, 'masked'), values_view(g, v), views[v], obs[v], xm, xv)
        check('masked view %d' % v, means[v], variances[v], want)
        base = (model.signal_variance[v].detach() + 1.0 / model.noise_precision[v].detach()).reshape(1)
        assert torch.equal(means[v][:, 1], torch.zeros_like(means[v][:, 1]))
        assert torch.equal(variances[v][:, 1], base.expand(N_T))
    with pytest.raises(NotImplementedError):
        model.predict_missing_data(views[:1], marginal_variance=True)
    full = build_mrd_masked(g, dev, [np.ones(y.shape, dtype=bool) for y in views])
    plain = build_mrd(g, dev)
    have, ref = full.predictive_marginals(xm, xv), plain.predictive_marginals(xm, xv)
    for v in range(nv):
        close(have[0][v], ref[0][v].cpu().numpy(), 1e-9, 'all-True masks: mean of view %d' % v)
        close(have[1][v], ref[1][v].cpu().numpy(), 1e-9, 'all-True masks: var of view %d' % v)


# --------------------------------------------------------------------------------------------------------------- cross-model
def test_over_t_with_one_atom_equals_the_masked_bgplvm(dev):
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm_t
    g = golden(BGPLVM)
    y = g['y']
    obs = mask(*y.shape, 17)
    iv = dict(x_mean=g['x_mean'], x_var=softplus(g['x_var_raw']), x_u=g['x_u'], gamma_atoms=softplus(g['gamma_raw']),
              alpha_atoms=softplus(g['alpha_raw']), beta_atoms=softplus(g['beta_raw']))
    over_t = dp_gp_lvm_t(np.where(obs, y, np.nan), num_latent_dims=g['x_mean'].shape[1], num_inducing_points=g['x_u'].shape[0],
                         truncation_level=1, device=dev, initial_values=iv, observed=obs)
    one = build_masked(g, dev, obs, y=np.where(obs, y, np.nan))
    _, xm, xv = points(g['x_mean'], N_T, 3)
    have, want = one.predictive_marginals(xm, xv), over_t.predictive_marginals(xm, xv)
    close(have[0], want[0].cpu().numpy(), 1e-9, 'mean')
    close(have[1], want[1].cpu().numpy(), 1e-9, 'var')


def over_d_one_hot(dev):
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
    g = dict(golden(OVER_D))
    d, t = g['dp_logits'].shape
    logits = np.full((d, t), -50.0)
    logits[np.arange(d), np.arange(d) % t] = 50.0
    g['dp_logits'] = logits
    return g, build_dp(dp_gp_lvm, g, dev, 'f64')


def test_over_d_with_one_hot_assignments_equals_over_t(dev):
    g, over_d = over_d_one_hot(dev)
    over_t, _ = build_t(g, dev, None)
    _, xm, xv = points(g['x_mean'], N_T, 3)
    have, want = over_d.predictive_marginals(xm, xv), over_t.predictive_marginals(xm, xv)
    print('over-D against over-T: max |err| mean %.3e, var %.3e' % (float((have[0] - want[0]).abs().max()), float((have[1] - want[1]).abs().max())))
    close(have[0], want[0].cpu().numpy(), 1e-9, 'mean')
    close(have[1], want[1].cpu().numpy(), 1e-9, 'var')
    some = [4, 0]
    part = over_d.predictive_marginals(xm, xv, columns=some)                   # (another K: another split of the pair tiles)
    close(part[0], have[0][:, some].cpu().numpy(), 1e-12, 'chosen columns: mean')
    close(part[1], have[1][:, some].cpu().numpy(), 1e-12, 'chosen columns: var')


def test_over_d_moments_means_and_marginal_variance(dev):
    """Every column under its own mixed kernel (the fixture's soft assignments): the restatement with that kernel as one atom."""
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
    g = golden(OVER_D)
    model = build_dp(dp_gp_lvm, g, dev, 'f64')
    y, do = g['y'], int(g['n_observed'])
    n, d = y.shape
    gam, al, be = (a.detach().cpu().numpy() for a in (model.ard_weights, model.signal_variance, model.noise_precision))
    xm = g['missing_x_test_mean']
    xv = np.random.default_rng(2).uniform(0.3, 1.0, xm.shape)
    mean, var = model.predictive_marginals(xm, xv)
    s = softplus(g['x_var_raw'])
    for col in range(d):
        v = one_atom(g['x_u'], gam[col], al.reshape(-1)[col], be.reshape(-1)[col], g['x_mean'], s, d)
        want = moments_numpy(v, y, np.ones((n, d), dtype=bool), xm, xv, [col])
        check('column %d' % col, mean[:, col:col + 1], var[:, col:col + 1], want)
    out = model.predict_missing_data(g['y_test'][:, :do], x_test_mean=xm, x_test_var=xv)
    out_v = model.predict_missing_data(g['y_test'][:, :do], x_test_mean=xm, x_test_var=xv, marginal_variance=True)
    close(mean[:, do:], out[3].cpu().numpy(), 1e-10, 'mean against predicted_mean')
    assert tuple(out[4].shape) == (d - do, xm.shape[0], xm.shape[0])
    var_u = model.predictive_marginals(xm, xv, columns=np.arange(do, d))[1]
    assert tuple(out_v[4].shape) == (xm.shape[0], d - do) and torch.equal(out_v[4], var_u)
    close(var_u, var[:, do:].cpu().numpy(), 1e-12, 'chosen columns: var')
    # the default output at the fixture's q(X*) (variances 1) is the reference's array
    out = model.predict_missing_data(g['y_test'][:, :do], x_test_mean=xm)
    np.testing.assert_allclose(out[4].cpu().numpy(), g['predicted_covar'], rtol=0, atol=1e-8 * np.abs(g['predicted_covar']).max())
