"""GPU tests of training dp_gp_lvm (the over-D model) on data with missing entries (observed=...): the bound of
models/masked_bound_d.py on the weighted fp64 operators, against the reference's fixtures and the unmasked fp64 model (all-True
mask), the committed fp64 oracle evaluated per column on the rows at which that column was observed (general masks, odd shapes),
the masked bayesian_gp_lvm (T = 1), training + imputation on synthetic data, the predictive moments and the test-point bound of
a mask-trained model.  Tolerances: rtol 1e-10 for objectives at the fixtures (1e-7 at the odd shapes, as the unmasked test),
1e-7 of max(1, largest entry) for gradients, 1e-9 for moments (the fp64 tolerances of the README)."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_gpu_predict_b1 import close
from test_gpu_train_masked import synthetic

pytestmark = pytest.mark.gpu
FIXTURES = ['grad_ref_40_6_12_3_T4', 'grad_ref_60_10_15_4_T5']
REF2RAW = dict(x_mean='x_mean', x_var_raw='x_var', x_u='x_u', dp_logits='dp_logits', gamma_1_raw='dp_gamma_1',
               gamma_2_raw='dp_gamma_2', gamma_atoms_raw='gamma_atoms', alpha_atoms_raw='alpha_atoms', beta_atoms_raw='beta_atoms')
RAW_ORDER = ['x_mean', 'x_var', 'x_u', 'dp_logits', 'dp_gamma_1', 'dp_gamma_2', 'dp_w', 'gamma_atoms', 'alpha_atoms', 'beta_atoms']


def softplus(x):
    return np.logaddexp(0.0, x)


def masks(n, d):
    """rand30: 30 % missing at random.  edge: the same at another seed, then column 0 never observed, row 3 never observed and
    column 1 observed only in row 5."""
    rand30 = np.random.default_rng(0).random((n, d)) >= 0.3
    edge = np.random.default_rng(1).random((n, d)) >= 0.3
    edge[:, 0] = False
    edge[3, :] = False
    edge[:, 1] = False
    edge[5, 1] = True
    return dict(rand30=rand30, edge=edge)


def raw_of(g):
    from oracle import dpgp_oracle_torch as ot
    return {k: np.asarray(g[k], dtype=np.float64) for k in ot.NAMES}


def build(raw, y, dev, obs, s_1=1.0, s_2=1.0, mask_size=1, **kw):
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
    sp = softplus
    iv = dict(x_mean=raw['x_mean'], x_var=sp(raw['x_var_raw']), x_u=raw['x_u'], phi_logits=raw['dp_logits'],
              gamma_atoms=sp(raw['gamma_atoms_raw']), alpha_atoms=sp(raw['alpha_atoms_raw']), beta_atoms=sp(raw['beta_atoms_raw']),
              gamma_1=sp(raw['gamma_1_raw']), gamma_2=sp(raw['gamma_2_raw']), w_1=float(sp(raw['w_1_raw'])),
              w_2=float(sp(raw['w_2_raw'])))
    args = dict(num_latent_dims=raw['x_mean'].shape[1], num_inducing_points=raw['x_u'].shape[0],
                truncation_level=raw['dp_logits'].shape[1], alpha_prior_params=np.array([s_1, s_2]), mask_size=mask_size, device=dev,
                initial_values=iv)
    if obs is not None:
        args['observed'] = obs
    args.update(kw)
    return dp_gp_lvm(y, **args)


def build_fixture(g, dev, obs, y=None, **kw):
    return build(raw_of(g), g['y'] if y is None else y, dev, obs, float(g['s_1']), float(g['s_2']), **kw)


def oracle_masked_d(y, obs, raw_np, s_1=1.0, s_2=1.0, mask_size=1):
    """dp_objective - (sum_d f_hat of column d on its rows R_d - KL over all rows) - hyper-prior, composed as ot.objective, at the
    given raw variables; its gradients by autograd.  Returns (objective, {name: gradient}, f_hat, KL)."""
    from oracle import dpgp_oracle_torch as ot
    raw = {k: torch.tensor(np.asarray(v, dtype=np.float64), dtype=torch.float64, requires_grad=True) for k, v in raw_np.items()}
    yt = torch.as_tensor(np.where(obs, y, 0.0), dtype=torch.float64)
    mu, z, s = raw['x_mean'], raw['x_u'], ot._softplus(raw['x_var_raw'])
    phi = torch.softmax(raw['dp_logits'], dim=-1)
    if mask_size != 1:
        phi = torch.repeat_interleave(phi, int(mask_size), dim=0)
    g1, g2 = ot._softplus(raw['gamma_1_raw']).reshape(-1), ot._softplus(raw['gamma_2_raw']).reshape(-1)
    w1, w2 = ot._softplus(raw['w_1_raw']).reshape(()), ot._softplus(raw['w_2_raw']).reshape(())
    gat, aat, bat = (ot._softplus(raw[k]) for k in ('gamma_atoms_raw', 'alpha_atoms_raw', 'beta_atoms_raw'))
    gamma, alpha, beta = phi @ gat, (phi @ aat)[:, 0], (phi @ bat)[:, 0]
    f = torch.zeros((), dtype=torch.float64)
    for d in range(obs.shape[1]):
        r = np.flatnonzero(obs[:, d])
        if r.size:
            f = f + torch.sum(ot.fhat(yt[r, d:d + 1], z, mu[r], s[r], gamma[d:d + 1], alpha[d:d + 1], beta[d:d + 1]))
    kl = 0.5 * (torch.sum(mu * mu) + torch.sum(s - torch.log(s)) - mu.shape[0] * mu.shape[1])
    hyper = sum(torch.sum(ot._log_normal_log_pdf(a)) for a in (gat, aat, bat))
    dp = ot.dp_objective(phi, g1, g2, w1, w2, float(s_1), float(s_2))
    obj = dp - (f - kl) - hyper
    grads = torch.autograd.grad(obj, [raw[k] for k in ot.NAMES], allow_unused=True)
    grads = {k: (np.zeros(tuple(raw[k].shape)) if v is None else v.numpy()) for k, v in zip(ot.NAMES, grads)}
    return float(obj.detach()), grads, float(f.detach()), float(kl.detach())


ORACLE = {}


def oracle_of(fixture, kind):
    """The oracle's answer for (fixture, mask kind), computed once and shared."""
    if (fixture, kind) not in ORACLE:
        g = golden(fixture)
        obs = masks(*g['y'].shape)[kind]
        ORACLE[(fixture, kind)] = (obs,) + oracle_masked_d(g['y'], obs, raw_of(g), float(g['s_1']), float(g['s_2']))
    return ORACLE[(fixture, kind)]


def check_gradients(model, got, want_of, tol=1e-7):
    """The formula of test_gpu_grad.test_model_gradients_match_the_reference: eleven gradients, rtol = tol, atol = tol max(1, |want|)."""
    assert list(got) == RAW_ORDER
    for k, v in got.items():
        assert v.shape == model.raw[k].shape and v.dtype == torch.float64, k
    for ref_name, raw_name in REF2RAW.items():
        want = np.asarray(want_of(ref_name))
        if want.size == 0:
            continue
        have = got[raw_name].cpu().numpy().reshape(-1)[:want.size].reshape(want.shape)
        print('%s: max |err| %.3e of %.3e' % (ref_name, np.abs(have - want).max(), np.abs(want).max()))
        np.testing.assert_allclose(have, want, rtol=tol, atol=tol * max(1.0, np.abs(want).max()), err_msg=ref_name)
    np.testing.assert_allclose(got['dp_w'].cpu().numpy(), [float(want_of('w_1_raw')), float(want_of('w_2_raw'))], rtol=tol, atol=tol)


def assert_not_flagged(model):
    terms, info = model.per_dimension_terms
    assert not info.cpu().numpy().any(), 'no evaluation of these tests may fail a factorisation: info = %s' % info.unique().tolist()
    return terms


@pytest.mark.parametrize('fixture', FIXTURES)
def test_all_true_mask_equals_the_reference_and_the_unmasked_model(dev, fixture):
    g = golden(fixture)
    n, d = g['y'].shape
    model = build_fixture(g, dev, np.ones((n, d), dtype=bool))
    terms = model.objective_terms
    print('objective %.15g (fixture %.15g)' % (float(terms[0]), float(g['objective'])))
    assert tuple(terms.shape) == (5,)
    np.testing.assert_allclose(float(model.objective), float(g['objective']), rtol=1e-10)
    got = model.gradients()
    per_dim = assert_not_flagged(model)
    assert tuple(per_dim.shape) == (d, 5)
    check_gradients(model, got, lambda name: g['grad_' + name])
    plain = build_fixture(g, dev, None, precision='f64', backward_precision='f64')
    np.testing.assert_allclose(terms.cpu().numpy(), plain.objective_terms.cpu().numpy(), rtol=1e-10)
    want = plain.gradients()
    for k in RAW_ORDER:
        w = want[k].cpu().numpy()
        np.testing.assert_allclose(got[k].cpu().numpy(), w, rtol=1e-7, atol=1e-7 * max(1.0, np.abs(w).max()), err_msg=k)
    np.testing.assert_allclose(float(per_dim.sum()), float(plain.per_dimension_terms[0].sum()), rtol=1e-10)


@pytest.mark.parametrize('kind', ['rand30', 'edge'])
@pytest.mark.parametrize('fixture', FIXTURES)
def test_general_masks_match_the_oracle(dev, fixture, kind):
    g = golden(fixture)
    obs, want, grads, f, kl = oracle_of(fixture, kind)
    model = build_fixture(g, dev, obs, y=np.where(obs, g['y'], np.nan))          # unobserved entries are NaN: they are ignored
    have = model.objective
    assert have.dim() == 0 and have.dtype == torch.float64 and have.is_cuda
    terms = model.objective_terms.cpu().numpy()
    print('%s %s: objective %.15g (oracle %.15g)' % (fixture, kind, float(have), want))
    np.testing.assert_allclose(float(have), want, rtol=1e-10)
    np.testing.assert_allclose(terms[1:3], [f, kl], rtol=1e-10)
    got = model.gradients()
    per_dim = assert_not_flagged(model).cpu().numpy()
    never = ~obs.any(axis=0)
    assert per_dim.shape == (obs.shape[1], 5) and not per_dim[never].any() and np.abs(per_dim[~never]).sum(axis=1).all()
    np.testing.assert_allclose(per_dim.sum(), f, rtol=1e-10)
    check_gradients(model, got, lambda name: grads[name])


def test_evaluate_graph_is_the_eager_evaluation(dev):
    """With observed= nothing is captured into a HIP graph: evaluate_graph() is the eager evaluation (the same launches, so the
    same bits), and it sees an update of the raw variables."""
    g = golden(FIXTURES[0])
    obs, want, _, _, _ = oracle_of(FIXTURES[0], 'rand30')
    model = build_fixture(g, dev, obs)
    first = model.evaluate_graph().clone()
    assert tuple(first.shape) == (5,) and torch.equal(first, model.objective_terms)
    np.testing.assert_allclose(float(first[0]), want, rtol=1e-10)
    with torch.no_grad():
        model.raw['x_mean'].mul_(1.01)
    second = model.evaluate_graph().clone()
    assert torch.equal(second, model.objective_terms) and float(second[0]) != float(first[0])


@pytest.mark.parametrize('shape', [(33, 5, 17, 5, 1, 1), (70, 9, 33, 9, 3, 3), (160, 6, 140, 5, 3, 1)])
def test_odd_shapes_match_the_oracle(dev, shape):
    """test_gpu_grad.test_model_gradients_odd_shapes' recipe (M not a multiple of 16, Q not a multiple of 4, T = 1, mask_size > 1,
    M > 128: the 64-point blocks of the fp64 stage B) with 30 % of the entries missing."""
    n, d, m, q, t, mask = shape
    rng = np.random.default_rng(n + d)
    y = rng.standard_normal((n, d))
    y = (y - y.mean(0)) / y.std(0)
    raw = dict(x_mean=rng.standard_normal((n, q)), x_var_raw=0.3 * rng.standard_normal((n, q)),
               x_u=(4.0 if m > 128 else 1.0) * rng.standard_normal((m, q)), dp_logits=rng.standard_normal((d // mask, t)),
               gamma_1_raw=rng.standard_normal(max(t - 1, 0)), gamma_2_raw=rng.standard_normal(max(t - 1, 0)),
               w_1_raw=np.array(0.4), w_2_raw=np.array(0.7), gamma_atoms_raw=0.5 * rng.standard_normal((t, q)),
               alpha_atoms_raw=0.5 * rng.standard_normal((t, 1)), beta_atoms_raw=0.5 * rng.standard_normal((t, 1)) + 1.0)
    obs = np.random.default_rng(7).random((n, d)) >= 0.3
    want, grads, _, _ = oracle_masked_d(y, obs, raw, mask_size=mask)
    model = build(raw, np.where(obs, y, np.nan), dev, obs, mask_size=mask)
    print('%s: objective %.15g (oracle %.15g)' % (shape, float(model.objective), want))
    np.testing.assert_allclose(float(model.objective), want, rtol=1e-7)
    got = model.gradients()
    assert_not_flagged(model)
    check_gradients(model, got, lambda name: grads[name])


def test_one_atom_equals_the_masked_bayesian_gp_lvm(dev):
    from test_gpu_predict_masked import masks_of
    from test_gpu_train_masked import build_masked
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
    g = golden('bgplvm_ref_70_9_20_4')
    y = g['y']
    obs = masks_of(*y.shape, 23)['random30']
    y_nan = np.where(obs, y, np.nan)
    one = build_masked(g, dev, obs, y=y_nan)
    iv = dict(x_mean=g['x_mean'], x_var=softplus(g['x_var_raw']), x_u=g['x_u'], gamma_atoms=softplus(g['gamma_raw']),
              alpha_atoms=softplus(g['alpha_raw']), beta_atoms=softplus(g['beta_raw']))
    model = dp_gp_lvm(y_nan, num_latent_dims=g['x_mean'].shape[1], num_inducing_points=g['x_u'].shape[0], truncation_level=1,
                      device=dev, initial_values=iv, observed=obs)
    have = model.objective_terms.cpu().numpy()                               # (objective, f_hat, KL, DP objective, hyper-prior)
    float(one.objective)
    f = float(one.objective_terms.sum())                                     # (the masked B-GPLVM's [slots x 5] f_hat terms)
    print('f_hat %.15g (B-GPLVM %.15g)' % (have[1], f))
    np.testing.assert_allclose(have[1], f, rtol=1e-10)
    assert_not_flagged(model)


def restated_posterior_means(model, y, mask):
    """beta_d Psi1_d[n,:] (K_d + beta_d Psi2_d)^-1 Psi1_d^T y_d per column in NumPy fp64 at the model's parameters (Psi2_d and y_d
    over the rows at which d was observed); observed entries as given, a never-observed column 0."""
    from oracle import dpgp_oracle_torch as ot
    n, d = y.shape
    z, mu = model.inducing_input.detach().cpu(), model.q_x[0].detach().cpu()
    s = torch.diagonal(model.q_x[1], dim1=-2, dim2=-1).detach().cpu()
    gam, al, be = (a.detach().cpu() for a in (model.ard_weights, model.signal_variance, model.noise_precision))
    want = np.where(mask, y, 0.0)
    for j in range(d):
        r = np.flatnonzero(mask[:, j])
        if r.size == 0:
            continue
        _, _, psi1 = ot.psi_pieces(torch.eye(n, dtype=torch.float64), z, mu, s, gam[j:j + 1].expand(n, -1), al[j, 0].expand(n))
        psi1 = psi1.numpy()                                                                           # [N, M]: row i = Psi1_j[i, :]
        k_uu, p2, _ = ot.psi_pieces(torch.as_tensor(y[r, j:j + 1]), z, mu[r], s[r], gam[j:j + 1], al[j])
        b = float(be[j])
        col = b * psi1 @ np.linalg.solve(k_uu[0].numpy() + b * p2[0].numpy(), psi1[r].T @ y[r, j])
        want[~mask[:, j], j] = col[~mask[:, j]]
    return want


@pytest.mark.parametrize('seed', [5, 6, 7])
def test_training_and_imputation(dev, seed):
    """T = 3, Q = 2, M = 10, 300 Adam steps at 0.05 from the over-T test's start (x_mean: the standardised PCA of the
    column-mean-filled data; zero logits, unit atoms) with unit gamma_1, gamma_2 and w.  Reference figures (CPU oracle + torch
    Adam, the same formulation): imputation RMSE 0.116 / 0.132 / 0.118 against 0.713 / 0.745 / 0.722 for column means; the objective
    falls from about 516 to about 209."""
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
    from dp_gp_lvm_amd.utils import missing
    from dp_gp_lvm_amd.utils.expressions import principal_component_analysis as pca
    y, mask = synthetic(seed)
    n, d, t = y.shape[0], y.shape[1], 3
    filled = missing.column_mean_filled(y, mask)
    x0 = pca(filled, num_latent_dimensions=2)
    x0 = (x0 - x0.mean(axis=0)) / x0.std(axis=0)
    x_u = x0[np.random.default_rng(seed + 100).permutation(n)[:10]]
    model = dp_gp_lvm(np.where(mask, y, np.nan), num_latent_dims=2, num_inducing_points=10, truncation_level=t, device=dev,
                      observed=mask,
                      initial_values=dict(x_mean=x0, x_var=np.full((n, 2), 0.5), x_u=x_u, phi_logits=np.zeros((d, t)),
                                          gamma_atoms=np.ones((t, 2)), alpha_atoms=np.ones((t, 1)), beta_atoms=np.ones((t, 1)),
                                          gamma_1=np.ones(t - 1), gamma_2=np.ones(t - 1), w_1=1.0, w_2=1.0))
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
    close(imputed, restated_posterior_means(model, y, mask), 1e-9, 'imputation')


def trained_with_a_mask(dev, fixture=FIXTURES[1], kind='edge'):
    g = golden(fixture)
    obs = masks(*g['y'].shape)[kind]
    return g, obs, build_fixture(g, dev, obs, y=np.where(obs, g['y'], np.nan))


def test_imputation_variance_and_marginals_at_the_training_points_agree(dev):
    """impute_training_data(return_variance=True): the filled tensor of the plain call, the variance of predictive_marginals at the
    training q(X) at the unobserved entries and 0 at the observed ones; a never-observed column: mean 0, variance alpha_d + 1/beta_d."""
    g, obs, model = trained_with_a_mask(dev)
    filled, var = model.impute_training_data(return_variance=True)
    assert torch.equal(filled, model.impute_training_data())
    mu, cov = model.q_x
    mean_m, var_m = model.predictive_marginals(mu, torch.diagonal(cov, dim1=-2, dim2=-1))
    assert tuple(var.shape) == obs.shape == tuple(mean_m.shape)
    close(filled, np.where(obs, g['y'], mean_m.cpu().numpy()), 1e-9, 'filled against the marginal means')
    close(var, np.where(obs, 0.0, var_m.cpu().numpy()), 1e-9, 'variance against the marginal variances')
    close(filled, restated_posterior_means(model, np.where(obs, g['y'], 0.0), obs), 1e-9, 'filled against the restatement')
    al, be = model.signal_variance[0, 0], model.noise_precision[0, 0]
    assert not filled[:, 0].any() and torch.allclose(var[:, 0], (al + 1.0 / be).expand(obs.shape[0]), rtol=1e-14, atol=0)


def test_predictive_marginals_match_the_numpy_restatement(dev):
    """Every column is its own mixed kernel: the one-kernel restatement of test_gpu_predict_t.moments_numpy per column, a column never
    observed (0) and a column observed in one row (1) included; a subset of columns gives the same numbers."""
    from test_gpu_predict_t import moments_numpy
    from test_gpu_predictive_marginals import one_atom, points
    g, obs, model = trained_with_a_mask(dev)
    y0 = np.where(obs, g['y'], 0.0)
    n, d = y0.shape
    _, xm, xv = points(g['x_mean'], 7, 3)
    mean, var = model.predictive_marginals(xm, xv)
    assert tuple(mean.shape) == (7, d) == tuple(var.shape)
    z, mu = model.inducing_input.detach().cpu().numpy(), model.q_x[0].detach().cpu().numpy()
    s = torch.diagonal(model.q_x[1], dim1=-2, dim2=-1).detach().cpu().numpy()
    gam, al, be = (a.detach().cpu().numpy() for a in (model.ard_weights, model.signal_variance, model.noise_precision))
    want_mean, want_var = np.zeros((7, d)), np.zeros((7, d))
    for j in range(d):
        v = one_atom(z, gam[j], al[j], be[j], mu, s, d)
        m_j, v_j = moments_numpy(v, y0, obs, xm, xv, [j])
        want_mean[:, j], want_var[:, j] = m_j[:, 0], v_j[:, 0]
    for name, have, want in (('mean', mean, want_mean), ('var', var, want_var)):
        print('%s: max |err| %.3e of %.3e (bound 1e-9)' % (name, np.abs(have.cpu().numpy() - want).max(), np.abs(want).max()))
        close(have, want, 1e-9, name)
    assert not mean[:, 0].any() and np.allclose(var[:, 0].cpu().numpy(), al[0, 0] + 1.0 / be[0, 0], rtol=1e-14, atol=0)
    cols = [4, 0, 1]
    mean_c, var_c = model.predictive_marginals(xm, xv, columns=cols)
    close(mean_c, want_mean[:, cols], 1e-9, 'mean, columns')
    close(var_c, want_var[:, cols], 1e-9, 'var, columns')


def points_near_training(g, seed, n_t=6):
    rs = np.random.default_rng(seed)
    n, d = g['y'].shape
    rows = rs.permutation(n)[:n_t]
    y_t = g['y'][rows] + 0.05 * rs.standard_normal((n_t, d))
    o_t = rs.random((n_t, d)) >= 0.3
    o_t[:, 2] = False
    xm = g['x_mean'][rows] + 0.05 * rs.standard_normal((n_t, g['x_mean'].shape[1]))
    return y_t, o_t, xm, rs.uniform(0.3, 1.0, xm.shape)


def test_test_latent_gradients_do_not_see_the_training_data(dev):
    """The test bound holds the trained kernels and inducing inputs fixed and never reads y_train: on a mask-trained model its
    gradient equals, at 1e-12, that of an unmasked model built from the same parameter values."""
    g, obs, model = trained_with_a_mask(dev)
    plain = build_fixture(g, dev, None, precision='f64', backward_precision='f64')
    y_t, o_t, xm, xv = points_near_training(g, 11)
    got = model.test_latent_gradients(np.where(o_t, y_t, np.nan), xm, xv, observed=o_t)
    want = plain.test_latent_gradients(np.where(o_t, y_t, np.nan), xm, xv, observed=o_t)
    for name, a, b in zip(('d mean', 'd var'), got, want):
        assert tuple(a.shape) == xm.shape
        close(a, b.cpu().numpy(), 1e-12, name)


def test_optimise_test_latents_lowers_the_test_objective(dev):
    from dp_gp_lvm_amd import ops
    g, obs, model = trained_with_a_mask(dev)
    y_t, o_t, xm, xv = points_near_training(g, 12)
    y_nan = np.where(o_t, y_t, np.nan)

    def test_objective(xm_, xv_):
        """-(f_hat* - KL(q(X*))): its gradient is minus what test_latent_gradients returns."""
        model.test_latent_gradients(y_nan, xm_, xv_, observed=o_t)
        t = lambda a: torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a), dtype=torch.float64, device=dev)
        return -(float(model.prediction_terms.sum()) - float(ops.kl_qx(t(xm_), t(xv_))))
    before = test_objective(xm, xv)
    xm1, xv1 = model.optimise_test_latents(y_nan, num_iterations=10, learning_rate=0.01, x_test_mean=xm, x_test_var=xv, observed=o_t)
    after = test_objective(xm1, xv1)
    print('test objective %.6f -> %.6f' % (before, after))
    assert np.isfinite(after) and after < before
    # the default start: the training latent mean of the nearest training row over the jointly observed columns
    xm2, xv2 = model.optimise_test_latents(y_nan, num_iterations=1, observed=o_t)
    assert tuple(xm2.shape) == xm.shape and torch.isfinite(xm2).all() and torch.isfinite(xv2).all()


def test_argument_checks(dev):
    g = golden(FIXTURES[0])
    y = g['y']
    obs = masks(*y.shape)['rand30']
    model = build_fixture(g, dev, obs, precision='f64', backward_precision='f64')           # fine
    for kw in (dict(precision='mixed'), dict(precision='f32'), dict(backward_precision='mixed'), dict(backward_precision='mixed_fast'),
               dict(process_group=object())):
        with pytest.raises(AssertionError):
            build_fixture(g, dev, obs, **kw)
    with pytest.raises(AssertionError):
        build_fixture(g, dev, obs.astype(np.float64))                          # not boolean
    with pytest.raises(AssertionError):
        build_fixture(g, dev, obs[:-1])                                        # shape mismatch
    with pytest.raises(AssertionError):
        build_fixture(g, dev, np.zeros(y.shape, dtype=bool))                   # nothing observed
    with pytest.raises(NotImplementedError, match='not built for a model trained with observed='):
        model.predict_new_latent_variables(y[:3])
    with pytest.raises(NotImplementedError, match='not built for a model trained with observed='):
        model.predict_missing_data(y[:3, :4])
    with pytest.raises(AssertionError):
        build_fixture(g, dev, None).impute_training_data()
    from dp_gp_lvm_amd.utils import missing
    assert np.array_equal(missing.observed_mask(np.where(obs, y, np.nan)), obs)
    from dp_gp_lvm_amd.utils import types
    shapes = []
    for o in (obs, None):                                # get_training_variables: the same ten variables, in the same order
        types.reset_variable_collections()
        build_fixture(g, dev, o)
        shapes.append([tuple(v.shape) for v in types.get_training_variables()])
    assert len(shapes[0]) == 10 and shapes[0] == shapes[1]
