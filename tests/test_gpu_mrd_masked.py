"""GPU tests of training manifold_relevance_determination on views with missing entries (observed=[...]): the masked model's
objective and raw gradients against the reference's MRD fixtures (all-True masks / None entries) and, for general masks,
against the committed fp64 oracle evaluated per view and per output dim on the rows at which that dim was observed; training
and imputation on synthetic two-view data; the test-point methods on a mask-trained model; argument checks and default
construction.  Tolerances: rtol 1e-10 for objectives and bounds, 1e-7 of each variable's largest entry for raw gradients, 1e-8
for q(X*) gradients, 1e-9 for the imputation (the project's fp64 tolerances, README)."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_gpu_predict_b1 import close
from test_gpu_predict_masked import masks_of
from test_gpu_train_masked import oracle_masked_fhat, softplus

pytestmark = pytest.mark.gpu
FIXTURES = ['mrd_ref_50_2views_12_3', 'mrd_ref_60_3views_15_4']
KINDS = ['random30', 'block', 'odd', 'rows']


def views_of(g):
    return [g['view_%d' % v] for v in range(int(g['num_views']))]


def build(g, dev, observed, views=None, prec=None):
    from dp_gp_lvm_amd.models.gaussian_process import manifold_relevance_determination
    nv = int(g['num_views'])
    views = views_of(g) if views is None else views
    iv = dict(x_mean=g['x_mean'], x_var=softplus(g['x_var_raw']), x_u=[g['x_u_%d' % i] for i in range(nv)],
              gamma=[softplus(g['gamma_raw_%d' % i]) for i in range(nv)], alpha=[softplus(g['alpha_raw_%d' % i]) for i in range(nv)],
              beta=[softplus(g['beta_raw_%d' % i]) for i in range(nv)])
    kw = {} if observed is None else dict(observed=observed)
    return manifold_relevance_determination(views, num_latent_dims=g['x_mean'].shape[1], num_inducing_points=g['x_u_0'].shape[0],
                                            device=dev, precision=prec, initial_values=iv, **kw)


def ref2raw(nv):
    names = dict(x_mean='x_mean', x_var_raw='x_var')
    for i in range(nv):
        names.update({'x_u_%d' % i: 'x_u_%d' % i, 'gamma_raw_%d' % i: 'gamma_atoms_%d' % i,
                      'alpha_raw_%d' % i: 'alpha_atoms_%d' % i, 'beta_raw_%d' % i: 'beta_atoms_%d' % i})
    return names


def masks(g, kind):
    views = views_of(g)
    n, nv = views[0].shape[0], len(views)
    if kind != 'rows':
        return [masks_of(n, y.shape[1], 23 + v)[kind] for v, y in enumerate(views)]
    out = []
    for v, y in enumerate(views):                            # a whole view absent for n // 3 rows; the last row in every view
        o = np.ones(y.shape, dtype=bool)
        start = (v * n) // (nv + 1)
        o[start:start + n // 3] = False
        o[-1] = False
        out.append(o)
    return out


def oracle_objective(g, obs):
    """-(sum_v sum_d f_hat of column d of view v on the rows R_d - KL over all rows + sum_v hyper-prior_v) at the fixture's raw
    variables, its raw gradients (by the fixture's names), sum f_hat and KL."""
    from oracle import dpgp_oracle_torch as ot
    nv = int(g['num_views'])
    names = list(ref2raw(nv))
    raw = {k: torch.tensor(np.asarray(g[k], dtype=np.float64), dtype=torch.float64, requires_grad=True) for k in names}
    mu, s = raw['x_mean'], ot._softplus(raw['x_var_raw'])
    f = torch.zeros((), dtype=torch.float64)
    hyper = torch.zeros((), dtype=torch.float64)
    for v in range(nv):
        gam, al, be = (ot._softplus(raw['%s_raw_%d' % (k, v)]) for k in ('gamma', 'alpha', 'beta'))
        yt = torch.as_tensor(np.where(obs[v], g['view_%d' % v], 0.0), dtype=torch.float64)
        f = f + oracle_masked_fhat(yt, obs[v], raw['x_u_%d' % v], mu, s, gam, al[:, 0], be[:, 0])
        hyper = hyper + sum(torch.sum(ot._log_normal_log_pdf(a)) for a in (gam, al, be))
    kl = 0.5 * (torch.sum(mu * mu) + torch.sum(s - torch.log(s)) - mu.shape[0] * mu.shape[1])
    obj = -(f - kl + hyper)
    grads = torch.autograd.grad(obj, [raw[k] for k in names])
    return float(obj.detach()), {k: v.numpy() for k, v in zip(names, grads)}, float(f.detach()), float(kl.detach())


_ORACLE = {}


def oracle_of(fixture, kind):
    """(masks, oracle_objective(...)) of a fixture and mask kind: computed once, shared by the tests, left unchanged."""
    if (fixture, kind) not in _ORACLE:
        g = golden(fixture)
        obs = masks(g, kind)
        _ORACLE[(fixture, kind)] = (obs, oracle_objective(g, obs))
    return _ORACLE[(fixture, kind)]


def check_gradients(got, want_of, nv):
    for ref_name, raw_name in ref2raw(nv).items():
        want = np.asarray(want_of(ref_name))
        have = got[raw_name].cpu().numpy().reshape(want.shape)
        scale = np.abs(want).max()
        print('%s: max |err| %.3e of %.3e' % (ref_name, np.abs(have - want).max(), scale))
        np.testing.assert_allclose(have, want, rtol=0, atol=1e-7 * scale, err_msg=ref_name)


@pytest.mark.parametrize('entries', ['all_true', 'none'])
@pytest.mark.parametrize('fixture', FIXTURES)
def test_all_true_masks_equal_the_reference(dev, fixture, entries):
    g = golden(fixture)
    views = views_of(g)
    obs = [np.ones(y.shape, dtype=bool) if entries == 'all_true' or v == 0 else None for v, y in enumerate(views)]
    model = build(g, dev, obs)
    print('objective %.15g (fixture %.15g)' % (float(model.objective), float(g['objective'])))
    np.testing.assert_allclose(float(model.objective), float(g['objective']), rtol=1e-10)
    assert tuple(model.objective_terms.shape) == (len(views), 5)
    plain = build(g, dev, None, prec='f64')
    assert list(model.raw_variables) == list(plain.raw_variables)
    for k, v in plain.raw_variables.items():
        assert model.raw_variables[k].shape == v.shape, k
    got = model.gradients()
    assert list(got) == list(plain.raw_variables)
    for k, v in got.items():
        assert v.shape == model.raw_variables[k].shape, k
    check_gradients(got, lambda name: g['grad_' + name], len(views))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('fixture', FIXTURES)
def test_general_masks_match_the_oracle(dev, fixture, kind):
    g = golden(fixture)
    obs, (want, grads, _, _) = oracle_of(fixture, kind)
    views = [np.where(o, y, np.nan) for o, y in zip(obs, views_of(g))]   # unobserved entries are NaN: they are ignored
    model = build(g, dev, obs, views=views)
    have = model.objective
    assert have.dim() == 0 and have.dtype == torch.float64 and have.is_cuda
    print('%s %s: objective %.15g (oracle %.15g)' % (fixture, kind, float(have), want))
    np.testing.assert_allclose(float(have), want, rtol=1e-10)
    slots = sum(len({o[:, d].tobytes() for d in range(o.shape[1]) if o[:, d].any()}) for o in obs)
    assert tuple(model.objective_terms.shape) == (slots, 5)
    check_gradients(model.gradients(), lambda name: grads[name], len(views))


def synthetic(seed):
    rs = np.random.default_rng(seed)
    t = np.sort(rs.uniform(-2.5, 2.5, 60))
    y0 = np.sin(1.3 * t[:, None] + np.pi * np.arange(8)[None, :] / 8.0) + 0.05 * rs.standard_normal((60, 8))
    y1 = np.cos(0.9 * t[:, None] + np.pi * np.arange(5)[None, :] / 5.0) + 0.05 * rs.standard_normal((60, 5))
    m0 = rs.random((60, 8)) >= 0.2
    m1 = np.ones((60, 5), dtype=bool)
    m1[rs.permutation(60)[:18]] = False
    return [y0, y1], [m0, m1]


@pytest.mark.parametrize('seed', [5, 6, 7])
def test_training_and_imputation(dev, seed):
    """x_mean: the PCA of the stacked column-mean-filled views, its columns standardised.  Reference figures (CPU oracle + torch
    Adam, the same formulation): the objective falls from about 850 to about 270; imputation RMSE 0.093 / 0.098 / 0.116 (view 0)
    and 0.178 / 0.197 / 0.247 (view 1) against 0.69 - 0.76 and 0.66 - 0.68 for column means."""
    from dp_gp_lvm_amd.models.gaussian_process import manifold_relevance_determination
    from dp_gp_lvm_amd.utils import missing
    from dp_gp_lvm_amd.utils.expressions import principal_component_analysis as pca
    from oracle import dpgp_oracle_torch as ot
    ys, ms = synthetic(seed)
    filled = [missing.column_mean_filled(y, m) for y, m in zip(ys, ms)]
    x0 = pca(np.hstack(filled), num_latent_dimensions=2)
    x0 = (x0 - x0.mean(axis=0)) / x0.std(axis=0)
    rs = np.random.default_rng(seed + 100)
    x_u = [x0[rs.permutation(60)[:10]] for _ in ys]
    model = manifold_relevance_determination(
        [np.where(m, y, np.nan) for y, m in zip(ys, ms)], num_latent_dims=2, num_inducing_points=10, device=dev, observed=ms,
        initial_values=dict(x_mean=x0, x_var=np.full((60, 2), 0.5), x_u=x_u, gamma=[np.ones((1, 2))] * 2, alpha=[1.0] * 2,
                            beta=[1.0] * 2))
    before = float(model.objective)
    model.optimise(300, learning_rate=0.05)
    after = float(model.objective)
    imputed = model.impute_training_data()
    assert isinstance(imputed, list) and len(imputed) == 2
    print('seed %d: objective %.6f -> %.6f' % (seed, before, after))
    assert np.isfinite(after) and after < before
    mu = model.q_x[0].detach().cpu()
    s = torch.diagonal(model.q_x[1], dim1=-2, dim2=-1).detach().cpu()
    for v, (y, mask) in enumerate(zip(ys, ms)):
        assert tuple(imputed[v].shape) == y.shape and imputed[v].dtype == torch.float64
        imp = imputed[v].cpu().numpy()
        np.testing.assert_array_equal(imp[mask], y[mask])
        rmse = np.sqrt(np.mean((imp[~mask] - y[~mask]) ** 2))
        rmse_mean = np.sqrt(np.mean((filled[v][~mask] - y[~mask]) ** 2))
        print('seed %d view %d: imputation RMSE %.4f, column means %.4f' % (seed, v, rmse, rmse_mean))
        assert rmse < 0.5 * rmse_mean
        # the posterior-mean formula per column, in NumPy fp64 at the model's final parameters
        z = model.inducing_input[v].detach().cpu()
        gam, al, be = (a[v].detach().cpu() for a in (model.ard_weights, model.signal_variance, model.noise_precision))
        _, _, v_all = ot.psi_pieces_t(torch.eye(60, dtype=torch.float64), z, mu, s, gam, al[:, 0])  # Psi1^T of every row [1,M,N]
        psi1 = v_all[0].numpy().T                                                                   # [N, M]
        want = np.where(mask, y, 0.0)
        for d in range(y.shape[1]):
            r = np.flatnonzero(mask[:, d])
            k_uu, p2, _ = ot.psi_pieces_t(torch.as_tensor(y[r, d:d + 1]), z, mu[r], s[r], gam, al[:, 0])
            a = k_uu[0].numpy() + float(be) * p2[0].numpy()
            col = float(be) * psi1 @ np.linalg.solve(a, psi1[r].T @ y[r, d])
            want[~mask[:, d], d] = col[~mask[:, d]]
        close(imputed[v], want, 1e-9, 'imputation of view %d' % v)


def test_test_points_on_a_mask_trained_model(dev):
    from oracle import dpgp_oracle as orc
    p = golden('predb1_mrd_60_4views_15_4')
    nv = int(p['num_views'])
    views, views_test = views_of(p), [p['test_view_%d' % v] for v in range(nv)]
    obs = [masks_of(60, y.shape[1], 23 + v)['random30'] for v, y in enumerate(views)]
    model = build(p, dev, obs, views=[np.where(o, y, np.nan) for o, y in zip(obs, views)])
    _, _, f_train, kl_train = oracle_objective(p, obs)
    xm, xv = p['x_test_mean'], p['x_test_var']
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    hyp = [tuple(t(softplus(p['%s_raw_%d' % (k, v)])) for k in ('gamma', 'alpha', 'beta')) for v in range(nv)]

    def f_star(obs_t, mu_t, s_t):
        return sum(oracle_masked_fhat(t(np.where(o, y, 0.0)), o, t(p['x_u_%d' % v]), mu_t, s_t, hyp[v][0], hyp[v][1][:, 0],
                                      hyp[v][2][:, 0]) for v, (o, y) in enumerate(zip(obs_t, views_test)))
    full = [np.ones(y.shape, dtype=bool) for y in views_test]
    f_test = float(f_star(full, t(xm), t(xv)))
    kl_t = orc.kl_qx(xm, xv)
    lb, mean, covar = model.predict_new_latent_variables(views_test, x_test_mean=xm, x_test_var=xv)
    print('bound %.15g (want %.15g)' % (float(lb), f_train + f_test - kl_train - kl_t))
    close(model.prediction_terms.sum(), f_test, 1e-10, 'f_hat*')
    close(lb, f_train + f_test - kl_train - kl_t, 1e-10, 'bound')
    close(mean, xm, 1e-15)
    # q(X*) gradients: every view observed, and the test points with their own masks
    for obs_t, kw in ((full, {}), ([masks_of(y.shape[0], y.shape[1], 29 + v)['random30'] for v, y in enumerate(views_test)], None)):
        mu_t, s_t = t(xm).requires_grad_(), t(xv).requires_grad_()
        d_mu, d_s = torch.autograd.grad(f_star(obs_t, mu_t, s_t), [mu_t, s_t])
        if kw is None:
            kw = dict(observed=obs_t)
            views_in = [np.where(o, y, np.nan) for o, y in zip(obs_t, views_test)]
        else:
            views_in = views_test
        g_mu, g_s = model.test_latent_gradients(views_in, xm, xv, **kw)
        close(g_mu, d_mu.numpy() - xm, 1e-8, 'd/dmean')
        close(g_s, d_s.numpy() - 0.5 * (1.0 - 1.0 / xv), 1e-8, 'd/dvar')
    np.random.seed(0)
    xm2, xv2 = model.optimise_test_latents(views_test[:2], 5, learning_rate=0.01)          # the default start
    assert tuple(xm2.shape) == xm.shape and bool(torch.isfinite(xm2).all()) and bool((xv2 > 0).all())
    xm3, xv3 = model.optimise_test_latents(views_in, 5, learning_rate=0.01, observed=kw['observed'])
    assert bool(torch.isfinite(xm3).all()) and bool((xv3 > 0).all())
    with pytest.raises(NotImplementedError, match='impute_training_data'):
        model.predict_missing_data(views_test[:2])
    with pytest.raises(NotImplementedError, match='impute_training_data'):
        model.predict_missing_data(views_in, observed=kw['observed'])


def test_argument_checks(dev):
    g = golden(FIXTURES[0])
    views = views_of(g)
    obs = masks(g, 'random30')
    build(g, dev, obs, prec='f64')                                          # fine
    with pytest.raises(AssertionError):
        build(g, dev, obs, prec='mixed')
    with pytest.raises(AssertionError):
        build(g, dev, [obs[0].astype(np.float64), obs[1]])                  # not boolean
    with pytest.raises(AssertionError):
        build(g, dev, obs[:1])                                              # wrong list length
    with pytest.raises(AssertionError):
        build(g, dev, [obs[0], obs[1][:-1]])                                # shape mismatch
    with pytest.raises(AssertionError):
        build(g, dev, [obs[0], np.zeros(views[1].shape, dtype=bool)])       # a view with nothing observed
    plain = build(g, dev, None)
    with pytest.raises(AssertionError):
        plain.impute_training_data()
    assert plain.objective_terms is None


def test_default_construction_with_masks(dev):
    from dp_gp_lvm_amd.models.gaussian_process import manifold_relevance_determination
    ys, ms = synthetic(5)
    np.random.seed(3)
    model = manifold_relevance_determination([np.where(m, y, np.nan) for y, m in zip(ys, ms)], num_latent_dims=2,
                                             num_inducing_points=10, device=dev, observed=ms)
    assert [tuple(z.shape) for z in model.inducing_input] == [(10, 2), (10, 2)] and tuple(model.q_x[0].shape) == (60, 2)
    np.testing.assert_allclose(torch.diagonal(model.q_x[1], dim1=-2, dim2=-1).cpu().numpy(), 1.0, rtol=1e-12)
    before = float(model.objective)
    model.optimise(20, learning_rate=0.01)
    assert float(model.objective) < before
