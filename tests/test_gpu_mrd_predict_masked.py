"""GPU tests of per-entry observation masks at test time for manifold_relevance_determination trained on complete views
(predict_missing_data / test_latent_gradients / optimise_test_latents with observed=[...]): masks that are the reference's
"first Vo views" case against its own fixtures; general masks against the committed fp64 oracle, evaluated per view (that
view's inducing inputs and kernel) and per output dim on the test points at which that dim was observed; all-True masks
against the unmasked gradient; the optimiser, a test point observed in no view, and the argument checks.  Tolerances: 1e-10
for bounds and predictive moments, 1e-8 for q(X*) gradients (those of test_gpu_predict_b1.py / test_gpu_predict_masked.py)."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_gpu_predict_b1 import MRD, build_mrd, close, softplus
from test_gpu_predict_masked import masks_of, oracle_masked

pytestmark = pytest.mark.gpu


def views_at_test(g):
    return [g['test_view_%d' % v] for v in range(int(g['num_views']))]


def oracle_views(g, views_test, obs, xm, xv):
    """sum over the views of oracle_masked with that view's Z and kernel: (f_hat*, d/dmu, d/ds)."""
    f, d_mu, d_s = 0.0, np.zeros_like(xm), np.zeros_like(xv)
    for v, (y, o) in enumerate(zip(views_test, obs)):
        dd = y.shape[1]
        rep = lambda a: np.repeat(softplus(a).reshape(1, -1), dd, axis=0)
        fv, mv, sv = oracle_masked(np.where(o, y, 0.0), o, g['x_u_%d' % v], xm, xv, rep(g['gamma_raw_%d' % v]),
                                   rep(g['alpha_raw_%d' % v])[:, 0], rep(g['beta_raw_%d' % v])[:, 0])
        f, d_mu, d_s = f + fv, d_mu + mv, d_s + sv
    return f, d_mu, d_s


@pytest.mark.parametrize('fixture', MRD)
def test_first_views_masks_reproduce_the_reference(dev, fixture):
    g = golden(fixture)
    model = build_mrd(g, dev)
    nv, vo = int(g['num_views']), int(g['n_observed'])
    views_test, xm, xv = views_at_test(g), g['x_test_mean'], g['x_test_var']
    obs = [np.full(y.shape, v < vo) for v, y in enumerate(views_test)]
    obs[0] = None                                                       # (None: the view is complete)
    views_in = [y if v < vo else np.full(y.shape, np.nan) for v, y in enumerate(views_test)]
    mlb, mean, covar, means, covars = model.predict_missing_data(views_in, x_test_mean=xm, x_test_var=xv, observed=obs)
    close(mlb, g['missing_lower_bound'], 1e-10, 'missing-data bound')
    close(mean, xm, 1e-15)
    close(torch.diagonal(covar, dim1=-2, dim2=-1), xv, 1e-15)
    assert model.missing_views == list(range(vo, nv)) and len(means) == len(covars) == nv - vo
    for i, v in enumerate(range(vo, nv)):
        np.testing.assert_array_equal(model.missing_columns[i], np.arange(views_test[v].shape[1]))
        close(means[i], g['predicted_mean_%d' % i], 1e-10, 'mean %d' % i)
        close(covars[i], g['predicted_covar_%d' % i], 1e-10, 'covariance %d' % i)
    assert tuple(model.prediction_terms.shape) == (vo, 5)
    g_mu, g_s = model.test_latent_gradients(views_in, xm, xv, observed=obs)
    close(g_mu, g['missing_grad_mean'], 1e-8, 'd/dmean')
    close(g_s, g['missing_grad_var'], 1e-8, 'd/dvar')
    # the existing interface is untouched and reports the same views and columns
    out = model.predict_missing_data(views_test[:vo], x_test_mean=xm, x_test_var=xv)
    close(out[0], g['missing_lower_bound'], 1e-10, 'missing-data bound (first Vo views)')
    assert model.missing_views == list(range(vo, nv))
    for a, b in zip(out[3], means):
        close(a, b.cpu().numpy(), 1e-12, 'means of the two interfaces')


@pytest.mark.parametrize('kind', ['random30', 'block', 'odd'])
@pytest.mark.parametrize('fixture', MRD)
def test_general_masks_match_the_oracle(dev, fixture, kind):
    from oracle import dpgp_oracle as orc
    g = golden(fixture)
    model = build_mrd(g, dev)
    views_test, xm, xv = views_at_test(g), g['x_test_mean'], g['x_test_var']
    n_t = xm.shape[0]
    obs = [masks_of(n_t, y.shape[1], 29 + v)[kind] for v, y in enumerate(views_test)]
    views_in = [np.where(o, y, np.nan) for o, y in zip(obs, views_test)]
    f_want, dmu_want, ds_want = oracle_views(g, views_test, obs, xm, xv)
    kl_t = orc.kl_qx(xm, xv)
    # the training side sum_v f_hat_v - KL(q(X)) from an unmasked call: bound = f_hat + f_hat*(full) - KL - KL*
    lb_full = float(model.predict_new_latent_variables(views_test, x_test_mean=xm, x_test_var=xv)[0])
    train = lb_full - float(model.prediction_terms.sum()) + kl_t
    lb, _, _, means, covars = model.predict_missing_data(views_in, x_test_mean=xm, x_test_var=xv, observed=obs)
    f_have = float(model.prediction_terms.sum())
    print('%s %s: f_hat* %.15g (oracle %.15g), bound %.15g (want %.15g)' % (fixture, kind, f_have, f_want, float(lb),
                                                                            train + f_want - kl_t))
    close(f_have, f_want, 1e-10, 'f_hat*')
    close(lb, train + f_want - kl_t, 1e-10, 'bound')
    slots = sum(len({o[:, d].tobytes() for d in range(o.shape[1]) if o[:, d].any()}) for o in obs)
    assert tuple(model.prediction_terms.shape) == (slots, 5)
    mv = [v for v, o in enumerate(obs) if not o.all()]
    assert model.missing_views == mv and len(means) == len(covars) == len(mv)
    for i, v in enumerate(mv):
        mc = np.flatnonzero(~obs[v].all(axis=0))
        np.testing.assert_array_equal(model.missing_columns[i], mc)
        assert tuple(means[i].shape) == (n_t, mc.size) and tuple(covars[i].shape) == (mc.size, n_t, n_t)
        assert bool(torch.isfinite(means[i]).all()) and bool(torch.isfinite(covars[i]).all())
    g_mu, g_s = model.test_latent_gradients(views_in, xm, xv, observed=obs)
    close(g_mu, dmu_want - xm, 1e-8, 'd/dmean')
    close(g_s, ds_want - 0.5 * (1.0 - 1.0 / xv), 1e-8, 'd/dvar')


def test_moments_of_a_column_mask_equal_the_view_interface(dev):
    """Views 2 and 3 absent except that view 2 keeps its first two columns: the moments of view 3 are those of the 'first Vo
    views' interface at the same q(X*) (they depend on the mask only through q(X*)), and view 2's are its remaining columns'."""
    g = golden(MRD[1])
    model = build_mrd(g, dev)
    views_test, xm, xv = views_at_test(g), g['x_test_mean'], g['x_test_var']
    obs = [None, None, np.zeros(views_test[2].shape, dtype=bool), np.zeros(views_test[3].shape, dtype=bool)]
    obs[2][:, :2] = True
    _, _, _, means, covars = model.predict_missing_data(views_test, x_test_mean=xm, x_test_var=xv, observed=obs)
    assert model.missing_views == [2, 3]
    np.testing.assert_array_equal(model.missing_columns[0], np.arange(2, views_test[2].shape[1]))
    close(means[0], g['predicted_mean_0'][:, 2:], 1e-10, 'view 2')
    close(covars[0], g['predicted_covar_0'][2:], 1e-10, 'view 2 covariance')
    close(means[1], g['predicted_mean_1'], 1e-10, 'view 3')
    close(covars[1], g['predicted_covar_1'], 1e-10, 'view 3 covariance')


def test_all_true_masks_give_the_unmasked_gradient(dev):
    g = golden(MRD[1])
    model = build_mrd(g, dev)
    views_test, xm, xv = views_at_test(g), g['x_test_mean'], g['x_test_var']
    want = model.test_latent_gradients(views_test, xm, xv)
    have = model.test_latent_gradients(views_test, xm, xv, observed=[np.ones(y.shape, dtype=bool) for y in views_test])
    close(have[0], want[0].cpu().numpy(), 1e-12, 'd/dmean')
    close(have[1], want[1].cpu().numpy(), 1e-12, 'd/dvar')
    have = model.test_latent_gradients(views_test, xm, xv, observed=[None] * len(views_test))
    close(have[0], want[0].cpu().numpy(), 1e-12, 'd/dmean (None entries)')


def test_optimise_test_latents_raises_the_masked_bound(dev):
    g = golden(MRD[1])
    model = build_mrd(g, dev)
    views_test, xm0, xv0 = views_at_test(g), g['x_test_mean'], g['x_test_var']
    obs = [np.random.default_rng(31 + v).random(y.shape) >= 0.3 for v, y in enumerate(views_test)]
    views_in = [np.where(o, y, np.nan) for o, y in zip(obs, views_test)]
    before = float(model.predict_missing_data(views_in, x_test_mean=xm0, x_test_var=xv0, observed=obs)[0])
    xm, xv = model.optimise_test_latents(views_in, 20, learning_rate=0.05, x_test_mean=xm0, x_test_var=xv0, observed=obs)
    after = float(model.predict_missing_data(views_in, x_test_mean=xm, x_test_var=xv, observed=obs)[0])
    print('masked bound before %.9g after %.9g' % (before, after))
    assert np.isfinite(after) and after > before, (before, after)


def test_a_row_observed_in_no_view(dev):
    """It starts at 0 (plus the N(0, 0.01^2) noise of every start) and its gradient is exactly the KL's."""
    g = golden(MRD[0])
    model = build_mrd(g, dev)
    rows = [3, 17, 5, 8]
    views_test = [g['view_%d' % v][rows] + 1e-3 for v in range(2)]
    obs = [np.random.default_rng(37 + v).random(y.shape) >= 0.3 for v, y in enumerate(views_test)]
    for o in obs:
        o[2] = False
    views_in = [np.where(o, y, np.nan) for o, y in zip(obs, views_test)]
    np.random.seed(0)
    lb, xm, _, _, _ = model.predict_missing_data(views_in, observed=obs)
    assert bool(torch.isfinite(lb))
    xm = xm.cpu().numpy()
    assert np.abs(xm[[0, 1, 3]] - g['x_mean'][[3, 17, 8]]).max() < 0.06 and np.abs(xm[2]).max() < 0.06
    xv = 0.5 + np.random.default_rng(0).random(xm.shape)
    g_mu, g_s = model.test_latent_gradients(views_in, xm, xv, observed=obs)
    np.testing.assert_array_equal(g_mu[2].cpu().numpy(), -xm[2])
    np.testing.assert_array_equal(g_s[2].cpu().numpy(), -(0.5 * (1.0 - 1.0 / xv[2])))
    assert bool((g_mu[[0, 1, 3]].cpu() != torch.as_tensor(-xm[[0, 1, 3]])).any())


def test_argument_checks(dev):
    g = golden(MRD[1])
    model = build_mrd(g, dev)
    views_test, xm, xv = views_at_test(g), g['x_test_mean'], g['x_test_var']
    obs = [np.random.default_rng(41 + v).random(y.shape) >= 0.3 for v, y in enumerate(views_test)]
    kw = dict(x_test_mean=xm, x_test_var=xv)
    model.predict_missing_data(views_test, observed=obs, **kw)                                        # fine
    with pytest.raises(AssertionError):
        model.predict_missing_data(views_test, observed=obs[:-1], **kw)                               # list length
    with pytest.raises(AssertionError):
        model.predict_missing_data(views_test[:-1], observed=obs, **kw)                               # all V views are needed
    with pytest.raises(AssertionError):
        model.predict_missing_data(views_test, observed=[obs[0].astype(np.float64)] + obs[1:], **kw)  # not boolean
    with pytest.raises(AssertionError):
        model.predict_missing_data(views_test, observed=[obs[0][:-1]] + obs[1:], **kw)                # shape mismatch
    with pytest.raises(AssertionError):
        model.predict_missing_data(views_test, observed=[np.ones(y.shape, dtype=bool) for y in views_test], **kw)
    with pytest.raises(AssertionError):
        model.predict_missing_data(views_test, observed=[None] * len(views_test), **kw)               # nothing missing
    with pytest.raises(AssertionError):
        model.predict_missing_data(views_test, observed=[np.zeros(y.shape, dtype=bool) for y in views_test], **kw)
    with pytest.raises(AssertionError):
        model.predict_missing_data(views_test, observed=obs, reference_compat=True, **kw)
    with pytest.raises(AssertionError):
        model.test_latent_gradients(views_test, xm, xv, observed=[o.astype(np.int64) for o in obs])
    with pytest.raises(AssertionError):
        model.optimise_test_latents(views_test, 1, observed=obs[1:], **kw)
    # observed=None: the existing paths and their assertions
    with pytest.raises(AssertionError):
        model.predict_missing_data(views_test, **kw)                                                  # Vo = V
    out = model.predict_missing_data(views_test[:2], **kw)
    assert len(out[3]) == 2 and model.missing_views == [2, 3]
