"""GPU tests of the test-time q(X*) surface that the four latent-variable models build on models/test_latents.py, on untrained
models at test_gpu_latent_metric.py's shapes (N = 40, D = 12, M = 9, Q = 3, T = 3, N* = 7): the public signatures, the fit pinned
through the public test_latent_gradients (sign, parametrisation and KL term), the seeded start, dp_gp_lvm's registered q(X*) and
prediction_terms of the two DP models."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dp_gp_lvm_amd.utils.types import get_prediction_variables
from test_gpu_latent_api import untrained
from test_gpu_latent_metric import D, D0, DEV, N_T, Q

pytestmark = pytest.mark.gpu

# str(inspect.signature(model.<name>)) of the commit before the fit was written once (859e6e5)
SIGNATURES = {
    'bgplvm': {
        'predict_new_latent_variables': '(y_test, use_pca=False, x_test_mean=None, x_test_var=None, reference_compat=False)',
        'predict_missing_data': '(y_test, use_pca=False, x_test_mean=None, x_test_var=None, reference_compat=False, observed=None, '
                                'marginal_variance=False)',
        'test_latent_gradients': '(y_test, x_test_mean, x_test_var, observed=None)',
        'optimise_test_latents': '(y_test, num_iterations=200, learning_rate=0.01, use_pca=False, x_test_mean=None, '
                                 'x_test_var=None, observed=None)',
    },
    'mrd': {
        'predict_new_latent_variables': '(views_test, use_pca=False, x_test_mean=None, x_test_var=None, reference_compat=False)',
        'predict_missing_data': '(views_test, use_pca=False, x_test_mean=None, x_test_var=None, reference_compat=False, '
                                'observed=None, marginal_variance=False)',
        'test_latent_gradients': '(views_test, x_test_mean, x_test_var, observed=None)',
        'optimise_test_latents': '(views_test, num_iterations=200, learning_rate=0.01, use_pca=False, x_test_mean=None, '
                                 'x_test_var=None, observed=None)',
    },
    'over_d': {
        'predict_new_latent_variables': '(y_test, use_pca=False, x_test_mean=None, x_test_var=None, reference_compat=False, '
                                        'observed=None)',
        'predict_missing_data': '(y_test, use_pca=False, x_test_mean=None, x_test_var=None, reference_compat=False, observed=None, '
                                "marginal_variance=False, form='slots')",
        'test_latent_gradients': "(y_test, x_test_mean, x_test_var, observed=None, form='slots')",
        'optimise_test_latents': '(y_test, num_iterations=200, learning_rate=0.01, use_pca=False, x_test_mean=None, '
                                 "x_test_var=None, observed=None, form='slots')",
    },
    'over_t': {
        'predict_new_latent_variables': '(y_test, use_pca=False, x_test_mean=None, x_test_var=None)',
        'predict_missing_data': '(y_test, use_pca=False, x_test_mean=None, x_test_var=None, observed=None)',
        'test_latent_gradients': '(y_test, x_test_mean, x_test_var, observed=None)',
        'optimise_test_latents': '(y_test, num_iterations=200, learning_rate=0.01, use_pca=False, x_test_mean=None, '
                                 'x_test_var=None, observed=None)',
    },
}
KINDS = list(SIGNATURES)
DO = 5                                                           # the observed first columns of the first-columns form
FORMS = [(kind, form) for kind in KINDS for form in ('first', 'observed')] + [('over_d', 'shared')]
LEARNING_RATE = 0.05


def new_rows():
    rs = np.random.default_rng(23)
    t = rs.uniform(-2.0, 2.0, (N_T, 2))
    y = np.sin(t @ rs.standard_normal((2, D)) + rs.uniform(0, np.pi, D)) + 0.05 * rs.standard_normal((N_T, D))
    obs = rs.random((N_T, D)) >= 0.3
    obs[:, 0] = True                                             # (every row and both views keep an observed entry)
    obs[:, D0] = True
    obs[0, 1] = False
    return y, obs


def arguments(kind, form):
    """(the positional test data, the keywords) of one argument form of test_latent_gradients / optimise_test_latents."""
    y, obs = new_rows()
    if kind == 'mrd':
        if form == 'first':
            return [y[:, :D0]], {}
        return [np.where(obs, y, np.nan)[:, :D0], np.where(obs, y, np.nan)[:, D0:]], dict(observed=[obs[:, :D0], obs[:, D0:]])
    if form == 'first':
        return y[:, :DO], {}
    kw = dict(observed=obs)
    return np.where(obs, y, np.nan), (dict(kw, form='shared') if form == 'shared' else kw)


def supplied_start(model):
    rs = np.random.default_rng(29)
    m0 = model.q_x[0].detach()[:N_T].to(torch.float64) + torch.as_tensor(0.1 * rs.standard_normal((N_T, Q)), device=DEV)
    return m0.contiguous(), torch.as_tensor(rs.uniform(0.5, 1.5, (N_T, Q)), device=DEV)


@pytest.mark.parametrize('kind', KINDS)
def test_signatures_are_those_of_the_models_own_copies(kind):
    model = untrained(kind)
    assert len(SIGNATURES[kind]) == 4
    for name, want in SIGNATURES[kind].items():
        method = getattr(model, name)
        assert str(inspect.signature(method)) == want, name
        assert (method.__doc__ or '').strip(), name


@pytest.mark.parametrize('kind,form', FORMS)
def test_fit_is_three_adam_steps_on_the_public_gradients(kind, form):
    model = untrained(kind)
    y_arg, kw = arguments(kind, form)
    m0, v0 = supplied_start(model)
    keep_m, keep_v = m0.clone(), v0.clone()
    got_m, got_v = model.optimise_test_latents(y_arg, num_iterations=3, learning_rate=LEARNING_RATE, x_test_mean=m0, x_test_var=v0,
                                               **kw)
    assert torch.equal(m0, keep_m) and torch.equal(v0, keep_v)                       # (the caller's tensors are not touched)
    if kind == 'over_d':
        assert got_m is get_prediction_variables()[-2]

    x, raw = keep_m.clone(), torch.log(torch.expm1(keep_v))
    opt = torch.optim.Adam([x, raw], lr=LEARNING_RATE)
    for _ in range(3):
        sv = F.softplus(raw)
        g_mu, g_s = model.test_latent_gradients(y_arg, x, sv, **kw)
        assert tuple(g_mu.shape) == tuple(g_s.shape) == (N_T, Q)
        x.grad, raw.grad = -g_mu, -g_s * torch.sigmoid(raw)
        opt.step()
    assert torch.equal(got_m, x) and torch.equal(got_v, F.softplus(raw))
    assert float((got_m - keep_m).abs().max()) > 1e-3 and float((got_v - keep_v).abs().max()) > 1e-3    # (the fit moved q(X*))
    assert bool(torch.isfinite(got_m).all()) and float(got_v.min()) > 0.0


@pytest.mark.parametrize('kind,form', FORMS)
def test_a_seeded_start_repeats(kind, form):
    model = untrained(kind)
    y_arg, kw = arguments(kind, form)
    out = []
    for _ in range(2):
        np.random.seed(17)
        out.append(model.optimise_test_latents(y_arg, num_iterations=2, learning_rate=LEARNING_RATE, **kw))
        if kind == 'over_d':
            assert out[-1][0] is get_prediction_variables()[-2]
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert tuple(out[0][0].shape) == tuple(out[0][1].shape) == (N_T, Q)
    np.random.seed(18)
    other = model.optimise_test_latents(y_arg, num_iterations=2, learning_rate=LEARNING_RATE, **kw)
    assert not torch.equal(other[0], out[0][0])                                       # (the start does draw its noise)


@pytest.mark.parametrize('kind,form', [('over_d', 'observed'), ('over_d', 'shared'), ('over_t', 'first'), ('over_t', 'observed')])
def test_prediction_terms_are_those_of_the_fit(kind, form):
    """The DP models assign prediction_terms after the loop (dp_gp_lvm's first-columns form evaluates no bound object and sets
    none): a call leaves a terms tensor of its own bound, not an earlier call's."""
    model = untrained(kind)
    y_arg, kw = arguments(kind, form)
    m0, v0 = supplied_start(model)
    model.optimise_test_latents(y_arg, num_iterations=1, x_test_mean=m0, x_test_var=v0, **kw)
    first = model.prediction_terms
    model.optimise_test_latents(y_arg, num_iterations=1, x_test_mean=m0, x_test_var=v0, **kw)
    second = model.prediction_terms
    assert first is not None and second is not None and second is not first
    assert second.dtype == torch.float64 and bool(torch.isfinite(second).all()) and torch.equal(first, second)
