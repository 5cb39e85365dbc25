"""GPU tests of predictive_jacobian / latent_metric / magnification on bayesian_gp_lvm, MRD, dp_gp_lvm and dp_gp_lvm_t, each trained
on complete data and with a 30 % random mask (one column never observed), at N = 40, D = 12, M = 9, Q = 3, T = 3, N* = 7 after 20
optimise iterations.  The Jacobian is pinned to the existing frozen predictors' VJP at x_var = 0, the metric to a NumPy restatement
built column by column from the model's own marginals._Marginals pieces (recorded while the model builds them)."""
import functools
import os

import numpy as np
import pytest
import torch

from dp_gp_lvm_amd.models import frozen_bound_t, marginals
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm, dp_gp_lvm_t
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm, manifold_relevance_determination

pytestmark = pytest.mark.gpu
N, D, M, Q, T, N_T, D0 = 40, 12, 9, 3, 3, 7, 7
UNSEEN = 1                                                   # the column never observed by the masked models
MODELS = ['bgplvm', 'mrd', 'over_d', 'over_t']
CASES = [m + s for m in MODELS for s in ('', ' masked')]
DEV = 'cuda:0'


@functools.lru_cache(maxsize=None)
def data():
    rs = np.random.default_rng(11)
    t = rs.uniform(-2.0, 2.0, (N, 2))
    y = np.sin(t @ rs.standard_normal((2, D)) + rs.uniform(0, np.pi, D)) + 0.05 * rs.standard_normal((N, D))
    y = (y - y.mean(0)) / y.std(0)
    obs = rs.random((N, D)) >= 0.3
    obs[:, UNSEEN] = False
    return y, obs


@functools.lru_cache(maxsize=None)
def model_of(case, t=T):
    """The trained model of a case, once per process (the tests only read it)."""
    y, obs = data()
    masked = case.endswith('masked')
    kind = case.split()[0]
    torch.manual_seed(0)
    np.random.seed(0)
    yy = np.where(obs, y, np.nan) if masked else y
    kw = dict(num_latent_dims=Q, num_inducing_points=M, device=DEV)
    if kind == 'bgplvm':
        model = bayesian_gp_lvm(yy, precision='f64', **(dict(kw, observed=obs) if masked else kw))
    elif kind == 'mrd':
        views, ms = [yy[:, :D0], yy[:, D0:]], [obs[:, :D0], obs[:, D0:]]
        model = manifold_relevance_determination(views, precision='f64', **(dict(kw, observed=ms) if masked else kw))
    else:
        make = dp_gp_lvm if kind == 'over_d' else dp_gp_lvm_t
        model = make(yy, truncation_level=t, precision='f64', **(dict(kw, observed=obs) if masked else kw))
    model.optimise(20, learning_rate=0.05)
    return model


@functools.lru_cache(maxsize=None)
def points(case):
    """N* latent points near training latents (where the features are alive), as a device tensor."""
    xm = model_of(case).q_x[0].detach().cpu().numpy()
    rs = np.random.default_rng(5)
    return torch.as_tensor(xm[rs.permutation(N)[:N_T]] + 0.1 * rs.standard_normal((N_T, Q)), device=DEV)


def outputs(case, model, x, **kw):
    """(jacobian, metric, magnification) as lists over the model's kernels' outputs (views for MRD, one entry otherwise)."""
    out = model.predictive_jacobian(x, **kw), model.latent_metric(x, **kw), model.magnification(x, **kw)
    return out if case.startswith('mrd') else tuple([o] for o in out)


def predictors(case, model):
    return model.frozen_predictor() if case.startswith('mrd') else [model.frozen_predictor()]


# ---- the Jacobian against the frozen predictors' VJP at x_var = 0 ---------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_jacobian_is_the_predictors_vjp_at_zero_variance(case):
    model, x = model_of(case), points(case)
    jacs = outputs(case, model, x)[0]
    zero = torch.zeros_like(x)
    for jac, p in zip(jacs, predictors(case, model)):
        d = p.num_columns
        assert tuple(jac.shape) == (N_T, d, Q) and jac.dtype == torch.float64 and jac.is_cuda
        worst = 0.0
        for j in range(d):
            e = torch.zeros((N_T, d), dtype=torch.float64, device=DEV)
            e[:, j] = 1.0                                                # every row's own e_nj at once: mean[n, j] depends on x_n only
            d_mu, _ = p.vjp(x, zero, e, torch.zeros_like(e))
            worst = max(worst, float((jac[:, j, :] - d_mu).abs().max()))
        scale = max(1.0, float(jac.abs().max()))
        print('%s: max |jacobian - vjp| %.3e of %.3e' % (case, worst, float(jac.abs().max())))
        assert worst <= 1e-9 * scale
        assert float(jac.abs().max()) > 1e-3                             # (not a comparison of zeros)


# ---- the metric against a NumPy restatement from the model's own pieces ---------------------------------------------------------
def features(z, x, gamma, alpha):
    d = x[:, None, :] - z[None, :, :]                                    # [N*, M, Q]
    return -gamma * d * (alpha * np.exp(-0.5 * np.sum(gamma * d * d, axis=-1)))[..., None]


def restated(marg, x, cols=None, weights=None):
    """sum over the kernels and columns of w (m_d m_d^T + alpha diag(gamma) - b^T C_p(d) b), column by column."""
    num = lambda a: a.detach().cpu().numpy()
    z, gamma, alpha, c, r, gidx = (num(a) for a in (marg.z, marg.gamma, marg.alpha, marg.c, marg.r, marg.gidx))
    cols = range(r.shape[2]) if cols is None else cols
    g = np.zeros((x.shape[0], x.shape[1], x.shape[1]))
    for k in range(z.shape[0]):
        b = features(z[k], x, gamma[k], alpha[k])
        for d in cols:
            m = np.einsum('nmq,m->nq', b, r[k, :, d])
            cov = np.broadcast_to(alpha[k] * np.diag(gamma[k]), g.shape).copy()
            if gidx[k, d] >= 0:
                cov -= np.einsum('nmq,mp,npr->nqr', b, c[k, gidx[k, d]], b)
            else:
                assert np.all(r[k, :, d] == 0)
            g += (1.0 if weights is None else weights[k, d]) * (m[:, :, None] * m[:, None, :] + cov)
    return g


class Recorder:
    """Records the _Marginals (and the over-T model's _MomentsT) that a model builds inside one call."""

    def __init__(self, monkeypatch):
        self.marg, self.mom = [], []
        for cls, store in ((marginals._Marginals, self.marg), (frozen_bound_t._MomentsT, self.mom)):
            init = cls.__init__

            def wrapped(obj, *a, _init=init, _store=store, **kw):
                _init(obj, *a, **kw)
                _store.append(obj)
            monkeypatch.setattr(cls, '__init__', wrapped)


@pytest.mark.parametrize('case', CASES)
def test_metric_is_the_column_by_column_restatement(case, monkeypatch):
    model, x = model_of(case), points(case)
    rec = Recorder(monkeypatch)
    metrics = model.latent_metric(x)                                     # (one call: one training side per view is recorded)
    metrics = metrics if case.startswith('mrd') else [metrics]
    xn = x.cpu().numpy()
    kind, masked = case.split()[0], case.endswith('masked')
    if kind == 'mrd':
        want = [restated(m, xn) for m in rec.marg]
    elif kind == 'bgplvm':
        want = [restated(rec.marg[0], xn)]
    elif kind == 'over_t':
        want = [restated(rec.marg[0], xn, weights=rec.mom[0].phit.cpu().numpy())]
    else:
        want = restated(rec.marg[0], xn)                                 # K observed columns, one kernel each
        assert rec.marg[0].z.shape[0] == D - masked
        if masked:
            want = want + float(model.signal_variance[UNSEEN]) * np.diag(model.ard_weights[UNSEEN].detach().cpu().numpy())
        want = [want]
    assert len(want) == len(metrics)
    for g, w in zip(metrics, want):
        assert tuple(g.shape) == (N_T, Q, Q) and g.dtype == torch.float64 and g.is_cuda
        err, scale = np.max(np.abs(g.cpu().numpy() - w)), np.max(np.abs(w))
        print('%s: max |metric - restatement| %.3e of %.3e' % (case, err, scale))
        assert err <= 1e-9 * max(1.0, scale)


@pytest.mark.parametrize('case', CASES)
def test_metric_is_symmetric_positive_and_magnification_is_its_volume(case):
    model, x = model_of(case), points(case)
    _, metrics, mags = outputs(case, model, x)
    for g, mag in zip(metrics, mags):
        norm = torch.linalg.matrix_norm(g, ord=2)
        assert float((g - g.transpose(1, 2)).abs().max()) <= 1e-12 * max(1.0, float(norm.max()))
        low = torch.linalg.eigvalsh(0.5 * (g + g.transpose(1, 2)))[:, 0]
        assert bool(torch.all(low >= -1e-10 * norm)), (low, norm)
        want = torch.sqrt(torch.linalg.det(g))
        assert tuple(mag.shape) == (N_T,) and mag.dtype == torch.float64 and mag.is_cuda
        assert float(((mag - want).abs() / want).max()) <= 1e-10, (mag, want)


@pytest.mark.parametrize('case', [c for c in CASES if not c.startswith('mrd')])
def test_metrics_add_over_a_partition_of_the_columns(case):
    model, x = model_of(case), points(case)
    a, b = [0, 1, 5, 11], [2, 3, 4, 6, 7, 8, 9, 10]
    whole = model.latent_metric(x)
    parts = model.latent_metric(x, columns=a) + model.latent_metric(x, columns=b)
    assert float((parts - whole).abs().max()) <= 1e-11 * max(1.0, float(whole.abs().max()))
    assert torch.equal(model.latent_metric(x, columns=a + b), model.latent_metric(x, columns=np.array(a + b)))
    jac = model.predictive_jacobian(x)
    assert float((model.predictive_jacobian(x, columns=a) - jac[:, a]).abs().max()) <= 1e-11 * max(1.0, float(jac.abs().max()))
    assert float((model.predictive_jacobian(x.cpu().numpy(), columns=b) - jac[:, b]).abs().max()) <= 1e-11 * max(1.0, float(jac.abs().max()))
    with pytest.raises(AssertionError):
        model.latent_metric(x, columns=[D])
    with pytest.raises(AssertionError):
        model.predictive_jacobian(x[:, :2])


@pytest.mark.parametrize('case', ['mrd', 'mrd masked'])
def test_mrd_total_is_the_sum_of_the_views(case):
    model, x = model_of(case), points(case)
    views = model.latent_metric(x)
    total = model.latent_metric(x, total=True)
    assert len(views) == 2 and tuple(total.shape) == (N_T, Q, Q)
    assert float((views[0] + views[1] - total).abs().max()) <= 1e-11 * max(1.0, float(total.abs().max()))
    one = model.latent_metric(x, views=[1])
    assert len(one) == 1 and torch.equal(one[0], views[1])
    assert torch.equal(model.latent_metric(x, views=[1], total=True), views[1])
    assert torch.equal(model.magnification(x, views=[1])[0], model.magnification(x)[1])
    assert torch.equal(model.predictive_jacobian(x, views=[0])[0], model.predictive_jacobian(x)[0])
    with pytest.raises(AssertionError):
        model.latent_metric(x, views=[2])


@pytest.mark.parametrize('masked', [False, True], ids=['complete', 'masked'])
def test_over_t_with_one_atom_is_the_bayesian_gp_lvm(masked):
    y, obs = data()
    yy = np.where(obs, y, np.nan) if masked else y
    one = model_of('bgplvm' + (' masked' if masked else ''))
    x = points('bgplvm' + (' masked' if masked else ''))
    g, a, b = one.ard_weights, one.signal_variance, one.noise_precision
    num = lambda v: v.detach().cpu().numpy()
    iv = dict(x_mean=num(one.q_x[0]), x_var=num(torch.diagonal(one.q_x[1], dim1=-2, dim2=-1)), x_u=num(one.inducing_input),
              gamma_atoms=num(g).reshape(1, Q), alpha_atoms=num(a).reshape(1, 1), beta_atoms=num(b).reshape(1, 1))
    kw = dict(observed=obs) if masked else {}
    over_t = dp_gp_lvm_t(yy, num_latent_dims=Q, num_inducing_points=M, truncation_level=1, device=DEV, precision='f64',
                         initial_values=iv, **kw)
    for name in ('latent_metric', 'predictive_jacobian', 'magnification'):
        have, want = getattr(over_t, name)(x), getattr(one, name)(x)
        err = float((have - want).abs().max())
        print('T = 1 %s: max |diff| %.3e of %.3e' % (name, err, float(want.abs().max())))
        assert err <= 1e-9 * max(1.0, float(want.abs().max())), name


@pytest.mark.parametrize('case', [m + ' masked' for m in MODELS])
def test_a_never_observed_column_contributes_its_prior(case, monkeypatch):
    model, x = model_of(case), points(case)
    kw = dict(views=[0]) if case.startswith('mrd') else {}
    jac, metric, _ = outputs(case, model, x, **kw)
    rec = Recorder(monkeypatch)
    model.latent_metric(x, **kw)                                         # (the pieces of one call)
    assert float(jac[0][:, UNSEEN].abs().max()) == 0.0 and float(jac[0].abs().max()) > 0.0
    if case.startswith('mrd'):
        alone = restated(rec.marg[0], x.cpu().numpy(), cols=[UNSEEN])
        marg = rec.marg[0]
        prior = float(marg.alpha[0]) * np.diag(marg.gamma[0].cpu().numpy())
        assert np.max(np.abs(alone - prior)) == 0.0
        others = restated(marg, x.cpu().numpy(), cols=[d for d in range(D0) if d != UNSEEN])
        assert np.max(np.abs(metric[0].cpu().numpy() - others - prior)) <= 1e-9 * max(1.0, np.max(np.abs(others)))
        return
    alone = model.latent_metric(x, columns=[UNSEEN]).cpu().numpy()
    if case.startswith('over_d'):
        prior = float(model.signal_variance[UNSEEN]) * np.diag(model.ard_weights[UNSEEN].detach().cpu().numpy())
    elif case.startswith('over_t'):
        mom = rec.mom[0]
        w = (mom.phit[:, UNSEEN] * mom.aat).cpu().numpy()
        prior = np.diag(w @ mom.gat.cpu().numpy())
    else:
        marg = rec.marg[0]
        prior = float(marg.alpha[0]) * np.diag(marg.gamma[0].cpu().numpy())
    assert np.max(np.abs(alone - prior[None])) <= 1e-13 * np.max(prior)  # the same at every point: no data term
    assert np.all(np.diag(prior) > 0)
    assert float(model.predictive_jacobian(x, columns=[UNSEEN]).abs().max()) == 0.0
    mag = model.magnification(x, columns=[UNSEEN]).cpu().numpy()
    assert np.max(np.abs(mag - np.sqrt(np.prod(np.diag(prior))))) <= 1e-10 * np.sqrt(np.prod(np.diag(prior)))


def test_a_sharded_model_is_refused():
    import torch.distributed as dist
    y, _ = data()
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', str(29600 + os.getpid() % 1000))
    created = not dist.is_initialized()
    if created:
        dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        model = dp_gp_lvm(y, num_latent_dims=Q, num_inducing_points=M, truncation_level=T, device=DEV, precision='f64',
                          process_group=dist.group.WORLD)
        x = np.zeros((N_T, Q))
        for name in ('predictive_jacobian', 'latent_metric', 'magnification'):
            with pytest.raises(AssertionError, match='%s is not built for a model sharded over a process group' % name):
                getattr(model, name)(x)
    finally:
        if created:
            dist.destroy_process_group()
