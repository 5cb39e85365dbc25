"""GPU tests of predictive_covariance / sample_functions on bayesian_gp_lvm, MRD, dp_gp_lvm and dp_gp_lvm_t, each trained on complete
data and with a 30 % random mask (one column never observed), at N = 40, D = 8, M = 12, Q = 3, T = 3, N* = 7 after 20 optimise
iterations.  The covariance is pinned on its diagonal to predictive_marginals (an already pinned quantity) and as a whole to a NumPy
restatement built column by column from the model's own marginals._Marginals pieces (recorded while the model builds them); the
samples are pinned through their factors (unit-vector draws), their affinity in the draws and the moments of their whitened
residuals."""
import functools
import os

import numpy as np
import pytest
import torch

from dp_gp_lvm_amd.models import frozen_bound_t, marginals
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm, dp_gp_lvm_t
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm, manifold_relevance_determination

pytestmark = pytest.mark.gpu
N, D, M, Q, T, N_T, D0 = 40, 8, 12, 3, 3, 7, 5
UNSEEN = 1                                                   # the column never observed by the masked models
MODELS = ['bgplvm', 'mrd', 'over_d', 'over_t']
CASES = [m + s for m in MODELS for s in ('', ' masked')]
DEV = 'cuda:0'
JITTER = 1e-6
TOL = 1e-9


@functools.lru_cache(maxsize=None)
def data():
    rs = np.random.default_rng(23)
    t = rs.uniform(-2.0, 2.0, (N, 2))
    y = np.sin(t @ rs.standard_normal((2, D)) + rs.uniform(0, np.pi, D)) + 0.05 * rs.standard_normal((N, D))
    y = (y - y.mean(0)) / y.std(0)
    obs = rs.random((N, D)) >= 0.3
    obs[:, UNSEEN] = False
    return y, obs


@functools.lru_cache(maxsize=None)
def model_of(case):
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
        model = make(yy, truncation_level=T, precision='f64', **(dict(kw, observed=obs) if masked else kw))
    model.optimise(20, learning_rate=0.05)
    return model


@functools.lru_cache(maxsize=None)
def points(case):
    """N* latent points near training latents (where the features are alive), as a device tensor."""
    xm = model_of(case).q_x[0].detach().cpu().numpy()
    rs = np.random.default_rng(5)
    return torch.as_tensor(xm[rs.permutation(N)[:N_T]] + 0.1 * rs.standard_normal((N_T, Q)), device=DEV)


def listed(case, out):
    """A result as a list over the model's outputs (views for MRD, one entry otherwise)."""
    return list(out) if case.startswith('mrd') else [out]


# ---- the NumPy restatement from the model's own pieces ---------------------------------------------------------------------------
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


def kernel_pieces(marg, x, k, col):
    """(cov [N*, N*], mean [N*], alpha, beta) of column `col` under kernel k of a recorded _Marginals, in NumPy."""
    num = lambda a: a.detach().cpu().numpy()
    z, gamma, alpha, beta, c, r, gidx = (num(a) for a in (marg.z, marg.gamma, marg.alpha, marg.beta, marg.c, marg.r, marg.gidx))
    d = x[:, None, :] - z[k][None, :, :]
    kv = alpha[k] * np.exp(-0.5 * np.sum(gamma[k] * d * d, axis=-1))                      # [N*, M]
    dx = x[:, None, :] - x[None, :, :]
    cov = alpha[k] * np.exp(-0.5 * np.sum(gamma[k] * dx * dx, axis=-1))
    if gidx[k, col] >= 0:
        cov = cov - kv @ c[k, gidx[k, col]] @ kv.T
    else:
        assert np.all(r[k, :, col] == 0)
    return cov, kv @ r[k, :, col], float(alpha[k]), float(beta.reshape(-1)[k])


def restated(case, model, x, monkeypatch, columns=None):
    """Per output of the model (views for MRD) the column-by-column pieces: dict(cov [J, N*, N*], mean [N*, J], alpha [J], beta [J])
    of the single-kernel models; for over_t the per-atom arrays cov [T, J, ..], mean [T, N*, J], alpha [T], beta [T] and phi [T, J]."""
    rec = Recorder(monkeypatch)
    kind = case.split()[0]
    kw = {} if columns is None else dict(columns=columns)
    model.predictive_covariance(x, **kw)                                 # (one call: the training side is recorded)
    monkeypatch.undo()
    xn = x.cpu().numpy()
    stack = lambda ps: dict(cov=np.stack([p[0] for p in ps]), mean=np.stack([p[1] for p in ps], axis=1),
                            alpha=np.array([p[2] for p in ps]), beta=np.array([p[3] for p in ps]))
    if kind == 'over_d':
        marg = rec.marg[-1]                                              # K = J kernels with one column each
        return [stack([kernel_pieces(marg, xn, k, 0) for k in range(marg.z.shape[0])])]
    if kind == 'over_t':
        marg, cols = rec.marg[-1], (range(D) if columns is None else columns)
        per = [stack([kernel_pieces(marg, xn, t, c) for c in cols]) for t in range(T)]
        phi = rec.mom[-1].phit.cpu().numpy()[:, list(cols)]
        return [dict(cov=np.stack([p['cov'] for p in per]), mean=np.stack([p['mean'] for p in per]),
                     alpha=np.array([p['alpha'][0] for p in per]), beta=np.array([p['beta'][0] for p in per]), phi=phi)]
    margs = rec.marg if kind == 'mrd' else rec.marg[:1]
    out = []
    for v, marg in enumerate(margs):
        cols = range(marg.r.shape[2]) if columns is None else (columns[v] if kind == 'mrd' else columns)
        out.append(stack([kernel_pieces(marg, xn, 0, c) for c in cols]))
    return out


def mixture(p, noise):
    """(covariance [J, N*, N*], mean [N*, J]) of the over-T mixture from its per-atom pieces."""
    eye = np.eye(p['cov'].shape[-1])
    cov_t = p['cov'] + (1.0 / p['beta'])[:, None, None, None] * eye if noise else p['cov']
    m_t = p['mean'].transpose(0, 2, 1)                                   # [T, J, N*]
    mean = np.sum(p['phi'][:, :, None] * m_t, axis=0)
    second = cov_t + m_t[:, :, :, None] * m_t[:, :, None, :]
    return np.sum(p['phi'][:, :, None, None] * second, axis=0) - mean[:, :, None] * mean[:, None, :], mean.T


def close(got, want, tol=TOL):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    err, scale = float(np.max(np.abs(got - want))), max(1.0, float(np.max(np.abs(want))))
    return err <= tol * scale, err, scale


# ---- predictive_covariance -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_diagonal_plus_noise_is_the_marginal_variance(case):
    model, x = model_of(case), points(case)
    covs = listed(case, model.predictive_covariance(x))
    noisy = listed(case, model.predictive_covariance(x, noise=True))
    _, variances = model.predictive_marginals(x, torch.zeros_like(x))
    for cov, cn, var in zip(covs, noisy, listed(case, variances)):
        j = var.shape[1]
        assert tuple(cov.shape) == (j, N_T, N_T) and cov.dtype == torch.float64 and cov.is_cuda
        assert torch.equal(cov, cov.transpose(1, 2)) and torch.equal(cn, cn.transpose(1, 2))
        ok, err, scale = close(torch.diagonal(cn, dim1=1, dim2=2).transpose(0, 1), var.cpu().numpy())
        print('%s: max |diag(cov) + 1/beta - var| %.3e of %.3e' % (case, err, scale))
        assert ok
        off = ~torch.eye(N_T, dtype=torch.bool, device=DEV)
        assert torch.equal(cn[:, off], cov[:, off])                      # the noise enters on the diagonal only
        assert float(cov.abs().max()) > 1e-3 and float(cov[:, off].abs().max()) > 1e-4          # (not a comparison of zeros)


@pytest.mark.parametrize('case', CASES)
def test_covariance_is_the_column_by_column_restatement(case, monkeypatch):
    model, x = model_of(case), points(case)
    pieces = restated(case, model, x, monkeypatch)
    for noise in (False, True):
        covs = listed(case, model.predictive_covariance(x, noise=noise))
        assert len(covs) == len(pieces)
        for cov, p in zip(covs, pieces):
            if case.startswith('over_t'):
                want, _ = mixture(p, noise)
            else:
                want = p['cov'] + (1.0 / p['beta'])[:, None, None] * np.eye(N_T) if noise else p['cov']
            ok, err, scale = close(cov, want)
            print('%s noise=%s: max |cov - restatement| %.3e of %.3e' % (case, noise, err, scale))
            assert ok
    if case.endswith('masked') and not case.startswith('over_t'):       # the column never observed: its prior gram
        p = pieces[0]
        xn = x.cpu().numpy()
        dx = xn[:, None, :] - xn[None, :, :]
        gamma = (model.ard_weights[UNSEEN] if case.startswith('over_d') else None)
        assert np.all(p['mean'][:, UNSEEN] == 0)
        assert abs(p['cov'][UNSEEN][0, 0] - p['alpha'][UNSEEN]) <= 1e-12 * p['alpha'][UNSEEN]
        if gamma is not None:
            g = gamma.detach().cpu().numpy()
            assert close(p['cov'][UNSEEN], p['alpha'][UNSEEN] * np.exp(-0.5 * np.sum(g * dx * dx, axis=-1)), 1e-12)[0]


@pytest.mark.parametrize('case', CASES)
def test_noise_adds_one_over_beta_on_the_diagonal(case, monkeypatch):
    model, x = model_of(case), points(case)
    pieces = restated(case, model, x, monkeypatch)
    covs, noisy = listed(case, model.predictive_covariance(x)), listed(case, model.predictive_covariance(x, noise=True))
    for cov, cn, p in zip(covs, noisy, pieces):
        inv = np.sum(p['phi'] / p['beta'][:, None], axis=0) if case.startswith('over_t') else 1.0 / p['beta']     # [J]
        diff = torch.diagonal(cn - cov, dim1=1, dim2=2).cpu().numpy()
        assert np.max(np.abs(diff - inv[:, None]) / inv[:, None]) <= 1e-10
        assert np.min(inv) > 0


@pytest.mark.parametrize('case', CASES)
def test_columns_and_views_select_what_they_say(case):
    model, x = model_of(case), points(case)
    if case.startswith('mrd'):
        whole = model.predictive_covariance(x)
        assert len(whole) == 2 and [w.shape[0] for w in whole] == [D0, D - D0]
        only = model.predictive_covariance(x, views=[1])
        assert len(only) == 1 and torch.equal(only[0], whole[1])
        pick = model.predictive_covariance(x, views=[1, 0], columns=[[2, 0], [4]])
        assert torch.equal(pick[0], whole[1][[2, 0]]) and torch.equal(pick[1], whole[0][[4]])
        s_whole = model.sample_functions(x, num_samples=3, seed=4)
        s_pick = model.sample_functions(x, num_samples=3, seed=4, views=[0])
        assert len(s_whole) == 2 and tuple(s_whole[1].shape) == (3, N_T, D - D0) and torch.equal(s_pick[0], s_whole[0])
        with pytest.raises(AssertionError):
            model.predictive_covariance(x, views=[2])
        return
    whole = model.predictive_covariance(x)
    a = [5, 0, UNSEEN, 5]
    part = model.predictive_covariance(x, columns=a)
    tol = 0.0 if case.startswith('bgplvm') else 1e-12                    # (over_d / over_t: the training side is formed for the chosen columns)
    assert float((part - whole[a]).abs().max()) <= tol * max(1.0, float(whole.abs().max()))
    assert torch.equal(model.predictive_covariance(x.cpu().numpy(), columns=np.array(a)), part)
    draws = np.random.default_rng(3).standard_normal((2, N_T, D))
    f = model.sample_functions(x, draws=draws, **({'atoms': np.zeros((2, D), dtype=np.int64)} if case.startswith('over_t') else {}))
    fa = model.sample_functions(x, draws=draws[:, :, a], columns=a,
                                **({'atoms': np.zeros((2, len(a)), dtype=np.int64)} if case.startswith('over_t') else {}))
    assert tuple(f.shape) == (2, N_T, D) and float((fa - f[:, :, a]).abs().max()) <= 1e-12 * max(1.0, float(f.abs().max()))
    with pytest.raises(AssertionError):
        model.predictive_covariance(x, columns=[D])
    with pytest.raises(AssertionError):
        model.sample_functions(x[:, :2])


# ---- sample_functions ------------------------------------------------------------------------------------------------------------
def unit_draws(j):
    return np.broadcast_to(np.eye(N_T)[:, :, None], (N_T, N_T, j)).copy()                  # draws[s, :, col] = e_s


@pytest.mark.parametrize('case', [c for c in CASES if not c.startswith('over_t')])
def test_unit_vector_draws_give_the_factor(case, monkeypatch):
    """sample - mean with draws = the N* unit vectors is L; L L^T against cov + jitter alpha I is a backward-error check of the
    factorisation: conditioning does not enter."""
    model, x = model_of(case), points(case)
    pieces = restated(case, model, x, monkeypatch)
    draws = [unit_draws(p['cov'].shape[0]) for p in pieces]
    out = model.sample_functions(x, draws=draws if case.startswith('mrd') else draws[0])
    for f, p in zip(listed(case, out), pieces):
        assert tuple(f.shape) == (N_T, N_T, p['cov'].shape[0]) and f.dtype == torch.float64 and f.is_cuda
        dev = f.cpu().numpy() - p['mean'][None]
        for col in range(p['cov'].shape[0]):
            l = dev[:, :, col].T                                         # l[n, s]
            assert np.max(np.abs(np.triu(l, 1))) <= 1e-9 * np.max(np.abs(l))
            want = p['cov'][col] + JITTER * p['alpha'][col] * np.eye(N_T)
            assert np.max(np.abs(l @ l.T - want)) <= TOL * np.max(np.abs(p['cov'][col])), (case, col)


@pytest.mark.parametrize('case', ['over_t', 'over_t masked'])
def test_given_atoms_give_the_per_atom_restatement(case, monkeypatch):
    model, x = model_of(case), points(case)
    p = restated(case, model, x, monkeypatch)[0]
    atoms = (np.arange(N_T)[:, None] + np.arange(D)[None, :]) % T          # every atom at every column
    f = model.sample_functions(x, draws=unit_draws(D), atoms=atoms).cpu().numpy()
    for t in range(T):
        for col in range(D):
            rows = np.flatnonzero(atoms[:, col] == t)
            dev = f[rows, :, col] - p['mean'][t][:, col][None]            # columns `rows` of L_t,col, transposed
            want = p['cov'][t, col] + JITTER * p['alpha'][t] * np.eye(N_T)
            l = np.linalg.cholesky(want)                                 # forward error: cond(want) eps <= 1e6 x 2e-16, times 500
            assert np.max(np.abs(dev.T - l[:, rows])) <= 1e-7 * np.max(np.abs(l)), (t, col)
    # all samples on one atom: the factor as a whole, by its backward error
    for t in range(T):
        f = model.sample_functions(x, draws=unit_draws(D), atoms=np.full((N_T, D), t)).cpu().numpy()
        for col in range(D):
            l = (f[:, :, col] - p['mean'][t][:, col][None]).T
            want = p['cov'][t, col] + JITTER * p['alpha'][t] * np.eye(N_T)
            assert np.max(np.abs(l @ l.T - want)) <= TOL * np.max(np.abs(p['cov'][t, col])), (t, col)
    with pytest.raises(AssertionError):
        model.sample_functions(x, atoms=np.full((2, D), T))


@pytest.mark.parametrize('case', CASES)
def test_samples_are_affine_in_the_draws_and_seeded(case):
    model, x = model_of(case), points(case)
    rs = np.random.default_rng(8)
    mrd, over_t = case.startswith('mrd'), case.startswith('over_t')
    widths = [D0, D - D0] if mrd else [D]
    kw = dict(atoms=rs.integers(0, T, (3, D))) if over_t else {}
    a, b = [rs.standard_normal((3, N_T, w)) for w in widths], [rs.standard_normal((3, N_T, w)) for w in widths]
    run = lambda ds: listed(case, model.sample_functions(x, draws=ds if mrd else ds[0], **kw))
    zero = run([np.zeros_like(d) for d in a])
    fa, fb, fc = run(a), run(b), run([2.0 * p - 0.5 * q for p, q in zip(a, b)])
    for z, one, two, both in zip(zero, fa, fb, fc):
        want = z + 2.0 * (one - z) - 0.5 * (two - z)
        assert float((both - want).abs().max()) <= 1e-12 * max(1.0, float(both.abs().max()))
        assert float((one - z).abs().max()) > 1e-3
    s0, s0b, s1 = (listed(case, model.sample_functions(x, num_samples=5, seed=s)) for s in (0, 0, 1))
    for p, q, r in zip(s0, s0b, s1):
        assert tuple(p.shape)[:2] == (5, N_T) and torch.equal(p, q) and not torch.equal(p, r)
        assert torch.isfinite(p).all()


@pytest.mark.parametrize('case', CASES)
def test_whitened_residuals_are_standard_normal(case, monkeypatch):
    """noise=True, seed 0, S = 4096: L^-1 (sample - mean), L applied on the host, has component means within 6 / sqrt(S) of 0 and
    variances within 6 sqrt(2 / S) of 1 (six standard errors; the seed is fixed, so the test is deterministic)."""
    s = 4096
    model, x = model_of(case), points(case)
    pieces = restated(case, model, x, monkeypatch)
    if case.startswith('over_t'):
        p = pieces[0]
        atoms = np.random.default_rng(2).integers(0, T, (s, D))
        f = model.sample_functions(x, num_samples=s, noise=True, seed=0, atoms=atoms).cpu().numpy()
        res = np.zeros_like(f)
        for t in range(T):
            for col in range(D):
                l = np.linalg.cholesky(p['cov'][t, col] + (JITTER * p['alpha'][t] + 1.0 / p['beta'][t]) * np.eye(N_T))
                rows = atoms[:, col] == t
                res[rows, :, col] = np.linalg.solve(l, (f[rows, :, col] - p['mean'][t][:, col][None]).T).T
        residuals = [res]
    else:
        residuals = []
        for f, p in zip(listed(case, model.sample_functions(x, num_samples=s, noise=True, seed=0)), pieces):
            f = f.cpu().numpy()
            assert f.shape == (s, N_T, p['cov'].shape[0])
            res = np.zeros_like(f)
            for col in range(f.shape[2]):
                l = np.linalg.cholesky(p['cov'][col] + (JITTER * p['alpha'][col] + 1.0 / p['beta'][col]) * np.eye(N_T))
                res[:, :, col] = np.linalg.solve(l, (f[:, :, col] - p['mean'][:, col][None]).T).T
            residuals.append(res)
    for res in residuals:
        mean, var = res.mean(axis=0), res.var(axis=0)
        print('%s: max |mean| %.4f (bound %.4f), max |var - 1| %.4f (bound %.4f)'
              % (case, np.max(np.abs(mean)), 6 / np.sqrt(s), np.max(np.abs(var - 1)), 6 * np.sqrt(2 / s)))
        assert np.max(np.abs(mean)) <= 6 / np.sqrt(s)
        assert np.max(np.abs(var - 1)) <= 6 * np.sqrt(2 / s)


@pytest.mark.parametrize('case', CASES)
def test_a_short_segment_needs_the_jitter(case):
    """33 points on a short straight segment: a gram whose small eigenvalues lie below rounding."""
    model, x = model_of(case), points(case)
    w = torch.linspace(0.0, 1.0, 33, dtype=torch.float64, device=DEV)[:, None]
    seg = x[0][None] + w * 0.05 * (x[1] - x[0])[None]
    out = listed(case, model.sample_functions(seg, num_samples=2))
    assert all(torch.isfinite(f).all() and f.shape[:2] == (2, 33) for f in out)
    with pytest.raises(FloatingPointError, match='jitter'):
        model.sample_functions(seg, num_samples=2, jitter=0.0)


@pytest.mark.parametrize('case', ['bgplvm', 'bgplvm masked', 'mrd masked', 'over_t masked'])
def test_only_the_patterns_that_the_columns_touch_are_evaluated(case, monkeypatch):
    from dp_gp_lvm_amd import ops
    model, x = model_of(case), points(case)
    seen = []
    real = ops.ard_rbf_point_cov
    monkeypatch.setattr(ops, 'ard_rbf_point_cov', lambda z, xx, gamma, alpha, c: seen.append(tuple(c.shape[:2])) or real(z, xx, gamma, alpha, c))
    kw = (lambda cols: dict(views=[0], columns=[cols])) if case.startswith('mrd') else (lambda cols: dict(columns=cols))
    whole = listed(case, model.predictive_covariance(x, **(dict(views=[0]) if case.startswith('mrd') else {})))[0]
    k = T if case.startswith('over_t') else 1
    if not case.endswith('masked'):
        assert seen == [(1, 1)]                                          # complete data: one pattern, no prior pattern
        return
    assert seen[0][0] == k and seen[0][1] >= 3                          # the random mask: several row patterns (+ the prior's)
    for cols, want in (([0], 1), ([UNSEEN], 1), ([0, UNSEEN], 2), ([0, 0], 1)):
        del seen[:]
        part = listed(case, model.predictive_covariance(x, **kw(cols)))[0]
        assert seen == [(k, want)], (cols, seen)
        assert float((part - whole[cols]).abs().max()) <= (0.0 if k == 1 else 1e-12)


# ---- the composed route of marginals._Marginals.pattern_covariance (many points) ---------------------------------------------------
def test_composed_form_is_the_fused_operator():
    from dp_gp_lvm_amd import ops
    from test_point_cov_refs import CASES as OP_CASES, case as op_case
    i = OP_CASES.index(dict(K=2, G=3, N=63, M=129, Q=10))
    inp, ref = op_case(i)
    z, x, gamma, alpha, c = (torch.as_tensor(np.array(inp[n]), device=DEV) for n in ('z', 'x', 'gamma', 'alpha', 'c'))
    fused, comp = ops.ard_rbf_point_cov(z, x, gamma, alpha, c), marginals.composed_covariance(z, x, gamma, alpha, c)
    assert torch.equal(comp, comp.transpose(2, 3))
    den = np.asarray(ref['den'], dtype=np.float64)
    assert np.max(np.abs(comp.cpu().numpy() - np.asarray(ref['out'], dtype=np.float64)) / den) <= 1e-12
    assert np.max(np.abs((comp - fused).cpu().numpy()) / den) <= 1e-12


@pytest.mark.parametrize('case', ['bgplvm', 'over_t masked'])
def test_many_points_take_the_composed_route_and_agree(case, monkeypatch):
    model = model_of(case)
    n_big = 2048
    k, g = (1, 1) if case == 'bgplvm' else (T, 3)
    assert marginals.composed_is_faster(k, g, n_big, M) and not marginals.composed_is_faster(k, g, 33, M)
    assert not marginals.composed_is_faster(60, 1, 33, 50) and marginals.composed_is_faster(8, 16, 500, 128)
    xm = model.q_x[0].detach()
    rs = np.random.default_rng(6)
    x = xm[torch.as_tensor(rs.integers(0, N, n_big), device=DEV)] + 0.2 * torch.as_tensor(rs.standard_normal((n_big, Q)), device=DEV)
    calls = []
    real = marginals.composed_covariance
    monkeypatch.setattr(marginals, 'composed_covariance', lambda *a: calls.append(1) or real(*a))
    routed = model.predictive_covariance(x, columns=[0], noise=True)
    assert calls and torch.equal(routed, routed.transpose(1, 2))
    monkeypatch.setattr(marginals, 'composed_is_faster', lambda *a: False)
    fused = model.predictive_covariance(x, columns=[0], noise=True)
    assert len(calls) == 1
    assert float((routed - fused).abs().max()) <= 1e-12 * float(fused.abs().max())
    _, var = model.predictive_marginals(x, torch.zeros_like(x), columns=[0])
    assert close(torch.diagonal(routed, dim1=1, dim2=2).transpose(0, 1), var.cpu().numpy())[0]


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
        for name in ('predictive_covariance', 'sample_functions'):
            with pytest.raises(AssertionError, match='%s is not built for a model sharded over a process group' % name):
                getattr(model, name)(x)
    finally:
        if created:
            dist.destroy_process_group()
