"""GPU tests of training dp_gp_lvm_t on data with missing entries (observed=...): the T x P slot bound of
models/masked_bound_t.py, on the pattern-grouped Psi operators (default) and in the slot form on the weighted operators
(DPGP_GROUPED_PSI=0), against the reference's fixtures (all-True mask), the committed fp64 oracle evaluated per output dim on the
rows at which that dim was observed (general masks), the masked bayesian_gp_lvm (T = 1), and training + imputation on synthetic
data.  Tolerances: rtol 1e-10 for objectives, 1e-7 of each variable's largest entry for gradients (the fp64 tolerances of the
README)."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_gpu_predict_b1 import close
from test_gpu_predict_masked import masks_of
from test_gpu_train_masked import synthetic

pytestmark = pytest.mark.gpu
FIXTURES = ['model_t_ref_40_6_12_3_T4', 'model_t_ref_60_10_15_4_T5']
REF2RAW = dict(x_mean='x_mean', x_var_raw='x_var', x_u='x_u', dp_logits='dp_logits', gamma_1_raw='dp_gamma_1',
               gamma_2_raw='dp_gamma_2', gamma_atoms_raw='gamma_atoms', alpha_atoms_raw='alpha_atoms', beta_atoms_raw='beta_atoms')
RAW_ORDER = ['x_mean', 'x_var', 'x_u', 'gamma_atoms', 'alpha_atoms', 'beta_atoms', 'dp_logits', 'dp_gamma_1', 'dp_gamma_2', 'dp_w']


def softplus(x):
    return np.logaddexp(0.0, x)


def raw_of(g, mask_size=1):
    from oracle import dpgp_oracle_torch as ot
    raw = {k: np.asarray(g[k], dtype=np.float64) for k in ot.NAMES}
    if mask_size != 1:
        raw['dp_logits'] = raw['dp_logits'][:raw['dp_logits'].shape[0] // mask_size]
    return raw


def build_masked_t(g, dev, obs, y=None, mask_size=1, **kw):
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm_t
    sp, raw = softplus, raw_of(g, mask_size)
    iv = dict(x_mean=raw['x_mean'], x_var=sp(raw['x_var_raw']), x_u=raw['x_u'], phi_logits=raw['dp_logits'],
              gamma_atoms=sp(raw['gamma_atoms_raw']), alpha_atoms=sp(raw['alpha_atoms_raw']), beta_atoms=sp(raw['beta_atoms_raw']),
              gamma_1=sp(raw['gamma_1_raw']), gamma_2=sp(raw['gamma_2_raw']), w_1=float(sp(raw['w_1_raw'])),
              w_2=float(sp(raw['w_2_raw'])))
    args = dict(num_latent_dims=raw['x_mean'].shape[1], num_inducing_points=raw['x_u'].shape[0],
                truncation_level=raw['dp_logits'].shape[1], alpha_prior_params=np.array([float(g['s_1']), float(g['s_2'])]),
                mask_size=mask_size, device=dev, initial_values=iv, observed=obs)
    args.update(kw)
    return dp_gp_lvm_t(g['y'] if y is None else y, **args)


def oracle_masked_t(y, obs, g, mask_size=1):
    """dp_objective - (sum_d f_hat_t of column d on its rows R_d - KL over all rows) - hyper-prior, composed as ot.objective_t, at
    the fixture's raw variables; its gradients by autograd.  Returns (objective, {name: gradient}, f_hat, KL)."""
    from oracle import dpgp_oracle_torch as ot
    raw = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in raw_of(g, mask_size).items()}
    yt = torch.as_tensor(np.where(obs, y, 0.0), dtype=torch.float64)
    mu, z, s = raw['x_mean'], raw['x_u'], ot._softplus(raw['x_var_raw'])
    phi = torch.softmax(raw['dp_logits'], dim=-1)
    if mask_size != 1:
        phi = torch.repeat_interleave(phi, int(mask_size), dim=0)
    g1, g2 = ot._softplus(raw['gamma_1_raw']).reshape(-1), ot._softplus(raw['gamma_2_raw']).reshape(-1)
    w1, w2 = ot._softplus(raw['w_1_raw']).reshape(()), ot._softplus(raw['w_2_raw']).reshape(())
    gat, aat, bat = (ot._softplus(raw[k]) for k in ('gamma_atoms_raw', 'alpha_atoms_raw', 'beta_atoms_raw'))
    f = torch.zeros((), dtype=torch.float64)
    for d in range(obs.shape[1]):
        r = np.flatnonzero(obs[:, d])
        if r.size:
            f = f + ot.fhat_t(yt[r, d:d + 1], z, mu[r], s[r], phi[d:d + 1], gat, aat[:, 0], bat[:, 0])
    kl = 0.5 * (torch.sum(mu * mu) + torch.sum(s - torch.log(s)) - mu.shape[0] * mu.shape[1])
    hyper = sum(torch.sum(ot._log_normal_log_pdf(a)) for a in (gat, aat, bat))
    dp = ot.dp_objective(phi, g1, g2, w1, w2, float(g['s_1']), float(g['s_2']))
    obj = dp - (f - kl) - hyper
    grads = torch.autograd.grad(obj, [raw[k] for k in ot.NAMES], allow_unused=True)
    grads = {k: (np.zeros(tuple(raw[k].shape)) if v is None else v.numpy()) for k, v in zip(ot.NAMES, grads)}
    return float(obj.detach()), grads, float(f.detach()), float(kl.detach())


ORACLE = {}


def oracle_of(fixture, kind, mask_size=1):
    """The oracle's answer for (fixture, mask kind), computed once and shared by the two operator settings."""
    key = (fixture, kind, mask_size)
    if key not in ORACLE:
        g = golden(fixture)
        obs = masks_of(*g['y'].shape, 23)[kind]
        ORACLE[key] = (obs,) + oracle_masked_t(g['y'], obs, g, mask_size)
    return ORACLE[key]


def check_gradients(model, got, want_of):
    assert list(got) == RAW_ORDER
    for k, v in got.items():
        assert v.shape == model.raw[k].shape and v.dtype == torch.float64, k
    pairs = [(ref, got[raw].cpu().numpy(), np.asarray(want_of(ref))) for ref, raw in REF2RAW.items()]
    pairs.append(('w_raw', got['dp_w'].cpu().numpy(), np.array([float(want_of('w_1_raw')), float(want_of('w_2_raw'))])))
    for name, have, want in pairs:
        scale = np.abs(want).max()
        print('%s: max |err| %.3e of %.3e' % (name, np.abs(have.reshape(want.shape) - want).max(), scale))
        np.testing.assert_allclose(have.reshape(want.shape), want, rtol=0, atol=1e-7 * scale, err_msg=name)


@pytest.mark.parametrize('grouped', ['1', '0'])
@pytest.mark.parametrize('fixture', FIXTURES)
def test_all_true_mask_equals_the_reference(dev, fixture, grouped, monkeypatch):
    monkeypatch.setenv('DPGP_GROUPED_PSI', grouped)
    g = golden(fixture)
    model = build_masked_t(g, dev, np.ones(g['y'].shape, dtype=bool))
    terms = model.objective_terms
    print('objective %.15g (fixture %.15g)' % (float(terms[0]), float(g['objective'])))
    assert tuple(terms.shape) == (5,) and int(model.cholesky_info) == 0
    np.testing.assert_allclose(float(model.objective), float(g['objective']), rtol=1e-10)
    check_gradients(model, model.gradients(), lambda name: g['grad_' + name])


@pytest.mark.parametrize('grouped', ['1', '0'])
@pytest.mark.parametrize('kind', ['random30', 'block', 'odd'])
@pytest.mark.parametrize('fixture', FIXTURES)
def test_general_masks_match_the_oracle(dev, fixture, kind, grouped, monkeypatch):
    monkeypatch.setenv('DPGP_GROUPED_PSI', grouped)
    g = golden(fixture)
    obs, want, grads, f, kl = oracle_of(fixture, kind)
    model = build_masked_t(g, dev, obs, y=np.where(obs, g['y'], np.nan))      # unobserved entries are NaN: they are ignored
    have = model.objective
    assert have.dim() == 0 and have.dtype == torch.float64 and have.is_cuda
    terms = model.objective_terms.cpu().numpy()
    print('%s %s: objective %.15g (oracle %.15g), %d patterns' % (fixture, kind, float(have), want,
                                                                  len({obs[:, d].tobytes() for d in range(obs.shape[1])})))
    np.testing.assert_allclose(float(have), want, rtol=1e-10)
    np.testing.assert_allclose(terms[1:3], [f, kl], rtol=1e-10)
    assert int(model.cholesky_info) == 0
    check_gradients(model, model.gradients(), lambda name: grads[name])


def test_objective_terms_graph_is_the_eager_evaluation(dev):
    """With observed= nothing is captured into a HIP graph: objective_terms_graph() is the eager evaluation (same launches, so
    the same bits), it matches the oracle, and it sees an update of the raw variables."""
    g = golden(FIXTURES[0])
    obs, want, _, _, _ = oracle_of(FIXTURES[0], 'random30')
    model = build_masked_t(g, dev, obs, y=np.where(obs, g['y'], np.nan))
    first = model.objective_terms_graph()
    assert tuple(first.shape) == (5,) and torch.equal(first, model.objective_terms)
    np.testing.assert_allclose(float(first[0]), want, rtol=1e-10)
    with torch.no_grad():
        model.raw['x_mean'].mul_(1.01)
    second = model.objective_terms_graph()
    assert torch.equal(second, model.objective_terms) and float(second[0]) != float(first[0])


@pytest.mark.parametrize('grouped', ['1', '0'])
def test_mask_size_two(dev, grouped, monkeypatch):
    """mask_size = 2: a logits row serves two output dims; the first D / 2 rows of the fixture's logits."""
    monkeypatch.setenv('DPGP_GROUPED_PSI', grouped)
    g = golden(FIXTURES[1])
    obs, want, grads, _, _ = oracle_of(FIXTURES[1], 'random30', 2)
    model = build_masked_t(g, dev, obs, y=np.where(obs, g['y'], np.nan), mask_size=2)
    assert tuple(model.raw['dp_logits'].shape) == (g['y'].shape[1] // 2, g['dp_logits'].shape[1])
    np.testing.assert_allclose(float(model.objective), want, rtol=1e-10)
    check_gradients(model, model.gradients(), lambda name: grads[name])


@pytest.mark.parametrize('grouped', ['1', '0'])
def test_one_atom_equals_the_masked_bayesian_gp_lvm(dev, grouped, monkeypatch):
    monkeypatch.setenv('DPGP_GROUPED_PSI', grouped)
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm_t
    from test_gpu_train_masked import build_masked
    g = golden('bgplvm_ref_70_9_20_4')
    y = g['y']
    obs = masks_of(*y.shape, 23)['random30']
    y_nan = np.where(obs, y, np.nan)
    one = build_masked(g, dev, obs, y=y_nan)
    iv = dict(x_mean=g['x_mean'], x_var=softplus(g['x_var_raw']), x_u=g['x_u'], gamma_atoms=softplus(g['gamma_raw']),
              alpha_atoms=softplus(g['alpha_raw']), beta_atoms=softplus(g['beta_raw']))
    model = dp_gp_lvm_t(y_nan, num_latent_dims=g['x_mean'].shape[1], num_inducing_points=g['x_u'].shape[0], truncation_level=1,
                        device=dev, initial_values=iv, observed=obs)
    have = model.objective_terms.cpu().numpy()                               # (objective, f_hat, KL, DP objective, hyper-prior)
    objective_one = float(one.objective)
    f = float(one.objective_terms.sum())                                     # (the masked B-GPLVM's [slots x 5] f_hat terms)
    mu, sv = g['x_mean'], softplus(g['x_var_raw'])
    kl = 0.5 * (np.sum(mu * mu) + np.sum(sv - np.log(sv)) - mu.size)
    print('f_hat %.15g (B-GPLVM %.15g), KL %.15g (%.15g)' % (have[1], f, have[2], kl))
    np.testing.assert_allclose(have[1], f, rtol=1e-10)
    np.testing.assert_allclose(have[2], kl, rtol=1e-10)
    np.testing.assert_allclose(have[0] - have[3], objective_one, rtol=1e-10)      # (all but the DP objective)
    got, want = model.gradients(), one.gradients()
    for k in ('x_mean', 'x_var', 'x_u', 'gamma_atoms', 'alpha_atoms', 'beta_atoms'):
        close(got[k], want[k].cpu().numpy().reshape(tuple(got[k].shape)), 1e-10, k)


@pytest.mark.parametrize('seed', [5, 6, 7])
def test_training_and_imputation(dev, seed):
    """T = 3, Q = 2, M = 10, 300 Adam steps at 0.05 from the masked bayesian_gp_lvm test's start (x_mean: the standardised PCA of
    the column-mean-filled data), zero logits, unit atoms.  Reference figures (CPU oracle + torch Adam, the same formulation):
    imputation RMSE 0.116 / 0.131 / 0.118 against 0.713 / 0.745 / 0.722 for column means; the objective falls from about 510 to
    about 210."""
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm_t
    from dp_gp_lvm_amd.utils import missing
    from dp_gp_lvm_amd.utils.expressions import principal_component_analysis as pca
    from oracle import dpgp_oracle_torch as ot
    y, mask = synthetic(seed)
    n, d, t = y.shape[0], y.shape[1], 3
    filled = missing.column_mean_filled(y, mask)
    x0 = pca(filled, num_latent_dimensions=2)
    x0 = (x0 - x0.mean(axis=0)) / x0.std(axis=0)
    x_u = x0[np.random.default_rng(seed + 100).permutation(n)[:10]]
    model = dp_gp_lvm_t(np.where(mask, y, np.nan), num_latent_dims=2, num_inducing_points=10, truncation_level=t, device=dev,
                        observed=mask,
                        initial_values=dict(x_mean=x0, x_var=np.full((n, 2), 0.5), x_u=x_u, phi_logits=np.zeros((d, t)),
                                            gamma_atoms=np.ones((t, 2)), alpha_atoms=np.ones((t, 1)), beta_atoms=np.ones((t, 1))))
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
    # the per-column mixture formula in NumPy fp64 at the model's final parameters
    z, mu = model.inducing_input.detach().cpu(), model.q_x[0].detach().cpu()
    s = torch.diagonal(model.q_x[1], dim1=-2, dim2=-1).detach().cpu()
    gam, al, be = (a.detach().cpu() for a in model.dp_atoms)
    phi = model.assignments.detach().cpu().numpy()                                                   # [D, T]
    _, _, v_all = ot.psi_pieces_t(torch.eye(n, dtype=torch.float64), z, mu, s, gam, al[:, 0])       # Psi1_t^T of every row [T,M,N]
    want = np.where(mask, y, 0.0)
    for j in range(d):
        r = np.flatnonzero(mask[:, j])
        k_uu, p2, _ = ot.psi_pieces_t(torch.as_tensor(y[r, j:j + 1]), z, mu[r], s[r], gam, al[:, 0])
        col = np.zeros(n)
        for a in range(t):
            psi1 = v_all[a].numpy().T                                                                # [N, M]
            col += phi[j, a] * float(be[a]) * psi1 @ np.linalg.solve(k_uu[a].numpy() + float(be[a]) * p2[a].numpy(),
                                                                      psi1[r].T @ y[r, j])
        want[~mask[:, j], j] = col[~mask[:, j]]
    close(imputed, want, 1e-9, 'imputation')


def test_argument_checks(dev):
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm_t
    g = golden(FIXTURES[0])
    y = g['y']
    obs = masks_of(*y.shape, 23)['random30']
    build_masked_t(g, dev, obs, precision='f64')                               # fine
    with pytest.raises(AssertionError):
        build_masked_t(g, dev, obs, precision='mixed')
    with pytest.raises(AssertionError):
        build_masked_t(g, dev, obs, process_group=object())
    with pytest.raises(AssertionError):
        build_masked_t(g, dev, obs.astype(np.float64))                          # not boolean
    with pytest.raises(AssertionError):
        build_masked_t(g, dev, obs[:-1])                                        # shape mismatch
    with pytest.raises(AssertionError):
        build_masked_t(g, dev, np.zeros(y.shape, dtype=bool))                   # nothing observed
    plain = dp_gp_lvm_t(y, num_latent_dims=3, num_inducing_points=12, truncation_level=4, device=dev)
    with pytest.raises(AssertionError):
        plain.impute_training_data()
