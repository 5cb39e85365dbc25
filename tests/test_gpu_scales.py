"""GPU tests of the mixed-precision training step across input magnitudes ("Magnitude sweep").

Every existing test of the f16 hi/lo-split pass kernels (psi2_pairs_grad.hip) draws its inputs from one regime: y ~ N(0,1), gamma
~ 0.5, s ~ 1, alpha ~ 1, beta ~ 2.  An f16 pair has a narrow range (normal from 6.1e-5, overflow past 65504, its lo half subnormal
below ~2^-3), and training visits other magnitudes: ARD drives the gamma of unused latent dims down, the variances s shrink or
grow per point, beta grows as the fit improves, and Adam normalises every gradient entry on its own.  Here one axis at a time moves
away from a well-conditioned base point, and every path is held to its documented tolerance PER COLUMN (per latent dim for
d mu, d S, d z, d gamma; per output dim for d alpha, d beta and the f_hat terms), so that a small column is held to account.

References: the fp64 autograd oracle (oracle/dpgp_oracle_torch.py) on the small shape; the library's all-fp64 path (itself pinned
to the oracle at 1e-8 at every point of the sweep) at the model-level shape (BASELINE config 2)."""
import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import ops
from oracle import dpgp_oracle as orc
from oracle import dpgp_oracle_torch as ot

pytestmark = pytest.mark.gpu

SHAPE = (240, 6, 16, 6)                       # N, D, M, Q
GRAD_TOL = 5e-4                               # mixed-precision gradients, per column
TERM_TOL = 2e-5                               # mixed f_hat terms: of each output dim's largest term
SUM_RTOL = 2e-6
F64_TOL = 1e-8                                # the fp64 path against the oracle

# axis -> values.  'y': the whole matrix times the value; 'ycol': each output dim its own scale; 'gamma_half': half the latent dims at
# the value; 'gamma_big': every gamma near the value; 's', 'alpha', 'beta': the whole array times the value
CASES = ([('y', v) for v in (2.0 ** -20, 2.0 ** -12, 1e-4, 1.0, 1e3, 1e5, 2.0 ** 20)] + [('ycol', 0.0)]
         + [('gamma_half', v) for v in (1e-2, 1e-4, 1e-6)] + [('gamma_big', 20.0)]
         + [('s', v) for v in (1e-6, 1e2)] + [('alpha', v) for v in (1e-3, 1e3)] + [('beta', v) for v in (1e-2, 1e2)])
# the conditioning guard's bound is absolute and grows with y^2 and beta^3: info = -2 is allowed on these axes (the terms and gradients
# are still written and still compared)
GUARD_AXES = ('y', 'ycol', 'beta')
Z_SPREAD, G0 = 1.0, 1.0             # (inducing inputs inside the cloud of latent means, length scales ~1: K_uu well conditioned)


def case_id(c):
    return '%s=%g' % c if c[0] != 'ycol' else 'ycol'


def problem(shape, axis, v, seed=7):
    """fp64 NumPy inputs of one sweep point: a well-conditioned base (inducing inputs inside the cloud of latent means), one axis
    moved."""
    n, d, m, q = shape
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((n, d))
    y = (y - y.mean(0)) / y.std(0)
    mu = rng.standard_normal((n, q))
    z = Z_SPREAD * rng.standard_normal((m, q))
    s = 0.5 * np.exp(0.3 * rng.standard_normal((n, q)))
    gamma = G0 * np.exp(0.2 * rng.standard_normal((d, q)))
    alpha = np.exp(0.2 * rng.standard_normal(d))
    beta = 2.0 * np.exp(0.2 * rng.standard_normal(d))
    if axis == 'y':
        y = y * v
    elif axis == 'ycol':
        y = y * np.logspace(-4.0, 5.0, d)[None, :]
    elif axis == 'gamma_half':
        gamma[:, q // 2:] = v * np.exp(0.2 * rng.standard_normal((d, q - q // 2)))
    elif axis == 'gamma_big':
        # length scales of ~0.2: latent means and inducing inputs on the same small cloud, so that every point sees an inducing input
        # (range guard of the f16-split exponent: psi2_pairs.hip) and K_uu stays near the identity
        gamma = v * np.exp(0.1 * rng.standard_normal((d, q)))
        mu, z = 0.15 * mu, 0.15 * z
        s = 0.02 * s
    elif axis == 's':
        s = s * v
    elif axis == 'alpha':
        alpha = alpha * v
    elif axis == 'beta':
        beta = beta * v
    return dict(y=y, z=z, mu=mu, s=s, gamma=gamma, alpha=alpha, beta=beta)


NAMES = ('y', 'z', 'mu', 's', 'gamma', 'alpha', 'beta')


def on_dev(p, dev):
    return [torch.as_tensor(np.ascontiguousarray(p[k]), dtype=torch.float64, device=dev) for k in NAMES]


def npy(a):
    return a.detach().cpu().numpy()


def check_cols(got, want, tol, what):
    """|got - want| <= tol * max |want[:, j]| for every column j (a [N|M|D, Q] gradient: per latent dim)."""
    got, want = np.asarray(got), np.asarray(want)
    assert np.isfinite(got).all(), '%s: non-finite entries' % what
    scale = np.abs(want).max(axis=0)
    err = np.abs(got - want).max(axis=0)
    bad = err > tol * scale
    assert not bad.any(), '%s: columns %s off by %s of their largest entry (tolerance %g)' % (
        what, np.flatnonzero(bad).tolist(), (err / np.where(scale > 0, scale, 1.0))[bad].tolist(), tol)


def check_rows(got, want, tol, what):
    """per output dim: |got[d] - want[d]| <= tol * max |want[d, :]|"""
    check_cols(np.asarray(got).reshape(len(want), -1).T, np.asarray(want).reshape(len(want), -1).T, tol, what)


def check_rel(got, want, tol, what):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert np.isfinite(got).all(), '%s: non-finite entries' % what
    err = np.abs(got - want) / np.abs(want)
    assert (err <= tol).all(), '%s: entries %s off by %s relative (tolerance %g)' % (what, np.flatnonzero(err > tol).tolist(),
                                                                                      err[err > tol].tolist(), tol)


def check_grads(got, ref, tol, what):
    """got: (d_mu, d_S, d_z, d_gamma[, d_alpha_beta]); ref: fhat_input_gradients-like dict."""
    for name, g in zip(('d_mu', 'd_s', 'd_z', 'd_gamma'), got[:4]):
        check_cols(npy(g), ref[name], tol, '%s: %s' % (what, name))
    if len(got) > 4:
        dab = npy(got[4])
        check_rel(dab[:, 0], ref['d_alpha'], tol, what + ': d_alpha')
        check_rel(dab[:, 1], ref['d_beta'], tol, what + ': d_beta')


def check_info(info, axis, what):
    info = npy(info)
    assert (info <= 0).all(), '%s: failed factorisation, info = %s' % (what, info)
    if axis not in GUARD_AXES:
        assert (info == 0).all(), '%s: flagged off the y / beta axes (move the point), info = %s' % (what, info)
    return np.flatnonzero(info == -2).tolist()


_REF = {}


def reference(axis, v):
    """oracle terms [D,5] and d f_hat / d (mu, S, z, gamma, alpha, beta) of a sweep point (cached: several tests share it)."""
    key = (axis, v)
    if key not in _REF:
        p = problem(SHAPE, axis, v)
        tt = {k: torch.as_tensor(p[k], dtype=torch.float64) for k in NAMES}
        terms = ot.fhat(tt['y'], tt['z'], tt['mu'], tt['s'], tt['gamma'], tt['alpha'], tt['beta']).numpy()
        g = ot.fhat_input_gradients(p['y'], p['z'], p['mu'], p['s'], p['gamma'], p['alpha'], p['beta'])
        _REF[key] = (p, terms, g)
    return _REF[key]


def f64_path(args, shape, dev):
    """the library's all-fp64 evaluation: terms, sums, info, stage-A adjoints, gradients"""
    n, d, m, q = shape
    w = ops.ElboWorkspace(d, n, m, q, 'f64', dev)
    terms, sums, info = [a.clone() for a in ops.elbo_fhat(*args, prec='f64', workspace=w)]
    gp, wk, gv, dab, infog = ops.elbo_grad_chain(args[5], args[6], w)
    g = ops.elbo_grad_psi(args[0], args[1], args[2], args[3], args[4], args[5], gp, wk, gv, prec='f64')
    return terms, sums, info, (gp, wk, gv), (*g, dab), infog


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_fp64_path_against_the_oracle(dev, case):
    """The reference of the mixed paths at the model-level shape is the library's fp64 path: pinned to the oracle at every scale."""
    axis, v = case
    p, terms_ref, gref = reference(axis, v)
    args = on_dev(p, dev)
    terms, sums, info, _, grads, infog = f64_path(args, SHAPE, dev)
    assert not npy(info).any() and not npy(infog).any()
    check_rows(npy(terms), terms_ref, F64_TOL, 'fp64 terms')
    check_grads(grads, gref, F64_TOL, 'fp64 gradients')


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_mixed_forward(dev, case):
    """ops.elbo_fhat(prec='mixed'): the f_hat terms within 2e-5 of each output dim's largest term, f_hat within 2e-6."""
    axis, v = case
    p, terms_ref, _ = reference(axis, v)
    n, d, m, q = SHAPE
    w = ops.ElboWorkspace(d, n, m, q, 'mixed', dev)
    terms, sums, info = ops.elbo_fhat(*on_dev(p, dev), prec='mixed', workspace=w)
    check_info(info, axis, 'mixed forward')
    check_rows(npy(terms), terms_ref, TERM_TOL, 'mixed forward terms')
    check_rel(npy(sums)[0], terms_ref.sum(), SUM_RTOL, 'mixed forward f_hat')


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_mixed_stage_b_on_exact_adjoints(dev, case):
    """Stage B alone, elbo_grad_psi(prec='mixed') — the pair-tile form of the Psi2 term and the Psi1 term through the same passes —
    on the fp64 forward's adjoints (no guard in the way): d mu, d S, d z, d gamma within 5e-4 of each column's largest entry."""
    axis, v = case
    p, _, gref = reference(axis, v)
    args = on_dev(p, dev)
    _, _, _, adj, _, _ = f64_path(args, SHAPE, dev)
    got = ops.elbo_grad_psi(args[0], args[1], args[2], args[3], args[4], args[5], *adj, prec='mixed')
    check_grads(got, gref, GRAD_TOL, 'mixed stage B')


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_mixed_three_calls(dev, case):
    """elbo_fhat(prec='mixed') + elbo_grad_chain + elbo_grad_psi(prec='mixed') against the oracle."""
    axis, v = case
    p, terms_ref, gref = reference(axis, v)
    args = on_dev(p, dev)
    n, d, m, q = SHAPE
    w = ops.ElboWorkspace(d, n, m, q, 'mixed', dev)
    terms, sums, info = ops.elbo_fhat(*args, prec='mixed', workspace=w)
    check_info(info, axis, 'three calls, forward')
    gp, wk, gv, dab, infog = ops.elbo_grad_chain(args[5], args[6], w)
    check_info(infog, axis, 'three calls, stage A')
    g = ops.elbo_grad_psi(args[0], args[1], args[2], args[3], args[4], args[5], gp, wk, gv, prec='mixed')
    check_rows(npy(terms), terms_ref, TERM_TOL, 'three calls, terms')
    check_grads((*g, dab), gref, GRAD_TOL, 'three calls')


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_mixed_training_step(dev, case):
    """ops.elbo_step (dpgp_elbo_step: Psi2 and Psi1^T y out of the first passes of stage B) against the oracle: terms, f_hat,
    and all six gradients."""
    axis, v = case
    p, terms_ref, gref = reference(axis, v)
    args = on_dev(p, dev)
    n, d, m, q = SHAPE
    w = ops.ElboWorkspace(d, n, m, q, 'mixed', dev)
    b = ops.ElboStepBuffers(d, n, m, q, dev)
    (terms, sums, info), grads = ops.elbo_step(*args, workspace=w, buffers=b)
    check_info(info, axis, 'step, forward')
    check_info(grads[5], axis, 'step, stage A')
    check_rows(npy(terms), terms_ref, TERM_TOL, 'step, terms')
    check_rel(npy(sums)[0], terms_ref.sum(), SUM_RTOL, 'step, f_hat')
    check_grads(grads[:5], gref, GRAD_TOL, 'step')


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_fp32_psi_statistics(dev, case):
    """The standalone fp32 kernels ops.psi1T_y and ops.psi2 against the NumPy oracle, per output dim (tolerances of
    tests/test_gpu_kernels.py: Psi1^T y 2e-5 of the output dim's largest entry; Psi2 rtol 1e-4 + 1e-6 of its largest entry)."""
    axis, v = case
    p = problem(SHAPE, axis, v)
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    zs = [f32(p[k]) for k in ('z', 'mu', 's', 'gamma')] + [f32(p['alpha'][:, None])]
    want1 = orc.psi1T_y(p['z'], p['mu'], p['s'], p['gamma'], p['alpha'][:, None], p['y'])
    check_rows(npy(ops.psi1T_y(*zs, f32(p['y']))).astype(np.float64), want1, 2e-5, 'psi1T_y')
    want2 = orc.psi2(p['z'], p['mu'], p['s'], p['gamma'], p['alpha'][:, None])
    got2 = npy(ops.psi2(*zs)).astype(np.float64)
    assert np.isfinite(got2).all()
    err = np.abs(got2 - want2) - 1e-4 * np.abs(want2)
    scale = np.abs(want2).reshape(len(want2), -1).max(axis=1)
    assert (err.reshape(len(want2), -1).max(axis=1) <= 1e-6 * scale).all(), 'psi2'


# ---- model level, BASELINE config 2 (N = 2000, D = 64, M = 128, Q = 10): the training configuration and the mixed model against
# the fp64 model, on the y axis (the data enters the model as it is given; the other axes are reached by training from there)
MODEL_CASES = [('y', 2.0 ** -12), ('y', 1.0), ('y', 1e3), ('ycol', 0.0)]
RAW_NAMES = ('x_mean', 'x_var', 'x_u', 'gamma_atoms', 'alpha_atoms', 'beta_atoms')


def _model(p, y, dev, **kw):
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
    return dp_gp_lvm(y, num_latent_dims=p['mu'].shape[1], num_inducing_points=p['z'].shape[0], truncation_level=p['phi'].shape[1],
                     alpha_prior_params=np.array([p['s1'], p['s2']]), device=dev,
                     initial_values=dict(x_mean=p['mu'], x_var=p['s'], x_u=p['z'], phi_logits=np.log(p['phi']),
                                         gamma_atoms=p['gamma_atoms'], alpha_atoms=p['alpha_atoms'], beta_atoms=p['beta_atoms'],
                                         gamma_1=p['g1'], gamma_2=p['g2'], w_1=p['w1'], w_2=p['w2']), **kw)


@pytest.mark.parametrize('case', MODEL_CASES, ids=case_id)
def test_model_gradients_across_y_scales(dev, case):
    """gradients() with precision='mixed' and with precision='f64', backward_precision='mixed' against precision='f64', per column of
    every raw variable; and model.objective against the objective terms the gradient evaluation computed on the way."""
    from dp_gp_lvm_amd.utils.synthetic import make_problem
    axis, v = case
    p = make_problem(2)
    y = p['y'] * (v if axis == 'y' else np.logspace(-4.0, 5.0, p['y'].shape[1])[None, :])
    ref_model = _model(p, y, dev, precision='f64')
    ref = {k: npy(g).copy() for k, g in ref_model.gradients().items()}
    for kw in (dict(precision='mixed'), dict(precision='f64', backward_precision='mixed')):
        what = ', '.join('%s=%s' % i for i in kw.items())
        mdl = _model(p, y, dev, **kw)
        got = mdl.gradients()
        grad_terms, info = (npy(a).copy() for a in mdl.per_dimension_terms)
        assert (info <= 0).all()
        flagged = np.flatnonzero(info == -2).tolist()
        obj = float(mdl.objective)
        assert np.isfinite(obj)
        fwd_terms = npy(mdl.per_dimension_terms[0])
        check_rows(grad_terms, fwd_terms, TERM_TOL, '%s: terms of gradients() against model.objective' % what)
        if kw['precision'] == 'f64' and not flagged:
            assert mdl.last_stage_b_form in ('mixed', 'mixed_patch')
        for k in RAW_NAMES:
            check_cols(npy(got[k]).reshape(ref[k].shape[0], -1), ref[k].reshape(ref[k].shape[0], -1), GRAD_TOL, '%s: %s' % (what, k))
