"""GPU tests of the over-T gradient path — dpgp_model_prepare_t, _fhat_forward(for_backward=True), the hand-written adjoints of
_fhat_backward, stage B with a full Psi1 adjoint and dpgp_model_backward_t — that dp_gp_lvm_t, bayesian_gp_lvm and
manifold_relevance_determination share, against the pinned fp64 autograd oracles (oracle/dpgp_oracle_torch.py:
objective_t_and_gradients, objective_bgplvm_and_gradients, objective_mrd_and_gradients; tests/test_oracle_grad.py pins them to the
reference) at random raw variables and at shapes off the reference fixtures: M a multiple of 128 (the persistent triangular
inverse), M > 128 (the composed forward), N > 256, Q past the pair-tile limit of stage B, T = D, D >= 64, y far from unit scale.

Tolerances by where a gradient is computed:
  objective                                     f64: 1e-10 relative, mixed: 2e-6
  x_mean, x_var, x_u (per latent dim),          5e-4 of each column's (gamma_atoms: each atom row's) largest entry: they pass
  gamma_atoms (per atom row)                    through stage B, which runs in mixed precision for either model precision
  alpha_atoms, beta_atoms, dp_*                 f64: 1e-8 of the array's largest entry (formed in fp64 from the forward's
                                                statistics, never in stage B); mixed: 5e-4
Then the HIP-graph replay of the gradients and of optimise() (bit for bit against the eager path) and optimise()'s trouble flag."""
import functools

import numpy as np
import pytest
import torch

from oracle import dpgp_oracle_torch as ot

pytestmark = pytest.mark.gpu
OBJ_RTOL = dict(f64=1e-10, mixed=2e-6)
STAGE_B_TOL = 5e-4
F64_PART_TOL = dict(f64=1e-8, mixed=5e-4)
REF2RAW = dict(x_mean='x_mean', x_var_raw='x_var', x_u='x_u', dp_logits='dp_logits', gamma_1_raw='dp_gamma_1',
               gamma_2_raw='dp_gamma_2', gamma_atoms_raw='gamma_atoms', alpha_atoms_raw='alpha_atoms', beta_atoms_raw='beta_atoms')


def softplus(x):
    return np.logaddexp(0.0, x)


def _rel(err, scale):
    return float((err / np.where(scale > 0, scale, 1.0)).max()) if np.size(err) else 0.0


def check_cols(got, want, tol, what):
    """|got - want| <= tol * max |want[:, j]| for every column j; returns the largest error relative to its column's scale."""
    got, want = np.asarray(got), np.asarray(want)
    assert np.isfinite(got).all(), '%s: non-finite entries' % what
    scale, err = np.abs(want).max(axis=0), np.abs(got - want).max(axis=0)
    bad = err > tol * scale
    assert not bad.any(), '%s: columns %s off by %s of their largest entry (tolerance %g)' % (
        what, np.flatnonzero(bad).tolist(), (err / np.where(scale > 0, scale, 1.0))[bad].tolist(), tol)
    return _rel(err, scale)


def check_array(got, want, tol, what):
    """|got - want| <= tol * max |want| over the whole array."""
    got, want = np.asarray(got), np.asarray(want)
    assert np.isfinite(got).all(), '%s: non-finite entries' % what
    scale, err = np.abs(want).max(), np.abs(got - want).max()
    assert err <= tol * scale, '%s: off by %g of its largest entry %g (tolerance %g)' % (what, err / max(scale, 1e-300), scale, tol)
    return _rel(err, scale)


def check_gradient(name, got, want, prec, cls):
    """cls 'cols': per latent dim; 'rows': per atom row; 'f64': the array's largest entry at the fp64 / mixed tolerance."""
    got = np.asarray(got).reshape(-1)[:want.size].reshape(want.shape)
    if cls == 'cols':
        return check_cols(got.reshape(want.shape[0], -1), want.reshape(want.shape[0], -1), STAGE_B_TOL, name)
    if cls == 'rows':
        return check_cols(got.T, want.T, STAGE_B_TOL, name)
    return check_array(got, want, F64_PART_TOL[prec], name)


def gradient_class(raw_name):
    if raw_name in ('x_mean', 'x_var') or raw_name.startswith('x_u'):
        return 'cols'
    return 'rows' if raw_name.startswith('gamma_atoms') else 'f64'


def _y(rng, n, d, y_scale):
    y = rng.standard_normal((n, d))
    y = (y - y.mean(0)) / y.std(0)
    if y_scale == 'col':
        y[:, 0] *= 1e5
    else:
        y *= y_scale
    return y


# ---- dp_gp_lvm_t -----------------------------------------------------------------------------------------------------------
# (N, D, M, Q, T, mask_size): M off the tiles, M = 64 / 128 / 256 (the persistent triangular inverse), M > 128 (composed forward,
# stage B's M > 128 path), N = 257 / 513 (more than one workgroup of psi1_grad_n_kernel), Q = 20 / 21 (last pair-tile shapes) / 22 /
# 30 (patch form), T = 1, T = D, M = N, D = 70
T_SHAPES = [(33, 5, 17, 4, 1, 1), (70, 9, 33, 8, 3, 3), (257, 12, 64, 5, 4, 1), (200, 8, 65, 7, 2, 1), (160, 30, 128, 20, 5, 1),
            (90, 24, 40, 21, 3, 1), (90, 24, 40, 22, 3, 1), (120, 40, 24, 30, 3, 1), (200, 12, 129, 8, 3, 1),
            (300, 9, 256, 5, 2, 1), (40, 6, 40, 3, 6, 1), (513, 70, 100, 10, 8, 1)]
Y_SCALE_SHAPE = (120, 10, 40, 5, 3, 1)


def _t_raw(shape, y_scale=1.0):
    n, d, m, q, t, mask = shape
    rng = np.random.default_rng(n + d + 100 * q)
    y = _y(rng, n, d, y_scale)
    # M > 128: the inducing inputs spread over four length scales, so that K_uu stays well conditioned (as test_gpu_grad.py's
    # odd shapes); over two where more than ten of them crowd each latent dim (M = N = 40 in Q = 3: cond(K_uu) 9e5 at unit scale)
    zs = 4.0 if m > 128 else (2.0 if m > 10 * q else 1.0)
    raw = dict(x_mean=rng.standard_normal((n, q)), x_var_raw=0.3 * rng.standard_normal((n, q)),
               x_u=zs * rng.standard_normal((m, q)), dp_logits=rng.standard_normal((d // mask, t)),
               gamma_1_raw=rng.standard_normal(max(t - 1, 0)), gamma_2_raw=rng.standard_normal(max(t - 1, 0)),
               w_1_raw=np.array(0.4), w_2_raw=np.array(0.7), gamma_atoms_raw=0.5 * rng.standard_normal((t, q)),
               alpha_atoms_raw=0.5 * rng.standard_normal((t, 1)), beta_atoms_raw=0.5 * rng.standard_normal((t, 1)) + 1.0)
    if y_scale in (1e5, 'col'):
        # the noise precision where such data puts it, beta ~ 1 / var(y) (one column at 1e5: in between): at unit-scale beta the
        # mixed forward's conditioning guard (its bound grows with beta y^2) flags every atom
        raw['beta_atoms_raw'] = np.log(np.expm1(softplus(raw['beta_atoms_raw']) * (1e-10 if y_scale == 1e5 else 1e-5)))
    return y, raw


@functools.lru_cache(maxsize=None)
def _t_oracle(shape, y_scale=1.0):
    y, raw = _t_raw(shape, y_scale)
    return ot.objective_t_and_gradients(y, raw, s_1=1.0, s_2=1.0, mask_size=shape[5])


def build_t(dev, shape, prec, y_scale=1.0):
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm_t
    n, d, m, q, t, mask = shape
    y, raw = _t_raw(shape, y_scale)
    sp = softplus
    return dp_gp_lvm_t(y, num_latent_dims=q, num_inducing_points=m, truncation_level=t, alpha_prior_params=np.array([1.0, 1.0]),
                       mask_size=mask, device=dev, precision=prec,
                       initial_values=dict(x_mean=raw['x_mean'], x_var=sp(raw['x_var_raw']), x_u=raw['x_u'],
                                           phi_logits=raw['dp_logits'], gamma_atoms=sp(raw['gamma_atoms_raw']),
                                           alpha_atoms=sp(raw['alpha_atoms_raw']), beta_atoms=sp(raw['beta_atoms_raw']),
                                           gamma_1=sp(raw['gamma_1_raw']), gamma_2=sp(raw['gamma_2_raw']),
                                           w_1=float(sp(raw['w_1_raw'])), w_2=float(sp(raw['w_2_raw']))))


def _check_t(dev, shape, prec, record_property, y_scale=1.0):
    obj, ref = _t_oracle(shape, y_scale)
    model = build_t(dev, shape, prec, y_scale)
    assert int(model.cholesky_info) == 0
    got_obj = float(model.objective)
    np.testing.assert_allclose(got_obj, obj, rtol=OBJ_RTOL[prec])
    got = model.gradients()
    worst = dict(objective=abs(got_obj - obj) / abs(obj), stage_b=0.0, f64_part=0.0)
    for ref_name, raw_name in REF2RAW.items():
        want = ref[ref_name]
        if want.size == 0:
            continue
        cls = gradient_class(raw_name)
        e = check_gradient('%s (%s, %s)' % (raw_name, prec, shape), got[raw_name].cpu().numpy(), want, prec, cls)
        key = 'f64_part' if cls == 'f64' else 'stage_b'
        worst[key] = max(worst[key], e)
    w_ref = np.array([float(ref['w_1_raw']), float(ref['w_2_raw'])])
    worst['f64_part'] = max(worst['f64_part'], check_array(got['dp_w'].cpu().numpy(), w_ref, F64_PART_TOL[prec], 'dp_w'))
    for k, v in worst.items():
        record_property(k, v)


@pytest.mark.parametrize('prec', ['f64', 'mixed'])
@pytest.mark.parametrize('shape', T_SHAPES, ids=lambda s: 'N%d_D%d_M%d_Q%d_T%d_mask%d' % s)
def test_over_t_gradients_odd_shapes(dev, shape, prec, record_property):
    _check_t(dev, shape, prec, record_property)


@pytest.mark.parametrize('prec', ['f64', 'mixed'])
@pytest.mark.parametrize('y_scale', [1e-4, 1e5, 'col'], ids=['y1e-4', 'y1e5', 'ycol1e5'])
def test_over_t_gradients_far_from_unit_scale(dev, y_scale, prec, record_property):
    """y times 1e-4, times 1e5, and one column at 1e5 (the others at unit scale)."""
    _check_t(dev, Y_SCALE_SHAPE, prec, record_property, y_scale)


# ---- bayesian_gp_lvm ---------------------------------------------------------------------------------------------------------
# (N, D, M, Q): the M > 128 shape of the predb1_bgplvm_150_12_136_8 fixture, D = 64 with Q = 24 (patch form) at M = 128, M = N - 1
B_SHAPES = [(60, 7, 17, 3), (300, 40, 136, 8), (257, 64, 128, 24), (48, 8, 47, 5)]


def _b_raw(shape):
    n, d, m, q = shape
    rng = np.random.default_rng(7 * n + d + m)
    y = _y(rng, n, d, 1.0)
    raw = dict(x_mean=rng.standard_normal((n, q)), x_var_raw=0.3 * rng.standard_normal((n, q)) - 0.5,
               x_u=(4.0 if m > 128 else 1.5) * rng.standard_normal((m, q)), gamma_raw=0.5 * rng.standard_normal((1, q)),
               alpha_raw=0.5 * rng.standard_normal((1, 1)), beta_raw=0.5 * rng.standard_normal((1, 1)) + 1.0)
    return y, raw


@functools.lru_cache(maxsize=None)
def _b_oracle(shape):
    return ot.objective_bgplvm_and_gradients(*_b_raw(shape))


def build_b(dev, shape, prec):
    from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm
    n, d, m, q = shape
    y, raw = _b_raw(shape)
    sp = softplus
    return bayesian_gp_lvm(y, num_latent_dims=q, num_inducing_points=m, device=dev, precision=prec,
                           initial_values=dict(x_mean=raw['x_mean'], x_var=sp(raw['x_var_raw']), x_u=raw['x_u'],
                                               gamma=sp(raw['gamma_raw']), alpha=sp(raw['alpha_raw']), beta=sp(raw['beta_raw'])))


@pytest.mark.parametrize('prec', ['f64', 'mixed'])
@pytest.mark.parametrize('shape', B_SHAPES, ids=lambda s: 'N%d_D%d_M%d_Q%d' % s)
def test_bgplvm_gradients_odd_shapes(dev, shape, prec, record_property):
    obj, ref = _b_oracle(shape)
    model = build_b(dev, shape, prec)
    got_obj = float(model.objective)
    np.testing.assert_allclose(got_obj, obj, rtol=OBJ_RTOL[prec])
    got = model.gradients()
    worst = dict(objective=abs(got_obj - obj) / abs(obj), stage_b=0.0, f64_part=0.0)
    for ref_name, raw_name in dict(x_mean='x_mean', x_var_raw='x_var', x_u='x_u', gamma_raw='gamma_atoms', alpha_raw='alpha_atoms',
                                   beta_raw='beta_atoms').items():
        cls = gradient_class(raw_name)
        e = check_gradient('%s (%s, %s)' % (raw_name, prec, shape), got[raw_name].cpu().numpy(), ref[ref_name], prec, cls)
        key = 'f64_part' if cls == 'f64' else 'stage_b'
        worst[key] = max(worst[key], e)
    for k, v in worst.items():
        record_property(k, v)


def test_bgplvm_optimise_raises_on_a_non_finite_gradient(dev):
    """optimise() steps Adam only on finite gradients of a successful factorisation (as dp_gp_lvm_t's and MRD's): a NaN inducing
    input raises FloatingPointError and leaves the raw variables as they were."""
    model = build_b(dev, B_SHAPES[0], 'mixed')
    model.optimise(2, learning_rate=0.01)
    raw = model.raw_variables
    raw['x_u'][0, 0] = float('nan')
    before = {k: v.detach().cpu().numpy().copy() for k, v in raw.items()}
    with pytest.raises(FloatingPointError, match='iteration 0'):
        model.optimise(3, learning_rate=0.01)
    for k, v in raw.items():
        np.testing.assert_array_equal(v.detach().cpu().numpy(), before[k], err_msg=k)


# ---- manifold_relevance_determination ----------------------------------------------------------------------------------------
# (N, M, Q, view widths): views narrower than Q (_view_of_many), five views, two views at M = 130
MRD_CASES = [(80, 20, 4, (1, 2, 9)), (90, 25, 5, (3, 5, 2, 7, 4)), (200, 130, 6, (6, 10))]


def _mrd_raw(case):
    n, m, q, widths = case
    rng = np.random.default_rng(n + m + sum(widths))
    views = [_y(rng, n, w, 1.0) for w in widths]
    raw = dict(x_mean=rng.standard_normal((n, q)), x_var_raw=0.3 * rng.standard_normal((n, q)))
    for i in range(len(widths)):
        raw['x_u_%d' % i] = (4.0 if m > 128 else 1.5) * rng.standard_normal((m, q))
        raw['gamma_raw_%d' % i] = 0.5 * rng.standard_normal((1, q))
        raw['alpha_raw_%d' % i] = 0.5 * rng.standard_normal((1, 1))
        raw['beta_raw_%d' % i] = 0.5 * rng.standard_normal((1, 1)) + 1.0
    return views, raw


@functools.lru_cache(maxsize=None)
def _mrd_oracle(case):
    return ot.objective_mrd_and_gradients(*_mrd_raw(case))


@pytest.mark.parametrize('prec', ['f64', 'mixed'])
@pytest.mark.parametrize('case', MRD_CASES, ids=lambda c: 'N%d_M%d_Q%d_views%s' % (c[0], c[1], c[2], '-'.join(map(str, c[3]))))
def test_mrd_gradients_odd_shapes(dev, case, prec, record_property):
    from dp_gp_lvm_amd.models.gaussian_process import manifold_relevance_determination
    n, m, q, widths = case
    views, raw = _mrd_raw(case)
    nv, sp = len(views), softplus
    iv = dict(x_mean=raw['x_mean'], x_var=sp(raw['x_var_raw']), x_u=[raw['x_u_%d' % i] for i in range(nv)],
              gamma=[sp(raw['gamma_raw_%d' % i]) for i in range(nv)], alpha=[sp(raw['alpha_raw_%d' % i]) for i in range(nv)],
              beta=[sp(raw['beta_raw_%d' % i]) for i in range(nv)])
    model = manifold_relevance_determination(views, num_latent_dims=q, num_inducing_points=m, device=dev, precision=prec,
                                             initial_values=iv)
    obj, ref = _mrd_oracle(case)
    got_obj = float(model.objective)
    np.testing.assert_allclose(got_obj, obj, rtol=OBJ_RTOL[prec])
    got = model.gradients()
    worst = dict(objective=abs(got_obj - obj) / abs(obj), stage_b=0.0, f64_part=0.0)
    ref2raw = dict(x_mean='x_mean', x_var_raw='x_var')
    for i in range(nv):
        ref2raw.update({'gamma_raw_%d' % i: 'gamma_atoms_%d' % i, 'alpha_raw_%d' % i: 'alpha_atoms_%d' % i,
                        'beta_raw_%d' % i: 'beta_atoms_%d' % i, 'x_u_%d' % i: 'x_u_%d' % i})
    for ref_name, raw_name in ref2raw.items():
        cls = gradient_class(raw_name)
        e = check_gradient('%s (%s, %s)' % (raw_name, prec, case), got[raw_name].cpu().numpy(), ref[ref_name], prec, cls)
        key = 'f64_part' if cls == 'f64' else 'stage_b'
        worst[key] = max(worst[key], e)
    for k, v in worst.items():
        record_property(k, v)


# ---- HIP-graph replay and optimise()'s trouble flag (dp_gp_lvm_t) --------------------------------------------------------------
GRAPH_SHAPES = [(120, 10, 40, 5, 3, 1), (200, 12, 129, 8, 3, 1)]


def _host(g):
    return {k: v.cpu().numpy().copy() for k, v in g.items()}


@pytest.mark.parametrize('prec', ['f64', 'mixed'])
@pytest.mark.parametrize('shape', GRAPH_SHAPES, ids=lambda s: 'N%d_D%d_M%d_Q%d_T%d_mask%d' % s)
def test_graph_replay_equals_the_eager_gradients(dev, shape, prec):
    """gradients(graph=True) against gradients(), bit for bit, before and after an in-place update of every raw variable (the graph
    reads them in place; the library's gradient kernels add their partial sums in a fixed order, no floating-point atomics)."""
    model = build_t(dev, shape, prec)
    for step in range(2):
        replay, eager = _host(model.gradients(graph=True)), _host(model.gradients())
        assert np.isfinite(np.concatenate([v.reshape(-1) for v in eager.values()])).all()
        for k in eager:
            np.testing.assert_array_equal(replay[k], eager[k], err_msg='%s (update %d)' % (k, step))
        with torch.no_grad():
            for k, v in model.raw.items():
                v.add_(0.01 * torch.linspace(-1.0, 1.0, v.numel(), dtype=v.dtype, device=v.device).reshape(v.shape))


def test_optimise_from_the_graph_follows_the_eager_trajectory(dev, monkeypatch):
    """optimise(k) replays the captured gradient evaluation; with DPGP_GRAPH_T=0 it runs eagerly: the same raw variables after every
    iteration, bit for bit."""
    shape = GRAPH_SHAPES[0]
    traj = {}
    for mode in ('1', '0'):
        monkeypatch.setenv('DPGP_GRAPH_T', mode)
        model = build_t(dev, shape, 'mixed')
        traj[mode] = []
        model.optimise(6, learning_rate=0.02,
                       callback=lambda it: traj[mode].append(torch.cat([v.detach().reshape(-1) for v in model.raw.values()]).cpu()))
    assert len(traj['1']) == len(traj['0']) == 6
    for it, (a, b) in enumerate(zip(traj['1'], traj['0'])):
        np.testing.assert_array_equal(a.numpy(), b.numpy(), err_msg='iteration %d' % it)
    assert not np.array_equal(traj['1'][0].numpy(), traj['1'][-1].numpy())


def test_optimise_raises_on_a_nan_after_the_graph_is_captured(dev):
    """A NaN written into x_u after the graph has been captured: the replayed step flags it, optimise() raises FloatingPointError at
    that iteration and does not step (NaN arithmetic, not a fault: test_fp64_psi_kernels_propagate_nan)."""
    model = build_t(dev, GRAPH_SHAPES[0], 'mixed')
    snap = {}

    def inject(it):
        if it == 1:
            with torch.no_grad():
                model.raw['x_u'][2, 1] = float('nan')
            snap.update({k: v.detach().cpu().numpy().copy() for k, v in model.raw.items()})
    with pytest.raises(FloatingPointError, match='iteration 2'):
        model.optimise(5, learning_rate=0.01, callback=inject)
    for k, v in model.raw.items():
        np.testing.assert_array_equal(v.detach().cpu().numpy(), snap[k], err_msg=k)
