"""
TEST INFRASTRUCTURE, CONTAINER-ONLY: fixtures for the prediction paths of ``bayesian_gp_lvm`` and
``manifold_relevance_determination`` (reference src/models/gaussian_process.py:329-538, :729-990).  Run as
``python tools/gen_golden_predict_b1.py`` where the reference checkout that ``oracle/gen_golden_grad.py`` links is present; it
never runs on the GPU box.

Builds the reference's own models under the PyTorch stand-in for TensorFlow with the steered trainable variables of
oracle/gen_golden_bgplvm.py / oracle/gen_golden_mrd.py, then calls the reference's own ``predict_new_latent_variables`` and
``predict_missing_data``.  The two NON-trainable variables those methods create (x_test_mean [N*,Q], then the raw test
variances [N*,Q]: gaussian_process.py:362-365) are steered to stored values, so no random draw matters, and are made
differentiable: ``tf.gradients`` of each bound with respect to them gives the gradient with respect to q(X*) (the variances'
through the softplus).  Recorded per method: the bound, the test log-likelihood (bgplvm), the predicted means and covariances
(missing data), and the two gradients.
MRD's predicted means use the last training view's C for every unobserved view (gaussian_process.py:938; ``c`` is left over
from the training loop).  The fixtures store the reference's numbers (``*_compat``) and, for MRD, the means with each view's own
C, computed here from the same stand-in tensors by the reference's formula (:935-939) with ``c`` replaced.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
import numpy as np                                                           # noqa: E402
import torch                                                                 # noqa: E402
from oracle import gen_golden_bgplvm as gb                                   # noqa: E402
from oracle import gen_golden_mrd as gm                                      # noqa: E402
from oracle import gen_golden_grad as gg                                     # noqa: E402

# name: (kind, case, N*, observed dims (bgplvm) or views (MRD), seed of q(X*))
CASES = {
    'predb1_bgplvm_40_6_12_3': ('bgplvm', (40, 6, 12, 3, 71), 1, 4, 81),
    'predb1_bgplvm_70_9_20_4': ('bgplvm', (70, 9, 20, 4, 72), 9, 5, 82),
    'predb1_bgplvm_150_12_136_8': ('bgplvm', (150, 12, 136, 8, 73), 4, 7, 83),
    'predb1_mrd_50_2views_12_3': ('mrd', (50, (5, 7), 12, 3, 74), 6, 1, 84),
    'predb1_mrd_60_4views_15_4': ('mrd', (60, (4, 6, 5, 3), 15, 4, 75), 5, 2, 85),
}


def _np(t):
    return np.asarray(t.detach().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64)


def call_steered(tf, fn, arg, xm, xv):
    """fn(arg) with the method's two non-trainable variables set to (xm, inverse softplus of xv), differentiable."""
    made = []
    real_variable = tf.Variable
    vals = iter([xm, np.log(np.expm1(xv))])

    def steered(initial_value=None, dtype=None, trainable=True, **kw):
        if not trainable:
            v = torch.as_tensor(np.asarray(next(vals), dtype=np.float64)).clone().requires_grad_(True)
            made.append(v)
            return v
        return real_variable(initial_value, dtype=dtype, trainable=trainable, **kw)
    real_map_fn = tf.map_fn
    tf.Variable = steered
    # (the nearest-neighbour initial value is replaced by the steered one; detached, it can be added to its NumPy noise)
    tf.map_fn = lambda *a, **k: real_map_fn(*a, **k).detach().numpy()
    try:
        out = fn(arg)
    finally:
        tf.Variable, tf.map_fn = real_variable, real_map_fn
    assert len(made) == 2, len(made)
    g_mu, g_raw = torch.autograd.grad(out[0], made, retain_graph=True)
    return out, _np(g_mu), _np(g_raw) / _np(torch.sigmoid(made[1]))


def main():
    for name, (kind, case, n_t, n_obs, seed) in CASES.items():
        rng = np.random.default_rng(seed)
        rec = {}
        if kind == 'bgplvm':
            tf, model, variables, y = gb.build('standin_torch', case)
            vals = [v.detach().numpy().copy() for v in variables]
            rec.update(y=y, **dict(zip(gb.NAMES, vals)))
            y_test = y[rng.choice(y.shape[0], n_t, replace=False)] + 0.1 * rng.standard_normal((n_t, y.shape[1]))
            data_new, data_mis = y_test, y_test[:, :n_obs]
        else:
            tf, model, variables, views = gm.build('standin_torch', case)
            names = __import__('oracle.dpgp_oracle_torch', fromlist=['mrd_names']).mrd_names(len(views))
            vals = [v.detach().numpy().copy() for v in variables]
            rec.update(num_views=len(views), **{'view_%d' % i: v for i, v in enumerate(views)}, **dict(zip(names, vals)))
            rows = rng.choice(views[0].shape[0], n_t, replace=False)
            views_test = [v[rows] + 0.1 * rng.standard_normal((n_t, v.shape[1])) for v in views]
            rec.update({'test_view_%d' % i: v for i, v in enumerate(views_test)})
            data_new, data_mis = views_test, views_test[:n_obs]
        q = case[3]
        xm = rng.standard_normal((n_t, q))
        xv = rng.uniform(0.2, 1.5, (n_t, q))
        rec.update(y_test=data_new if kind == 'bgplvm' else np.zeros(0), n_observed=n_obs, x_test_mean=xm, x_test_var=xv)
        out, gmu, gs = call_steered(tf, model.predict_new_latent_variables, data_new, xm, xv)
        rec.update(new_lower_bound=float(_np(out[0])), new_grad_mean=gmu, new_grad_var=gs)
        np.testing.assert_allclose(_np(out[1]), xm, rtol=1e-15)
        if kind == 'bgplvm':
            rec.update(new_test_log_likelihood=float(_np(out[3])))
        out, gmu, gs = call_steered(tf, model.predict_missing_data, data_mis, xm, xv)
        rec.update(missing_lower_bound=float(_np(out[0])), missing_grad_mean=gmu, missing_grad_var=gs)
        if kind == 'bgplvm':
            rec.update(predicted_mean=_np(out[3]), predicted_covar=_np(out[4]))
        else:
            nu = len(out[3])
            rec.update({'predicted_mean_compat_%d' % i: _np(out[3][i]) for i in range(nu)})
            rec.update({'predicted_covar_%d' % i: _np(out[4][i]) for i in range(nu)})
            rec.update({'predicted_mean_%d' % i: own_c_mean(model, views, n_obs + i, out[1], out[2]) for i in range(nu)})
        np.savez_compressed(os.path.join(gg.OUT, name + '.npz'), kind=kind, **rec)
        print('wrote %s: bounds %.10f / %.10f' % (name, rec['new_lower_bound'], rec['missing_lower_bound']))


def own_c_mean(model, views, v, x_test_mean, x_test_covar):
    """The reference's predicted mean of view v (gaussian_process.py:929-939) with view v's own training C in place of the
    leaked last-view C: beta_v (L_A_v^-1 L_v^-1 Psi1*_v^T)^T (L_A_v^-1 L_v^-1 Psi1_v^T) Y_v, restated in torch."""
    kern, z = model.kernels[v], model.inducing_input[v]
    mu, cov = model.q_x
    with torch.no_grad():
        psi1 = kern.psi_1(inducing_input=z, latent_input_mean=mu, latent_input_covariance=cov)[0]
        psi2 = kern.psi_2(inducing_input=z, latent_input_mean=mu, latent_input_covariance=cov)[0]
        psi1t = kern.psi_1(inducing_input=z, latent_input_mean=x_test_mean, latent_input_covariance=x_test_covar)[0]
        k_uu = kern.covariance_matrix(input_0=z, input_1=None, include_noise=False, include_jitter=True)[0]
        beta = kern.noise_precision.reshape(-1)[0]
        l_uu = torch.linalg.cholesky(k_uu)
        li = torch.linalg.solve_triangular(l_uu, torch.eye(l_uu.shape[0], dtype=l_uu.dtype), upper=False)
        a = beta * li @ psi2 @ li.T + torch.eye(l_uu.shape[0], dtype=l_uu.dtype)
        l_a = torch.linalg.cholesky(a)
        c = torch.linalg.solve_triangular(l_a, li @ psi1.T, upper=False)
        c_pred = torch.linalg.solve_triangular(l_a, li @ psi1t.T, upper=False)
        return _np(beta * (c_pred.T @ c) @ torch.as_tensor(views[v]))


if __name__ == '__main__':
    main()
