"""
TEST INFRASTRUCTURE, CONTAINER-ONLY: fixtures for ``gp_regression`` and ``gp_lvm`` (reference
src/models/gaussian_process.py:22-129).  Run as ``python tools/gen_golden_gp.py`` where the reference checkout that
``oracle/gen_golden_grad.py`` links is present; it never runs on the GPU box.

Runs the reference's own, unmodified ``gp_regression`` / ``gp_lvm`` under the PyTorch stand-in for TensorFlow with steered
initial values (as oracle/gen_golden_mrd.py: 0.25 N(0, 1) added to every trainable variable's initial value) and records
    inputs, raw variables (creation order: gp_lvm's latent X [N,Q], then gamma_raw [1,Q], alpha_raw [1,1], beta_raw [1,1]),
    objective, log_likelihood [D], tf.gradients of the objective with respect to the trainables, and
    predict_mean_covar at a test set.
The stand-ins lack TensorFlow's ``Tensor.get_shape`` (the reference reads shapes with it): it is added here at run time,
to torch tensors and to an ndarray subclass for the NumPy stand-in; gp_lvm's y_train is such a tensor, so the PCA it
starts from (which asserts an ndarray) is handed its array.
Checks before writing: the NumPy stand-in at the same variable values (objective, log-likelihood and prediction, 1e-11)
and central differences of its objective along random directions.
"""
import importlib
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
import numpy as np                                                           # noqa: E402
import torch                                                                 # noqa: E402
from oracle import gen_golden_grad as gg                                     # noqa: E402

ORACLE = os.path.join(REPO, 'oracle')
# name: (kind, N, Q, D, N_test, seed).  N <= 128: the LDS Cholesky; 150, 130: potrf_big and the identity-solve inverse;
# 256: the trtri inverse.
CASES = {
    'gpr_ref_40_3_1': ('gpr', 40, 3, 1, 7, 61),
    'gpr_ref_150_4_5': ('gpr', 150, 4, 5, 9, 62),
    'gpr_ref_256_2_3': ('gpr', 256, 2, 3, 5, 63),
    'gplvm_ref_60_8_3': ('gplvm', 60, 3, 8, 6, 64),
    'gplvm_ref_130_12_4': ('gplvm', 130, 4, 12, 8, 65),
}


class _Shape(tuple):
    def as_list(self):
        return list(self)


class _Shaped(np.ndarray):
    def get_shape(self):
        return _Shape(self.shape)


torch.Tensor.get_shape = lambda self: _Shape(self.shape)


def data(case):
    kind, n, q, d, ns, seed = case
    rng = np.random.default_rng(seed)
    if kind == 'gpr':
        x = rng.uniform(-2.0, 2.0, (n, q))
        w = rng.standard_normal((q, d))
        y = np.sin(x @ w) + 0.1 * rng.standard_normal((n, d))
        xs = rng.uniform(-2.5, 2.5, (ns, q))
    else:
        t = rng.standard_normal((n, 2))
        y = np.tanh(t) @ rng.standard_normal((2, d)) + 0.3 * rng.standard_normal((n, d))
        y = (y - y.mean(axis=0)) / y.std(axis=0)
        x = None
        xs = rng.standard_normal((ns, q))
    return x, y, xs


def build(backend, case, overrides=None):
    for k in [k for k in sys.modules if k == 'tensorflow' or k.startswith('tensorflow.') or k == 'tensorflow_probability'
              or k == 'src' or k.startswith('src.')]:
        del sys.modules[k]
    sys.path[:] = [p for p in sys.path if os.path.basename(p) not in ('standin', 'standin_torch')]
    sys.path[:0] = [os.path.join(ORACLE, backend), gg.LINK]
    tf = importlib.import_module('tensorflow')
    assert backend in tf.__file__
    gpm = importlib.import_module('src.models.gaussian_process')
    kind, n, q, d, ns, seed = case
    x, y, xs = data(case)
    pert = np.random.default_rng(seed + 1000)
    tf.reset_default_graph()
    np.random.seed(seed)
    it = iter(overrides) if overrides is not None else None
    real_variable = tf.Variable
    wrap = (lambda v: v) if backend == 'standin_torch' else (lambda v: v.view(_Shaped))

    def steered_variable(initial_value=None, dtype=None, trainable=True, **kw):
        if trainable:
            init = np.asarray(initial_value, dtype=np.float64)
            initial_value = next(it) if it is not None else init + 0.25 * pert.standard_normal(init.shape)
        return wrap(real_variable(np.asarray(initial_value), dtype=dtype, trainable=trainable, **kw))
    tf.Variable = steered_variable
    try:
        if kind == 'gpr':
            model = gpm.gp_regression(x_train=wrap(tf.constant(x)), y_train=wrap(tf.constant(y)))
        else:
            pca = gpm.pca
            gpm.pca = lambda a, **kw: pca(np.asarray(a.detach() if isinstance(a, torch.Tensor) else a).view(np.ndarray), **kw)
            try:
                model = gpm.gp_lvm(y_train=wrap(tf.constant(y)), num_latent_dims=q)
            finally:
                gpm.pca = pca
    finally:
        tf.Variable = real_variable
    variables = tf.get_collection(tf.GraphKeys.TRAINABLE_VARIABLES)
    return tf, model, variables, (x, y, wrap(tf.constant(xs)))


def _np(t):
    return np.asarray(t.detach().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64)


def evaluate(backend, case, overrides=None):
    tf, model, variables, (x, y, xs) = build(backend, case, overrides)
    mean, covar = model.predict_mean_covar(xs)
    return tf, model, variables, float(_np(model.objective)), _np(model.log_likelihood), _np(mean), _np(covar), (x, y, xs)


def main():
    for name, case in CASES.items():
        kind = case[0]
        tf, model, variables, obj, ll, mean, covar, (x, y, xs) = evaluate('standin_torch', case)
        names = (['x_latent'] if kind == 'gplvm' else []) + ['gamma_raw', 'alpha_raw', 'beta_raw']
        assert len(variables) == len(names), (len(variables), names)
        grads = tf.gradients(model.objective, variables)
        vals = [v.detach().numpy().copy() for v in variables]
        g = [np.zeros_like(v) if gi is None else gi.detach().numpy().copy() for v, gi in zip(vals, grads)]
        # (1) the NumPy stand-in at the same values
        _, _, _, o2, ll2, m2, c2, _ = evaluate('standin', case, overrides=vals)
        np.testing.assert_allclose(o2, obj, rtol=1e-11)
        np.testing.assert_allclose(ll2, ll, rtol=1e-11)
        np.testing.assert_allclose(m2, mean, rtol=1e-11, atol=1e-11 * np.abs(mean).max())
        np.testing.assert_allclose(c2, covar, rtol=1e-11, atol=1e-11 * np.abs(covar).max())
        # (2) central differences of the NumPy objective
        rs = np.random.default_rng(5)
        for _ in range(4):
            dirs = [rs.standard_normal(v.shape) for v in vals]
            h = 1e-5
            fd = (evaluate('standin', case, [v + h * e for v, e in zip(vals, dirs)])[3] -
                  evaluate('standin', case, [v - h * e for v, e in zip(vals, dirs)])[3]) / (2 * h)
            an = sum(float(np.sum(gi * e)) for gi, e in zip(g, dirs))
            assert abs(fd - an) <= 2e-6 * max(1.0, abs(an)), (name, fd, an)
        extra = {} if x is None else {'x': x}
        np.savez_compressed(os.path.join(gg.OUT, name + '.npz'), kind=kind, y=y, x_test=_np(xs), objective=obj,
                            log_likelihood=ll, pred_mean=mean, pred_covar=covar, **extra, **dict(zip(names, vals)),
                            **{'grad_' + k: gi for k, gi in zip(names, g)})
        print('wrote %s: objective %.12f' % (name, obj))


if __name__ == '__main__':
    main()
