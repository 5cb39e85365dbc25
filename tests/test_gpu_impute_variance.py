"""GPU tests of impute_training_data(return_variance=True) on the mask-trained bayesian_gp_lvm, manifold_relevance_determination and
dp_gp_lvm_t: the filled data are bit-equal to the plain call's, the variance is 0 at the observed entries and, at the unobserved
ones, the per-entry predictive variance at the training q(X) (the NumPy restatement of test_gpu_predict_t.moments_numpy, 1e-9),
never below the observation noise 1/beta."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_gpu_mrd_masked import build as build_mrd_masked
from test_gpu_predict_b1 import close, softplus
from test_gpu_predict_t import build_t, moments_numpy, values_of
from test_gpu_predictive_marginals import BGPLVM, MRD, mask, scalar, values_b, values_view
from test_gpu_train_masked import build_masked
from test_gpu_train_masked_t import FIXTURES as OVER_T

pytestmark = pytest.mark.gpu


def check(tag, model_out, plain, obs, want_var, beta_min):
    """model_out = (filled, var) of one data matrix; want_var [N x D] the restated variance at every entry."""
    filled, var = model_out
    assert torch.equal(filled, plain), tag + ': filled data differ from impute_training_data()'
    assert tuple(var.shape) == obs.shape
    o = torch.as_tensor(obs, device=var.device)
    assert torch.equal(var[o], torch.zeros_like(var[o])), tag + ': variance at observed entries'
    want = np.where(obs, 0.0, want_var)
    print('%s: max |err| %.3e of %.3e (bound 1e-9); smallest unobserved variance %.6e, 1/beta %.6e' %
          (tag, np.abs(var.cpu().numpy() - want).max(), np.abs(want).max(), float(var[~o].min()), 1.0 / beta_min))
    close(var, want, 1e-9, tag + ': variance')
    assert float(var[~o].min()) >= 1.0 / beta_min - 1e-9, tag + ': variance below the observation noise'


def test_bgplvm(dev):
    g = golden(BGPLVM)
    y = g['y']
    obs = mask(*y.shape, 17)
    model = build_masked(g, dev, obs, y=np.where(obs, y, np.nan))
    v = values_b(g)
    _, want = moments_numpy(v, np.where(obs, y, 0.0), obs, v['mu'].numpy(), v['s'].numpy(), list(range(y.shape[1])))
    check('bayesian_gp_lvm', model.impute_training_data(return_variance=True), model.impute_training_data(), obs, want,
          scalar(softplus(g['beta_raw'])))


def test_mrd_per_view(dev):
    g = golden(MRD)
    nv = int(g['num_views'])
    views = [g['view_%d' % v] for v in range(nv)]
    obs = [mask(*views[v].shape, 17 + v) for v in range(nv)]
    model = build_mrd_masked(g, dev, obs, views=[np.where(o, y, np.nan) for o, y in zip(obs, views)])
    plain = model.impute_training_data()
    filled, variances = model.impute_training_data(return_variance=True)
    assert len(filled) == len(variances) == nv
    for v in range(nv):
        vals = values_view(g, v)
        _, want = moments_numpy(vals, np.where(obs[v], views[v], 0.0), obs[v], vals['mu'].numpy(), vals['s'].numpy(),
                                list(range(views[v].shape[1])))
        check('view %d' % v, (filled[v], variances[v]), plain[v], obs[v], want, scalar(softplus(g['beta_raw_%d' % v])))


def test_over_t(dev):
    g = golden(OVER_T[0])
    model, obs = build_t(g, dev, 'odd')
    v = values_of(g)
    y = np.where(obs, g['y'], 0.0)
    _, want = moments_numpy(v, y, obs, v['mu'].numpy(), v['s'].numpy(), list(range(y.shape[1])))
    check('dp_gp_lvm_t', model.impute_training_data(return_variance=True), model.impute_training_data(), obs, want,
          float(v['bat'].max()))


def test_over_t_with_one_atom_equals_the_bgplvm(dev):
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm_t
    g = golden(BGPLVM)
    y = g['y']
    obs = mask(*y.shape, 17)
    y_nan = np.where(obs, y, np.nan)
    iv = dict(x_mean=g['x_mean'], x_var=softplus(g['x_var_raw']), x_u=g['x_u'], gamma_atoms=softplus(g['gamma_raw']),
              alpha_atoms=softplus(g['alpha_raw']), beta_atoms=softplus(g['beta_raw']))
    over_t = dp_gp_lvm_t(y_nan, num_latent_dims=g['x_mean'].shape[1], num_inducing_points=g['x_u'].shape[0], truncation_level=1,
                         device=dev, initial_values=iv, observed=obs)
    one = build_masked(g, dev, obs, y=y_nan)
    have, want = one.impute_training_data(return_variance=True), over_t.impute_training_data(return_variance=True)
    close(have[0], want[0].cpu().numpy(), 1e-9, 'filled')
    close(have[1], want[1].cpu().numpy(), 1e-9, 'variance')


def test_needs_a_mask_trained_model(dev):
    from test_gpu_predict_b1 import build_bgplvm
    with pytest.raises(AssertionError):
        build_bgplvm(golden(BGPLVM), dev).impute_training_data(return_variance=True)
