"""GPU tests of the latent-geometry surface that the four latent-variable models share (models/latent_geometry.py), on untrained
models at test_gpu_latent_metric.py's shapes (N = 40, D = 12, M = 9, Q = 3, T = 3): the public signatures, the refusal of a sharded
dp_gp_lvm under every method's own name, and the prior-only metric of dp_gp_lvm when no chosen column was observed in training."""
import functools
import inspect
import os

import numpy as np
import pytest
import torch

from dp_gp_lvm_amd.models import geodesic
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm, dp_gp_lvm_t
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm, manifold_relevance_determination
from test_gpu_latent_metric import D0, DEV, M, N_T, Q, T, UNSEEN, data

pytestmark = pytest.mark.gpu

# str(inspect.signature(model.<name>)) of the commit before the methods were written once (17d916b), where each model had its own
COLUMN_SIGNATURES = {
    'latent_metric': '(x, columns=None)',
    'magnification': '(x, columns=None)',
    'curve_energy': '(curve, columns=None, return_gradient=False)',
    'curve_length': '(curve, columns=None)',
    'latent_geodesic': '(x_from, x_to, num_segments=32, num_iterations=200, learning_rate=0.01, columns=None, init=None)',
    'geodesic_acceleration': '(x, v, columns=None)',
    'latent_exp_map': '(x, v, num_steps=64, columns=None, return_velocity=False)',
    'geodesic_deviation': '(x, v, dx, dv, columns=None)',
    'latent_exp_map_tangent': '(x, v, dx, dv, num_steps=64, columns=None, return_velocity=False)',
    'latent_log_map': '(x_from, x_to, num_steps=64, max_iterations=20, tol=1e-10, columns=None, init=None)',
}
VIEW_SIGNATURES = {
    'latent_metric': '(x, views=None, total=False)',
    'magnification': '(x, views=None)',
    'curve_energy': '(curve, views=None, total=False, return_gradient=False)',
    'curve_length': '(curve, views=None, total=False)',
    'latent_geodesic': '(x_from, x_to, num_segments=32, num_iterations=200, learning_rate=0.01, views=None, total=False, init=None)',
    'geodesic_acceleration': '(x, v, views=None, total=False)',
    'latent_exp_map': '(x, v, num_steps=64, views=None, total=False, return_velocity=False)',
    'geodesic_deviation': '(x, v, dx, dv, views=None, total=False)',
    'latent_exp_map_tangent': '(x, v, dx, dv, num_steps=64, views=None, total=False, return_velocity=False)',
    'latent_log_map': '(x_from, x_to, num_steps=64, max_iterations=20, tol=1e-10, views=None, total=False, init=None)',
}


@functools.lru_cache(maxsize=None)
def untrained(kind, masked=False):
    y, obs = data()
    torch.manual_seed(0)
    np.random.seed(0)
    yy = np.where(obs, y, np.nan) if masked else y
    kw = dict(num_latent_dims=Q, num_inducing_points=M, device=DEV, precision='f64')
    if kind == 'bgplvm':
        return bayesian_gp_lvm(yy, **(dict(kw, observed=obs) if masked else kw))
    if kind == 'mrd':
        views, ms = [yy[:, :D0], yy[:, D0:]], [obs[:, :D0], obs[:, D0:]]
        return manifold_relevance_determination(views, **(dict(kw, observed=ms) if masked else kw))
    make = dp_gp_lvm if kind == 'over_d' else dp_gp_lvm_t
    return make(yy, truncation_level=T, **(dict(kw, observed=obs) if masked else kw))


@pytest.mark.parametrize('kind', ['bgplvm', 'mrd', 'over_d', 'over_t'])
def test_signatures_are_those_of_the_models_own_copies(kind):
    model = untrained(kind)
    table = VIEW_SIGNATURES if kind == 'mrd' else COLUMN_SIGNATURES
    assert len(table) == 10
    for name, want in table.items():
        method = getattr(model, name)
        assert str(inspect.signature(method)) == want, name
        assert (method.__doc__ or '').strip(), name


def test_a_sharded_model_is_refused_under_every_methods_own_name():
    """Every method that dp_gp_lvm refuses on a sharded model, each with its least valid set of arguments: the five that the model
    keeps (and frozen_predictor), and the nine whose name reaches the refusal through the shared surface's hook."""
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
        x, curve = np.zeros((N_T, Q)), np.zeros((2, Q))
        calls = dict(frozen_predictor=(), predictive_jacobian=(x,), latent_metric=(x,), magnification=(x,),
                     predictive_covariance=(x,), sample_functions=(x,), curve_energy=(curve,), curve_length=(curve,),
                     latent_geodesic=(x, x), geodesic_acceleration=(x, x), latent_exp_map=(x, x),
                     geodesic_deviation=(x, x, x, x), latent_exp_map_tangent=(x, x, x, x), latent_log_map=(x, x))
        assert set(COLUMN_SIGNATURES) <= set(calls)
        for name, args in calls.items():
            with pytest.raises(AssertionError) as raised:
                getattr(model, name)(*args)
            assert str(raised.value) == '%s is not built for a model sharded over a process group' % name
    finally:
        if created:
            dist.destroy_process_group()


def test_no_observed_column_is_the_prior_only_metric():
    """dp_gp_lvm trained with observed=, columns=[UNSEEN]: the metric is the constant alpha_d diag(gamma_d) of that column, so the
    curve terms are geodesic.prior_terms' on the same segments (equal bits), geodesics are straight lines (acceleration exactly
    0) and so is the acceleration's derivative.  w is read off the model's own latent_metric, whose entries it is, and tied to
    alpha_d gamma_d of the accessors at 1e-13 (the accessors mix the atoms in another product: a few roundings of fp64)."""
    model = untrained('over_d', masked=True)
    rs = np.random.default_rng(3)
    curves = torch.as_tensor(rs.standard_normal((2, 5, Q)), device=DEV)
    x, v, dx, dv = (torch.as_tensor(rs.standard_normal((N_T, Q)), device=DEV) for _ in range(4))
    g = model.latent_metric(x, columns=[UNSEEN])
    w = torch.diagonal(g[0]).contiguous()
    assert torch.equal(g, torch.diag_embed(w)[None].expand(N_T, Q, Q))
    want = (float(model.signal_variance[UNSEEN]) * model.ard_weights[UNSEEN]).detach().to(torch.float64)
    assert float((w - want).abs().max()) <= 1e-13 * float(want.max()) and float(w.min()) > 0.0

    mid, direction = geodesic.segments(curves)
    e, gx, gv = geodesic.prior_terms(direction, w)
    energy, grad = model.curve_energy(curves, columns=[UNSEEN], return_gradient=True)
    assert torch.equal(energy, geodesic.energy(e, 2)) and torch.equal(grad, geodesic.gradient(gx, gv, 2))
    assert float(energy.min()) > 0.0 and float(grad.abs().max()) > 0.0
    assert torch.equal(model.curve_length(curves, columns=[UNSEEN]), geodesic.length(e, 2))

    a = model.geodesic_acceleration(x, v, columns=[UNSEEN])
    assert tuple(a.shape) == (N_T, Q) and float(a.abs().max()) == 0.0
    a, da = model.geodesic_deviation(x, v, dx, dv, columns=[UNSEEN])
    assert tuple(a.shape) == tuple(da.shape) == (N_T, Q) and float(a.abs().max()) == 0.0 and float(da.abs().max()) == 0.0
