"""GPU tests of model.integrator = 'device' for latent_exp_map / latent_exp_map_tangent / latent_log_map on bayesian_gp_lvm, MRD, dp_gp_lvm and
dp_gp_lvm_t, each trained on complete data and with a 30 % random mask: the models and points of tests/test_gpu_latent_metric.py
(N = 40, D = 12, M = 9, Q = 3, T = 3, N* = 7), the velocities of tests/test_gpu_latent_exp_map.py, the directions and the C = 4 pairs
of tests/test_gpu_latent_log_map.py.  The device route (marginals.Metric.shoot / shoot_tangent on ops.geodesic_shoot[_tangent]) has
to return the BITS of the host route, model.integrator = 'host' (the default), which is pinned by those files.  The choice is an
attribute of the model: the three methods' signatures are pinned by tests/test_gpu_latent_api.py."""
import os

import numpy as np
import pytest
import torch

from dp_gp_lvm_amd.models import marginals
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
from test_gpu_latent_exp_map import as_list, velocities
from test_gpu_latent_log_map import C, directions, round_trip
from test_gpu_latent_metric import CASES, DEV, M, N_T, Q, T, UNSEEN, data, model_of, points

pytestmark = pytest.mark.gpu
STEPS = 16


class on:
    """model with its integrator set to `where` for the length of one method call (the models are shared between the tests)."""

    def __init__(self, model, where):
        self.model, self.where = model, where

    def __getattr__(self, name):
        def call(*a, **kw):
            before = self.model.integrator
            self.model.integrator = self.where
            try:
                return getattr(self.model, name)(*a, **kw)
            finally:
                self.model.integrator = before
        return call


def flat(case, out, kw=()):
    """Every tensor of a public call's result, in order."""
    return [t for entry in as_list(case, out, kw) for t in (entry if isinstance(entry, tuple) else (entry,))]


def same(case, have, want, kw=()):
    have, want = flat(case, have, kw), flat(case, want, kw)
    return len(have) == len(want) and all(h.shape == w.shape and torch.equal(h, w) for h, w in zip(have, want))


def num(t):
    return t.cpu().numpy()


@pytest.mark.parametrize('case', CASES)
def test_exp_map_on_the_device_is_the_host_routes_bits(case):
    model, x, v = model_of(case), points(case), velocities(case)
    for rv in (False, True):
        have = on(model, 'device').latent_exp_map(x, v, num_steps=STEPS, return_velocity=rv)
        assert same(case, have, on(model, 'host').latent_exp_map(x, v, num_steps=STEPS, return_velocity=rv))
        assert same(case, have, model.latent_exp_map(x, v, num_steps=STEPS, return_velocity=rv))          # (the default is 'host')
    whole = flat(case, on(model, 'device').latent_exp_map(x, v, num_steps=STEPS, return_velocity=True))
    one = flat(case, on(model, 'device').latent_exp_map(num(x[3]), num(v[3]), num_steps=STEPS, return_velocity=True))
    for o, w in zip(one, whole):
        assert tuple(o.shape) == (STEPS + 1, Q) and torch.equal(o, w[3])                                  # a batch is its curves


@pytest.mark.parametrize('case', CASES)
def test_exp_map_tangent_on_the_device_is_the_host_routes_bits(case):
    model, x, v = model_of(case), points(case), velocities(case)
    dx, dv = directions(case)
    for rv in (False, True):
        have = on(model, 'device').latent_exp_map_tangent(x, v, dx, dv, num_steps=STEPS, return_velocity=rv)
        assert same(case, have, on(model, 'host').latent_exp_map_tangent(x, v, dx, dv, num_steps=STEPS, return_velocity=rv))
    whole = flat(case, on(model, 'device').latent_exp_map_tangent(x, v, dx, dv, num_steps=STEPS))
    one = flat(case, on(model, 'device').latent_exp_map_tangent(num(x[3]), num(v[3]), num(dx[3]), num(dv[3]), num_steps=STEPS))
    for o, w in zip(one, whole):
        assert tuple(o.shape) == (STEPS + 1, Q) and torch.equal(o, w[3])


@pytest.mark.parametrize('case', CASES)
def test_log_map_on_the_device_is_the_host_routes_bits_and_inverts_the_exp_map(case):
    model = model_of(case)
    model.integrator = 'device'
    try:
        x, v0, ends = round_trip(case, model)
    finally:
        model.integrator = 'host'
    for i, y in enumerate(ends):
        kw = dict(views=[i]) if case.startswith('mrd') else {}
        have = on(model, 'device').latent_log_map(x, y, num_steps=STEPS, **kw)
        assert same(case, have, on(model, 'host').latent_log_map(x, y, num_steps=STEPS, **kw))
        v, dist, curve, res = as_list(case, have)[0]
        tol = 1e-10 * torch.clamp(y.norm(dim=1), min=1.0)
        relv = float(((v - v0).norm(dim=1) / v0.norm(dim=1)).max())
        print('%s: residual %.3e, |v - v0| / |v0| %.3e' % (case, float(res.max()), relv))
        assert bool(torch.all(res <= tol)) and relv <= 1e-8 and torch.equal(curve[:, 0], x)
        one = as_list(case, on(model, 'device').latent_log_map(num(x[2]), num(y[2]), num_steps=STEPS, **kw))[0]
        assert tuple(one[0].shape) == (Q,) and all(torch.equal(o, w[2]) for o, w in zip(one, (v, dist, curve, res)))


@pytest.mark.parametrize('case', ['over_d', 'over_d masked', 'over_t', 'over_t masked', 'bgplvm masked'])
def test_columns_of_one_group(case):
    model, x, v = model_of(case), points(case), velocities(case)
    dx, dv = directions(case)
    if case.startswith('bgplvm'):
        cols = [0, UNSEEN, 5, 11]
    else:
        group = torch.argmax(model.assignments, dim=1).cpu().numpy()
        cols = sorted(set(np.flatnonzero(group == group[0]).tolist()) | ({UNSEEN} if case.endswith('masked') else set()))
    picks = [cols] + ([[UNSEEN]] if case.endswith('masked') and not case.startswith('bgplvm') else [])   # the prior alone: the host loop
    for columns in picks:
        runs = [(on(model, i).latent_exp_map(x, v, num_steps=STEPS, columns=columns, return_velocity=True),
                 on(model, i).latent_exp_map_tangent(x, v, dx, dv, num_steps=STEPS, columns=columns)) for i in ('device', 'host')]
        assert same(case, runs[0][0], runs[1][0]) and same(case, runs[0][1], runs[1][1])
        xs = x[:C].contiguous()
        y = runs[0][0][0][:C, -1].contiguous()
        assert same(case, on(model, 'device').latent_log_map(xs, y, num_steps=STEPS, columns=columns),
                    on(model, 'host').latent_log_map(xs, y, num_steps=STEPS, columns=columns))


@pytest.mark.parametrize('case', ['mrd', 'mrd masked'])
def test_mrd_views_and_total(case):
    model, x, v = model_of(case), points(case), velocities(case)
    dx, dv = directions(case)
    xs = x[:C].contiguous()
    for kw in (dict(views=[1]), dict(total=True), dict(views=[1], total=True)):
        dev, hst = (on(model, i).latent_exp_map(x, v, num_steps=STEPS, return_velocity=True, **kw) for i in ('device', 'host'))
        assert same(case, dev, hst, kw)
        assert same(case, on(model, 'device').latent_exp_map_tangent(x, v, dx, dv, num_steps=STEPS, **kw),
                    on(model, 'host').latent_exp_map_tangent(x, v, dx, dv, num_steps=STEPS, **kw), kw)
        y = flat(case, dev, kw)[0][:C, -1].contiguous()
        assert same(case, on(model, 'device').latent_log_map(xs, y, num_steps=STEPS, **kw),
                    on(model, 'host').latent_log_map(xs, y, num_steps=STEPS, **kw), kw)


@pytest.mark.parametrize('case', ['bgplvm', 'mrd masked', 'over_d masked', 'over_t'])
def test_blocks_of_three_curves_give_the_unblocked_bits(case, monkeypatch):
    model, x, v = model_of(case), points(case), velocities(case)
    dx, dv = directions(case)
    kw = dict(total=True) if case.startswith('mrd') else {}
    whole = (on(model, 'device').latent_exp_map(x, v, num_steps=STEPS, return_velocity=True, **kw),
             on(model, 'device').latent_exp_map_tangent(x, v, dx, dv, num_steps=STEPS, return_velocity=True, **kw))
    init, calls = marginals.Metric.__init__, []

    def small(self, *a, **k):
        init(self, *a, **k)
        self.block = 3                                         # shoot: 3 curves per call; shoot_tangent: 3 // 2 = 1
        calls.append(self)
    monkeypatch.setattr(marginals.Metric, '__init__', small)
    assert same(case, on(model, 'device').latent_exp_map(x, v, num_steps=STEPS, return_velocity=True, **kw), whole[0], kw)
    assert same(case, on(model, 'device').latent_exp_map_tangent(x, v, dx, dv, num_steps=STEPS, return_velocity=True, **kw),
                whole[1], kw)
    assert len(calls) >= 2 and all(m.block == 3 for m in calls)


@pytest.mark.parametrize('case', ['bgplvm', 'mrd', 'over_d masked', 'over_t masked'])
def test_a_metric_that_fails_to_factor_raises_the_host_routes_text(case, monkeypatch):
    model, x, v = model_of(case), points(case), velocities(case)
    dx, dv = directions(case)
    init = marginals.Metric.__init__

    def negative(self, *a, **k):
        init(self, *a, **k)
        self.w = self.w - 1e6                                  # G = data term + diag(w): not positive definite anywhere
    monkeypatch.setattr(marginals.Metric, '__init__', negative)
    kw = dict(total=True) if case.startswith('mrd') else {}
    calls = (lambda i: on(model, i).latent_exp_map(x, v, num_steps=2, **kw),
             lambda i: on(model, i).latent_exp_map_tangent(x, v, dx, dv, num_steps=2, **kw),
             lambda i: on(model, i).latent_log_map(x[:C], x[:C] + v[:C], num_steps=2, **kw))
    for run in calls:
        texts = []
        for integrator in ('host', 'device'):
            with pytest.raises(FloatingPointError) as err:
                run(integrator)
            texts.append(str(err.value))
        assert texts[0] == texts[1] and 'failed to factor' in texts[0], texts


def test_an_unknown_integrator_is_refused_and_the_default_is_the_host():
    for case in ('bgplvm', 'mrd', 'over_d', 'over_t'):
        model = model_of(case)
        assert model.integrator == 'host'
        for bad in ('gpu', None, 'Device'):
            with pytest.raises(ValueError, match="integrator must be 'host' or 'device'"):
                model.integrator = bad
            assert model.integrator == 'host'                                   # a refused value leaves the choice as it was
        model.integrator = 'device'
        assert model.integrator == 'device'
        model.integrator = 'host'


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
        model.integrator = 'device'
        for name, args in (('latent_exp_map', (x, x)), ('latent_exp_map_tangent', (x, x, x, x)), ('latent_log_map', (x, x))):
            with pytest.raises(AssertionError, match='%s is not built for a model sharded over a process group' % name):
                getattr(model, name)(*args)
    finally:
        if created:
            dist.destroy_process_group()
