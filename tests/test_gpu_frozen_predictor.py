"""GPU tests of the frozen predictors (models/predictor.py, model.frozen_predictor): bayesian_gp_lvm, MRD, dp_gp_lvm and dp_gp_lvm_t,
each trained on complete data and with observed= (a column never observed among the masked cases), at the small fixtures of
test_gpu_predictive_marginals.py.  p(x, s) must be the bits of predictive_marginals; torch.autograd.grad through p must be the
bits of p.vjp; p.vjp is checked against central differences of predictive_marginals along 4 random directions of q(X*) (h = 1e-5,
bound 1e-5 max(1, |analytic|), the precedent of test_gpu_predict.py); cross-model identities at 1e-9 (the moments' tolerance)."""
import os

import numpy as np
import pytest
import torch

from conftest import golden
from test_gpu_model_t import build as build_dp
from test_gpu_mrd_masked import build as build_mrd_masked
from test_gpu_predict_b1 import build_bgplvm, build_mrd, close, softplus
from test_gpu_predict_t import build_t
from test_gpu_predictive_marginals import BGPLVM, MRD, N_T, OVER_D, mask, over_d_one_hot, points
from test_gpu_train_masked import build_masked
from test_gpu_train_masked_d import build_fixture as build_d_masked
from test_gpu_train_masked_t import build_masked_t

pytestmark = pytest.mark.gpu
CASES = ['bgplvm', 'bgplvm masked', 'mrd', 'mrd masked', 'over_d', 'over_d masked', 'over_t', 'over_t masked']


def model_of(dev, case):
    """(model, pairs): pairs a list of (predictor, marginals(xm, xv) -> (mean, var), never-observed column or None)."""
    masked = case.endswith('masked')
    if case.startswith('mrd'):
        g = golden(MRD)
        nv = int(g['num_views'])
        views = [g['view_%d' % v] for v in range(nv)]
        if masked:
            obs = [mask(*views[v].shape, 17 + v) for v in range(nv)]
            model = build_mrd_masked(g, dev, obs, views=[np.where(o, y, np.nan) for o, y in zip(obs, views)])
        else:
            model = build_mrd(g, dev)
        preds = model.frozen_predictor()
        assert len(preds) == nv
        view = lambda v: (lambda xm, xv: tuple(o[0] for o in model.predictive_marginals(xm, xv, views=[v])))
        return g, model, [(preds[v], view(v), 1 if masked else None) for v in range(nv)]
    g = golden(BGPLVM if case.startswith('bgplvm') else OVER_D)
    y = g['y']
    obs = mask(*y.shape, 17)
    y_nan = np.where(obs, y, np.nan)
    if case.startswith('bgplvm'):
        model = build_masked(g, dev, obs, y=y_nan) if masked else build_bgplvm(g, dev)
    elif case.startswith('over_d'):
        from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
        model = build_d_masked(g, dev, obs, y=y_nan) if masked else build_dp(dp_gp_lvm, g, dev, 'f64')
    else:
        model = build_masked_t(g, dev, obs, y=y_nan) if masked else build_t(g, dev, None)[0]
    return g, model, [(model.frozen_predictor(), model.predictive_marginals, 1 if masked else None)]


def functional(shape, dev, seed):
    rs = np.random.default_rng(seed)
    return torch.as_tensor(rs.standard_normal(shape), device=dev), torch.as_tensor(rs.standard_normal(shape), device=dev)


def check_predictor(tag, dev, p, marginals, xm, xv, unseen):
    want = marginals(xm, xv)
    have = p(xm, xv)
    assert have[0].grad_fn is None and torch.equal(have[0], want[0]) and torch.equal(have[1], want[1]), tag + ': p(x, s) differs'
    n, j = want[0].shape
    assert p.num_columns == j
    g_mean, g_var = functional((n, j), dev, 5)
    xt = torch.as_tensor(xm, device=dev).requires_grad_(True)
    st = torch.as_tensor(xv, device=dev).requires_grad_(True)
    mean, var = p(xt, st)
    assert mean.grad_fn is not None and var.grad_fn is not None and torch.equal(mean, want[0]) and torch.equal(var, want[1])
    auto = torch.autograd.grad(torch.sum(g_mean * mean) + torch.sum(g_var * var), (xt, st))
    d_mu, d_s = p.vjp(xm, xv, g_mean, g_var)
    assert tuple(d_mu.shape) == tuple(xm.shape) == tuple(d_s.shape)
    assert torch.equal(auto[0], d_mu) and torch.equal(auto[1], d_s), tag + ': autograd and vjp differ'
    only_mean = torch.autograd.grad(torch.sum(g_mean * p(xt, st)[0]), (xt, st))          # (var unused: its adjoint is None)
    zero = torch.zeros_like(g_var)
    assert all(torch.equal(a, b) for a, b in zip(only_mean, p.vjp(xm, xv, g_mean, zero)))
    rs = np.random.default_rng(23)
    value = lambda a, b: float(sum(torch.sum(gg * o) for gg, o in zip((g_mean, g_var), marginals(a, b))))
    step = 1e-5
    for i in range(4):
        e_mu, e_s = rs.standard_normal(xm.shape), rs.standard_normal(xv.shape)
        norm = np.sqrt(np.sum(e_mu ** 2) + np.sum(e_s ** 2))
        e_mu, e_s = e_mu / norm, e_s / norm
        fd = (value(xm + step * e_mu, xv + step * e_s) - value(xm - step * e_mu, xv - step * e_s)) / (2.0 * step)
        analytic = float(torch.sum(d_mu.cpu() * torch.as_tensor(e_mu)) + torch.sum(d_s.cpu() * torch.as_tensor(e_s)))
        print('%s direction %d: analytic %.9e, central difference %.9e, |diff| %.3e' % (tag, i, analytic, fd, abs(fd - analytic)))
        assert abs(fd - analytic) <= 1e-5 * max(1.0, abs(analytic)), tag
    if unseen is not None:
        assert float(want[0][:, unseen].abs().max()) == 0.0
        keep = torch.zeros((1, j), dtype=torch.float64, device=dev)
        keep[0, unseen] = 1.0
        z_mu, z_s = p.vjp(xm, xv, g_mean * keep, g_var * keep)
        assert float(z_mu.abs().max()) == 0.0 and float(z_s.abs().max()) == 0.0, tag + ': a never-observed column has a gradient'
        assert float(d_mu.abs().max()) > 0.0


@pytest.mark.parametrize('case', CASES)
def test_predictor(dev, case):
    g, model, pairs = model_of(dev, case)
    _, xm, xv = points(g['x_mean'], N_T, 3)
    for i, (p, marginals, unseen) in enumerate(pairs):
        check_predictor('%s[%d]' % (case, i), dev, p, marginals, xm, xv, unseen)


def test_column_and_view_subsets(dev):
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
    g = golden(BGPLVM)
    _, xm, xv = points(g['x_mean'], N_T, 3)
    d = g['y'].shape[1]
    some = [d - 1, 0, 2]
    g_mean, g_var = functional((N_T, d), dev, 7)
    go = golden(OVER_D)
    obs = mask(*go['y'].shape, 17)
    for tag, model in (('bgplvm', build_bgplvm(g, dev)), ('over_d', build_dp(dp_gp_lvm, go, dev, 'f64')),
                       ('over_d masked', build_d_masked(go, dev, obs, y=np.where(obs, go['y'], np.nan))),
                       ('over_t', build_t(go, dev, None)[0])):
        p = model.frozen_predictor(columns=some)
        want = model.predictive_marginals(xm, xv, columns=some)
        have = p(xm, xv)
        assert torch.equal(have[0], want[0]) and torch.equal(have[1], want[1]), tag
        # the other columns' adjoints zero: the whole model's VJP is the subset's
        whole = model.frozen_predictor()
        pad_m, pad_v = torch.zeros_like(g_mean), torch.zeros_like(g_var)
        pad_m[:, some], pad_v[:, some] = g_mean[:, some], g_var[:, some]
        a = whole.vjp(xm, xv, pad_m, pad_v)
        b = p.vjp(xm, xv, g_mean[:, some].contiguous(), g_var[:, some].contiguous())
        close(b[0], a[0].cpu().numpy(), 1e-10, tag + ' d_mu')
        close(b[1], a[1].cpu().numpy(), 1e-10, tag + ' d_s')
        with pytest.raises(AssertionError):
            model.frozen_predictor(columns=[d])
    gm = golden(MRD)
    mrd = build_mrd(gm, dev)
    nv = int(gm['num_views'])
    one = mrd.frozen_predictor(views=[nv - 1])
    want = mrd.predictive_marginals(xm, xv, views=[nv - 1])
    have = one[0](xm, xv)
    assert len(one) == 1 and torch.equal(have[0], want[0][0]) and torch.equal(have[1], want[1][0])
    with pytest.raises(AssertionError):
        mrd.frozen_predictor(views=[nv])


def test_cross_model_identities(dev):
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm_t
    g = golden(BGPLVM)
    y = g['y']
    obs = mask(*y.shape, 17)
    iv = dict(x_mean=g['x_mean'], x_var=softplus(g['x_var_raw']), x_u=g['x_u'], gamma_atoms=softplus(g['gamma_raw']),
              alpha_atoms=softplus(g['alpha_raw']), beta_atoms=softplus(g['beta_raw']))
    over_t = dp_gp_lvm_t(np.where(obs, y, np.nan), num_latent_dims=g['x_mean'].shape[1], num_inducing_points=g['x_u'].shape[0],
                         truncation_level=1, device=dev, initial_values=iv, observed=obs)
    one = build_masked(g, dev, obs, y=np.where(obs, y, np.nan))
    _, xm, xv = points(g['x_mean'], N_T, 3)
    g_mean, g_var = functional((N_T, y.shape[1]), dev, 9)
    pairs = [('T = 1 against the masked bayesian_gp_lvm', over_t.frozen_predictor(), one.frozen_predictor())]
    go, over_d = over_d_one_hot(dev)
    pairs.append(('one-hot over-D against over-T', over_d.frozen_predictor(), build_t(go, dev, None)[0].frozen_predictor()))
    for tag, pa, pb in pairs:
        if tag.startswith('one-hot'):
            _, xm, xv = points(go['x_mean'], N_T, 3)
            g_mean, g_var = functional((N_T, go['y'].shape[1]), dev, 9)
        for name, a, b in zip(('mean', 'var'), pa(xm, xv), pb(xm, xv)):
            close(a, b.cpu().numpy(), 1e-9, tag + ' ' + name)
        for name, a, b in zip(('d_mu', 'd_s'), pa.vjp(xm, xv, g_mean, g_var), pb.vjp(xm, xv, g_mean, g_var)):
            print('%s %s: max |diff| %.3e of %.3e' % (tag, name, float((a - b).abs().max()), float(b.abs().max())))
            close(a, b.cpu().numpy(), 1e-9, tag + ' ' + name)


def test_adam_on_the_held_out_density_lowers_it(dev):
    """The loop of examples/latent_targets.py: rows of which 3 columns are given, q(X*) by Adam through p(x, s)."""
    from dp_gp_lvm_amd.models.predictor import negative_log_density
    g = golden(BGPLVM)
    model = build_bgplvm(g, dev)
    p = model.frozen_predictor()
    idx, xm, _ = points(g['x_mean'], N_T, 3)
    y = torch.as_tensor(g['y'][idx], device=dev)
    given = torch.zeros(y.shape, dtype=torch.bool, device=dev)
    given[:, [0, 2, 4]] = True
    xt = torch.zeros((N_T, xm.shape[1]), dtype=torch.float64, device=dev, requires_grad=True)
    raw = torch.zeros_like(xt).requires_grad_(True)
    opt = torch.optim.Adam([xt, raw], lr=0.05)
    losses = []
    for _ in range(25):
        opt.zero_grad()
        loss = negative_log_density(*p(xt, torch.nn.functional.softplus(raw)), y, given)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print('held-out negative log density: %.6f -> %.6f' % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]


def test_sharded_models_are_refused(dev):
    import torch.distributed as dist
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
    g = golden(OVER_D)
    obs = mask(*g['y'].shape, 17)
    for kw in (dict(obs=None), dict(obs=obs, y=np.where(obs, g['y'], np.nan))):
        share = build_d_masked(g, dev, kw.pop('obs'), _shard_of=(0, 2), **kw)
        with pytest.raises(AssertionError):
            share.frozen_predictor()
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', str(29600 + os.getpid() % 1000))
    created = not dist.is_initialized()
    if created:
        dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        with pytest.raises(AssertionError):
            build_t(g, dev, None, process_group=dist.group.WORLD)[0].frozen_predictor()
    finally:
        if created:
            dist.destroy_process_group()
