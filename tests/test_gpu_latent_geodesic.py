"""GPU tests of curve_energy / curve_length / latent_geodesic on bayesian_gp_lvm, MRD, dp_gp_lvm and dp_gp_lvm_t, each trained on
complete data and with a 30 % random mask (one column never observed), at N = 40, D = 12, M = 9, Q = 3, T = 3 after 10 optimise
iterations; C = 3 curves of S = 5 segments and of S = 1.  Energy and length are pinned to the composition
S sum_i v_i^T latent_metric(x_i) v_i of the model's own latent_metric (another operator), the gradient to central differences of
that composition."""
import functools
import os

import numpy as np
import pytest
import torch

from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm, dp_gp_lvm_t
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm, manifold_relevance_determination

pytestmark = pytest.mark.gpu
N, D, M, Q, T, D0, C = 40, 12, 9, 3, 3, 7, 3
UNSEEN = 1                                                   # the column never observed by the masked models
MODELS = ['bgplvm', 'mrd', 'over_d', 'over_t']
CASES = [m + s for m in MODELS for s in ('', ' masked')]
SEGMENTS = [5, 1]
DEV = 'cuda:0'


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
    model.optimise(10, learning_rate=0.05)
    return model


@functools.lru_cache(maxsize=None)
def curves(case, s):
    """C bent curves of s segments between training latents (where the features are alive), as a device tensor."""
    xm = model_of(case).q_x[0].detach().cpu().numpy()
    rs = np.random.default_rng(5 + s)
    ends = rs.permutation(N)[:2 * C]
    t = np.linspace(0.0, 1.0, s + 1)[None, :, None]
    c = xm[ends[:C], None, :] * (1.0 - t) + xm[ends[C:], None, :] * t + 0.1 * rs.standard_normal((C, s + 1, Q))
    return torch.as_tensor(c, device=DEV)


def as_list(case, out):
    return list(out) if case.startswith('mrd') else [out]


def segment_terms(metric, c):
    """e [C, S] = v_i^T G(x_i) v_i from a latent_metric callable."""
    x, v = 0.5 * (c[:, :-1] + c[:, 1:]), c[:, 1:] - c[:, :-1]
    g = metric(x.reshape(-1, Q))
    return [torch.einsum('nq,nqr,nr->n', v.reshape(-1, Q), gi, v.reshape(-1, Q)).reshape(c.shape[0], -1) for gi in g]


def composed(case, model, c, **kw):
    """(E, L), each a list of [C] (one per view for MRD), composed of the model's latent_metric."""
    e = segment_terms(lambda x: as_list(case, model.latent_metric(x, **kw)), c)
    s = c.shape[1] - 1
    return [s * ei.sum(1) for ei in e], [torch.sqrt(ei).sum(1) for ei in e]


def close(have, want, tol):
    err, scale = float((have - want).abs().max()), max(1.0, float(want.abs().max()))
    return err <= tol * scale, (err, scale)


@pytest.mark.parametrize('s', SEGMENTS)
@pytest.mark.parametrize('case', CASES)
def test_energy_and_length_are_composed_of_the_latent_metric(case, s):
    model, c = model_of(case), curves(case, s)
    want_e, want_l = composed(case, model, c)
    have_e, have_l = as_list(case, model.curve_energy(c)), as_list(case, model.curve_length(c))
    assert len(have_e) == len(want_e) == len(have_l)
    for he, we, hl, wl in zip(have_e, want_e, have_l, want_l):
        assert tuple(he.shape) == (C,) and he.dtype == torch.float64 and he.is_cuda and tuple(hl.shape) == (C,)
        ok_e, fig_e = close(he, we, 1e-9)
        ok_l, fig_l = close(hl, wl, 1e-9)
        print('%s S=%d: |E - composed| %.2e of %.2e, |L - composed| %.2e of %.2e' % ((case, s) + fig_e + fig_l))
        assert ok_e and ok_l
        assert float(we.min()) > 1e-3                                    # (not a comparison of zeros)
        assert bool(torch.all(hl * hl <= he * (1 + 1e-12)))
    # numpy curves and a single curve take the same path
    one = as_list(case, model.curve_energy(c[1].cpu().numpy()))
    for o, he in zip(one, have_e):
        assert tuple(o.shape) == (1,) and torch.equal(o[0], he[1])


@pytest.mark.parametrize('s', SEGMENTS)
@pytest.mark.parametrize('case', CASES)
def test_gradient_against_central_differences_of_the_composed_energy(case, s):
    model, c = model_of(case), curves(case, s)
    out = as_list(case, model.curve_energy(c, return_gradient=True))
    if not case.startswith('mrd'):
        out = [tuple(out[0])]
    rs = np.random.default_rng(17)
    h = 1e-5
    for _ in range(4):
        u = torch.as_tensor(rs.standard_normal((C, s + 1, Q)), device=DEV)
        up, _ = composed(case, model, c + h * u)
        dn, _ = composed(case, model, c - h * u)
        for (e, g), ep, en in zip(out, up, dn):
            assert tuple(g.shape) == tuple(c.shape) and g.dtype == torch.float64
            analytic, numeric = (g * u).sum(dim=(1, 2)), (ep - en) / (2 * h)
            err = (analytic - numeric).abs()
            print('%s S=%d: |analytic - numeric| %.2e of %.2e' % (case, s, float(err.max()), float(analytic.abs().max())))
            assert bool(torch.all(err <= 1e-5 * torch.clamp(analytic.abs(), min=1.0))), (analytic, numeric)
    single = as_list(case, model.curve_energy(c[2], return_gradient=True))
    if not case.startswith('mrd'):
        single = [tuple(single[0])]
    for (e1, g1), (e, g) in zip(single, out):
        assert tuple(g1.shape) == (s + 1, Q) and torch.equal(g1, g[2]) and torch.equal(e1[0], e[2])


@pytest.mark.parametrize('case', [c for c in CASES if not c.startswith('mrd')])
def test_energies_add_over_a_partition_of_the_columns(case):
    model, c = model_of(case), curves(case, 5)
    a, b = [0, 1, 5, 11], [2, 3, 4, 6, 7, 8, 9, 10]
    whole, grad = model.curve_energy(c, return_gradient=True)
    ea, ga = model.curve_energy(c, columns=a, return_gradient=True)
    eb, gb = model.curve_energy(c, columns=np.array(b), return_gradient=True)
    assert float((ea + eb - whole).abs().max()) <= 1e-11 * max(1.0, float(whole.abs().max()))
    assert float((ga + gb - grad).abs().max()) <= 1e-11 * max(1.0, float(grad.abs().max()))
    assert float(ea.min()) > 0 and float(eb.min()) > 0
    alone = model.curve_energy(c, columns=[UNSEEN])                      # masked: the prior alone; a constant metric
    if case.endswith('masked'):
        want, _ = composed(case, model, c, columns=[UNSEEN])
        assert close(alone, want[0], 1e-12)[0]
    with pytest.raises(AssertionError):
        model.curve_energy(c, columns=[D])
    with pytest.raises(AssertionError):
        model.curve_length(c[:, :, :2])
    with pytest.raises(AssertionError):
        model.curve_energy(c[:, :1])                                     # a curve needs two points


@pytest.mark.parametrize('case', ['mrd', 'mrd masked'])
def test_mrd_total_is_the_sum_of_the_views(case):
    model, c = model_of(case), curves(case, 5)
    views = model.curve_energy(c, return_gradient=True)
    total, grad = model.curve_energy(c, total=True, return_gradient=True)
    assert len(views) == 2 and tuple(total.shape) == (C,) and tuple(grad.shape) == tuple(c.shape)
    assert float((views[0][0] + views[1][0] - total).abs().max()) <= 1e-11 * max(1.0, float(total.abs().max()))
    assert float((views[0][1] + views[1][1] - grad).abs().max()) <= 1e-11 * max(1.0, float(grad.abs().max()))
    g = model.latent_metric(0.5 * (c[:, :-1] + c[:, 1:]).reshape(-1, Q), total=True)
    v = (c[:, 1:] - c[:, :-1]).reshape(-1, Q)
    e = torch.einsum('nq,nqr,nr->n', v, g, v).reshape(C, -1)
    assert close(model.curve_length(c, total=True), torch.sqrt(e).sum(1), 1e-9)[0]
    one = model.curve_energy(c, views=[1])
    assert len(one) == 1 and torch.equal(one[0], views[1][0])
    assert torch.equal(model.curve_energy(c, views=[1], total=True), views[1][0])
    with pytest.raises(AssertionError):
        model.curve_energy(c, views=[2])


@pytest.mark.parametrize('masked', [False, True], ids=['complete', 'masked'])
def test_over_t_with_one_atom_is_the_bayesian_gp_lvm(masked):
    y, obs = data()
    yy = np.where(obs, y, np.nan) if masked else y
    case = 'bgplvm' + (' masked' if masked else '')
    one, c = model_of(case), curves(case, 5)
    num = lambda v: v.detach().cpu().numpy()
    iv = dict(x_mean=num(one.q_x[0]), x_var=num(torch.diagonal(one.q_x[1], dim1=-2, dim2=-1)), x_u=num(one.inducing_input),
              gamma_atoms=num(one.ard_weights).reshape(1, Q), alpha_atoms=num(one.signal_variance).reshape(1, 1),
              beta_atoms=num(one.noise_precision).reshape(1, 1))
    over_t = dp_gp_lvm_t(yy, num_latent_dims=Q, num_inducing_points=M, truncation_level=1, device=DEV, precision='f64',
                         initial_values=iv, **(dict(observed=obs) if masked else {}))
    (he, hg), (we, wg) = over_t.curve_energy(c, return_gradient=True), one.curve_energy(c, return_gradient=True)
    for have, want, name in ((he, we, 'energy'), (hg, wg, 'gradient'), (over_t.curve_length(c), one.curve_length(c), 'length')):
        ok, fig = close(have, want, 1e-9)
        print('T = 1 %s: max |diff| %.3e of %.3e' % ((name,) + fig))
        assert ok, name


def opposite_ends(model):
    """Two training latents on opposite sides of the data: the extremes along the latents' first principal direction."""
    xm = model.q_x[0].detach().cpu().numpy()
    u = np.linalg.svd(xm - xm.mean(0), full_matrices=False)[2][0]
    proj = (xm - xm.mean(0)) @ u
    return xm[np.argmin(proj)], xm[np.argmax(proj)]


@pytest.mark.parametrize('case', CASES)
def test_geodesic_never_exceeds_the_straight_line_and_keeps_its_ends(case):
    model = model_of(case)
    xm = model.q_x[0].detach().cpu().numpy()
    lo, hi = opposite_ends(model)
    rs = np.random.default_rng(3)
    pick = rs.permutation(N)[:2 * (C - 1)]
    a = torch.as_tensor(np.vstack([lo[None], xm[pick[:C - 1]]]), device=DEV)
    b = torch.as_tensor(np.vstack([hi[None], xm[pick[C - 1:]]]), device=DEV)
    kw = dict(total=True) if case.startswith('mrd') else {}
    start = model.latent_geodesic(a, b, num_segments=5, num_iterations=0, **kw)
    curve, length, energy = model.latent_geodesic(a, b, num_segments=5, num_iterations=50, **kw)
    assert tuple(curve.shape) == (C, 6, Q) and tuple(length.shape) == (C,) and tuple(energy.shape) == (C,)
    assert torch.equal(curve[:, 0], a) and torch.equal(curve[:, -1], b)
    assert torch.equal(start[0][:, 0], a) and torch.equal(start[0][:, -1], b)
    line = a[:, None, :] + torch.arange(6, dtype=torch.float64, device=DEV)[None, :, None] / 5 * (b - a)[:, None, :]
    assert float((start[0] - line).abs().max()) <= 1e-14 * max(1.0, float(line.abs().max()))
    print('%s: straight %s, geodesic %s' % (case, start[2].tolist(), energy.tolist()))
    assert bool(torch.all(energy <= start[2]))
    assert bool(energy[0] < start[2][0])                                 # strictly below between the opposite ends of the data
    assert close(model.curve_energy(curve, **kw), energy, 1e-12)[0]
    assert close(model.curve_length(curve, **kw), length, 1e-12)[0]
    assert bool(torch.all(length * length <= energy * (1 + 1e-12)))
    # a batch is the single-curve calls; init restarts from a given curve and can only improve on it
    c1, l1, e1 = model.latent_geodesic(a[0], b[0].cpu().numpy(), num_segments=5, num_iterations=50, **kw)
    assert tuple(c1.shape) == (1, 6, Q)
    assert close(c1[0], curve[0], 1e-12)[0] and close(e1, energy[:1], 1e-12)[0] and close(l1, length[:1], 1e-12)[0]
    c2, _, e2 = model.latent_geodesic(a, b, num_segments=5, num_iterations=5, init=curve, **kw)
    assert bool(torch.all(e2 <= energy)) and torch.equal(c2[:, 0], a) and torch.equal(c2[:, -1], b)
    # S = 1 has no interior point: the straight segment comes back
    c3, l3, e3 = model.latent_geodesic(a, b, num_segments=1, num_iterations=50, **kw)
    assert torch.equal(c3[:, 0], a) and torch.equal(c3[:, 1], b) and close(l3 * l3, e3, 1e-12)[0]


@pytest.mark.parametrize('case', ['mrd', 'mrd masked'])
def test_mrd_geodesics_per_view(case):
    model = model_of(case)
    lo, hi = opposite_ends(model)
    out = model.latent_geodesic(lo, hi, num_segments=5, num_iterations=5)
    assert len(out) == 2
    energies = model.curve_energy(out[1][0], views=[1])
    assert close(energies[0], out[1][2], 1e-12)[0]
    only = model.latent_geodesic(lo, hi, num_segments=5, num_iterations=5, views=[1])
    assert len(only) == 1 and torch.equal(only[0][0], out[1][0])


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
        c = np.zeros((2, 4, Q))
        for name, args in (('curve_energy', (c,)), ('curve_length', (c,)), ('latent_geodesic', (c[:, 0], c[:, 1]))):
            with pytest.raises(AssertionError, match='%s is not built for a model sharded over a process group' % name):
                getattr(model, name)(*args)
    finally:
        if created:
            dist.destroy_process_group()
