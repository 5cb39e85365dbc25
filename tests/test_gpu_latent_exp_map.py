"""GPU tests of geodesic_acceleration / latent_exp_map on bayesian_gp_lvm, MRD, dp_gp_lvm and dp_gp_lvm_t, each trained on complete
data and with a 30 % random mask (one column never observed): the models, points and recorder of tests/test_gpu_latent_metric.py
(N = 40, D = 12, M = 9, Q = 3, T = 3, N* = 7).  The acceleration is pinned to a NumPy restatement built column by column from the
model's own marginals._Marginals pieces and to central differences of the model's own latent_metric, the exponential map to the
NumPy RK4 restatement of tests/test_point_christoffel_refs.py on that restated acceleration."""
import os

import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models import geodesic
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
from test_gpu_latent_metric import CASES, D, D0, DEV, M, N_T, Q, T, UNSEEN, Recorder, data, features, model_of, points, restated
from test_point_christoffel_refs import check_fourth_order, fixture, rk4_ref

pytestmark = pytest.mark.gpu
STEPS = 16


def velocities(case):
    return torch.as_tensor(0.4 * np.random.default_rng(41).standard_normal((N_T, Q)), device=DEV)


def as_list(case, out, kw=()):
    return list(out) if case.startswith('mrd') and not dict(kw).get('total') else [out]


# ---- the NumPy restatement, column by column -----------------------------------------------------------------------------------------
def restated_gam(marg, x, v, cols=None, weights=None):
    """sum over the kernels and columns of w (b^T r_d r_d^T d - b^T C_p(d) d), d_m = k_m [(sum_q gamma_q (x_q - z_mq) v_q)^2 -
    sum_q gamma_q v_q^2]: the contracted Christoffel symbol of test_gpu_latent_metric.restated's metric."""
    num = lambda a: a.detach().cpu().numpy()
    z, gamma, alpha, c, r, gidx = (num(a) for a in (marg.z, marg.gamma, marg.alpha, marg.c, marg.r, marg.gidx))
    cols = range(r.shape[2]) if cols is None else cols
    out = np.zeros_like(x)
    for k in range(z.shape[0]):
        b = features(z[k], x, gamma[k], alpha[k])                                 # [N*, M, Q]
        diff = x[:, None, :] - z[k][None]
        kv = alpha[k] * np.exp(-0.5 * np.sum(gamma[k] * diff * diff, axis=-1))
        dv = kv * (np.sum(gamma[k] * diff * v[:, None, :], axis=-1) ** 2 - np.sum(gamma[k] * v * v, axis=-1)[:, None])   # [N*, M]
        for d in cols:
            w = 1.0 if weights is None else weights[k, d]
            out += w * np.einsum('nmq,m->nq', b, r[k, :, d]) * (dv @ r[k, :, d])[:, None]
            if gidx[k, d] >= 0:
                out -= w * np.einsum('nmq,mp,np->nq', b, c[k, gidx[k, d]], dv)
    return out


def restatement(case, model, monkeypatch, **kw):
    """The callable (x, v) -> (a, G) in NumPy of model.geodesic_acceleration(., ., **kw), one per returned entry, from the pieces
    that the model builds inside one call."""
    rec = Recorder(monkeypatch)
    model.geodesic_acceleration(points(case), velocities(case), **kw)
    monkeypatch.undo()
    kind, masked = case.split()[0], case.endswith('masked')
    cols = kw.get('columns')

    def of(parts, extra=None):
        def accel(x, v):
            g = sum(restated(m, x, c, w) for m, c, w in parts) + (0.0 if extra is None else extra)
            gam = sum(restated_gam(m, x, v, c, w) for m, c, w in parts)
            return -np.linalg.solve(g, gam[:, :, None])[:, :, 0], g
        return accel

    if kind == 'mrd':
        views = [(m, None, None) for m in rec.marg]                           # the training side builds every view, in order
        views = [views[i] for i in kw.get('views', range(len(views)))]
        return [of(views)] if kw.get('total') else [of([p]) for p in views]
    if kind == 'bgplvm':
        return [of([(rec.marg[0], cols, None)])]
    if kind == 'over_t':
        return [of([(rec.marg[0], cols, rec.mom[0].phit.cpu().numpy())])]
    chosen = list(range(D)) if cols is None else list(cols)                    # over_d: one kernel per observed column of `columns`
    unseen = masked and UNSEEN in chosen
    assert rec.marg[0].z.shape[0] == len(chosen) - unseen
    extra = float(model.signal_variance[UNSEEN]) * np.diag(model.ard_weights[UNSEEN].detach().cpu().numpy()) if unseen else None
    return [of([(rec.marg[0], None, None)], extra)]


def rel(have, want):
    return float(np.max(np.abs(have - want))), float(np.max(np.abs(want)))


@pytest.mark.parametrize('case', CASES)
def test_acceleration_is_the_column_by_column_restatement(case, monkeypatch):
    model, x, v = model_of(case), points(case), velocities(case)
    want = restatement(case, model, monkeypatch)
    have = as_list(case, model.geodesic_acceleration(x, v))
    assert len(have) == len(want)
    for a, w in zip(have, want):
        assert tuple(a.shape) == (N_T, Q) and a.dtype == torch.float64 and a.is_cuda
        err, scale = rel(a.cpu().numpy(), w(x.cpu().numpy(), v.cpu().numpy())[0])
        print('%s: max |a - restatement| %.3e of %.3e' % (case, err, scale))
        assert scale > 1e-3 and err <= 1e-9 * scale
    # one point, numpy inputs: the same bits
    one = as_list(case, model.geodesic_acceleration(x[2].cpu().numpy(), v[2].cpu().numpy()))
    for o, a in zip(one, have):
        assert tuple(o.shape) == (Q,) and torch.equal(o, a[2])


@pytest.mark.parametrize('case', CASES)
def test_acceleration_against_central_differences_of_the_latent_metric(case):
    model, x, v = model_of(case), points(case), velocities(case)
    metric = lambda xx: as_list(case, model.latent_metric(xx))
    have = as_list(case, model.geodesic_acceleration(x, v))
    h = 1e-5
    up, dn, g0 = metric(x + h * v), metric(x - h * v), metric(x)
    grads = [torch.zeros_like(x) for _ in have]
    for j in range(Q):
        e = torch.zeros(Q, dtype=torch.float64, device=DEV)
        e[j] = h
        for gr, gp, gm in zip(grads, metric(x + e), metric(x - e)):
            gr[:, j] = torch.einsum('nq,nqr,nr->n', v, gp - gm, v) / (2 * h)
    for a, gp, gm, g, gr in zip(have, up, dn, g0, grads):
        gam = torch.einsum('nqr,nr->nq', (gp - gm) / (2 * h), v) - 0.5 * gr
        want = -torch.linalg.solve(g, gam[:, :, None])[:, :, 0]
        err, scale = float((a - want).abs().max()), float(want.abs().max())
        print('%s: max |a - central differences| %.3e of %.3e' % (case, err, scale))
        assert scale > 1e-3 and err <= 1e-5 * max(1.0, scale)


@pytest.mark.parametrize('case', CASES)
def test_exp_map_is_the_numpy_rk4_of_the_restatement(case, monkeypatch):
    model, x, v = model_of(case), points(case), velocities(case)
    want = restatement(case, model, monkeypatch)
    have = as_list(case, model.latent_exp_map(x, v, num_steps=STEPS, return_velocity=True))
    plain = as_list(case, model.latent_exp_map(x, v, num_steps=STEPS))
    single = as_list(case, model.latent_exp_map(x[3], v[3].cpu().numpy(), num_steps=STEPS, return_velocity=True))
    for (c, w), p, (c1, w1), acc in zip(have, plain, single, want):
        assert tuple(c.shape) == (N_T, STEPS + 1, Q) == tuple(w.shape) and c.dtype == torch.float64 and c.is_cuda
        assert torch.equal(c[:, 0], x) and torch.equal(w[:, 0], v) and torch.equal(p, c)          # row 0: the bits of x
        rc, rw = rk4_ref(lambda xx, vv: acc(xx, vv)[0], x.cpu().numpy(), v.cpu().numpy(), STEPS)
        (ec, sc), (ew, sw) = rel(c.cpu().numpy(), rc), rel(w.cpu().numpy(), rw)
        bend = float(np.max(np.abs(rc[:, -1] - (rc[:, 0] + rw[:, 0]))))
        print('%s: |curve - rk4| %.3e of %.3e, |velocity - rk4| %.3e of %.3e; end off the straight line by %.3e'
              % (case, ec, sc, ew, sw, bend))
        assert ec <= 1e-9 * max(1.0, sc) and ew <= 1e-9 * max(1.0, sw)
        assert bend > 1e-4                                                   # (the curves bend: not a test of x + t v)
        assert tuple(c1.shape) == (STEPS + 1, Q) and torch.equal(c1, c[3]) and torch.equal(w1, w[3])   # a batch is its curves


def test_fourth_order_on_the_gpu():
    """The drift and reversal ratios of the CPU file's integrator fixture, through the two operators and geodesic.exp_map."""
    f = fixture()
    t = lambda a: torch.as_tensor(np.array(a, dtype=np.float64), device=DEV)
    z, gamma, alpha, p, prior = (t(f[n]) for n in ('z', 'gamma', 'alpha', 'p', 'prior'))

    def accel(x, v):
        return ops.geodesic_accel(*ops.ard_rbf_point_christoffel(z, x, v, gamma, alpha, p), prior, v)

    def shoot(x, v, s):
        c, w = geodesic.exp_map(accel, t(x), t(v), 3, DEV, s, return_velocity=True)
        return c.cpu().numpy(), w.cpu().numpy()

    metric = lambda x: (ops.ard_rbf_point_metric(z, t(x), gamma, alpha, p)[0] + torch.diag(prior)).cpu().numpy()
    check_fourth_order(shoot, metric, np.asarray(f['x']), np.asarray(f['v']))


@pytest.mark.parametrize('case', CASES)
def test_far_from_the_inducing_inputs_the_geodesic_is_the_straight_line(case):
    model, x, v = model_of(case), points(case) + 100.0, velocities(case)
    for a in as_list(case, model.geodesic_acceleration(x, v)):
        assert torch.all(a == 0)
    t = torch.arange(5, dtype=torch.float64, device=DEV) / 4
    line = x[:, None, :] + t[None, :, None] * v[:, None, :]
    for c in as_list(case, model.latent_exp_map(x, v, num_steps=4)):
        assert float((c - line).abs().max()) <= 1e-14 * float(line.abs().max())


@pytest.mark.parametrize('case', ['bgplvm', 'mrd masked', 'over_d masked', 'over_t'])
def test_curve_length_converges_to_the_initial_speed(case):
    """A geodesic has constant speed |v|_G, so its length over t in [0, 1] is sqrt(v^T G(x) v); curve_length is the midpoint rule
    (second order) on an RK4 curve (fourth order): the gap shrinks by >= 3 when the steps double (theory: 4)."""
    model, x, v = model_of(case), points(case), velocities(case)
    kw = dict(total=True) if case.startswith('mrd') else {}
    g = model.latent_metric(x, **kw)
    speed = torch.sqrt(torch.einsum('nq,nqr,nr->n', v, g, v))
    gaps = []
    for s in (8, 16):
        length = model.curve_length(model.latent_exp_map(x, v, num_steps=s, **kw), **kw)
        gaps.append((length - speed).abs() / speed)
    worst = int(torch.argmax(gaps[0]))
    print('%s: relative gaps %.3e, %.3e (ratio %.2f)' % (case, float(gaps[0][worst]), float(gaps[1][worst]),
                                                          float(gaps[0][worst] / gaps[1][worst])))
    live = gaps[0] > 1e-8                                                    # (a ray whose gap is already at rounding says nothing)
    assert bool(live.any()) and bool(torch.all(gaps[0][live] >= 3.0 * gaps[1][live]))


@pytest.mark.parametrize('case', ['over_d', 'over_d masked', 'over_t', 'over_t masked', 'bgplvm masked'])
def test_columns_of_one_group_match_the_restatement(case, monkeypatch):
    model, x, v = model_of(case), points(case), velocities(case)
    if case.startswith('bgplvm'):
        cols = [0, UNSEEN, 5, 11]
    else:
        group = torch.argmax(model.assignments, dim=1).cpu().numpy()
        cols = sorted(set(np.flatnonzero(group == group[0]).tolist()) | ({UNSEEN} if case.endswith('masked') else set()))
    assert 1 <= len(cols) <= D
    want = restatement(case, model, monkeypatch, columns=cols)[0]
    xn, vn = x.cpu().numpy(), v.cpu().numpy()
    a = model.geodesic_acceleration(x, v, columns=np.array(cols))
    err, scale = rel(a.cpu().numpy(), want(xn, vn)[0])
    print('%s columns %s: max |a - restatement| %.3e of %.3e' % (case, cols, err, scale))
    assert err <= 1e-9 * max(scale, 1e-3)
    c = model.latent_exp_map(x, v, num_steps=STEPS, columns=cols)
    ec, sc = rel(c.cpu().numpy(), rk4_ref(lambda xx, vv: want(xx, vv)[0], xn, vn, STEPS)[0])
    assert ec <= 1e-9 * max(1.0, sc)
    with pytest.raises(AssertionError):
        model.geodesic_acceleration(x, v, columns=[D])
    with pytest.raises(AssertionError):
        model.latent_exp_map(x[:, :2], v[:, :2])
    with pytest.raises(AssertionError):
        model.latent_exp_map(x, v[:3])
    if case.endswith('masked') and not case.startswith('bgplvm'):            # the prior alone: a constant metric, straight lines
        assert torch.all(model.geodesic_acceleration(x, v, columns=[UNSEEN]) == 0)


@pytest.mark.parametrize('case', ['mrd', 'mrd masked'])
def test_mrd_views_and_total_match_the_restatement(case, monkeypatch):
    model, x, v = model_of(case), points(case), velocities(case)
    xn, vn = x.cpu().numpy(), v.cpu().numpy()
    both = model.geodesic_acceleration(x, v)
    assert len(both) == 2
    for kw in (dict(views=[1]), dict(total=True), dict(views=[1], total=True)):
        want = restatement(case, model, monkeypatch, **kw)[0]
        a = model.geodesic_acceleration(x, v, **kw)
        a = a if kw.get('total') else a[0]
        err, scale = rel(a.cpu().numpy(), want(xn, vn)[0])
        print('%s %s: max |a - restatement| %.3e of %.3e' % (case, kw, err, scale))
        assert scale > 1e-3 and err <= 1e-9 * scale
        c = model.latent_exp_map(x, v, num_steps=STEPS, **kw)
        c = c if kw.get('total') else c[0]
        ec, sc = rel(c.cpu().numpy(), rk4_ref(lambda xx, vv: want(xx, vv)[0], xn, vn, STEPS)[0])
        assert ec <= 1e-9 * max(1.0, sc)
    assert torch.equal(model.geodesic_acceleration(x, v, views=[1])[0], both[1])
    assert torch.equal(model.geodesic_acceleration(x, v, views=[1], total=True), both[1])
    with pytest.raises(AssertionError):
        model.latent_exp_map(x, v, views=[2])


def test_a_failed_factorisation_raises_once_at_the_end():
    nan = torch.full((2, Q), float('nan'), dtype=torch.float64, device=DEV)

    def accel(x, v):                                                         # the second curve fails at every stage
        info = torch.as_tensor([0, 2], dtype=torch.int32, device=DEV)
        return torch.where(info[:, None] != 0, nan, torch.zeros_like(x)), torch.zeros(2, device=DEV), info

    with pytest.raises(FloatingPointError, match='1 of 2'):
        geodesic.exp_map(accel, np.zeros((2, Q)), np.ones((2, Q)), Q, DEV, 3)


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
        for name in ('geodesic_acceleration', 'latent_exp_map'):
            with pytest.raises(AssertionError, match='%s is not built for a model sharded over a process group' % name):
                getattr(model, name)(x, x)
    finally:
        if created:
            dist.destroy_process_group()
