"""GPU tests of geodesic_deviation / latent_exp_map_tangent / latent_log_map on bayesian_gp_lvm, MRD, dp_gp_lvm and dp_gp_lvm_t, each
trained on complete data and with a 30 % random mask (one column never observed): the models, points and recorder of
tests/test_gpu_latent_metric.py (N = 40, D = 12, M = 9, Q = 3, T = 3, N* = 7) and the velocities of tests/test_gpu_latent_exp_map.py.
The deviation is pinned to a NumPy restatement built column by column from the model's own marginals._Marginals pieces and to
central differences of the model's own geodesic_acceleration; the tangent of the exponential map to the NumPy tangent-linear RK4
of tests/test_point_tangent_refs.py on that restatement and to central differences of the model's own latent_exp_map; the
logarithm map to the round trip through latent_exp_map and to the CPU file's shooting fixture."""
import os

import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models import geodesic
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
from test_gpu_latent_exp_map import as_list, restated_gam, velocities
from test_gpu_latent_metric import CASES, D, DEV, M, N_T, Q, T, UNSEEN, Recorder, data, features, model_of, points, restated
from test_point_christoffel_refs import fixture
from test_point_tangent_refs import fixture_targets, rk4_tangent_ref

pytestmark = pytest.mark.gpu
STEPS = 16
C = 4                                                            # pairs per logarithm-map call


def directions(case):
    rs = np.random.default_rng(43)
    return (torch.as_tensor(0.5 * rs.standard_normal((N_T, Q)), device=DEV), torch.as_tensor(0.5 * rs.standard_normal((N_T, Q)), device=DEV))


# ---- the NumPy restatement, column by column -----------------------------------------------------------------------------------------
def restated_tangent(marg, x, v, dx, dv, cols=None, weights=None):
    """(dG [N*, Q, Q], dgam [N*, Q]): the derivatives of test_gpu_latent_metric.restated's metric and of restated_gam's symbol along
    the direction (dx, dv) of (x, v), column by column: with m_d = b^T r_d,
    dG_d = dm_d m_d^T + m_d dm_d^T - db^T C b - b^T C db,   dgam_d = db^T r_d (r_d . d) + b^T r_d (r_d . dd) - db^T C d - b^T C dd."""
    num = lambda a: a.detach().cpu().numpy()
    z, gamma, alpha, c, r, gidx = (num(a) for a in (marg.z, marg.gamma, marg.alpha, marg.c, marg.r, marg.gidx))
    cols = range(r.shape[2]) if cols is None else cols
    dg, dgam = np.zeros((x.shape[0], x.shape[1], x.shape[1])), np.zeros_like(x)
    for k in range(z.shape[0]):
        b = features(z[k], x, gamma[k], alpha[k])                                 # [N*, M, Q]
        diff = x[:, None, :] - z[k][None]
        u = gamma[k] * diff
        kv = alpha[k] * np.exp(-0.5 * np.sum(u * diff, axis=-1))                  # [N*, M]
        a, e, f = (np.sum(u * w[:, None, :], axis=-1) for w in (v, dx, dv))
        s, c1, c2 = (np.sum(gamma[k] * w1 * w2, axis=-1)[:, None] for w1, w2 in ((v, v), (dx, v), (v, dv)))
        dvec = kv * (a * a - s)
        ddvec = kv * (-e * (a * a - s) + 2 * a * (c1 + f) - 2 * c2)
        db = kv[..., None] * (e[..., None] * u - gamma[k] * dx[:, None, :])
        for d in cols:
            w = 1.0 if weights is None else weights[k, d]
            m, dm = np.einsum('nmq,m->nq', b, r[k, :, d]), np.einsum('nmq,m->nq', db, r[k, :, d])
            dg += w * (dm[:, :, None] * m[:, None, :] + m[:, :, None] * dm[:, None, :])
            dgam += w * (dm * (dvec @ r[k, :, d])[:, None] + m * (ddvec @ r[k, :, d])[:, None])
            if gidx[k, d] >= 0:
                cm = c[k, gidx[k, d]]
                dg -= w * (np.einsum('nmq,mp,npr->nqr', db, cm, b) + np.einsum('nmq,mp,npr->nqr', b, cm, db))
                dgam -= w * (np.einsum('nmq,mp,np->nq', db, cm, dvec) + np.einsum('nmq,mp,np->nq', b, cm, ddvec))
    return dg, dgam


def restatement(case, model, monkeypatch, **kw):
    """The callables (x, v, dx, dv) -> (a, da) in NumPy of model.geodesic_deviation(., ., ., ., **kw), one per returned entry, from
    the pieces that the model builds inside one call (the branches of test_gpu_latent_exp_map.restatement)."""
    rec = Recorder(monkeypatch)
    model.geodesic_deviation(points(case), velocities(case), *directions(case), **kw)
    monkeypatch.undo()
    kind, masked = case.split()[0], case.endswith('masked')
    cols = kw.get('columns')

    def of(parts, extra=None):
        def accel(x, v, dx, dv):
            g = sum(restated(m, x, c, w) for m, c, w in parts) + (0.0 if extra is None else extra)
            gam = sum(restated_gam(m, x, v, c, w) for m, c, w in parts)
            both = [restated_tangent(m, x, v, dx, dv, c, w) for m, c, w in parts]
            dg, dgam = sum(t[0] for t in both), sum(t[1] for t in both)
            a = -np.linalg.solve(g, gam[:, :, None])[:, :, 0]
            rhs = dgam + np.einsum('nqr,nr->nq', dg, a)
            return a, -np.linalg.solve(g, rhs[:, :, None])[:, :, 0]
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


def num(t):
    return t.cpu().numpy()


class Shots:
    """Counts the stages that go through ops.geodesic_accel_tangent: a shot of S steps is 4 S of them."""

    def __init__(self, monkeypatch):
        self.calls = 0
        inner = ops.geodesic_accel_tangent

        def counted(*a, **kw):
            self.calls += 1
            return inner(*a, **kw)
        monkeypatch.setattr(ops, 'geodesic_accel_tangent', counted)

    def updates(self, steps, results=1):
        assert self.calls % (4 * steps * results) == 0
        return self.calls // (4 * steps * results) - 1


# ---- the deviation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_deviation_is_the_restatement_and_the_central_difference_of_the_acceleration(case, monkeypatch):
    model, x, v = model_of(case), points(case), velocities(case)
    dx, dv = directions(case)
    want = restatement(case, model, monkeypatch)
    have = as_list(case, model.geodesic_deviation(x, v, dx, dv))
    plain = as_list(case, model.geodesic_acceleration(x, v))
    h = 1e-5
    up, dn = as_list(case, model.geodesic_acceleration(x + h * dx, v + h * dv)), as_list(case, model.geodesic_acceleration(x - h * dx, v - h * dv))
    assert len(have) == len(want)
    for (a, da), w, p, u, d in zip(have, want, plain, up, dn):
        assert tuple(da.shape) == (N_T, Q) and da.dtype == torch.float64 and da.is_cuda
        assert torch.equal(a, p)                                             # geodesic_acceleration's bits
        err, scale = rel(num(da), w(num(x), num(v), num(dx), num(dv))[1])
        fd = (u - d) / (2 * h)
        err_fd, scale_fd = float((da - fd).abs().max()), float(fd.abs().max())
        print('%s: max |da - restatement| %.3e of %.3e, |da - central differences| %.3e of %.3e' % (case, err, scale, err_fd, scale_fd))
        assert scale > 1e-3 and err <= 1e-9 * scale
        assert err_fd <= 1e-5 * max(1.0, scale_fd)
    one = as_list(case, model.geodesic_deviation(num(x[2]), num(v[2]), num(dx[2]), num(dv[2])))       # one point, numpy inputs
    for (a1, da1), (a, da) in zip(one, have):
        assert tuple(da1.shape) == (Q,) and torch.equal(a1, a[2]) and torch.equal(da1, da[2])


# ---- the tangent of the exponential map --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_exp_map_tangent_is_the_numpy_tangent_rk4_and_the_central_difference_of_the_exp_map(case, monkeypatch):
    model, x, v = model_of(case), points(case), velocities(case)
    dx, dv = directions(case)
    want = restatement(case, model, monkeypatch)
    have = as_list(case, model.latent_exp_map_tangent(x, v, dx, dv, num_steps=STEPS, return_velocity=True))
    short = as_list(case, model.latent_exp_map_tangent(x, v, dx, dv, num_steps=STEPS))
    plain = as_list(case, model.latent_exp_map(x, v, num_steps=STEPS, return_velocity=True))
    h = 1e-5
    up = as_list(case, model.latent_exp_map(x + h * dx, v + h * dv, num_steps=STEPS))
    dn = as_list(case, model.latent_exp_map(x - h * dx, v - h * dv, num_steps=STEPS))
    single = as_list(case, model.latent_exp_map_tangent(x[3], num(v[3]), dx[3], dv[3], num_steps=STEPS))
    for (c, dc, w, dw), s, (pc, pw), u, d, (c1, dc1), acc in zip(have, short, plain, up, dn, single, want):
        assert tuple(dc.shape) == (N_T, STEPS + 1, Q) == tuple(dw.shape) and dc.dtype == torch.float64 and dc.is_cuda
        assert torch.equal(c, pc) and torch.equal(w, pw)                     # latent_exp_map's bits
        assert torch.equal(dc[:, 0], dx) and torch.equal(dw[:, 0], dv) and torch.equal(s[0], c) and torch.equal(s[1], dc)
        _, rdc, _, rdw = rk4_tangent_ref(acc, num(x), num(v), num(dx), num(dv), STEPS)
        (ec, sc), (ew, sw) = rel(num(dc), rdc), rel(num(dw), rdw)
        fd = (u - d) / (2 * h)
        efd, sfd = float((dc - fd).abs().max()), float(fd.abs().max())
        print('%s: |dcurve - tangent rk4| %.3e of %.3e, |dvelocity - tangent rk4| %.3e of %.3e, |dcurve - central differences| '
              '%.3e of %.3e' % (case, ec, sc, ew, sw, efd, sfd))
        assert ec <= 1e-9 * max(1.0, sc) and ew <= 1e-9 * max(1.0, sw)
        assert efd <= 1e-5 * max(1.0, sfd)
        assert tuple(dc1.shape) == (STEPS + 1, Q) and torch.equal(c1, c[3]) and torch.equal(dc1, dc[3])     # a batch is its curves


# ---- the logarithm map ---------------------------------------------------------------------------------------------------------------
def test_the_shooting_fixture_through_the_gpu_operators():
    """The CPU file's fixture: converged in at most 5 updates (the NumPy restatement's 3 plus 2), to its residual and velocity."""
    f = fixture()
    t = lambda a: torch.as_tensor(np.array(a, dtype=np.float64), device=DEV)
    z, gamma, alpha, p, prior = (t(f[n]) for n in ('z', 'gamma', 'alpha', 'p', 'prior'))
    calls = [0]

    def accel_tangent(x, v, dx, dv):
        calls[0] += 1
        return ops.geodesic_accel_tangent(*ops.ard_rbf_point_christoffel_tangent(z, x, v, dx, dv, gamma, alpha, p), prior, v)

    y, v0 = fixture_targets(STEPS)
    v, dist, curve, res = geodesic.log_map(accel_tangent, t(f['x']), t(y), 3, DEV, num_steps=STEPS)
    updates = calls[0] // (4 * STEPS) - 1
    relv = np.linalg.norm(num(v) - v0, axis=1) / np.linalg.norm(v0, axis=1)
    print('updates %d, residual %.3e, |v - v0| / |v0| %.3e' % (updates, float(res.max()), relv.max()))
    assert updates <= 5 and float(res.max()) <= 1e-10 and relv.max() <= 1e-8
    assert tuple(curve.shape) == (4, STEPS + 1, 3) and torch.equal(curve[:, 0], t(f['x']))
    assert float((curve[:, -1] - t(y)).norm(dim=1).sub(res).abs().max()) <= 1e-15 * float(res.max())


def round_trip(case, model, steps=STEPS, **kw):
    """(x, v0, y): C of the case's points, the exp-map test's velocities there and the ends of their exponential maps."""
    x, v0 = points(case)[:C].contiguous(), velocities(case)[:C].contiguous()
    y = model.latent_exp_map(x, v0, num_steps=steps, **kw)
    return x, v0, [c[:, -1].contiguous() for c in as_list(case, y, kw)]


@pytest.mark.parametrize('case', CASES)
def test_log_map_inverts_the_exp_map(case, monkeypatch):
    model = model_of(case)
    x, v0, ends = round_trip(case, model)
    for i, y in enumerate(ends):
        bend = float((y - (x + v0)).norm(dim=1).max())
        kw = dict(views=[i]) if case.startswith('mrd') else {}
        shots = Shots(monkeypatch)
        v, dist, curve, res = as_list(case, model.latent_log_map(x, y, num_steps=STEPS, **kw))[0]
        monkeypatch.undo()
        updates = shots.updates(STEPS)
        relv = float(((v - v0).norm(dim=1) / v0.norm(dim=1)).max())
        tol = 1e-10 * torch.clamp(y.norm(dim=1), min=1.0)
        print('%s: %d updates, end off the straight end by %.3e, residual %.3e, |v - v0| / |v0| %.3e'
              % (case, updates, bend, float(res.max()), relv))
        assert tuple(v.shape) == (C, Q) and tuple(dist.shape) == (C,) == tuple(res.shape) and tuple(curve.shape) == (C, STEPS + 1, Q)
        assert updates <= 20 and bool(torch.all(res <= tol)) and relv <= 1e-8
        assert bend > 1e-4 and torch.equal(curve[:, 0], x)
        g = as_list(case, model.latent_metric(x, **kw))[0]
        want = torch.sqrt(torch.einsum('nq,nqr,nr->n', v, g, v))
        assert float(((dist - want).abs() / want).max()) <= 1e-11           # (two orders of summing Q^2 K terms of a positive form)


@pytest.mark.parametrize('case', ['bgplvm', 'mrd masked', 'over_d masked', 'over_t'])
def test_distance_is_the_limit_of_the_returned_curves_length(case):
    """distance = |v|_G(x_from), the length of the geodesic; curve_length is the midpoint rule (second order) on the returned RK4
    curve (fourth order): the gap shrinks by >= 3 when the steps double (theory: 4), as in the exponential map's test."""
    model = model_of(case)
    kw = dict(total=True) if case.startswith('mrd') else {}
    gaps = []
    for s in (8, 16):
        x, v0, (y,) = round_trip(case, model, s, **kw)
        v, dist, curve, res = model.latent_log_map(x, y, num_steps=s, **kw)
        assert bool(torch.all(res <= 1e-10 * torch.clamp(y.norm(dim=1), min=1.0)))
        gaps.append((model.curve_length(curve, **kw) - dist).abs() / dist)
    worst = int(torch.argmax(gaps[0]))
    print('%s: relative gaps %.3e, %.3e (ratio %.2f)' % (case, float(gaps[0][worst]), float(gaps[1][worst]),
                                                          float(gaps[0][worst] / gaps[1][worst])))
    live = gaps[0] > 1e-8
    assert bool(live.any()) and bool(torch.all(gaps[0][live] >= 3.0 * gaps[1][live]))


@pytest.mark.parametrize('case', CASES)
def test_far_from_the_inducing_inputs_the_logarithm_is_the_difference(case, monkeypatch):
    model, x, v0 = model_of(case), points(case)[:C] + 100.0, velocities(case)[:C]
    y = x + v0
    shots = Shots(monkeypatch)
    out = as_list(case, model.latent_log_map(x, y, num_steps=4))
    monkeypatch.undo()
    assert shots.updates(4, len(out)) <= 1
    for v, dist, curve, res in out:
        assert float((v - (y - x)).abs().max()) <= 1e-14 * float(y.abs().max())
        assert float(res.max()) <= 1e-14 * float(y.abs().max())


@pytest.mark.parametrize('case', ['bgplvm', 'over_t masked'])
def test_one_iteration_is_never_worse_than_the_start_and_a_single_pair_is_its_row(case):
    model = model_of(case)
    x, v0, (y,) = round_trip(case, model)
    start = (model.latent_exp_map(x, y - x, num_steps=STEPS)[:, -1] - y).norm(dim=1)
    v, dist, curve, res = model.latent_log_map(x, y, num_steps=STEPS, max_iterations=1)
    tol = 1e-10 * torch.clamp(y.norm(dim=1), min=1.0)
    print('%s: start %.3e, after one update %.3e' % (case, float(start.max()), float(res.max())))
    assert bool(torch.any(res > tol)) and bool(torch.all(res <= start))
    zero = model.latent_log_map(x, y, num_steps=STEPS, max_iterations=0)
    assert torch.equal(zero[0], y - x) and float((zero[3] - start).abs().max()) <= 1e-15 * float(start.max())
    whole = model.latent_log_map(x, y, num_steps=STEPS)
    one = model.latent_log_map(num(x[2]), y[2], num_steps=STEPS)
    assert tuple(one[0].shape) == (Q,) and one[1].dim() == 0 and tuple(one[2].shape) == (STEPS + 1, Q) and one[3].dim() == 0
    for o, w in zip(one, whole):
        assert torch.equal(o, w[2])
    again = model.latent_log_map(x, y, num_steps=STEPS, init=whole[0])
    assert bool(torch.all(again[3] <= tol))


@pytest.mark.parametrize('case', ['over_d', 'over_d masked', 'over_t', 'over_t masked', 'bgplvm masked'])
def test_columns_of_one_group(case, monkeypatch):
    model, x, v = model_of(case), points(case), velocities(case)
    dx, dv = directions(case)
    if case.startswith('bgplvm'):
        cols = [0, UNSEEN, 5, 11]
    else:
        group = torch.argmax(model.assignments, dim=1).cpu().numpy()
        cols = sorted(set(np.flatnonzero(group == group[0]).tolist()) | ({UNSEEN} if case.endswith('masked') else set()))
    want = restatement(case, model, monkeypatch, columns=cols)[0]
    a, da = model.geodesic_deviation(x, v, dx, dv, columns=np.array(cols))
    assert torch.equal(a, model.geodesic_acceleration(x, v, columns=cols))
    err, scale = rel(num(da), want(num(x), num(v), num(dx), num(dv))[1])
    print('%s columns %s: max |da - restatement| %.3e of %.3e' % (case, cols, err, scale))
    assert err <= 1e-9 * max(scale, 1e-3)
    xs, v0 = x[:C].contiguous(), v[:C].contiguous()
    y = model.latent_exp_map(xs, v0, num_steps=STEPS, columns=cols)[:, -1].contiguous()
    got, _, curve, res = model.latent_log_map(xs, y, num_steps=STEPS, columns=cols)
    assert bool(torch.all(res <= 1e-10 * torch.clamp(y.norm(dim=1), min=1.0)))
    assert float(((got - v0).norm(dim=1) / v0.norm(dim=1)).max()) <= 1e-8
    with pytest.raises(AssertionError):
        model.geodesic_deviation(x, v, dx, dv, columns=[D])
    with pytest.raises(AssertionError):
        model.latent_log_map(xs, y[:3])
    with pytest.raises(AssertionError):
        model.latent_exp_map_tangent(x, v, dx[:, :2], dv)
    if case.endswith('masked') and not case.startswith('bgplvm'):            # the prior alone: a constant metric, straight lines
        a, da = model.geodesic_deviation(x, v, dx, dv, columns=[UNSEEN])
        assert torch.all(a == 0) and torch.all(da == 0)
        assert torch.equal(model.latent_log_map(xs, y, num_steps=4, columns=[UNSEEN])[0], y - xs)


@pytest.mark.parametrize('case', ['mrd', 'mrd masked'])
def test_mrd_views_and_total(case, monkeypatch):
    model, x, v = model_of(case), points(case), velocities(case)
    dx, dv = directions(case)
    both = model.geodesic_deviation(x, v, dx, dv)
    assert len(both) == 2
    xs, v0 = x[:C].contiguous(), v[:C].contiguous()
    for kw in (dict(views=[1]), dict(total=True), dict(views=[1], total=True)):
        want = restatement(case, model, monkeypatch, **kw)[0]
        out = model.geodesic_deviation(x, v, dx, dv, **kw)
        a, da = out if kw.get('total') else out[0]
        err, scale = rel(num(da), want(num(x), num(v), num(dx), num(dv))[1])
        print('%s %s: max |da - restatement| %.3e of %.3e' % (case, kw, err, scale))
        assert scale > 1e-3 and err <= 1e-9 * scale
        y = as_list(case, model.latent_exp_map(xs, v0, num_steps=STEPS, **kw), kw)[0][:, -1].contiguous()
        got, _, _, res = as_list(case, model.latent_log_map(xs, y, num_steps=STEPS, **kw), kw)[0]
        assert bool(torch.all(res <= 1e-10 * torch.clamp(y.norm(dim=1), min=1.0)))
        assert float(((got - v0).norm(dim=1) / v0.norm(dim=1)).max()) <= 1e-8
    assert torch.equal(model.geodesic_deviation(x, v, dx, dv, views=[1])[0][1], both[1][1])
    assert torch.equal(model.geodesic_deviation(x, v, dx, dv, views=[1], total=True)[1], both[1][1])
    with pytest.raises(AssertionError):
        model.latent_log_map(xs, xs, views=[2])


def test_a_first_shot_that_fails_to_factor_raises():
    def failing(per_pair):
        def accel_tangent(x, v, dx, dv):                                     # the second pair fails at every stage
            info = torch.as_tensor([0] * per_pair + [2] * per_pair, dtype=torch.int32, device=DEV)
            a = torch.where(info[:, None] != 0, torch.full_like(x, float('nan')), torch.zeros_like(x))
            return a, a, torch.zeros(2 * per_pair, dtype=torch.float64, device=DEV), info
        return accel_tangent

    with pytest.raises(FloatingPointError, match='1 of 2'):
        geodesic.log_map(failing(Q), np.zeros((2, Q)), np.ones((2, Q)), Q, DEV, 3)
    with pytest.raises(FloatingPointError, match='1 of 2'):
        geodesic.exp_map_tangent(failing(1), np.zeros((2, Q)), np.ones((2, Q)), np.zeros((2, Q)), np.ones((2, Q)), Q, DEV, 3)


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
        for name, args in (('geodesic_deviation', (x, x, x, x)), ('latent_exp_map_tangent', (x, x, x, x)), ('latent_log_map', (x, x))):
            with pytest.raises(AssertionError, match='%s is not built for a model sharded over a process group' % name):
                getattr(model, name)(*args)
    finally:
        if created:
            dist.destroy_process_group()
