"""GPU tests of parallel_transport_rate / latent_parallel_transport / latent_transport_to on bayesian_gp_lvm, MRD, dp_gp_lvm and
dp_gp_lvm_t, each trained on complete data and with a 30 % random mask (one column never observed): the models, points and
recorder of tests/test_gpu_latent_metric.py (N = 40, D = 12, M = 9, Q = 3, T = 3, N* = 7), the velocities of
tests/test_gpu_latent_exp_map.py and a frame of F = 2 vectors per point.  The rate is pinned to a NumPy restatement built column by
column from the model's own marginals._Marginals pieces and to half of geodesic_deviation's da along (0, w); the transported
frames to the NumPy RK4 of tests/test_point_transport_refs.py on that restatement, to the exponential map's bits, and to what
parallel transport keeps: the frame's Gram matrix under latent_metric, and the way back."""
import os

import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models import geodesic, marginals
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
from test_gpu_latent_exp_map import as_list, restated_gam, velocities
from test_gpu_latent_metric import CASES, D, DEV, M, N_T, Q, T, UNSEEN, Recorder, data, features, model_of, points, restated
from test_point_transport_refs import check_transport_fourth_order, rk4_transport_ref

pytestmark = pytest.mark.gpu
STEPS = 16
F = 2
C = 4                                                            # pairs per transport_to call


def frame(case, f=F):
    return torch.as_tensor(0.5 * np.random.default_rng(45).standard_normal((N_T, f, Q)), device=DEV)


def num(t):
    return t.cpu().numpy()


def rel(have, want):
    return float(np.max(np.abs(have - want))), float(np.max(np.abs(want)))


# ---- the NumPy restatement, column by column -----------------------------------------------------------------------------------------
def restated_tgam(marg, x, v, w, cols=None, weights=None):
    """[N*, Q]: test_gpu_latent_exp_map.restated_gam with d(v, w) = k [(u . v) (u . w) - sum_q gamma_q v_q w_q], u = gamma (x - z), in
    the place of d(v, v): the Christoffel symbol of test_gpu_latent_metric.restated's metric contracted with v and w [N*, Q]."""
    z, gamma, alpha, c, r, gidx = (a.detach().cpu().numpy() for a in (marg.z, marg.gamma, marg.alpha, marg.c, marg.r, marg.gidx))
    cols = range(r.shape[2]) if cols is None else cols
    out = np.zeros_like(x)
    for k in range(z.shape[0]):
        b = features(z[k], x, gamma[k], alpha[k])                                 # [N*, M, Q]
        diff = x[:, None, :] - z[k][None]
        kv = alpha[k] * np.exp(-0.5 * np.sum(gamma[k] * diff * diff, axis=-1))
        dvw = kv * (np.sum(gamma[k] * diff * v[:, None, :], axis=-1) * np.sum(gamma[k] * diff * w[:, None, :], axis=-1)
                    - np.sum(gamma[k] * v * w, axis=-1)[:, None])                  # [N*, M]
        for d in cols:
            wt = 1.0 if weights is None else weights[k, d]
            out += wt * np.einsum('nmq,m->nq', b, r[k, :, d]) * (dvw @ r[k, :, d])[:, None]
            if gidx[k, d] >= 0:
                out -= wt * np.einsum('nmq,mp,np->nq', b, c[k, gidx[k, d]], dvw)
    return out


def restatement(case, model, monkeypatch, **kw):
    """The callables (x, v [N, Q], w [N, F, Q]) -> (a, dw) in NumPy of model.parallel_transport_rate(., ., ., **kw), one per returned
    entry, from the pieces that the model builds inside one call (the branches of test_gpu_latent_exp_map.restatement)."""
    rec = Recorder(monkeypatch)
    model.parallel_transport_rate(points(case), velocities(case), frame(case), **kw)
    monkeypatch.undo()
    kind, masked = case.split()[0], case.endswith('masked')
    cols = kw.get('columns')

    def of(parts, extra=None):
        def transport(x, v, w):
            g = sum(restated(m, x, c, wt) for m, c, wt in parts) + (0.0 if extra is None else extra)
            gam = sum(restated_gam(m, x, v, c, wt) for m, c, wt in parts)
            tgam = np.stack([sum(restated_tgam(m, x, v, w[:, r], c, wt) for m, c, wt in parts) for r in range(w.shape[1])], axis=1)
            return -np.linalg.solve(g, gam[:, :, None])[:, :, 0], -np.linalg.solve(g[:, None], tgam[..., None])[..., 0]
        return transport

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


# ---- the rate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_rate_is_the_restatement_and_half_the_deviation_along_the_vector(case, monkeypatch):
    model, x, v, w = model_of(case), points(case), velocities(case), frame(case)
    want = restatement(case, model, monkeypatch)
    have = as_list(case, model.parallel_transport_rate(x, v, w))
    plain = as_list(case, model.geodesic_acceleration(x, v))
    zero = torch.zeros_like(x)
    dev = [as_list(case, model.geodesic_deviation(x, v, zero, w[:, r].contiguous())) for r in range(F)]
    assert len(have) == len(want)
    for i, ((a, dw), t, p) in enumerate(zip(have, want, plain)):
        assert tuple(dw.shape) == (N_T, F, Q) and dw.dtype == torch.float64 and dw.is_cuda
        assert torch.equal(a, p)                                             # geodesic_acceleration's bits
        err, scale = rel(num(dw), t(num(x), num(v), num(w))[1])
        half = torch.stack([0.5 * dev[r][i][1] for r in range(F)], dim=1)
        err_d, scale_d = float((dw - half).abs().max()), float(half.abs().max())
        print('%s: max |dw - restatement| %.3e of %.3e, |dw - da / 2| %.3e of %.3e' % (case, err, scale, err_d, scale_d))
        assert scale > 1e-3 and err <= 1e-9 * scale and err_d <= 1e-9 * scale_d
    # one vector per point, and one point with numpy inputs: the same bits
    for r in range(F):
        for (a1, dw1), (a, dw) in zip(as_list(case, model.parallel_transport_rate(x, v, w[:, r])), have):
            assert tuple(dw1.shape) == (N_T, Q) and torch.equal(a1, a) and torch.equal(dw1, dw[:, r])
    for (a1, dw1), (a, dw) in zip(as_list(case, model.parallel_transport_rate(num(x[2]), num(v[2]), num(w[2, 1]))), have):
        assert tuple(dw1.shape) == (Q,) and torch.equal(a1, a[2]) and torch.equal(dw1, dw[2, 1])


# ---- the transport -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_transport_is_the_numpy_rk4_on_the_exp_maps_curve(case, monkeypatch):
    model, x, v, w = model_of(case), points(case), velocities(case), frame(case)
    want = restatement(case, model, monkeypatch)
    have = as_list(case, model.latent_parallel_transport(x, v, w, num_steps=STEPS, return_curve=True))
    ends = as_list(case, model.latent_parallel_transport(x, v, w, num_steps=STEPS))
    plain = as_list(case, model.latent_exp_map(x, v, num_steps=STEPS, return_velocity=True))
    own = as_list(case, model.latent_parallel_transport(x, v, v, num_steps=STEPS, return_curve=True))
    rng = np.random.default_rng(46)
    w2 = torch.as_tensor(0.5 * rng.standard_normal((N_T, F, Q)), device=DEV)
    two = as_list(case, model.latent_parallel_transport(x, v, w2, num_steps=STEPS))
    both = as_list(case, model.latent_parallel_transport(x, v, 2.5 * w - w2, num_steps=STEPS))
    batch = as_list(case, model.latent_parallel_transport(x, v, w[:, 1], num_steps=STEPS))
    single = as_list(case, model.latent_parallel_transport(x[3], num(v[3]), w[3, 1], num_steps=STEPS, return_curve=True))
    for (c, u, fr), e, (pc, pu), (oc, ou, ofr), t2, tb, b1, (c1, u1, f1), t in zip(have, ends, plain, own, two, both, batch, single, want):
        assert tuple(fr.shape) == (N_T, STEPS + 1, F, Q) and fr.dtype == torch.float64 and fr.is_cuda
        assert torch.equal(c, pc) and torch.equal(u, pu)                     # latent_exp_map's bits
        assert torch.equal(fr[:, 0], w) and torch.equal(e, fr[:, -1])        # row 0: the bits of w
        assert tuple(ofr.shape) == (N_T, STEPS + 1, Q) and torch.equal(ofr, ou) and torch.equal(ou, pu)    # w = v: the velocity
        _, _, rf = rk4_transport_ref(t, num(x), num(v), num(w), STEPS)
        err, scale = rel(num(fr), rf)
        moved = float((fr[:, -1] - w).abs().max())
        lin, lin_scale = float((tb - (2.5 * e - t2)).abs().max()), float(e.abs().max())
        print('%s: |frames - rk4| %.3e of %.3e; the frame moves by %.3e; linearity %.3e of %.3e' % (case, err, scale, moved, lin, lin_scale))
        assert err <= 1e-9 * max(1.0, scale) and moved > 1e-4 and lin <= 1e-10 * lin_scale
        assert tuple(b1.shape) == (N_T, Q) and torch.equal(b1, fr[:, -1, 1])                     # one vector per curve: its row of a frame
        assert tuple(f1.shape) == (STEPS + 1, Q) and torch.equal(f1, fr[3, :, 1]) and torch.equal(c1, c[3]) and torch.equal(u1, u[3])


@pytest.mark.parametrize('case', CASES)
def test_transport_keeps_the_gram_matrix_and_comes_back_at_fourth_order(case):
    """The Gram drift under the model's own latent_metric and the return error fall by >= 8 when the steps double, at the
    velocities of the exponential map's tests: there the integrator is in its asymptotic range (the drift's ratios over 4, 8, 16, 32
    steps tend to 16 on every case: DESIGN.md 7.31; at twice these velocities they wander between 5 and 60, next-order terms of
    either sign), and both figures at 16 steps stay above 1e-10 of their scale (smallest: 1.0e-9 and 8.0e-10)."""
    model = model_of(case)
    kw = dict(total=True) if case.startswith('mrd') else {}
    t = lambda a: torch.as_tensor(np.array(a, dtype=np.float64), device=DEV)

    def shoot(x, v, w, s):
        return tuple(num(o) for o in model.latent_parallel_transport(t(x), t(v), t(w), num_steps=s, return_curve=True, **kw))

    metric = lambda x: num(model.latent_metric(t(x), **kw))
    check_transport_fourth_order(shoot, metric, num(points(case)), num(velocities(case)), num(frame(case)))


@pytest.mark.parametrize('case', CASES)
def test_transport_to_is_the_log_map_and_then_the_transport(case):
    model = model_of(case)
    x, v0, w = points(case)[:C].contiguous(), velocities(case)[:C].contiguous(), frame(case)[:C].contiguous()
    kw = dict(total=True) if case.startswith('mrd') else {}
    y = model.latent_exp_map(x, v0, num_steps=STEPS, **kw)[:, -1].contiguous()
    v, dist, _, res = model.latent_log_map(x, y, num_steps=STEPS, **kw)
    moved, v1, dist1, res1 = model.latent_transport_to(x, y, w, num_steps=STEPS, **kw)
    assert torch.equal(v1, v) and torch.equal(dist1, dist) and torch.equal(res1, res)
    assert bool(torch.all(res <= 1e-10 * torch.clamp(y.norm(dim=1), min=1.0)))
    assert torch.equal(moved, model.latent_parallel_transport(x, v, w, num_steps=STEPS, **kw))
    end = model.latent_exp_map(x, v, num_steps=STEPS, return_velocity=True, **kw)[1][:, -1]
    assert torch.equal(model.latent_transport_to(x, y, v, num_steps=STEPS, **kw)[0], end)       # log_a(b) arrives as the end velocity
    if not case.startswith('mrd'):                                          # one pair, one vector: its row of the batch
        each = model.latent_transport_to(x[2], num(y[2]), w[2, 0], num_steps=STEPS)
        assert tuple(each[0].shape) == (Q,) and torch.equal(each[0], moved[2, 0]) and torch.equal(each[1], v[2])


# ---- the model surface -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['over_d', 'over_d masked', 'over_t', 'over_t masked', 'bgplvm masked'])
def test_columns_of_one_group(case, monkeypatch):
    model, x, v, w = model_of(case), points(case), velocities(case), frame(case)
    if case.startswith('bgplvm'):
        cols = [0, UNSEEN, 5, 11]
    else:
        group = torch.argmax(model.assignments, dim=1).cpu().numpy()
        cols = sorted(set(np.flatnonzero(group == group[0]).tolist()) | ({UNSEEN} if case.endswith('masked') else set()))
    want = restatement(case, model, monkeypatch, columns=cols)[0]
    a, dw = model.parallel_transport_rate(x, v, w, columns=np.array(cols))
    assert torch.equal(a, model.geodesic_acceleration(x, v, columns=cols))
    err, scale = rel(num(dw), want(num(x), num(v), num(w))[1])
    print('%s columns %s: max |dw - restatement| %.3e of %.3e' % (case, cols, err, scale))
    assert err <= 1e-9 * max(scale, 1e-3)
    c, u, fr = model.latent_parallel_transport(x, v, w, num_steps=STEPS, columns=cols, return_curve=True)
    assert torch.equal(c, model.latent_exp_map(x, v, num_steps=STEPS, columns=cols))
    err, scale = rel(num(fr), rk4_transport_ref(want, num(x), num(v), num(w), STEPS)[2])
    assert err <= 1e-9 * max(1.0, scale)
    with pytest.raises(AssertionError):
        model.parallel_transport_rate(x, v, w, columns=[D])
    with pytest.raises(AssertionError):
        model.latent_parallel_transport(x, v, w[:3])
    with pytest.raises(AssertionError):
        model.latent_parallel_transport(x, v, w[:, :, :2])
    with pytest.raises(AssertionError):
        model.latent_parallel_transport(x[0], v[0], w[:1])
    if case.endswith('masked') and not case.startswith('bgplvm'):            # the prior alone: a flat metric, the frame keeps its bits
        a, dw = model.parallel_transport_rate(x, v, w, columns=[UNSEEN])
        assert torch.all(a == 0) and torch.all(dw == 0) and tuple(dw.shape) == (N_T, F, Q)
        c, u, fr = model.latent_parallel_transport(x, v, w, num_steps=4, columns=[UNSEEN], return_curve=True)
        assert torch.equal(fr, w[:, None].expand(N_T, 5, F, Q)) and torch.equal(u[:, -1], v)
        y = (x + v)[:C].contiguous()
        moved, v1, _, _ = model.latent_transport_to(x[:C], y, w[:C], num_steps=4, columns=[UNSEEN])
        assert torch.equal(moved, w[:C]) and torch.equal(v1, y - x[:C])


@pytest.mark.parametrize('case', ['mrd', 'mrd masked'])
def test_mrd_views_and_total(case, monkeypatch):
    model, x, v, w = model_of(case), points(case), velocities(case), frame(case)
    both = model.parallel_transport_rate(x, v, w)
    assert len(both) == 2
    for kw in (dict(views=[1]), dict(total=True), dict(views=[1], total=True)):
        want = restatement(case, model, monkeypatch, **kw)[0]
        out = model.parallel_transport_rate(x, v, w, **kw)
        a, dw = out if kw.get('total') else out[0]
        err, scale = rel(num(dw), want(num(x), num(v), num(w))[1])
        print('%s %s: max |dw - restatement| %.3e of %.3e' % (case, kw, err, scale))
        assert scale > 1e-3 and err <= 1e-9 * scale
        fr = as_list(case, model.latent_parallel_transport(x, v, w, num_steps=STEPS, **kw), kw)[0]
        err, scale = rel(num(fr), rk4_transport_ref(want, num(x), num(v), num(w), STEPS)[2][:, -1])
        assert err <= 1e-9 * max(1.0, scale)
    assert torch.equal(model.parallel_transport_rate(x, v, w, views=[1])[0][1], both[1][1])
    assert torch.equal(model.parallel_transport_rate(x, v, w, views=[1], total=True)[1], both[1][1])
    with pytest.raises(AssertionError):
        model.latent_parallel_transport(x, v, w, views=[2])


@pytest.mark.parametrize('case', ['bgplvm', 'mrd masked', 'over_d masked', 'over_t'])
def test_the_integrator_on_the_device_leaves_the_transports_bits(case):
    model = model_of(case)
    x, v, w = points(case)[:C].contiguous(), velocities(case)[:C].contiguous(), frame(case)[:C].contiguous()
    kw = dict(total=True) if case.startswith('mrd') else {}
    y = model.latent_exp_map(x, v, num_steps=STEPS, **kw)[:, -1].contiguous()
    assert model.integrator == 'host'
    host = model.latent_parallel_transport(x, v, w, num_steps=STEPS, return_curve=True, **kw), model.latent_transport_to(x, y, w, num_steps=STEPS, **kw)
    try:
        model.integrator = 'device'
        device = model.latent_parallel_transport(x, v, w, num_steps=STEPS, return_curve=True, **kw), model.latent_transport_to(x, y, w, num_steps=STEPS, **kw)
    finally:
        model.integrator = 'host'
    for hs, ds in zip(host, device):
        for h, d in zip(hs, ds):
            assert torch.equal(h, d)


@pytest.mark.parametrize('case', ['bgplvm', 'mrd masked', 'over_d masked', 'over_t'])
def test_blocks_of_points_leave_every_bit(case, monkeypatch):
    """Metric.block = 3 (accel's points per block): transport's share of it is 3 (Q^2 + Q) // (Q^2 + Q + F Q) = 2 points per block
    at F = 2 and 1 at F = 7, so the N* = 7 points go through 4 and 7 blocks, w sliced and dw concatenated."""
    model, x, v = model_of(case), points(case), velocities(case)
    kw = dict(total=True) if case.startswith('mrd') else {}
    frames = [frame(case), frame(case, 7)]
    whole = [(model.parallel_transport_rate(x, v, w, **kw), model.latent_parallel_transport(x, v, w, num_steps=4, return_curve=True, **kw))
             for w in frames]
    init, calls, sizes = marginals.Metric.__init__, [], []

    def small(self, *a, **k):
        init(self, *a, **k)
        self.block = 3
        calls.append(self)

    inner = ops.geodesic_transport

    def counted(g, *a, **k):
        sizes.append(g.shape[1])
        return inner(g, *a, **k)
    monkeypatch.setattr(marginals.Metric, '__init__', small)
    monkeypatch.setattr(ops, 'geodesic_transport', counted)
    for w, (rate, moved), per in zip(frames, whole, (2, 1)):
        del sizes[:]
        for have, want in zip(model.parallel_transport_rate(x, v, w, **kw), rate):
            assert torch.equal(have, want)
        assert sizes == [per] * (N_T // per) + [N_T % per] * (N_T % per > 0)
        for have, want in zip(model.latent_parallel_transport(x, v, w, num_steps=4, return_curve=True, **kw), moved):
            assert torch.equal(have, want)
    assert len(calls) >= 4 and all(m.block == 3 for m in calls)


def test_a_failed_factorisation_raises_once_at_the_end():
    def transport(x, v, w):                                                   # the second curve fails at every stage
        info = torch.as_tensor([0, 2], dtype=torch.int32, device=DEV)
        a = torch.where(info[:, None] != 0, torch.full_like(x, float('nan')), torch.zeros_like(x))
        return a, a[:, None, :].expand_as(w), torch.zeros(2, dtype=torch.float64, device=DEV), info

    with pytest.raises(FloatingPointError, match='latent_parallel_transport.*1 of 2'):
        geodesic.parallel_transport(transport, np.zeros((2, Q)), np.ones((2, Q)), np.ones((2, F, Q)), Q, DEV, 3)


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
        for name, args in (('parallel_transport_rate', (x, x, x)), ('latent_parallel_transport', (x, x, x)),
                           ('latent_transport_to', (x, x, x))):
            with pytest.raises(AssertionError, match='%s is not built for a model sharded over a process group' % name):
                getattr(model, name)(*args)
    finally:
        if created:
            dist.destroy_process_group()
