# Timings of the integrators on the device against the host integrators they sit behind, on one GPU.  Medians of
# `reps` timings; a form's figure is the median of 7 repeats of that median with their min and max; the two forms of a comparison
# take turns within every repeat.
#   python tools/time_geodesic_shoot.py [ops] [model]
# (a) ops:   ops.geodesic_shoot / ops.geodesic_shoot_tangent against the host composition (models/geodesic._rk4 / _rk4_tangent on
#            ops.ard_rbf_point_christoffel[_tangent] and ops.geodesic_accel[_tangent]) at (sum K, C, M, Q, S) = (1, 10, 50, 10, 64),
#            (60, 10, 50, 10, 64), (8, 100, 128, 10, 64), the tangent also at C = 100 (the rows of a Newton shot); HIP events.  Both
#            forms are checked to give the same bits first.
# (b) model: latent_exp_map(num_steps=64), one Newton iteration of latent_log_map (the time of max_iterations = 3 less that of 1, over
#            2, at tol = 0: every iteration is made) and one latent_log_map(num_steps=64) call per model at N = 400, M = 50, D = 60,
#            Q = 10, C = 10, model.integrator = 'device' against 'host'; wall clock around a device synchronise.
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models import geodesic
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm, dp_gp_lvm_t
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm, manifold_relevance_determination
dev = torch.device('cuda', 0)
f64 = dict(dtype=torch.float64, device=dev)
what = set(sys.argv[1:]) or {'ops', 'model'}


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def alternate(forms, timer, warmup=2, reps=3, repeats=7):
    """{name: (median of the repeats' medians, min, max)} in milliseconds; the forms take turns within every repeat."""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    meds = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            meds[k].append(float(np.median([timer(fn) for _ in range(reps)])))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in meds.items()}


def fmt(r):
    return '%.3f ms [%.3f, %.3f]' % r


def verdict(res):
    host, device = res['host'], res['device']
    return 'host / device %.2f, ranges %s' % (host[0] / device[0], 'apart' if device[2] < host[1] else 'OVERLAP' if device[1] <= host[2]
                                               else 'apart, the device route SLOWER')


rng = np.random.default_rng(0)
if 'ops' in what:
    for tangent, shapes in ((False, ((1, 10, 50, 10, 64), (60, 10, 50, 10, 64), (8, 100, 128, 10, 64))),
                            (True, ((1, 10, 50, 10, 64), (60, 10, 50, 10, 64), (8, 100, 128, 10, 64), (1, 100, 50, 10, 64),
                                    (60, 100, 50, 10, 64)))):
        for k, c, m, q, s in shapes:
            sc = 1.0 / np.sqrt(q)
            a = rng.standard_normal((k, m, m))
            z = torch.as_tensor(1.5 * sc * rng.standard_normal((k, m, q)), **f64)
            gam, al = torch.as_tensor(rng.uniform(0.5, 1.5, (k, q)), **f64), torch.ones(k, **f64)
            p = torch.as_tensor(0.15 * (20.0 / m) / np.sqrt(k) * (a + a.transpose(0, 2, 1)), **f64)
            prior = torch.as_tensor(rng.uniform(4.0, 6.0, q), **f64)
            n = 4 if tangent else 2
            state = [torch.as_tensor(w * sc * rng.standard_normal((c, q)), **f64) for w in (0.5, 1.0, 0.5, 0.5)[:n]]
            parts = [(z, gam, al, p)]
            if tangent:
                accel = lambda x, v, dx, dv: ops.geodesic_accel_tangent(*ops.ard_rbf_point_christoffel_tangent(z, x, v, dx, dv, gam, al, p), prior, v)
                host = lambda: geodesic._rk4_tangent(accel, *state, s)
                device = lambda: ops.geodesic_shoot_tangent(parts, prior, *state, s)
            else:
                accel = lambda x, v: ops.geodesic_accel(*ops.ard_rbf_point_christoffel(z, x, v, gam, al, p), prior, v)
                host = lambda: geodesic._rk4(accel, *state, s)
                device = lambda: ops.geodesic_shoot(parts, prior, *state, s)
            h, d = host(), device()
            assert all(torch.equal(t, u) for t, u in zip(h, d)) and not bool(d[-2 if tangent else -1].any())
            del h, d
            res = alternate(dict(host=host, device=device), event_ms)
            print('%s sum K=%d C=%d M=%d Q=%d S=%d: device %s (%.4f ms per stage), host composition %s; %s'
                  % ('geodesic_shoot_tangent' if tangent else 'geodesic_shoot', k, c, m, q, s, fmt(res['device']),
                     res['device'][0] / (4 * s), fmt(res['host']), verdict(res)), flush=True)

if 'model' in what:
    n, d, m, q, c = 400, 60, 50, 10, 10
    y = np.tanh(rng.standard_normal((n, 3))) @ rng.standard_normal((3, d)) + 0.3 * rng.standard_normal((n, d))
    kw = dict(num_latent_dims=q, num_inducing_points=m, device=dev, precision='f64')
    models = (('bayesian_gp_lvm', lambda: bayesian_gp_lvm(y, **kw)),
              ('manifold_relevance_determination (2 views, total)', lambda: manifold_relevance_determination([y[:, :30], y[:, 30:]], **kw)),
              ('dp_gp_lvm (T = 5)', lambda: dp_gp_lvm(y, truncation_level=5, **kw)),
              ('dp_gp_lvm_t (T = 5)', lambda: dp_gp_lvm_t(y, truncation_level=5, **kw)))
    for name, make in models:
        model = make()
        xm = model.q_x[0].detach()
        a, v0 = xm[:c].contiguous(), 0.5 * (xm[c:2 * c] - xm[:c]).contiguous()
        extra = dict(total=True) if name.startswith('manifold') else {}

        def under(i, fn):
            model.integrator = i
            try:
                return fn()
            finally:
                model.integrator = 'host'

        exp = lambda i: under(i, lambda: model.latent_exp_map(a, v0, num_steps=64, **extra))
        b = exp('host')[:, -1].contiguous()
        assert torch.equal(exp('device'), exp('host'))
        log = lambda i, its, tol: under(i, lambda: model.latent_log_map(a, b, num_steps=64, max_iterations=its, tol=tol, **extra))
        full = log('device', 20, 1e-10)
        assert all(torch.equal(t, u) for t, u in zip(full, log('host', 20, 1e-10)))
        res = alternate({i: (lambda i=i: exp(i)) for i in ('host', 'device')}, wall_ms)
        print('%s: C=%d, N=%d M=%d D=%d Q=%d: latent_exp_map(num_steps=64) device %s, host %s; %s'
              % (name, c, n, m, d, q, fmt(res['device']), fmt(res['host']), verdict(res)), flush=True)
        shots = {i: [] for i in ('host', 'device')}
        for i in shots:
            log(i, 1, 0.0)
        for _ in range(7):
            for i in shots:
                t1 = float(np.median([wall_ms(lambda: log(i, 1, 0.0)) for _ in range(3)]))
                t3 = float(np.median([wall_ms(lambda: log(i, 3, 0.0)) for _ in range(3)]))
                shots[i].append((t3 - t1) / 2.0)
        res = {i: (float(np.median(t)), min(t), max(t)) for i, t in shots.items()}
        print('%s: one Newton iteration (a shot of 64 steps over C Q = %d rows) device %s, host %s; %s'
              % (name, c * q, fmt(res['device']), fmt(res['host']), verdict(res)), flush=True)
        res = alternate({i: (lambda i=i: log(i, 20, 1e-10)) for i in ('host', 'device')}, wall_ms)
        print('%s: latent_log_map(num_steps=64) device %s, host %s; %s; largest end residual %.1e'
              % (name, fmt(res['device']), fmt(res['host']), verdict(res), float(full[3].max())), flush=True)
