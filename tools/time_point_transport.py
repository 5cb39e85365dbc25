# Timings of the parallel-transport operators and of latent_parallel_transport on them, on one GPU.  The protocol of
# tools/time_point_tangent.py: HIP events, warm-up, medians of `reps` timings; a form's figure is the median of 7 repeats of that
# median with their min and max; the forms of one comparison take turns within every repeat.
#   python tools/time_point_transport.py [ops] [accel] [model]
# (a) ops:   ops.ard_rbf_point_transport at F = 1, 5, Q against ops.ard_rbf_point_christoffel alone on the same inputs and against
#            the route it replaces, F calls of ops.ard_rbf_point_christoffel_tangent(dx = 0, dv = w_r), at (K, N, M) = (1, 3200, 128),
#            (8, 3200, 128), (512, 320, 128), Q = 10 and Q = 7, and at F = Q = 15, 23, 31 (QT = 2, 3, 4) at (8, 320, 128).
# (b) accel: ops.geodesic_transport against ops.geodesic_accel and F calls of ops.geodesic_accel_tangent(dg = 0, dgam = 2 tgam_r).
# (c) model: one latent_parallel_transport(num_steps=64) call per model at N = 400, M = 50, D = 60, Q = 10, C = 10, F = 1 and 10,
#            beside latent_exp_map on the same curves in the same run.
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm, dp_gp_lvm_t
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm, manifold_relevance_determination
dev = torch.device('cuda', 0)
f64 = dict(dtype=torch.float64, device=dev)
what = set(sys.argv[1:]) or {'ops', 'accel', 'model'}


def timings_ms(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def alternate(forms, warmup=2, reps=9, repeats=7):
    """{name: (median of the repeats' medians, min, max)} in milliseconds; the forms take turns within every repeat."""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    meds = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            meds[k].append(float(np.median(timings_ms(fn, reps))))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in meds.items()}


def fmt(r):
    return '%.3f ms [%.3f, %.3f]' % r


rng = np.random.default_rng(0)
if 'ops' in what:
    # the family's shapes at Q = 10 and 7, then full frames at the tile counts QT = 2, 3, 4 (W = 31, 47, 63), where one point per
    # workgroup forms all of d(v, w_r) in one wave
    shapes = [(k, n, m, q, (1, 5, q)) for q in (10, 7) for k, n, m in ((1, 3200, 128), (8, 3200, 128), (512, 320, 128))]
    shapes += [(8, 320, 128, q, (q,)) for q in (15, 23, 31)]
    for k, n, m, q, fs in shapes:
        sc = 1.0 / np.sqrt(q)
        z = torch.as_tensor(sc * rng.standard_normal((k, m, q)), **f64)
        x, v = (torch.as_tensor(sc * rng.standard_normal((n, q)), **f64) for _ in range(2))
        zero = torch.zeros((n, q), **f64)
        gam, al = torch.as_tensor(rng.uniform(0.2, 3.0, (k, q)), **f64), torch.ones(k, **f64)
        p = torch.as_tensor(rng.standard_normal((k, m, m)), **f64)
        chris = lambda: ops.ard_rbf_point_christoffel(z, x, v, gam, al, p)
        for f in fs:
            w = torch.as_tensor(sc * rng.standard_normal((n, f, q)), **f64)
            cols = [w[:, r].contiguous() for r in range(f)]
            fused = lambda: ops.ard_rbf_point_transport(z, x, v, w, gam, al, p)
            calls = lambda: [ops.ard_rbf_point_christoffel_tangent(z, x, v, zero, c, gam, al, p) for c in cols]
            a, b = fused(), calls()
            err = max(float((2.0 * a[2][:, :, r] - b[r][3]).abs().max() / b[r][3].abs().max()) for r in range(f))
            del a, b
            res = alternate(dict(fused=fused, christoffel=chris, calls=calls), reps=9 if k < 512 else 5)
            print('K=%d N=%d M=%d Q=%d F=%d (W = %d): transport %s, christoffel alone %s (transport / christoffel %.2f), %d tangent '
                  'calls %s (transport / tangent calls %.2f; largest relative difference %.1e)'
                  % (k, n, m, q, f, q + 1 + f, fmt(res['fused']), fmt(res['christoffel']), res['fused'][0] / res['christoffel'][0], f,
                     fmt(res['calls']), res['fused'][0] / res['calls'][0], err), flush=True)

if 'accel' in what:
    for k, n, q in ((1, 3200, 10), (8, 3200, 10), (512, 320, 10), (8, 3200, 7), (8, 3200, 31)):
        g = torch.as_tensor(0.1 * rng.standard_normal((k, n, q, q)), **f64)
        g = 0.5 * (g + g.transpose(2, 3)).contiguous()
        gam, v = torch.as_tensor(rng.standard_normal((k, n, q)), **f64), torch.as_tensor(rng.standard_normal((n, q)), **f64)
        prior = torch.full((q,), 4.0 * np.sqrt(k * q), **f64)
        zero = torch.zeros_like(g)
        plain = lambda: ops.geodesic_accel(g, gam, prior, v)
        for f in (1, 5, q):
            tgam = torch.as_tensor(rng.standard_normal((k, n, f, q)), **f64)
            twice = [(2.0 * tgam[:, :, r]).contiguous() for r in range(f)]
            fused = lambda: ops.geodesic_transport(g, gam, tgam, prior, v)
            calls = lambda: [ops.geodesic_accel_tangent(g, gam, zero, t, prior, v) for t in twice]
            a, b = fused(), plain()
            assert int(a[3].abs().max()) == 0 and torch.equal(a[0], b[0]) and torch.equal(a[2], b[1])
            res = alternate(dict(fused=fused, plain=plain, calls=calls))
            print('K=%d N=%d Q=%d F=%d: geodesic_transport %s, geodesic_accel %s (ratio %.2f), %d geodesic_accel_tangent calls %s '
                  '(transport / tangent calls %.2f)' % (k, n, q, f, fmt(res['fused']), fmt(res['plain']), res['fused'][0] / res['plain'][0],
                                                        f, fmt(res['calls']), res['fused'][0] / res['calls'][0]), flush=True)

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
        a, v = xm[:c].contiguous(), 0.5 * (xm[c:2 * c] - xm[:c]).contiguous()
        extra = dict(total=True) if name.startswith('manifold') else {}
        forms = dict(exp=lambda: model.latent_exp_map(a, v, num_steps=64, **extra))
        for f in (1, 10):
            w = torch.as_tensor(rng.standard_normal((c, f, q)), **f64)
            forms['F%d' % f] = (lambda w: lambda: model.latent_parallel_transport(a, v, w, num_steps=64, **extra))(w)
        res = alternate(forms, warmup=1, reps=3)
        print('%s: C=%d, N=%d M=%d D=%d Q=%d, 64 steps: latent_exp_map %s; latent_parallel_transport F=1 %s (%.2f of the exp map), '
              'F=10 %s (%.2f)' % (name, c, n, m, d, q, fmt(res['exp']), fmt(res['F1']), res['F1'][0] / res['exp'][0], fmt(res['F10']),
                                  res['F10'][0] / res['exp'][0]), flush=True)
