# Timings of the geodesic-tangent operators and of latent_log_map on them, on one GPU.  The protocol of
# tools/time_point_christoffel.py: HIP events, warm-up, medians of `reps` timings; a form's figure is the median of 7 repeats of that
# median with their min and max; the forms of one comparison take turns within every repeat.
#   python tools/time_point_tangent.py [ops] [accel] [model]
# (a) ops:   ops.ard_rbf_point_christoffel_tangent against ops.ard_rbf_point_christoffel alone on the same inputs, against TWO
#            christoffel calls (what a central difference costs per direction) and against the composition that materialises k, B, d,
#            dB [K,N,M,Q] and dd [K,N,M] with torch and contracts with ops.matmul, at (K, N, M) = (1, 3200, 128), (8, 3200, 128),
#            (512, 320, 128), Q = 10 (QT = 2, NP = 2) and Q = 7 (QT = 1, NP = 8); the peak device memory of each form.
# (b) accel: ops.geodesic_accel_tangent against ops.geodesic_accel.
# (c) model: one Newton iteration of latent_log_map (the time of max_iterations = 3 less that of 1, over 2, at tol = 0: every
#            iteration is made) and one latent_log_map(num_steps=64) call per model at N = 400, M = 50, D = 60, Q = 10, C = 10.
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


def composed(z, x, v, dx, dv, gamma, alpha, p):
    k, m, q = z.shape
    n = x.shape[0]
    d = x[None, :, None, :] - z[:, None, :, :]                                                     # [K, N, M, Q]
    g = gamma[:, None, None, :]
    u = g * d
    kv = alpha[:, None, None] * torch.exp(-0.5 * torch.sum(u * d, dim=-1))                         # [K, N, M]
    a, e, f = (torch.sum(u * w[None, :, None, :], dim=-1) for w in (v, dx, dv))
    s, c1, c2 = (torch.sum(gamma[:, None, :] * (w1 * w2)[None], dim=-1)[:, :, None] for w1, w2 in ((v, v), (dx, v), (v, dv)))
    dd = kv * (a * a - s)
    ddd = kv * (2.0 * a * (c1 + f) - e * (a * a - s) - 2.0 * c2)
    db = kv[..., None] * (e[..., None] * u - g * dx[None, :, None, :])
    w = 2 * q + 2
    feat = torch.cat([-u * kv[..., None], dd[..., None], db, ddd[..., None]], dim=-1)              # [B | d | dB | dd]: [K, N, M, W]
    pf = ops.matmul(p, feat.permute(0, 2, 1, 3).reshape(k, m, n * w))                              # p F [K, M, (n, w)]
    pf = pf.view(k, m, n, w).permute(0, 2, 1, 3).reshape(k * n, m, w)
    out = ops.matmul(feat.reshape(k * n, m, w).transpose(1, 2), pf).view(k, n, w, w)
    return (out[:, :, :q, :q].contiguous(), out[:, :, :q, q].contiguous(),
            out[:, :, :q, q + 1:w - 1] + out[:, :, q + 1:w - 1, :q], out[:, :, q + 1:w - 1, q] + out[:, :, :q, w - 1])


def peak_mb(fn):
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def fmt(r):
    return '%.3f ms [%.3f, %.3f]' % r


rng = np.random.default_rng(0)
if 'ops' in what:
    for q in (10, 7):
        for k, n, m in ((1, 3200, 128), (8, 3200, 128), (512, 320, 128)):
            sc = 1.0 / np.sqrt(q)
            z = torch.as_tensor(sc * rng.standard_normal((k, m, q)), **f64)
            x, v, dx, dv = (torch.as_tensor(sc * rng.standard_normal((n, q)), **f64) for _ in range(4))
            gam, al = torch.as_tensor(rng.uniform(0.2, 3.0, (k, q)), **f64), torch.ones(k, **f64)
            p = torch.as_tensor(rng.standard_normal((k, m, m)), **f64)
            fused = lambda: ops.ard_rbf_point_christoffel_tangent(z, x, v, dx, dv, gam, al, p)
            chris = lambda: ops.ard_rbf_point_christoffel(z, x, v, gam, al, p)
            twice = lambda: (ops.ard_rbf_point_christoffel(z, x, v, gam, al, p), ops.ard_rbf_point_christoffel(z, dx, dv, gam, al, p))
            comp = lambda: composed(z, x, v, dx, dv, gam, al, p)
            a, b = fused(), comp()
            err = max(float((s - t).abs().max() / t.abs().max()) for s, t in zip(a, b))
            del a, b
            res = alternate(dict(fused=fused, christoffel=chris, twice=twice, composition=comp), reps=9 if k < 512 else 5)
            print('K=%d N=%d M=%d Q=%d: tangent %s, christoffel alone %s (tangent / christoffel %.2f), two christoffel calls %s '
                  '(tangent / two calls %.2f), composition %s (composition / tangent %.2f; largest relative difference %.1e); peak '
                  'device memory: tangent %.1f MB, composition %.1f MB'
                  % (k, n, m, q, fmt(res['fused']), fmt(res['christoffel']), res['fused'][0] / res['christoffel'][0],
                     fmt(res['twice']), res['fused'][0] / res['twice'][0], fmt(res['composition']),
                     res['composition'][0] / res['fused'][0], err, peak_mb(fused), peak_mb(comp)), flush=True)

if 'accel' in what:
    for k, n, q in ((1, 3200, 10), (8, 3200, 10), (512, 320, 10), (8, 3200, 3), (8, 3200, 31)):
        g = torch.as_tensor(0.1 * rng.standard_normal((k, n, q, q)), **f64)
        g = 0.5 * (g + g.transpose(2, 3)).contiguous()
        gam, v = torch.as_tensor(rng.standard_normal((k, n, q)), **f64), torch.as_tensor(rng.standard_normal((n, q)), **f64)
        dg, dgam = torch.as_tensor(rng.standard_normal((k, n, q, q)), **f64), torch.as_tensor(rng.standard_normal((k, n, q)), **f64)
        prior = torch.full((q,), 4.0 * np.sqrt(k * q), **f64)
        fused = lambda: ops.geodesic_accel_tangent(g, gam, dg, dgam, prior, v)
        plain = lambda: ops.geodesic_accel(g, gam, prior, v)
        a, b = fused(), plain()
        assert int(a[3].abs().max()) == 0 and torch.equal(a[0], b[0]) and torch.equal(a[2], b[1])
        res = alternate(dict(fused=fused, plain=plain))
        print('K=%d N=%d Q=%d: geodesic_accel_tangent %s, geodesic_accel %s, ratio %.2f'
              % (k, n, q, fmt(res['fused']), fmt(res['plain']), res['fused'][0] / res['plain'][0]), flush=True)

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
        a = xm[:c].contiguous()
        extra = dict(total=True) if name.startswith('manifold') else {}
        b = model.latent_exp_map(a, 0.5 * (xm[c:2 * c] - xm[:c]).contiguous(), num_steps=64, **extra)[:, -1].contiguous()
        run = lambda its, tol: model.latent_log_map(a, b, num_steps=64, max_iterations=its, tol=tol, **extra)
        run(1, 0.0)
        res = run(20, 1e-10)[3]
        per, whole = [], []
        for _ in range(7):
            t1, t3 = float(np.median(timings_ms(lambda: run(1, 0.0), 3))), float(np.median(timings_ms(lambda: run(3, 0.0), 3)))
            per.append((t3 - t1) / 2.0)
            whole.append(float(np.median(timings_ms(lambda: run(20, 1e-10), 3))))
        print('%s: C=%d, N=%d M=%d D=%d Q=%d: one Newton iteration (a shot of 64 steps over C Q = %d rows) %.3f ms [%.3f, %.3f]; '
              'latent_log_map(num_steps=64) %.3f ms [%.3f, %.3f], largest end residual %.1e'
              % (name, c, n, m, d, q, c * q, float(np.median(per)), min(per), max(per), float(np.median(whole)), min(whole),
                 max(whole), float(res.max())), flush=True)
