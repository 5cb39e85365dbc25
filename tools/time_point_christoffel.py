# Timings of the geodesic-equation operators and of latent_exp_map on them, on one GPU.  HIP events, warm-up,
# medians of `reps` timings; a form's figure is the median of 7 repeats of that median with their min and max; the forms of one
# comparison take turns within every repeat.
#   python tools/time_point_christoffel.py [ops] [accel] [model]
# (a) ops:   ops.ard_rbf_point_christoffel against ops.ard_rbf_point_metric alone on the same inputs (the new kernel carries one
#            more feature column: (Q + 1) / Q of the matrix work, a whole extra column tile at Q = 16) and against the composition
#            that materialises k, B [K,N,M,Q] and d [K,N,M] with torch and contracts with ops.matmul, at (K, N, M) = (1, 3200, 128),
#            (8, 3200, 128), (512, 320, 128), Q = 10 and 16; the peak device memory of each form.
# (b) accel: ops.geodesic_accel against the torch composition it replaces (sum over K, + diag, cholesky, cholesky_solve, the speed).
# (c) model: one RK4 step of latent_exp_map (the time of 5 steps less that of 1, over 4: the training side drops out) and one
#            latent_exp_map(num_steps=64) call per model at N = 400, M = 50, D = 60, Q = 10, C = 10.
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


def composed(z, x, v, gamma, alpha, p):
    k, m, q = z.shape
    n = x.shape[0]
    d = x[None, :, None, :] - z[:, None, :, :]                                                     # [K, N, M, Q]
    g = gamma[:, None, None, :]
    kv = alpha[:, None, None] * torch.exp(-0.5 * torch.sum(g * d * d, dim=-1))                     # [K, N, M]
    a = torch.sum(g * d * v[None, :, None, :], dim=-1)
    dd = kv * (a * a - torch.sum(gamma[:, None, :] * v[None] * v[None], dim=-1)[:, :, None])
    f = torch.cat([-g * d * kv[..., None], dd[..., None]], dim=-1)                                 # [B | d]: [K, N, M, Q + 1]
    u = ops.matmul(p, f.permute(0, 2, 1, 3).reshape(k, m, n * (q + 1)))                            # p F [K, M, (n, w)]
    u = u.view(k, m, n, q + 1).permute(0, 2, 1, 3).reshape(k * n, m, q + 1)
    out = ops.matmul(f[..., :q].reshape(k * n, m, q).transpose(1, 2), u).view(k, n, q, q + 1)
    return out[..., :q].contiguous(), out[..., q].contiguous()


def composed_accel(g, gam, prior, v):
    big = torch.sum(g, dim=0) + torch.diag(prior)
    l, info = torch.linalg.cholesky_ex(big)
    a = -torch.cholesky_solve(torch.sum(gam, dim=0)[:, :, None], l)[:, :, 0]
    return a, torch.einsum('nq,nqr,nr->n', v, big, v), info


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
    for q in (10, 16):
        for k, n, m in ((1, 3200, 128), (8, 3200, 128), (512, 320, 128)):
            sc = 1.0 / np.sqrt(q)
            z = torch.as_tensor(sc * rng.standard_normal((k, m, q)), **f64)
            x, v = (torch.as_tensor(sc * rng.standard_normal((n, q)), **f64) for _ in range(2))
            gam, al = torch.as_tensor(rng.uniform(0.2, 3.0, (k, q)), **f64), torch.ones(k, **f64)
            p = torch.as_tensor(rng.standard_normal((k, m, m)), **f64)
            fused = lambda: ops.ard_rbf_point_christoffel(z, x, v, gam, al, p)
            metric = lambda: ops.ard_rbf_point_metric(z, x, gam, al, p)
            comp = lambda: composed(z, x, v, gam, al, p)
            a, b = fused(), comp()
            err = max(float((s - t).abs().max() / t.abs().max()) for s, t in zip(a, b))
            del a, b
            res = alternate(dict(fused=fused, metric=metric, composition=comp), reps=9 if k < 512 else 5)
            print('K=%d N=%d M=%d Q=%d: christoffel %s, metric alone %s (christoffel / metric %.2f), composition %s (composition / '
                  'christoffel %.2f; largest relative difference %.1e); peak device memory: christoffel %.1f MB, composition %.1f MB'
                  % (k, n, m, q, fmt(res['fused']), fmt(res['metric']), res['fused'][0] / res['metric'][0], fmt(res['composition']),
                     res['composition'][0] / res['fused'][0], err, peak_mb(fused), peak_mb(comp)), flush=True)

if 'accel' in what:
    for k, n, q in ((1, 3200, 10), (8, 3200, 10), (512, 320, 10), (8, 3200, 3), (8, 3200, 63)):
        g = torch.as_tensor(0.1 * rng.standard_normal((k, n, q, q)), **f64)
        g = 0.5 * (g + g.transpose(2, 3)).contiguous()
        gam, v = torch.as_tensor(rng.standard_normal((k, n, q)), **f64), torch.as_tensor(rng.standard_normal((n, q)), **f64)
        prior = torch.full((q,), 4.0 * np.sqrt(k * q), **f64)
        fused = lambda: ops.geodesic_accel(g, gam, prior, v)
        comp = lambda: composed_accel(g, gam, prior, v)
        a, b = fused(), comp()
        assert int(a[2].abs().max()) == 0 and int(b[2].abs().max()) == 0
        err = float((a[0] - b[0]).abs().max() / b[0].abs().max())
        res = alternate(dict(fused=fused, composition=comp))
        print('K=%d N=%d Q=%d: geodesic_accel %s, torch composition %s, ratio %.2f (largest relative difference %.1e)'
              % (k, n, q, fmt(res['fused']), fmt(res['composition']), res['composition'][0] / res['fused'][0], err), flush=True)

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
        a, b = xm[:c].contiguous(), 0.5 * (xm[c:2 * c] - xm[:c]).contiguous()
        extra = dict(total=True) if name.startswith('manifold') else {}
        run = lambda steps: model.latent_exp_map(a, b, num_steps=steps, **extra)
        run(1); run(5)
        per, whole = [], []
        for _ in range(7):
            t1, t5 = float(np.median(timings_ms(lambda: run(1), 3))), float(np.median(timings_ms(lambda: run(5), 3)))
            per.append((t5 - t1) / 4.0)
            whole.append(float(np.median(timings_ms(lambda: run(64), 3))))
        print('%s: C=%d, N=%d M=%d D=%d Q=%d: one RK4 step (4 stages) %.3f ms [%.3f, %.3f]; latent_exp_map(num_steps=64) %.3f ms '
              '[%.3f, %.3f]' % (name, c, n, m, d, q, float(np.median(per)), min(per), max(per), float(np.median(whole)), min(whole),
                               max(whole)), flush=True)
