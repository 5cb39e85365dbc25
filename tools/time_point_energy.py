# Timings of the curve-energy operator and of one latent_geodesic iteration on it, on one GPU.  HIP events, warm-up,
# medians of `reps` timings; a form's figure is the median of 7 repeats of that median with their min and max; the two forms of (a)
# take turns within every repeat.
#   python tools/time_point_energy.py [ops] [model]
# (a) ops:   ops.ard_rbf_point_energy against the torch composition that materialises k, a, c [K,N,M] (and d [K,N,M,Q]) and takes
#            W = C (p + p^T) by ops.matmul, at (K, N, M, Q) = (1, 3200, 128, 10), (8, 3200, 128, 10) and (512, 320, 128, 10)
#            (N = C S = 100 x 32 and 10 x 32 segments); the peak device memory of each form.
# (b) model: one iteration of latent_geodesic (one operator call on C S segments + the curve's element-wise work and the Adam
#            update) per model at N = 400, M = 50, D = 60, Q = 10, C = 10, S = 32: the time of 21 iterations less that of 1, over 20
#            (the training side is built once per call and drops out of the difference).
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm, dp_gp_lvm_t
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm, manifold_relevance_determination
dev = torch.device('cuda', 0)
f64 = dict(dtype=torch.float64, device=dev)
what = set(sys.argv[1:]) or {'ops', 'model'}


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
    d = x[None, :, None, :] - z[:, None, :, :]                                                     # [K, N, M, Q]
    g = gamma[:, None, None, :]
    kv = alpha[:, None, None] * torch.exp(-0.5 * torch.sum(g * d * d, dim=-1))                     # [K, N, M]
    a = torch.sum(g * d * v[None, :, None, :], dim=-1)
    c = -kv * a
    w = ops.matmul(c, p + p.transpose(1, 2))                                                       # [K, N, M]
    u = w * kv
    e = 0.5 * torch.sum(w * c, dim=-1)
    dx = gamma[:, None, :] * (torch.einsum('knm,knmq->knq', u * a, d) - v[None] * torch.sum(u, dim=-1, keepdim=True))
    dv = -gamma[:, None, :] * torch.einsum('knm,knmq->knq', u, d)
    return e, dx, dv


def peak_mb(fn):
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 1e6


rng = np.random.default_rng(0)
if 'ops' in what:
    for k, n, m, q in ((1, 3200, 128, 10), (8, 3200, 128, 10), (512, 320, 128, 10)):
        sc = 1.0 / np.sqrt(q)
        z = torch.as_tensor(sc * rng.standard_normal((k, m, q)), **f64)
        x, v = (torch.as_tensor(sc * rng.standard_normal((n, q)), **f64) for _ in range(2))
        gam, al = torch.as_tensor(rng.uniform(0.2, 3.0, (k, q)), **f64), torch.ones(k, **f64)
        p = torch.as_tensor(rng.standard_normal((k, m, m)), **f64)
        fused = lambda: ops.ard_rbf_point_energy(z, x, v, gam, al, p)
        comp = lambda: composed(z, x, v, gam, al, p)
        a, b = fused(), comp()
        err = max(float((s - t).abs().max() / t.abs().max()) for s, t in zip(a, b))
        del a, b
        res = alternate(dict(fused=fused, composition=comp), reps=9 if k < 512 else 5)
        print('K=%d N=%d M=%d Q=%d: fused %.3f ms [%.3f, %.3f], composition %.3f ms [%.3f, %.3f], ratio %.2f (largest relative '
              'difference %.1e); peak device memory: fused %.1f MB, composition %.1f MB'
              % ((k, n, m, q) + res['fused'] + res['composition'] + (res['composition'][0] / res['fused'][0], err,
                                                                     peak_mb(fused), peak_mb(comp))), flush=True)

if 'model' in what:
    n, d, m, q, c, s = 400, 60, 50, 10, 10, 32
    y = np.tanh(rng.standard_normal((n, 3))) @ rng.standard_normal((3, d)) + 0.3 * rng.standard_normal((n, d))
    kw = dict(num_latent_dims=q, num_inducing_points=m, device=dev, precision='f64')
    models = (('bayesian_gp_lvm', lambda: bayesian_gp_lvm(y, **kw)),
              ('manifold_relevance_determination (2 views, total)', lambda: manifold_relevance_determination([y[:, :30], y[:, 30:]], **kw)),
              ('dp_gp_lvm (T = 5)', lambda: dp_gp_lvm(y, truncation_level=5, **kw)),
              ('dp_gp_lvm_t (T = 5)', lambda: dp_gp_lvm_t(y, truncation_level=5, **kw)))
    for name, make in models:
        model = make()
        xm = model.q_x[0].detach()
        a, b = xm[:c].contiguous(), xm[c:2 * c].contiguous()
        extra = dict(total=True) if name.startswith('manifold') else {}
        run = lambda its: model.latent_geodesic(a, b, num_segments=s, num_iterations=its, **extra)
        run(1); run(21)
        per = []
        for _ in range(7):
            t1, t21 = float(np.median(timings_ms(lambda: run(1), 3))), float(np.median(timings_ms(lambda: run(21), 3)))
            per.append((t21 - t1) / 20.0)
        print('%s: one latent_geodesic iteration, C=%d S=%d, N=%d M=%d D=%d Q=%d: %.3f ms [%.3f, %.3f]'
              % (name, c, s, n, m, d, q, float(np.median(per)), min(per), max(per)), flush=True)
