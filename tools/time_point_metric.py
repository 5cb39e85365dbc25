# Timings of the latent-metric operator and of the models' latent_metric on it, on one GPU.  HIP events, warm-up,
# medians of `reps` timings; a form's figure is the median of 7 repeats of that median with their min and max; the two forms of (a)
# take turns within every repeat.
#   python tools/time_point_metric.py [ops] [model]
# (a) ops:   ops.ard_rbf_point_metric against the composition that materialises the derivative features B [K,N,M,Q] with torch and
#            contracts them with ops.matmul (p B, then B_n^T (p B)_n per point), at (K, N, M, Q) = (1, 10000, 128, 10),
#            (8, 2500, 128, 10) and (512, 500, 128, 10); for the last shape also the peak device memory of each form.
# (b) model: latent_metric of every model on a 100 x 100 grid through two latent dimensions at N = 400, M = 50, D = 60, Q = 10
#            (the training side included: it is built once per call).
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


def composed(z, x, gamma, alpha, p):
    k, m, q = z.shape
    n = x.shape[0]
    d = x[None, :, None, :] - z[:, None, :, :]                                                     # [K, N, M, Q]
    kv = alpha[:, None, None] * torch.exp(-0.5 * torch.sum(gamma[:, None, None, :] * d * d, dim=-1))
    b = -gamma[:, None, None, :] * d * kv[..., None]
    u = ops.matmul(p, b.permute(0, 2, 1, 3).reshape(k, m, n * q))                                  # p B [K, M, (n, q')]
    u = u.view(k, m, n, q).permute(0, 2, 1, 3).reshape(k * n, m, q)
    return ops.matmul(b.view(k * n, m, q).transpose(1, 2), u).view(k, n, q, q)


def peak_mb(fn):
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 1e6


rng = np.random.default_rng(0)
if 'ops' in what:
    for k, n, m, q in ((1, 10000, 128, 10), (8, 2500, 128, 10), (512, 500, 128, 10)):
        z = torch.as_tensor(rng.standard_normal((k, m, q)), **f64)
        x = torch.as_tensor(rng.standard_normal((n, q)), **f64)
        gam, al = torch.as_tensor(rng.uniform(0.2, 1.0, (k, q)), **f64), torch.ones(k, **f64)
        p = torch.as_tensor(rng.standard_normal((k, m, m)), **f64)
        fused = lambda: ops.ard_rbf_point_metric(z, x, gam, al, p)
        comp = lambda: composed(z, x, gam, al, p)
        a, b = fused(), comp()
        err = float((a - b).abs().max() / b.abs().max())
        del a, b
        res = alternate(dict(fused=fused, composition=comp), reps=9 if k < 512 else 5)
        mem = ''
        if k == 512:
            mem = '; peak device memory: fused %.0f MB, composition %.0f MB' % (peak_mb(fused), peak_mb(comp))
        print('K=%d N=%d M=%d Q=%d: fused %.3f ms [%.3f, %.3f], composition %.3f ms [%.3f, %.3f], ratio %.2f (largest relative '
              'difference %.1e; B alone %.0f MB)%s'
              % ((k, n, m, q) + res['fused'] + res['composition'] + (res['composition'][0] / res['fused'][0], err,
                                                                     8e-6 * k * n * m * q, mem)), flush=True)

if 'model' in what:
    n, d, m, q, side = 400, 60, 50, 10, 100
    y = np.tanh(rng.standard_normal((n, 3))) @ rng.standard_normal((3, d)) + 0.3 * rng.standard_normal((n, d))
    kw = dict(num_latent_dims=q, num_inducing_points=m, device=dev, precision='f64')
    axis = np.linspace(-2.0, 2.0, side)
    grid = np.zeros((side * side, q))
    grid[:, 0], grid[:, 1] = np.repeat(axis, side), np.tile(axis, side)
    xg = torch.as_tensor(grid, **f64)
    models = (('bayesian_gp_lvm', lambda: bayesian_gp_lvm(y, **kw)),
              ('manifold_relevance_determination (2 views, total)', lambda: manifold_relevance_determination([y[:, :30], y[:, 30:]], **kw)),
              ('dp_gp_lvm (T = 5)', lambda: dp_gp_lvm(y, truncation_level=5, **kw)),
              ('dp_gp_lvm_t (T = 5)', lambda: dp_gp_lvm_t(y, truncation_level=5, **kw)))
    for name, make in models:
        model = make()
        fn = (lambda: model.latent_metric(xg, total=True)) if name.startswith('manifold') else (lambda: model.latent_metric(xg))
        fn(); fn()
        v = [float(np.median(timings_ms(fn, 3))) for _ in range(7)]
        print('%s: latent_metric on a %d x %d grid, N=%d M=%d D=%d Q=%d: %.2f ms [%.2f, %.2f]'
              % (name, side, side, n, m, d, q, float(np.median(v)), min(v), max(v)), flush=True)
