# Timings of the joint-covariance operator and of one sample_functions call on it, on one GPU.  HIP events, warm-up,
# medians of `reps` timings; a form's figure is the median of 7 repeats of that median with their min and max; the two forms of (a)
# take turns within every repeat.
#   python tools/time_point_cov.py [ops] [model]
# (a) ops:   ops.ard_rbf_point_cov against the composition on the other operators: ops.ard_rbf_gram per kernel (its own z) for the
#            features [K,N,M], two ops.matmul (U = F c [K G,N,M], Q = U F^T [K G,N,N]), ops.ard_rbf_gram(x, None) for the prior and
#            the subtraction, at (K, G, N, M, Q) = (1, 1, 2000, 128, 10), (8, 16, 500, 128, 10) and (512, 1, 320, 128, 10); the
#            peak device memory of each form.  c is symmetric here (the composition uses it as given).
# (c) route: the fused operator against marginals.composed_covariance (the composition as the models take it: c symmetrised, the
#            result symmetrised) at the models' own layouts K = 1 | 5, G = 1 | 3, M = 50, Q = 10 over N* = 33 .. 2048: where
#            marginals.composed_is_faster draws its line.
# (b) model: one sample_functions call (S = 16) per model at N = 400, M = 50, D = 60, Q = 10, N* = 33 (the training side is built
#            inside the call, as in every call of the prediction methods).
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models import marginals
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm, dp_gp_lvm_t
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm, manifold_relevance_determination
dev = torch.device('cuda', 0)
f64 = dict(dtype=torch.float64, device=dev)
what = set(sys.argv[1:]) or {'ops', 'route', 'model'}


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


def composed(z, x, gamma, alpha, c):
    k, g = c.shape[0], c.shape[1]                        # (ard_rbf_gram takes a beta; without include_noise it is not used)
    feat = torch.stack([ops.ard_rbf_gram(x, z[i], gamma[i:i + 1], alpha[i:i + 1], alpha[i:i + 1])[0] for i in range(k)])    # [K, N, M]
    u = ops.matmul(feat[:, None].expand(-1, g, -1, -1).reshape(k * g, feat.shape[1], feat.shape[2]), c.reshape(k * g, *c.shape[2:]))
    quad = ops.matmul(u, feat.transpose(1, 2)[:, None].expand(-1, g, -1, -1).reshape(k * g, feat.shape[2], feat.shape[1]))
    prior = ops.ard_rbf_gram(x, None, gamma, alpha, alpha)                                                          # [K, N, N]
    return prior[:, None] - quad.reshape(k, g, *quad.shape[1:])


def peak_mb(fn):
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 1e6


rng = np.random.default_rng(0)
if 'ops' in what:
    for k, g, n, m, q in ((1, 1, 2000, 128, 10), (8, 16, 500, 128, 10), (512, 1, 320, 128, 10)):
        sc = 1.0 / np.sqrt(q)
        z = torch.as_tensor(sc * rng.standard_normal((k, m, q)), **f64)
        x = torch.as_tensor(sc * rng.standard_normal((n, q)), **f64)
        gam, al = torch.as_tensor(rng.uniform(0.2, 3.0, (k, q)), **f64), torch.ones(k, **f64)
        c = torch.as_tensor(rng.standard_normal((k, g, m, m)), **f64)
        c = (0.5 * (c + c.transpose(2, 3))).contiguous()
        fused = lambda: ops.ard_rbf_point_cov(z, x, gam, al, c)
        comp = lambda: composed(z, x, gam, al, c)
        a, b = fused(), comp()
        err = float((a - b).abs().max() / b.abs().max())
        del a, b
        res = alternate(dict(fused=fused, composition=comp), reps=9 if k < 512 else 5)
        print('K=%d G=%d N=%d M=%d Q=%d: fused %.3f ms [%.3f, %.3f], composition %.3f ms [%.3f, %.3f], ratio %.2f (largest relative '
              'difference %.1e); peak device memory: fused %.1f MB, composition %.1f MB'
              % ((k, g, n, m, q) + res['fused'] + res['composition'] + (res['composition'][0] / res['fused'][0], err,
                                                                        peak_mb(fused), peak_mb(comp))), flush=True)

if 'route' in what:
    m, q = 50, 10
    for k, g in ((1, 1), (1, 3), (5, 1), (5, 3), (16, 1)):
        for n in (33, 128, 256, 512, 1024, 2048):
            sc = 1.0 / np.sqrt(q)
            z = torch.as_tensor(sc * rng.standard_normal((k, m, q)), **f64)
            x = torch.as_tensor(sc * rng.standard_normal((n, q)), **f64)
            gam, al = torch.as_tensor(rng.uniform(0.2, 3.0, (k, q)), **f64), torch.ones(k, **f64)
            c = torch.as_tensor(rng.standard_normal((k, g, m, m)), **f64)
            res = alternate(dict(fused=lambda: ops.ard_rbf_point_cov(z, x, gam, al, c),
                                 composition=lambda: marginals.composed_covariance(z, x, gam, al, c)), reps=5, repeats=3)
            print('route K=%d G=%d N=%d M=%d Q=%d: fused %.3f ms [%.3f, %.3f], composition %.3f ms [%.3f, %.3f]'
                  % ((k, g, n, m, q) + res['fused'] + res['composition']), flush=True)

if 'model' in what:
    n, d, m, q, n_t, s = 400, 60, 50, 10, 33, 16
    y = np.tanh(rng.standard_normal((n, 3))) @ rng.standard_normal((3, d)) + 0.3 * rng.standard_normal((n, d))
    kw = dict(num_latent_dims=q, num_inducing_points=m, device=dev, precision='f64')
    models = (('bayesian_gp_lvm', lambda: bayesian_gp_lvm(y, **kw)),
              ('manifold_relevance_determination (2 views)', lambda: manifold_relevance_determination([y[:, :30], y[:, 30:]], **kw)),
              ('dp_gp_lvm (T = 5)', lambda: dp_gp_lvm(y, truncation_level=5, **kw)),
              ('dp_gp_lvm_t (T = 5)', lambda: dp_gp_lvm_t(y, truncation_level=5, **kw)))
    for name, make in models:
        model = make()
        xm = model.q_x[0].detach()
        w = torch.linspace(0.0, 1.0, n_t, **f64)[:, None]
        pts = (xm[0][None] + w * (xm[1] - xm[0])[None]).contiguous()
        run = lambda: model.sample_functions(pts, num_samples=s)
        cov = lambda: model.predictive_covariance(pts)
        res = alternate(dict(sample=run, covariance=cov), reps=5)
        print('%s: N*=%d S=%d, N=%d M=%d D=%d Q=%d: sample_functions %.3f ms [%.3f, %.3f], predictive_covariance %.3f ms '
              '[%.3f, %.3f]' % ((name, n_t, s, n, m, d, q) + res['sample'] + res['covariance']), flush=True)
