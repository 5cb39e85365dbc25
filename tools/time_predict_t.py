# Timings of the over-T model's prediction paths on one GPU.  HIP events, warm-up, medians of 15 timings; the
# spread of a form is min to max of 7 repeats of that median; the two forms of (a) take turns within every repeat.
#   python tools/time_predict_t.py [ops] [model]
# (a) ops:   ops.qx_psi_pointwise against the composition of what existed before it: every test point's Psi2 term materialised
#            as [K,N,M,M] with torch (one exponential per element, direct differences), then two einsum contractions.
# (b) model: one optimise_test_latents iteration ((T(12 iterations) - T(4 iterations)) / 8) and one predict_missing_data call.
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm_t
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


def alternate(forms, warmup=3, reps=15, repeats=7):
    """{name: (median of the repeats' medians, min, max)} in microseconds; the forms take turns within every repeat."""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    meds = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            meds[k].append(float(np.median(timings_ms(fn, reps))) * 1e3)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in meds.items()}


def composed(z, mu, s, gam, al, zf, c, r):
    """tr, quad from psi2_kn [K,N,M,M] in memory (the exponent as a sum over q of [K,N,M,M] terms: no [K,N,M,M,Q] array)."""
    k, m, q = z.shape
    zbar = 0.5 * (z[:, :, None, :] + z[:, None, :, :])                                       # [K,M,M,Q]
    w2 = 2.0 * gam[:, None, :] * s[None] + 1.0                                               # [K,N,Q]
    e = torch.zeros((k, mu.shape[0], m, m), **f64)
    for i in range(q):
        d = mu[None, :, None, None, i] - zbar[:, None, :, :, i]
        e += (gam[:, i, None] / w2[:, :, i])[:, :, None, None] * d * d
    psi2n = zf[:, None] * torch.exp(-e - 0.5 * torch.log(w2).sum(-1)[:, :, None, None])
    return torch.einsum('kgab,knab->kng', c, psi2n), torch.einsum('kaj,knab,kbj->knj', r, psi2n, r)


rng = np.random.default_rng(0)
if 'ops' in what:
    for k, g, j, m, q, n in ((4, 4, 60, 50, 10, 100), (8, 16, 512, 128, 10, 500)):
        z = torch.as_tensor(rng.standard_normal((k, m, q)), **f64)
        gam, al = torch.full((k, q), 0.5, **f64), torch.ones(k, **f64)
        mu, s = torch.as_tensor(rng.standard_normal((n, q)), **f64), torch.ones(n, q, **f64)
        c, r = torch.as_tensor(rng.standard_normal((k, g, m, m)), **f64), torch.as_tensor(rng.standard_normal((k, m, j)), **f64)
        zf = ops.qx_pair_factor(z, gam, al)
        a, b = ops.qx_psi_pointwise(z, mu, s, gam, al, c, r, zfac=zf), composed(z, mu, s, gam, al, zf, c, r)
        err = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(a, b))
        res = alternate(dict(operator=lambda: ops.qx_psi_pointwise(z, mu, s, gam, al, c, r, zfac=zf),
                             composition=lambda: composed(z, mu, s, gam, al, zf, c, r)))
        print('K=%d G=%d J=%d M=%d Q=%d N=%d: operator %.1f us [%.1f, %.1f], composition %.1f us [%.1f, %.1f], ratio %.1f '
              '(largest relative difference %.1e; psi2_kn alone %.0f MB)'
              % ((k, g, j, m, q, n) + res['operator'] + res['composition'] + (res['composition'][0] / res['operator'][0], err,
                                                                              8e-6 * k * n * m * m)), flush=True)


def pattern_mask(n, d, p, rng):
    pats = []
    while len(pats) < p:
        cand = rng.random(n) >= 0.3
        if cand.any() and not any(np.array_equal(cand, o) for o in pats):
            pats.append(cand)
    return np.stack([pats[c % p] for c in range(d)], axis=1)


if 'model' in what:
    for n, n_t, d, m, q, t_, pats in ((400, 100, 60, 50, 10, 5, (4, 60)), (2000, 500, 512, 128, 10, 8, (16,))):
        y = np.tanh(rng.standard_normal((n + n_t, 3))) @ rng.standard_normal((3, d)) + 0.3 * rng.standard_normal((n + n_t, d))
        model = dp_gp_lvm_t(y[:n], num_latent_dims=q, num_inducing_points=m, truncation_level=t_, device=dev, precision='f64')
        for p in pats:
            obs = pattern_mask(n_t, d, p, rng)
            y_nan = np.where(obs, y[n:], np.nan)
            xm, xv = model.optimise_test_latents(y_nan, 2, observed=obs)
            t = {}
            for it in (4, 12):
                run = lambda: model.optimise_test_latents(y_nan, it, x_test_mean=xm, x_test_var=xv, observed=obs)
                run(); run()
                t[it] = float(np.median(timings_ms(run, 9)))
            pred = lambda: model.predict_missing_data(y_nan, x_test_mean=xm, x_test_var=xv, observed=obs)
            marg = lambda: model.predictive_marginals(xm, xv)
            pred(); marg()
            print('N*=%d M=%d T=%d D=%d, %d test patterns: optimise_test_latents %.3f ms per iteration; predict_missing_data %.2f ms; '
                  'predictive_marginals (all %d columns) %.2f ms'
                  % (n_t, m, t_, d, p, (t[12] - t[4]) / 8.0, float(np.median(timings_ms(pred, 9))), d,
                     float(np.median(timings_ms(marg, 9)))), flush=True)
