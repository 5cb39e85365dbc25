# Timings of the per-entry moments operator and of the model methods on it, on one GPU.  HIP events, warm-up,
# medians of 15 timings; the spread of a form is min to max of 7 repeats of that median; the two forms of (a) take turns within
# every repeat.
#   python tools/time_point_moments.py [ops] [model]
# (a) ops:   ops.qx_psi_point_moments against the composition of the operators that existed before it, as frozen_bound_t._MomentsT.at
#            composes them: ops.qx_psi_pointwise, ops.psi1 (Psi1* [K,N,M] in memory), ops.matmul, two gathers, element-wise work.
#            The condition of 7.12: the fused median is no greater than the largest of the composition's 7 repeats.
# (b) model: predictive_marginals and impute_training_data(return_variance=True) of a mask-trained bayesian_gp_lvm at the three
#            settings of 7.11 (training patterns in place of test patterns).
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm
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


def composed(z0, zk, mu, s, gam, al, be, zf, c, r, gidx):
    tr, quad = ops.qx_psi_pointwise(zk, mu, s, gam, al, c, r, zfac=zf)
    mean = ops.matmul(ops.psi1(z0, mu, s, gam, al), r)
    idx = gidx.long()
    seen = ((idx >= 0) & (idx < c.shape[1])).to(torch.float64)[:, None, :]
    tr_d = torch.gather(tr, 2, idx.clamp(0, c.shape[1] - 1)[:, None, :].expand(-1, mu.shape[0], -1)) * seen
    return mean, (al + 1.0 / be)[:, None, None] - tr_d + quad - mean * mean


rng = np.random.default_rng(0)
if 'ops' in what:
    for k, g, j, m, q, n in ((4, 4, 60, 50, 10, 100), (8, 16, 512, 128, 10, 500), (512, 1, 1, 128, 10, 500)):
        z0 = torch.as_tensor(rng.standard_normal((m, q)), **f64)                               # (shared by the kernels, as in the models)
        zk = z0[None].expand(k, -1, -1).contiguous()
        gam, al, be = torch.full((k, q), 0.5, **f64), torch.ones(k, **f64), torch.full((k,), 4.0, **f64)
        mu, s = torch.as_tensor(rng.standard_normal((n, q)), **f64), torch.ones(n, q, **f64)
        c, r = torch.as_tensor(rng.standard_normal((k, g, m, m)), **f64), torch.as_tensor(rng.standard_normal((k, m, j)), **f64)
        gidx = torch.as_tensor(rng.integers(0, g, (k, j)), dtype=torch.int32, device=dev)
        zf = ops.qx_pair_factor(zk, gam, al)
        fused = lambda: ops.qx_psi_point_moments(zk, mu, s, gam, al, c, r, gidx, be, zfac=zf)
        comp = lambda: composed(z0, zk, mu, s, gam, al, be, zf, c, r, gidx)
        err = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(fused(), comp()))
        res = alternate(dict(fused=fused, composition=comp))
        ok = res['fused'][0] <= res['composition'][2]
        print('K=%d G=%d J=%d M=%d Q=%d N=%d: fused %.1f us [%.1f, %.1f], composition %.1f us [%.1f, %.1f], ratio %.2f; fused median '
              '<= largest composition repeat: %s (largest relative difference %.1e; Psi1* alone %.1f MB)'
              % ((k, g, j, m, q, n) + res['fused'] + res['composition'] + (res['composition'][0] / res['fused'][0], ok, err,
                                                                          8e-6 * k * n * m)), flush=True)


def pattern_mask(n, d, p, rng):
    pats = []
    while len(pats) < p:
        cand = rng.random(n) >= 0.3
        if cand.any() and not any(np.array_equal(cand, o) for o in pats):
            pats.append(cand)
    return np.stack([pats[c % p] for c in range(d)], axis=1)


if 'model' in what:
    for n, n_t, d, m, q, pats in ((400, 100, 60, 50, 10, (4, 60)), (2000, 500, 512, 128, 10, (16,))):
        y = np.tanh(rng.standard_normal((n + n_t, 3))) @ rng.standard_normal((3, d)) + 0.3 * rng.standard_normal((n + n_t, d))
        for p in pats:
            obs = pattern_mask(n, d, p, rng)
            model = bayesian_gp_lvm(np.where(obs, y[:n], np.nan), num_latent_dims=q, num_inducing_points=m, device=dev, observed=obs)
            xm = torch.as_tensor(rng.standard_normal((n_t, q)), **f64)
            xv = torch.full((n_t, q), 0.5, **f64)
            marg = lambda: model.predictive_marginals(xm, xv)
            fill = lambda: model.impute_training_data()
            fill_v = lambda: model.impute_training_data(return_variance=True)
            marg(); fill(); fill_v()
            print('N=%d N*=%d M=%d D=%d, %d training patterns: predictive_marginals (all %d columns) %.2f ms; impute_training_data '
                  '%.2f ms, with return_variance=True %.2f ms'
                  % (n, n_t, m, d, p, d, float(np.median(timings_ms(marg, 9))), float(np.median(timings_ms(fill, 9))),
                     float(np.median(timings_ms(fill_v, 9)))), flush=True)
