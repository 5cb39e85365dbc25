# scratch: training bayesian_gp_lvm on data with missing entries (observed=...): the parameter adjoint of the weighted Psi
# statistics (ops.qx_psi_param_adjoint) alone beside qx_psi_adjoint(weights=) and qx_psi_stats_batched(weights=), one optimise()
# iteration of the masked model with P row patterns beside one of the unmasked precision='f64' model, and the zero-weight skip.
# HIP events, warm-up, medians of >= 15 repeats.  A per-iteration figure is (T(12 iterations) - T(4 iterations)) / 8.
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm
dev = torch.device('cuda', 0)
f64 = dict(dtype=torch.float64, device=dev)


def median_ms(fn, warmup=3, reps=15):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def op_case(b, n, m, q, rng):
    z = torch.as_tensor(rng.standard_normal((b, m, q)), **f64)
    gam, al = torch.full((b, q), 0.5, **f64), torch.ones(b, **f64)
    mu, s = torch.as_tensor(rng.standard_normal((n, q)), **f64), torch.ones(n, q, **f64)
    g1, g2 = torch.as_tensor(rng.standard_normal((b, n, m)), **f64), torch.as_tensor(rng.standard_normal((b, m, m)), **f64)
    return z, mu, s, gam, al, g1, g2, ops.qx_pair_factor(z, gam, al)


def three_ops_us(w, b, n, m, q, rng):
    z, mu, s, gam, al, g1, g2, zf = op_case(b, n, m, q, rng)
    par = median_ms(lambda: ops.qx_psi_param_adjoint(z, mu, s, gam, al, g1, g2, zf, weights=w), warmup=5, reps=20)
    adj = median_ms(lambda: ops.qx_psi_adjoint(z, mu, s, gam, al, g1, g2, zf, weights=w), warmup=5, reps=20)
    st = median_ms(lambda: ops.qx_psi_stats_batched(z, mu, s, gam, al, zf, weights=w), warmup=5, reps=20)
    return par * 1e3, adj * 1e3, st * 1e3


def pattern_mask(n, d, p, rng):
    pats = [np.ones(n, dtype=bool)]
    while len(pats) < p:
        cand = rng.random(n) >= 0.3
        if not any(np.array_equal(cand, o) for o in pats):
            pats.append(cand)
    return np.stack([pats[c % p] for c in range(d)], axis=1)


rng = np.random.default_rng(0)
for b, n, m, q in ((1, 100, 50, 10), (60, 200, 50, 10), (1, 2000, 128, 10), (16, 2000, 128, 10)):
    w = torch.ones(b, n, **f64) if b == 1 else torch.as_tensor((rng.random((b, n)) >= 0.3).astype(np.float64), **f64).contiguous()
    print('operators B=%d N=%d M=%d Q=%d: param adjoint %.1f us, (mu, S) adjoint %.1f us, stats %.1f us'
          % ((b, n, m, q) + three_ops_us(w, b, n, m, q, rng)), flush=True)
b, n, m, q = 64, 500, 128, 10
blocks = torch.as_tensor(np.tile(((np.arange(n) // 32) % 2 == 0).astype(np.float64), (b, 1)), **f64).contiguous()
for name, w in (('weights=None', None), ('all ones', torch.ones(b, n, **f64)), ('50 % zeros in alternating blocks of 32 rows', blocks)):
    print('zero-weight skip B=%d N=%d M=%d Q=%d, %s: param adjoint %.1f us, (mu, S) adjoint %.1f us, stats %.1f us'
          % ((b, n, m, q, name) + three_ops_us(w, b, n, m, q, rng)), flush=True)
n, d, m, q = 2000, 512, 128, 10
y = np.tanh(rng.standard_normal((n, 3))) @ rng.standard_normal((3, d)) + 0.3 * rng.standard_normal((n, d))


def per_iteration(make):
    t = {}
    for k in (4, 12):
        def run():
            make().optimise(k, learning_rate=1e-3)
        t[k] = median_ms(run, warmup=2, reps=15)
    return (t[12] - t[4]) / 8.0


print('unmasked precision=f64 N=%d D=%d M=%d Q=%d: %.3f ms per optimise() iteration'
      % (n, d, m, q, per_iteration(lambda: bayesian_gp_lvm(y, num_latent_dims=q, num_inducing_points=m, device=dev, precision='f64'))),
      flush=True)
for p in (1, 16):
    obs = pattern_mask(n, d, p, rng)
    y_nan = np.where(obs, y, np.nan)
    print('masked P=%d patterns N=%d D=%d M=%d Q=%d: %.3f ms per optimise() iteration'
          % (p, n, d, m, q, per_iteration(lambda: bayesian_gp_lvm(y_nan, num_latent_dims=q, num_inducing_points=m, device=dev,
                                                                  observed=obs))), flush=True)
