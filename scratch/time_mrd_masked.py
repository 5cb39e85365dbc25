# scratch: the batched gram-gradient contraction (ops.ard_rbf_gram_grad_batched) beside a host loop of B single-kernel calls
# (ops.ard_rbf_gram_grad, unchanged code), and one optimise() iteration of manifold_relevance_determination(observed=...) with
# P row patterns per view beside one of the unmasked precision='f64' model of the same shape.
# HIP events, warm-up, medians of >= 15 repeats, one process.  A per-iteration figure is T(8 iterations) / 8 on a built model.
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models.gaussian_process import manifold_relevance_determination
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


rng = np.random.default_rng(0)
for b, n, q in ((3, 50, 10), (20, 50, 10), (4, 128, 10), (512, 128, 10)):
    x = torch.as_tensor(rng.standard_normal((b, n, q)), **f64)
    gam, al = torch.as_tensor(rng.uniform(0.2, 1.0, (b, q)), **f64), torch.as_tensor(rng.uniform(0.5, 2.0, b), **f64)
    w = torch.as_tensor(rng.standard_normal((b, n, n)), **f64)
    gs, als = [gam[i:i + 1] for i in range(b)], [al[i:i + 1] for i in range(b)]

    def loop():
        return [ops.ard_rbf_gram_grad(x[i], gs[i], als[i], w[i]) for i in range(b)]
    got, ref = ops.ard_rbf_gram_grad_batched(x, gam, al, w), loop()
    err = max(float((got[k][i] - ref[i][k]).abs().max() / ref[i][k].abs().max()) for i in range(b) for k in range(3))
    # the two alternate: batched, loop, batched, loop
    t = [[], []]
    for _ in range(2):
        t[0].append(median_ms(lambda: ops.ard_rbf_gram_grad_batched(x, gam, al, w), warmup=5, reps=20))
        t[1].append(median_ms(loop, warmup=3, reps=20 if b <= 20 else 15))
    print('gram grad B=%d N=%d Q=%d: batched %.1f us, loop of %d calls %.1f us (x %.1f); largest relative difference %.1e'
          % (b, n, q, min(t[0]) * 1e3, b, min(t[1]) * 1e3, min(t[1]) / min(t[0]), err), flush=True)

nv, n, d, m, q = 3, 2000, 64, 128, 10
lat = np.tanh(rng.standard_normal((n, 3)))
views = [lat @ rng.standard_normal((3, d)) + 0.3 * rng.standard_normal((n, d)) for _ in range(nv)]


def pattern_mask(p):
    pats = [np.ones(n, dtype=bool)] + [rng.random(n) >= 0.3 for _ in range(p - 1)]
    return np.stack([pats[c % p] for c in range(d)], axis=1)


def per_iteration(model):
    return median_ms(lambda: model.optimise(8, learning_rate=1e-3), warmup=2, reps=15) / 8.0


np.random.seed(0)
plain = manifold_relevance_determination(views, num_latent_dims=q, num_inducing_points=m, device=dev, precision='f64')
print('unmasked precision=f64 V=%d N=%d D_v=%d M=%d Q=%d: %.3f ms per optimise() iteration' % (nv, n, d, m, q, per_iteration(plain)),
      flush=True)
del plain
for p in (1, 8):
    obs = [pattern_mask(p) for _ in range(nv)]
    np.random.seed(0)
    model = manifold_relevance_determination([np.where(o, y, np.nan) for o, y in zip(obs, views)], num_latent_dims=q,
                                             num_inducing_points=m, device=dev, observed=obs)
    print('masked P=%d patterns per view (%d slots) V=%d N=%d D_v=%d M=%d Q=%d: %.3f ms per optimise() iteration'
          % (p, model.objective_terms.shape[0] if model.objective_terms is not None else nv * p, nv, n, d, m, q,
             per_iteration(model)), flush=True)
