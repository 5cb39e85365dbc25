# scratch: one q(X*) iteration of the prediction paths (bound gradient with respect to q(X*): qx_psi_stats_batched + the dense
# chain + qx_psi_adjoint) for bayesian_gp_lvm and a 20-view MRD at a horse-mocap-like shape (N=200, N*=100, D=60 in 3-dim views,
# M=50, Q=10) and at config-3 scale (N=2000, N*=500, D=512, M=128, Q=10), and the two operators' share, HIP events, warm-up,
# median of repeats.
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm, manifold_relevance_determination
dev = torch.device('cuda', 0)


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
for name, n, nt, d, m, q, views in (('bgplvm', 200, 100, 60, 50, 10, 1), ('mrd', 200, 100, 60, 50, 10, 20),
                                    ('bgplvm', 2000, 500, 512, 128, 10, 1)):
    y = np.tanh(rng.standard_normal((n + nt, 3))) @ rng.standard_normal((3, d)) + 0.3 * rng.standard_normal((n + nt, d))
    y_tr, y_te = y[:n], y[n:]
    if views == 1:
        model = bayesian_gp_lvm(y_tr, num_latent_dims=q, num_inducing_points=m, device=dev, precision='f64')
        obs = y_te
    else:
        dv = d // views
        model = manifold_relevance_determination([y_tr[:, i * dv:(i + 1) * dv] for i in range(views)], num_latent_dims=q,
                                                 num_inducing_points=m, device=dev, precision='f64')
        obs = [y_te[:, i * dv:(i + 1) * dv] for i in range(views)]
    xm = torch.as_tensor(rng.standard_normal((nt, q)), device=dev)
    xv = torch.ones(nt, q, dtype=torch.float64, device=dev)
    step = median_ms(lambda: model.optimise_test_latents(obs, 10, x_test_mean=xm, x_test_var=xv)) / 10.0
    b = views
    z = torch.as_tensor(rng.standard_normal((b, m, q)), device=dev)
    gam = torch.full((b, q), 0.5, dtype=torch.float64, device=dev)
    al = torch.ones(b, dtype=torch.float64, device=dev)
    zf = ops.qx_pair_factor(z, gam, al)
    g1 = torch.as_tensor(rng.standard_normal((b, nt, m)), device=dev)
    g2 = torch.as_tensor(rng.standard_normal((b, m, m)), device=dev)
    st = median_ms(lambda: ops.qx_psi_stats_batched(z, xm, xv, gam, al, zf), warmup=5, reps=50)
    adj = median_ms(lambda: ops.qx_psi_adjoint(z, xm, xv, gam, al, g1, g2, zf), warmup=5, reps=50)
    print('%s N=%d N*=%d D=%d M=%d Q=%d B=%d: %.3f ms per optimise_test_latents iteration; qx_psi_stats_batched %.1f us, '
          'qx_psi_adjoint %.1f us (%.0f%% of the iteration)' % (name, n, nt, d, m, q, b, step, st * 1e3, adj * 1e3,
                                                             100.0 * (st + adj) / step))
