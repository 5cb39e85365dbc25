# scratch: gp_lvm (N=2000, D=512, Q=10) and gp_regression (N=4096, D=1, Q=8): ms per objective + gradients (model.gradients(),
# the whole chain) and the gram-gradient kernel alone (dpgp_ard_rbf_gram_grad_f64), HIP events, warm-up, median of repeats.
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models.gaussian_process import gp_lvm, gp_regression
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
for name, n, d, q in (('gp_lvm', 2000, 512, 10), ('gp_regression', 4096, 1, 8)):
    if name == 'gp_lvm':
        y = np.tanh(rng.standard_normal((n, 3))) @ rng.standard_normal((3, d)) + 0.3 * rng.standard_normal((n, d))
        model = gp_lvm(y, num_latent_dims=q, device=dev)
        x = model.latent_input.detach()
    else:
        xh = rng.uniform(-2, 2, (n, q))
        model = gp_regression(xh, np.sin(xh.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((n, 1)), device=dev)
        x = torch.as_tensor(xh, device=dev)
    step = median_ms(lambda: model.gradients())
    fwd = median_ms(lambda: model.objective.detach())
    w = torch.as_tensor(rng.standard_normal((n, n)), device=dev)
    gamma = torch.full((1, q), 0.5, dtype=torch.float64, device=dev)
    alpha = torch.ones(1, 1, dtype=torch.float64, device=dev)
    kern = median_ms(lambda: ops.ard_rbf_gram_grad(x, gamma, alpha, w), warmup=5, reps=50)
    flops = 2.0 * n ** 3 + 4.0 * n * n * d
    print('%s N=%d D=%d Q=%d: objective + gradients %.3f ms (%.1f TFLOP/s on 2N^3 + 4N^2 D), objective %.3f ms, '
          'gram_grad %.1f us (W read %.2f TB/s; %d x %d x 3Q fp64 ops)'
          % (name, n, d, q, step, flops / step / 1e9, fwd, kern * 1e3, 8.0 * n * n / kern / 1e9, n, n))
