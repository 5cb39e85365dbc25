# Time of one optimise_test_latents iteration of the four latent-variable models on one GPU: the fit of q(X*)
# from a supplied start, (T(12 iterations) - T(4 iterations)) / 8, which leaves out the start and the construction of the bound.
# HIP events, warm-up; each figure is the median of 7 such differences with [min, max].  N = 400, N* = 100, D = 60, M = 50, Q = 10,
# T = 5 (the small shape of tools/time_predict_t.py); untrained fp64 models; `observed=` with 30 % of the test entries missing.
#   python tools/time_test_latents.py            -> one line per row and one JSON line {row: [median, min, max]} in microseconds
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm, dp_gp_lvm_t
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm, manifold_relevance_determination
dev = torch.device('cuda', 0)
N, N_T, D, M, Q, T = 400, 100, 60, 50, 10, 5
REPEATS, WARMUP = 7, 2


def timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def per_iteration_us(fit):
    """fit(iterations) runs optimise_test_latents; (median, min, max) over REPEATS of (T(12) - T(4)) / 8 in microseconds."""
    for _ in range(WARMUP):
        fit(4); fit(12)
    vals = [(timed_ms(lambda: fit(12)) - timed_ms(lambda: fit(4))) / 8.0 * 1e3 for _ in range(REPEATS)]
    return [float(np.median(vals)), min(vals), max(vals)]


rng = np.random.default_rng(0)
y = np.tanh(rng.standard_normal((N + N_T, 3))) @ rng.standard_normal((3, D)) + 0.3 * rng.standard_normal((N + N_T, D))
y_train, y_test = y[:N], y[N:]
obs = rng.random((N_T, D)) >= 0.3
obs[:, 0] = obs[:, D // 2] = True                                    # (every row, and every view of MRD, keeps an observed entry)
y_nan = np.where(obs, y_test, np.nan)
kw = dict(num_latent_dims=Q, num_inducing_points=M, device=dev, precision='f64')
half = D // 2
models = dict(
    bayesian_gp_lvm=lambda: bayesian_gp_lvm(y_train, **kw),
    manifold_relevance_determination=lambda: manifold_relevance_determination([y_train[:, :half], y_train[:, half:]], **kw),
    dp_gp_lvm=lambda: dp_gp_lvm(y_train, truncation_level=T, **kw),
    dp_gp_lvm_t=lambda: dp_gp_lvm_t(y_train, truncation_level=T, **kw))
result = {}
for name, make in models.items():
    torch.manual_seed(0)
    np.random.seed(0)
    model = make()
    mrd = name == 'manifold_relevance_determination'
    rows = {'first': ([y_test[:, :half]] if mrd else y_test[:, :half], {}),
            'observed': ([y_nan[:, :half], y_nan[:, half:]] if mrd else y_nan,
                         dict(observed=[obs[:, :half], obs[:, half:]] if mrd else obs))}
    if name == 'dp_gp_lvm':
        rows['observed shared'] = (y_nan, dict(observed=obs, form='shared'))
    for row, (y_arg, kwargs) in rows.items():
        xm, xv = model.optimise_test_latents(y_arg, 2, **kwargs)
        xm, xv = xm.clone(), xv.clone()
        fit = lambda it: model.optimise_test_latents(y_arg, it, x_test_mean=xm, x_test_var=xv, **kwargs)
        result['%s %s' % (name, row)] = per_iteration_us(fit)
        print('%-50s %9.1f us per iteration [%.1f, %.1f]' % (('%s %s' % (name, row),) + tuple(result['%s %s' % (name, row)])),
              flush=True)
print(json.dumps(result))
