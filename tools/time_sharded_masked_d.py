"""Timings for DESIGN.md section 7.15 (dp_gp_lvm trained with observed=, D-sharded), HIP events on ONE GPU in one process: the
8 shares of a world of 8 are built one after another with _shard_of=(r, 8) — each is what one rank would run between its
collectives — and objective + gradients of each share is timed, median [min, max] of 7 repeats (each repeat the median of 3
calls), the shares taking turns within every repeat.  No communicator and no second GPU: the all-reduces (2 fp64 scalars, then
the packed gradients) and their latency are NOT in these numbers.

    python tools/time_sharded_masked_d.py [random] [block]

N=2000, D=512, M=128, Q=10, T=8, two masks:
random: 30 % missing at random.
block:  the same, then columns 0-127 observed in the first quarter of the rows only.
For each mask: the unsharded step, then the 8 shares for shard_by='count' and for shard_by='observed', with the maximum and the
mean over the shares and each share's bounds and number of observed entries.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm                    # noqa: E402

dev = torch.device('cuda', 0)
what = set(sys.argv[1:]) or {'random', 'block'}
N, D, M, Q, T, WORLD = 2000, 512, 128, 10, 8, 8


def timings_ms(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def alternate(forms, warmup=1, reps=3, repeats=7):
    """{name: (median of the repeats' medians, min, max)} in ms; the forms take turns within every repeat."""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    meds = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            meds[k].append(float(np.median(timings_ms(fn, reps))))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in meds.items()}


rng = np.random.default_rng(0)
y = np.tanh(rng.standard_normal((N, 3))) @ rng.standard_normal((3, D)) + 0.3 * rng.standard_normal((N, D))
y = (y - y.mean(0)) / y.std(0)
random30 = rng.random((N, D)) >= 0.3
block = random30.copy()
block[N // 4:, :128] = False
x0 = rng.standard_normal((N, Q))
iv = dict(x_mean=x0, x_u=x0[:M] + 0.01 * rng.standard_normal((M, Q)))
kw = dict(num_latent_dims=Q, num_inducing_points=M, truncation_level=T, device=dev, initial_values=iv)

for name, obs in (('random', random30), ('block', block)):
    if name not in what:
        continue
    y_nan = np.where(obs, y, np.nan)
    tag = '%s mask, N=%d D=%d M=%d Q=%d T=%d, %.1f %% observed' % (name, N, D, M, Q, T, 100.0 * obs.mean())
    whole = dp_gp_lvm(y_nan, observed=obs, **kw)
    r = alternate({'unsharded': whole.gradients})['unsharded']
    print('%s | unsharded objective + gradients | %.3f ms [%.3f, %.3f]' % ((tag,) + r), flush=True)
    del whole
    for shard_by in ('count', 'observed'):
        shares = [dp_gp_lvm(y_nan, observed=obs, shard_by=shard_by, _shard_of=(rank, WORLD), **kw) for rank in range(WORLD)]
        res = alternate({rank: m.gradients for rank, m in enumerate(shares)})
        for rank, m in enumerate(shares):
            lo, hi = m.shard
            print('%s | shard_by=%s | share %d: columns [%d, %d), %d observed entries | %.3f ms [%.3f, %.3f]'
                  % ((tag, shard_by, rank, lo, hi, int(obs[:, lo:hi].sum())) + res[rank]), flush=True)
        med = [res[rank][0] for rank in range(WORLD)]
        print('%s | shard_by=%s | over the %d shares: maximum %.3f ms, mean %.3f ms' % (tag, shard_by, WORLD, max(med), float(np.mean(med))),
              flush=True)
        del shares
