# scratch: prediction with per-entry observation masks (observed=...): one optimise_test_latents iteration of bayesian_gp_lvm and
# dp_gp_lvm and the two weighted operators under it, the effect of the zero-weight skip of the stats kernel, and (with
# --parent PATH: a libdpgp_hip.so of the parent commit, e.g. scratch/libdpgp_hip_parent.so) the unweighted entry points of this
# build against the parent's, alternating in one process.  HIP events, warm-up, medians of >= 15 repeats.
# A per-iteration figure is (T(30 iterations) - T(10 iterations)) / 20: what a call sets up once (K_uu, its factor, the slots'
# outputs and weights, for dp_gp_lvm one model evaluation) is not in it.
import argparse, ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dp_gp_lvm_amd import _lib, ops
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm
ap = argparse.ArgumentParser()
ap.add_argument('--parent', default=None)
args = ap.parse_args()
dev = torch.device('cuda', 0)
f64 = dict(dtype=torch.float64, device=dev)


def times_ms(fn, warmup=3, reps=15):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return np.asarray(ts)


def median_ms(fn, warmup=3, reps=15):
    return float(np.median(times_ms(fn, warmup, reps)))


def per_iteration(model, y, xm, xv, **kw):
    t = {k: median_ms(lambda: model.optimise_test_latents(y, k, x_test_mean=xm, x_test_var=xv, **kw)) for k in (10, 30)}
    return (t[30] - t[10]) / 20.0


def pattern_mask(nt, d, p, rng):
    """p distinct row patterns over the d columns (column c has pattern c % p); pattern 0 observes every row, the others miss
    about 30 % of the rows."""
    pats = [np.ones(nt, dtype=bool)]
    while len(pats) < p:
        cand = rng.random(nt) >= 0.3
        if not any(np.array_equal(cand, o) for o in pats):
            pats.append(cand)
    return np.stack([pats[c % p] for c in range(d)], axis=1)


def op_case(b, nt, m, q, rng):
    z = torch.as_tensor(rng.standard_normal((b, m, q)), **f64)
    gam, al = torch.full((b, q), 0.5, **f64), torch.ones(b, **f64)
    xm, xv = torch.as_tensor(rng.standard_normal((nt, q)), **f64), torch.ones(nt, q, **f64)
    g1, g2 = torch.as_tensor(rng.standard_normal((b, nt, m)), **f64), torch.as_tensor(rng.standard_normal((b, m, m)), **f64)
    return z, xm, xv, gam, al, g1, g2, ops.qx_pair_factor(z, gam, al)


def weighted_ops_us(w, nt, m, q, rng):
    z, xm, xv, gam, al, g1, g2, zf = op_case(w.shape[0], nt, m, q, rng)
    st = median_ms(lambda: ops.qx_psi_stats_batched(z, xm, xv, gam, al, zf, weights=w), warmup=5, reps=30)
    adj = median_ms(lambda: ops.qx_psi_adjoint(z, xm, xv, gam, al, g1, g2, zf, weights=w), warmup=5, reps=30)
    return st * 1e3, adj * 1e3


rng = np.random.default_rng(0)
for n, nt, d, m, q, ps in ((200, 100, 60, 50, 10, (1, 4, 60)), (2000, 500, 512, 128, 10, (1, 16))):
    y = np.tanh(rng.standard_normal((n + nt, 3))) @ rng.standard_normal((3, d)) + 0.3 * rng.standard_normal((n + nt, d))
    model = bayesian_gp_lvm(y[:n], num_latent_dims=q, num_inducing_points=m, device=dev, precision='f64')
    xm, xv = torch.as_tensor(rng.standard_normal((nt, q)), **f64), torch.ones(nt, q, **f64)
    base = per_iteration(model, y[n:], xm, xv)
    print('bgplvm N=%d N*=%d D=%d M=%d Q=%d unmasked (observed=None, all D columns): %.3f ms per iteration' % (n, nt, d, m, q, base))
    for p in ps:
        obs = pattern_mask(nt, d, p, rng)
        it = per_iteration(model, np.where(obs, y[n:], np.nan), xm, xv, observed=obs)
        w = torch.as_tensor(np.unique(obs, axis=1).T.astype(np.float64), **f64).contiguous()
        st, adj = weighted_ops_us(w, nt, m, q, rng)
        print('bgplvm N=%d N*=%d D=%d M=%d Q=%d P=%d patterns (%d slots): %.3f ms per iteration; weighted stats %.1f us, '
              'weighted adjoint %.1f us' % (n, nt, d, m, q, p, w.shape[0], it, st, adj))
n, nt, d, m, q = 2000, 500, 512, 128, 10
y = np.tanh(rng.standard_normal((n + nt, 3))) @ rng.standard_normal((3, d)) + 0.3 * rng.standard_normal((n + nt, d))
model = dp_gp_lvm(y[:n], num_latent_dims=q, num_inducing_points=m, device=dev, precision='mixed')
xm, xv = torch.as_tensor(rng.standard_normal((nt, q)), **f64), torch.ones(nt, q, **f64)
masks = {'30 % of the entries missing at random': rng.random((nt, d)) >= 0.3,
         'column-only mask, 128 missing columns (the last 128)': np.repeat(np.arange(d)[None, :] < d - 128, nt, axis=0)}
for name, obs in masks.items():
    it = per_iteration(model, np.where(obs, y[n:], np.nan), xm.cpu().numpy(), xv.cpu().numpy(), observed=obs)
    cols = np.flatnonzero(obs.any(axis=0))
    w = torch.as_tensor(obs[:, cols].T.astype(np.float64), **f64).contiguous()
    st, adj = weighted_ops_us(w, nt, m, q, rng)
    print('dp_gp_lvm N=%d N*=%d D=%d M=%d Q=%d, %s (%d slots): %.3f ms per iteration (fp64 slots); weighted stats %.1f us, '
          'weighted adjoint %.1f us' % (n, nt, d, m, q, name, w.shape[0], it, st, adj))
it = per_iteration(model, y[n:, :d - 128], xm.cpu().numpy(), xv.cpu().numpy())
print('dp_gp_lvm same shape, the existing fused-ELBO path on y_test[:, :384] (observed=None; a different arithmetic: the '
      "model's mixed precision, one model evaluation per iteration): %.3f ms per iteration" % it)

# ---- the zero-weight skip of the stats kernel: 50 % zero weights in contiguous row blocks against all ones
b, nt, m, q = 64, 500, 128, 10
z, xm, xv, gam, al, g1, g2, zf = op_case(b, nt, m, q, rng)
ones = torch.ones(b, nt, **f64)
half = ones.clone()
half[:, (torch.arange(nt, device=dev) // 32) % 2 == 1] = 0.0                     # every other block of 32 rows
scattered = torch.as_tensor((rng.random((b, nt)) >= 0.5).astype(np.float64), **f64)
for name, w in (('all ones', ones), ('50 %% zeros in blocks of 32 rows (%.0f %% zero)' % (100 * float((half == 0).double().mean())), half),
                ('50 % zeros scattered', scattered), ('weights=None (unweighted kernels)', None)):
    st = median_ms(lambda: ops.qx_psi_stats_batched(z, xm, xv, gam, al, zf, weights=w), warmup=5, reps=30)
    adj = median_ms(lambda: ops.qx_psi_adjoint(z, xm, xv, gam, al, g1, g2, zf, weights=w), warmup=5, reps=30)
    print('B=%d N*=%d M=%d Q=%d, %s: stats %.1f us, adjoint %.1f us' % (b, nt, m, q, name, st * 1e3, adj * 1e3))

# ---- the unweighted entry points: this build against the parent's library, alternating, the three shapes of DESIGN 7.6
if args.parent:
    new, old = _lib.lib(), ctypes.CDLL(os.path.abspath(args.parent))
    for name in ('dpgp_qx_psi_stats_batched_f64', 'dpgp_qx_psi_adjoint_f64', 'dpgp_qx_psi_stats_workspace_bytes',
                 'dpgp_qx_psi_adjoint_workspace_bytes'):
        getattr(old, name).restype, getattr(old, name).argtypes = _lib.SIGNATURES[name]
    assert not hasattr(old, 'dpgp_qx_psi_stats_weighted_f64'), '--parent must be a library of the parent commit'
    stream = torch.cuda.current_stream().cuda_stream
    for b, nt, m, q in ((1, 100, 50, 10), (20, 100, 50, 10), (1, 500, 128, 10)):
        z, xm, xv, gam, al, g1, g2, zf = op_case(b, nt, m, q, rng)
        psi1, psi2 = torch.empty(b, nt, m, **f64), torch.empty(b, m, m, **f64)
        dmu, ds = torch.empty(nt, q, **f64), torch.empty(nt, q, **f64)
        ws = torch.empty(max(new.dpgp_qx_psi_stats_workspace_bytes(b, nt, m, q), new.dpgp_qx_psi_adjoint_workspace_bytes(b, nt, m, q),
                             256), dtype=torch.uint8, device=dev)
        p = lambda t: t.data_ptr()

        def stats(l):
            assert l.dpgp_qx_psi_stats_batched_f64(b, nt, m, q, p(z), p(xm), p(xv), p(gam), p(al), p(zf), p(psi1), p(psi2), p(ws),
                                                   ws.numel(), stream) == 0

        def adjoint(l):
            assert l.dpgp_qx_psi_adjoint_f64(b, nt, m, q, p(z), p(xm), p(xv), p(gam), p(al), p(zf), p(g1), p(g2), p(dmu), p(ds),
                                             p(ws), ws.numel(), stream) == 0
        for opname, fn in (('stats', stats), ('adjoint', adjoint)):
            meds = {'parent': [], 'new': []}
            for _ in range(7):                                                      # alternating: parent, new, parent, new, ...
                for tag, l in (('parent', old), ('new', new)):
                    meds[tag].append(1e3 * float(np.median(times_ms(lambda: fn(l), warmup=5, reps=50))))
            po, pn = np.asarray(meds['parent']), np.asarray(meds['new'])
            print('unweighted %s B=%d N*=%d M=%d Q=%d: parent median %.1f us (min %.1f, max %.1f, spread %.1f), new median %.1f us '
                  '(min %.1f, max %.1f); new - parent %+.1f us: %s the parent\'s spread'
                  % (opname, b, nt, m, q, np.median(po), po.min(), po.max(), po.max() - po.min(), np.median(pn), pn.min(), pn.max(),
                     np.median(pn) - np.median(po), 'within' if po.min() <= np.median(pn) <= po.max() else 'OUTSIDE'))
