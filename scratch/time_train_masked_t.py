# scratch: training dp_gp_lvm_t on data with missing entries (observed=...): each pattern-grouped Psi operator
# (ops.qx_psi_*_grouped, K kernels x P weight rows) beside the existing weighted operator in the K P slot form, alternating in one
# process; the zero-weight skip; one optimise() iteration of the masked over-T model with 1 / 16 row patterns, grouped and slot
# form (DPGP_GROUPED_PSI), beside the unmasked precision='f64' model.  HIP events, warm-up, medians of >= 15 timings; the spread
# of a form is min to max of 7 repeats of that median.  A per-iteration figure is (T(12 iterations) - T(4 iterations)) / 8.
#   python scratch/time_train_masked_t.py [ops] [skip] [model] [parent=PATH]
# parent=PATH (a libdpgp_hip.so of the parent commit, e.g. scratch/libdpgp_hip_parent.so): the existing weighted entry points of
# this build against the parent's at the three shapes of DESIGN 7.7, both loaded in one process, alternating.
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm_t
dev = torch.device('cuda', 0)
f64 = dict(dtype=torch.float64, device=dev)
parent = [a.split('=', 1)[1] for a in sys.argv[1:] if a.startswith('parent=')]
what = {a for a in sys.argv[1:] if '=' not in a} or ({'ops', 'skip', 'model'} if not parent else set())


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


def case(k, p, n, m, q, rng, w=None):
    z = torch.as_tensor(rng.standard_normal((k, m, q)), **f64)
    gam, al = torch.full((k, q), 0.5, **f64), torch.ones(k, **f64)
    mu, s = torch.as_tensor(rng.standard_normal((n, q)), **f64), torch.ones(n, q, **f64)
    g1 = torch.as_tensor(rng.standard_normal((k, n, m)), **f64)
    g2 = torch.as_tensor(rng.standard_normal((k, p, m, m)), **f64)
    if w is None:
        w = np.ones((p, n)) if p == 1 else (rng.random((p, n)) >= 0.3).astype(np.float64)
    w = torch.as_tensor(w, **f64).contiguous()
    zf = ops.qx_pair_factor(z, gam, al)
    rep = lambda t: t.repeat_interleave(p, dim=0).contiguous()
    g1s = torch.zeros((k, p, n, m), **f64)
    g1s[:, 0] = g1
    slot = (rep(z), mu, s, rep(gam), rep(al), g1s.reshape(k * p, n, m), g2.reshape(k * p, m, m), rep(zf), w.repeat(k, 1).contiguous())
    return (z, mu, s, gam, al, g1, g2, w, zf), slot


def three_ops(k, p, n, m, q, rng, w=None):
    """The C entry points themselves, on preallocated outputs and workspaces (no wrapper or allocator time between the events)."""
    from dp_gp_lvm_amd import _lib
    l, stream, ptr = _lib.lib(), torch.cuda.current_stream().cuda_stream, (lambda t: t.data_ptr())
    (z, mu, s, gam, al, g1, g2, w, zf), (zs, _, _, gs, als, g1s, g2s, zfs, ws_) = case(k, p, n, m, q, rng, w)
    b = k * p
    out = dict(psi1=torch.empty(k, n, m, **f64), psi2=torch.empty(k, p, m, m, **f64), psi1s=torch.empty(b, n, m, **f64),
               dmu=torch.empty(n, q, **f64), ds=torch.empty(n, q, **f64), dz=torch.empty(b, m, q, **f64), dg=torch.empty(b, q, **f64),
               da=torch.empty(b, **f64))
    need = [getattr(l, 'dpgp_qx_psi_%s_grouped_workspace_bytes' % o)(k, p, n, m, q) for o in ('stats', 'adjoint', 'param_adjoint')] + \
           [getattr(l, 'dpgp_qx_psi_%s_workspace_bytes' % o)(b, n, m, q) for o in ('stats', 'adjoint', 'param_adjoint')]
    ws = torch.empty(max(need) + 256, dtype=torch.uint8, device=dev)
    grp = (k, p, n, m, q, ptr(z), ptr(mu), ptr(s), ptr(gam), ptr(al), ptr(zf), ptr(w))
    slt = (b, n, m, q, ptr(zs), ptr(mu), ptr(s), ptr(gs), ptr(als), ptr(zfs), ptr(ws_))
    tail = (ptr(ws), ws.numel(), stream)
    o = {name: ptr(t) for name, t in out.items()}
    forms = dict(
        stats=dict(grouped=lambda: l.dpgp_qx_psi_stats_grouped_f64(*grp, o['psi1'], o['psi2'], *tail),
                   slot=lambda: l.dpgp_qx_psi_stats_weighted_f64(*slt, o['psi1s'], o['psi2'], *tail)),
        adjoint=dict(grouped=lambda: l.dpgp_qx_psi_adjoint_grouped_f64(*grp, ptr(g1), ptr(g2), o['dmu'], o['ds'], *tail),
                     slot=lambda: l.dpgp_qx_psi_adjoint_weighted_f64(*slt, ptr(g1s), ptr(g2s), o['dmu'], o['ds'], *tail)),
        param=dict(grouped=lambda: l.dpgp_qx_psi_param_adjoint_grouped_f64(*grp, ptr(g1), ptr(g2), o['dz'], o['dg'], o['da'], *tail),
                   slot=lambda: l.dpgp_qx_psi_param_adjoint_weighted_f64(*slt, ptr(g1s), ptr(g2s), o['dz'], o['dg'], o['da'], *tail)))
    for f in forms.values():
        assert f['grouped']() == 0 and f['slot']() == 0
    return {name: alternate(f) for name, f in forms.items()}


def show(tag, res):
    for op, r in res.items():
        print('%s %s: grouped %.1f us [%.1f, %.1f], slot form %.1f us [%.1f, %.1f]' % ((tag, op) + r['grouped'] + r['slot']), flush=True)


rng = np.random.default_rng(0)
if 'ops' in what:
    for k, p, n, m, q in ((1, 1, 2000, 128, 10), (1, 16, 2000, 128, 10), (8, 16, 2000, 128, 10), (4, 60, 200, 50, 10)):
        show('K=%d P=%d N=%d M=%d Q=%d' % (k, p, n, m, q), three_ops(k, p, n, m, q, rng))
if 'skip' in what:
    k, p, n, m, q = 1, 8, 500, 128, 10
    blocks = np.tile(((np.arange(n) // 64) % 2 == 0).astype(np.float64), (p, 1))
    for name, w in (('all ones', np.ones((p, n))), ('50 % zeros in alternating blocks of 64 rows', blocks)):
        show('zero-weight skip K=%d P=%d N=%d M=%d Q=%d, %s' % (k, p, n, m, q, name), three_ops(k, p, n, m, q, rng, w))


def pattern_mask(n, d, p, rng):
    pats = [np.ones(n, dtype=bool)]
    while len(pats) < p:
        cand = rng.random(n) >= 0.3
        if not any(np.array_equal(cand, o) for o in pats):
            pats.append(cand)
    return np.stack([pats[c % p] for c in range(d)], axis=1)


def per_iteration(make):
    t = {}
    for it in (4, 12):
        def run():
            make().optimise(it, learning_rate=1e-3)
        run(); run()
        t[it] = float(np.median(timings_ms(run, 15)))
    return (t[12] - t[4]) / 8.0


if 'model' in what:
    n, d, m, q, t_ = 2000, 512, 128, 10, 8
    y = np.tanh(rng.standard_normal((n, 3))) @ rng.standard_normal((3, d)) + 0.3 * rng.standard_normal((n, d))
    kw = dict(num_latent_dims=q, num_inducing_points=m, truncation_level=t_, device=dev)
    print('unmasked precision=f64 N=%d D=%d M=%d Q=%d T=%d: %.3f ms per optimise() iteration'
          % (n, d, m, q, t_, per_iteration(lambda: dp_gp_lvm_t(y, precision='f64', **kw))), flush=True)
    for p in (1, 16):
        obs = pattern_mask(n, d, p, rng)
        y_nan = np.where(obs, y, np.nan)
        for grouped in ('1', '0'):
            os.environ['DPGP_GROUPED_PSI'] = grouped
            print('masked P=%d patterns, DPGP_GROUPED_PSI=%s: %.3f ms per optimise() iteration'
                  % (p, grouped, per_iteration(lambda: dp_gp_lvm_t(y_nan, observed=obs, **kw))), flush=True)

if parent:
    import ctypes
    from dp_gp_lvm_amd import _lib
    new, old = _lib.lib(), ctypes.CDLL(os.path.abspath(parent[0]))
    names = ('dpgp_qx_psi_stats_weighted_f64', 'dpgp_qx_psi_adjoint_weighted_f64', 'dpgp_qx_psi_param_adjoint_weighted_f64',
             'dpgp_qx_psi_stats_workspace_bytes', 'dpgp_qx_psi_adjoint_workspace_bytes', 'dpgp_qx_psi_param_adjoint_workspace_bytes')
    for name in names:
        getattr(old, name).restype, getattr(old, name).argtypes = _lib.SIGNATURES[name]
    assert not hasattr(old, 'dpgp_qx_psi_stats_grouped_f64'), 'parent= must be a library of the parent commit'
    stream = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr()
    for b, n, m, q in ((1, 100, 50, 10), (20, 100, 50, 10), (1, 500, 128, 10)):
        (z, mu, s, gam, al, g1, g2, _, zf), _ = case(b, 1, n, m, q, rng)
        g2 = g2.reshape(b, m, m)
        w = torch.as_tensor((rng.random((b, n)) >= 0.3).astype(np.float64), **f64).contiguous()
        psi1, psi2 = torch.empty(b, n, m, **f64), torch.empty(b, m, m, **f64)
        dmu, ds = torch.empty(n, q, **f64), torch.empty(n, q, **f64)
        dz, dg, da = torch.empty(b, m, q, **f64), torch.empty(b, q, **f64), torch.empty(b, **f64)
        ws = torch.empty(max(getattr(new, k)(b, n, m, q) for k in names[3:]) + 256, dtype=torch.uint8, device=dev)
        common = lambda: (b, n, m, q, ptr(z), ptr(mu), ptr(s), ptr(gam), ptr(al), ptr(zf), ptr(w))
        calls = dict(
            stats=lambda l: l.dpgp_qx_psi_stats_weighted_f64(*common(), ptr(psi1), ptr(psi2), ptr(ws), ws.numel(), stream),
            adjoint=lambda l: l.dpgp_qx_psi_adjoint_weighted_f64(*common(), ptr(g1), ptr(g2), ptr(dmu), ptr(ds), ptr(ws), ws.numel(), stream),
            param=lambda l: l.dpgp_qx_psi_param_adjoint_weighted_f64(*common(), ptr(g1), ptr(g2), ptr(dz), ptr(dg), ptr(da), ptr(ws),
                                                                     ws.numel(), stream))
        for op, fn in calls.items():
            assert fn(new) == 0 and fn(old) == 0
            r = alternate(dict(parent=lambda: fn(old), new=lambda: fn(new)), warmup=5, reps=50)
            print('weighted %s B=%d N=%d M=%d Q=%d: parent %.1f us [%.1f, %.1f], new %.1f us [%.1f, %.1f]: %s the parent\'s min - max'
                  % ((op, b, n, m, q) + r['parent'] + r['new'] + ('within' if r['parent'][1] <= r['new'][0] <= r['parent'][2] else 'OUTSIDE',)),
                  flush=True)
