"""Timings for DESIGN.md section 7.13 (training dp_gp_lvm on data with missing entries), HIP events on one GPU: medians with
min - max of 7 repeats, the forms of a comparison taking turns within every repeat in one process.

    python tools/time_train_masked_d.py [ops] [model] [slots] [parent=PATH]

ops:    ops.psi2 (fp64) and ops.elbo_grad_psi(prec='f64') at (B, N, M, Q) = (512, 2000, 128, 10) through the C entry points on
        preallocated buffers: unweighted, weighted with all ones, with 30 % zeros scattered, with 30 % zeros in blocks of 64 rows.
        parent=PATH (a libdpgp_hip.so built from the parent commit): the unweighted entry points of that library take turns with
        this build's.
model:  objective + gradients of the masked model at N=2000, D=512, M=128, Q=10, T=8 with 30 % missing, beside the unmasked
        precision='f64', backward_precision='f64' model, and the masked step's stages.
slots:  the same bound composed from the weighted qx_psi_* operators at B = D slots (one replicated Z per column), once, with
        torch.cuda.max_memory_allocated.
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dp_gp_lvm_amd import _lib, ops                                     # noqa: E402
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm                    # noqa: E402

dev = torch.device('cuda', 0)
f64 = dict(dtype=torch.float64, device=dev)
parent = [a.split('=', 1)[1] for a in sys.argv[1:] if a.startswith('parent=')]
what = {a for a in sys.argv[1:] if '=' not in a} or {'ops', 'model'}
B, N, M, Q, T = 512, 2000, 128, 10, 8


def timings_ms(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def alternate(forms, warmup=2, reps=5, repeats=7):
    """{name: (median of the repeats' medians, min, max)} in ms; the forms take turns within every repeat."""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    meds = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            meds[k].append(float(np.median(timings_ms(fn, reps))))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in meds.items()}


def show(tag, res):
    for k, r in res.items():
        print('%s | %s | %.3f ms [%.3f, %.3f]' % ((tag, k) + r), flush=True)
    if 'parent' in res and 'unweighted' in res:
        lo, hi = res['parent'][1], res['parent'][2]
        print('%s | unweighted median %s the parent\'s min - max' % (tag, 'within' if lo <= res['unweighted'][0] <= hi else 'OUTSIDE'), flush=True)


rng = np.random.default_rng(0)
weights = {'all ones': np.ones((B, N)), '30 % zeros scattered': (rng.random((B, N)) >= 0.3).astype(np.float64),
           '30 % zeros in blocks of 64 rows': np.repeat((rng.random((B, -(-N // 64))) >= 0.3).astype(np.float64), 64, axis=1)[:, :N]}

if 'ops' in what:
    l, stream, ptr = _lib.lib(), torch.cuda.current_stream().cuda_stream, (lambda t: t.data_ptr())
    z, mu, s = (torch.as_tensor(a, **f64) for a in (rng.standard_normal((M, Q)), rng.standard_normal((N, Q)), rng.uniform(0.3, 1.0, (N, Q))))
    gam, al = torch.as_tensor(rng.uniform(0.3, 1.0, (B, Q)), **f64), torch.as_tensor(rng.uniform(0.5, 2.0, B), **f64)
    sym = lambda a: a + a.transpose(0, 2, 1)
    g2, wk = (torch.as_tensor(sym(rng.standard_normal((B, M, M))), **f64) for _ in range(2))
    gv = torch.as_tensor(rng.standard_normal((B, M)), **f64)
    y_full = rng.standard_normal((N, B))
    out, dmu, ds, dz, dg = (torch.empty(sh, **f64) for sh in ((B, M, M), (N, Q), (N, Q), (M, Q), (B, Q)))
    wsb = max(l.dpgp_psi2_workspace_bytes(B, N, M, Q, 8), l.dpgp_elbo_grad_psi_workspace_bytes_ex(B, N, M, Q, _lib.PREC['f64']))
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device=dev)
    old = None
    if parent:
        old = ctypes.CDLL(os.path.abspath(parent[0]))
        assert not hasattr(old, 'dpgp_psi2_weighted_f64'), 'parent= must be a library of the parent commit'
        for name in ('dpgp_psi2_f64', 'dpgp_elbo_grad_psi'):
            getattr(old, name).restype, getattr(old, name).argtypes = _lib.SIGNATURES[name]
    kern = (B, N, M, Q, ptr(z), ptr(mu), ptr(s), ptr(gam), ptr(al))
    psi2_plain = lambda lib_: lib_.dpgp_psi2_f64(*kern, ptr(out), ptr(ws), ws.numel(), 0, stream)
    forms = dict(unweighted=lambda: psi2_plain(l))
    if old is not None:
        forms = dict(parent=lambda: psi2_plain(old), **forms)
    w_dev = {k: torch.as_tensor(w, **f64).contiguous() for k, w in weights.items()}
    for k, w in w_dev.items():
        forms[k] = (lambda w_: lambda: l.dpgp_psi2_weighted_f64(*kern, ptr(w_), ptr(out), ptr(ws), ws.numel(), 0, stream))(w)
    for fn in forms.values():
        assert fn() == 0
    show('psi2 fp64 B=%d N=%d M=%d Q=%d' % (B, N, M, Q), alternate(forms))
    ys = {k: torch.as_tensor(y_full * w.T, **f64).contiguous() for k, w in weights.items()}       # the caller zero-fills y
    y_dev = torch.as_tensor(y_full, **f64).contiguous()
    grad_plain = lambda lib_: lib_.dpgp_elbo_grad_psi(B, N, M, Q, ptr(y_dev), B, ptr(z), ptr(mu), ptr(s), ptr(gam), ptr(al), ptr(g2), ptr(wk),
                                                      ptr(gv), _lib.PREC['f64'], ptr(ws), ws.numel(), ptr(dmu), ptr(ds), ptr(dz), ptr(dg), stream)
    forms = dict(unweighted=lambda: grad_plain(l))
    if old is not None:
        forms = dict(parent=lambda: grad_plain(old), **forms)
    for k, w in w_dev.items():
        forms[k] = (lambda w_, y_: lambda: l.dpgp_elbo_grad_psi_weighted_f64(
            B, N, M, Q, ptr(y_), B, ptr(z), ptr(mu), ptr(s), ptr(gam), ptr(al), ptr(w_), ptr(g2), ptr(wk), ptr(gv), ptr(ws), ws.numel(),
            ptr(dmu), ptr(ds), ptr(dz), ptr(dg), stream))(w, ys[k])
    for fn in forms.values():
        assert fn() == 0
    show('elbo_grad_psi fp64 D=%d N=%d M=%d Q=%d' % (B, N, M, Q), alternate(forms, warmup=1, reps=3))

y = np.tanh(rng.standard_normal((N, 3))) @ rng.standard_normal((3, B)) + 0.3 * rng.standard_normal((N, B))
y = (y - y.mean(0)) / y.std(0)
obs = weights['30 % zeros scattered'].T.astype(bool)
kw = dict(num_latent_dims=Q, num_inducing_points=M, truncation_level=T, device=dev)

if 'model' in what:
    x0 = rng.standard_normal((N, Q))
    iv = dict(x_mean=x0, x_u=x0[:M] + 0.01 * rng.standard_normal((M, Q)))
    masked = dp_gp_lvm(np.where(obs, y, np.nan), observed=obs, initial_values=iv, **kw)
    plain = dp_gp_lvm(y, precision='f64', backward_precision='f64', initial_values=iv, **kw)
    show('objective + gradients N=%d D=%d M=%d Q=%d T=%d' % (N, B, M, Q, T),
         alternate({'unmasked f64 / f64': plain.gradients, 'masked, 30 % missing': masked.gradients}, warmup=1, reps=3))
    # where the masked step's time goes: its operators on the model's own mixed hyper-parameters
    masked.objective
    from dp_gp_lvm_amd.models.dp_gp_lvm import F
    z, mu, s = masked.inducing_input.detach(), masked.q_x[0].detach(), F.softplus(masked.raw['x_var']).detach()
    gam, al, be = (a.detach().contiguous() for a in (masked.ard_weights, masked.signal_variance[:, 0], masked.noise_precision[:, 0]))
    w_ = torch.as_tensor(obs.T, **f64).contiguous()
    y0 = torch.as_tensor(np.where(obs, y, 0.0), **f64).contiguous()
    mp = 16 * ((M + 15) // 16)
    g2p, wkp, gvp = torch.zeros(B, mp, mp, **f64), torch.zeros(B, mp, mp, **f64), torch.zeros(B, mp, **f64)
    k_uu = ops.ard_rbf_gram(z, None, gam, al, be, include_jitter=True)

    def dense():
        l_k, _ = ops.potrf_batched(k_uu)
        li = ops.tril_inverse_batched(l_k)
        tm = ops.matmul(ops.matmul(li, k_uu), li.transpose(1, 2))
        l_a, _ = ops.potrf_batched(tm)
        r0 = ops.matmul(ops.tril_inverse_batched(l_a), li)
        p = ops.matmul(r0.transpose(1, 2), r0)
        kp = ops.matmul(ops.matmul(li.transpose(1, 2), li), k_uu)
        return ops.matmul(ops.matmul(kp, p), kp.transpose(1, 2))
    show('masked step, by stage', alternate({
        'K_uu (gram)': lambda: ops.ard_rbf_gram(z, None, gam, al, be, include_jitter=True),
        'weighted Psi2': lambda: ops.psi2(z, mu, s, gam, al, weights=w_),
        'Psi1^T y': lambda: ops.psi1T_y(z, mu, s, gam, al, y0),
        'dense chain (2 potrf, 2 inverses, 9 products)': dense,
        'weighted stage B': lambda: ops.elbo_grad_psi(y0, z, mu, s, gam, al, g2p, wkp, gvp, prec='f64', weights=w_)}, warmup=1, reps=3))

if 'slots' in what:
    # the alternative the feature avoids: one slot per column on the weighted test-point operators (replicated Z, Psi1 and its
    # adjoint [D, N, M] in memory); forward statistics + both adjoints, once
    torch.cuda.reset_peak_memory_stats()
    z = torch.as_tensor(rng.standard_normal((M, Q)), **f64)
    mu, s = torch.as_tensor(rng.standard_normal((N, Q)), **f64), torch.full((N, Q), 0.5, **f64)
    gam, al = torch.full((B, Q), 0.5, **f64), torch.ones(B, **f64)
    zr = z[None].expand(B, -1, -1).contiguous()
    zf = ops.qx_pair_factor(zr, gam, al)
    w_ = torch.as_tensor(obs.T, **f64).contiguous()

    def slots():
        psi1, psi2 = ops.qx_psi_stats_batched(zr, mu, s, gam, al, zf, weights=w_)
        g1, g2 = torch.ones_like(psi1), torch.ones_like(psi2)
        ops.qx_psi_adjoint(zr, mu, s, gam, al, g1, g2, zf, weights=w_)
        ops.qx_psi_param_adjoint(zr, mu, s, gam, al, g1, g2, zf, weights=w_)
    slots()
    t = timings_ms(slots, 1)[0]
    print('slot form at B = D = %d slots (statistics + (mu, S) adjoint + parameter adjoint, dense chain not included): %.1f ms, '
          'max_memory_allocated %.2f GB' % (B, t, torch.cuda.max_memory_allocated() / 2 ** 30), flush=True)
