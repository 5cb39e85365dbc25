"""Timings for DESIGN.md section 7.14 (the shared-inducing test bound of dp_gp_lvm), HIP events on one GPU: medians with min - max of
7 repeats, the forms of a comparison taking turns within every repeat in one process.

    python tools/time_test_bound_d.py [ops] [model]

ops:    ops.psi_latent_adjoint against ops.elbo_grad_psi(prec='f64', weights=) (which also forms d_z and d_gamma) and against
        ops.qx_psi_adjoint(weights=) on B slots (replicated z, g1 = y (x) g_v [B,N,M]) through the C entry points on preallocated
        buffers, at (B, N, M, Q) = (512, 500, 128, 10) and (60, 100, 50, 10); weights all ones, 30 % zeros scattered, 30 % zeros in
        blocks of 64 points.
model:  one q(X*) iteration (bound + gradient, as optimise_test_latents runs it) at D = 512, N* = 500, M = 128, Q = 10 with 30 % of the
        test entries missing, form='slots' against 'shared', and torch.cuda.max_memory_allocated of each (bound object included).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dp_gp_lvm_amd import _lib, ops                                     # noqa: E402
from dp_gp_lvm_amd.models.frozen_bound import _TestBound                # noqa: E402
from dp_gp_lvm_amd.models.frozen_bound_d import _TestBoundD           # noqa: E402

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


def show(tag, res):
    for k, r in res.items():
        print('%s | %s | %.3f ms [%.3f, %.3f]' % ((tag, k) + r), flush=True)


def weights_of(rng, b, n):
    return {'all ones': np.ones((b, n)), '30 % zeros scattered': (rng.random((b, n)) >= 0.3).astype(np.float64),
            '30 % zeros in blocks of 64': np.repeat((rng.random((b, -(-n // 64))) >= 0.3).astype(np.float64), 64, axis=1)[:, :n]}


if 'ops' in what:
    l, stream, ptr = _lib.lib(), torch.cuda.current_stream().cuda_stream, (lambda t: t.data_ptr())
    for B, N, M, Q in ((512, 500, 128, 10), (60, 100, 50, 10)):
        rng = np.random.default_rng(0)
        mp = 16 * ((M + 15) // 16)
        z, mu, s = (torch.as_tensor(a, **f64) for a in (rng.standard_normal((M, Q)), rng.standard_normal((N, Q)), rng.uniform(0.3, 1.0, (N, Q))))
        gam, al = torch.as_tensor(rng.uniform(0.3, 1.0, (B, Q)), **f64), torch.as_tensor(rng.uniform(0.5, 2.0, B), **f64)
        g2_np = rng.standard_normal((B, M, M))
        g2 = torch.as_tensor(g2_np + g2_np.transpose(0, 2, 1), **f64).contiguous()
        gv = torch.as_tensor(rng.standard_normal((B, M)), **f64)
        pad = torch.nn.functional.pad
        g2p, gvp = pad(g2, (0, mp - M, 0, mp - M)).contiguous(), pad(gv, (0, mp - M)).contiguous()
        wkp = torch.zeros_like(g2p)
        zr = z[None].expand(B, -1, -1).contiguous()
        y_full = rng.standard_normal((N, B))
        dmu, ds, dz, dg = (torch.empty(sh, **f64) for sh in ((N, Q), (N, Q), (M, Q), (B, Q)))
        wsb = max(l.dpgp_psi_latent_adjoint_workspace_bytes(B, N, M, Q), l.dpgp_elbo_grad_psi_workspace_bytes_ex(B, N, M, Q, _lib.PREC['f64']),
                  l.dpgp_qx_psi_adjoint_workspace_bytes(B, N, M, Q))
        ws = torch.empty(wsb + 256, dtype=torch.uint8, device=dev)
        for kind, w_np in weights_of(rng, B, N).items():
            w = torch.as_tensor(w_np, **f64).contiguous()
            y = torch.as_tensor(y_full * w_np.T, **f64).contiguous()                          # the caller zero-fills y
            g1 = (y.T[:, :, None] * gv[:, None, :]).contiguous()
            forms = {
                'psi_latent_adjoint': lambda: l.dpgp_psi_latent_adjoint_f64(
                    B, N, M, Q, ptr(z), ptr(mu), ptr(s), ptr(gam), ptr(al), ptr(y), B, ptr(w), ptr(gv), ptr(g2), ptr(dmu), ptr(ds), ptr(ws),
                    ws.numel(), stream),
                'elbo_grad_psi f64, weighted': lambda: l.dpgp_elbo_grad_psi_weighted_f64(
                    B, N, M, Q, ptr(y), B, ptr(z), ptr(mu), ptr(s), ptr(gam), ptr(al), ptr(w), ptr(g2p), ptr(wkp), ptr(gvp), ptr(ws), ws.numel(),
                    ptr(dmu), ptr(ds), ptr(dz), ptr(dg), stream),
                'qx_psi_adjoint on B slots': lambda: l.dpgp_qx_psi_adjoint_weighted_f64(
                    B, N, M, Q, ptr(zr), ptr(mu), ptr(s), ptr(gam), ptr(al), None, ptr(w), ptr(g1), ptr(g2), ptr(dmu), ptr(ds), ptr(ws),
                    ws.numel(), stream)}
            for k, fn in forms.items():
                assert fn() == 0, k
            show('(B, N, M, Q) = (%d, %d, %d, %d), weights %s' % (B, N, M, Q, kind), alternate(forms))

if 'model' in what:
    D, N, M, Q = 512, 500, 128, 10
    rng = np.random.default_rng(1)
    z = torch.as_tensor(rng.standard_normal((M, Q)), **f64)
    mu, s = torch.as_tensor(rng.standard_normal((N, Q)), **f64), torch.as_tensor(rng.uniform(0.3, 1.0, (N, Q)), **f64)
    gam, al, be = (torch.as_tensor(a, **f64) for a in (rng.uniform(0.3, 1.0, (D, Q)), rng.uniform(0.5, 2.0, D), rng.uniform(2.0, 20.0, D)))
    obs = rng.random((N, D)) >= 0.3
    y0 = torch.as_tensor(np.where(obs, rng.standard_normal((N, D)), 0.0), **f64).contiguous()
    w = torch.as_tensor(obs.T, **f64).contiguous()
    bounds, peak = {}, {}
    for form in ('slots', 'shared'):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        if form == 'slots':
            bounds[form] = _TestBound.slots(z, gam, al, be, y0.T[:, :, None].contiguous(), np.ones(D), w, dev)
        else:
            bounds[form] = _TestBoundD(z, gam, al, be, y0, w, dev)
        bounds[form].evaluate(mu, s, grad=True)
        torch.cuda.synchronize()
        peak[form] = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
    f = {k: float(b.evaluate(mu, s, grad=True)[0]) for k, b in bounds.items()}
    print('bound: slots %.12g, shared %.12g' % (f['slots'], f['shared']), flush=True)
    show('one q(X*) iteration, D = %d, N* = %d, M = %d, Q = %d, 30 %% missing' % (D, N, M, Q),
         alternate({k: (lambda b_: lambda: b_.evaluate(mu, s, grad=True))(b) for k, b in bounds.items()}))
    for k in bounds:
        print('max_memory_allocated above the inputs, form %s: %.3f GB' % (k, peak[k]), flush=True)
    sh = bounds['shared']
    g2 = torch.as_tensor(rng.standard_normal((D, M, M)), **f64)
    gv = torch.as_tensor(rng.standard_normal((D, M)), **f64)
    li = sh.li

    def dense():
        tm = ops.matmul(ops.matmul(li, g2), li.transpose(1, 2))
        l_a, _ = ops.potrf_batched(0.0 * tm + sh.eye)
        r0 = ops.matmul(ops.tril_inverse_batched(l_a), li)
        u = ops.matmul(r0, gv[:, :, None])
        r = ops.matmul(r0.transpose(1, 2), u)
        return ops.matmul(r0.transpose(1, 2), r0) - ops.matmul(r, r.transpose(1, 2))
    show("form 'shared', by stage", alternate({
        'weighted Psi2': lambda: ops.psi2(sh.z, mu, s, sh.gamma, sh.alpha, weights=sh.weights),
        'Psi1^T y': lambda: ops.psi1T_y(sh.z, mu, s, sh.gamma, sh.alpha, sh.y),
        'dense chain (potrf, inverse, 7 products)': dense,
        'psi_latent_adjoint': lambda: ops.psi_latent_adjoint(sh.z, mu, s, sh.gamma, sh.alpha, sh.y, gv, g2, weights=sh.weights)}))
