# Timings of the predictive moments' latent adjoint and of the frozen predictors on it, on one GPU.  HIP events,
# 2 warm-ups, the median and min - max of 7 repeats; the forms of (a) take turns within every repeat.
#   python tools/time_predictor_vjp.py [ops] [model]
# (a) ops:   ops.qx_psi_pointwise (the forward operator), ops.qx_psi_pointwise_adjoint (its latent adjoint) and the same adjoint
#            composed of ops.psi_latent_adjoint calls with J + G replicated slots per kernel (every exponential and every moment
#            product J + G times).  At K = 512, G = J = 1 the kernels share Z: the composition is ONE ops.psi_latent_adjoint call
#            with the over-D substitution of models/predictor.py, the route dp_gp_lvm's predictor takes.
# (b) model: one Adam iteration of the loop of examples/latent_targets.py (p(x, s), the held-out negative log density of 3 given
#            columns, backward, step) per model kind, N = 400, N* = 100, D = 60, M = 50, Q = 10.
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import torch.nn.functional as F
from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm, dp_gp_lvm_t
from dp_gp_lvm_amd.models.gaussian_process import bayesian_gp_lvm, manifold_relevance_determination
from dp_gp_lvm_amd.models.predictor import negative_log_density
dev = torch.device('cuda', 0)
f64 = dict(dtype=torch.float64, device=dev)
what = set(sys.argv[1:]) or {'ops', 'model'}


def time_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(forms, warmup=2, repeats=7):
    """{name: (median, min, max)} of the repeats in milliseconds; the forms take turns within every repeat."""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    ts = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            ts[k].append(time_ms(fn))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in ts.items()}


def slot_inputs(zk, gam, al, c, r, h, gq, gt, k):
    j, g, m, n = r.shape[2], c.shape[1], r.shape[1], h.shape[1]
    rt = r[k].transpose(0, 1).contiguous()
    return dict(z=zk[k], gamma=gam[k][None].expand(j + g, -1).contiguous(), alpha=al[k].expand(j + g).contiguous(),
                y=torch.cat([h[k], torch.zeros((n, g), **f64)], dim=1).contiguous(), g_v=torch.cat([rt, torch.zeros((g, m), **f64)]).contiguous(),
                g_psi2=torch.cat([rt[:, :, None] * rt[:, None, :], c[k]]).contiguous(),
                w=torch.cat([gq[k], gt[k]], dim=1).transpose(0, 1).contiguous())


rng = np.random.default_rng(0)
if 'ops' in what:
    for k, g, j, m, q, n in ((4, 4, 60, 50, 10, 100), (8, 16, 512, 128, 10, 500), (512, 1, 1, 128, 10, 500)):
        z0 = torch.as_tensor(rng.standard_normal((m, q)), **f64)                               # (shared by the kernels, as in the models)
        zk = z0[None].expand(k, -1, -1).contiguous()
        gam, al = torch.full((k, q), 0.5, **f64), torch.ones(k, **f64)
        mu, s = torch.as_tensor(rng.standard_normal((n, q)), **f64), torch.ones(n, q, **f64)
        c, r = torch.as_tensor(rng.standard_normal((k, g, m, m)), **f64), torch.as_tensor(rng.standard_normal((k, m, j)), **f64)
        h, gq, gt = (torch.as_tensor(rng.standard_normal(sh), **f64) for sh in ((k, n, j), (k, n, j), (k, n, g)))
        zf = ops.qx_pair_factor(zk, gam, al)
        forward = lambda: ops.qx_psi_pointwise(zk, mu, s, gam, al, c, r, zfac=zf)
        adjoint = lambda: ops.qx_psi_pointwise_adjoint(zk, mu, s, gam, al, c, r, h, gq, gt, zfac=zf)
        if g == 1 and j == 1:
            gt = -gq                                                                           # (var = .. - tr + quad: what the predictor passes)
            r1, zero = r[:, :, 0].contiguous(), torch.zeros((k, m), **f64)
            rr = (r1[:, :, None] * r1[:, None, :]).contiguous()
            y1 = h[:, :, 0].transpose(0, 1).contiguous()                                       # [N, K]
            both = dict(gamma=torch.cat([gam, gam]).contiguous(), alpha=torch.cat([al, al]).contiguous(),
                        y=torch.cat([y1, torch.zeros_like(y1)], dim=1).contiguous(), g_v=torch.cat([r1, zero]).contiguous(),
                        g_psi2=torch.cat([rr, c[:, 0]]).contiguous(), w=torch.cat([gq[:, :, 0], gt[:, :, 0]]).contiguous())
            g2, w1 = (rr - c[:, 0]).contiguous(), gq[:, :, 0].contiguous()
            slots = lambda: ops.psi_latent_adjoint(z0, mu, s, both['gamma'], both['alpha'], both['y'], both['g_v'], both['g_psi2'],
                                                   weights=both['w'])
            one = lambda: ops.psi_latent_adjoint(z0, mu, s, gam, al, y1, r1, g2, weights=w1)
        else:
            per = [slot_inputs(zk, gam, al, c, r, h, gq, gt, kk) for kk in range(k)]

            def slots():
                outs = [ops.psi_latent_adjoint(p['z'], mu, s, p['gamma'], p['alpha'], p['y'], p['g_v'], p['g_psi2'], weights=p['w']) for p in per]
                return sum(o[0] for o in outs), sum(o[1] for o in outs)
            one = None
        err = max(float((x - y_).abs().max() / y_.abs().max()) for x, y_ in zip(adjoint(), slots()))
        forms = dict(forward=forward, adjoint=adjoint, slots=slots)
        if one is not None:
            forms['over_d'] = one
        res = alternate(forms)
        line = 'K=%d G=%d J=%d M=%d Q=%d N=%d: ' % (k, g, j, m, q, n)
        line += '; '.join('%s %.3f ms [%.3f, %.3f]' % ((name,) + res[name]) for name in forms)
        print(line + '; slots / adjoint %.2f (largest relative difference %.1e)' % (res['slots'][0] / res['adjoint'][0], err), flush=True)


def adam_iteration(preds, ys, givens, n_t, q):
    xt = torch.zeros((n_t, q), **f64).requires_grad_(True)
    raw = torch.zeros((n_t, q), **f64).requires_grad_(True)
    opt = torch.optim.Adam([xt, raw], lr=0.05)

    def step():
        opt.zero_grad()
        sv = F.softplus(raw)
        loss = sum(negative_log_density(*p(xt, sv), y, gv) for p, y, gv in zip(preds, ys, givens))
        loss.backward()
        opt.step()
    return step


if 'model' in what:
    n, n_t, d, m, q, t = 400, 100, 60, 50, 10, 4
    y = np.tanh(rng.standard_normal((n + n_t, 3))) @ rng.standard_normal((3, d)) + 0.3 * rng.standard_normal((n + n_t, d))
    y = (y - y[:n].mean(axis=0)) / y[:n].std(axis=0)
    kinds = dict(bayesian_gp_lvm=lambda: bayesian_gp_lvm(y[:n], num_latent_dims=q, num_inducing_points=m, device=dev, precision='f64'),
                 mrd=lambda: manifold_relevance_determination([y[:n, :d // 2], y[:n, d // 2:]], num_latent_dims=q, num_inducing_points=m,
                                                              device=dev, precision='f64'),
                 dp_gp_lvm=lambda: dp_gp_lvm(y[:n], num_latent_dims=q, num_inducing_points=m, truncation_level=t, device=dev, precision='f64'),
                 dp_gp_lvm_t=lambda: dp_gp_lvm_t(y[:n], num_latent_dims=q, num_inducing_points=m, truncation_level=t, device=dev,
                                                 precision='f64'))
    for name, make in kinds.items():
        model = make()
        e0 = time_ms(lambda: model.frozen_predictor())
        preds = model.frozen_predictor()
        preds = preds if isinstance(preds, list) else [preds]
        widths = [p.num_columns for p in preds]
        offs = np.concatenate([[0], np.cumsum(widths)])
        ys = [torch.as_tensor(y[n:, offs[i]:offs[i + 1]], **f64) for i in range(len(preds))]
        givens = []
        for yy in ys:
            gv = torch.zeros(yy.shape, dtype=torch.bool, device=dev)
            gv[:, [0, 3, 6]] = True
            givens.append(gv)
        res = alternate(dict(step=adam_iteration(preds, ys, givens, n_t, q), forward=lambda: [p(ys[0].new_zeros((n_t, q)), ys[0].new_ones((n_t, q))) for p in preds]))
        print('%s (N=%d N*=%d D=%d M=%d Q=%d): frozen_predictor() %.2f ms (first call); one Adam iteration %.3f ms [%.3f, %.3f]; '
              'p(x, s) alone %.3f ms [%.3f, %.3f]' % ((name, n, n_t, d, m, q, e0) + res['step'] + res['forward']), flush=True)
