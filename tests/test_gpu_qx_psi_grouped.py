"""GPU tests of the pattern-grouped Psi operators (dpgp_qx_psi_{stats,adjoint,param_adjoint}_grouped_f64, csrc/qx_psi.hip): K
kernels x P weight rows shared by the kernels.  Each operator against fp64 torch autograd (CPU) of the plain restatement of
rbf_kernel.py:135-199, with psi2_kn formed once per kernel and contracted with the weights, and against the existing weighted
operators called in the K P slot form.  Tolerance: 1e-12, the project's operator tolerance.  The shapes cover M and N that are
no multiples of 32 / 64, M over 128, the LDS bound at Q = 64, chunk boundaries in P (P = PC and PC + 1 for the widths the
host picks: 8 at Q = 10, 2 for the (mu, S) adjoint at Q = 64) and a chunk made only of zero weights."""
import numpy as np
import pytest
import torch

from test_gpu_predict_b1 import close

pytestmark = pytest.mark.gpu

#          K, P,  M,   Q,  N
SHAPES = [(1, 1, 1, 1, 1), (1, 3, 17, 10, 300), (3, 8, 64, 10, 300), (2, 9, 65, 23, 130), (1, 17, 128, 10, 300), (3, 5, 200, 3, 70),
          (2, 4, 40, 64, 70), (1, 9, 40, 10, 70), (1, 2, 40, 64, 70), (1, 3, 40, 64, 70)]
KINDS = ['binary', 'pattern_off', 'normal']


def case_of(k, p, m, q, n, kind, seed):
    rs = np.random.default_rng(seed)
    c = dict(z=rs.standard_normal((k, m, q)), mu=rs.standard_normal((n, q)), s=rs.uniform(0.1, 1.5, (n, q)),
             gamma=rs.uniform(0.2, 2.0, (k, q)), alpha=rs.uniform(0.5, 2.0, k), g1=rs.standard_normal((k, n, m)),
             g2=rs.standard_normal((k, p, m, m)))
    if kind == 'normal':
        w = rs.standard_normal((p, n))
    else:
        w = (rs.random((p, n)) >= 0.4).astype(np.float64)
        if kind == 'pattern_off':
            w[p - 1] = 0.0                  # (the last pattern: with P = 9 or 17 a whole chunk of the kernels is zero weights)
    c['w'] = w
    return {name: torch.as_tensor(a, dtype=torch.float64) for name, a in c.items()}


def restated(c):
    """psi1 [K,N,M], psi2 [K,P,M,M] and the gradients of L = sum_k <g1_k, Psi1_k> + sum_kp <g2_kp, Psi2_kp> with respect to
    (mu, s, z, gamma, alpha), torch fp64 on the CPU; psi2_kn is formed once per kernel, in chunks of points."""
    z, mu, s, gamma, alpha = (c[k].clone().requires_grad_() for k in ('z', 'mu', 's', 'gamma', 'alpha'))
    w, g1, g2 = c['w'], c['g1'], c['g2']
    leaves = [mu, s, z, gamma, alpha]
    kk, m, q = z.shape
    n = mu.shape[0]
    grads = [torch.zeros_like(a) for a in leaves]
    psi1s, psi2s = [], []
    step = max(1, int(1.5e7 // (m * m * q)))
    for k in range(kk):
        den1 = gamma[k] * s[:, None, :] + 1.0                                             # [N,1,Q]
        num1 = gamma[k] * (mu[:, None, :] - z[k][None, :, :]) ** 2                       # [N,M,Q]
        psi1 = torch.exp(torch.log(alpha[k]) - 0.5 * torch.sum(num1 / den1 + torch.log(den1), dim=-1))
        psi1s.append(psi1.detach())
        for a, g in zip(grads, torch.autograd.grad(torch.sum(g1[k] * psi1), leaves, allow_unused=True)):
            if g is not None:
                a += g
        psi2 = torch.zeros_like(g2[k])
        for n0 in range(0, n, step):
            mc, sc = mu[n0:n0 + step], s[n0:n0 + step]
            zbar = 0.5 * (z[k][:, None, :] + z[k][None, :, :])                            # [M,M,Q]
            t1 = 0.25 * gamma[k] * (z[k][:, None, :] - z[k][None, :, :]) ** 2
            den2 = 2.0 * gamma[k] * sc[:, None, None, :] + 1.0                            # [n,1,1,Q]
            num2 = gamma[k] * (mc[:, None, None, :] - zbar[None]) ** 2                    # [n,M,M,Q]
            psi2n = torch.exp(2.0 * torch.log(alpha[k]) - torch.sum(0.5 * torch.log(den2) + t1[None] + num2 / den2, dim=-1))
            part = torch.einsum('pn,nab->pab', w[:, n0:n0 + step], psi2n)
            psi2 = psi2 + part.detach()
            for a, g in zip(grads, torch.autograd.grad(torch.sum(g2[k] * part), leaves, allow_unused=True)):
                if g is not None:
                    a += g
        psi2s.append(psi2)
    return dict(psi1=torch.stack(psi1s), psi2=torch.stack(psi2s), d_mu=grads[0], d_s=grads[1], d_z=grads[2], d_gamma=grads[3],
                d_alpha=grads[4])


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('k,p,m,q,n', SHAPES)
def test_grouped_operators(dev, k, p, m, q, n, kind):
    from dp_gp_lvm_amd import ops
    c = case_of(k, p, m, q, n, kind, 10000 * k + 1000 * p + 10 * m + q + n)
    want = restated(c)
    z, mu, s, gamma, alpha, g1, g2, w = (c[name].to(dev).contiguous() for name in ('z', 'mu', 's', 'gamma', 'alpha', 'g1', 'g2', 'w'))
    dz = z[:, :, None, :] - z[:, None, :, :]
    zfac = ((alpha * alpha)[:, None, None] * torch.exp(-0.25 * torch.sum(gamma[:, None, None, :] * dz * dz, dim=-1))).contiguous()
    # the slot form: slot (k, p) carries kernel k's inputs and weight row p; g1 of a kernel rides in its first slot
    rep = lambda t: t.repeat_interleave(p, dim=0).contiguous()
    w_slot = w.repeat(k, 1).contiguous()
    g1_slot = torch.zeros((k, p) + tuple(g1.shape[1:]), dtype=torch.float64, device=dev)
    g1_slot[:, 0] = g1
    g1_slot, g2_slot = g1_slot.reshape(k * p, n, m), g2.reshape(k * p, m, m)
    for zf in (None, zfac):
        tag = '%s zfac=%s ' % (kind, zf is not None)
        zf_slot = None if zf is None else rep(zf)
        # ---- statistics
        psi1, psi2 = ops.qx_psi_stats_grouped(z, mu, s, gamma, alpha, w, zfac=zf)
        psi1_b, psi2_b = ops.qx_psi_stats_grouped(z, mu, s, gamma, alpha, w, zfac=zf)
        assert tuple(psi1.shape) == (k, n, m) and tuple(psi2.shape) == (k, p, m, m)
        for name, h in (('psi1', psi1), ('psi2', psi2)):
            print(tag + '%s: max |err| %.3e of %.3e' % (name, float((h.cpu() - want[name]).abs().max()), float(want[name].abs().max())))
        close(psi1, want['psi1'].numpy(), 1e-12, tag + 'psi1')
        close(psi2, want['psi2'].numpy(), 1e-12, tag + 'psi2')
        assert torch.equal(psi1, psi1_b) and torch.equal(psi2, psi2_b), tag + 'stats: two calls differ'
        assert torch.equal(psi2, psi2.transpose(2, 3)), tag + 'psi2 is not exactly symmetric'
        if kind == 'pattern_off':
            assert bool((psi2[:, p - 1] == 0.0).all()), tag + 'the all-zero pattern has a non-zero psi2'
        psi1_s, psi2_s = ops.qx_psi_stats_batched(rep(z), mu, s, rep(gamma), rep(alpha), zfac=zf_slot, weights=w_slot)
        close(psi1, psi1_s.reshape(k, p, n, m)[:, 0].cpu().numpy(), 1e-12, tag + 'psi1 against the slot form')
        close(psi2, psi2_s.reshape(k, p, m, m).cpu().numpy(), 1e-12, tag + 'psi2 against the slot form')
        # ---- (mu, S) adjoint
        have = ops.qx_psi_adjoint_grouped(z, mu, s, gamma, alpha, g1, g2, w, zfac=zf)
        again = ops.qx_psi_adjoint_grouped(z, mu, s, gamma, alpha, g1, g2, w, zfac=zf)
        slot = ops.qx_psi_adjoint(rep(z), mu, s, rep(gamma), rep(alpha), g1_slot, g2_slot, zfac=zf_slot, weights=w_slot)
        for name, h, a, sl in zip(('d_mu', 'd_s'), have, again, slot):
            print(tag + '%s: max |err| %.3e of %.3e' % (name, float((h.cpu() - want[name]).abs().max()), float(want[name].abs().max())))
            close(h, want[name].numpy(), 1e-12, tag + name)
            assert torch.equal(h, a), tag + name + ': two calls differ'
            close(h, sl.cpu().numpy(), 1e-12, tag + name + ' against the slot form')
        # ---- parameter adjoint
        have = ops.qx_psi_param_adjoint_grouped(z, mu, s, gamma, alpha, g1, g2, w, zfac=zf)
        again = ops.qx_psi_param_adjoint_grouped(z, mu, s, gamma, alpha, g1, g2, w, zfac=zf)
        slot = ops.qx_psi_param_adjoint(rep(z), mu, s, rep(gamma), rep(alpha), g1_slot, g2_slot, zfac=zf_slot, weights=w_slot)
        for name, h, a, sl in zip(('d_z', 'd_gamma', 'd_alpha'), have, again, slot):
            print(tag + '%s: max |err| %.3e of %.3e' % (name, float((h.cpu() - want[name]).abs().max()), float(want[name].abs().max())))
            close(h, want[name].numpy(), 1e-12, tag + name)
            assert torch.equal(h, a), tag + name + ': two calls differ'
            close(h, sl.reshape((k, p) + tuple(h.shape[1:])).sum(dim=1).cpu().numpy(), 1e-12, tag + name + ' against the slot form')


def test_argument_checks(dev):
    from dp_gp_lvm_amd import ops
    c = case_of(2, 3, 5, 2, 7, 'binary', 1)
    z, mu, s, gamma, alpha, g1, g2, w = (c[name].to(dev).contiguous() for name in ('z', 'mu', 's', 'gamma', 'alpha', 'g1', 'g2', 'w'))
    with pytest.raises(TypeError):
        ops.qx_psi_stats_grouped(z, mu, s, gamma, alpha, None)                  # the weights are required
    with pytest.raises(AssertionError):
        ops.qx_psi_stats_grouped(z, mu, s, gamma, alpha, w[:, :-1].contiguous())
    with pytest.raises(AssertionError):
        ops.qx_psi_adjoint_grouped(z, mu, s, gamma, alpha, g1, g2[:, :2].contiguous(), w)
    with pytest.raises(AssertionError):
        ops.qx_psi_param_adjoint_grouped(z, mu, s, gamma, alpha, g1[:1].contiguous(), g2, w)
