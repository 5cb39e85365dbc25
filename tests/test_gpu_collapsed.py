"""
models/collapsed.py on its own: the forward pass, both forms of G2, G_v, GK and the beta summand of B = 3 slots against a dense
torch.linalg evaluation in fp64 on the host, differentiated by torch.autograd.  M = 5 is no multiple of any tile, J = 2 columns
per slot; beta spans 0.5 ... 30, the multiplier D takes an integer, 1 and a real value, phi is positive and random.

The inputs are well conditioned (cond K_uu and cond A below 1e4 for the committed seed: test_inputs_are_well_conditioned, host
only), so the operators' fp64 tolerance holds: rtol 1e-10, atol 1e-10 max(1, |want|_max).
"""
import math

import numpy as np
import pytest
import torch

from dp_gp_lvm_amd.utils.constants import GP_DEFAULT_JITTER

B, M, J, Q, N = 3, 5, 2, 2, 9
SEED = 5
F64 = torch.float64


def inputs():
    rng = np.random.default_rng(SEED)
    w = rng.standard_normal((B, M, N))
    return dict(z=rng.standard_normal((B, M, Q)), psi_2=w @ w.transpose(0, 2, 1) / N, v=rng.standard_normal((B, M, J)),
                phi=0.2 + rng.random((B, J)), beta=np.array([0.5, 2.0, 30.0]), dd=np.array([1.0, 3.0, 2.5]),
                n_w=np.array([9.0, 4.0, 7.0]), alpha=np.ones(B), yy=1.0 + rng.random(B))


def host_gram(z):
    """K_uu [B,M,M] of gamma = 1, alpha = 1 with the project's jitter (torch, host)."""
    sq = ((z[:, :, None, :] - z[:, None, :, :]) ** 2).sum(-1)
    return torch.exp(-0.5 * sq) + GP_DEFAULT_JITTER * torch.eye(M, dtype=F64)


def dense(k, psi_2, v, beta, p):
    """(f, f + the terms without factorisations) of the module's docstring, with torch.linalg on the host."""
    t = lambda a: torch.as_tensor(a, dtype=F64)
    dd, phi, n_w, al, yy = t(p['dd']), t(p['phi']), t(p['n_w']), t(p['alpha']), t(p['yy'])
    kb = k + beta[:, None, None] * psi_2
    logdet_la = 0.5 * (torch.linalg.slogdet(kb)[1] - torch.linalg.slogdet(k)[1])
    tr = torch.diagonal(torch.linalg.solve(k, psi_2), dim1=-2, dim2=-1).sum(-1)
    uu = torch.sum(phi * torch.sum(v * torch.linalg.solve(kb, v), dim=1), dim=1)
    f = torch.sum(-dd * logdet_la + 0.5 * dd * beta * tr + 0.5 * beta * beta * uu)
    rest = torch.sum(0.5 * n_w * dd * (torch.log(beta) - math.log(2.0 * math.pi)) - 0.5 * dd * beta * al * n_w - 0.5 * beta * yy)
    return f, f + rest, logdet_la, tr


def test_inputs_are_well_conditioned():
    p = inputs()
    k = host_gram(torch.as_tensor(p['z'], dtype=F64))
    li = torch.linalg.inv(torch.linalg.cholesky(k))
    a = torch.as_tensor(p['beta'], dtype=F64)[:, None, None] * (li @ torch.as_tensor(p['psi_2'], dtype=F64) @ li.transpose(1, 2)) \
        + torch.eye(M, dtype=F64)
    cond_k, cond_a = float(torch.linalg.cond(k).max()), float(torch.linalg.cond(a).max())
    print('cond K_uu %.3g, cond A %.3g' % (cond_k, cond_a))
    assert cond_k < 1e4 and cond_a < 1e4


def close(got, want, what):
    want = want.detach().numpy()
    got = got.cpu().numpy()
    print('%s: max |err| %.3e of %.3e' % (what, np.abs(got - want).max(), np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-10 * max(1.0, np.abs(want).max()), err_msg=what)


@pytest.mark.gpu
def test_core_against_dense_autograd(dev):
    from dp_gp_lvm_amd import ops
    from dp_gp_lvm_amd.models import collapsed
    p = inputs()
    h = lambda a: torch.as_tensor(a, dtype=F64)
    d = lambda a: torch.as_tensor(a, dtype=F64, device=dev).contiguous()

    # the reference: dense, on the host
    k_h = host_gram(h(p['z'])).requires_grad_()
    psi_h, v_h, be_h = h(p['psi_2']).requires_grad_(), h(p['v']).requires_grad_(), h(p['beta']).requires_grad_()
    f_h, full_h, logdet_h, tr_h = dense(k_h, psi_h, v_h, be_h, p)
    g2_h, gv_h, gk_h = torch.autograd.grad(f_h, (psi_h, v_h, k_h), retain_graph=True)
    db_h, = torch.autograd.grad(full_h, be_h)

    # the core: K_uu from the gram operator, one kernel per slot
    one, gamma = torch.ones(1, dtype=F64, device=dev), torch.ones((1, Q), dtype=F64, device=dev)
    k = torch.cat([ops.ard_rbf_gram(d(p['z'][b]), None, gamma, one, one, include_noise=False, include_jitter=True,
                                    jitter=GP_DEFAULT_JITTER) for b in range(B)])
    close(k, k_h, 'K_uu')
    li, info = collapsed.factors(k)
    kinv = collapsed.k_inverse(li)
    beta, dd, phi = d(p['beta']), d(p['dd']), d(p['phi'])
    ch = collapsed.Chain(li, d(p['psi_2']), beta).project(d(p['v']))
    assert not info.any() and not ch.info.any()
    uu = torch.sum(phi * torch.sum(ch.u * ch.u, dim=1), dim=1)
    f = torch.sum(-dd * ch.logdet + 0.5 * dd * beta * ch.tr + 0.5 * beta * beta * uu)
    close(ch.logdet, logdet_h, 'log|L_A|')
    close(ch.tr, tr_h, 'tr T')
    close(f, f_h, 'f')

    adj = collapsed.Adjoint(ch, dd, phi)
    g2_product, g2_difference = adj.g2_product(kinv), adj.g2_difference(kinv)
    close(g2_product, g2_h, 'G2, product form')
    close(g2_difference, g2_h, 'G2, difference form')
    close(g2_product, g2_difference.cpu(), 'G2, the two forms')
    close(adj.b3 * adj.b3 * adj.rphi, gv_h, 'G_v')
    close(adj.gk(), gk_h, 'GK')
    close(adj.d_beta(d(p['n_w']), d(p['alpha']), uu, d(p['yy'])), db_h, 'the beta summand')

    # the posterior pieces: rhs = beta P v, C = K_uu^-1 - P
    rhs, c = collapsed.posterior(ch.r0, kinv, beta, d(p['v']))
    kb = (k_h + be_h[:, None, None] * psi_h).detach()
    close(rhs, be_h.detach()[:, None, None] * torch.linalg.solve(kb, v_h.detach()), 'rhs')
    close(c, torch.linalg.inv(k_h.detach()) - torch.linalg.inv(kb), 'C')
