"""CPU tests (no GPU) of the references that pin the latent adjoint of the per-point contractions (dpgp_qx_psi_pointwise_adjoint_f64,
csrc/qx_psi_point_adjoint.hip) and of the host algebra around it.  The reference of the GPU tests is torch autograd through
`restated` of test_gpu_qx_psi_pointwise.py, contracted with the adjoints (h, gq, gt):
    L = sum h (psi1 r) + sum gq quad + sum gt tr,      (d_mu, d_s) = autograd of L.
Here it is checked against the closed form that the kernel implements (a pair m <= m' visited once, c symmetrised, moments
S0, S1, S2; 1e-12, a row with s = 0 included) and against central differences (h = 1e-5, bound 1e-5 max(1, |.|), the precedent of
test_gpu_predict.py) at one small shape; the VJPs of the moments' combination step (ops.point_moments_adjoints) and of
frozen_bound_t.mixture_moments (predictor.mixture_moments_vjp) are checked against autograd.  CASES is the table the GPU file runs;
the references are computed once per case, shared, and never modified."""
import numpy as np
import torch

from test_gpu_predict_b1 import close
from test_gpu_qx_psi_point_moments import gidx_of
from test_gpu_qx_psi_pointwise import inputs_of, restated

#         K, G,   J,   M,  Q,   N         what the shape covers
CASES = [(1, 1, 1, 1, 1, 1),            # smallest problem
         (2, 3, 17, 33, 10, 65),        # M, N, J off the 32 / 64 / 16 tile edges
         (1, 2, 130, 40, 10, 70),       # more than one column chunk
         (3, 2, 40, 65, 17, 130),       # Q just past the register path
         (1, 2, 15, 40, 64, 70),        # the Q bound
         (1, 1, 5, 200, 10, 33),        # pair-tile slabs at small N K
         (5, 1, 1, 50, 10, 100)]        # over-D layout
_REFS = {}


def adjoint_case(shape, variant=''):
    """(inputs, (h, gq, gt)): inputs_of plus random normal adjoints.  variant 's0': the variances of one row are 0;
    'block': N is taken as given and the adjoints of the points 64..127 and 130..193 are 0."""
    k, g, j, m, q, n = shape
    c = inputs_of(*shape)
    rs = np.random.default_rng(17 + sum(shape))
    h, gq, gt = (torch.as_tensor(rs.standard_normal(sh)) for sh in ((k, n, j), (k, n, j), (k, n, g)))
    if variant == 's0':
        c['s'] = c['s'].clone()
        c['s'][min(1, n - 1)] = 0.0
    if variant == 'block':
        for a in (h, gq, gt):
            a[:, 64:128] = 0.0
            a[:, 130:194] = 0.0
    return c, (h, gq, gt)


def autograd_of(c, adj):
    h, gq, gt = adj
    mu, s = c['mu'].clone().requires_grad_(True), c['s'].clone().requires_grad_(True)
    w = restated(dict(c, mu=mu, s=s))
    loss = torch.sum(h * torch.matmul(w['psi1'], c['r'])) + torch.sum(gq * w['quad']) + torch.sum(gt * w['tr'])
    d_mu, d_s = torch.autograd.grad(loss, (mu, s))
    return d_mu.detach(), d_s.detach()


def reference(shape, variant=''):
    """(inputs, adjoints, (d_mu, d_s) by autograd) of a case: computed once, shared by the tests, never modified."""
    key = (shape, variant)
    if key not in _REFS:
        c, adj = adjoint_case(shape, variant)
        _REFS[key] = (c, adj, autograd_of(c, adj))
    return _REFS[key]


def closed_form(c, adj):
    """The algebra of csrc/qx_psi_point_adjoint.hip in torch fp64, per kernel, every pair m <= m' once."""
    h, gq, gt = adj
    z, mu, s, gamma, alpha = (c[k] for k in ('z', 'mu', 's', 'gamma', 'alpha'))
    kk, m, q = z.shape
    d_mu, d_s = torch.zeros_like(mu), torch.zeros_like(s)
    a, b = torch.triu_indices(m, m)
    for k in range(kk):
        zk, g, al, r, cs = z[k], gamma[k], alpha[k], c['r'][k], c['c'][k]
        off = (a != b).to(torch.float64)
        zbar = 0.5 * (zk[a] + zk[b])                                                   # [P,Q]
        f = al * al * torch.exp(-0.25 * torch.sum(g * (zk[a] - zk[b]) ** 2, dim=-1))  # [P]
        rr = r[a] * r[b] * (1.0 + off)[:, None]                                        # [P,J]
        ct = torch.where(off > 0, cs[:, a, b] + cs[:, b, a], cs[:, a, a])              # [G,P]
        t = gq[k] @ rr.T + gt[k] @ ct                                                  # [N,P]
        gr = g / (2.0 * g * s + 1.0)
        c2 = torch.prod((2.0 * g * s + 1.0) ** -0.5, dim=-1)
        e = c2[:, None] * torch.exp(-torch.sum(gr[:, None, :] * (mu[:, None, :] - zbar[None]) ** 2, dim=-1))
        d = t * e * f
        s0, s1, s2 = d.sum(dim=1, keepdim=True), d @ zbar, d @ (zbar * zbar)
        d_mu += -2.0 * gr * (mu * s0 - s1)
        d_s += -gr * s0 + 2.0 * gr * gr * (mu * mu * s0 - 2.0 * mu * s1 + s2)
        a1 = h[k] @ r.T                                                                # [N,M]
        gr1 = g / (g * s + 1.0)
        e1 = al * torch.prod((g * s + 1.0) ** -0.5, dim=-1)[:, None] * \
            torch.exp(-0.5 * torch.sum(gr1[:, None, :] * (mu[:, None, :] - zk[None]) ** 2, dim=-1))
        d1 = a1 * e1
        t0, t1, t2 = d1.sum(dim=1, keepdim=True), d1 @ zk, d1 @ (zk * zk)
        d_mu += -gr1 * (mu * t0 - t1)
        d_s += 0.5 * (-gr1 * t0 + gr1 * gr1 * (mu * mu * t0 - 2.0 * mu * t1 + t2))
    return d_mu, d_s


def test_closed_form_against_autograd():
    for shape, variant in [(CASES[0], ''), (CASES[1], ''), (CASES[1], 's0'), (CASES[3], ''), (CASES[6], 's0'), ((2, 2, 3, 5, 2, 7), 's0')]:
        c, adj, want = reference(shape, variant)
        have = closed_form(c, adj)
        for name, hv, wv in zip(('d_mu', 'd_s'), have, want):
            print('%s %s %s: max |err| %.3e of %.3e' % (shape, variant, name, float((hv - wv).abs().max()), float(wv.abs().max())))
            assert bool(torch.isfinite(hv).all())
            close(hv, wv.numpy(), 1e-12, '%s %s %s' % (shape, variant, name))


def test_autograd_against_central_differences():
    shape = (2, 2, 3, 5, 2, 7)
    c, adj, (d_mu, d_s) = reference(shape)
    h, gq, gt = adj

    def loss(mu, s):
        w = restated(dict(c, mu=mu, s=s))
        return float(torch.sum(h * torch.matmul(w['psi1'], c['r'])) + torch.sum(gq * w['quad']) + torch.sum(gt * w['tr']))
    step = 1e-5
    for name, grad in (('mu', d_mu), ('s', d_s)):
        for i in range(c[name].numel()):
            e = torch.zeros(c[name].numel(), dtype=torch.float64)
            e[i] = step
            e = e.reshape(c[name].shape)
            up = loss(c['mu'] + e, c['s']) if name == 'mu' else loss(c['mu'], c['s'] + e)
            dn = loss(c['mu'] - e, c['s']) if name == 'mu' else loss(c['mu'], c['s'] - e)
            want = float(grad.reshape(-1)[i])
            assert abs((up - dn) / (2.0 * step) - want) <= 1e-5 * max(1.0, abs(want)), (name, i)


def test_combination_step_vjp_against_autograd():
    from dp_gp_lvm_amd import ops
    k, g, j, n = 3, 4, 9, 6
    rs = np.random.default_rng(5)
    psi1r, quad = (torch.as_tensor(rs.standard_normal((k, n, j)), dtype=torch.float64).requires_grad_(True) for _ in range(2))
    tr = torch.as_tensor(rs.standard_normal((k, n, g))).requires_grad_(True)
    g_mean, g_var = torch.as_tensor(rs.standard_normal((k, n, j))), torch.as_tensor(rs.standard_normal((k, n, j)))
    for kind in ('random', 'last', 'mixed'):
        gidx = gidx_of(kind, k, g, j)
        idx = gidx.long()
        seen = ((idx >= 0) & (idx < g)).to(torch.float64)[:, None, :]
        var = 3.0 - torch.gather(tr, 2, idx.clamp(0, g - 1)[:, None, :].expand(-1, n, -1)) * seen + quad - psi1r * psi1r
        want = torch.autograd.grad(torch.sum(g_mean * psi1r) + torch.sum(g_var * var), (psi1r, quad, tr))
        have = ops.point_moments_adjoints(gidx, g, psi1r.detach(), g_mean, g_var)
        for hv, wv, name in zip(have, want, ('h', 'gq', 'gt')):
            close(hv, wv.numpy(), 1e-14, kind + ' ' + name)
        if kind == 'mixed':
            assert float(have[2].abs().sum()) < float(g_var.abs().sum())          # (-1 and G: those columns add nothing)


def test_mixture_moments_vjp_against_autograd():
    from dp_gp_lvm_amd.models.frozen_bound_t import mixture_moments
    from dp_gp_lvm_amd.models.predictor import mixture_moments_vjp
    t, n, j = 4, 5, 3
    rs = np.random.default_rng(9)
    phit = torch.softmax(torch.as_tensor(rs.standard_normal((t, j))), dim=0)
    mean_t = torch.as_tensor(rs.standard_normal((t, n, j))).requires_grad_(True)
    var_t = torch.as_tensor(rs.uniform(0.1, 2.0, (t, n, j))).requires_grad_(True)
    g_mean, g_var = torch.as_tensor(rs.standard_normal((n, j))), torch.as_tensor(rs.standard_normal((n, j)))
    mean, var = mixture_moments(phit, mean_t, var_t)
    want = torch.autograd.grad(torch.sum(g_mean * mean) + torch.sum(g_var * var), (mean_t, var_t))
    have = mixture_moments_vjp(phit, mean_t.detach(), mean.detach(), g_mean, g_var)
    close(have[0], want[0].numpy(), 1e-14, 'g_mean_t')
    close(have[1], want[1].numpy(), 1e-14, 'g_var_t')


def test_case_table():
    from dp_gp_lvm_amd import _lib
    assert len(CASES) == 7 and len(set(CASES)) == 7
    for k, g, j, m, q, n in CASES:
        # (the operator takes K, G, J, N, M, Q)
        assert _lib.lib().dpgp_qx_psi_pointwise_adjoint_workspace_bytes(k, g, j, n, m, q) > 0
    assert any(g + j > 64 for _, g, j, _, _, _ in CASES) and any(q == 64 for *_, q, _ in CASES) and any(q == 17 for *_, q, _ in CASES)
