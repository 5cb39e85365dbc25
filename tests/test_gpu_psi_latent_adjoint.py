"""GPU tests of the shared-inducing latent adjoint (dpgp_psi_latent_adjoint_f64, csrc/psi_latent_adjoint.hip; ops.psi_latent_adjoint):
(d_mu, d_s) of  L = sum_b <g_psi2_b, sum_n w[b,n] psi2_bn> + sum_b g_v_b . (Psi1_b^T y_b)  for B kernels that share z and q(X*).

Reference: torch fp64 autograd of a restatement of L on the CPU; bound atol = 1e-8 max|want| (the project's adjoint tolerance, the
measure of test_gpu_psi2_weighted.py).  The restatement forms every point's psi2 term explicitly from zbar = (z_m + z_m') / 2 where
that is small (N M M Q <= 2e6) and otherwise through (mu - zbar)^2 = 1/2 (mu - z_m)^2 + 1/2 (mu - z_m')^2 - 1/4 (z_m - z_m')^2, whose
q-sum over the pairs is one matrix product; one reference per case, cached.  Against the library's other routes to the same numbers,
ops.elbo_grad_psi(prec='f64', weights=, w_kuu=0) (M <= 128, Q <= 30) and ops.qx_psi_adjoint(weights=) on B replicated copies of z
with g1 = y (x) g_v: 1e-10.

Shapes: B in {1, 3, 17} x M in {1, 17, 64, 65, 130} x N in {1, 5, 33, 129} x Q in {1, 8, 10, 23} and (3, 17, 5, 64): pair counts and
N off the 4 / 16 MFMA steps, 1 + 2Q = 3 / 17 / 21 / 47 / 129 off the 16-column tiles (129: two chunks), M past one 32-tile and past
128.  Every case of the grid takes one of the weight kinds in turn; test_weight_kinds runs all of them on four shapes.

Slabs.  The plan gives every column b its own slab whenever ceil(N / 64) B <= 512, so every B > 1 case here adds partial sums
across column-slab boundaries, and it splits the pair tiles over slabs at small N B (e.g. B = 1, M = 130, N = 5: 15 tiles in 15
slabs).  Slabs of SEVERAL columns (the accumulation inside a workgroup across columns, what B = 512 runs) and chosen pair-tile splits
are forced with DPGP_PLA_COL_SLABS / DPGP_PLA_PAIR_SLABS, the knobs of pl_plan (as DPGP_PSI2_NS in test_gpu_psi2_weighted.py)."""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F64 = torch.float64
KINDS = ['none', 'binary', 'zero_column', 'runs', 'positive']
GRID = list(itertools.product((1, 3, 17), (1, 17, 64, 65, 130), (1, 5, 33, 129), (1, 8, 10, 23))) + [(3, 17, 5, 64)]


def weights_of(kind, b, n, rs):
    if kind == 'none':
        return None
    if kind == 'ones':
        return np.ones((b, n))
    if kind == 'binary':
        return (rs.random((b, n)) >= 0.3).astype(np.float64)
    if kind == 'zero_column':                        # 0 / 1 at random and one column with no test point at all
        w = (rs.random((b, n)) >= 0.3).astype(np.float64)
        w[b // 2] = 0.0
        return w
    if kind == 'runs':                               # all-zero leading and trailing 16-point runs: whole waves without a point
        w = np.ones((b, n))
        w[:, :16] = 0.0
        w[::2, max(n - 16, 0):] = 0.0
        w[1::2, max(n - 40, 0):max(n - 20, 0)] = 0.0
        return w
    if kind == 'positive':
        return rs.uniform(0.1, 3.0, (b, n))
    if kind == 'signed':
        return rs.standard_normal((b, n))
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def case(b, m, n, q, kind, shift=0.0):
    """Inputs on the CPU (torch fp64): points near the inducing inputs, y zero where the weight is zero (and in a few more places)."""
    rs = np.random.default_rng(1000003 * b + 10007 * m + 101 * n + q + 17 * (KINDS + ['ones', 'signed']).index(kind))
    z = rs.standard_normal((m, q)) + shift
    mu = z[rs.integers(0, m, n)] + 0.3 * rs.standard_normal((n, q))
    w = weights_of(kind, b, n, rs)
    y = rs.standard_normal((n, b))
    if w is not None:
        y = np.where(w.T != 0.0, y, 0.0)
    y[rs.random((n, b)) < 0.1] = 0.0
    c = dict(z=z, mu=mu, s=rs.uniform(0.05, 1.5, (n, q)), gamma=rs.uniform(0.3, 2.0, (b, q)) / q ** 0.5, alpha=rs.uniform(0.5, 2.0, b),
             y=y, g_v=rs.standard_normal((b, m)), g_psi2=rs.standard_normal((b, m, m)))          # g_psi2: not symmetric
    c = {k: torch.as_tensor(v, dtype=F64) for k, v in c.items()}
    c['w'] = None if w is None else torch.as_tensor(w, dtype=F64)
    return c


def restated_l(c, mu, s):
    """L as a torch expression of (mu, s), column by column."""
    z, gamma, alpha, y, g_v, g2, w = (c[k] for k in ('z', 'gamma', 'alpha', 'y', 'g_v', 'g_psi2', 'w'))
    m, q = z.shape
    n = mu.shape[0]
    dz2 = (z[:, None, :] - z[None, :, :]) ** 2                                             # [M, M, Q]
    dmu2 = (mu[:, None, :] - z[None, :, :]) ** 2                                           # [N, M, Q]
    total = torch.zeros((), dtype=F64)
    for b in range(gamma.shape[0]):
        g, a = gamma[b], alpha[b]
        den1 = g * s + 1.0
        psi1 = a * torch.exp(-0.5 * torch.sum(torch.log(den1), dim=1))[:, None] * \
            torch.exp(-0.5 * torch.sum((g / den1)[:, None, :] * dmu2, dim=2))             # [N, M]
        total = total + torch.sum(y[:, b] * (psi1 @ g_v[b]))
        den2 = 2.0 * g * s + 1.0
        c2 = torch.exp(-0.5 * torch.sum(torch.log(den2), dim=1))                          # [N]
        gr = g / den2                                                                      # [N, Q]
        fac = a * a * torch.exp(-0.25 * torch.sum(g * dz2, dim=2)) * g2[b]                # [M, M]
        if n * m * m * q <= 2e6:
            zbar = 0.5 * (z[:, None, :] + z[None, :, :])
            ex = torch.sum(gr[:, None, None, :] * (mu[:, None, None, :] - zbar[None]) ** 2, dim=3)         # [N, M, M]
        else:
            e1 = torch.sum(gr[:, None, :] * dmu2, dim=2)                                   # [N, M]
            ex = 0.5 * (e1[:, :, None] + e1[:, None, :]) - 0.25 * (gr @ dz2.reshape(m * m, q).T).reshape(n, m, m)
        per_point = c2 * torch.sum(torch.exp(-ex) * fac[None], dim=(1, 2))                # [N]
        total = total + torch.sum(per_point if w is None else w[b] * per_point)
    return total


@functools.lru_cache(maxsize=None)
def want_of(b, m, n, q, kind, shift=0.0):
    c = case(b, m, n, q, kind, shift)
    mu, s = c['mu'].clone().requires_grad_(True), c['s'].clone().requires_grad_(True)
    restated_l(c, mu, s).backward()
    return mu.grad.numpy(), s.grad.numpy()


def close(got, want, tol, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    top = max(np.abs(want).max(), 1e-300)
    print('%s: max |err| %.3e of %.3e (bound %.0e of that)' % (what, np.abs(got - want).max(), top, tol))
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * top, err_msg=what)


def run(dev, c, w='own', g_psi2=None):
    from dp_gp_lvm_amd import ops
    d = {k: v.to(dev) for k, v in c.items() if v is not None}
    w = d.get('w') if isinstance(w, str) else (None if w is None else w.to(dev))
    return ops.psi_latent_adjoint(d['z'], d['mu'], d['s'], d['gamma'], d['alpha'], d['y'], d['g_v'],
                                  d['g_psi2'] if g_psi2 is None else g_psi2.to(dev), weights=w)


def other_routes(dev, c):
    """(name, d_mu, d_s) by the library's older operators, on the symmetric part of g_psi2 (what stage A hands them)."""
    from dp_gp_lvm_amd import ops
    d = {k: v.to(dev) for k, v in c.items() if v is not None}
    (m, q), b = d['z'].shape, d['gamma'].shape[0]
    w = d.get('w')
    gs = 0.5 * (d['g_psi2'] + d['g_psi2'].transpose(1, 2))
    out = []
    if m <= 128 and q <= 30:
        mp = 16 * ((m + 15) // 16)
        pad = torch.nn.functional.pad
        gp = pad(gs, (0, mp - m, 0, mp - m)).contiguous()
        r = ops.elbo_grad_psi(d['y'].contiguous(), d['z'], d['mu'], d['s'], d['gamma'], d['alpha'][:, None].contiguous(), gp,
                              torch.zeros_like(gp), pad(d['g_v'], (0, mp - m)).contiguous(), prec='f64', weights=w)
        out.append(('elbo_grad_psi', r[0], r[1]))
    g1 = (d['y'].T[:, :, None] * d['g_v'][:, None, :]).contiguous()
    r = ops.qx_psi_adjoint(d['z'][None].expand(b, m, q).contiguous(), d['mu'], d['s'], d['gamma'], d['alpha'], g1, gs.contiguous(), weights=w)
    out.append(('qx_psi_adjoint', r[0], r[1]))
    return out


@pytest.mark.parametrize('b,m,n,q', GRID)
def test_against_autograd_and_the_other_operators(dev, b, m, n, q):
    kind = KINDS[GRID.index((b, m, n, q)) % len(KINDS)]
    c = case(b, m, n, q, kind)
    want = want_of(b, m, n, q, kind)
    got = run(dev, c)
    again = run(dev, c)
    tag = 'B %d M %d N %d Q %d, weights %s: ' % (b, m, n, q, kind)
    assert tuple(got[0].shape) == (n, q) and tuple(got[1].shape) == (n, q)
    for name, g, g_again, w_ in zip(('d_mu', 'd_s'), got, again, want):
        close(g, w_, 1e-8, tag + name + ' against autograd')
        assert torch.equal(g, g_again), tag + name + ': two runs differ'
    # a non-symmetric g_psi2 and its symmetric part are the same functional
    sym = run(dev, c, g_psi2=0.5 * (c['g_psi2'] + c['g_psi2'].transpose(1, 2)))
    for name, g, g_sym in zip(('d_mu', 'd_s'), got, sym):
        close(g_sym, g, 1e-14, tag + name + ' of the symmetric part of g_psi2')
    for route, a_mu, a_s in other_routes(dev, c):
        close(got[0], a_mu, 1e-10, tag + 'd_mu against ' + route)
        close(got[1], a_s, 1e-10, tag + 'd_s against ' + route)


@pytest.mark.parametrize('kind', KINDS + ['ones', 'signed'])
@pytest.mark.parametrize('b,m,n,q', [(3, 17, 33, 8), (17, 65, 129, 10), (3, 130, 5, 23), (1, 64, 129, 1)])
def test_weight_kinds(dev, b, m, n, q, kind):
    """Every kind of weights on four shapes ('signed': any finite reals, which only the autograd restatement takes)."""
    c = case(b, m, n, q, kind)
    got = run(dev, c)
    tag = 'B %d M %d N %d Q %d, weights %s: ' % (b, m, n, q, kind)
    for name, g, w_ in zip(('d_mu', 'd_s'), got, want_of(b, m, n, q, kind)):
        close(g, w_, 1e-8, tag + name + ' against autograd')
    if kind == 'ones':                               # weights of one against no weights
        for name, g, g0 in zip(('d_mu', 'd_s'), got, run(dev, c, w=None)):
            close(g, g0, 1e-14, tag + name + ' against weights=None')
    elif kind != 'signed':
        for route, a_mu, a_s in other_routes(dev, c):
            close(got[0], a_mu, 1e-10, tag + 'd_mu against ' + route)
            close(got[1], a_s, 1e-10, tag + 'd_s against ' + route)


@pytest.mark.parametrize('b,m,n,q', [(3, 17, 33, 8), (4, 65, 70, 10)])
def test_a_column_without_points_or_data_changes_no_bit(dev, monkeypatch, b, m, n, q):
    """A column with all-zero weights and all-zero y against the call without that column, under a plan that does not depend on B:
    one slab of columns (so the columns are added in ascending order inside the workgroup in both calls) and one of pair tiles."""
    monkeypatch.setenv('DPGP_PLA_COL_SLABS', '1')
    monkeypatch.setenv('DPGP_PLA_PAIR_SLABS', '1')
    c = dict(case(b, m, n, q, 'binary'))
    for at in (0, b // 2, b - 1):
        keep = [i for i in range(b) if i != at]
        full = dict(c, w=c['w'].clone(), y=c['y'].clone())
        full['w'][at] = 0.0
        full['y'][:, at] = 0.0
        less = dict(c, w=c['w'][keep].contiguous(), y=c['y'][:, keep].contiguous(), gamma=c['gamma'][keep].contiguous(),
                    alpha=c['alpha'][keep].contiguous(), g_v=c['g_v'][keep].contiguous(), g_psi2=c['g_psi2'][keep].contiguous())
        for name, g_full, g_less in zip(('d_mu', 'd_s'), run(dev, full), run(dev, less)):
            assert torch.equal(g_full, g_less), '%s: the empty column %d of %d moved bits' % (name, at, b)


def test_latents_shifted_by_fifty(dev):
    """z and mu moved by +50 in every latent dim: the moment forms expand (mu - zbar)^2; the kernel centres both on a test point."""
    for b, m, n, q in [(3, 65, 33, 10), (3, 17, 129, 23)]:
        c = case(b, m, n, q, 'binary', 50.0)
        want = want_of(b, m, n, q, 'binary', 50.0)
        for name, g, w_ in zip(('d_mu', 'd_s'), run(dev, c), want):
            close(g, w_, 1e-8, 'shifted by 50, B %d M %d N %d Q %d: %s' % (b, m, n, q, name))


@pytest.mark.parametrize('cs,ps', [(1, 1), (2, 1), (5, 3), (17, 1), (1, 6), (4, 15)])
def test_forced_slabs(dev, monkeypatch, cs, ps):
    """DPGP_PLA_COL_SLABS / DPGP_PLA_PAIR_SLABS force the numbers of column slabs and of pair-tile slabs (clamped to B and to the
    tiles): slabs of several columns with a ragged last one (17 columns in 5 slabs of 4, 4, 4, 4, 1), an all-zero column at a slab
    boundary, pair-tile splits that cut the block triangle inside a block row (M = 130: 15 tiles), all against the same autograd
    values and the natural plan."""
    from dp_gp_lvm_amd import _lib
    b, m, n, q = 17, 130, 33, 10
    c = dict(case(b, m, n, q, 'zero_column'))
    c['w'] = c['w'].clone()
    c['w'][3] = 0.0                                  # (the last column of the first slab of 4)
    natural = run(dev, c)
    mu, s = c['mu'].clone().requires_grad_(True), c['s'].clone().requires_grad_(True)
    restated_l(c, mu, s).backward()
    monkeypatch.setenv('DPGP_PLA_COL_SLABS', str(cs))
    monkeypatch.setenv('DPGP_PLA_PAIR_SLABS', str(ps))
    cols_per_slab = -(-b // cs)
    tiles_per_slab = -(-15 // ps)
    slabs = -(-b // cols_per_slab) * -(-15 // tiles_per_slab)
    assert _lib.lib().dpgp_psi_latent_adjoint_workspace_bytes(b, n, m, q) == slabs * 2 * n * q * 8, 'the plan did not take the knobs'
    got, again = run(dev, c), run(dev, c)
    for name, g, g2, g_nat, w_ in zip(('d_mu', 'd_s'), got, again, natural, (mu.grad, s.grad)):
        close(g, w_, 1e-8, 'col slabs %d, pair slabs %d: %s against autograd' % (cs, ps, name))
        close(g, g_nat, 1e-12, 'col slabs %d, pair slabs %d: %s against the natural plan' % (cs, ps, name))
        assert torch.equal(g, g2), 'two runs differ'


def test_argument_checks(dev):
    from dp_gp_lvm_amd import ops
    c = case(3, 17, 5, 8, 'binary')
    d = {k: v.to(dev) for k, v in c.items()}
    args = [d[k] for k in ('z', 'mu', 's', 'gamma', 'alpha', 'y', 'g_v', 'g_psi2')]
    ops.psi_latent_adjoint(*args, weights=d['w'])
    with pytest.raises(TypeError):
        ops.psi_latent_adjoint(*args, weights=d['w'].float())
    with pytest.raises(AssertionError):
        ops.psi_latent_adjoint(*args, weights=d['w'][:, :-1].contiguous())
    with pytest.raises(AssertionError):
        ops.psi_latent_adjoint(*(args[:6] + [d['g_v'][:, :-1].contiguous(), d['g_psi2']]))
    with pytest.raises(AssertionError):
        ops.psi_latent_adjoint(*(args[:5] + [d['y'][:, :-1].contiguous()] + args[6:]))
    # y as a strided view of a wider matrix (ldy > B) is taken as it is
    wide = torch.zeros((5, 7), dtype=F64, device=dev)
    wide[:, :3] = d['y']
    a = ops.psi_latent_adjoint(*(args[:5] + [wide[:, :3]] + args[6:]), weights=d['w'])
    b_ = ops.psi_latent_adjoint(*args, weights=d['w'])
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])
