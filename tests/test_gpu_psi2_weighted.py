"""GPU tests of the two weighted fp64 operators of the masked over-D model: ops.psi2(weights=) (dpgp_psi2_weighted_f64,
csrc/psi2.hip) and ops.elbo_grad_psi(prec='f64', weights=) (dpgp_elbo_grad_psi_weighted_f64, csrc/grad.hip).

Forward references, both held to 1e-12 of each matrix's largest entry (the project's operator tolerance): a plain fp64 torch
restatement of rbf_kernel.py:164-199 with the weight on the sum over n (the Psi2 part of test_gpu_train_masked.restated_param
with one shared z), and, for 0 / 1 weights, the unweighted ops.psi2 on the rows with weight 1, per kernel.
Backward references: torch autograd of the restatement at 1e-8 of each result's largest entry (what test_gpu_grad.py holds the
fp64 stage B to), and, for 0 / 1 weights, the unweighted operator called per column on its rows (d_mu, d_s scattered back, d_z
summed) at 1e-12.  M = 130 goes through the 64-point blocks of ops._elbo_grad_psi_f64_blocks.
Also: weights=None returns the bits of the call without weights, all-ones weights agree with it to 1e-14, two calls give the
same bits, every result is exactly symmetric, and a kernel whose weights are all 0 gets exactly 0.0."""
import itertools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F64 = torch.float64
KINDS = ['binary', 'tail', 'block', 'kernel_off', 'positive', 'none']
ALGOS = ['auto', 'plain']
GRID = list(itertools.product([1, 3], [1, 17, 64, 65, 130], [1, 5, 33, 129], [1, 10, 13, 23]))


def case(dev, b, n, m, q, seed):
    rs = np.random.default_rng(seed)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=F64, device=dev)
    mp = 16 * ((m + 15) // 16)
    g2 = rs.standard_normal((b, m, m))
    g2 = np.pad(g2 + g2.transpose(0, 2, 1), ((0, 0), (0, mp - m), (0, mp - m)))
    wk = rs.standard_normal((b, m, m))
    wk = np.pad(wk + wk.transpose(0, 2, 1), ((0, 0), (0, mp - m), (0, mp - m)))
    gv = np.pad(rs.standard_normal((b, m)), ((0, 0), (0, mp - m)))
    return dict(z=t(rs.standard_normal((m, q))), mu=t(rs.standard_normal((n, q))), s=t(rs.uniform(0.1, 1.5, (n, q))),
                gamma=t(rs.uniform(0.2, 2.0, (b, q))), alpha=t(rs.uniform(0.5, 2.0, b)), y=t(rs.standard_normal((n, b))),
                g_psi2=t(g2), w_kuu=t(wk), g_v=t(gv))


def weights(kind, b, n, seed, dev):
    rs = np.random.default_rng(seed)
    if kind == 'none':
        return None
    if kind == 'binary':                                     # 30 % zeros
        w = (rs.random((b, n)) >= 0.3).astype(np.float64)
    elif kind == 'tail':                                     # the last ceil(N / 3) rows zero
        w = np.ones((b, n))
        w[:, n - math.ceil(n / 3):] = 0.0
    elif kind == 'block':                                    # the first half zero
        w = np.ones((b, n))
        w[:, :n // 2] = 0.0
    elif kind == 'kernel_off':                               # one kernel all zero, the others 0 / 1
        w = (rs.random((b, n)) >= 0.3).astype(np.float64)
        w[rs.integers(0, b)] = 0.0
    else:                                                    # 'positive'
        w = rs.uniform(0.25, 4.0, (b, n))
    return torch.as_tensor(w, dtype=F64, device=dev).contiguous()


def restated_psi2(z, mu, s, gamma, alpha, w):
    """sum_n w[b,n] psi2_bn [B,M,M], the literal formula in chunks of observations."""
    b_, (m_, q_) = gamma.shape[0], z.shape
    step = max(1, int(2e7 // max(1, b_ * m_ * m_ * q_)))
    zbar = 0.5 * (z[:, None, :] + z[None, :, :])                                           # [M,M,Q]
    t1 = 0.25 * gamma[:, None, None, :] * (z[:, None, :] - z[None, :, :]) ** 2             # [B,M,M,Q]
    out = 0.0
    for n0 in range(0, mu.shape[0], step):
        mc, sc = mu[n0:n0 + step], s[n0:n0 + step]
        gq = gamma[:, None, None, None, :]
        den2 = 2.0 * gq * sc[None, :, None, None, :] + 1.0                                  # [B,n,1,1,Q]
        num2 = gq * (mc[None, :, None, None, :] - zbar[None, None]) ** 2                    # [B,n,M,M,Q]
        lg = 2.0 * torch.log(alpha)[:, None, None, None] - torch.sum(0.5 * torch.log(den2) + t1[:, None] + num2 / den2, dim=-1)
        out = out + (w[:, n0:n0 + step, None, None] * torch.exp(lg)).sum(dim=1)
    return out


def restated_grad(c, w, m):
    """d/d(mu, s, z, gamma) of sum_d <g_psi2_d, sum_n w[d,n] psi2_dn> + <g_v_d, Psi1_d^T y_d> + <w_kuu_d, log K_uu,d> (the K_uu
    term: d K = K .* d log K with w_kuu = G_K .* K held fixed; alpha a constant factor), by torch autograd."""
    z, mu, s, gamma = (c[k].detach().clone().requires_grad_() for k in ('z', 'mu', 's', 'gamma'))
    alpha = c['alpha']
    f = torch.sum(c['g_psi2'][:, :m, :m] * restated_psi2(z, mu, s, gamma, alpha, w))
    ga = gamma[:, None, None, :]
    den1 = ga * s[None, :, None, :] + 1.0                                                  # [D,N,1,Q]
    num1 = ga * (mu[None, :, None, :] - z[None, None, :, :]) ** 2                          # [D,N,M,Q]
    psi1 = alpha[:, None, None] * torch.exp(-0.5 * torch.sum(num1 / den1 + torch.log(den1), dim=-1))
    f = f + torch.sum(c['g_v'][:, :m] * torch.einsum('dnm,nd->dm', psi1, c['y']))
    logk = -0.5 * torch.sum(ga * (z[None, :, None, :] - z[None, None, :, :]) ** 2, dim=-1)   # [D,M,M]
    f = f + torch.sum(c['w_kuu'][:, :m, :m] * logk)
    return [g.cpu().numpy() for g in torch.autograd.grad(f, [mu, s, z, gamma])]


def close(got, want, tol, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.cpu().numpy() if isinstance(want, torch.Tensor) else want
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * max(np.abs(want).max(), 1e-300), err_msg=what)


def close_per_matrix(got, want, tol, what):
    for i in range(want.shape[0]):
        np.testing.assert_allclose(got[i].cpu().numpy(), want[i].cpu().numpy(), rtol=0, atol=tol * float(want[i].abs().max()),
                                   err_msg='%s, kernel %d' % (what, i))


def per_kernel_unweighted(ops, c, w, algo):
    """For 0 / 1 weights: the unweighted operator on the rows with weight 1, kernel by kernel (no rows: zeros)."""
    b, m = c['gamma'].shape[0], c['z'].shape[0]
    out = torch.zeros((b, m, m), dtype=F64, device=w.device)
    for i in range(b):
        rows = torch.nonzero(w[i] == 1.0)[:, 0]
        if rows.numel():
            out[i] = ops.psi2(c['z'], c['mu'][rows].contiguous(), c['s'][rows].contiguous(), c['gamma'][i:i + 1],
                              c['alpha'][i:i + 1], algo=algo)[0]
    return out


@pytest.mark.parametrize('b,m,n,q', GRID)
def test_forward_matches_both_references(dev, b, m, n, q):
    from dp_gp_lvm_amd import ops
    seed = 1000 * b + 10 * m + q + n
    c = case(dev, b, n, m, q, seed)
    args = (c['z'], c['mu'], c['s'], c['gamma'], c['alpha'])
    ones = torch.ones((b, n), dtype=F64, device=dev)
    wts = {kind: weights(kind, b, n, seed + 1, dev) for kind in KINDS}
    refs = {kind: restated_psi2(*args, ones if w is None else w) for kind, w in wts.items()}     # once, shared by both kernels
    for algo in ALGOS:
        plain = ops.psi2(*args, algo=algo)
        for kind in KINDS:
            w = wts[kind]
            what = '%s, %s' % (kind, algo)
            got = ops.psi2(*args, algo=algo, weights=w)
            assert torch.equal(got, ops.psi2(*args, algo=algo, weights=w)), what + ': two calls differ'
            assert torch.equal(got, got.transpose(1, 2)), what + ': not symmetric'
            close_per_matrix(got, refs[kind], 1e-12, what + ' (restatement)')
            if kind == 'none':
                assert torch.equal(got, plain), what + ': weights=None must be the unweighted call'
            elif kind != 'positive':
                close_per_matrix(got, per_kernel_unweighted(ops, c, w, algo), 1e-12, what + ' (unweighted on the rows)')
            if kind == 'kernel_off':
                off = torch.nonzero(w.sum(dim=1) == 0)[:, 0]
                assert off.numel() >= 1 and torch.count_nonzero(got[off]) == 0, what + ': an all-zero kernel must give exactly 0.0'
        close_per_matrix(ops.psi2(*args, algo=algo, weights=ones), plain, 1e-14, 'all ones, %s' % algo)


def per_column_unweighted_grad(ops, c, w, m):
    """For 0 / 1 weights and y zero-filled to match: the unweighted stage B per column on its rows; d_mu, d_s scattered back,
    d_z summed.  A column without rows keeps its K_uu term (one row with y = 0 and a zero Psi2 adjoint carries it)."""
    d, (n, q) = c['gamma'].shape[0], c['mu'].shape
    dev = w.device
    dmu, ds = torch.zeros((n, q), dtype=F64, device=dev), torch.zeros((n, q), dtype=F64, device=dev)
    dz, dg = torch.zeros((m, q), dtype=F64, device=dev), torch.zeros((d, q), dtype=F64, device=dev)
    for i in range(d):
        rows = torch.nonzero(w[i] == 1.0)[:, 0]
        g2 = c['g_psi2'][i:i + 1]
        y = c['y']
        if rows.numel() == 0:
            rows, g2, y = torch.zeros(1, dtype=torch.long, device=dev), torch.zeros_like(g2), torch.zeros_like(y)
        a, b_, c_, e = ops.elbo_grad_psi(y[rows, i:i + 1].contiguous(), c['z'], c['mu'][rows].contiguous(), c['s'][rows].contiguous(),
                                         c['gamma'][i:i + 1], c['alpha'][i:i + 1], g2.contiguous(), c['w_kuu'][i:i + 1].contiguous(),
                                         c['g_v'][i:i + 1].contiguous(), prec='f64')
        dmu[rows] += a
        ds[rows] += b_
        dz += c_
        dg[i] = e[0]
    return dmu, ds, dz, dg


NAMES = ('d mu', 'd S', 'd z', 'd gamma')


@pytest.mark.parametrize('b,m,n,q', GRID)
def test_backward_matches_both_references(dev, b, m, n, q):
    from dp_gp_lvm_amd import ops
    seed = 1000 * b + 10 * m + q + n + 7
    c = case(dev, b, n, m, q, seed)
    ones = torch.ones((b, n), dtype=F64, device=dev)

    def run(c_, w):
        return ops.elbo_grad_psi(c_['y'], c_['z'], c_['mu'], c_['s'], c_['gamma'], c_['alpha'], c_['g_psi2'], c_['w_kuu'], c_['g_v'],
                                 prec='f64', weights=w)
    plain = ops.elbo_grad_psi(c['y'], c['z'], c['mu'], c['s'], c['gamma'], c['alpha'], c['g_psi2'], c['w_kuu'], c['g_v'], prec='f64')
    for kind in KINDS:
        w = weights(kind, b, n, seed + 1, dev)
        cc = dict(c)
        if kind not in ('none', 'positive'):
            cc['y'] = (c['y'] * w.t()).contiguous()              # the caller zero-fills y: it alone governs the Psi1 term
        got = run(cc, w)
        again = run(cc, w)
        want = restated_grad(cc, ones if w is None else w, m)
        for name, g, a, r in zip(NAMES, got, again, want):
            what = '%s, %s' % (name, kind)
            assert torch.equal(g, a), what + ': two calls differ'
            close(g, r, 1e-8, what + ' (autograd of the restatement)')
        if kind == 'none':
            for name, g, p in zip(NAMES, got, plain):
                assert torch.equal(g, p), '%s: weights=None must be the unweighted call' % name
        elif kind != 'positive':
            for name, g, r in zip(NAMES, got, per_column_unweighted_grad(ops, cc, w, m)):
                close(g, r, 1e-12, '%s, %s (unweighted per column on its rows)' % (name, kind))
        if kind == 'kernel_off':
            # the Psi2 share of d_gamma alone (no Psi1 and K_uu terms): exactly 0.0 for the kernel whose weights are all 0
            z0 = dict(cc, w_kuu=torch.zeros_like(c['w_kuu']), g_v=torch.zeros_like(c['g_v']))
            off = torch.nonzero(w.sum(dim=1) == 0)[:, 0]
            assert off.numel() >= 1 and torch.count_nonzero(run(z0, w)[3][off]) == 0
    for name, g, p in zip(NAMES, run(c, ones), plain):
        close(g, p, 1e-14, '%s, all ones' % name)


def split_rows(n, ns):
    """Rows per split of the matrix-core kernel for a forced split count (psi2_nsplit, launch_psi2_ks of csrc/psi2.hip)."""
    while ns > 1 and (ns - 1) * -(-n // ns) >= n:
        ns -= 1
    return 32 * -(-(-(-n // ns)) // 32)


@pytest.mark.parametrize('pattern', ['straddle', 'whole_split'])
@pytest.mark.parametrize('ns,n,q', list(itertools.product([2, 5], [57, 65], [4, 22])))
def test_forced_splits(dev, monkeypatch, ns, n, q, pattern):
    """DPGP_PSI2_NS forces the number of n-splits: zero rows straddling a split boundary, and one split whose rows are all zero."""
    from dp_gp_lvm_amd import ops
    b, m = 3, 40
    c = case(dev, b, n, m, q, 31 * ns + n + q)
    args = (c['z'], c['mu'], c['s'], c['gamma'], c['alpha'])
    nper = split_rows(n, ns)
    assert nper < n                                             # more than one split holds rows
    w = np.ones((b, n))
    if pattern == 'straddle':
        w[:, nper - 5:nper + 3] = 0.0
        w[1, nper - 1:nper + 1] = 1.0                          # (one kernel keeps the two rows at the boundary itself)
    else:
        w[:, nper:2 * nper] = 0.0                              # the second split: all of its rows
    w = torch.as_tensor(w, dtype=F64, device=dev)
    want = restated_psi2(*args, w)
    monkeypatch.setenv('DPGP_PSI2_NS', str(ns))
    got = ops.psi2(*args, weights=w)
    assert torch.equal(got, ops.psi2(*args, weights=w)) and torch.equal(got, got.transpose(1, 2))
    close_per_matrix(got, want, 1e-12, 'forced splits (restatement)')
    close_per_matrix(got, per_kernel_unweighted(ops, c, w, 'auto'), 1e-12, 'forced splits (unweighted on the rows)')
    close_per_matrix(ops.psi2(*args, weights=torch.ones_like(w)), ops.psi2(*args), 1e-14, 'forced splits, all ones')


def test_argument_checks(dev):
    from dp_gp_lvm_amd import ops
    c = case(dev, 2, 9, 5, 3, 0)
    args = (c['z'], c['mu'], c['s'], c['gamma'], c['alpha'])
    w = torch.ones((2, 9), dtype=F64, device=dev)
    with pytest.raises(AssertionError):
        ops.psi2(*(a.float() for a in args), weights=w)
    with pytest.raises(TypeError):
        ops.psi2(*args, weights=w.float())
    with pytest.raises(AssertionError):
        ops.psi2(*args, weights=w[:, :8].contiguous())
    with pytest.raises(ValueError):
        ops.psi2(*args, algo='mfma_f32', weights=w)
    for prec in ('mixed', 'mixed_fast', 'f32'):
        with pytest.raises(AssertionError):
            ops.elbo_grad_psi(c['y'], c['z'], c['mu'], c['s'], c['gamma'], c['alpha'], c['g_psi2'], c['w_kuu'], c['g_v'], prec=prec,
                              weights=w)
