"""GPU tests of the per-point Psi2 contractions (dpgp_qx_psi_pointwise_f64, csrc/qx_psi_point.hip): tr [K,N,G] and quad [K,N,J]
against a torch-fp64 CPU restatement that forms every test point's own Psi2 term explicitly (in chunks of points).  Tolerance:
1e-12, the project's operator tolerance.  The shapes cover the smallest problem, M / N / G + J that are no multiples of 32 / 64 /
16, more than one chunk of columns (G + J > 128; > 64 at Q = 64), a chunk that mixes tr and quad columns, M over 128 (slabs of
pair tiles at small N), the register path (Q <= 16) and the LDS path at its bound (Q = 64)."""
import numpy as np
import pytest
import torch

from test_gpu_predict_b1 import close
from test_gpu_qx_psi_grouped import case_of

pytestmark = pytest.mark.gpu

#          K, G,  J,  M,  Q,  N
SHAPES = [(1, 1, 1, 1, 1, 1), (1, 1, 16, 32, 10, 64), (2, 3, 17, 33, 10, 65), (3, 2, 40, 65, 23, 130), (1, 9, 5, 128, 10, 70),
          (2, 1, 70, 50, 3, 100), (1, 2, 15, 40, 64, 70), (1, 4, 33, 200, 10, 33)]


def inputs_of(k, g, j, m, q, n, shift=0.0):
    seed = 100000 * k + 10000 * g + 100 * j + 10 * m + q + n
    c = case_of(k, g, m, q, n, 'binary', seed)
    rs = np.random.default_rng(seed + 1)
    out = {name: c[name] for name in ('z', 'mu', 's', 'gamma', 'alpha')}
    out['mu'] = out['mu'] + shift
    out['c'] = torch.as_tensor(rs.standard_normal((k, g, m, m)))                       # not symmetric
    out['r'] = torch.as_tensor(rs.standard_normal((k, m, j)))
    return out


def restated(c):
    """tr [K,N,G], quad [K,N,J], psi1 [K,N,M] and psi2 summed over the points [K,M,M]: torch fp64 on the CPU, psi2_kn formed
    explicitly, in chunks of points."""
    z, mu, s, gamma, alpha = (c[k] for k in ('z', 'mu', 's', 'gamma', 'alpha'))
    kk, m, q = z.shape
    n = mu.shape[0]
    step = max(1, int(1.5e7 // (m * m * q)))
    trs, quads, psi1s, psi2s = [], [], [], []
    for k in range(kk):
        den1 = gamma[k] * s[:, None, :] + 1.0
        num1 = gamma[k] * (mu[:, None, :] - z[k][None, :, :]) ** 2
        psi1s.append(torch.exp(torch.log(alpha[k]) - 0.5 * torch.sum(num1 / den1 + torch.log(den1), dim=-1)))
        zbar = 0.5 * (z[k][:, None, :] + z[k][None, :, :])
        t1 = 0.25 * gamma[k] * (z[k][:, None, :] - z[k][None, :, :]) ** 2
        tr, quad, psi2 = [], [], torch.zeros((m, m), dtype=torch.float64)
        for n0 in range(0, n, step):
            mc, sc = mu[n0:n0 + step], s[n0:n0 + step]
            den2 = 2.0 * gamma[k] * sc[:, None, None, :] + 1.0
            num2 = gamma[k] * (mc[:, None, None, :] - zbar[None]) ** 2
            psi2n = torch.exp(2.0 * torch.log(alpha[k]) - torch.sum(0.5 * torch.log(den2) + t1[None] + num2 / den2, dim=-1))
            tr.append(torch.einsum('gab,nab->ng', c['c'][k], psi2n))
            quad.append(torch.einsum('aj,nab,bj->nj', c['r'][k], psi2n, c['r'][k]))
            psi2 = psi2 + psi2n.sum(dim=0)
        trs.append(torch.cat(tr))
        quads.append(torch.cat(quad))
        psi2s.append(psi2)
    return dict(tr=torch.stack(trs), quad=torch.stack(quads), psi1=torch.stack(psi1s), psi2=torch.stack(psi2s))


def on(dev, c):
    return {name: a.to(dev).contiguous() for name, a in c.items()}


def pair_factor(d):
    dz = d['z'][:, :, None, :] - d['z'][:, None, :, :]
    return ((d['alpha'] ** 2)[:, None, None] * torch.exp(-0.25 * torch.sum(d['gamma'][:, None, None, :] * dz * dz, dim=-1))).contiguous()


def report(tag, name, have, want):
    print('%s%s: max |err| %.3e of %.3e (bound 1e-12 relative to max(1, that))' %
          (tag, name, float((have.cpu() - want).abs().max()), float(want.abs().max())))


@pytest.mark.parametrize('k,g,j,m,q,n', SHAPES)
def test_pointwise_operator(dev, k, g, j, m, q, n):
    from dp_gp_lvm_amd import ops
    c = inputs_of(k, g, j, m, q, n)
    want = restated(c)
    d = on(dev, c)
    args = (d['z'], d['mu'], d['s'], d['gamma'], d['alpha'])
    outs = {}
    for zf in (None, pair_factor(d)):
        tag = 'zfac=%s ' % (zf is not None)
        tr, quad = ops.qx_psi_pointwise(*args, d['c'], d['r'], zfac=zf)
        tr_b, quad_b = ops.qx_psi_pointwise(*args, d['c'], d['r'], zfac=zf)
        assert tuple(tr.shape) == (k, n, g) and tuple(quad.shape) == (k, n, j)
        report(tag, 'tr', tr, want['tr'])
        report(tag, 'quad', quad, want['quad'])
        close(tr, want['tr'].numpy(), 1e-12, tag + 'tr')
        close(quad, want['quad'].numpy(), 1e-12, tag + 'quad')
        assert torch.equal(tr, tr_b) and torch.equal(quad, quad_b), tag + 'two calls differ'
        outs[zf is not None] = (tr, quad)
        # c and its symmetric part give the same trace
        tr_s, _ = ops.qx_psi_pointwise(*args, (0.5 * (d['c'] + d['c'].transpose(2, 3))).contiguous(), d['r'], zfac=zf)
        close(tr_s, tr.cpu().numpy(), 1e-12, tag + 'tr of the symmetric part of c')
        # summed over the points: <c_kg, Psi2_k> of the statistics operator
        psi1, psi2 = ops.qx_psi_stats_batched(*args, zfac=zf)
        inner = torch.einsum('kgab,kab->kg', d['c'], psi2)
        report(tag, 'sum_n tr against <c, Psi2>', tr.sum(dim=1), inner.cpu())
        close(tr.sum(dim=1), inner.cpu().numpy(), 1e-12, tag + 'sum_n tr against <c, Psi2>')
        # Jensen: Psi2(n) - psi1(n) psi1(n)^T is positive semi-definite
        gap = quad - torch.matmul(psi1, d['r']) ** 2
        floor = -1e-12 * float(quad.abs().max())
        print(tag + 'min (quad - (Psi1 r)^2) = %.3e (bound %.3e)' % (float(gap.min()), floor))
        assert float(gap.min()) >= floor, tag + 'quad < (Psi1 r)^2'
    close(outs[False][0], outs[True][0].cpu().numpy(), 1e-12, 'tr: zfac=None against a given zfac')
    close(outs[False][1], outs[True][1].cpu().numpy(), 1e-12, 'quad: zfac=None against a given zfac')


def test_points_far_from_the_inducing_inputs(dev):
    """mu shifted by 30 in every dim: every exponent is far below the fp64 range of interest; the outputs are finite, 0 or tiny
    and agree with the restatement."""
    from dp_gp_lvm_amd import ops
    c = inputs_of(2, 3, 17, 33, 10, 65, shift=30.0)
    want = restated(c)
    d = on(dev, c)
    tr, quad = ops.qx_psi_pointwise(d['z'], d['mu'], d['s'], d['gamma'], d['alpha'], d['c'], d['r'])
    assert bool(torch.isfinite(tr).all()) and bool(torch.isfinite(quad).all())
    print('shifted: max |tr| %.3e (restated %.3e), max |quad| %.3e (restated %.3e)' %
          (float(tr.abs().max()), float(want['tr'].abs().max()), float(quad.abs().max()), float(want['quad'].abs().max())))
    assert float(tr.abs().max()) < 1e-100 and float(quad.abs().max()) < 1e-100
    close(tr, want['tr'].numpy(), 1e-12, 'shifted tr')
    close(quad, want['quad'].numpy(), 1e-12, 'shifted quad')


def test_argument_checks(dev):
    from dp_gp_lvm_amd import ops
    d = on(dev, inputs_of(2, 3, 4, 5, 2, 7))
    args = (d['z'], d['mu'], d['s'], d['gamma'], d['alpha'])
    with pytest.raises(TypeError):
        ops.qx_psi_pointwise(*args, d['c'].float(), d['r'])
    with pytest.raises(TypeError):
        ops.qx_psi_pointwise(*args, d['c'], d['r'].cpu().numpy())
    with pytest.raises(ValueError):
        ops.qx_psi_pointwise(*args, d['c'][:, :, :-1].contiguous(), d['r'])
    with pytest.raises(ValueError):
        ops.qx_psi_pointwise(*args, d['c'][:1].contiguous(), d['r'])
    with pytest.raises(ValueError):
        ops.qx_psi_pointwise(*args, d['c'], d['r'][:, :-1].contiguous())
    with pytest.raises(ValueError):
        ops.qx_psi_pointwise(*args, d['c'], d['r'][:, :, :0].contiguous())
