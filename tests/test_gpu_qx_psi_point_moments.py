"""GPU tests of the per-entry moments operator (dpgp_qx_psi_point_moments_f64, csrc/qx_psi_point.hip, ops.qx_psi_point_moments):
mean [K,N,J] and var [K,N,J] against the torch-fp64 CPU restatement of test_gpu_qx_psi_pointwise that forms every test point's
own Psi2 term explicitly.  Tolerance: 1e-12, the project's operator tolerance.  The shapes cover the smallest problem, every tile
edge (M / N / J no multiples of 32 / 64 / 16), two column chunks of the finishing kernel (J > 64) and of the pair kernel
(G + J > 128), the LDS point path of the pair kernel just past Q = 16, the Q bound, slabs of pair tiles at small N K, J below a
matrix-pipe tile (plain FMA finishing) and the over-D layout (G = J = 1, many kernels)."""
import numpy as np
import pytest
import torch

from test_gpu_predict_b1 import close
from test_gpu_qx_psi_pointwise import inputs_of, on, pair_factor, restated

pytestmark = pytest.mark.gpu

#          K, G,   J,   M,  Q,   N
SHAPES = [(1, 1, 1, 1, 1, 1), (2, 3, 17, 33, 10, 65), (1, 2, 130, 40, 10, 70), (3, 2, 40, 65, 17, 130), (1, 2, 15, 40, 64, 70),
          (1, 1, 5, 200, 10, 33), (5, 1, 1, 50, 10, 100)]
GIDX = ('random', 'last', 'mixed')
_CASES = {}


def gidx_of(kind, k, g, j):
    rs = np.random.default_rng(7 + 13 * k + g + 101 * j)
    if kind == 'random':
        a = rs.integers(0, g, (k, j))
    elif kind == 'last':
        a = np.full((k, j), g - 1)
    else:
        a = rs.integers(-1, g + 1, (k, j))                 # -1 and G: no trace term
        a.flat[0], a.flat[-1] = -1, g
    return torch.as_tensor(a, dtype=torch.int32)


def case(shape):
    """Inputs, beta and the restated tr / quad / psi1 of a shape: computed once, shared by the tests, never modified."""
    if shape not in _CASES:
        c = inputs_of(*shape)
        c['beta'] = torch.as_tensor(np.random.default_rng(sum(shape)).uniform(0.5, 20.0, shape[0]))
        _CASES[shape] = (c, restated(c))
    return _CASES[shape]


def moments_of(c, want, gidx):
    """(mean, var, largest term) from the restated pieces; gidx outside [0, G) behaves as -1: no trace term."""
    g = c['c'].shape[1]
    mean = torch.matmul(want['psi1'], c['r'])
    idx = gidx.long()
    seen = ((idx >= 0) & (idx < g)).to(torch.float64)[:, None, :]
    tr = torch.gather(want['tr'], 2, idx.clamp(0, g - 1)[:, None, :].expand(-1, mean.shape[1], -1)) * seen
    base = (c['alpha'] + 1.0 / c['beta'])[:, None, None]
    var = base - tr + want['quad'] - mean * mean
    top = max(float(base.max()), float(tr.abs().max()), float(want['quad'].abs().max()), float((mean * mean).max()))
    return mean, var, top


def run(d, gidx, zfac=None):
    from dp_gp_lvm_amd import ops
    return ops.qx_psi_point_moments(d['z'], d['mu'], d['s'], d['gamma'], d['alpha'], d['c'], d['r'], gidx.to(d['z'].device), d['beta'],
                                    zfac=zfac)


def close_var(have, want, top, msg):
    print('%s: max |err| %.3e of %.3e, largest term %.3e (bound 1e-12 relative to max(1, max |var|))' %
          (msg, float((have.cpu() - want).abs().max()), float(want.abs().max()), top))
    close(have, want.numpy(), 1e-12, msg)


@pytest.mark.parametrize('kind', GIDX)
@pytest.mark.parametrize('k,g,j,m,q,n', SHAPES)
def test_moments_operator(dev, k, g, j, m, q, n, kind):
    c, want = case((k, g, j, m, q, n))
    d = on(dev, c)
    gidx = gidx_of(kind, k, g, j)
    mean_w, var_w, top = moments_of(c, want, gidx)
    outs = {}
    for zf in (None, pair_factor(d)):
        tag = '%s zfac=%s ' % (kind, zf is not None)
        mean, var = run(d, gidx, zf)
        mean_b, var_b = run(d, gidx, zf)
        assert tuple(mean.shape) == (k, n, j) and tuple(var.shape) == (k, n, j)
        print('%smean: max |err| %.3e of %.3e' % (tag, float((mean.cpu() - mean_w).abs().max()), float(mean_w.abs().max())))
        close(mean, mean_w.numpy(), 1e-12, tag + 'mean')
        close_var(var, var_w, top, tag + 'var')
        assert torch.equal(mean, mean_b) and torch.equal(var, var_b), tag + 'two calls differ'
        outs[zf is not None] = (mean, var)
    close(outs[False][0], outs[True][0].cpu().numpy(), 1e-12, 'mean: zfac=None against a given zfac')
    close_var(outs[False][1], outs[True][1].cpu(), top, 'var: zfac=None against a given zfac')


@pytest.mark.parametrize('k,g,j,m,q,n', SHAPES)
def test_equals_the_composition_of_the_existing_operators(dev, k, g, j, m, q, n):
    from dp_gp_lvm_amd import ops
    c, _ = case((k, g, j, m, q, n))
    d = on(dev, c)
    gidx = gidx_of('mixed', k, g, j)
    args = (d['z'], d['mu'], d['s'], d['gamma'], d['alpha'])
    tr, quad = ops.qx_psi_pointwise(*args, d['c'], d['r'])
    if q <= 30:                                                 # (DPGP_MAX_Q of dpgp_psi1; above it the statistics operator's Psi1)
        psi_1 = torch.stack([ops.psi1(d['z'][i], d['mu'], d['s'], d['gamma'][i:i + 1], d['alpha'][i:i + 1])[0] for i in range(k)])
    else:
        psi_1 = ops.qx_psi_stats_batched(*args)[0]
    composed = moments_of(dict(c=d['c'], r=d['r'], alpha=d['alpha'], beta=d['beta']), dict(psi1=psi_1, tr=tr, quad=quad),
                          gidx.to(dev))
    mean, var = run(d, gidx)
    close(mean, composed[0].cpu().numpy(), 1e-12, 'mean against psi1 + matmul')
    close_var(var, composed[1].cpu(), composed[2], 'var against qx_psi_pointwise + psi1 + matmul')


def test_zero_columns_of_r(dev):
    """r = 0 in a column and no trace term: mean 0 and var = alpha + 1/beta, exactly."""
    shape = (2, 3, 17, 33, 10, 65)
    c, _ = case(shape)
    d = on(dev, c)
    zero = [0, 5, 16]
    r = d['r'].clone()
    r[:, :, zero] = 0.0
    gidx = gidx_of('random', 2, 3, 17)
    gidx[:, zero] = -1
    mean, var = run(dict(d, r=r), gidx)
    base = (d['alpha'] + 1.0 / d['beta'])[:, None, None].expand(-1, 65, len(zero))
    assert torch.equal(mean[:, :, zero], torch.zeros_like(base)) and torch.equal(var[:, :, zero], base)
    # the other columns are what they are with the full r
    mean_f, var_f = run(d, gidx)
    keep = [i for i in range(17) if i not in zero]
    assert torch.equal(mean[:, :, keep], mean_f[:, :, keep]) and torch.equal(var[:, :, keep], var_f[:, :, keep])


@pytest.mark.parametrize('k,g,j,m,q,n', [(2, 2, 17, 33, 10, 65), (3, 1, 1, 50, 10, 100)])
def test_jensen_with_a_real_chain(dev, k, g, j, m, q, n):
    """c = K^-1 - P_g and r = beta P_g Psi1^T y of a sparse GP posterior (P_g = (K + beta Psi2_g)^-1, Psi2_g the statistics of
    the points of pattern g): var - 1/beta = alpha - tr(K^-1 Psi2*) + tr(P Psi2*) + r^T (Psi2* - psi1* psi1*^T) r >= 0, since
    alpha >= tr(K^-1 Psi2*) (Nystrom), P is positive definite and Psi2* - psi1* psi1*^T positive semi-definite (Jensen)."""
    c, _ = case((k, g, j, m, q, n))
    c = dict(c)
    rs = np.random.default_rng(5)
    gidx = torch.as_tensor(rs.integers(0, g, (k, j)), dtype=torch.int32)
    y = torch.as_tensor(rs.standard_normal((n, j)))
    rows = torch.as_tensor(rs.random((g, n)) < 0.7)
    rows[:, 0] = True
    cs, rr = [], []
    for i in range(k):
        dz = c['z'][i][:, None, :] - c['z'][i][None, :, :]
        kmm = c['alpha'][i] * torch.exp(-0.5 * torch.sum(c['gamma'][i] * dz * dz, dim=-1)) + 1e-8 * torch.eye(m, dtype=torch.float64)
        kinv = torch.linalg.inv(kmm)
        ps, rcol = [], torch.zeros((m, j), dtype=torch.float64)
        for gi in range(g):
            sub = {name: (a[rows[gi]] if name in ('mu', 's') else a[i:i + 1]) for name, a in c.items()
                   if name in ('z', 'mu', 's', 'gamma', 'alpha')}
            sub['c'], sub['r'] = torch.zeros((1, 1, m, m), dtype=torch.float64), torch.zeros((1, m, 1), dtype=torch.float64)
            st = restated(sub)
            p = torch.linalg.inv(kmm + c['beta'][i] * st['psi2'][0])
            p = 0.5 * (p + p.T)
            ps.append(kinv - p)
            cols = (gidx[i] == gi)
            rcol[:, cols] = c['beta'][i] * p @ st['psi1'][0].T @ y[rows[gi]][:, cols]
        cs.append(torch.stack(ps))
        rr.append(rcol)
    c['c'], c['r'] = torch.stack(cs), torch.stack(rr)
    want = restated(c)
    mean_w, var_w, top = moments_of(c, want, gidx)
    floor = -1e-12 * top
    gap_w = var_w - (1.0 / c['beta'])[:, None, None]
    print('restated: min (var - 1/beta) = %.3e (bound %.3e)' % (float(gap_w.min()), floor))
    assert float(gap_w.min()) >= floor
    mean, var = run(on(dev, c), gidx)
    close(mean, mean_w.numpy(), 1e-12, 'mean')
    close_var(var, var_w, top, 'var')
    gap = var.cpu() - (1.0 / c['beta'])[:, None, None]
    print('operator: min (var - 1/beta) = %.3e (bound %.3e)' % (float(gap.min()), floor))
    assert float(gap.min()) >= floor, 'var < 1/beta'


def test_argument_checks(dev):
    from dp_gp_lvm_amd import ops
    c, _ = case((2, 3, 17, 33, 10, 65))
    d = on(dev, c)
    args = (d['z'], d['mu'], d['s'], d['gamma'], d['alpha'], d['c'], d['r'])
    gidx = gidx_of('random', 2, 3, 17).to(dev)
    with pytest.raises(TypeError):
        ops.qx_psi_point_moments(*args, gidx.long(), d['beta'])
    with pytest.raises(TypeError):
        ops.qx_psi_point_moments(*args, gidx, d['beta'].float())
    with pytest.raises(ValueError):
        ops.qx_psi_point_moments(*args, gidx[:, :-1].contiguous(), d['beta'])
    with pytest.raises(ValueError):
        ops.qx_psi_point_moments(*args, gidx, d['beta'][:1])
    with pytest.raises(RuntimeError):
        ops.qx_psi_point_moments(*args, gidx.cpu(), d['beta'])
