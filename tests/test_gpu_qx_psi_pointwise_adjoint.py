"""GPU tests of the latent adjoint of the per-point contractions (dpgp_qx_psi_pointwise_adjoint_f64, csrc/qx_psi_point_adjoint.hip)
and of the moments' VJP on top of it (ops.qx_psi_point_moments_adjoint).  References and the case table:
test_pointwise_adjoint_refs.py (torch autograd through the CPU restatement of the forward operator, checked there against the closed
form and central differences).  Tolerances: 1e-8 for an adjoint operator against autograd, 1e-10 operator to
operator (the slot composition through ops.psi_latent_adjoint, zfac given against zfac=None); `close` takes them relative to
max(1, max |reference|).  Two calls must give the same bits, zero adjoints exact zeros."""
import numpy as np
import pytest
import torch

from test_gpu_predict_b1 import close
from test_gpu_qx_psi_point_moments import GIDX, gidx_of, moments_of
from test_gpu_qx_psi_pointwise import on, pair_factor, restated
from test_pointwise_adjoint_refs import CASES, adjoint_case, reference

pytestmark = pytest.mark.gpu


def run(d, adj, zfac=None):
    from dp_gp_lvm_amd import ops
    return ops.qx_psi_pointwise_adjoint(d['z'], d['mu'], d['s'], d['gamma'], d['alpha'], d['c'], d['r'], *adj, zfac=zfac)


def report(tag, have, want):
    for name, hv, wv in zip(('d_mu', 'd_s'), have, want):
        print('%s %s: max |err| %.3e of %.3e' % (tag, name, float((hv.cpu() - wv.cpu()).abs().max()), float(wv.abs().max())))


def check(tag, have, want, tol):
    report(tag, have, want)
    for name, hv, wv in zip(('d_mu', 'd_s'), have, want):
        assert bool(torch.isfinite(hv).all()), tag + ' ' + name
        close(hv, wv.cpu().numpy(), tol, tag + ' ' + name)


def slot_composition(d, adj, k):
    """Kernel k through ops.psi_latent_adjoint: J + G slots that replicate its (gamma, alpha) on its z."""
    from dp_gp_lvm_amd import ops
    h, gq, gt = (a[k] for a in adj)                                                    # [N,J], [N,J], [N,G]
    r, c = d['r'][k], d['c'][k]                                                        # [M,J], [G,M,M]
    j, g, n = r.shape[1], c.shape[0], h.shape[0]
    rt = r.transpose(0, 1).contiguous()                                                # [J,M]
    g_psi2 = torch.cat([rt[:, :, None] * rt[:, None, :], c]).contiguous()
    g_v = torch.cat([rt, torch.zeros((g, r.shape[0]), dtype=torch.float64, device=r.device)]).contiguous()
    y = torch.cat([h, torch.zeros((n, g), dtype=torch.float64, device=r.device)], dim=1).contiguous()
    w = torch.cat([gq, gt], dim=1).transpose(0, 1).contiguous()
    return ops.psi_latent_adjoint(d['z'][k], d['mu'], d['s'], d['gamma'][k][None].expand(j + g, -1).contiguous(),
                                  d['alpha'][k].expand(j + g).contiguous(), y, g_v, g_psi2, weights=w)


@pytest.mark.parametrize('k,g,j,m,q,n', CASES)
def test_adjoint_operator(dev, k, g, j, m, q, n):
    c, adj, want = reference((k, g, j, m, q, n))
    d, a = on(dev, c), tuple(x.to(dev) for x in adj)
    have = run(d, a)
    assert tuple(have[0].shape) == (n, q) and tuple(have[1].shape) == (n, q)
    check('autograd', have, want, 1e-8)
    again = run(d, a)
    assert torch.equal(have[0], again[0]) and torch.equal(have[1], again[1]), 'two calls differ'
    check('zfac given', run(d, a, zfac=pair_factor(d)), have, 1e-10)
    total = [torch.zeros_like(have[0]), torch.zeros_like(have[1])]
    for kk in range(k):
        one = {name: (v[kk:kk + 1].contiguous() if name in ('z', 'gamma', 'alpha', 'c', 'r') else v) for name, v in d.items()}
        own = run(one, tuple(x[kk:kk + 1].contiguous() for x in a))
        comp = slot_composition(d, a, kk)
        check('kernel %d against the slot composition' % kk, own, comp, 1e-10)
        total = [total[0] + comp[0], total[1] + comp[1]]
    check('sum of the slot compositions', have, total, 1e-10)


def test_zero_adjoints(dev):
    """Points 64..127 (a whole workgroup: its waves skip) and 130..193 (waves that hold other points too) have h = gq = gt = 0:
    exactly 0.0 rows; the other rows agree with autograd.  All-zero adjoints: all-zero outputs."""
    shape = (2, 3, 17, 33, 10, 200)
    c, adj, want = reference(shape, 'block')
    d, a = on(dev, c), tuple(x.to(dev) for x in adj)
    have = run(d, a)
    check('block', have, want, 1e-8)
    for out in have:
        assert float(out[64:128].abs().max()) == 0.0 and float(out[130:194].abs().max()) == 0.0
        assert float(out[:64].abs().min()) > 0.0
    none = run(d, tuple(torch.zeros_like(x) for x in a))
    assert float(none[0].abs().max()) == 0.0 and float(none[1].abs().max()) == 0.0


def test_row_with_zero_variance(dev):
    c, adj, want = reference(CASES[1], 's0')
    assert float(c['s'][1].abs().max()) == 0.0
    check('s = 0 row', run(on(dev, c), tuple(x.to(dev) for x in adj)), want, 1e-8)


@pytest.mark.filterwarnings('ignore:Converting a tensor with requires_grad')       # (moments_of prints its largest term)
@pytest.mark.parametrize('kind', GIDX)
def test_moments_adjoint(dev, kind):
    """ops.qx_psi_point_moments_adjoint against autograd of the restated moments, gidx inside [0, G), all G - 1, and with -1 / G."""
    from dp_gp_lvm_amd import ops
    shape = CASES[1]
    k, g, j, m, q, n = shape
    c, _ = adjoint_case(shape)
    c['beta'] = torch.as_tensor(np.random.default_rng(3).uniform(0.5, 20.0, k))
    gidx = gidx_of(kind, k, g, j)
    rs = np.random.default_rng(11)
    g_mean, g_var = torch.as_tensor(rs.standard_normal((k, n, j))), torch.as_tensor(rs.standard_normal((k, n, j)))
    mu, s = c['mu'].clone().requires_grad_(True), c['s'].clone().requires_grad_(True)
    cc = dict(c, mu=mu, s=s)
    mean, var, _ = moments_of(cc, restated(cc), gidx)
    want = torch.autograd.grad(torch.sum(g_mean * mean) + torch.sum(g_var * var), (mu, s))
    d = on(dev, c)
    mean_d, _ = ops.qx_psi_point_moments(d['z'], d['mu'], d['s'], d['gamma'], d['alpha'], d['c'], d['r'], gidx.to(dev), d['beta'])
    have = ops.qx_psi_point_moments_adjoint(d['z'], d['mu'], d['s'], d['gamma'], d['alpha'], d['c'], d['r'], gidx.to(dev), d['beta'],
                                            mean_d, g_mean.to(dev), g_var.to(dev))
    check(kind, have, want, 1e-8)


def test_argument_checks(dev):
    c, adj = adjoint_case((2, 3, 4, 5, 2, 7))
    d, (h, gq, gt) = on(dev, c), tuple(x.to(dev) for x in adj)
    with pytest.raises(TypeError):
        run(d, (h.float(), gq, gt))
    with pytest.raises(TypeError):
        run(d, (h, gq, gt.cpu().numpy()))
    with pytest.raises(RuntimeError):
        run(d, (h, gq.cpu(), gt))
    with pytest.raises(ValueError):
        run(d, (h[:, :-1].contiguous(), gq, gt))
    with pytest.raises(ValueError):
        run(d, (h, gq, gt[:, :, :-1].contiguous()))
    with pytest.raises(ValueError):
        run(dict(d, c=d['c'][:1].contiguous()), (h, gq, gt))
