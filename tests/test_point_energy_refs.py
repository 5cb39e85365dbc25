"""CPU tests (no GPU) of the references that pin ops.ard_rbf_point_energy (csrc/ard_rbf_point_energy.hip): a NumPy restatement in
np.longdouble, checked here against autograd and against test_point_metric_refs.metric_ref, the case table that
tests/test_gpu_point_energy.py runs, and the curve-gradient assembly of models/geodesic.py against autograd.

    d_mq = x_q - z_mq,   k_m = alpha exp(-1/2 sum_q gamma_q d_mq^2),   a_m = sum_q gamma_q d_mq v_q,   c_m = -k_m a_m
    w_m  = sum_m' (p[m,m'] + p[m',m]) c_m'
    e    = sum_{m,m'} p[m,m'] c_m c_m' = 1/2 sum_m w_m c_m
    dx_q = gamma_q sum_m w_m k_m (a_m d_mq - v_q),        dv_q = -gamma_q sum_m w_m k_m d_mq
The denominators are the same sums with every elementary term (gamma d v in a, p c in w, a d and v in dx) replaced by its absolute
value: the sum of the absolute values of the terms of each entry in this difference form."""
import functools

import numpy as np
import torch

from dp_gp_lvm_amd.models import geodesic
from test_point_metric_refs import metric_ref

LD = np.longdouble


def _forms(d, kv, v, gamma, p, absolute):
    """(e, dx, dv) of the formulas above from d [K,N,M,Q], k [K,N,M], v [N,Q], gamma [K,Q], p [K,M,M]; absolute: the
    denominators (every elementary term by its absolute value)."""
    fix = np.abs if absolute else (lambda t: t)
    sgn = 1.0 if absolute else -1.0
    d, v, p = fix(d), fix(v), fix(p)
    g = gamma[:, None, None, :]
    a = np.sum(g * d * v[None, :, None, :], axis=-1)                             # [K, N, M]
    c = sgn * kv * a
    w = np.matmul(c, p + p.transpose(0, 2, 1))                                   # [K, N, M]: sum_m' (p[m,m'] + p[m',m]) c[m'] (symmetric)
    u = w * kv
    e = 0.5 * np.sum(w * c, axis=-1)
    su = np.sum(u, axis=-1)[..., None]
    uad = np.einsum('knm,knmq->knq', u * a, d)
    dx = gamma[:, None, :] * (uad + v[None] * su if absolute else uad - v[None] * su)
    dv = sgn * gamma[:, None, :] * np.einsum('knm,knmq->knq', u, d)
    return e, dx, dv


def energy_ref(z, x, v, gamma, alpha, p):
    """((e [K,N], dx [K,N,Q], dv [K,N,Q]), (their denominators)) in np.longdouble."""
    z, x, v, gamma, alpha, p = (np.asarray(a, dtype=LD) for a in (z, x, v, gamma, alpha, p))
    d = x[None, :, None, :] - z[:, None, :, :]                                   # [K, N, M, Q]
    kv = alpha.reshape(-1)[:, None, None] * np.exp(-0.5 * np.sum(gamma[:, None, None, :] * d * d, axis=-1))
    return _forms(d, kv, v, gamma, p, False), _forms(d, kv, v, gamma, p, True)


# ---- the case table: one sweep per axis around (K, N, M, Q) = (3, 65, 50, 10), the corners, and the edges of the kernel's own
# tiling: 64 rows of p per slab and 64 inducing points per chunk (M = 63 .. 65, 127 .. 129), 16 points per workgroup = one column
# tile (N = 15 | 16 | 17, 33), 16 latent dims per step of the (point, column) sums per thread (Q = 16 | 17, 32 | 33, 49, 64).
BASE = dict(K=3, N=65, M=50, Q=10)


def _cases():
    out = [dict(BASE)]
    out += [dict(BASE, M=m) for m in (1, 3, 16, 17, 63, 64, 65, 127, 128, 129, 200)]
    out += [dict(BASE, Q=q) for q in (1, 2, 7, 16, 17, 21, 32, 33, 49, 64)]
    out += [dict(BASE, N=n) for n in (1, 15, 16, 17, 33, 130)]
    out += [dict(BASE, K=1)]
    out += [dict(K=1, N=1, M=1, Q=1), dict(K=3, N=130, M=200, Q=21)]
    return out


CASES = _cases()


def case_id(c):
    return 'K%d-N%d-M%d-Q%d' % (c['K'], c['N'], c['M'], c['Q'])


@functools.lru_cache(maxsize=None)
def _case(i):
    c = CASES[i]
    k, n, m, q = c['K'], c['N'], c['M'], c['Q']
    rng = np.random.default_rng(7300 + i)
    sc = 1.0 / np.sqrt(q)                                                        # every exponent stays O(1) at every Q
    inp = dict(z=sc * rng.standard_normal((k, m, q)), x=sc * rng.standard_normal((n, q)), v=sc * rng.standard_normal((n, q)),
               gamma=rng.uniform(0.2, 3.0, (k, q)), alpha=rng.uniform(0.5, 2.0, k), p=rng.standard_normal((k, m, m)))
    for a in inp.values():
        a.setflags(write=False)
    (e, dx, dv), (e_den, dx_den, dv_den) = energy_ref(**inp)
    ref = dict(e=e, dx=dx, dv=dv, e_den=e_den, dx_den=dx_den, dv_den=dv_den)
    for a in ref.values():
        a.setflags(write=False)
    return inp, ref


def case(i):
    """(inputs, references) of CASES[i]: read-only arrays, computed once per process.  p is random, indefinite and NOT symmetric."""
    return _case(i)


# ---- the references against autograd ----------------------------------------------------------------------------------------
def _features(x, z, gamma, alpha):
    d = x[None, :] - z
    return -gamma * d * (alpha * torch.exp(-0.5 * torch.sum(gamma * d * d, dim=1)))[:, None]       # b [M, Q]


def _small(seed, k=2, n=3, m=6, q=4):
    rng = np.random.default_rng(seed)
    return dict(z=rng.standard_normal((k, m, q)), x=rng.standard_normal((n, q)), v=rng.standard_normal((n, q)),
                gamma=rng.uniform(0.2, 3.0, (k, q)), alpha=rng.uniform(0.5, 2.0, k), p=rng.standard_normal((k, m, m)))


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want)) / max(1.0, np.max(np.abs(want))))


def test_reference_is_autograd_of_the_quadratic_form():
    for seed, shape in ((1, {}), (2, dict(k=1, n=2, m=9, q=1)), (3, dict(k=3, n=1, m=1, q=5))):
        inp = _small(seed, **shape)
        (e, dx, dv), _ = energy_ref(**inp)
        t = {name: torch.tensor(a) for name, a in inp.items()}
        for k in range(inp['z'].shape[0]):
            for n in range(inp['x'].shape[0]):
                xn, vn = t['x'][n].clone().requires_grad_(True), t['v'][n].clone().requires_grad_(True)
                b = _features(xn, t['z'][k], t['gamma'][k], t['alpha'][k])
                val = vn @ (b.T @ t['p'][k] @ b) @ vn
                gx, gv = torch.autograd.grad(val, (xn, vn))
                assert _rel(e[k, n], val.item()) <= 1e-12
                assert _rel(dx[k, n], gx.numpy()) <= 1e-12 and _rel(dv[k, n], gv.numpy()) <= 1e-12


def test_energy_is_the_metric_reference_along_v():
    for seed in (4, 5):
        inp = _small(seed, k=2, n=5, m=7, q=3)
        (e, _, _), (e_den, _, _) = energy_ref(**inp)
        g, g_den = metric_ref(inp['z'], inp['x'], inp['gamma'], inp['alpha'], inp['p'])
        v = np.asarray(inp['v'], dtype=LD)
        want = np.einsum('nq,knqr,nr->kn', v, g, v)
        assert _rel(e, want) <= 1e-12
        # the denominator is the same expansion: sum |p| |b v| |b v| term by term
        assert _rel(e_den, np.einsum('nq,knqr,nr->kn', np.abs(v), g_den, np.abs(v))) <= 1e-12
        assert np.all(e_den >= np.abs(e))


def test_results_depend_on_the_symmetric_part_of_p_only():
    inp = _small(6)
    p = inp['p']
    assert np.max(np.abs(p - p.transpose(0, 2, 1))) > 0.1                        # NOT symmetric
    a, a_den = energy_ref(**inp)
    b, b_den = energy_ref(**dict(inp, p=np.ascontiguousarray(p.transpose(0, 2, 1))))
    for one, two, den in zip(a + a_den, b + b_den, a_den + a_den):
        assert np.max(np.abs(one - two) / den) <= 1e-17
    pl = np.asarray(p, dtype=LD)                                                 # (halves and doubles are exact: the same p + p^T)
    c, _ = energy_ref(**dict(inp, p=0.5 * (pl + pl.transpose(0, 2, 1))))
    for one, two, den in zip(a, c, a_den):
        assert np.max(np.abs(one - two) / den) <= 1e-17


def test_curve_gradient_assembly_is_autograd_of_the_energy():
    """E = S sum_i v_i^T G(x_i) v_i with G = sum_k (b_k^T p_k b_k + prior_k diag(gamma_k)) restated in torch, against
    geodesic.gradient on the reference's (dx, dv) plus the prior's share; C = 2 curves, S = 4 and S = 1."""
    for seed, s in ((7, 4), (8, 1)):
        rng = np.random.default_rng(seed)
        k, m, q, c = 2, 5, 3, 2
        z, gamma, alpha = rng.standard_normal((k, m, q)), rng.uniform(0.2, 3.0, (k, q)), rng.uniform(0.5, 2.0, k)
        p, prior = rng.standard_normal((k, m, m)), rng.uniform(0.5, 2.0, k)
        curve = torch.tensor(rng.standard_normal((c, s + 1, q)))
        x, v = geodesic.segments(curve)
        assert tuple(x.shape) == (c * s, q) and torch.equal(x[0], 0.5 * (curve[0, 0] + curve[0, 1]))
        assert torch.equal(v[s - 1], curve[0, s] - curve[0, s - 1])
        (e, dx, dv), _ = energy_ref(z, x.numpy(), v.numpy(), gamma, alpha, p)
        w = torch.tensor((prior[:, None] * alpha[:, None] * gamma).sum(0))          # [Q]
        pe, pdx, pdv = geodesic.prior_terms(v, w)
        e_t = torch.tensor(np.asarray(e.sum(0), dtype=np.float64)) + pe
        dx_t = torch.tensor(np.asarray(dx.sum(0), dtype=np.float64)) + pdx
        dv_t = torch.tensor(np.asarray(dv.sum(0), dtype=np.float64)) + pdv
        have_e, have_g = geodesic.energy(e_t, c), geodesic.gradient(dx_t, dv_t, c)

        cv = curve.clone().requires_grad_(True)
        total = []
        for ci in range(c):
            acc = 0.0
            for i in range(s):
                xi, vi = 0.5 * (cv[ci, i] + cv[ci, i + 1]), cv[ci, i + 1] - cv[ci, i]
                for kk in range(k):
                    b = _features(xi, torch.tensor(z[kk]), torch.tensor(gamma[kk]), float(alpha[kk]))
                    g = b.T @ torch.tensor(p[kk]) @ b + prior[kk] * alpha[kk] * torch.diag(torch.tensor(gamma[kk]))
                    acc = acc + vi @ g @ vi
            total.append(s * acc)
        want_e = torch.stack(total)
        (want_g,) = torch.autograd.grad(want_e.sum(), cv)
        assert tuple(have_g.shape) == (c, s + 1, q)
        assert _rel(have_e.numpy(), want_e.detach().numpy()) <= 1e-10
        assert _rel(have_g.numpy(), want_g.numpy()) <= 1e-10
        assert float(want_g.abs().max()) > 1e-3
        ln = geodesic.length(e_t.clamp(min=0), c)
        assert torch.all(ln * ln <= geodesic.energy(e_t.clamp(min=0), c) * (1 + 1e-12))


def test_straight_line_keeps_the_end_points_bits():
    rng = np.random.default_rng(9)
    a, b = torch.tensor(rng.standard_normal((3, 4))), torch.tensor(rng.standard_normal((3, 4)))
    for s in (1, 5, 32):
        c = geodesic.straight_line(a, b, s)
        assert tuple(c.shape) == (3, s + 1, 4) and torch.equal(c[:, 0], a) and torch.equal(c[:, -1], b)
        assert float((c[:, 1:] - c[:, :-1] - (b - a)[:, None] / s).abs().max()) <= 1e-15


def test_case_table_is_finite_and_alive_in_every_case():
    need = dict(M={1, 3, 16, 17, 50, 63, 64, 65, 127, 128, 129, 200}, Q={1, 2, 7, 10, 16, 17, 21, 32, 33, 49, 64},
                N={1, 15, 16, 17, 33, 65, 130}, K={1, 3})
    for axis, values in need.items():
        assert values <= {c[axis] for c in CASES}, axis
    assert dict(K=1, N=1, M=1, Q=1) in CASES and dict(K=3, N=130, M=200, Q=21) in CASES
    for i in range(len(CASES)):
        inp, ref = case(i)
        assert np.max(np.abs(inp['p'] - inp['p'].transpose(0, 2, 1))) > 0 or CASES[i]['M'] == 1
        for name, a in ref.items():
            assert np.all(np.isfinite(a)), (case_id(CASES[i]), name)
        for name in ('e', 'dx', 'dv'):
            assert float(np.max(np.abs(ref[name]))) > 1e-6, (case_id(CASES[i]), name)
            assert np.all(ref[name + '_den'] >= np.abs(ref[name]) * (1 - 1e-15))
