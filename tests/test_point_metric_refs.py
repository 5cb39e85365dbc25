"""CPU tests (no GPU) of the references that pin ops.ard_rbf_point_metric / ops.ard_rbf_point_jacobian (csrc/ard_rbf_point_metric.hip):
NumPy restatements in np.longdouble, checked here against autograd, and the case table that tests/test_gpu_point_metric.py runs.

    k_m(x)  = alpha exp(-1/2 sum_q gamma_q (x_q - z_mq)^2)
    b_mq(x) = d k_m / d x_q = -gamma_q (x_q - z_mq) k_m(x)
    metric_ref:    g[k,n,q,q']  = sum_{m,m'} p[k,m,m'] b_kmq(x_n) b_km'q'(x_n)
    jacobian_ref:  jac[k,n,j,q] = sum_m b_kmq(x_n) r[k,m,j]
Both also return the sum of the absolute values of each entry's terms, the denominator of the GPU file's tolerance."""
import functools

import numpy as np
import torch

LD = np.longdouble


def features_ref(z, x, gamma, alpha):
    """b [K, N, M, Q] in np.longdouble."""
    z, x, gamma, alpha = (np.asarray(a, dtype=LD) for a in (z, x, gamma, alpha))
    d = x[None, :, None, :] - z[:, None, :, :]                                   # [K, N, M, Q]
    kv = alpha.reshape(-1)[:, None, None] * np.exp(-0.5 * np.sum(gamma[:, None, None, :] * d * d, axis=-1))
    return -gamma[:, None, None, :] * d * kv[..., None]


def _quad(b, p):
    k, n, m, q = b.shape
    out = np.empty((k, n, q, q), dtype=b.dtype)
    for kk in range(k):
        bm = np.ascontiguousarray(b[kk].transpose(1, 0, 2)).reshape(m, n * q)    # [M, (n, q')]
        u = np.matmul(p[kk], bm).reshape(m, n, q)                                # U[m, n, q'] = sum_m' p[m,m'] b[n,m',q']
        out[kk] = np.einsum('nmq,mnr->nqr', b[kk], u)
    return out


def metric_ref(z, x, gamma, alpha, p):
    """(g, den) [K, N, Q, Q] in np.longdouble; den the same sum over the absolute values of the terms."""
    b, p = features_ref(z, x, gamma, alpha), np.asarray(p, dtype=LD)
    den = _quad(np.abs(b).astype(np.float64), np.abs(p).astype(np.float64))       # (a denominator: fp64 is plenty, and quick)
    return _quad(b, p), den.astype(LD)


def jacobian_ref(z, x, gamma, alpha, r):
    """(jac, den) [K, N, J, Q] in np.longdouble."""
    b, r = features_ref(z, x, gamma, alpha), np.asarray(r, dtype=LD)
    return np.einsum('knmq,kmj->knjq', b, r), np.einsum('knmq,kmj->knjq', np.abs(b), np.abs(r))


# ---- the case table: one sweep per axis around (K, N, M, Q) = (3, 65, 50, 10), the corners, and the edges of the kernel's own
# tiling: 64 rows of p (or columns of r) per slab and 64 inducing points per chunk (M, J = 63 .. 65, 127 .. 129), 16 latent
# dims per column tile (Q = 16 | 17, 32 | 33, 48 | 49, 64), 8 / 2 / 1 / 1 points per workgroup for Q <= 16 / 32 / 48 / 64.
BASE = dict(K=3, N=65, M=50, Q=10, J=5)


def _cases():
    out = [dict(BASE)]
    out += [dict(BASE, M=m) for m in (1, 3, 16, 17, 63, 64, 65, 127, 128, 129, 200)]
    out += [dict(BASE, Q=q) for q in (1, 2, 7, 16, 17, 21)]
    out += [dict(BASE, N=n) for n in (1, 7, 8, 9, 63, 64, 130)]
    out += [dict(BASE, K=1)]
    out += [dict(BASE, J=j) for j in (1, 15, 16, 17, 60, 63, 64, 65, 129)]
    out += [dict(K=1, N=1, M=1, Q=1, J=1), dict(K=3, N=130, M=200, Q=21, J=60)]
    out += [dict(K=2, N=3, M=70, Q=17, J=3), dict(K=2, N=4, M=70, Q=32, J=17), dict(K=1, N=3, M=65, Q=33, J=2),
            dict(K=1, N=2, M=40, Q=49, J=2), dict(K=1, N=3, M=130, Q=64, J=70)]
    return out


CASES = _cases()


def case_id(c):
    return 'K%d-N%d-M%d-Q%d-J%d' % (c['K'], c['N'], c['M'], c['Q'], c['J'])


@functools.lru_cache(maxsize=None)
def _case(i):
    c = CASES[i]
    k, n, m, q, j = c['K'], c['N'], c['M'], c['Q'], c['J']
    rng = np.random.default_rng(7100 + i)
    inp = dict(z=rng.standard_normal((k, m, q)), x=rng.standard_normal((n, q)), gamma=rng.uniform(0.2, 3.0, (k, q)),
               alpha=rng.uniform(0.5, 2.0, k), p=rng.standard_normal((k, m, m)), r=rng.standard_normal((k, m, j)))
    for a in inp.values():
        a.setflags(write=False)
    g, g_den = metric_ref(inp['z'], inp['x'], inp['gamma'], inp['alpha'], inp['p'])
    jac, jac_den = jacobian_ref(inp['z'], inp['x'], inp['gamma'], inp['alpha'], inp['r'])
    ref = dict(g=g, g_den=g_den, jac=jac, jac_den=jac_den)
    for a in ref.values():
        a.setflags(write=False)
    return inp, ref


def case(i):
    """(inputs, references) of CASES[i]: read-only arrays, computed once per process.  p is random, indefinite and NOT symmetric."""
    return _case(i)


# ---- the references against autograd ----------------------------------------------------------------------------------------
def _kxu(x, z, gamma, alpha):
    d = x[None, :] - z
    return alpha * torch.exp(-0.5 * torch.sum(gamma * d * d, dim=1))             # [M]


def _small(seed, m=6, q=4):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((1, m, q)), rng.standard_normal((3, q)), rng.uniform(0.2, 3.0, (1, q)), rng.uniform(0.5, 2.0, 1))


def test_features_are_the_autograd_jacobian_of_kxu():
    z, x, gamma, alpha = _small(1)
    m = z.shape[1]
    jac, den = jacobian_ref(z, x, gamma, alpha, np.eye(m)[None])                # r = I: jac[0, n, m, q] = b_mq(x_n)
    tz, tg, ta = torch.tensor(z[0]), torch.tensor(gamma[0]), torch.tensor(alpha[0])
    for n in range(x.shape[0]):
        auto = torch.autograd.functional.jacobian(lambda v: _kxu(v, tz, tg, ta), torch.tensor(x[n])).numpy()     # [M, Q]
        got = np.asarray(jac[0, n], dtype=np.float64)
        assert np.max(np.abs(got - auto)) <= 1e-12 * max(1.0, np.max(np.abs(auto)))
        assert np.allclose(np.asarray(den[0, n], dtype=np.float64), np.abs(auto), rtol=1e-12, atol=0)


def test_jacobian_covariance_is_the_mixed_second_derivative_of_the_posterior_kernel():
    z, x, gamma, alpha = _small(2)
    m, q = z.shape[1:]
    rng = np.random.default_rng(3)
    a = rng.standard_normal((m, m))
    c = a @ a.T / m                                                             # a symmetric C, as K_uu^-1 - (K_uu + beta Psi2)^-1 is
    tz, tg, ta, tc = torch.tensor(z[0]), torch.tensor(gamma[0]), torch.tensor(alpha[0]), torch.tensor(c)

    def post(u, v):                                                             # c(x, x') = k(x, x') - k_xu C k_ux'
        d = u - v
        return ta * torch.exp(-0.5 * torch.sum(tg * d * d)) - _kxu(u, tz, tg, ta) @ tc @ _kxu(v, tz, tg, ta)

    quad, _ = metric_ref(z, x, gamma, alpha, c[None])
    for n in range(x.shape[0]):
        xn = torch.tensor(x[n])
        inner = lambda u: torch.autograd.functional.jacobian(lambda v: post(u, v), xn.clone(), create_graph=True)
        auto = torch.autograd.functional.jacobian(inner, xn).numpy().T           # [q (of x), q' (of x')]
        want = alpha[0] * np.diag(gamma[0]) - np.asarray(quad[0, n], dtype=np.float64)
        assert np.max(np.abs(auto - want)) <= 1e-10 * max(1.0, np.max(np.abs(want)))


def test_references_do_not_symmetrise_p():
    z, x, gamma, alpha = _small(4)
    m = z.shape[1]
    p = np.random.default_rng(5).standard_normal((1, m, m))
    g, _ = metric_ref(z, x, gamma, alpha, p)
    gt, _ = metric_ref(z, x, gamma, alpha, p.transpose(0, 2, 1))
    assert np.max(np.abs(g - gt.transpose(0, 1, 3, 2))) <= 1e-15 * np.max(np.abs(g))
    assert np.max(np.abs(g - g.transpose(0, 1, 3, 2))) > 1e-3 * np.max(np.abs(g))


def test_case_table_is_finite_and_not_vacuous():
    need = dict(M={1, 3, 16, 17, 50, 64, 65, 128, 129, 200}, Q={1, 2, 7, 10, 16, 17, 21}, N={1, 63, 64, 65, 130}, K={1, 3},
                J={1, 15, 16, 17, 60})
    for axis, values in need.items():
        assert values <= {c[axis] for c in CASES}, axis
    alive = 0
    for i in range(len(CASES)):
        _, ref = case(i)
        for a in ref.values():
            assert np.all(np.isfinite(a)), case_id(CASES[i])
        alive += float(np.max(np.abs(ref['g']))) > 1e-6
    assert alive >= 0.9 * len(CASES), (alive, len(CASES))
