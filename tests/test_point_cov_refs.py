"""CPU tests (no GPU) of the reference that pins ops.ard_rbf_point_cov (csrc/ard_rbf_point_cov.hip): a NumPy restatement in
np.longdouble, checked here against a naive loop over (i, j, m, m'), and the case table that tests/test_gpu_point_cov.py runs.

    k_m(x) = alpha exp(-1/2 sum_q gamma_q (x_q - z_mq)^2),        ct = (c + c^T) / 2
    out[i, j] = alpha exp(-1/2 sum_q gamma_q (x_iq - x_jq)^2) - sum_{m,m'} k_m(x_i) ct[m, m'] k_m'(x_j)
The denominator of an entry is the sum of the absolute values of its terms, |prior term| + sum_{m,m'} |k_m(x_i) ct[m, m'] k_m'(x_j)|."""
import functools

import numpy as np

LD = np.longdouble

# (K, G, N, M, Q): the smallest shapes at which the operator's tiling can go wrong: tiles of 32 points walked in pairs J <= I
# (N = 63 | 64 | 65, 129 | 130: a last tile of 1 or 2 points), blocks of 64 inducing points walked in pairs (M = 63 | 64 | 65, 129, 200;
# M = 1 and 3), several patterns and kernels, Q = 1, 64 and odd values
SHAPES = [(1, 1, 1, 1, 1), (1, 1, 64, 64, 16), (1, 1, 65, 65, 17), (2, 3, 63, 129, 10), (1, 2, 129, 63, 33), (1, 1, 5, 3, 64),
          (1, 1, 130, 1, 10), (3, 2, 130, 200, 21)]
CASES = [dict(K=k, G=g, N=n, M=m, Q=q) for k, g, n, m, q in SHAPES]


def case_id(c):
    return 'K%d-G%d-N%d-M%d-Q%d' % (c['K'], c['G'], c['N'], c['M'], c['Q'])


def features(z, x, gamma, alpha):
    """k [K, N, M] in np.longdouble."""
    d = x[None, :, None, :] - z[:, None, :, :]
    return alpha.reshape(-1)[:, None, None] * np.exp(-0.5 * np.sum(gamma[:, None, None, :] * d * d, axis=-1))


def prior_ref(x, gamma, alpha):
    """alpha_k exp(-1/2 sum_q gamma_kq (x_iq - x_jq)^2) [K, N, N] in np.longdouble (exactly symmetric: d^2 = (-d)^2)."""
    x, gamma, alpha = (np.asarray(a, dtype=LD) for a in (x, gamma, alpha))
    d = x[:, None, :] - x[None, :, :]
    return alpha.reshape(-1)[:, None, None] * np.exp(-0.5 * np.sum(gamma[:, None, None, :] * (d * d)[None], axis=-1))


def cov_ref(z, x, gamma, alpha, c):
    """(out [K, G, N, N], its denominators) in np.longdouble.  The quadratic form is taken as (q + q^T) / 2, so that the reference
    is exactly symmetric as the formula is."""
    z, x, gamma, alpha, c = (np.asarray(a, dtype=LD) for a in (z, x, gamma, alpha, c))
    kv = features(z, x, gamma, alpha)                                            # [K, N, M]
    ct = 0.5 * (c + c.transpose(0, 1, 3, 2))                                     # [K, G, M, M]
    prior = prior_ref(x, gamma, alpha)[:, None]
    q = np.matmul(np.matmul(kv[:, None], ct), kv[:, None].transpose(0, 1, 3, 2))
    qa = np.matmul(np.matmul(kv[:, None], np.abs(ct)), kv[:, None].transpose(0, 1, 3, 2))
    q, qa = 0.5 * (q + q.transpose(0, 1, 3, 2)), 0.5 * (qa + qa.transpose(0, 1, 3, 2))
    return prior - q, np.abs(prior) + qa


@functools.lru_cache(maxsize=None)
def _case(i):
    c = CASES[i]
    k, g, n, m, q = c['K'], c['G'], c['N'], c['M'], c['Q']
    rng = np.random.default_rng(7400 + i)
    sc = 1.0 / np.sqrt(q)                                                        # every exponent stays O(1) at every Q
    inp = dict(z=sc * rng.standard_normal((k, m, q)), x=sc * rng.standard_normal((n, q)), gamma=rng.uniform(0.2, 3.0, (k, q)),
               alpha=rng.uniform(0.5, 2.0, k), c=rng.standard_normal((k, g, m, m)))
    for a in inp.values():
        a.setflags(write=False)
    out, den = cov_ref(**inp)
    ref = dict(out=out, den=den)
    for a in ref.values():
        a.setflags(write=False)
    return inp, ref


def case(i):
    """(inputs, references) of CASES[i]: read-only arrays, computed once per process.  c is random, indefinite and NOT symmetric."""
    return _case(i)


def _naive(inp):
    z, x, gamma, alpha, c = (np.asarray(inp[n], dtype=LD) for n in ('z', 'x', 'gamma', 'alpha', 'c'))
    (kk, m, q), n, g = z.shape, x.shape[0], c.shape[1]
    out, den = np.zeros((kk, g, n, n), dtype=LD), np.zeros((kk, g, n, n), dtype=LD)
    for k in range(kk):
        feat = [[alpha[k] * np.exp(-0.5 * sum(gamma[k, a] * (x[i, a] - z[k, b, a]) ** 2 for a in range(q))) for b in range(m)]
                for i in range(n)]
        for gi in range(g):
            for i in range(n):
                for j in range(n):
                    pr = alpha[k] * np.exp(-0.5 * sum(gamma[k, a] * (x[i, a] - x[j, a]) ** 2 for a in range(q)))
                    s, sa = LD(0), LD(0)
                    for a in range(m):
                        for b in range(m):
                            term = feat[i][a] * (0.5 * (c[k, gi, a, b] + c[k, gi, b, a])) * feat[j][b]
                            s, sa = s + term, sa + abs(term)
                    out[k, gi, i, j], den[k, gi, i, j] = pr - s, abs(pr) + sa
    return out, den


def test_reference_is_the_naive_loop_on_the_two_smallest_cases():
    small = sorted(range(len(CASES)), key=lambda i: int(np.prod(SHAPES[i])))[:2]
    assert [SHAPES[i] for i in small] == [(1, 1, 1, 1, 1), (1, 1, 5, 3, 64)]
    for i in small:
        inp, ref = case(i)
        out, den = _naive(inp)
        assert np.max(np.abs(out - ref['out']) / den) <= 1e-17
        assert np.max(np.abs(den - ref['den']) / den) <= 1e-17


def test_reference_is_exactly_symmetric():
    for i in range(len(CASES)):
        _, ref = case(i)
        for a in ref.values():
            assert np.array_equal(a, a.transpose(0, 1, 3, 2)), case_id(CASES[i])


def test_reference_depends_on_the_symmetric_part_of_c_only():
    inp, ref = case(3)
    c = np.asarray(inp['c'])
    assert np.max(np.abs(c - c.transpose(0, 1, 3, 2))) > 0.1                     # NOT symmetric
    out, _ = cov_ref(**dict(inp, c=np.ascontiguousarray(c.transpose(0, 1, 3, 2))))
    assert np.max(np.abs(out - ref['out']) / ref['den']) <= 1e-17


def test_diagonal_is_alpha_minus_the_quadratic_form():
    inp, ref = case(3)
    z, x, gamma, alpha, c = (np.asarray(inp[n], dtype=LD) for n in ('z', 'x', 'gamma', 'alpha', 'c'))
    kv = features(z, x, gamma, alpha)
    quad = np.einsum('knm,kgmp,knp->kgn', kv, c, kv)                             # c as given: the antisymmetric part drops out
    diag = np.diagonal(ref['out'], axis1=2, axis2=3)
    assert np.max(np.abs(diag - (alpha[:, None, None] - quad)) / np.diagonal(ref['den'], axis1=2, axis2=3)) <= 1e-16


def test_case_table_is_the_stated_one_finite_and_alive():
    assert SHAPES == [(1, 1, 1, 1, 1), (1, 1, 64, 64, 16), (1, 1, 65, 65, 17), (2, 3, 63, 129, 10), (1, 2, 129, 63, 33),
                      (1, 1, 5, 3, 64), (1, 1, 130, 1, 10), (3, 2, 130, 200, 21)]
    for i in range(len(CASES)):
        inp, ref = case(i)
        c = np.asarray(inp['c'])
        assert np.max(np.abs(c - c.transpose(0, 1, 3, 2))) > 0 or CASES[i]['M'] == 1
        assert tuple(ref['out'].shape) == (CASES[i]['K'], CASES[i]['G'], CASES[i]['N'], CASES[i]['N'])
        for a in ref.values():
            assert np.all(np.isfinite(a)), case_id(CASES[i])
        assert float(np.max(np.abs(ref['out']))) > 1e-6
        assert np.all(ref['den'] >= np.abs(ref['out']) * (1 - 1e-15)) and np.all(ref['den'] > 0)
        if CASES[i]['M'] > 1:                                                     # the quadratic form is not negligible: it is tested
            assert float(np.max(ref['den'] - np.abs(prior_ref(inp['x'], inp['gamma'], inp['alpha'])[:, None]))) > 1e-2
