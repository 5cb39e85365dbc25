"""CPU tests (no GPU) of the references that pin ops.ard_rbf_point_christoffel / ops.geodesic_accel
(csrc/ard_rbf_point_metric.hip, csrc/geodesic_accel.hip) and latent_exp_map (models/geodesic.exp_map): NumPy restatements in np.longdouble, a NumPy RK4
restatement of the integrator, the case tables that tests/test_gpu_point_christoffel.py and tests/test_gpu_latent_exp_map.py run,
and checks of the references themselves.

    k_m(x)    = alpha exp(-1/2 sum_q gamma_q (x_q - z_mq)^2),   b_mq(x) = d k_m / d x_q = -gamma_q (x_q - z_mq) k_m(x)
    d_m(x, v) = v^T (d^2 k_m / dx dx) v = k_m(x) [ (sum_q gamma_q (x_q - z_mq) v_q)^2 - sum_q gamma_q v_q^2 ]
    christoffel_ref:  g[k,n,q,q'] = sum_{m,m'} p[k,m,m'] b_kmq(x_n) b_km'q'(x_n),   gam[k,n,q] = sum_{m,m'} b_kmq(x_n) p[k,m,m'] d_km'(x_n, v_n)
    accel_ref:        G_n = sum_k g[k,n] + diag(prior),  speed_n = v_n^T G_n v_n,  a_n = -G_n^-1 sum_k gam[k,n]   (Cholesky, lower triangle)
Every reference also returns the sum of the absolute values of each entry's terms, the denominator of the GPU file's tolerance."""
import functools

import numpy as np

from test_point_metric_refs import features_ref, metric_ref

LD = np.longdouble


def second_ref(z, x, v, gamma, alpha):
    """(d, |terms| of d) [K, N, M] in np.longdouble."""
    z, x, v, gamma, alpha = (np.asarray(a, dtype=LD) for a in (z, x, v, gamma, alpha))
    diff = x[None, :, None, :] - z[:, None, :, :]                                # [K, N, M, Q]
    kv = alpha.reshape(-1)[:, None, None] * np.exp(-0.5 * np.sum(gamma[:, None, None, :] * diff * diff, axis=-1))
    t = gamma[:, None, None, :] * diff * v[None, :, None, :]
    s2 = np.sum(gamma[:, None, :] * v[None] * v[None], axis=-1)[:, :, None]      # [K, N, 1]
    return kv * (np.sum(t, axis=-1) ** 2 - s2), kv * (np.sum(np.abs(t), axis=-1) ** 2 + s2)


def christoffel_ref(z, x, v, gamma, alpha, p):
    """(g, g_den [K, N, Q, Q], gam, gam_den [K, N, Q]) in np.longdouble."""
    b, p = features_ref(z, x, gamma, alpha), np.asarray(p, dtype=LD)
    d, d_abs = second_ref(z, x, v, gamma, alpha)
    g, g_den = metric_ref(z, x, gamma, alpha, p)
    gam = np.einsum('knmq,kmj,knj->knq', b, p, d)
    gam_den = np.einsum('knmq,kmj,knj->knq', *(np.asarray(a, dtype=np.float64) for a in (np.abs(b), np.abs(p), d_abs)))
    return g, g_den, gam, gam_den.astype(LD)


def cholesky_ref(a):
    """(L, info) of one matrix in its own dtype, reading the lower triangle; info: 0 or the 1-based failing pivot."""
    a = np.array(a)
    q = a.shape[0]
    for j in range(q):
        if not a[j, j] > 0:
            return a, j + 1
        a[j, j] = np.sqrt(a[j, j])
        a[j + 1:, j] /= a[j, j]
        for c in range(j + 1, q):
            a[c:, c] -= a[c:, j] * a[c, j]
    return np.tril(a), 0


def accel_ref(g, gam, prior, v, dtype=LD):
    """(a [N, Q], speed [N], info [N], G [N, Q, Q]) in `dtype`."""
    g, gam, prior, v = (np.asarray(t, dtype=dtype) for t in (g, gam, prior, v))
    big = np.sum(g, axis=0) + np.diag(prior)[None]
    rhs = -np.sum(gam, axis=0)
    n, q = rhs.shape
    a, info = np.full((n, q), np.nan, dtype=dtype), np.zeros(n, dtype=np.int32)
    for i in range(n):
        l, info[i] = cholesky_ref(big[i])
        if info[i]:
            continue
        y = np.zeros(q, dtype=dtype)
        for j in range(q):
            y[j] = (rhs[i, j] - l[j, :j] @ y[:j]) / l[j, j]
        for j in range(q - 1, -1, -1):
            a[i, j] = (y[j] - l[j + 1:, j] @ a[i, j + 1:]) / l[j, j]
    return a, np.einsum('nq,nqr,nr->n', v, big, v), info, big


def rk4_ref(accel, x, v, num_steps):
    """(curve, velocities) [C, S+1, Q]: the NumPy restatement of models/geodesic.exp_map; accel: (x, v) [C, Q] -> a [C, Q]."""
    x, v = np.array(x, dtype=np.float64), np.array(v, dtype=np.float64)
    h = 1.0 / num_steps
    xs, vs = [x], [v]
    for _ in range(num_steps):
        k1x, k1v = v, accel(x, v)
        k2x = v + 0.5 * h * k1v
        k2v = accel(x + 0.5 * h * k1x, k2x)
        k3x = v + 0.5 * h * k2v
        k3v = accel(x + 0.5 * h * k2x, k3x)
        k4x = v + h * k3v
        k4v = accel(x + h * k3x, k4x)
        x = x + (h / 6.0) * (k1x + 2.0 * k2x + 2.0 * k3x + k4x)
        v = v + (h / 6.0) * (k1v + 2.0 * k2v + 2.0 * k3v + k4v)
        xs.append(x)
        vs.append(v)
    return np.stack(xs, axis=1), np.stack(vs, axis=1)


# ---- the case table of the operator: W = Q + 1 across every column-tile edge (Q = 15 | 16, 31 | 32, 47 | 48, 63: the d column in
# the padding, in a tile of its own, in the last column of the last tile), M across the 64-row slab / chunk edges as a cross with
# one Q of three tile counts, N around the NP = 8 / 2 / 1 / 1 points per workgroup of QT = 1 .. 4, K in {1, 3}.
def points_per_group(q):
    qt = (q + 1 + 15) // 16
    return 8 if qt == 1 else 2 if qt == 2 else 1


def _cases():
    out = [dict(K=3, N=points_per_group(q) + 1, M=50, Q=q) for q in (1, 2, 10, 15, 16, 17, 31, 32, 47, 48, 63)]
    out += [dict(K=1 + 2 * (i % 2), N=points_per_group(q) + 1, M=m, Q=q)
            for q in (10, 16, 48) for i, m in enumerate((1, 3, 63, 64, 65, 128, 130))]
    out += [dict(K=3, N=n, M=50, Q=10) for n in (1, 7, 8, 65)]
    out += [dict(K=1, N=n, M=50, Q=q) for q, n in ((16, 1), (16, 2), (31, 5), (32, 1), (47, 3), (48, 1), (63, 1), (63, 3))]
    out += [dict(K=1, N=9, M=50, Q=10), dict(K=1, N=1, M=1, Q=1)]
    return out


CASES = _cases()
BASE = CASES.index(dict(K=3, N=9, M=50, Q=10))
WIDE = CASES.index(dict(K=3, N=3, M=50, Q=17))


def case_id(c):
    return 'K%d-N%d-M%d-Q%d' % (c['K'], c['N'], c['M'], c['Q'])


def inputs(k, n, m, q, seed):
    """z, x, v ~ N(0, 1) / sqrt(Q) (the exponent stays O(1) at every Q), gamma in [0.2, 3], random indefinite NON-symmetric p."""
    rng = np.random.default_rng(seed)
    s = 1.0 / np.sqrt(q)
    inp = dict(z=s * rng.standard_normal((k, m, q)), x=s * rng.standard_normal((n, q)), v=s * rng.standard_normal((n, q)),
               gamma=rng.uniform(0.2, 3.0, (k, q)), alpha=rng.uniform(0.5, 2.0, k), p=rng.standard_normal((k, m, m)))
    for a in inp.values():
        a.setflags(write=False)
    return inp


@functools.lru_cache(maxsize=None)
def case(i):
    """(inputs, references) of CASES[i]: read-only arrays, computed once per process."""
    c = CASES[i]
    inp = inputs(c['K'], c['N'], c['M'], c['Q'], 9100 + i)
    g, g_den, gam, gam_den = christoffel_ref(inp['z'], inp['x'], inp['v'], inp['gamma'], inp['alpha'], inp['p'])
    ref = dict(g=g, g_den=g_den, gam=gam, gam_den=gam_den)
    for a in ref.values():
        a.setflags(write=False)
    return inp, ref


# ---- the finishing operator's cases: symmetric positive definite slabs' sums of condition number <= 1e4 ---------------------------
MAX_COND = 1e4
ACCEL_CASES = [dict(K=1, N=5, Q=1), dict(K=5, N=5, Q=1), dict(K=1, N=6, Q=3), dict(K=5, N=70, Q=3), dict(K=5, N=4, Q=10),
               dict(K=1, N=3, Q=63), dict(K=5, N=3, Q=63), dict(K=1, N=2, Q=64)]


def accel_case_id(c):
    return 'K%d-N%d-Q%d' % (c['K'], c['N'], c['Q'])


@functools.lru_cache(maxsize=None)
def accel_case(i):
    """(inputs, references): K indefinite symmetric slabs g whose sum plus diag(prior) has eigenvalues in [1, 100] times a scale."""
    c = ACCEL_CASES[i]
    k, n, q = c['K'], c['N'], c['Q']
    rng = np.random.default_rng(9500 + i)
    g = rng.standard_normal((k, n, q, q))
    g = 0.5 * (g + g.transpose(0, 1, 3, 2))
    basis = np.linalg.qr(rng.standard_normal((n, q, q)))[0]
    want = np.einsum('nqi,ni,nri->nqr', basis, rng.uniform(1.0, 100.0, (n, q)), basis)
    prior = rng.uniform(0.5, 2.0, q)
    g[0] += 0.5 * (want + want.transpose(0, 2, 1)) - np.sum(g, axis=0) - np.diag(prior)[None]
    inp = dict(g=g, gam=rng.standard_normal((k, n, q)), prior=prior, v=rng.standard_normal((n, q)))
    for a in inp.values():
        a.setflags(write=False)
    a, speed, info, big = accel_ref(inp['g'], inp['gam'], inp['prior'], inp['v'])
    ref = dict(a=a, speed=speed, info=info, G=big)
    return inp, ref


# ---- the integrator fixture: M = 20, Q = 3, one kernel, a symmetric INDEFINITE p, a prior that keeps cond(G) <= 1e4 -------------
@functools.lru_cache(maxsize=None)
def fixture():
    rng = np.random.default_rng(77)
    m, q = 20, 3
    a = rng.standard_normal((m, m))
    fix = dict(z=rng.standard_normal((1, m, q)), gamma=rng.uniform(0.5, 1.5, (1, q)), alpha=np.array([1.0]),
               p=(0.15 * (a + a.T))[None], prior=np.array([4.0, 5.0, 6.0]),
               x=0.3 * rng.standard_normal((4, q)), v=0.8 * rng.standard_normal((4, q)))
    for t in fix.values():
        t.setflags(write=False)
    return fix


def fixture_metric(x, dtype=np.float64):
    f = fixture()
    g, _ = metric_ref(f['z'], x, f['gamma'], f['alpha'], f['p'])
    return (np.asarray(g[0], dtype=LD) + np.diag(f['prior'])[None]).astype(dtype)


def fixture_accel(x, v):
    """The fp64 acceleration of the fixture from the long-double references; asserts the factorisation went through."""
    f = fixture()
    g, _, gam, _ = christoffel_ref(f['z'], x, v, f['gamma'], f['alpha'], f['p'])
    a, _, info, _ = accel_ref(g, gam, f['prior'], v)
    assert not info.any()
    return a.astype(np.float64)


def drift_and_return(shoot, metric, x, v, steps):
    """(relative drift of v^T G v at the end, |return error| / |v|) of `shoot`(x, v, S) -> (curve, velocities) [C, S+1, Q]: the speed
    is conserved along a geodesic, and shooting back from the end with the reversed velocity returns to the start."""
    c, w = shoot(x, v, steps)
    speed = lambda xx, vv: np.einsum('nq,nqr,nr->n', vv, metric(xx), vv)
    s0, s1 = speed(c[:, 0], w[:, 0]), speed(c[:, -1], w[:, -1])
    back, _ = shoot(c[:, -1], -w[:, -1], steps)
    return np.max(np.abs(s1 - s0) / s0), np.max(np.linalg.norm(back[:, -1] - x, axis=1) / np.linalg.norm(v, axis=1))


def check_fourth_order(shoot, metric, x, v):
    """The ratio test of the integrator: halving the step divides the drift and the return error by >= 8 (fourth order gives 16;
    8 leaves room for the next-order term), with both figures above 1e-9 so that the ratio is not one of rounding errors."""
    d8, r8 = drift_and_return(shoot, metric, x, v, 8)
    d16, r16 = drift_and_return(shoot, metric, x, v, 16)
    print('drift of v^T G v: %.3e at 8 steps, %.3e at 16 (ratio %.1f); return error %.3e, %.3e (ratio %.1f)'
          % (d8, d16, d8 / d16, r8, r16, r8 / r16))
    assert d8 > 1e-9 and d16 > 1e-9 and r8 > 1e-9 and r16 > 1e-9
    assert d8 / d16 >= 8.0 and r8 / r16 >= 8.0
    return d8, d16, r8, r16


# ---- checks of the references ----------------------------------------------------------------------------------------------------
def test_gam_is_the_contracted_christoffel_symbol_of_the_reference_metric():
    """(i): gam of a SYMMETRIC p against central differences of the reference metric, (D_v G) v - 1/2 grad_x (v^T G v)."""
    for seed, (k, n, m, q) in enumerate([(1, 3, 20, 3), (2, 2, 7, 5), (1, 2, 70, 17)]):
        inp = dict(inputs(k, n, m, q, 300 + seed))
        p = np.asarray(inp['p'])
        inp['p'] = 0.5 * (p + p.transpose(0, 2, 1))
        _, _, gam, _ = christoffel_ref(inp['z'], inp['x'], inp['v'], inp['gamma'], inp['alpha'], inp['p'])
        x, v = np.asarray(inp['x'], dtype=LD), np.asarray(inp['v'], dtype=LD)
        metric = lambda xx: metric_ref(inp['z'], xx, inp['gamma'], inp['alpha'], inp['p'])[0]
        h = LD(1e-5)
        dvg = (metric(x + h * v) - metric(x - h * v)) / (2 * h)                        # D_v G [K, N, Q, Q]
        first = np.einsum('knqr,nr->knq', dvg, v)
        grad = np.zeros_like(first)
        for j in range(q):
            e = np.zeros(q, dtype=LD)
            e[j] = h
            grad[:, :, j] = np.einsum('nq,knqr,nr->kn', v, metric(x + e) - metric(x - e), v) / (2 * h)
        want = first - 0.5 * grad
        err, scale = float(np.max(np.abs(gam - want))), float(np.max(np.abs(want)))
        print('K%d N%d M%d Q%d: |gam - central differences| %.2e of %.2e' % (k, n, m, q, err, scale))
        assert scale > 1e-3 and err <= 1e-5 * scale


def test_g_is_the_metric_reference():
    """(ii)"""
    for i in (BASE, WIDE):
        inp, ref = case(i)
        g, _ = metric_ref(inp['z'], inp['x'], inp['gamma'], inp['alpha'], inp['p'])
        assert np.max(np.abs(ref['g'] - g)) <= 1e-15 * np.max(np.abs(g))


def test_accel_reference_solves_its_system_and_reports_the_pivot():
    for i in range(len(ACCEL_CASES)):
        inp, ref = accel_case(i)
        big = np.asarray(ref['G'], dtype=np.float64)
        assert np.all(np.linalg.cond(big) <= MAX_COND), accel_case_id(ACCEL_CASES[i])
        assert not ref['info'].any()
        res = np.einsum('nqr,nr->nq', ref['G'], ref['a']) + np.sum(np.asarray(inp['gam'], dtype=LD), axis=0)
        assert np.max(np.abs(res)) <= 1e-15 * np.max(np.abs(inp['gam'])) * MAX_COND
    bad = np.diag([2.0, 3.0, -1.0, 4.0])
    assert cholesky_ref(bad)[1] == 3 and cholesky_ref(np.eye(3))[1] == 0


def test_integrator_fixture_is_well_conditioned_and_fourth_order():
    """(iii)"""
    f = fixture()
    met = []

    def metric(x):
        g = fixture_metric(x)
        met.append(g)
        return g

    def accel(x, v):
        metric(x)
        return fixture_accel(x, v)

    shoot = lambda x, v, s: rk4_ref(accel, x, v, s)
    p = np.asarray(f['p'][0])
    assert np.array_equal(p, p.T) and np.linalg.eigvalsh(p)[0] < -0.1 < 0.1 < np.linalg.eigvalsh(p)[-1]
    check_fourth_order(shoot, metric, np.asarray(f['x']), np.asarray(f['v']))
    conds = np.linalg.cond(np.concatenate(met))
    print('%d metrics met, condition number <= %.1f' % (conds.size, conds.max()))
    assert conds.max() <= MAX_COND
    moved = np.concatenate(met)
    assert np.max(np.abs(moved - np.diag(f['prior']))) > 0.1                       # (the data term is alive along the curves)


def test_case_tables_cover_the_edges_and_are_alive():
    assert {1, 2, 10, 15, 16, 17, 31, 32, 47, 48, 63} <= {c['Q'] for c in CASES}
    for q in (10, 16, 48):
        assert {1, 3, 63, 64, 65, 128, 130} <= {c['M'] for c in CASES if c['Q'] == q}
    for q, ns in ((10, {1, 7, 8, 9}), (16, {1, 2, 3}), (32, {1, 2}), (48, {1, 2}), (63, {1, 2})):
        assert ns <= {c['N'] for c in CASES if c['Q'] == q}, q
    assert {1, 3} <= {c['K'] for c in CASES}
    alive = 0
    for i in range(len(CASES)):
        _, ref = case(i)
        assert all(np.all(np.isfinite(a)) for a in ref.values()), case_id(CASES[i])
        alive += float(np.max(np.abs(ref['gam']))) > 1e-6 and float(np.max(np.abs(ref['g']))) > 1e-6
    assert alive >= 0.9 * len(CASES), (alive, len(CASES))
