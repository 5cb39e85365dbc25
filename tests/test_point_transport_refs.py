"""CPU tests (no GPU) of the references that pin ops.ard_rbf_point_transport / ops.geodesic_transport
(csrc/ard_rbf_point_metric.hip, csrc/geodesic_accel.hip) and latent_parallel_transport (models/geodesic.parallel_transport): NumPy
restatements in np.longdouble, the RK4 of the transport equation restated in NumPy, the case table that
tests/test_gpu_point_transport.py runs, and checks of the references themselves.  Notation of test_point_christoffel_refs, and for a
frame of F vectors w_r at a point with velocity v, per kernel, point and inducing point, with u_q = gamma_q (x_q - z_mq):

    a_v = sum_q u_q v_q,   a_w = sum_q u_q w_q,   d(v, w) = v^T (d^2 k / dx dx) w = k (a_v a_w - sum_q gamma_q v_q w_q)
    transport_ref:        tgam[k,n,r,q] = sum_{m,m'} b_kmq(x_n) p[k,m,m'] d_km'(v_n, w_nr)
    accel_transport_ref:  dw[n,r] = -G_n^-1 sum_k tgam[k,n,r]      on accel_ref's Cholesky factor
For a symmetric p, tgam is the Christoffel symbol of the first kind of g contracted with v and w, and w' = dw is parallel transport
along the geodesic x'' = a.  Every operator reference also returns the sum of the absolute values of each entry's terms, the
denominator of the GPU file's tolerance."""
import functools

import numpy as np

from test_point_christoffel_refs import (ACCEL_CASES, MAX_COND, accel_case, accel_case_id, accel_ref, cholesky_ref, christoffel_ref,
                                         fixture, fixture_accel, fixture_metric, inputs, rk4_ref)
from test_point_metric_refs import features_ref, metric_ref
from test_point_tangent_refs import SYM_SHAPES, _chol_solve, accel_tangent_ref, tangent_ref

LD = np.longdouble


def mixed_second_ref(z, x, v, w, gamma, alpha):
    """(d(v, w_r), |terms| of it) [K, N, F, M] in np.longdouble; w [N, F, Q]."""
    z, x, v, w, gamma, alpha = (np.asarray(a, dtype=LD) for a in (z, x, v, w, gamma, alpha))
    gm = gamma[:, None, None, :]
    diff = x[None, :, None, :] - z[:, None, :, :]                                # [K, N, M, Q]
    kv = alpha.reshape(-1)[:, None, None] * np.exp(-0.5 * np.sum(gm * diff * diff, axis=-1))
    u = gm * diff
    av, av_abs = np.einsum('knmq,nq->knm', u, v), np.einsum('knmq,nq->knm', np.abs(u), np.abs(v))
    aw, aw_abs = np.einsum('knmq,nfq->knfm', u, w), np.einsum('knmq,nfq->knfm', np.abs(u), np.abs(w))
    c = np.einsum('kq,nq,nfq->knf', gamma, v, w)[..., None]                      # [K, N, F, 1]
    c_abs = np.einsum('kq,nq,nfq->knf', gamma, np.abs(v), np.abs(w))[..., None]
    return kv[:, :, None, :] * (av[:, :, None, :] * aw - c), kv[:, :, None, :] * (av_abs[:, :, None, :] * aw_abs + c_abs)


def transport_ref(z, x, v, w, gamma, alpha, p):
    """(tgam, tgam_den) [K, N, F, Q] in np.longdouble."""
    b, p = features_ref(z, x, gamma, alpha), np.asarray(p, dtype=LD)
    d, d_abs = mixed_second_ref(z, x, v, w, gamma, alpha)
    tgam = np.einsum('knmq,kmj,knfj->knfq', b, p, d)
    den = np.einsum('knmq,kmj,knfj->knfq', *(np.asarray(a, dtype=np.float64) for a in (np.abs(b), np.abs(p), d_abs)))
    return tgam, den.astype(LD)


def accel_transport_ref(g, gam, tgam, prior, v, dtype=LD):
    """(a [N, Q], dw [N, F, Q], speed [N], info [N], G [N, Q, Q]) in `dtype`: accel_ref's results, and dw on the same factor."""
    a, speed, info, big = accel_ref(g, gam, prior, v, dtype)
    rhs = -np.sum(np.asarray(tgam, dtype=dtype), axis=0)                          # [N, F, Q]
    dw = np.full(rhs.shape, np.nan, dtype=dtype)
    for i in range(rhs.shape[0]):
        if info[i]:
            continue
        l, _ = cholesky_ref(big[i])
        for r in range(rhs.shape[1]):
            dw[i, r] = _chol_solve(l, rhs[i, r])
    return a, dw, speed, info, big


def rk4_transport_ref(transport, x, v, w, num_steps):
    """(curve, velocities [C, S+1, Q], frames [C, S+1, F, Q]): the NumPy restatement of models/geodesic._rk4_transport, the
    classical RK4 on the state (x, v, w_1 .. w_F); transport: (x, v [C, Q], w [C, F, Q]) -> (a [C, Q], dw [C, F, Q]).  The x and v
    statements are rk4_ref's."""
    x, v, w = (np.array(t, dtype=np.float64) for t in (x, v, w))
    h = 1.0 / num_steps
    xs, vs, ws = [x], [v], [w]
    for _ in range(num_steps):
        k1x = v
        k1v, k1w = transport(x, v, w)
        k2x = v + 0.5 * h * k1v
        k2v, k2w = transport(x + 0.5 * h * k1x, k2x, w + 0.5 * h * k1w)
        k3x = v + 0.5 * h * k2v
        k3v, k3w = transport(x + 0.5 * h * k2x, k3x, w + 0.5 * h * k2w)
        k4x = v + h * k3v
        k4v, k4w = transport(x + h * k3x, k4x, w + h * k3w)
        x = x + (h / 6.0) * (k1x + 2.0 * k2x + 2.0 * k3x + k4x)
        v = v + (h / 6.0) * (k1v + 2.0 * k2v + 2.0 * k3v + k4v)
        w = w + (h / 6.0) * (k1w + 2.0 * k2w + 2.0 * k3w + k4w)
        xs.append(x)
        vs.append(v)
        ws.append(w)
    return np.stack(xs, axis=1), np.stack(vs, axis=1), np.stack(ws, axis=1)


def fixture_transport(x, v, w, f=None):
    """The fp64 (a, dw) of the integrator fixture (or of f, a dict of the same keys) from the long-double references; a is
    fixture_accel's; asserts the factorisation went through."""
    f = fixture() if f is None else f
    g, _, gam, _ = christoffel_ref(f['z'], x, v, f['gamma'], f['alpha'], f['p'])
    tgam, _ = transport_ref(f['z'], x, v, w, f['gamma'], f['alpha'], f['p'])
    a, dw, _, info, _ = accel_transport_ref(g, gam, tgam, f['prior'], v)
    assert not info.any()
    return a.astype(np.float64), dw.astype(np.float64)


@functools.lru_cache(maxsize=None)
def fixture_frame(num=2):
    """`num` vectors per curve of the integrator fixture, of the size of its velocities."""
    f = fixture()
    w = 0.8 * np.random.default_rng(78).standard_normal((f['x'].shape[0], num, f['x'].shape[1]))
    w.setflags(write=False)
    return w


def gram(metric, x, w):
    """<w_i, w_j>_G [C, F, F] at the points x [C, Q]; metric: x -> G [C, Q, Q]."""
    return np.einsum('cfq,cqr,cgr->cfg', w, metric(x), w)


def gram_drift_and_return(shoot, metric, x, v, w, steps):
    """(drift of the frame's Gram matrix at the end relative to its largest entry, |return error| / |w|) of
    `shoot`(x, v, w, S) -> (curve, velocities, frames): parallel transport keeps every <w_i, w_j>_G, and transporting the end
    frame back from the end with the reversed velocity returns w."""
    c, u, fr = shoot(x, v, w, steps)
    g0, g1 = gram(metric, c[:, 0], fr[:, 0]), gram(metric, c[:, -1], fr[:, -1])
    _, _, back = shoot(c[:, -1], -u[:, -1], fr[:, -1], steps)
    ret = np.linalg.norm(back[:, -1] - w, axis=-1) / np.linalg.norm(w, axis=-1)
    return float(np.max(np.abs(g1 - g0)) / np.max(np.abs(g0))), float(np.max(ret))


def check_transport_fourth_order(shoot, metric, x, v, w):
    """The ratio test of the transport integrator: halving the step divides the Gram drift and the return error by >= 8 (fourth
    order gives 16; 8 leaves room for the next-order term), with both figures at 16 steps above 1e-10 of their scale so that the
    ratio is not taken between rounding errors."""
    d8, r8 = gram_drift_and_return(shoot, metric, x, v, w, 8)
    d16, r16 = gram_drift_and_return(shoot, metric, x, v, w, 16)
    print('Gram drift: %.3e at 8 steps, %.3e at 16 (ratio %.1f); return error %.3e, %.3e (ratio %.1f)'
          % (d8, d16, d8 / d16, r8, r16, r8 / r16))
    assert d16 > 1e-10 and r16 > 1e-10
    assert d8 / d16 >= 8.0 and r8 / r16 >= 8.0
    return d8, d16, r8, r16


# ---- the case table of the operator: W = Q + 1 + F across every column-tile edge (16 | 17, 32 | 33, 48 | 49, 64), the frame in the
# padding, in tiles of its own, one vector beside a wide Q and a wide frame beside Q = 1; M across the 64-row slab / chunk edges at
# three (Q, F); N around the NP = 8 / 2 / 1 / 1 points per workgroup of QT = 1 .. 4; K alternating 1 / 3.
MAX_W = 64


def transport_tiles(q, f):
    """mt_qt of the transport mode."""
    return (q + 1 + f + 15) // 16


def points_per_group(q, f):
    """MtCfg<QT>::NP."""
    qt = transport_tiles(q, f)
    return 8 if qt == 1 else 2 if qt == 2 else 1


def unread_tile(q, qi):
    """mt_trn_unread: result tiles of row tile qi are not formed."""
    return 16 * qi >= q


QF_CASES = [(1, 1), (10, 1), (10, 5), (10, 6), (10, 10), (14, 1), (15, 1), (15, 16), (15, 17), (23, 24), (23, 25), (31, 31), (31, 32),
            (62, 1), (1, 62)]
M_EDGES = (1, 3, 63, 64, 65, 128, 130)
N_EDGES = {(10, 5): (1, 7, 8, 9, 65), (10, 10): (1, 2, 3), (15, 17): (1, 2), (31, 32): (1, 2)}


def _cases():
    shapes = [(points_per_group(q, f) + 1, 50, q, f) for q, f in QF_CASES]
    shapes += [(points_per_group(q, f) + 1, m, q, f) for m in M_EDGES for q, f in ((7, 3), (10, 5), (10, 10))]
    shapes += [(n, 50, q, f) for (q, f), ns in N_EDGES.items() for n in ns]
    out = []
    for n, m, q, f in shapes:
        c = dict(K=1 + 2 * (len(out) % 2), N=n, M=m, Q=q, F=f)
        if c not in out and dict(c, K=4 - c['K']) not in out:
            out.append(c)
    return out


CASES = _cases()
QT_CASES = {transport_tiles(q, f): [i for i, c in enumerate(CASES) if (c['Q'], c['F'], c['M']) == (q, f, 50)
                                    and c['N'] == points_per_group(q, f) + 1][0] for q, f in N_EDGES}


def case_id(c):
    return 'K%d-N%d-M%d-Q%d-F%d' % (c['K'], c['N'], c['M'], c['Q'], c['F'])


def transport_inputs(k, n, m, q, f, seed):
    """inputs() of the christoffel file plus a frame w ~ N(0, 1) / sqrt(Q) [N, F, Q]."""
    inp = dict(inputs(k, n, m, q, seed))
    inp['w'] = np.random.default_rng(seed + 70000).standard_normal((n, f, q)) / np.sqrt(q)
    for a in inp.values():
        a.setflags(write=False)
    return inp


def run_refs(inp):
    g, g_den, gam, gam_den = christoffel_ref(inp['z'], inp['x'], inp['v'], inp['gamma'], inp['alpha'], inp['p'])
    tgam, tgam_den = transport_ref(inp['z'], inp['x'], inp['v'], inp['w'], inp['gamma'], inp['alpha'], inp['p'])
    ref = dict(g=g, g_den=g_den, gam=gam, gam_den=gam_den, tgam=tgam, tgam_den=tgam_den)
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def case(i):
    """(inputs, references) of CASES[i]: read-only arrays, computed once per process."""
    c = CASES[i]
    inp = transport_inputs(c['K'], c['N'], c['M'], c['Q'], c['F'], 10300 + i)
    return inp, run_refs(inp)


@functools.lru_cache(maxsize=None)
def accel_transport_case(i, f):
    """accel_case(i) of the christoffel file with a random tgam of F = f vectors (f = 0: F = Q): (inputs, references)."""
    inp, _ = accel_case(i)
    k, n, q = inp['gam'].shape
    rng = np.random.default_rng(10900 + 10 * i + f)
    inp = dict(inp, tgam=rng.standard_normal((k, n, f or q, q)))
    for a in inp.values():
        a.setflags(write=False)
    a, dw, speed, info, big = accel_transport_ref(inp['g'], inp['gam'], inp['tgam'], inp['prior'], inp['v'])
    return inp, dict(a=a, dw=dw, speed=speed, info=info, G=big)


# ---- checks of the references ----------------------------------------------------------------------------------------------------
def _sym(inp):
    p = np.asarray(inp['p'])
    return dict(inp, p=0.5 * (p + p.transpose(0, 2, 1)))


def test_tgam_is_the_christoffel_symbol_of_the_reference_metric():
    """Gamma(v, w) of a SYMMETRIC p against central differences of the long-double metric reference,
    1/2 (D_v g w + D_w g v - grad_x (v^T g w)), h = 1e-5."""
    for seed, (k, n, m, q) in enumerate(SYM_SHAPES):
        inp = _sym(transport_inputs(k, n, m, q, 2, 500 + seed))
        tgam, _ = transport_ref(inp['z'], inp['x'], inp['v'], inp['w'], inp['gamma'], inp['alpha'], inp['p'])
        x, v = np.asarray(inp['x'], dtype=LD), np.asarray(inp['v'], dtype=LD)
        metric = lambda xx: metric_ref(inp['z'], xx, inp['gamma'], inp['alpha'], inp['p'])[0]
        h = LD(1e-5)
        dvg = (metric(x + h * v) - metric(x - h * v)) / (2 * h)                        # D_v g [K, N, Q, Q]
        for r in range(2):
            w = np.asarray(inp['w'][:, r], dtype=LD)
            dwg = (metric(x + h * w) - metric(x - h * w)) / (2 * h)
            grad = np.zeros(dvg.shape[:3], dtype=LD)
            for j in range(q):
                e = np.zeros(q, dtype=LD)
                e[j] = h
                grad[:, :, j] = np.einsum('nq,knqr,nr->kn', v, metric(x + e) - metric(x - e), w) / (2 * h)
            want = 0.5 * (np.einsum('knqr,nr->knq', dvg, w) + np.einsum('knqr,nr->knq', dwg, v) - grad)
            err, scale = float(np.max(np.abs(tgam[:, :, r] - want))), float(np.max(np.abs(want)))
            print('K%d N%d M%d Q%d r%d: |tgam - central differences| %.2e of %.2e' % (k, n, m, q, r, err, scale))
            assert scale > 1e-3 and err <= 1e-5 * scale


def test_tgam_is_half_the_tangent_of_gam_along_the_velocity():
    """tgam = 1/2 dgam of tangent_ref(dx = 0, dv = w), any p; and the same through the two finishing references."""
    for seed, (k, n, m, q) in enumerate(SYM_SHAPES):
        inp = transport_inputs(k, n, m, q, 3, 520 + seed)
        tgam, _ = transport_ref(inp['z'], inp['x'], inp['v'], inp['w'], inp['gamma'], inp['alpha'], inp['p'])
        g, _, gam, _ = christoffel_ref(inp['z'], inp['x'], inp['v'], inp['gamma'], inp['alpha'], inp['p'])
        prior = np.full(q, 50.0 * float(np.max(np.abs(g))))                             # (any positive definite G will do)
        _, dw, _, info, _ = accel_transport_ref(g, gam, tgam, prior, inp['v'])
        assert not info.any()
        for r in range(3):
            dg, _, dgam, _ = tangent_ref(inp['z'], inp['x'], inp['v'], np.zeros_like(inp['x']), inp['w'][:, r], inp['gamma'],
                                         inp['alpha'], inp['p'])
            assert np.all(dg == 0)
            err, scale = float(np.max(np.abs(tgam[:, :, r] - 0.5 * dgam))), float(np.max(np.abs(dgam)))
            print('K%d N%d M%d Q%d r%d: |tgam - dgam / 2| %.2e of %.2e' % (k, n, m, q, r, err, scale))
            assert scale > 1e-3 and err <= 1e-12 * scale
            da = accel_tangent_ref(g, gam, dg, dgam, prior, inp['v'])[1]
            assert np.max(np.abs(dw[:, r] - 0.5 * da)) <= 1e-12 * np.max(np.abs(da))


def test_reference_symbol_is_symmetric_linear_and_zero_for_a_zero_vector():
    inp = _sym(transport_inputs(2, 3, 20, 5, 2, 540))
    run = lambda v, w: transport_ref(inp['z'], inp['x'], v, w, inp['gamma'], inp['alpha'], inp['p'])[0]
    v, w = np.asarray(inp['v'], dtype=LD), np.asarray(inp['w'], dtype=LD)
    one = run(v, w)
    for r in range(2):                                                                  # Gamma(v, w_r) = Gamma(w_r, v)
        swapped = run(w[:, r], v[:, None, :])[:, :, 0]
        assert np.max(np.abs(one[:, :, r] - swapped)) <= 1e-16 * np.max(np.abs(one))
    w2 = np.asarray(np.random.default_rng(6).standard_normal(w.shape), dtype=LD)
    both, two = run(v, LD(2.5) * w - w2), run(v, w2)
    assert np.max(np.abs(both - (LD(2.5) * one - two))) <= 1e-15 * np.max(np.abs(one))
    assert all(np.all(t == 0) for t in transport_ref(inp['z'], inp['x'], v, np.zeros_like(w), inp['gamma'], inp['alpha'], inp['p']))
    same = run(v, np.stack([v, v], axis=1))                                             # w = v: the contracted symbol
    gam = christoffel_ref(inp['z'], inp['x'], v, inp['gamma'], inp['alpha'], inp['p'])[2]
    assert np.max(np.abs(same - gam[:, :, None, :])) <= 1e-16 * np.max(np.abs(gam))


def test_accel_transport_reference_solves_its_systems():
    for i in range(len(ACCEL_CASES)):
        for f in (1, 3, 0):
            inp, ref = accel_transport_case(i, f)
            _, plain = accel_case(i)
            assert np.array_equal(ref['a'], plain['a']) and not ref['info'].any()
            rhs = np.sum(np.asarray(inp['tgam'], dtype=LD), axis=0)
            res = np.einsum('nqr,nfr->nfq', ref['G'], ref['dw']) + rhs
            assert np.max(np.abs(res)) <= 1e-15 * np.max(np.abs(rhs)) * MAX_COND, accel_case_id(ACCEL_CASES[i])


def test_transport_rk4_keeps_the_geodesic_and_moves_the_velocity_as_itself():
    f = fixture()
    x, v, w = np.asarray(f['x']), np.asarray(f['v']), np.asarray(fixture_frame())
    curve, vel, frames = rk4_transport_ref(fixture_transport, x, v, w, 16)
    plain = rk4_ref(fixture_accel, x, v, 16)
    assert np.array_equal(curve, plain[0]) and np.array_equal(vel, plain[1])
    assert np.array_equal(frames[:, 0], w)
    # w = v: the transported vector is the velocity curve (the two references sum Gamma(v, v) in different orders: rounding)
    _, vel2, own = rk4_transport_ref(fixture_transport, x, v, v[:, None, :], 16)
    assert np.max(np.abs(own[:, :, 0] - vel2)) <= 1e-14 * np.max(np.abs(vel2))


def test_transport_fixture_is_fourth_order():
    f = fixture()
    shoot = lambda x, v, w, s: rk4_transport_ref(fixture_transport, x, v, w, s)
    check_transport_fourth_order(shoot, fixture_metric, np.asarray(f['x']), np.asarray(f['v']), np.asarray(fixture_frame()))


@functools.lru_cache(maxsize=None)
def fixture_q1():
    """The integrator fixture at Q = 1: M = 20, one kernel, a symmetric indefinite p, prior 4."""
    rng = np.random.default_rng(79)
    m = 20
    a = rng.standard_normal((m, m))
    fix = dict(z=rng.standard_normal((1, m, 1)), gamma=np.array([[1.2]]), alpha=np.array([1.0]), p=(0.15 * (a + a.T))[None],
               prior=np.array([4.0]), x=0.3 * rng.standard_normal((4, 1)), v=0.8 * rng.standard_normal((4, 1)))
    for t in fix.values():
        t.setflags(write=False)
    return fix


def test_one_dimensional_transport_keeps_w_sqrt_g():
    """Q = 1: parallel transport keeps w(t) sqrt(g(x(t))); the drift falls as the Gram drift does."""
    f = fixture_q1()
    x, v = np.asarray(f['x']), np.asarray(f['v'])
    w = np.ones((x.shape[0], 1, 1))
    metric = lambda xx: (np.asarray(metric_ref(f['z'], xx, f['gamma'], f['alpha'], f['p'])[0][0], dtype=LD) + f['prior'][0]).astype(np.float64)
    assert np.min(metric(x)) > 0.5
    drift = {}
    for s in (8, 16):
        curve, _, frames = rk4_transport_ref(lambda xx, vv, ww: fixture_transport(xx, vv, ww, f), x, v, w, s)
        inv = frames[:, :, 0, 0] * np.sqrt(metric(curve.reshape(-1, 1))[:, 0, 0].reshape(curve.shape[:2]))
        assert np.max(np.abs(metric(curve[:, -1]) - metric(curve[:, 0]))) > 1e-3           # (the metric moves along the curves)
        drift[s] = float(np.max(np.abs(inv[:, -1] - inv[:, 0]) / np.abs(inv[:, 0])))
    print('drift of w sqrt(g): %.3e at 8 steps, %.3e at 16 (ratio %.1f)' % (drift[8], drift[16], drift[8] / drift[16]))
    assert drift[16] > 1e-10 and drift[8] / drift[16] >= 8.0


def test_case_tables_cover_the_edges_and_are_alive():
    assert set(QF_CASES) <= {(c['Q'], c['F']) for c in CASES if c['M'] == 50}
    assert all(c['Q'] + 1 + c['F'] <= MAX_W for c in CASES)
    widths = {c['Q'] + 1 + c['F'] for c in CASES}
    assert {16, 17, 32, 33, 48, 49, 64} <= widths
    assert {transport_tiles(c['Q'], c['F']) for c in CASES} == {1, 2, 3, 4} and sorted(QT_CASES) == [1, 2, 3, 4]
    for qt in (1, 2, 3, 4):
        np_ = 8 if qt == 1 else 2 if qt == 2 else 1
        ns = {c['N'] for c in CASES if transport_tiles(c['Q'], c['F']) == qt}
        assert {1, np_, np_ + 1} <= ns, (qt, ns)
    for qf in ((7, 3), (10, 5), (10, 10)):
        assert set(M_EDGES) <= {c['M'] for c in CASES if (c['Q'], c['F']) == qf}
    assert {1, 63, 64, 65, 130} <= {c['M'] for c in CASES}
    assert {1, 3} <= {c['K'] for c in CASES}
    # the mirror of the kernel's rules: tile counts, points per workgroup, the result tiles that are not formed
    assert [transport_tiles(q, f) for q, f in ((10, 5), (10, 6), (15, 16), (15, 17), (23, 24), (23, 25), (31, 32))] == [1, 2, 2, 3, 3, 4, 4]
    assert [points_per_group(q, f) for q, f in ((10, 5), (10, 10), (15, 17), (31, 32))] == [8, 2, 1, 1]
    assert not unread_tile(1, 0) and unread_tile(10, 1) and unread_tile(16, 1) and not unread_tile(17, 1) and unread_tile(31, 2)
    skipped = {(c['Q'], c['F']): sum(unread_tile(c['Q'], qi) for qi in range(transport_tiles(c['Q'], c['F']))) for c in CASES}
    assert skipped[(10, 5)] == 0 and skipped[(10, 10)] == 1 and skipped[(15, 17)] == 2 and skipped[(1, 62)] == 3 and skipped[(62, 1)] == 0
    alive = 0
    for i in range(len(CASES)):
        _, ref = case(i)
        assert all(np.all(np.isfinite(a)) for a in ref.values()), case_id(CASES[i])
        alive += float(np.max(np.abs(ref['tgam']))) > 1e-6
    assert alive >= 0.9 * len(CASES), (alive, len(CASES))
