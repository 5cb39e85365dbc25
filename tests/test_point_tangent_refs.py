"""CPU tests (no GPU) of the references that pin ops.ard_rbf_point_christoffel_tangent / ops.geodesic_accel_tangent
(csrc/ard_rbf_point_metric.hip, csrc/geodesic_accel.hip), latent_exp_map_tangent and latent_log_map (models/geodesic.py): NumPy
restatements in np.longdouble, the tangent-linear RK4 and the Newton shooting restated in NumPy, the case table that
tests/test_gpu_point_tangent.py runs, and checks of the references themselves.  Notation of test_point_christoffel_refs, and along
a direction (dx, dv) of the state (x, v), per kernel, point and inducing point, with u_q = gamma_q (x_q - z_mq), a = sum_q u_q v_q,
s = sum_q gamma_q v_q^2:

    e = sum_q u_q dx_q,   f = sum_q u_q dv_q,   c1 = sum_q gamma_q dx_q v_q,   c2 = sum_q gamma_q v_q dv_q
    db_q = k (e u_q - gamma_q dx_q),            dd = k (-e (a^2 - s) + 2 a (c1 + f) - 2 c2)
    tangent_ref:        dg = dB^T p B + B^T p dB,    dgam = dB^T p d + B^T p dd
    accel_tangent_ref:  da = -G^-1 (sum_k dgam + (sum_k dg) a)      on accel_ref's Cholesky factor
Every operator reference also returns the sum of the absolute values of each entry's terms, the denominator of the GPU file's
tolerance."""
import functools

import numpy as np

from test_point_christoffel_refs import (ACCEL_CASES, MAX_COND, accel_case, accel_case_id, accel_ref, cholesky_ref, christoffel_ref,
                                         fixture, fixture_accel, inputs, rk4_ref, second_ref)
from test_point_metric_refs import features_ref

LD = np.longdouble


def tangent_ref(z, x, v, dx, dv, gamma, alpha, p):
    """(dg, dg_den [K, N, Q, Q], dgam, dgam_den [K, N, Q]) in np.longdouble."""
    b = features_ref(z, x, gamma, alpha)
    d, d_abs = second_ref(z, x, v, gamma, alpha)
    z, x, v, dx, dv, gamma, alpha, p = (np.asarray(a, dtype=LD) for a in (z, x, v, dx, dv, gamma, alpha, p))
    gm = gamma[:, None, None, :]
    diff = x[None, :, None, :] - z[:, None, :, :]                                # [K, N, M, Q]
    kv = alpha.reshape(-1)[:, None, None] * np.exp(-0.5 * np.sum(gm * diff * diff, axis=-1))
    u = gm * diff
    dot = lambda w: (np.sum(u * w[None, :, None, :], axis=-1), np.sum(np.abs(u * w[None, :, None, :]), axis=-1))
    (a, a_abs), (e, e_abs), (f, f_abs) = dot(v), dot(dx), dot(dv)
    per_point = lambda w1, w2: np.sum(gamma[:, None, :] * (w1 * w2)[None], axis=-1)[:, :, None]          # [K, N, 1]
    s, c1, c2 = per_point(v, v), per_point(dx, v), per_point(v, dv)
    c1_abs, c2_abs = per_point(np.abs(dx), np.abs(v)), per_point(np.abs(v), np.abs(dv))
    db = kv[..., None] * (e[..., None] * u - gm * dx[None, :, None, :])
    db_abs = kv[..., None] * (e_abs[..., None] * np.abs(u) + gm * np.abs(dx)[None, :, None, :])
    dd = kv * (-e * (a * a - s) + 2 * a * (c1 + f) - 2 * c2)
    dd_abs = kv * (e_abs * (a_abs * a_abs + s) + 2 * a_abs * (c1_abs + f_abs) + 2 * c2_abs)
    dg = np.einsum('knmq,kmj,knjr->knqr', db, p, b) + np.einsum('knmq,kmj,knjr->knqr', b, p, db)
    dgam = np.einsum('knmq,kmj,knj->knq', db, p, d) + np.einsum('knmq,kmj,knj->knq', b, p, dd)
    f64 = lambda *arrays: [np.asarray(t, dtype=np.float64) for t in arrays]
    ab, apm, adb, ad, add = f64(np.abs(b), np.abs(p), db_abs, d_abs, dd_abs)
    dg_den = np.einsum('knmq,kmj,knjr->knqr', adb, apm, ab) + np.einsum('knmq,kmj,knjr->knqr', ab, apm, adb)
    dgam_den = np.einsum('knmq,kmj,knj->knq', adb, apm, ad) + np.einsum('knmq,kmj,knj->knq', ab, apm, add)
    return dg, dg_den.astype(LD), dgam, dgam_den.astype(LD)


def _chol_solve(l, rhs):
    q = rhs.shape[0]
    y, out = np.zeros(q, dtype=rhs.dtype), np.zeros(q, dtype=rhs.dtype)
    for j in range(q):
        y[j] = (rhs[j] - l[j, :j] @ y[:j]) / l[j, j]
    for j in range(q - 1, -1, -1):
        out[j] = (y[j] - l[j + 1:, j] @ out[j + 1:]) / l[j, j]
    return out


def accel_tangent_ref(g, gam, dg, dgam, prior, v, dtype=LD):
    """(a, da [N, Q], speed [N], info [N], G [N, Q, Q]) in `dtype`: accel_ref's results, and da on the same Cholesky factor."""
    a, speed, info, big = accel_ref(g, gam, prior, v, dtype)
    dg, dgam = np.sum(np.asarray(dg, dtype=dtype), axis=0), np.sum(np.asarray(dgam, dtype=dtype), axis=0)
    da = np.full(a.shape, np.nan, dtype=dtype)
    for i in range(a.shape[0]):
        if info[i]:
            continue
        l, _ = cholesky_ref(big[i])
        da[i] = _chol_solve(l, -(dgam[i] + dg[i] @ a[i]))
    return a, da, speed, info, big


def rk4_tangent_ref(accel_tangent, x, v, dx, dv, num_steps):
    """(curve, dcurve, velocities, dvelocities) [C, S+1, Q]: the NumPy restatement of models/geodesic.exp_map_tangent;
    accel_tangent: (x, v, dx, dv) [C, Q] -> (a, da) [C, Q]."""
    x, v, dx, dv = (np.array(t, dtype=np.float64) for t in (x, v, dx, dv))
    h = 1.0 / num_steps
    out = [[x], [dx], [v], [dv]]
    for _ in range(num_steps):
        k1x, d1x = v, dv
        k1v, d1v = accel_tangent(x, v, dx, dv)
        k2x, d2x = v + 0.5 * h * k1v, dv + 0.5 * h * d1v
        k2v, d2v = accel_tangent(x + 0.5 * h * k1x, k2x, dx + 0.5 * h * d1x, d2x)
        k3x, d3x = v + 0.5 * h * k2v, dv + 0.5 * h * d2v
        k3v, d3v = accel_tangent(x + 0.5 * h * k2x, k3x, dx + 0.5 * h * d2x, d3x)
        k4x, d4x = v + h * k3v, dv + h * d3v
        k4v, d4v = accel_tangent(x + h * k3x, k4x, dx + h * d3x, d4x)
        x = x + (h / 6.0) * (k1x + 2.0 * k2x + 2.0 * k3x + k4x)
        v = v + (h / 6.0) * (k1v + 2.0 * k2v + 2.0 * k3v + k4v)
        dx = dx + (h / 6.0) * (d1x + 2.0 * d2x + 2.0 * d3x + d4x)
        dv = dv + (h / 6.0) * (d1v + 2.0 * d2v + 2.0 * d3v + d4v)
        for lst, t in zip(out, (x, dx, v, dv)):
            lst.append(t)
    return tuple(np.stack(lst, axis=1) for lst in out)


def newton_ref(accel_tangent, x_from, x_to, num_steps, max_iterations=20, tol=1e-10, init=None):
    """(v [C, Q], residual [C], history): the NumPy restatement of models/geodesic.log_map.  history: one entry per shot,
    dict(residual [C] of the velocity the shot was fired with, accepted [C], frozen [C]: converged before this shot, cond [C] of its Jacobian)."""
    a, b = np.array(x_from, dtype=np.float64), np.array(x_to, dtype=np.float64)
    c, q = a.shape
    v = b - a if init is None else np.array(init, dtype=np.float64)
    bound = tol * np.maximum(1.0, np.linalg.norm(b, axis=1))
    lam, best, history = np.ones(c), None, []
    rep = lambda t: np.repeat(t, q, axis=0)
    for it in range(max_iterations + 1):
        curve, dcurve, _, _ = rk4_tangent_ref(accel_tangent, rep(a), rep(v), np.zeros((c * q, q)), np.tile(np.eye(q), (c, 1)),
                                              num_steps)
        end = curve.reshape(c, q, num_steps + 1, q)[:, 0, -1]
        jac = dcurve.reshape(c, q, num_steps + 1, q)[:, :, -1].transpose(0, 2, 1)
        res = end - b
        norm = np.linalg.norm(res, axis=1)
        step = np.linalg.solve(jac, res[:, :, None])[:, :, 0]
        if best is None:
            ok = np.isfinite(norm)
            assert ok.all()
            best = [v, norm, step]
        else:
            ok = (norm < best[1]) & ~conv
            best = [np.where(ok.reshape((c,) + (1,) * (o.ndim - 1)), n, o) for n, o in zip((v, norm, step), best)]
            lam = np.where(ok, np.minimum(1.0, 2.0 * lam), 0.5 * lam)
        history.append(dict(residual=norm, accepted=ok, frozen=np.zeros(c, dtype=bool) if it == 0 else conv,
                            cond=np.linalg.cond(jac)))
        conv = best[1] <= bound                                                     # (a converged curve is frozen)
        if np.all(conv):
            break
        v = np.where(conv[:, None], best[0], best[0] - lam[:, None] * best[2])
    return best[0], best[1], history


def fixture_accel_tangent(x, v, dx, dv):
    """The fp64 (a, da) of the integrator fixture from the long-double references; asserts the factorisation went through."""
    f = fixture()
    g, _, gam, _ = christoffel_ref(f['z'], x, v, f['gamma'], f['alpha'], f['p'])
    dg, _, dgam, _ = tangent_ref(f['z'], x, v, dx, dv, f['gamma'], f['alpha'], f['p'])
    a, da, _, info, _ = accel_tangent_ref(g, gam, dg, dgam, f['prior'], v)
    assert not info.any()
    return a.astype(np.float64), da.astype(np.float64)


# ---- the case table of the operator: W = 2 Q + 2 across every column-tile edge (Q = 7 | 8, 15 | 16, 23 | 24, 31), M across the
# 64-row slab / chunk edges as a cross with one Q of three tile counts, N around the NP = 8 / 2 / 1 / 1 points per workgroup of
# QT = 1 .. 4, K alternating 1 / 3.
def tangent_tiles(q):
    return (2 * q + 2 + 15) // 16


def points_per_group(q):
    qt = tangent_tiles(q)
    return 8 if qt == 1 else 2 if qt == 2 else 1


def _cases():
    shapes = [(points_per_group(q) + 1, 50, q) for q in (1, 2, 7, 8, 10, 15, 16, 23, 24, 31)]
    shapes += [(points_per_group(q) + 1, m, q) for m in (1, 3, 63, 64, 65, 128, 130) for q in (7, 10, 24)]
    shapes += [(n, 50, 7) for n in (1, 7, 8, 9, 65)] + [(n, 50, 10) for n in (1, 2, 3)]
    shapes += [(n, 50, q) for q in (16, 24, 31) for n in (1, 2)] + [(1, 1, 1)]
    out = []
    for n, m, q in shapes:
        c = dict(K=1 + 2 * (len(out) % 2), N=n, M=m, Q=q)
        if (n, m, q) == (1, 1, 1):
            c['K'] = 1
        if c not in out and dict(c, K=4 - c['K']) not in out:
            out.append(c)
    return out


CASES = _cases()
QT_CASES = {qt: [i for i, c in enumerate(CASES) if tangent_tiles(c['Q']) == qt and c['M'] == 50 and c['K'] == 3][0] for qt in (1, 2, 3, 4)}


def case_id(c):
    return 'K%d-N%d-M%d-Q%d' % (c['K'], c['N'], c['M'], c['Q'])


def tangent_inputs(k, n, m, q, seed):
    """inputs() of the christoffel file plus a direction dx, dv ~ N(0, 1) / sqrt(Q)."""
    inp = dict(inputs(k, n, m, q, seed))
    rng = np.random.default_rng(seed + 50000)
    s = 1.0 / np.sqrt(q)
    inp.update(dx=s * rng.standard_normal((n, q)), dv=s * rng.standard_normal((n, q)))
    for a in inp.values():
        a.setflags(write=False)
    return inp


def run_refs(inp):
    g, g_den, gam, gam_den = christoffel_ref(inp['z'], inp['x'], inp['v'], inp['gamma'], inp['alpha'], inp['p'])
    dg, dg_den, dgam, dgam_den = tangent_ref(inp['z'], inp['x'], inp['v'], inp['dx'], inp['dv'], inp['gamma'], inp['alpha'], inp['p'])
    ref = dict(g=g, g_den=g_den, gam=gam, gam_den=gam_den, dg=dg, dg_den=dg_den, dgam=dgam, dgam_den=dgam_den)
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def case(i):
    """(inputs, references) of CASES[i]: read-only arrays, computed once per process."""
    c = CASES[i]
    inp = tangent_inputs(c['K'], c['N'], c['M'], c['Q'], 9700 + i)
    return inp, run_refs(inp)


@functools.lru_cache(maxsize=None)
def accel_tangent_case(i):
    """accel_case(i) of the christoffel file with random dg, dgam: (inputs, references)."""
    inp, _ = accel_case(i)
    rng = np.random.default_rng(9900 + i)
    inp = dict(inp, dg=rng.standard_normal(inp['g'].shape), dgam=rng.standard_normal(inp['gam'].shape))
    for a in inp.values():
        a.setflags(write=False)
    a, da, speed, info, big = accel_tangent_ref(inp['g'], inp['gam'], inp['dg'], inp['dgam'], inp['prior'], inp['v'])
    return inp, dict(a=a, da=da, speed=speed, info=info, G=big)


# ---- checks of the references ----------------------------------------------------------------------------------------------------
def _sym(inp):
    p = np.asarray(inp['p'])
    return dict(inp, p=0.5 * (p + p.transpose(0, 2, 1)))


SYM_SHAPES = [(1, 3, 20, 3), (2, 3, 20, 5), (1, 2, 70, 17)]


def test_tangent_is_the_central_difference_of_the_christoffel_reference():
    for seed, (k, n, m, q) in enumerate(SYM_SHAPES):
        inp = _sym(tangent_inputs(k, n, m, q, 400 + seed))
        dg, _, dgam, _ = tangent_ref(inp['z'], inp['x'], inp['v'], inp['dx'], inp['dv'], inp['gamma'], inp['alpha'], inp['p'])
        x, v, dx, dv = (np.asarray(inp[t], dtype=LD) for t in ('x', 'v', 'dx', 'dv'))
        h = LD(1e-5)
        at = lambda s: christoffel_ref(inp['z'], x + s * dx, v + s * dv, inp['gamma'], inp['alpha'], inp['p'])
        (gp, _, gamp, _), (gm, _, gamm, _) = at(h), at(-h)
        fd_g, fd_gam = (gp - gm) / (2 * h), (gamp - gamm) / (2 * h)
        eg, sg = float(np.max(np.abs(dg - fd_g))), float(np.max(np.abs(fd_g)))
        egam, sgam = float(np.max(np.abs(dgam - fd_gam))), float(np.max(np.abs(fd_gam)))
        print('K%d N%d M%d Q%d: |dg - FD| %.2e of %.2e, |dgam - FD| %.2e of %.2e' % (k, n, m, q, eg, sg, egam, sgam))
        assert sg > 1e-3 and sgam > 1e-3 and eg <= 1e-5 * sg and egam <= 1e-5 * sgam


def test_dg_is_symmetric_for_a_symmetric_p():
    for seed, (k, n, m, q) in enumerate(SYM_SHAPES):
        inp = _sym(tangent_inputs(k, n, m, q, 400 + seed))
        dg = tangent_ref(inp['z'], inp['x'], inp['v'], inp['dx'], inp['dv'], inp['gamma'], inp['alpha'], inp['p'])[0]
        assert np.max(np.abs(dg - dg.transpose(0, 1, 3, 2))) <= 1e-16 * np.max(np.abs(dg))
    inp = tangent_inputs(1, 3, 20, 3, 400)                                         # and not for the non-symmetric p of the table
    dg = tangent_ref(inp['z'], inp['x'], inp['v'], inp['dx'], inp['dv'], inp['gamma'], inp['alpha'], inp['p'])[0]
    assert np.max(np.abs(dg - dg.transpose(0, 1, 3, 2))) > 1e-3 * np.max(np.abs(dg))


def test_tangent_is_linear_in_the_direction_and_zero_for_a_zero_direction():
    inp = tangent_inputs(2, 3, 20, 5, 410)
    run = lambda dx, dv: tangent_ref(inp['z'], inp['x'], inp['v'], dx, dv, inp['gamma'], inp['alpha'], inp['p'])
    rng = np.random.default_rng(5)
    dx2, dv2 = rng.standard_normal(inp['dx'].shape), rng.standard_normal(inp['dv'].shape)
    one, two = run(inp['dx'], inp['dv']), run(dx2, dv2)
    both = run(LD(2.5) * np.asarray(inp['dx'], dtype=LD) - dx2, LD(2.5) * np.asarray(inp['dv'], dtype=LD) - dv2)
    for j in (0, 2):
        want = LD(2.5) * one[j] - two[j]
        assert np.max(np.abs(both[j] - want)) <= 1e-15 * np.max(np.abs(want))
    zero = run(np.zeros_like(dx2), np.zeros_like(dv2))
    assert all(np.all(t == 0) for t in zero)


def test_accel_tangent_reference_solves_its_system():
    for i in range(len(ACCEL_CASES)):
        inp, ref = accel_tangent_case(i)
        _, plain = accel_case(i)
        assert np.array_equal(ref['a'], plain['a']) and not ref['info'].any()
        rhs = np.sum(np.asarray(inp['dgam'], dtype=LD), axis=0) + np.einsum('nqr,nr->nq', np.sum(np.asarray(inp['dg'], dtype=LD), axis=0),
                                                                               ref['a'])
        res = np.einsum('nqr,nr->nq', ref['G'], ref['da']) + rhs
        assert np.max(np.abs(res)) <= 1e-15 * np.max(np.abs(rhs)) * MAX_COND, accel_case_id(ACCEL_CASES[i])


def test_accel_tangent_is_the_central_difference_of_the_acceleration():
    """On the integrator fixture: da against (a(x + h dx, v + h dv) - a(x - h dx, v - h dv)) / 2 h."""
    f = fixture()
    rng = np.random.default_rng(3)
    x, v = np.asarray(f['x']), np.asarray(f['v'])
    dx, dv = rng.standard_normal(x.shape), rng.standard_normal(v.shape)
    _, da = fixture_accel_tangent(x, v, dx, dv)
    h = 1e-5
    fd = (fixture_accel(x + h * dx, v + h * dv) - fixture_accel(x - h * dx, v - h * dv)) / (2 * h)
    err, scale = np.max(np.abs(da - fd)), np.max(np.abs(fd))
    print('|da - FD| %.2e of %.2e' % (err, scale))
    assert scale > 1e-2 and err <= 1e-7 * scale


def test_tangent_rk4_is_the_central_difference_of_the_integrator():
    f = fixture()
    rng = np.random.default_rng(4)
    x, v = np.asarray(f['x']), np.asarray(f['v'])
    dx, dv = rng.standard_normal(x.shape), rng.standard_normal(v.shape)
    curve, dcurve, vel, dvel = rk4_tangent_ref(fixture_accel_tangent, x, v, dx, dv, 16)
    plain = rk4_ref(fixture_accel, x, v, 16)
    assert np.array_equal(curve, plain[0]) and np.array_equal(vel, plain[1])
    h = 1e-5
    (cp, vp), (cm, vm) = rk4_ref(fixture_accel, x + h * dx, v + h * dv, 16), rk4_ref(fixture_accel, x - h * dx, v - h * dv, 16)
    for name, got, fd in (('dcurve', dcurve, (cp - cm) / (2 * h)), ('dvelocity', dvel, (vp - vm) / (2 * h))):
        err, scale = np.max(np.abs(got - fd)), np.max(np.abs(fd))
        print('%s: |tangent - FD| %.2e of %.2e' % (name, err, scale))
        assert scale > 0.5 and err <= 1e-7 * scale


@functools.lru_cache(maxsize=None)
def fixture_targets(num_steps=16):
    """(y, v0): the ends y = exp_x(v0) of the fixture's curves at num_steps steps, the targets of the shooting tests."""
    f = fixture()
    curve, _ = rk4_ref(fixture_accel, np.asarray(f['x']), np.asarray(f['v']), num_steps)
    return curve[:, -1].copy(), np.asarray(f['v'])


def test_newton_shooting_converges_quadratically_on_the_fixture():
    f = fixture()
    x = np.asarray(f['x'])
    y, v0 = fixture_targets()
    off = np.linalg.norm(y - (x + v0), axis=1)
    print('ends off the straight ends by', off)
    assert off.min() > 0.01 and off.max() < 0.5
    v, res, hist = newton_ref(fixture_accel_tangent, x, y, 16)
    updates = len(hist) - 1
    r = np.stack([h['residual'] for h in hist])                                    # [shots, C]
    print('residuals per shot (worst curve):', r.max(axis=1), 'updates', updates)
    assert updates <= 3 and np.all(res <= 1e-10)
    assert all((h['accepted'] | h['frozen']).all() for h in hist)
    rel = np.linalg.norm(v - v0, axis=1) / np.linalg.norm(v0, axis=1)
    print('|v - v0| / |v0|', rel.max())
    assert rel.max() <= 1e-9
    floor = 1e-14                                                                   # (below it a residual is rounding, not Newton)
    live = ~np.stack([h['frozen'] for h in hist])                                  # (a frozen curve repeats its residual)
    const = max(float(np.max((r[i + 1] / np.maximum(r[i] ** 2, floor))[live[i + 1]])) for i in range(len(r) - 1))
    print('residual_{i+1} <= %.3f residual_i^2' % const)
    assert const <= 1.0                                                             # (quadratic: measured 0.072)
    cond = max(float(h['cond'].max()) for h in hist)
    print('cond(J) <= %.3f' % cond)
    assert cond <= 2.0


def test_case_tables_cover_the_edges_and_are_alive():
    assert {1, 2, 7, 8, 10, 15, 16, 23, 24, 31} <= {c['Q'] for c in CASES if c['M'] == 50 and c['N'] == points_per_group(c['Q']) + 1}
    for q in (7, 10, 24):
        assert {1, 3, 63, 64, 65, 128, 130} <= {c['M'] for c in CASES if c['Q'] == q}
    for q, ns in ((7, {1, 7, 8, 9, 65}), (10, {1, 2, 3}), (16, {1, 2}), (24, {1, 2}), (31, {1, 2})):
        assert ns <= {c['N'] for c in CASES if c['Q'] == q and c['M'] == 50}, q
    assert dict(K=1, N=1, M=1, Q=1) in CASES and {1, 3} <= {c['K'] for c in CASES}
    assert sorted(QT_CASES) == [1, 2, 3, 4]
    alive = 0
    for i in range(len(CASES)):
        _, ref = case(i)
        assert all(np.all(np.isfinite(a)) for a in ref.values()), case_id(CASES[i])
        alive += float(np.max(np.abs(ref['dg']))) > 1e-6 and float(np.max(np.abs(ref['dgam']))) > 1e-6
    assert alive >= 0.9 * len(CASES), (alive, len(CASES))
