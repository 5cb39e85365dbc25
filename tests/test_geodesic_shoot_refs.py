"""CPU tests (no GPU) of the data flow of the integrators on the device (csrc/geodesic_accel.hip: gs_kernel, behind
ops.geodesic_shoot / ops.geodesic_shoot_tangent): a NumPy mirror of what the stage kernel keeps between its launches (the next
stage's arguments in two alternating buffers, the running sums k1 + 2 k2 + 2 k3 + k4, the stage-4 row that is the next step's base)
gives the BITS of models/geodesic._rk4 / _rk4_tangent on the same acceleration, so the staging changes nothing and the kernel has
an order to follow; and the case tables that tests/test_gpu_geodesic_shoot.py runs, with their np.longdouble references and the
condition numbers of every metric met along them."""
import functools

import numpy as np
import pytest
import torch

from dp_gp_lvm_amd.models import geodesic
from test_point_christoffel_refs import MAX_COND, accel_ref, christoffel_ref, fixture, fixture_accel, rk4_ref
from test_point_tangent_refs import accel_tangent_ref, fixture_accel_tangent, rk4_tangent_ref, tangent_ref

STEPS = (1, 2, 16)


# ---- the mirror of the staged data flow ------------------------------------------------------------------------------------------
def staged_shoot(accel, x, v, num_steps, accel_tangent=None, dx=None, dv=None):
    """(rows of x, v[, dx, dv] [C, S+1, Q], launches): what 4 S launches of the stage kernel leave behind.  accel: (x, v) -> a, or
    with accel_tangent (x, v, dx, dv) -> (a, da) the tangent's four states.  Every product is rounded before its add (NumPy does
    no contraction); h, h/2 and h/6 are formed once in double, as the C call forms them."""
    tangent = accel_tangent is not None
    start = [np.array(t, dtype=np.float64) for t in ((x, v, dx, dv) if tangent else (x, v))]
    n = len(start)
    c, q = start[0].shape
    h = 1.0 / num_steps
    c_half, c_row = 0.5 * h, h / 6.0
    rows = [np.full((c, num_steps + 1, q), np.nan) for _ in range(n)]
    args = np.full((2, n, c, q), np.nan)                       # the two argument buffers: launch L reads (L - 1) & 1, writes L & 1
    sums = np.full((n, c, q), np.nan)
    launches = 0
    for launch in range(4 * num_steps):
        step, stage = launch // 4, launch % 4 + 1
        first = launch == 0
        arg_in = start if first else list(args[(launch - 1) & 1])
        out = args[launch & 1]
        if tangent:
            a, da = accel_tangent(*arg_in)
            ks = (arg_in[1], a, arg_in[3], da)                 # k_x = the stage's velocity argument, k_v = a; the same for (dx, dv)
        else:
            ks = (arg_in[1], accel(*arg_in))
        launches += 1
        for j, kk in enumerate(ks):
            base = start[j] if first else rows[j][:, step]
            if first:
                rows[j][:, 0] = base
            total = kk if stage == 1 else sums[j] + kk if stage == 4 else sums[j] + 2.0 * kk
            if stage < 4:
                sums[j] = total
                out[j] = base + (h if stage == 3 else c_half) * kk
            else:
                nxt = base + c_row * total
                rows[j][:, step + 1] = nxt
                out[j] = nxt
    return rows, launches


def _torch_accel(fn):
    """fn, a NumPy acceleration, as models/geodesic.py's callable on CPU tensors."""
    def accel(x, v):
        a = torch.as_tensor(fn(x.numpy(), v.numpy()))
        return a, torch.zeros(x.shape[0], dtype=torch.float64), torch.zeros(x.shape[0], dtype=torch.int32)
    return accel


def _torch_accel_tangent(fn):
    def accel_tangent(x, v, dx, dv):
        a, da = (torch.as_tensor(t) for t in fn(x.numpy(), v.numpy(), dx.numpy(), dv.numpy()))
        return a, da, torch.zeros(x.shape[0], dtype=torch.float64), torch.zeros(x.shape[0], dtype=torch.int32)
    return accel_tangent


def _fixture_direction():
    rng = np.random.default_rng(78)
    return 0.5 * rng.standard_normal((4, 3)), 0.5 * rng.standard_normal((4, 3))


@pytest.mark.parametrize('steps', STEPS)
def test_the_staged_flow_gives_the_bits_of_the_host_exponential_map(steps):
    f = fixture()
    x, v = np.array(f['x']), np.array(f['v'])
    (curve, vel), launches = staged_shoot(fixture_accel, x, v, steps)
    want_c, want_v = geodesic.exp_map(_torch_accel(fixture_accel), x, v, 3, 'cpu', steps, return_velocity=True)
    assert launches == 4 * steps
    assert torch.equal(torch.as_tensor(curve), want_c) and torch.equal(torch.as_tensor(vel), want_v)
    assert np.array_equal(curve[:, 0], x) and np.array_equal(vel[:, 0], v)                  # row 0: the bits of the inputs
    ref_c, ref_v = rk4_ref(fixture_accel, x, v, steps)                                      # (0.5 * h * k there: another order)
    assert np.max(np.abs(curve - ref_c)) <= 1e-14 * np.max(np.abs(ref_c)) and np.max(np.abs(vel - ref_v)) <= 1e-14 * np.max(np.abs(ref_v))
    assert np.max(np.abs(curve[:, -1] - (x + v))) > 1e-4                                    # (the curves bend)


@pytest.mark.parametrize('steps', STEPS)
def test_the_staged_flow_gives_the_bits_of_the_host_tangent_integrator(steps):
    f = fixture()
    x, v = np.array(f['x']), np.array(f['v'])
    dx, dv = _fixture_direction()
    rows, launches = staged_shoot(None, x, v, steps, fixture_accel_tangent, dx, dv)
    t = lambda a: torch.as_tensor(np.array(a, dtype=np.float64))
    want = geodesic._rk4_tangent(_torch_accel_tangent(fixture_accel_tangent), t(x), t(v), t(dx), t(dv), steps)
    assert launches == 4 * steps
    for have, w, start in zip(rows, want[:4], (x, v, dx, dv)):
        assert torch.equal(torch.as_tensor(have), w)
        assert np.array_equal(have[:, 0], start)
    plain, _ = staged_shoot(fixture_accel, x, v, steps)
    assert np.array_equal(plain[0], rows[0]) and np.array_equal(plain[1], rows[1])           # the tangent leaves the curve's bits alone
    ref = rk4_tangent_ref(fixture_accel_tangent, x, v, dx, dv, steps)                        # (curve, dcurve, velocities, dvelocities)
    for have, r in zip((rows[0], rows[2], rows[1], rows[3]), ref):
        assert np.max(np.abs(have - r)) <= 1e-14 * max(1.0, np.max(np.abs(r)))


def test_a_failed_stage_is_counted_and_stays_in_its_curve():
    """The host loop's rule that the kernel keeps: a stage that fails returns NaN for its curve, which every later stage of that
    curve inherits (its metric is NaN: it fails too), and the other curves do not see it."""
    f = fixture()
    x, v = np.array(f['x']), np.array(f['v'])

    def failing(xx, vv):
        a = fixture_accel(np.where(np.isfinite(xx), xx, 0.0), np.where(np.isfinite(vv), vv, 0.0))
        a[~np.isfinite(xx).all(axis=1) | ~np.isfinite(vv).all(axis=1)] = np.nan
        if np.array_equal(xx[1], x[1]):                        # curve 1 fails at its very first stage
            a[1] = np.nan
        return a

    (curve, vel), _ = staged_shoot(failing, x, v, 2)
    (good, good_v), _ = staged_shoot(fixture_accel, x, v, 2)
    keep = [0, 2, 3]
    assert np.array_equal(curve[keep], good[keep]) and np.array_equal(vel[keep], good_v[keep])
    assert np.array_equal(curve[1, 0], x[1]) and np.isnan(curve[1, 1:]).all() and np.isnan(vel[1, 1:]).all()


# ---- the case tables of tests/test_gpu_geodesic_shoot.py -------------------------------------------------------------------------
# A row: Q, the parts' (K_i, M_i), C curves, S steps.  Between them the rows meet Q at the edges of the christoffel kernel's column
# tiles (W = Q + 1: 15 | 16; tangent W = 2 Q + 2: 15 | 31) and of the two operators' limits (63, 31), sum K = 1, 8, 9, 17 (the slab
# sum takes one load, then eight at a time, then singly), C = 1, 7, 8, 9 (8 points per workgroup of the christoffel kernel at one
# column tile), S = 1, 2, 16, M = 1, 9, 65 (one slab of 64 inducing points, and two), one part and two parts of unlike (K, M).
def _row(q, parts, c, s):
    return dict(Q=q, parts=tuple(parts), C=c, S=s)


PLAIN = [_row(1, [(1, 9)], 1, 1), _row(3, [(8, 9)], 7, 2), _row(3, [(5, 9), (4, 65)], 9, 16), _row(10, [(9, 9), (8, 1)], 8, 2),
         _row(10, [(1, 65)], 9, 16), _row(15, [(8, 1)], 8, 1), _row(15, [(17, 9)], 9, 2), _row(16, [(1, 9), (8, 9)], 7, 2),
         _row(63, [(1, 9)], 1, 2), _row(63, [(1, 1), (8, 9)], 2, 1)]
TANGENT = [_row(1, [(1, 9)], 1, 1), _row(3, [(8, 9)], 7, 2), _row(3, [(5, 9), (4, 65)], 9, 16), _row(10, [(9, 9), (8, 1)], 8, 2),
           _row(10, [(1, 65)], 9, 16), _row(15, [(17, 1)], 8, 1), _row(15, [(1, 9), (8, 9)], 7, 2), _row(31, [(1, 9)], 1, 2),
           _row(31, [(1, 1), (8, 9)], 2, 1)]


def row_id(r):
    return 'Q%d-%s-C%d-S%d' % (r['Q'], '+'.join('K%dM%d' % km for km in r['parts']), r['C'], r['S'])


def shoot_inputs(row, seed, tangent=False):
    """The parts (z, gamma, alpha, p), prior and states of a row: inducing inputs within about two length scales of the curves at
    every Q, symmetric INDEFINITE p scaled so that the data term moves G by a fraction of the prior's few units."""
    rng = np.random.default_rng(seed)
    q, c = row['Q'], row['C']
    ktot = sum(k for k, _ in row['parts'])
    s = 1.0 / np.sqrt(q)
    parts = []
    for k, m in row['parts']:
        a = rng.standard_normal((k, m, m))
        parts.append(dict(z=1.5 * s * rng.standard_normal((k, m, q)), gamma=rng.uniform(0.5, 1.5, (k, q)), alpha=rng.uniform(0.8, 1.2, k),
                          p=0.15 * (20.0 / max(m, 10)) / np.sqrt(ktot) * (a + a.transpose(0, 2, 1))))
    inp = dict(parts=parts, prior=rng.uniform(4.0, 6.0, q), x=0.5 * s * rng.standard_normal((c, q)), v=s * rng.standard_normal((c, q)))
    if tangent:
        inp.update(dx=0.5 * s * rng.standard_normal((c, q)), dv=0.5 * s * rng.standard_normal((c, q)))
    for t in [inp[n] for n in inp if n != 'parts'] + [a for pt in parts for a in pt.values()]:
        t.setflags(write=False)
    return inp


def _slabs(fn, parts, *state):
    """fn(z, *state, gamma, alpha, p)'s results at even places (the odd ones are the tolerances' denominators) of every part,
    concatenated over the kernels in part order."""
    each = [fn(pt['z'], *state, pt['gamma'], pt['alpha'], pt['p'])[::2] for pt in parts]
    return [np.concatenate(ts) for ts in zip(*each)]


@functools.lru_cache(maxsize=None)
def plain_case(i):
    """(inputs, the np.longdouble-accelerated RK4 (curve, vel), the largest condition number of a metric met)."""
    row = PLAIN[i]
    inp = shoot_inputs(row, 9300 + i)
    conds = []

    def accel(x, v):
        g, gam = _slabs(christoffel_ref, inp['parts'], x, v)
        a, _, info, big = accel_ref(g, gam, inp['prior'], v)
        assert not info.any()
        conds.append(np.linalg.cond(np.asarray(big, dtype=np.float64)).max())
        return a.astype(np.float64)

    curve, vel = rk4_ref(accel, inp['x'], inp['v'], row['S'])
    return inp, (curve, vel), max(conds)


@functools.lru_cache(maxsize=None)
def tangent_case(i):
    """(inputs, the reference (curve, dcurve, vel, dvel), the largest condition number met)."""
    row = TANGENT[i]
    inp = shoot_inputs(row, 9400 + i, tangent=True)
    conds = []

    def accel_tangent(x, v, dx, dv):
        g, gam = _slabs(christoffel_ref, inp['parts'], x, v)
        dg, dgam = _slabs(tangent_ref, inp['parts'], x, v, dx, dv)
        a, da, _, info, big = accel_tangent_ref(g, gam, dg, dgam, inp['prior'], v)
        assert not info.any()
        conds.append(np.linalg.cond(np.asarray(big, dtype=np.float64)).max())
        return a.astype(np.float64), da.astype(np.float64)

    ref = rk4_tangent_ref(accel_tangent, inp['x'], inp['v'], inp['dx'], inp['dv'], row['S'])
    return inp, ref, max(conds)


def test_case_tables_cover_the_edges():
    for table, qs in ((PLAIN, {1, 3, 10, 15, 16, 63}), (TANGENT, {1, 3, 10, 15, 31})):
        assert {r['Q'] for r in table} == qs
        assert {1, 8, 9, 17} <= {sum(k for k, _ in r['parts']) for r in table}
        assert {1, 7, 8, 9} <= {r['C'] for r in table}
        assert {1, 2, 16} == {r['S'] for r in table}
        assert {1, 9, 65} <= {m for r in table for _, m in r['parts']}
        assert {1, 2} == {len(r['parts']) for r in table}
        assert any(len({km for km in r['parts']}) == 2 and r['parts'][0][0] != r['parts'][1][0] and r['parts'][0][1] != r['parts'][1][1]
                   for r in table)


@pytest.mark.parametrize('i', range(len(PLAIN)), ids=[row_id(r) for r in PLAIN])
def test_plain_rows_are_well_conditioned_and_alive(i):
    inp, (curve, vel), cond = plain_case(i)
    bend = float(np.max(np.abs(curve[:, -1] - (inp['x'] + inp['v']))))
    print('%s: condition number <= %.1f, end off the straight end by %.3e' % (row_id(PLAIN[i]), cond, bend))
    assert cond <= MAX_COND and np.all(np.isfinite(curve)) and np.all(np.isfinite(vel))
    assert bend > 1e-6


@pytest.mark.parametrize('i', range(len(TANGENT)), ids=[row_id(r) for r in TANGENT])
def test_tangent_rows_are_well_conditioned_and_alive(i):
    inp, (curve, dcurve, vel, dvel), cond = tangent_case(i)
    straight = inp['dx'] + inp['dv']
    bend = float(np.max(np.abs(dcurve[:, -1] - straight)))
    print('%s: condition number <= %.1f, end tangent off the straight one by %.3e' % (row_id(TANGENT[i]), cond, bend))
    assert cond <= MAX_COND and all(np.all(np.isfinite(t)) for t in (curve, dcurve, vel, dvel))
    assert bend > 1e-6
