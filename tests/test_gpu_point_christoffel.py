"""GPU tests of ops.ard_rbf_point_christoffel (csrc/ard_rbf_point_metric.hip) and ops.geodesic_accel (csrc/geodesic_accel.hip)
against the np.longdouble references and the case tables of tests/test_point_christoffel_refs.py: random indefinite NON-symmetric p, z, x, v ~ N(0, 1) /
sqrt(Q), gamma in [0.2, 3].  Tolerances: 1e-12 relative to the sum of the absolute values of each entry's terms for g and gam (the
sibling operators' bound); 1e-9 of max |a| for the acceleration, on matrices whose condition number the CPU file bounds by 1e4
(the backward error of a Cholesky solve, a few Q eps cond = 63 * 1.1e-16 * 1e4 * small ~ 1e-10 at the worst case here)."""
import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import ops
from test_point_christoffel_refs import (ACCEL_CASES, BASE, CASES, WIDE, accel_case, accel_case_id, accel_ref, case, case_id,
                                         points_per_group)

pytestmark = pytest.mark.gpu
TOL, TOL_A = 1e-12, 1e-9
LD = np.longdouble


def dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64), device='cuda')


def run(inp):
    return ops.ard_rbf_point_christoffel(dev(inp['z']), dev(inp['x']), dev(inp['v']), dev(inp['gamma']), dev(inp['alpha']),
                                         dev(inp['p']))


def finish(inp):
    return ops.geodesic_accel(dev(inp['g']), dev(inp['gam']), dev(inp['prior']), dev(inp['v']))


def worst(got, ref, den):
    """max over the entries of |got - ref| / sum |terms| (entries whose terms all vanish must be exact zeros)."""
    got = got.cpu().numpy().astype(LD)
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    assert np.all(err[den == 0] == 0)
    return float(np.max(np.where(den > 0, err / np.where(den > 0, den, 1), 0)))


@pytest.mark.parametrize('i', range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_operator_against_the_longdouble_reference(i):
    inp, ref = case(i)
    c = CASES[i]
    g, gam = run(inp)
    assert tuple(g.shape) == (c['K'], c['N'], c['Q'], c['Q']) and tuple(gam.shape) == (c['K'], c['N'], c['Q'])
    assert g.dtype == torch.float64 and gam.dtype == torch.float64
    ratios = worst(g, ref['g'], ref['g_den']), worst(gam, ref['gam'], ref['gam_den'])
    print('%s: g %.2e, gam %.2e of sum |terms|' % ((case_id(c),) + ratios))
    assert max(ratios) <= TOL, ratios


@pytest.mark.parametrize('i', range(11), ids=[case_id(c) for c in CASES[:11]])
def test_g_is_the_metric_operator(i):
    """g within the tolerance of the metric operator's result, and equal to it bit for bit.  The equality holds by construction:
    both operators are instantiations of one kernel (csrc/ard_rbf_point_metric.hip), the feature and exponent expressions are
    the same source lines, and the summation order of an entry does not depend on the tile count QT, so it holds whether or not
    the d column costs a tile (Q = 15 against Q = 16 in the case table)."""
    inp, ref = case(i)
    g, _ = run(inp)
    want = ops.ard_rbf_point_metric(dev(inp['z']), dev(inp['x']), dev(inp['gamma']), dev(inp['alpha']), dev(inp['p']))
    ratio = float(np.max(np.abs((g - want).cpu().numpy()) / np.asarray(ref['g_den'], dtype=np.float64)))
    print('%s: |g - metric operator| %.2e of sum |terms|' % (case_id(CASES[i]), ratio))
    assert ratio <= TOL
    assert torch.equal(g, want)


@pytest.mark.parametrize('i', [BASE, WIDE], ids=lambda i: case_id(CASES[i]))
def test_far_away_points_give_exact_zeros_and_a_zero_acceleration(i):
    inp, _ = case(i)
    x, v = np.asarray(inp['x']), np.asarray(inp['v'])
    far = dict(inp, x=x + 100.0)                                         # 100 units from every z: every exponential underflows
    g, gam = run(far)
    assert torch.all(g == 0) and torch.all(gam == 0)                     # (no NaN: NaN == 0 is False)
    prior = torch.ones(x.shape[1], dtype=torch.float64, device='cuda')
    a, speed, info = ops.geodesic_accel(g, gam, prior, dev(v))
    assert torch.all(a == 0) and torch.all(info == 0)
    assert float((speed - dev(v * v).sum(1)).abs().max()) <= 1e-14 * float(speed.max())        # G is the prior alone
    mixed = dict(inp, x=np.concatenate([x[:1], x[1:] + 100.0]))
    for o2, o1 in zip(run(mixed), run(inp)):
        assert torch.all(o2[:, 1:] == 0) and torch.isfinite(o2).all() and o2[:, :1].abs().max() > 0
        assert torch.equal(o2[:, :1], o1[:, :1])


@pytest.mark.parametrize('i', [BASE, WIDE], ids=lambda i: case_id(CASES[i]))
def test_two_runs_give_the_same_bits(i):
    inp, _ = case(i)
    for a, b in zip(run(inp), run(inp)):
        assert torch.equal(a, b)


@pytest.mark.parametrize('i', [BASE, WIDE], ids=lambda i: case_id(CASES[i]))
def test_three_kernels_equal_three_single_kernel_calls(i):
    inp, _ = case(i)
    assert CASES[i]['K'] == 3
    out = run(inp)
    for k in range(3):
        one = {name: (a if name in ('x', 'v') else np.asarray(a)[k:k + 1]) for name, a in inp.items()}
        for ok, o in zip(run(one), out):
            assert torch.equal(ok[0], o[k]), k


@pytest.mark.parametrize('q', [10, 16, 32, 63])
def test_a_points_bits_do_not_depend_on_n_or_on_its_place_in_x(q):
    i = [j for j, c in enumerate(CASES) if c['Q'] == q and c['M'] == 50][0]
    inp, _ = case(i)
    npg = points_per_group(q)
    rng = np.random.default_rng(q)
    n = 3 * npg + 2
    x, v = rng.standard_normal((n, q)) / np.sqrt(q), rng.standard_normal((n, q)) / np.sqrt(q)
    whole = run(dict(inp, x=x, v=v))
    for pick in (np.arange(1), np.arange(n - 1, n), np.arange(1, n), np.arange(n - 1, -1, -1), np.array([n - 1, 0, 0, npg, npg - 1])):
        part = run(dict(inp, x=x[pick], v=v[pick]))
        at = torch.as_tensor(pick, device='cuda')
        for o, w in zip(part, whole):
            assert torch.equal(o, w.index_select(1, at)), pick[:4]


# ---- the finishing operator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(ACCEL_CASES)), ids=[accel_case_id(c) for c in ACCEL_CASES])
def test_acceleration_against_the_longdouble_reference(i):
    inp, ref = accel_case(i)
    c = ACCEL_CASES[i]
    a, speed, info = finish(inp)
    assert tuple(a.shape) == (c['N'], c['Q']) and tuple(speed.shape) == (c['N'],) and tuple(info.shape) == (c['N'],)
    assert a.dtype == torch.float64 and info.dtype == torch.int32 and torch.all(info == 0)
    err_a = float(np.max(np.abs(a.cpu().numpy().astype(LD) - ref['a'])) / np.max(np.abs(ref['a'])))
    v = np.abs(np.asarray(inp['v'], dtype=LD))
    terms = np.einsum('nq,nqr,nr->n', v, np.sum(np.abs(np.asarray(inp['g'], dtype=LD)), axis=0) + np.diag(inp['prior'])[None], v)
    err_s = float(np.max(np.abs(speed.cpu().numpy().astype(LD) - ref['speed']) / terms))
    print('%s: a %.2e of max |a|, speed %.2e of sum |terms|' % (accel_case_id(c), err_a, err_s))
    assert err_a <= TOL_A and err_s <= TOL
    for one, two in zip(finish(inp), (a, speed, info)):
        assert torch.equal(one, two)                                     # the same bits on a second run


@pytest.mark.parametrize('i', [3, 6], ids=lambda i: accel_case_id(ACCEL_CASES[i]))
def test_an_indefinite_matrix_fails_alone(i):
    inp, ref = accel_case(i)
    c = ACCEL_CASES[i]
    n_bad, pivot = c['N'] // 2, (c['Q'] + 1) // 2                         # 1-based: the pivot that goes negative
    g = np.array(inp['g'])
    g[0, n_bad, pivot - 1, pivot - 1] -= 1e3
    assert accel_ref(g, inp['gam'], inp['prior'], inp['v'])[2][n_bad] == pivot
    good = finish(inp)
    a, speed, info = finish(dict(inp, g=g))
    keep = torch.as_tensor([j for j in range(c['N']) if j != n_bad], device='cuda')
    assert int(info[n_bad]) == pivot and torch.all(torch.isnan(a[n_bad]))
    assert torch.all(info.index_select(0, keep) == 0)
    assert torch.equal(a.index_select(0, keep), good[0].index_select(0, keep))
    assert torch.equal(speed.index_select(0, keep), good[1].index_select(0, keep))
    assert torch.isfinite(speed).all()


def test_the_pair_gives_the_acceleration_of_the_reference_chain():
    """Both operators in a row, K = 3 kernels: a = -G^-1 sum_k gam_k against the long-double chain of the two references."""
    inp, ref = case(BASE)
    p = np.asarray(inp['p'])
    sym = dict(inp, p=0.05 * (p + p.transpose(0, 2, 1)))
    prior = np.full(CASES[BASE]['Q'], 40.0)
    g, gam = run(sym)
    a, speed, info = ops.geodesic_accel(g, gam, dev(prior), dev(sym['v']))
    from test_point_christoffel_refs import MAX_COND, christoffel_ref
    rg, _, rgam, _ = christoffel_ref(sym['z'], sym['x'], sym['v'], sym['gamma'], sym['alpha'], sym['p'])
    ra, rspeed, rinfo, big = accel_ref(rg, rgam, prior, sym['v'])
    assert not rinfo.any() and torch.all(info == 0) and np.linalg.cond(big.astype(np.float64)).max() <= MAX_COND
    err = float(np.max(np.abs(a.cpu().numpy().astype(LD) - ra)) / np.max(np.abs(ra)))
    print('chain: a %.2e of max |a| = %.2e' % (err, float(np.max(np.abs(ra)))))
    assert err <= TOL_A and float(np.max(np.abs(ra))) > 1e-3
