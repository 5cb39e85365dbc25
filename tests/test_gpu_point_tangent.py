"""GPU tests of ops.ard_rbf_point_christoffel_tangent (csrc/ard_rbf_point_metric.hip, the tangent mode of mt_kernel) and
ops.geodesic_accel_tangent (csrc/geodesic_accel.hip) against the np.longdouble references and the case tables of
tests/test_point_tangent_refs.py: random indefinite NON-symmetric p, z, x, v, dx, dv ~ N(0, 1) / sqrt(Q), gamma in [0.2, 3].
Tolerances: 1e-12 relative to the sum of the absolute values of each entry's terms for g, gam, dg and dgam (the sibling operators'
bound); 1e-9 of max |da| for the acceleration's tangent, on matrices whose condition number the CPU file bounds by 1e4 (two
Cholesky solves in a row: a few Q eps cond each).  g, gam and a, speed, info carry the bits of the operators they extend."""
import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import ops
from test_point_christoffel_refs import ACCEL_CASES, accel_case_id, accel_ref
from test_point_tangent_refs import CASES, QT_CASES, accel_tangent_case, case, case_id, points_per_group, tangent_tiles

pytestmark = pytest.mark.gpu
TOL, TOL_A = 1e-12, 1e-9
LD = np.longdouble
NAMES = ('g', 'gam', 'dg', 'dgam')


def dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64), device='cuda')


def run(inp):
    return ops.ard_rbf_point_christoffel_tangent(dev(inp['z']), dev(inp['x']), dev(inp['v']), dev(inp['dx']), dev(inp['dv']),
                                                 dev(inp['gamma']), dev(inp['alpha']), dev(inp['p']))


def plain(inp):
    return ops.ard_rbf_point_christoffel(dev(inp['z']), dev(inp['x']), dev(inp['v']), dev(inp['gamma']), dev(inp['alpha']),
                                         dev(inp['p']))


def finish(inp):
    return ops.geodesic_accel_tangent(dev(inp['g']), dev(inp['gam']), dev(inp['dg']), dev(inp['dgam']), dev(inp['prior']),
                                      dev(inp['v']))


def worst(got, ref, den):
    """max over the entries of |got - ref| / sum |terms| (entries whose terms all vanish must be exact zeros)."""
    got = got.cpu().numpy().astype(LD)
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    assert np.all(err[den == 0] == 0)
    return float(np.max(np.where(den > 0, err / np.where(den > 0, den, 1), 0)))


@pytest.mark.parametrize('i', range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_operator_against_the_longdouble_reference_and_the_christoffel_operator(i):
    inp, ref = case(i)
    c = CASES[i]
    out = run(inp)
    for name, o in zip(NAMES, out):
        assert tuple(o.shape) == (c['K'], c['N']) + (c['Q'],) * (2 if name.endswith('g') else 1) and o.dtype == torch.float64
    ratios = tuple(worst(o, ref[name], ref[name + '_den']) for name, o in zip(NAMES, out))
    print('%s: g %.2e, gam %.2e, dg %.2e, dgam %.2e of sum |terms|' % ((case_id(c),) + ratios))
    assert max(ratios) <= TOL, ratios
    g, gam = plain(inp)
    assert torch.equal(out[0], g) and torch.equal(out[1], gam)           # the christoffel operator's bits, whatever QT and W


@pytest.mark.parametrize('qt', sorted(QT_CASES))
def test_zero_directions_and_far_away_points_give_exact_zeros(qt):
    inp, _ = case(QT_CASES[qt])
    x = np.asarray(inp['x'])
    zero = run(dict(inp, dx=np.zeros_like(x), dv=np.zeros_like(x)))
    assert torch.all(zero[2] == 0) and torch.all(zero[3] == 0)            # (no NaN: NaN == 0 is False)
    assert zero[0].abs().max() > 0 and zero[1].abs().max() > 0
    far = run(dict(inp, x=x + 100.0))                                     # 100 units from every z: every exponential underflows
    assert all(torch.all(o == 0) for o in far)
    mixed, whole = run(dict(inp, x=np.concatenate([x[:1], x[1:] + 100.0]))), run(inp)
    for o2, o1 in zip(mixed, whole):
        assert torch.all(o2[:, 1:] == 0) and torch.isfinite(o2).all() and o2[:, :1].abs().max() > 0
        assert torch.equal(o2[:, :1], o1[:, :1])


@pytest.mark.parametrize('qt', sorted(QT_CASES))
def test_two_runs_give_the_same_bits_and_three_kernels_equal_three_single_kernel_calls(qt):
    inp, _ = case(QT_CASES[qt])
    assert CASES[QT_CASES[qt]]['K'] == 3
    out = run(inp)
    for a, b in zip(out, run(inp)):
        assert torch.equal(a, b)
    for k in range(3):
        one = {name: (a if name in ('x', 'v', 'dx', 'dv') else np.asarray(a)[k:k + 1]) for name, a in inp.items()}
        for ok, o in zip(run(one), out):
            assert torch.equal(ok[0], o[k]), k


@pytest.mark.parametrize('qt', sorted(QT_CASES))
def test_a_points_bits_do_not_depend_on_n_or_on_its_place_in_x(qt):
    inp, _ = case(QT_CASES[qt])
    q = CASES[QT_CASES[qt]]['Q']
    assert tangent_tiles(q) == qt
    npg = points_per_group(q)
    rng = np.random.default_rng(q)
    n = 3 * npg + 2
    pts = {name: rng.standard_normal((n, q)) / np.sqrt(q) for name in ('x', 'v', 'dx', 'dv')}
    whole = run(dict(inp, **pts))
    for pick in (np.arange(1), np.arange(n - 1, n), np.arange(1, n), np.arange(n - 1, -1, -1), np.array([n - 1, 0, 0, npg, npg - 1])):
        part = run(dict(inp, **{name: a[pick] for name, a in pts.items()}))
        at = torch.as_tensor(pick, device='cuda')
        for o, w in zip(part, whole):
            assert torch.equal(o, w.index_select(1, at)), pick[:4]


# ---- the finishing operator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(ACCEL_CASES)), ids=[accel_case_id(c) for c in ACCEL_CASES])
def test_finishing_operator_against_the_reference_and_geodesic_accel(i):
    inp, ref = accel_tangent_case(i)
    c = ACCEL_CASES[i]
    a, da, speed, info = finish(inp)
    assert tuple(a.shape) == tuple(da.shape) == (c['N'], c['Q']) and tuple(speed.shape) == tuple(info.shape) == (c['N'],)
    assert da.dtype == torch.float64 and info.dtype == torch.int32 and torch.all(info == 0)
    for have, want in zip((a, speed, info), ops.geodesic_accel(dev(inp['g']), dev(inp['gam']), dev(inp['prior']), dev(inp['v']))):
        assert torch.equal(have, want)                                   # geodesic_accel's bits
    err, scale = float(np.max(np.abs(da.cpu().numpy().astype(LD) - ref['da']))), float(np.max(np.abs(ref['da'])))
    print('%s: da %.2e of max |da| = %.2e' % (accel_case_id(c), err / scale, scale))
    assert err <= TOL_A * scale
    for one, two in zip(finish(inp), (a, da, speed, info)):
        assert torch.equal(one, two)                                     # the same bits on a second run


@pytest.mark.parametrize('i', [3, 6], ids=lambda i: accel_case_id(ACCEL_CASES[i]))
def test_an_indefinite_matrix_fails_alone(i):
    inp, _ = accel_tangent_case(i)
    c = ACCEL_CASES[i]
    n_bad, pivot = c['N'] // 2, (c['Q'] + 1) // 2                         # 1-based: the pivot that goes negative
    g = np.array(inp['g'])
    g[0, n_bad, pivot - 1, pivot - 1] -= 1e3
    assert accel_ref(g, inp['gam'], inp['prior'], inp['v'])[2][n_bad] == pivot
    good = finish(inp)
    a, da, speed, info = finish(dict(inp, g=g))
    keep = torch.as_tensor([j for j in range(c['N']) if j != n_bad], device='cuda')
    assert int(info[n_bad]) == pivot and torch.all(torch.isnan(a[n_bad])) and torch.all(torch.isnan(da[n_bad]))
    assert torch.all(info.index_select(0, keep) == 0)
    for have, want in zip((a, da, speed), good):
        assert torch.equal(have.index_select(0, keep), want.index_select(0, keep))
    assert torch.isfinite(speed).all()
