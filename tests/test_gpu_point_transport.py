"""GPU tests of ops.ard_rbf_point_transport (csrc/ard_rbf_point_metric.hip, the transport mode of mt_kernel) and
ops.geodesic_transport (csrc/geodesic_accel.hip) against the np.longdouble references and the case tables of
tests/test_point_transport_refs.py: random indefinite NON-symmetric p, z, x, v, w ~ N(0, 1) / sqrt(Q), gamma in [0.2, 3].
Tolerances: 1e-12 relative to the sum of the absolute values of each entry's terms for g, gam and tgam (the sibling operators'
bound); 1e-9 of max |dw| for the frame's rates, on matrices whose condition number the CPU file bounds by 1e4.  g, gam and a,
speed, info carry the bits of the operators they extend; a vector's tgam does not know its frame; w_r = v gives gam and a."""
import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import ops
from test_point_christoffel_refs import ACCEL_CASES, accel_case_id, accel_ref
from test_point_transport_refs import (CASES, QT_CASES, accel_transport_case, case, case_id, points_per_group, transport_inputs,
                                       transport_ref, transport_tiles)

pytestmark = pytest.mark.gpu
TOL, TOL_A = 1e-12, 1e-9
LD = np.longdouble
NAMES = ('g', 'gam', 'tgam')


def dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64), device='cuda')


def run(inp):
    return ops.ard_rbf_point_transport(dev(inp['z']), dev(inp['x']), dev(inp['v']), dev(inp['w']), dev(inp['gamma']),
                                       dev(inp['alpha']), dev(inp['p']))


def plain(inp):
    return ops.ard_rbf_point_christoffel(dev(inp['z']), dev(inp['x']), dev(inp['v']), dev(inp['gamma']), dev(inp['alpha']),
                                         dev(inp['p']))


def finish(inp):
    return ops.geodesic_transport(dev(inp['g']), dev(inp['gam']), dev(inp['tgam']), dev(inp['prior']), dev(inp['v']))


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
    shapes = dict(g=(c['Q'], c['Q']), gam=(c['Q'],), tgam=(c['F'], c['Q']))
    for name, o in zip(NAMES, out):
        assert tuple(o.shape) == (c['K'], c['N']) + shapes[name] and o.dtype == torch.float64
    ratios = tuple(worst(o, ref[name], ref[name + '_den']) for name, o in zip(NAMES, out))
    print('%s: g %.2e, gam %.2e, tgam %.2e of sum |terms|' % ((case_id(c),) + ratios))
    assert max(ratios) <= TOL, ratios
    g, gam = plain(inp)
    assert torch.equal(out[0], g) and torch.equal(out[1], gam)           # the christoffel operator's bits, whatever QT and W
    if c['Q'] <= 31:                                                     # 2 tgam against the tangent mode's dgam along (0, w_r)
        zero = dev(np.zeros_like(inp['x']))
        den = np.asarray(ref['tgam_den'])
        for r in range(c['F']):
            dgam = ops.ard_rbf_point_christoffel_tangent(dev(inp['z']), dev(inp['x']), dev(inp['v']), zero, dev(inp['w'][:, r]),
                                                         dev(inp['gamma']), dev(inp['alpha']), dev(inp['p']))[3]
            diff = np.abs(2.0 * out[2][:, :, r].cpu().numpy().astype(LD) - dgam.cpu().numpy().astype(LD))
            assert np.all(diff <= TOL * 2.0 * den[:, :, r]), (r, float(np.max(diff / np.maximum(den[:, :, r], 1e-300))))


@pytest.mark.parametrize('qt', sorted(QT_CASES))
def test_a_vectors_symbol_does_not_know_its_frame_and_the_velocity_gives_gam(qt):
    """tgam[.., r, :] has the same bits whether w_r is alone, first, last, or in a frame that changes QT; w_r = v: gam's bits."""
    inp, _ = case(QT_CASES[qt])
    c = CASES[QT_CASES[qt]]
    q, f = c['Q'], c['F']
    whole = run(inp)
    w = np.asarray(inp['w'])
    for r in sorted({0, f - 1}):
        alone = run(dict(inp, w=w[:, r:r + 1]))
        assert transport_tiles(q, 1) <= qt
        assert torch.equal(alone[2][:, :, 0], whole[2][:, :, r]), r
        assert torch.equal(alone[0], whole[0]) and torch.equal(alone[1], whole[1])
    fmax = 63 - q                                                         # the widest frame: QT = 4, the vectors in other places
    rng = np.random.default_rng(qt)
    wide = rng.standard_normal((c['N'], fmax, q)) / np.sqrt(q)
    place = rng.permutation(fmax)[:f]
    wide[:, place] = w
    big = run(dict(inp, w=wide))
    assert torch.equal(big[2][:, :, torch.as_tensor(place, device='cuda')], whole[2])
    v = np.asarray(inp['v'])
    own = np.array(w)
    own[:, 0], own[:, -1] = v, v
    out = run(dict(inp, w=own))
    assert torch.equal(out[2][:, :, 0], out[1]) and torch.equal(out[2][:, :, -1], out[1])
    assert torch.equal(big[1], whole[1]) and torch.equal(run(dict(inp, w=np.repeat(v[:, None], fmax, axis=1)))[2][:, :, fmax - 1], whole[1])


@pytest.mark.parametrize('qt', sorted(QT_CASES))
def test_zero_vectors_and_far_away_points_give_exact_zeros(qt):
    inp, _ = case(QT_CASES[qt])
    x, w = np.asarray(inp['x']), np.array(inp['w'])
    zero = run(dict(inp, w=np.zeros_like(w)))
    assert torch.all(zero[2] == 0)                                        # (no NaN: NaN == 0 is False)
    assert zero[0].abs().max() > 0 and zero[1].abs().max() > 0
    w[:, 0] = 0.0
    part = run(dict(inp, w=w))
    assert torch.all(part[2][:, :, 0] == 0) and (w.shape[1] == 1 or part[2][:, :, 1:].abs().max() > 0)
    far = run(dict(inp, x=x + 100.0))                                     # 100 units from every z: every exponential underflows
    assert all(torch.all(o == 0) for o in far)
    mixed, whole = run(dict(inp, x=np.concatenate([x[:1], x[1:] + 100.0]))), run(inp)
    for o2, o1 in zip(mixed, whole):
        assert torch.all(o2[:, 1:] == 0) and torch.isfinite(o2).all() and o2[:, :1].abs().max() > 0
        assert torch.equal(o2[:, :1], o1[:, :1])


@pytest.mark.parametrize('qt', sorted(QT_CASES))
def test_two_runs_give_the_same_bits_and_three_kernels_equal_three_single_kernel_calls(qt):
    inp, _ = case(QT_CASES[qt])
    k = CASES[QT_CASES[qt]]['K']
    if k != 3:                                                            # (the table alternates K: take three kernels here)
        c = CASES[QT_CASES[qt]]
        inp = transport_inputs(3, c['N'], c['M'], c['Q'], c['F'], 11000 + qt)
    out = run(inp)
    for a, b in zip(out, run(inp)):
        assert torch.equal(a, b)
    for k in range(3):
        one = {name: (a if name in ('x', 'v', 'w') else np.asarray(a)[k:k + 1]) for name, a in inp.items()}
        for ok, o in zip(run(one), out):
            assert torch.equal(ok[0], o[k]), k


@pytest.mark.parametrize('qt', sorted(QT_CASES))
def test_a_points_bits_do_not_depend_on_n_or_on_its_place_in_x(qt):
    inp, _ = case(QT_CASES[qt])
    q, f = CASES[QT_CASES[qt]]['Q'], CASES[QT_CASES[qt]]['F']
    assert transport_tiles(q, f) == qt
    npg = points_per_group(q, f)
    rng = np.random.default_rng(q)
    n = 3 * npg + 2
    pts = {name: rng.standard_normal((n, q)) / np.sqrt(q) for name in ('x', 'v')}
    pts['w'] = rng.standard_normal((n, f, q)) / np.sqrt(q)
    whole = run(dict(inp, **pts))
    for pick in (np.arange(1), np.arange(n - 1, n), np.arange(1, n), np.arange(n - 1, -1, -1), np.array([n - 1, 0, 0, npg, npg - 1])):
        part = run(dict(inp, **{name: a[pick] for name, a in pts.items()}))
        at = torch.as_tensor(pick, device='cuda')
        for o, w in zip(part, whole):
            assert torch.equal(o, w.index_select(1, at)), pick[:4]


# ---- the finishing operator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f', [1, 3, 0], ids=['F1', 'F3', 'FQ'])
@pytest.mark.parametrize('i', range(len(ACCEL_CASES)), ids=[accel_case_id(c) for c in ACCEL_CASES])
def test_finishing_operator_against_the_reference_and_its_siblings(i, f):
    inp, ref = accel_transport_case(i, f)
    c = ACCEL_CASES[i]
    nf = f or c['Q']
    if nf > 63:
        nf = 63                                                          # (Q = 64: the operator's F stops at 63)
        inp = dict(inp, tgam=np.asarray(inp['tgam'])[:, :, :63])
        ref = dict(ref, dw=ref['dw'][:, :63])
    a, dw, speed, info = finish(inp)
    assert tuple(a.shape) == (c['N'], c['Q']) and tuple(dw.shape) == (c['N'], nf, c['Q'])
    assert tuple(speed.shape) == tuple(info.shape) == (c['N'],)
    assert dw.dtype == torch.float64 and info.dtype == torch.int32 and torch.all(info == 0)
    for have, want in zip((a, speed, info), ops.geodesic_accel(dev(inp['g']), dev(inp['gam']), dev(inp['prior']), dev(inp['v']))):
        assert torch.equal(have, want)                                   # geodesic_accel's bits
    err, scale = float(np.max(np.abs(dw.cpu().numpy().astype(LD) - ref['dw']))), float(np.max(np.abs(ref['dw'])))
    print('%s F%d: dw %.2e of max |dw| = %.2e' % (accel_case_id(c), nf, err / scale, scale))
    assert err <= TOL_A * scale
    zero = torch.zeros_like(dev(inp['g']))
    for r in range(nf):                                                  # 2 dw against da of the tangent operator on (0, 2 tgam_r)
        da = ops.geodesic_accel_tangent(dev(inp['g']), dev(inp['gam']), zero, 2.0 * dev(inp['tgam'])[:, :, r].contiguous(),
                                        dev(inp['prior']), dev(inp['v']))[1]
        assert float((2.0 * dw[:, r] - da).abs().max()) <= TOL_A * 2.0 * scale
    for one, two in zip(finish(inp), (a, dw, speed, info)):
        assert torch.equal(one, two)                                     # the same bits on a second run
    own = np.array(inp['tgam'])
    own[:, :, nf - 1] = inp['gam']                                       # tgam[r] = gam: dw_r = a, bit for bit
    a2, dw2, _, _ = finish(dict(inp, tgam=own))
    assert torch.equal(a2, a) and torch.equal(dw2[:, nf - 1], a) and torch.equal(dw2[:, :nf - 1], dw[:, :nf - 1])


@pytest.mark.parametrize('i', [3, 6], ids=lambda i: accel_case_id(ACCEL_CASES[i]))
def test_an_indefinite_matrix_fails_alone(i):
    inp, _ = accel_transport_case(i, 3)
    c = ACCEL_CASES[i]
    n_bad, pivot = c['N'] // 2, (c['Q'] + 1) // 2                         # 1-based: the pivot that goes negative
    g = np.array(inp['g'])
    g[0, n_bad, pivot - 1, pivot - 1] -= 1e3
    assert accel_ref(g, inp['gam'], inp['prior'], inp['v'])[2][n_bad] == pivot
    good = finish(inp)
    a, dw, speed, info = finish(dict(inp, g=g))
    keep = torch.as_tensor([j for j in range(c['N']) if j != n_bad], device='cuda')
    assert int(info[n_bad]) == pivot and torch.all(torch.isnan(a[n_bad])) and torch.all(torch.isnan(dw[n_bad]))
    assert torch.all(info.index_select(0, keep) == 0)
    for have, want in zip((a, dw, speed), good):
        assert torch.equal(have.index_select(0, keep), want.index_select(0, keep))
    assert torch.isfinite(speed).all()
