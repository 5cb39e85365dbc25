"""GPU tests of ops.geodesic_shoot / ops.geodesic_shoot_tangent (csrc/geodesic_accel.hip: the integrators on the device) on the case
tables of tests/test_geodesic_shoot_refs.py.  The host composition is models/geodesic._rk4 (the loop of exp_map) / _rk4_tangent on
ops.ard_rbf_point_christoffel[_tangent] per part, the slabs concatenated, and ops.geodesic_accel[_tangent]: the device call has to
give its BITS (torch.equal) at every row, which the CPU file's mirror of the staging shows to be attainable.  Against the
np.longdouble-accelerated NumPy integrators the bound is the host integrators' own, 1e-9 of max |.|."""
import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import ops
from dp_gp_lvm_amd.models import geodesic
from test_geodesic_shoot_refs import PLAIN, TANGENT, plain_case, row_id, shoot_inputs, tangent_case

pytestmark = pytest.mark.gpu
TOL = 1e-9


def dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64), device='cuda')


def operands(inp):
    """(parts as ops.geodesic_shoot takes them, prior, the states x, v[, dx, dv]) on the GPU."""
    parts = [tuple(dev(pt[n]) for n in ('z', 'gamma', 'alpha', 'p')) for pt in inp['parts']]
    return parts, dev(inp['prior']), [dev(inp[n]) for n in ('x', 'v', 'dx', 'dv') if n in inp]


def host_accel(parts, prior):
    def accel(x, v):
        slabs = [ops.ard_rbf_point_christoffel(z, x, v, gamma, alpha, p) for z, gamma, alpha, p in parts]
        return ops.geodesic_accel(*(slabs[0] if len(slabs) == 1 else [torch.cat(ss) for ss in zip(*slabs)]), prior, v)
    return accel


def host_accel_tangent(parts, prior):
    def accel_tangent(x, v, dx, dv):
        slabs = [ops.ard_rbf_point_christoffel_tangent(z, x, v, dx, dv, gamma, alpha, p) for z, gamma, alpha, p in parts]
        return ops.geodesic_accel_tangent(*(slabs[0] if len(slabs) == 1 else [torch.cat(ss) for ss in zip(*slabs)]), prior, v)
    return accel_tangent


def host(parts, prior, states, steps):
    """The host composition's results in the order of the device call's."""
    if len(states) == 2:
        return geodesic._rk4(host_accel(parts, prior), *states, steps)
    return geodesic._rk4_tangent(host_accel_tangent(parts, prior), *states, steps)


def device(parts, prior, states, steps):
    return (ops.geodesic_shoot if len(states) == 2 else ops.geodesic_shoot_tangent)(parts, prior, *states, steps)


def same_bits(have, want):
    return len(have) == len(want) and all(h.dtype == w.dtype and torch.equal(h, w) for h, w in zip(have, want))


@pytest.mark.parametrize('i', range(len(PLAIN)), ids=[row_id(r) for r in PLAIN])
def test_exponential_map_carries_the_bits_of_the_host_composition(i):
    row = PLAIN[i]
    inp, (ref_c, ref_v), _ = plain_case(i)
    parts, prior, states = operands(inp)
    have = device(parts, prior, states, row['S'])
    curve, vel, bad = have
    assert tuple(curve.shape) == (row['C'], row['S'] + 1, row['Q']) == tuple(vel.shape) and tuple(bad.shape) == (row['C'],)
    assert curve.dtype == torch.float64 and bad.dtype == torch.int32 and curve.is_cuda
    want = host(parts, prior, states, row['S'])
    for name, h, w in zip(('curve', 'vel', 'bad'), have, want):
        assert torch.equal(h, w), (name, float((h - w).abs().max()))
    assert not bool(bad.any())
    assert torch.equal(curve[:, 0], states[0]) and torch.equal(vel[:, 0], states[1])                  # row 0: the bits of the inputs
    ec, ev = float(np.max(np.abs(curve.cpu().numpy() - ref_c))), float(np.max(np.abs(vel.cpu().numpy() - ref_v)))
    sc, sv = float(np.max(np.abs(ref_c))), float(np.max(np.abs(ref_v)))
    print('%s: |curve - longdouble rk4| %.3e of %.3e, |vel - longdouble rk4| %.3e of %.3e' % (row_id(row), ec, sc, ev, sv))
    assert ec <= TOL * sc and ev <= TOL * sv
    assert same_bits(device(parts, prior, states, row['S']), have)                                    # equal bits on two runs


@pytest.mark.parametrize('i', range(len(TANGENT)), ids=[row_id(r) for r in TANGENT])
def test_tangent_carries_the_bits_of_the_host_composition(i):
    row = TANGENT[i]
    inp, refs, _ = tangent_case(i)                                                                    # (curve, dcurve, vel, dvel)
    parts, prior, states = operands(inp)
    have = device(parts, prior, states, row['S'])
    curve, vel, dcurve, dvel, bad, speed0 = have
    assert all(tuple(t.shape) == (row['C'], row['S'] + 1, row['Q']) for t in have[:4])
    assert tuple(bad.shape) == (row['C'],) == tuple(speed0.shape) and bad.dtype == torch.int32 and speed0.dtype == torch.float64
    want = host(parts, prior, states, row['S'])
    for name, h, w in zip(('curve', 'vel', 'dcurve', 'dvel', 'bad', 'speed0'), have, want):
        assert torch.equal(h, w), (name, float((h - w).abs().max()))
    assert not bool(bad.any())
    for rows, start in zip(have[:4], states):
        assert torch.equal(rows[:, 0], start)
    plain = device(parts, prior, states[:2], row['S'])                                                # the plain call's bits
    assert torch.equal(plain[0], curve) and torch.equal(plain[1], vel) and torch.equal(plain[2], bad)
    for name, h, r in zip(('curve', 'dcurve', 'vel', 'dvel'), (curve, dcurve, vel, dvel), refs):
        err, scale = float(np.max(np.abs(h.cpu().numpy() - r))), float(np.max(np.abs(r)))
        print('%s: |%s - longdouble tangent rk4| %.3e of %.3e' % (row_id(row), name, err, scale))
        assert err <= TOL * scale
    assert same_bits(device(parts, prior, states, row['S']), have)


MID = dict(Q=3, parts=((5, 9), (4, 65)), C=9, S=2)


@pytest.mark.parametrize('tangent', [False, True], ids=['plain', 'tangent'])
def test_a_curve_does_not_depend_on_its_batch(tangent):
    parts, prior, states = operands(shoot_inputs(MID, 9600, tangent))
    whole = device(parts, prior, states, MID['S'])
    one = device(parts, prior, [t[4:5].contiguous() for t in states], MID['S'])
    assert all(torch.equal(o[0], w[4]) for o, w in zip(one, whole))                                   # a single curve is its row
    flipped = device(parts, prior, [t.flip(0).contiguous() for t in states], MID['S'])
    assert all(torch.equal(f.flip(0), w) for f, w in zip(flipped, whole))
    for pick in ([0, 2, 4, 6, 8], [7, 1], [3]):
        sub = device(parts, prior, [t[pick].contiguous() for t in states], MID['S'])
        assert all(torch.equal(s, w[pick]) for s, w in zip(sub, whole)), pick


@pytest.mark.parametrize('tangent', [False, True], ids=['plain', 'tangent'])
def test_far_from_every_inducing_input_the_curves_are_exact_straight_lines(tangent):
    parts, prior, states = operands(shoot_inputs(MID, 9601, tangent))
    states[0] = states[0] + 100.0
    steps = 4
    have = device(parts, prior, states, steps)
    assert same_bits(have, host(parts, prior, states, steps))
    t = torch.arange(steps + 1, dtype=torch.float64, device='cuda') / steps
    line = states[0][:, None, :] + t[None, :, None] * states[1][:, None, :]
    assert float((have[0] - line).abs().max()) <= 1e-14 * float(line.abs().max())
    assert torch.equal(have[1], states[1][:, None, :].expand_as(have[1]))                             # a = 0 exactly: v never moves
    if tangent:
        dline = states[2][:, None, :] + t[None, :, None] * states[3][:, None, :]
        assert float((have[2] - dline).abs().max()) <= 1e-14 * float(dline.abs().max())
        assert torch.equal(have[3], states[3][:, None, :].expand_as(have[3]))


@pytest.mark.parametrize('tangent', [False, True], ids=['plain', 'tangent'])
def test_a_curve_whose_metric_is_indefinite_fails_alone(tangent):
    """A second part, one kernel on one inducing input far from the others with a large negative p, digs a pit into the metric
    around that input: the curve that starts in the pit fails to factor at its first stage; the others are five units away."""
    inp = shoot_inputs(dict(MID, parts=((5, 9),), C=5), 9602, tangent)
    parts, prior, states = operands(inp)
    q = MID['Q']
    centre = torch.full((q,), 5.0, dtype=torch.float64, device='cuda')
    parts.append((centre[None, None, :].clone(), torch.ones((1, q), dtype=torch.float64, device='cuda'),
                  torch.ones(1, dtype=torch.float64, device='cuda'), torch.full((1, 1, 1), -100.0, dtype=torch.float64, device='cuda')))
    states[0][2] = centre
    states[0][2, 0] += 1.0                                     # where the derivative feature is largest: G_00 = prior_0 - 100 / e
    steps, keep = 2, [0, 1, 3, 4]
    have = device(parts, prior, states, steps)
    want = host(parts, prior, states, steps)
    bad = have[-2] if tangent else have[-1]
    assert torch.equal(bad, want[-2] if tangent else want[-1])
    assert int(bad[2]) > 0 and not bool(bad[keep].any())
    print('bad:', bad.tolist())
    without = device(parts, prior, [t[keep].contiguous() for t in states], steps)
    for h, w, alone in zip(have, want, without):
        assert torch.equal(h[keep], alone) and torch.equal(h[keep], w[keep])                          # bitwise as without it
        if h.dim() == 3:
            assert bool(torch.isfinite(h[keep]).all()) and bool(torch.isnan(h[2, 1:]).any())
            assert torch.equal(torch.isnan(h[2]), torch.isnan(w[2]))
            assert torch.equal(h[2, 0], w[2, 0])
