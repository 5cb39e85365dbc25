"""GPU tests of ops.ard_rbf_point_energy (csrc/ard_rbf_point_energy.hip) against the np.longdouble reference and the case table of
tests/test_point_energy_refs.py: random indefinite NON-symmetric p, z, x, v ~ N(0, 1) / sqrt(Q), gamma in [0.2, 3].  Tolerance:
1e-12 relative to the sum of the absolute values of each entry's terms in the difference form, the metric operator's bound."""
import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import ops
from test_point_energy_refs import CASES, case, case_id

pytestmark = pytest.mark.gpu
TOL = 1e-12
NAMES = ('e', 'dx', 'dv')
BIG = CASES.index(dict(K=3, N=130, M=200, Q=21))


def dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64), device='cuda')


def run(inp):
    return ops.ard_rbf_point_energy(dev(inp['z']), dev(inp['x']), dev(inp['v']), dev(inp['gamma']), dev(inp['alpha']), dev(inp['p']))


def worst(got, ref, den):
    """max over the entries of |got - ref| / sum |terms| (entries whose terms all vanish must be exact zeros)."""
    got = got.cpu().numpy().astype(np.longdouble)
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    assert np.all(err[den == 0] == 0)
    return float(np.max(np.where(den > 0, err / np.where(den > 0, den, 1), 0)))


@pytest.mark.parametrize('i', range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_operator_against_the_longdouble_reference(i):
    inp, ref = case(i)
    c = CASES[i]
    out = run(inp)
    assert [tuple(o.shape) for o in out] == [(c['K'], c['N']), (c['K'], c['N'], c['Q']), (c['K'], c['N'], c['Q'])]
    ratios = [worst(o, ref[name], ref[name + '_den']) for o, name in zip(out, NAMES)]
    print('%s: e %.2e, dx %.2e, dv %.2e of sum |terms|' % ((case_id(c),) + tuple(ratios)))
    assert max(ratios) <= TOL, ratios


@pytest.mark.parametrize('i', [0, BIG], ids=lambda i: case_id(CASES[i]))
def test_energy_is_the_metric_operator_along_v(i):
    inp, ref = case(i)
    e, _, _ = run(inp)
    g = ops.ard_rbf_point_metric(dev(inp['z']), dev(inp['x']), dev(inp['gamma']), dev(inp['alpha']), dev(inp['p']))
    v = dev(inp['v'])
    want = torch.einsum('nq,knqr,nr->kn', v, g, v)
    ratio = float(np.max(np.abs((e - want).cpu().numpy()) / np.asarray(ref['e_den'], dtype=np.float64)))
    print('%s: |e - v^T metric v| %.2e of sum |terms|' % (case_id(CASES[i]), ratio))
    assert ratio <= TOL


def test_far_away_points_give_exact_zeros():
    inp, _ = case(0)
    far = dict(inp, x=np.asarray(inp['x']) + 100.0)                      # 100 units from every z: every exponential underflows
    for o in run(far):
        assert torch.all(o == 0)                                         # (no NaN: NaN == 0 is False)
    mixed = dict(inp, x=np.concatenate([np.asarray(inp['x'])[:5], np.asarray(inp['x'])[5:] + 100.0]))
    for o2, o1 in zip(run(mixed), run(inp)):
        assert torch.all(o2[:, 5:] == 0) and torch.isfinite(o2).all() and o2[:, :5].abs().max() > 0
        assert torch.equal(o2[:, :5], o1[:, :5])


@pytest.mark.parametrize('i', [0, BIG], ids=lambda i: case_id(CASES[i]))
def test_two_runs_give_the_same_bits(i):
    inp, _ = case(i)
    for a, b in zip(run(inp), run(inp)):
        assert torch.equal(a, b)


@pytest.mark.parametrize('i', [0, BIG], ids=lambda i: case_id(CASES[i]))
def test_three_kernels_equal_three_single_kernel_calls(i):
    inp, _ = case(i)
    assert CASES[i]['K'] == 3
    out = run(inp)
    for k in range(3):
        one = {name: (a if name in ('x', 'v') else np.asarray(a)[k:k + 1]) for name, a in inp.items()}
        for ok, o in zip(run(one), out):
            assert torch.equal(ok[0], o[k]), k


def test_a_points_bits_do_not_depend_on_n_or_on_its_place_in_the_tile():
    inp, _ = case(BIG)                                                   # N = 130: nine tiles of 16, the last with 2 points
    x, v = np.asarray(inp['x']), np.asarray(inp['v'])
    whole = run(inp)
    for pick in (np.arange(37, 38), np.arange(5, 130), np.arange(129, -1, -1), np.array([128, 3, 3, 77, 16, 15])):
        part = run(dict(inp, x=x[pick], v=v[pick]))
        at = torch.as_tensor(pick, device='cuda')
        for o, w in zip(part, whole):
            assert torch.equal(o, w.index_select(1, at)), pick[:4]


def test_p_and_its_transpose_agree():
    inp, ref = case(0)
    p = np.asarray(inp['p'])
    assert np.max(np.abs(p - p.transpose(0, 2, 1))) > 0.1
    a, b = run(inp), run(dict(inp, p=np.ascontiguousarray(p.transpose(0, 2, 1))))
    for one, two, name in zip(a, b, NAMES):
        ratio = float(np.max(np.abs((one - two).cpu().numpy()) / np.asarray(ref[name + '_den'], dtype=np.float64)))
        assert ratio <= TOL, (name, ratio)
        assert worst(two, ref[name], ref[name + '_den']) <= TOL
