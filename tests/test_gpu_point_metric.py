"""GPU tests of ops.ard_rbf_point_metric and ops.ard_rbf_point_jacobian (csrc/ard_rbf_point_metric.hip) against the np.longdouble
references and the case table of tests/test_point_metric_refs.py: random indefinite NON-symmetric p (a transposed index shows),
x, z ~ N(0, 1), gamma in [0.2, 3].  Tolerance: 1e-12 relative to the sum of the absolute values of each entry's terms, the
project's figure for a point operator against a CPU restatement."""
import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import ops
from test_point_metric_refs import CASES, case, case_id

pytestmark = pytest.mark.gpu
TOL = 1e-12


def dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64), device='cuda')


def run(inp):
    z, x, gamma, alpha = dev(inp['z']), dev(inp['x']), dev(inp['gamma']), dev(inp['alpha'])
    return ops.ard_rbf_point_metric(z, x, gamma, alpha, dev(inp['p'])), ops.ard_rbf_point_jacobian(z, x, gamma, alpha, dev(inp['r']))


def worst(got, ref, den):
    """max over the entries of |got - ref| / sum |terms| (entries whose terms all vanish must be exact zeros)."""
    got = got.cpu().numpy().astype(np.longdouble)
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    assert np.all(err[den == 0] == 0)
    return float(np.max(np.where(den > 0, err / np.where(den > 0, den, 1), 0)))


@pytest.mark.parametrize('i', range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_operators_against_the_longdouble_references(i):
    inp, ref = case(i)
    g, jac = run(inp)
    eg, ej = worst(g, ref['g'], ref['g_den']), worst(jac, ref['jac'], ref['jac_den'])
    print('%s: metric %.2e, jacobian %.2e of sum |terms|' % (case_id(CASES[i]), eg, ej))
    assert eg <= TOL and ej <= TOL, (eg, ej)


def test_far_away_points_give_exact_zeros():
    inp, _ = case(0)
    far = dict(inp, x=np.asarray(inp['x']) + 60.0)                       # |x - z| ~ 60: every exponential underflows
    g, jac = run(far)
    assert torch.all(g == 0) and torch.all(jac == 0)                     # (no NaN: NaN == 0 is False)
    mixed = dict(inp, x=np.concatenate([np.asarray(inp['x'])[:5], np.asarray(inp['x'])[5:] + 60.0]))
    g2, jac2 = run(mixed)
    g1, jac1 = run(inp)
    assert torch.all(g2[:, 5:] == 0) and torch.all(jac2[:, 5:] == 0)
    assert torch.isfinite(g2).all() and torch.isfinite(jac2).all() and g2[:, :5].abs().max() > 0
    assert torch.equal(g2[:, :5], g1[:, :5]) and torch.equal(jac2[:, :5], jac1[:, :5])


@pytest.mark.parametrize('i', [0, len(CASES) - 6], ids=lambda i: case_id(CASES[i]))
def test_two_runs_give_the_same_bits(i):
    inp, _ = case(i)
    (g1, j1), (g2, j2) = run(inp), run(inp)
    assert torch.equal(g1, g2) and torch.equal(j1, j2)


@pytest.mark.parametrize('i', [0, len(CASES) - 6], ids=lambda i: case_id(CASES[i]))
def test_three_kernels_equal_three_single_kernel_calls(i):
    inp, _ = case(i)
    assert CASES[i]['K'] == 3
    g, jac = run(inp)
    for k in range(3):
        one = {name: (a if name == 'x' else np.asarray(a)[k:k + 1]) for name, a in inp.items()}
        gk, jk = run(one)
        assert torch.equal(gk[0], g[k]) and torch.equal(jk[0], jac[k]), k


def test_p_is_used_as_given():
    inp, ref = case(0)
    g, _ = run(inp)
    gt, _ = run(dict(inp, p=np.ascontiguousarray(np.asarray(inp['p']).transpose(0, 2, 1))))
    scale = float(g.abs().max())
    assert float((g - g.transpose(2, 3)).abs().max()) > 1e-3 * scale     # a non-symmetric p gives a non-symmetric g
    assert worst(gt.transpose(2, 3).contiguous(), ref['g'], ref['g_den']) <= TOL
