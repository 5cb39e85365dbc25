"""GPU tests of ops.ard_rbf_point_cov (csrc/ard_rbf_point_cov.hip) against the np.longdouble reference and the case table of
tests/test_point_cov_refs.py: random indefinite NON-symmetric c, z, x ~ N(0, 1) / sqrt(Q), gamma in [0.2, 3].  Tolerance: 1e-12
relative to the sum of the absolute values of each entry's terms, the bound of the metric and energy operators."""
import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import ops
from test_point_cov_refs import CASES, case, case_id, features, prior_ref

pytestmark = pytest.mark.gpu
TOL = 1e-12
BIG = CASES.index(dict(K=3, G=2, N=130, M=200, Q=21))
MULTI = CASES.index(dict(K=2, G=3, N=63, M=129, Q=10))


def dev(a):
    return torch.as_tensor(np.array(a, dtype=np.float64), device='cuda')


def run(inp):
    return ops.ard_rbf_point_cov(dev(inp['z']), dev(inp['x']), dev(inp['gamma']), dev(inp['alpha']), dev(inp['c']))


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
    assert tuple(out.shape) == (c['K'], c['G'], c['N'], c['N'])
    ratio = worst(out, ref['out'], ref['den'])
    print('%s: %.2e of sum |terms|' % (case_id(c), ratio))
    assert ratio <= TOL
    assert torch.equal(out, out.transpose(2, 3))                         # bitwise symmetric


@pytest.mark.parametrize('i', [MULTI, BIG], ids=lambda i: case_id(CASES[i]))
def test_diagonal_is_alpha_minus_the_quadratic_form(i):
    inp, ref = case(i)
    ld = lambda name: np.asarray(inp[name], dtype=np.longdouble)
    kv = features(ld('z'), ld('x'), ld('gamma'), ld('alpha'))
    want = ld('alpha')[:, None, None] - np.einsum('knm,kgmp,knp->kgn', kv, ld('c'), kv)
    got = torch.diagonal(run(inp), dim1=2, dim2=3)
    assert worst(got, want, np.diagonal(ref['den'], axis1=2, axis2=3)) <= TOL


@pytest.mark.parametrize('i', [0, BIG], ids=lambda i: case_id(CASES[i]))
def test_two_runs_give_the_same_bits(i):
    inp, _ = case(i)
    assert torch.equal(run(inp), run(inp))


def test_three_kernels_equal_three_single_kernel_calls():
    inp, _ = case(BIG)
    assert CASES[BIG]['K'] == 3
    out = run(inp)
    for k in range(3):
        one = {name: (a if name == 'x' else np.asarray(a)[k:k + 1]) for name, a in inp.items()}
        assert torch.equal(run(one)[0], out[k]), k


@pytest.mark.parametrize('i', [MULTI, BIG], ids=lambda i: case_id(CASES[i]))
def test_g_patterns_equal_g_single_pattern_calls(i):
    inp, _ = case(i)
    out = run(inp)
    for g in range(CASES[i]['G']):
        assert torch.equal(run(dict(inp, c=np.asarray(inp['c'])[:, g:g + 1]))[:, 0], out[:, g]), g


def test_an_entrys_bits_do_not_depend_on_n_or_on_the_places_of_its_points():
    inp, _ = case(BIG)                                                   # N = 130: five tiles of 32, the last with 2 points
    x = np.asarray(inp['x'])
    whole = run(inp)
    for pick in (np.arange(37, 38), np.arange(5, 130), np.arange(129, -1, -1), np.array([128, 3, 3, 77, 16, 15])):
        part = run(dict(inp, x=x[pick]))
        at = torch.as_tensor(pick, device='cuda')
        assert torch.equal(part, whole.index_select(2, at).index_select(3, at)), pick[:4]


def test_c_and_its_transpose_agree():
    inp, ref = case(MULTI)
    c = np.asarray(inp['c'])
    assert np.max(np.abs(c - c.transpose(0, 1, 3, 2))) > 0.1
    a, b = run(inp), run(dict(inp, c=np.ascontiguousarray(c.transpose(0, 1, 3, 2))))
    ratio = float(np.max(np.abs((a - b).cpu().numpy()) / np.asarray(ref['den'], dtype=np.float64)))
    assert ratio <= TOL and worst(b, ref['out'], ref['den']) <= TOL


def test_far_away_points_give_the_prior_term_alone():
    inp, ref = case(MULTI)
    x = np.asarray(inp['x'])
    far = dict(inp, x=x + 100.0)                                         # 100 units from every z: every feature underflows to 0
    prior = run(dict(far, c=np.zeros_like(np.asarray(inp['c']))))       # the operator's own prior term
    want = prior_ref(far['x'], inp['gamma'], inp['alpha'])[:, None] + np.zeros_like(ref['out'])
    assert worst(prior, want, np.abs(want)) <= TOL
    out = run(far)
    assert torch.isfinite(out).all() and torch.equal(out, prior)
    mixed = dict(inp, x=np.concatenate([x[:5], x[5:] + 100.0]))
    o2, o1 = run(mixed), run(inp)
    assert torch.isfinite(o2).all()
    assert torch.equal(o2[:, :, 5:, 5:], prior[:, :, 5:, 5:])            # far with far: the prior term, exactly
    assert torch.equal(o2[:, :, :5, :5], o1[:, :, :5, :5])               # near with near: untouched
    cross = prior_ref(mixed['x'], inp['gamma'], inp['alpha'])[:, None, :5, 5:]
    assert np.all(cross < 1e-300) and torch.all(o2[:, :, :5, 5:] == 0) and torch.all(o2[:, :, 5:, :5] == 0)


def test_guard_bands_around_out_are_untouched(monkeypatch):
    inp, ref = case(MULTI)
    c = CASES[MULTI]
    numel, band = c['K'] * c['G'] * c['N'] * c['N'], 4096
    buf = torch.full((numel + 2 * band,), float('nan'), dtype=torch.float64, device='cuda')
    real_empty = torch.empty

    def empty(shape, *a, **kw):
        if isinstance(shape, tuple) and shape == (c['K'], c['G'], c['N'], c['N']):
            return buf[band:band + numel].view(*shape)
        return real_empty(shape, *a, **kw)

    monkeypatch.setattr(torch, 'empty', empty)
    out = run(inp)
    monkeypatch.undo()
    assert out.data_ptr() == buf.data_ptr() + 8 * band
    assert torch.isnan(buf[:band]).all() and torch.isnan(buf[band + numel:]).all()
    assert worst(out, ref['out'], ref['den']) <= TOL
