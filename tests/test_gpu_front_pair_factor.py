"""
GPU tests of the front launch of the fused ELBO evaluation (csrc/elementwise.hip, elbo_front_kernel) after it took over the pair factors
of the pair-tile Psi2 kernel (csrc/psi2_pairs.hip):

  * K_uu + jitter I: only the 64 x 64 tiles on and below the diagonal are computed, a tile below it is stored a second time transposed.
    The square the evaluation leaves in its workspace must equal the generic gram operator's BIT FOR BIT, and its own transpose.
  * the pair factors alpha^2 exp(-r^2 / 4), written by the same blocks into the pair kernel's table from the fp64 squared distances
    they hold, against fp64 arithmetic.  Tolerance (relative, where the factor is a normal fp32 number): 4 x 2^-24 -- one rounding each for the
    fraction of the exponent, alpha^2, the v_exp_f32 result and the product.  Below the normal range factor and reference are both at
    most 2^-126 alpha^2.
  * Psi2 as the fused forward evaluation leaves it (slabs of the workspace), against the fp64 oracle at TOL_PSI2 (test_gpu_kernels), and
    no further from it than the stand-alone operator, which still builds the table from fp32 distances in a launch of its own.
  * the training step (dpgp_elbo_step keeps the table built from fp32 distances) against the separate calls, whose forward evaluation
    takes the factors from the K_uu blocks: the tolerances of test_gpu_grad.test_training_step_equals_the_three_calls.

Every figure is printed before it is asserted (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import ops
from oracle import dpgp_oracle as orc
from test_gpu_kernels import TOL_PSI2
from test_gpu_grad import _stage_b_problem

pytestmark = pytest.mark.gpu

MS = [1, 15, 16, 17, 63, 64, 65, 127, 128]       # one tile, tile edge, two tile rows, ragged last tile
F64 = torch.float64
JITTER = 1e-8
FAC_RTOL = 4.0 * 2.0 ** -24
FLT_MIN = 2.0 ** -126


def t64(a, dev):
    return torch.as_tensor(np.array(a, dtype=np.float64), device=dev)     # (a copy: the cases are read-only)


@functools.lru_cache(maxsize=None)
def problem(n, d, m, q, geometry='normal', alphas=None, fp32_exact=False):
    """Host arrays (y, z, mu, s, gamma, alpha, beta) of one seeded case; read-only (shared by the tests that need them)."""
    rng = np.random.default_rng(1000 * m + 10 * q + d)
    z = rng.standard_normal((m, q))
    gamma = np.exp(0.3 * rng.standard_normal((d, q)))
    if geometry == 'clusters':                                   # two clusters 40 length scales (of the longest one) apart: far pairs underflow
        z = 0.5 * z
        z[m // 2:, 0] += 40.0 / np.sqrt(gamma[:, 0].min())
    mu = rng.standard_normal((n, q))
    s = np.exp(0.5 * rng.standard_normal((n, q)))
    alpha = np.exp(0.3 * rng.standard_normal(d)) if alphas is None else np.array(alphas, dtype=np.float64)
    beta = np.exp(0.2 * rng.standard_normal(d)) * 2.0
    y = rng.standard_normal((n, d))
    out = [y, z, mu, s, gamma, alpha, beta]
    if fp32_exact:                                               # the fp32 operator then sees the very same numbers
        out = [a.astype(np.float32).astype(np.float64) for a in out]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def forward(dev, p, n, d, m, q):
    w = ops.ElboWorkspace(d, n, m, q, 'mixed', dev)
    ops.elbo_fhat(*[t64(a, dev) for a in p], jitter=JITTER, prec='mixed', workspace=w)
    torch.cuda.synchronize()
    return w


@pytest.mark.parametrize('m', MS)
def test_kuu_is_the_gram_operators_bit_for_bit_and_symmetric(dev, m):
    n = 40
    for d in (1, 3):
        for q in (1, 10, 21):
            p = problem(n, d, m, q)
            w = forward(dev, p, n, d, m, q)
            z, gamma, alpha, beta = (t64(p[i], dev) for i in (1, 4, 5, 6))
            want = ops.ard_rbf_gram(z, None, gamma, alpha.view(d, 1), beta.view(d, 1), include_noise=False, include_jitter=True,
                                    jitter=JITTER)
            got = w.kuu()
            assert got.shape == want.shape == (d, m, m)
            what = 'M=%d D=%d Q=%d' % (m, d, q)
            assert torch.equal(got, want), '%s: K_uu of the front launch differs from the gram operator in %d entries' % (
                what, int((got != want).sum()))
            assert torch.equal(got, got.transpose(1, 2)), what + ': K_uu is not its own transpose'


def factor_reference(z, gamma, alpha):
    dz = z[:, None, :] - z[None, :, :]
    r2 = np.einsum('dq,mkq->dmk', gamma, dz * dz)
    return alpha[:, None, None] ** 2 * np.exp(-0.25 * r2)


@pytest.mark.parametrize('geometry', ['normal', 'clusters'])
@pytest.mark.parametrize('m', MS)
def test_pair_factors_against_fp64(dev, m, geometry):
    n, d, q = 40, 3, 10
    p = problem(n, d, m, q, geometry, alphas=(1e-3, 1.0, 1e3))
    w = forward(dev, p, n, d, m, q)
    fac = w.pair_factors()
    assert fac is not None and fac.shape == (d, m, m)
    got = fac.cpu().numpy().astype(np.float64)
    ref = factor_reference(p[1], p[4], p[5])
    low = np.tril(np.ones((m, m), dtype=bool))
    a2 = (p[5] ** 2)[:, None, None] * np.ones_like(ref)
    got, ref, a2 = got[:, low], ref[:, low], a2[:, low]
    assert np.isfinite(got).all() and (got >= 0).all()
    normal = ref >= FLT_MIN                                       # the factor is a normal fp32 number
    under = ref < FLT_MIN * a2                                    # below the range of the exponential: both at most 2^-126 alpha^2
    between = ~normal & ~under                                    # (alpha < 1 only) subnormal results: the grid's step 2^-149 on top
    rel = np.abs(got[normal] - ref[normal]) / ref[normal]
    print('pair factors M=%d %s: %d normal entries, max rel err %.3g = %.2f x 2^-24; %d below the range (largest %.3g), %d subnormal'
          % (m, geometry, normal.sum(), rel.max(), rel.max() / 2.0 ** -24, under.sum(), got[under].max() if under.any() else 0.0,
             between.sum()))
    assert rel.max() <= FAC_RTOL
    assert (got[under] <= FLT_MIN * a2[under]).all()
    assert (np.abs(got[between] - ref[between]) <= FAC_RTOL * ref[between] + 2.0 ** -149).all()
    if geometry == 'clusters' and m >= 15:
        assert under.any(), 'the far pairs were meant to underflow'
    # the diagonal is alpha^2, rounded once
    diag = fac.diagonal(dim1=1, dim2=2).cpu().numpy()
    assert (diag == (p[5] ** 2).astype(np.float32)[:, None]).all()


def psi2_error(got, ref):
    """Largest error relative to max(|ref|, 1e-2 max|ref|) -- the entry size at which TOL_PSI2's rtol hands over to its atol -- over the
    lower triangles."""
    m = ref.shape[-1]
    low = np.tril(np.ones((m, m), dtype=bool))
    g, r = got[:, low], ref[:, low]
    return float((np.abs(g - r) / np.maximum(np.abs(r), 1e-2 * np.abs(r).max())).max())


@pytest.mark.parametrize('shape', [(40, 2, 17, 10),      # Ppad padding, lanes without a pair
                                   (600, 2, 33, 10),     # two chunks: the factor is applied once per chunk and summed
                                   (96, 260, 16, 5),     # D >= 256: K_uu tasks at the end of the grid
                                   (96, 3, 64, 20),      # KS = 8, G = 2
                                   (96, 3, 24, 21)])
def test_psi2_of_the_fused_forward_against_the_oracle(dev, shape):
    n, d, m, q = shape
    p = problem(n, d, m, q, fp32_exact=True)
    y, z, mu, s, gamma, alpha, beta = p
    w = forward(dev, p, n, d, m, q)
    off_p2, ns2, esz, mp = w.layout[:4]
    assert esz == 4
    slabs = w.ws[off_p2:off_p2 + 4 * ns2 * d * mp * mp].view(torch.float32).view(ns2, d, mp, mp)
    low = torch.tril(slabs[:, :, :m, :m]).cpu().numpy().astype(np.float64).sum(axis=0)
    got = low + np.tril(low, -1).transpose(0, 2, 1)
    ref = orc.psi2(z, mu, s, gamma, alpha[:, None])
    tol = TOL_PSI2[torch.float32]
    # the fp32-distance table path on the same numbers: the stand-alone fp32 operator
    f32 = lambda a: torch.as_tensor(np.array(a, dtype=np.float32), device=dev)
    table = ops.psi2(f32(z), f32(mu), f32(s), f32(gamma), f32(alpha[:, None])).cpu().numpy().astype(np.float64)
    e_new, e_tab = psi2_error(got, ref), psi2_error(table, ref)
    print('psi2 N=%d D=%d M=%d Q=%d: error against the oracle, fused forward (factors from the K_uu blocks) %.4g, stand-alone (table from fp32 distances) %.4g'
          % (n, d, m, q, e_new, e_tab))
    lowm = np.tril(np.ones((m, m), dtype=bool))
    np.testing.assert_allclose(got[:, lowm], ref[:, lowm], rtol=tol['rtol'], atol=tol['atol_rel'] * np.abs(ref).max())
    assert e_new <= e_tab


def test_training_step_is_unchanged(dev):
    """dpgp_elbo_step builds the table from fp32 distances as before; the separate calls' forward evaluation takes it from the K_uu blocks.
    Both against each other and against the all-fp64 gradients, tolerances of test_gpu_grad.test_training_step_equals_the_three_calls."""
    shape = (96, 3, 24, 10)
    n, d, m, q = shape
    args = _stage_b_problem(dev, shape)
    args[1] = args[1] * 0.6
    w3 = ops.ElboWorkspace(d, n, m, q, 'mixed', dev)
    terms3, sums3, info3 = [a.clone() for a in ops.elbo_fhat(*args, prec='mixed', workspace=w3)]
    gp, wk, gv, dab3, infog3 = ops.elbo_grad_chain(args[5], args[6], w3)
    g3 = [a.cpu().numpy() for a in ops.elbo_grad_psi(args[0], args[1], args[2], args[3], args[4], args[5], gp, wk, gv, prec='mixed')]
    w1 = ops.ElboWorkspace(d, n, m, q, 'mixed', dev)
    b1 = ops.ElboStepBuffers(d, n, m, q, dev)
    assert ops.elbo_step_supported(m, q)
    (terms1, sums1, info1), (dmu, ds, dz, dg, dab1, infog1) = ops.elbo_step(*args, workspace=w1, buffers=b1)
    assert int(info1.abs().max()) == 0 and int(info3.abs().max()) == 0
    assert int(infog1.abs().max()) == 0 and int(infog3.abs().max()) == 0
    assert torch.equal(w1.kuu(), w3.kuu()), 'both paths hold the same K_uu'
    t3 = terms3.cpu().numpy()
    np.testing.assert_allclose(terms1.cpu().numpy(), t3, rtol=0, atol=2e-5 * np.abs(t3).max())
    np.testing.assert_allclose(sums1.cpu().numpy(), sums3.cpu().numpy(), rtol=2e-6)
    w64 = ops.ElboWorkspace(d, n, m, q, 'f64', dev)
    ops.elbo_fhat(*args, prec='f64', workspace=w64)
    gp, wk, gv, dab64, _ = ops.elbo_grad_chain(args[5], args[6], w64)
    g64 = [a.cpu().numpy() for a in ops.elbo_grad_psi(args[0], args[1], args[2], args[3], args[4], args[5], gp, wk, gv, prec='f64')]
    for path, dab, grads in (('step', dab1, [a.cpu().numpy() for a in (dmu, ds, dz, dg)]), ('three calls', dab3, g3)):
        np.testing.assert_allclose(dab.cpu().numpy(), dab64.cpu().numpy(), rtol=0, atol=5e-4 * float(dab64.abs().max()), err_msg=path)
        for name, got, want in zip(('d mu', 'd S', 'd z', 'd gamma'), grads, g64):
            print('%s, %s: %.3g of the largest entry' % (name, path, np.abs(got - want).max() / np.abs(want).max()))
            np.testing.assert_allclose(got, want, rtol=0, atol=5e-4 * np.abs(want).max(), err_msg='%s, %s' % (name, path))
