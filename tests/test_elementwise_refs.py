"""
CPU checks of the longdouble references that tests/test_gpu_elementwise_edges.py judges the HIP kernels by: on the golden
inputs (|x| < 4, where the oracle's expanded form is accurate) they agree with the oracle to 1e-13 of the largest entry for
all flag combinations and with the stored reference outputs at the fp64 tolerance of test_gpu_kernels; the case tables of
the GPU file cover every size its docstrings promise; the KL tolerance holds for the oracle's own fp64 sum.
"""
import numpy as np
import pytest
import torch

from conftest import golden
from oracle import dpgp_oracle as orc
import test_gpu_elementwise_edges as E
from test_gpu_kernels import TOL

COMBOS = {'xx': ('x0', None), 'x01': ('x0', 'x1'), 'x10': ('x1', 'x0'), 'uu_same': ('x_u', 'x_u'), 'uu': ('x_u', None)}


def rel_to_largest(a, b):
    return float(np.max(np.abs(a - b))) / float(np.max(np.abs(b)))


@pytest.mark.parametrize('fixture', ['kernel_b1', 'kernel_b7'])
def test_longdouble_references_agree_with_oracle_and_fixtures(fixture):
    g = golden(fixture)
    gam, al, be = g['gamma'], g['alpha'], g['beta']
    t64 = TOL[torch.float64]
    for tag, (a, c) in COMBOS.items():
        x1 = None if c is None else g[c]
        for noise in (False, True):
            for jit in (False, True):
                got, xe = E.gram_ld(g[a], x1, gam, al, be, noise, jit)
                want = orc.ard_rbf_gram(g[a], x1, gam, al, be, noise, jit)
                assert got.dtype == np.float64 and xe.shape == got.shape and (xe <= 0).all()
                assert rel_to_largest(got, want) <= 1e-13, (tag, noise, jit)
                stored = g['gram_%s_n%d_j%d' % (tag, noise, jit)]
                np.testing.assert_allclose(got, stored, rtol=t64['rtol'], atol=t64['atol_rel'] * np.abs(stored).max())
        # a non-default jitter and the exponent itself
        got, xe = E.gram_ld(g[a], x1, gam, al, be, True, True, jitter=3e-3)
        assert rel_to_largest(got, orc.ard_rbf_gram(g[a], x1, gam, al, be, True, True, jitter=3e-3)) <= 1e-13
        plain, _ = E.gram_ld(g[a], x1, gam, al)
        np.testing.assert_allclose(plain, np.asarray(al).reshape(-1, 1, 1) * np.exp(xe), rtol=1e-13)
    z, mu, s = g['x_u'], g['x_mean'], g['x_var']
    p1, ex = E.psi1_ld(z, mu, s, gam, al)
    assert rel_to_largest(p1, orc.psi1(z, mu, s, gam, al)) <= 1e-13
    np.testing.assert_allclose(p1, g['psi_1'], rtol=t64['rtol'], atol=t64['atol_rel'] * np.abs(g['psi_1']).max())
    np.testing.assert_allclose(p1, np.asarray(al).reshape(-1, 1, 1) * np.exp(ex), rtol=1e-13)
    y = np.random.default_rng(3).standard_normal((mu.shape[0], np.atleast_2d(gam).shape[0]))
    assert rel_to_largest(E.psi1T_y_ld(z, mu, s, gam, al, y), orc.psi1T_y(z, mu, s, gam, al, y)) <= 1e-13


def test_kernel_arithmetic_emulation_is_a_gram():
    """gram_emulated (the yardstick of the exponent sweep and of the far-from-origin test) computes the gram: at the origin
    it meets the kernels' own tolerances against gram_ld."""
    g = golden('kernel_b7')
    ref, _ = E.gram_ld(g['x0'], g['x1'], g['gamma'], g['alpha'])
    for ft, dt in ((np.float64, torch.float64), (np.float32, torch.float32)):
        emu = E.gram_emulated(g['x0'], g['x1'], g['gamma'], g['alpha'], ft)
        assert emu.dtype == ft
        np.testing.assert_allclose(emu, ref, rtol=TOL[dt]['rtol'], atol=TOL[dt]['atol_rel'] * ref.max())


def test_case_tables_cover_every_size():
    assert {s[1] for s in E.PSI1_SHAPES} == set(E._P1_NS) and {s[2] for s in E.PSI1_SHAPES} == set(E._P1_MS)
    assert {s[3] for s in E.PSI1_SHAPES} == set(E._P1_QS) and {s[0] for s in E.PSI1_SHAPES} == set(E._P1_BS)
    assert 25 <= len(set(E.PSI1_SHAPES)) <= 35
    assert {s[1] for s in E.P1Y_SHAPES_F64} == set(E._PY_NS) and {s[2] for s in E.P1Y_SHAPES_F64} == set(E._PY_MS)
    assert {s[3] for s in E.P1Y_SHAPES_F64} == {1, 30} and {s[0] for s in E.P1Y_SHAPES_F64} == {1, 3}
    for k in range(1, 7):               # both edges of each K-step instantiation's Q range (the lower edge of the first is Q = 1,
        qs = [q for q in range(1, 31) if -(-(6 * q + 2) // 32) == k]      # which test_psi_statistics_vs_oracle_ragged runs)
        assert qs[-1] in E.P1Y_QS_F32 and (k == 1 or qs[0] in E.P1Y_QS_F32), (k, qs)


@pytest.mark.parametrize('shape', E.KL_SHAPES)
def test_kl_tolerances_hold_for_the_oracles_fp64_sum(shape):
    for ft, rtol in ((np.float64, 1e-12), (np.float32, 1e-6)):
        mu, s = E.kl_inputs(shape[0], shape[1], ft)
        ref = E.kl_ld(mu, s)
        assert ref > 0
        np.testing.assert_allclose(orc.kl_qx(mu, s), ref, rtol=rtol)
        # conditioning: the sum of the terms' magnitudes over the result (1 = no cancellation at all)
        cond = float(np.sum(mu * mu + s + np.abs(np.log(s)) + 1.0)) * 0.5 / ref
        assert cond < 100.0, cond
