"""
CPU checks of what tests/test_gpu_psi2_edges.py judges the forward Psi2 kernels by: its longdouble reference against the
oracle and the stored reference outputs; the CPU emulations of the pair-tile and the patch kernel's operand arithmetic against
the pair kernel's documented accuracy model on exactly the inputs of the far-from-the-centre tests; and psi2_nsplit, observed
through the host-only dpgp_psi2_workspace_bytes.
"""
import numpy as np
import pytest

from conftest import golden
from dp_gp_lvm_amd import _lib
from oracle import dpgp_oracle as orc
import test_gpu_psi2_edges as P


@pytest.mark.parametrize('fixture', ['kernel_b1', 'kernel_b7'])
def test_longdouble_reference_agrees_with_oracle_and_fixtures(fixture):
    g = golden(fixture)
    args = (g['x_u'], g['x_mean'], g['x_var'], g['gamma'], g['alpha'])
    ref, cmax = P.psi2_ld(*args)
    want = orc.psi2(*args)
    assert ref.dtype == np.float64 and ref.shape == want.shape and cmax.shape == (want.shape[0],)
    np.testing.assert_allclose(ref, want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(ref, g['psi_2'], rtol=1e-12, atol=0)
    assert (ref == ref.transpose(0, 2, 1)).all() and (cmax > 0).all()
    assert P.psi2_ld(*args)[0] is ref, 'memoised'
    # a second shape through the chunked path of the oracle, and the row constant against its definition in fp64
    z, mu, s, gam, al = P.ordinary_case(2, 70, 40, 6)
    ref, cmax = P.psi2_ld(z, mu, s, gam, al)
    np.testing.assert_allclose(ref, orc.psi2(z, mu, s, gam, al), rtol=1e-12, atol=0)
    for b in range(2):
        np.testing.assert_allclose(cmax[b], P.pair_guard_quantity(z, mu, s, gam[b]).max(), rtol=1e-12)


def test_emulations_compute_the_exponent():
    """At ordinary geometry both emulations reproduce the exact exponent to fp32 accuracy (a few 1e-6 in log2 units)."""
    z, mu, s, gam, _ = P.ordinary_case(2, 70, 40, 6)
    for b in range(2):
        assert P.pairs_emulated(z, mu, s, gam[b])['err'] < 2e-5
        assert P.patch_emulated(z, mu, s, gam[b])['err'] < 2e-5


def test_pair_kernel_emulation_stays_below_the_documented_model():
    """The documented model of the pair-tile kernel — exponent good to |c''| 2^-21 — holds for the emulation of its operand
    arithmetic on the exact inputs of test_far_from_the_centre_pair_kernel, for every Q 1 - 21, Q = 5 and Q = 21 (two c''
    pieces) included: the GPU test's bound of twice the model leaves the factor 2 to what the emulation does not model."""
    ratios = {}
    for q in range(1, 22):
        emu = P.far_pairs_emulation(q)
        assert [e['three'] for e in emu] == [q not in (5, 21)] * P.FAR_B
        assert emu[0]['ks'] == (2 if q <= 5 else 4 if q <= 10 else 6 if q <= 15 else 8)
        _, cmax = P.psi2_ld(*P.far_case(q))
        for b, e in enumerate(emu):
            assert abs(e['cmax'] / cmax[b] - 1.0) < 1e-5        # the fp32 c'' of the emulation is the reference's c''
            assert 100.0 < e['cmax'] < P.PAIR_GUARD
        ratios[q] = max(e['ratio'] for e in emu)
    print('pair emulation, max error / (max|c\'\'| 2^-21) by Q:', ' '.join('%d: %.2f' % kv for kv in ratios.items()))
    assert max(ratios.values()) < 1.0, ratios
    assert min(ratios.values()) > 0.1, ratios          # the model is not slack by an order of magnitude either


def test_patch_kernel_emulation_measured_maximum():
    """The maximum exponent error of the patch kernel's emulation on the inputs of test_far_from_the_centre_other_kernels (the
    GPU test takes twice this as its bound): the recorded figures, in log2 units, and max |P| inside the kernel's +-30000 clamp."""
    recorded = {1: 7.5e-5, 5: 2.2e-4, 10: 3.8e-4, 21: 8.6e-4, 30: 9.0e-4}
    assert sorted(recorded) == P.FAR_PATCH_QS
    for q in P.FAR_PATCH_QS:
        emu = P.far_patch_emulation(q)
        err = max(e['err'] for e in emu)
        print('patch emulation Q=%d: max exponent error %.2e (max|P| %.0f, max|c\'| %.0f)'
              % (q, err, max(e['pmax'] for e in emu), max(e['cprime'] for e in emu)))
        assert 0.9 * recorded[q] < err < 1.1 * recorded[q], (q, err)
        assert max(e['pmax'] for e in emu) < P.PATCH_GUARD


def test_guard_cases_sit_where_they_should():
    for kernel, (q, _, quantity, line) in P.GUARDS.items():
        for factor in (0.98, 1.02):
            z, mu, s, gam, _ = P.guard_case(kernel, factor)
            got = quantity(z, mu, s, gam[0])
            assert abs(got[P.GUARD_ROW] / line - factor) < 1e-4
            assert mu.shape == (40, q) and (P.r32(mu) == mu).all()


# ---------------------------------------------------------------------------------------------------------------
# psi2_nsplit through dpgp_psi2_workspace_bytes
# ---------------------------------------------------------------------------------------------------------------

def nsplit(b, n, m, elem=4, q=3):
    """Mp^2 is a multiple of 256, so the slab term of the workspace is not padded and the other two terms do not depend on
    N: ns = 1 + (bytes(N) - bytes(N = 1)) / (elem B Mp^2) exactly (N = 1 always has one split)."""
    w = _lib.lib().dpgp_psi2_workspace_bytes
    mp = -(-m // 16) * 16
    extra = int(w(b, n, m, q, elem)) - int(w(b, 1, m, q, elem))
    assert extra % (elem * b * mp * mp) == 0
    return 1 + extra // (elem * b * mp * mp)


def test_nsplit_automatic_cases(monkeypatch):
    monkeypatch.delenv('DPGP_PSI2_NS', raising=False)
    for elem in (4, 8):
        assert nsplit(2, 1100, 33, elem) > 1
        assert nsplit(2, 700, 200, elem) > 1
        assert nsplit(130, 260, 17, elem) >= 1
        for n in (1, 10, 127, 255):                    # the automatic rule keeps >= 128 rows per split
            assert nsplit(2, n, 33, elem) == 1
    for n in range(1, 3000, 37):
        for b, m in ((1, 20), (2, 33), (64, 100), (130, 17), (2, 200), (600, 40)):
            ns = nsplit(b, n, m)
            assert ns == 1 or (2 <= ns <= 8 and n >= 128 * ns), (b, n, m, ns)


def test_nsplit_override_never_leaves_a_split_empty(monkeypatch):
    """DPGP_PSI2_NS takes effect, and is stepped down to the largest count for which every split of ceil(N / ns) rows — the
    pair-tile kernel's — starts before the last observation."""
    for ns in (1, 2, 3, 5, 8):
        monkeypatch.setenv('DPGP_PSI2_NS', str(ns))
        for n in (57, 64, 65, 100):
            assert nsplit(2, n, 33) == ns and nsplit(2, n, 33, 8) == ns
    for want in range(1, 9):
        monkeypatch.setenv('DPGP_PSI2_NS', str(want))
        for n in range(1, 301):
            ns = nsplit(2, n, 33)
            assert 1 <= ns <= want
            assert (ns - 1) * -(-n // ns) < n, (n, want, ns)
            assert all((v - 1) * -(-n // v) >= n for v in range(ns + 1, min(want, n) + 1)), (n, want, ns)
    monkeypatch.setenv('DPGP_PSI2_NS', '8')
    assert nsplit(2, 10, 33) == 5                      # the over-split cases of the GPU file: 8 x 2 rows -> 5 x 2 rows
    monkeypatch.setenv('DPGP_PSI2_NS', '7')
    assert nsplit(2, 20, 33) == 7                      # (7 x 3 rows: the last split starts at 18)
