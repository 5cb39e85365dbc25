"""
GPU tests of the pair-tile Psi2 kernel (csrc/psi2_pairs.hip) at the edges of its image build (phase A: every Q at which the
row layout of mu and s, the last K-step or the number of c'' pieces changes; rows off 16-byte boundaries), of its chunk loop
and of the column-operand refill between groups of resident pair tiles.

Helpers, reference (psi2_ld, longdouble) and tolerances are those of tests/test_gpu_psi2_edges.py.  The operator with fp32
inputs is called through the C ABI on a NaN-filled workspace (psi2_call).  With fp64 inputs the pair-tile kernel runs inside
the mixed-precision ELBO reduction only (psi2.hip has no operator entry with fp64 inputs and fp32 results): those cases hold
the five f_hat terms per output dim of ops.elbo_fhat(prec='mixed') to the CPU oracle (oracle.dpgp_oracle.fhat_terms, NumPy
fp64) at the tolerance tests/test_gpu_elbo.py holds the mixed reduction to against the same oracle's golden vectors.
"""
import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import _lib, ops
from oracle import dpgp_oracle as orc
from test_gpu_elbo import RTOL
from test_gpu_kernels import TOL_PSI2
from test_gpu_psi2_edges import (F32, F64, T, bits_equal, check, check_tol, npf, ordinary_case, ordinary_ref, psi2_call,
                                 psi2_ld, psi2_raw, reorder_tol)

pytestmark = pytest.mark.gpu

Q_LOADS = [1, 2, 3, 4, 5, 7, 10, 11, 16, 17, 20, 21]


def elbo_case(b, n, m, q):
    """ordinary_case with a y and a beta for the ELBO reduction.  At Q = 1 random inducing points share one latent dimension and
    K_uu is singular to working precision (the reduction flags it in info, in either precision): they are spread 1.5 apart."""
    z, mu, s, gam, al = ordinary_case(b, n, m, q)
    if q == 1:
        z = np.linspace(-0.75 * (m - 1), 0.75 * (m - 1), m).reshape(m, 1)
    rng = np.random.default_rng(77 + q)
    return dict(y=rng.standard_normal((n, b)), z=z, mu=mu, s=s, gamma=gam, alpha=al.reshape(-1),
                beta=np.exp(0.3 * rng.standard_normal(b)) * 4.0)


def elbo_terms(dev, p, prec, mu=None, s=None):
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=F64, device=dev)
    terms, sums, info = ops.elbo_fhat(t(p['y']), t(p['z']), t(p['mu']) if mu is None else mu, t(p['s']) if s is None else s,
                                      t(p['gamma']), t(p['alpha']), t(p['beta']), prec=prec)
    torch.cuda.synchronize()
    assert not info.cpu().numpy().any()
    return terms.cpu().numpy()


def oracle_terms(p):
    return orc.fhat_terms(p['y'], p['z'], p['mu'], p['s'], p['gamma'], p['alpha'], p['beta'])


def check_mixed(got, ref, what):
    err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    print('%-48s max|err|/max|ref| %.2e   (rtol %.1e)' % (what, err, RTOL['mixed']))
    np.testing.assert_allclose(got, ref, rtol=RTOL['mixed'], atol=RTOL['mixed'] * np.max(np.abs(ref)), err_msg=what)


def offset_view(a, dt, dev):
    """a [N, Q] as a contiguous view that starts 8 bytes into a larger allocation (which itself is 256-byte aligned)."""
    skip = 8 // (8 if dt == F64 else 4)
    buf = torch.full((a.size + skip + 64,), float('nan'), dtype=dt, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[skip:skip + a.size].view(a.shape)
    v.copy_(T(a, dt, dev))
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


# ---------------------------------------------------------------------------------------------------------------
# 1. load paths of phase A
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('q', Q_LOADS)
def test_phase_a_load_paths_f32(dev, q):
    """Q odd and even, Q % 4 != 0 (fp32 rows then start off 16-byte boundaries) and Q % 4 == 0, both sides of every KS step
    (5 | 7, 10 | 11, 16 | 17, 20 | 21).  N = 67 (two row tiles and 3 rows of a third), M = 9, B = 3."""
    got = psi2_call(dev, F32, 'auto', *ordinary_case(3, 67, 9, q))
    check_tol(got, ordinary_ref(3, 67, 9, q), F32, 'phase A, fp32 inputs, Q=%d' % q)


@pytest.mark.parametrize('q', Q_LOADS)
def test_phase_a_load_paths_f64(dev, q):
    """The same shapes with fp64 inputs (even Q: rows on 16-byte boundaries; odd Q: on 8-byte ones), through the mixed ELBO,
    against the CPU oracle."""
    p = elbo_case(3, 67, 9, q)
    check_mixed(elbo_terms(dev, p, 'mixed'), oracle_terms(p), 'phase A, fp64 inputs, Q=%d' % q)


@pytest.mark.parametrize('q', [4, 10, 16])
def test_phase_a_rows_off_16_bytes(dev, q):
    """mu and s as views 8 bytes into a larger allocation: rows whose starts are NOT 16-byte aligned although Q alone would put
    them there (fp32: Q = 4, 16; fp64: Q = 4, 10, 16).  Bitwise equal to the aligned call.  (A misaligned 16-byte global load
    does not fault on this hardware, so this pins results, not which loads a kernel issues.)"""
    z, mu, s, gam, al = ordinary_case(3, 67, 9, q)
    if q % 4 == 0:
        ts = [T(np.ascontiguousarray(a), F32, dev) for a in (z, mu, s, gam, al.reshape(-1))]
        rc, base = psi2_raw(dev, F32, 3, 67, 9, q, ts, _lib.ALGO['auto'])
        assert rc == 0
        ts[1], ts[2] = offset_view(mu, F32, dev), offset_view(s, F32, dev)
        rc, got = psi2_raw(dev, F32, 3, 67, 9, q, ts, _lib.ALGO['auto'])
        assert rc == 0
        check_tol(got, ordinary_ref(3, 67, 9, q), F32, 'phase A, fp32 rows at 8 mod 16, Q=%d' % q)
        assert bits_equal(got, base)
    p = elbo_case(3, 67, 9, q)
    base = elbo_terms(dev, p, 'mixed')
    got = elbo_terms(dev, p, 'mixed', mu=offset_view(mu, F64, dev), s=offset_view(s, F64, dev))
    check_mixed(got, oracle_terms(p), 'phase A, fp64 rows at 8 mod 16, Q=%d' % q)
    assert np.array_equal(got.view(np.int64), base.view(np.int64))


# ---------------------------------------------------------------------------------------------------------------
# 2. row edges
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [1, 31, 32, 33, 63, 65])
def test_row_edges(dev, n):
    """N = 1 .. 65 at Q = 10, M = 16, B = 2: threads without a row, rows past the end inside the last 32-row tile (they write
    exp2(-60000) = 0 rows), one, two and three row tiles (the peeled last row tile
    alone, behind one and behind two tiles of the loop)."""
    got = psi2_call(dev, F32, 'auto', *ordinary_case(2, n, 16, 10))
    check_tol(got, ordinary_ref(2, n, 16, 10), F32, 'rows N=%d' % n)
    p = elbo_case(2, n, 16, 10)
    check_mixed(elbo_terms(dev, p, 'mixed'), oracle_terms(p), 'rows N=%d, fp64 inputs' % n)


# ---------------------------------------------------------------------------------------------------------------
# 3. several chunks
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,q', [(545, 10), (1089, 10), (1200, 10), (289, 20), (600, 20)])
def test_several_chunks_identical_dims(dev, n, q, monkeypatch):
    """One n-split, so that a workgroup holds all N observations: N = 545 and 1089 are the first sizes needing two and three
    chunks at the 544-row limit of KS = 4 (Q = 10), N = 289 the first needing two at the 288-row limit of KS = 8 (Q = 20, G = 2,
    the deep-prefetch row loop); later chunks add to what the first stored.  M = 16 (136 pairs, 5 tiles), B = 4 output dims
    with IDENTICAL hyper-parameters: there is one chunk schedule, so all four results are bitwise equal; each is within
    TOL_PSI2 of the reference, and within the sum-reordering tolerance of the two-split result."""
    z, mu, s, gam, al = ordinary_case(1, n, 16, q)
    case = (z, mu, s, np.repeat(gam, 4, axis=0), np.repeat(al, 4, axis=0))
    ref = np.repeat(psi2_ld(z, mu, s, gam, al)[0], 4, axis=0)
    monkeypatch.setenv('DPGP_PSI2_NS', '1')
    got = psi2_call(dev, F32, 'auto', *case)
    check_tol(got, ref, F32, 'chunks N=%d Q=%d' % (n, q))
    for b in range(1, 4):
        assert bits_equal(got[b], got[0]), 'output dims with identical inputs differ: %d' % b
    monkeypatch.setenv('DPGP_PSI2_NS', '2')
    two = psi2_call(dev, F32, 'auto', *case)
    check(two, npf(got), reorder_tol(F32, n), TOL_PSI2[F32]['atol_rel'], 'chunks N=%d Q=%d, two splits against one' % (n, q))


# ---------------------------------------------------------------------------------------------------------------
# 4. group refill
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('q,m', [(10, 33), (10, 40), (10, 57), (16, 48), (20, 24), (20, 40)])
def test_group_refill(dev, q, m, monkeypatch):
    """The next group's column operands are fetched through the last row tile of a group, and only where a further FULL group
    follows in the wave's tile range (wave w starts at tile t0 + w, a group takes tiles 4 apart; a refill needs tb + 4 (2 G - 1)
    < t1).  N = 96 (three row tiles), one tile range unless said otherwise:
      Q = 10 (KS = 4, G = 6): M = 33, 40 (18, 26 tiles): 0 and 1 full group per wave plus every leftover shape, no refill;
                              M = 57 (52 tiles, 13 per wave): two full groups, one refill, one leftover tile;
      Q = 16 (KS = 6, G = 4): M = 48 (37 tiles, 9 - 10 per wave): two full groups, one refill, leftovers of 1 and 2;
      Q = 20 (KS = 8, G = 2, the deep-prefetch row loop): M = 24 (10 tiles, 2 - 3 per wave): one group, no refill;
                              M = 40 (26 tiles, 6 - 7 per wave): three groups, two refills, a leftover tile on two waves.
    With DPGP_PP_RANGES = 2 every range ends inside the tile list and the groups fall differently (M = 57: no refill left;
    Q = 20, M = 40: one per wave): a refill that reached past its range's t1 would fetch the next range's tiles or read past
    the image.  The ranges partition the pairs without changing a sum's order, so the results are bitwise equal.  Eight waves
    (tiles 8 apart) once more, against the reference."""
    case = ordinary_case(2, 96, m, q)
    ref = ordinary_ref(2, 96, m, q)
    monkeypatch.setenv('DPGP_PP_RANGES', '1')
    base = psi2_call(dev, F32, 'auto', *case)
    check_tol(base, ref, F32, 'refill Q=%d M=%d one range' % (q, m))
    monkeypatch.setenv('DPGP_PP_RANGES', '2')
    got = psi2_call(dev, F32, 'auto', *case)
    check_tol(got, ref, F32, 'refill Q=%d M=%d two ranges' % (q, m))
    assert bits_equal(got, base)
    monkeypatch.setenv('DPGP_PP_RANGES', '1')
    monkeypatch.setenv('DPGP_PP_NW', '8')
    eight = psi2_call(dev, F32, 'auto', *case)
    check_tol(eight, ref, F32, 'refill Q=%d M=%d eight waves' % (q, m))
