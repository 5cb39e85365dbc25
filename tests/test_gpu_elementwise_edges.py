"""
GPU tests of the first-layer operators (csrc/elementwise.hip: ard_rbf_gram, ard_rbf_diag, psi0, psi1, psi1T_y, kl_qx) at
tile and store edges, at every dispatch boundary and over the whole exponent range of their hand-written exponentials.

References are plain NumPy in np.longdouble (gram_ld, psi1_ld, psi1T_y_ld, kl_ld below; tests/test_elementwise_refs.py
pins them against the oracle and the golden fixtures on the CPU).  The gram reference is the DIRECT squared-difference
form: the oracle restates the reference's expanded form (|a|^2 + |b|^2 - 2 a.b), whose own error grows with the square of
the distance from the origin and cannot judge the kernel there.

Unless a test says otherwise every random input is rounded to fp32 first, so that the fp64 and the fp32 operator see the
same numbers and share one reference.  Tolerances are test_gpu_kernels.TOL unless stated.  Each case prints its observed
maximum error.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import golden  # noqa: F401  (the golden inputs are used by the CPU sibling of this file)
from dp_gp_lvm_amd import ops
from oracle import dpgp_oracle as orc
from test_gpu_kernels import TOL

pytestmark = pytest.mark.gpu

LD = np.longdouble
F64, F32 = torch.float64, torch.float32
DTYPES = [F64, F32]
NP_OF = {F64: np.float64, F32: np.float32}
JITTER = 3e-3
LOG2E = 1.4426950408889634
FLAGS = [(False, False), (True, False), (False, True), (True, True)]


# ---------------------------------------------------------------------------------------------------------------
# references (NumPy, longdouble)
# ---------------------------------------------------------------------------------------------------------------

def _hyp_ld(gamma, alpha):
    return np.atleast_2d(np.asarray(gamma, dtype=np.float64)).astype(LD), np.asarray(alpha, dtype=np.float64).reshape(-1).astype(LD)


def gram_ld(x0, x1, gamma, alpha, beta=None, include_noise=False, include_jitter=False, jitter=orc.GP_DEFAULT_JITTER):
    """alpha_b exp(x_e), x_e[b,i,j] = -1/2 sum_q gamma_bq (x0_iq - x1_jq)^2 with differences, products and the sum in
    longdouble -> (K [B,N0,N1] fp64, x_e fp64).  Noise and jitter go on the diagonal in fp64 exactly as
    oracle.ard_rbf_gram adds them, and only when x1 is None."""
    g, al = _hyp_ld(gamma, alpha)
    a = np.asarray(x0, dtype=np.float64).astype(LD)
    c = a if x1 is None else np.asarray(x1, dtype=np.float64).astype(LD)
    d = a[:, None, :] - c[None, :, :]                                              # [N0,N1,Q]
    xe = np.stack([LD(-0.5) * np.sum(d * d * g[b][None, None, :], axis=-1) for b in range(g.shape[0])])
    k = (al[:, None, None] * np.exp(xe)).astype(np.float64)
    if x1 is None:
        eye = np.eye(a.shape[0])
        if include_noise:
            k = k + (1.0 / np.asarray(beta, dtype=np.float64).reshape(-1))[:, None, None] * eye
        if include_jitter:
            k = k + jitter * eye
    return k, xe.astype(np.float64)


def psi1_ld(z, mu, s, gamma, alpha, keep_ld=False):
    """The log-form of oracle.psi1 in longdouble -> (psi1 [B,N,M], its exponent log(psi1 / alpha)); fp64 unless keep_ld."""
    g, al = _hyp_ld(gamma, alpha)
    z, mu, s = (np.asarray(a, dtype=np.float64).astype(LD) for a in (z, mu, s))
    sqd = np.square(mu[:, None, :] - z[None, :, :])                                # [N,M,Q]
    out, ex = [], []
    for b in range(g.shape[0]):
        den = g[b][None, :] * s + LD(1)                                            # [N,Q]
        e = np.sum(sqd * (g[b][None, :] / den)[:, None, :], axis=-1) + np.sum(np.log(den), axis=-1)[:, None]
        ex.append(LD(-0.5) * e)
        out.append(np.exp(np.log(al[b]) + ex[-1]))
    out, ex = np.stack(out), np.stack(ex)
    return (out, ex) if keep_ld else (out.astype(np.float64), ex.astype(np.float64))


def psi1T_y_ld(z, mu, s, gamma, alpha, y):
    """sum_n psi1[b,n,m] y[n,b] with psi1 and the sum in longdouble -> [B,M] fp64."""
    p1, _ = psi1_ld(z, mu, s, gamma, alpha, keep_ld=True)
    return np.einsum('bnm,nb->bm', p1, np.asarray(y, dtype=np.float64).astype(LD)).astype(np.float64)


def kl_ld(mu, s):
    """oracle.kl_qx with the sums in longdouble."""
    mu, s = np.asarray(mu, dtype=np.float64).astype(LD), np.asarray(s, dtype=np.float64).astype(LD)
    return float(LD(0.5) * (np.sum(mu * mu) + np.sum(s - np.log(s)) - LD(mu.shape[0] * mu.shape[1])))


def gram_emulated(x0, x1, gamma, alpha, ft):
    """The gram kernel's own arithmetic in NumPy at precision ft (np.float32 / np.float64), on the CPU: inputs pre-scaled by
    sqrt(gamma), subtracted, squares accumulated one latent dimension after the other (the kernel's fma is a product that is
    exact in the wider type, rounded once with the sum), scaled by -1/2 log2 e, exp2, times alpha."""
    wide = np.float64 if ft == np.float32 else LD
    g = np.atleast_2d(np.asarray(gamma)).astype(ft)
    al = np.asarray(alpha).reshape(-1).astype(ft)
    x0, x1 = np.asarray(x0).astype(ft), np.asarray(x1).astype(ft)
    out = np.empty((g.shape[0], x0.shape[0], x1.shape[0]), dtype=ft)
    for b in range(g.shape[0]):
        sg = np.sqrt(g[b])
        a, c = sg[None, :] * x0, sg[None, :] * x1
        acc = np.zeros((x0.shape[0], x1.shape[0]), dtype=ft)
        for q in range(g.shape[1]):
            d = (a[:, None, q] - c[None, :, q]).astype(ft)
            acc = (d.astype(wide) * d.astype(wide) + acc.astype(wide)).astype(ft)
        out[b] = al[b] * np.exp2(ft(-0.5 * LOG2E) * acc).astype(ft)
    return out


# ---------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------

def r32(a):
    """Rounded to fp32 and back: the fp64 and fp32 operators then see identical inputs."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def T(a, dt, dev):
    return torch.as_tensor(np.asarray(a), dtype=dt, device=dev)


def npf(t):
    return t.detach().cpu().numpy().astype(np.float64)


def check(got, ref, tol, what):
    """test_gpu_kernels.close, printing the observed errors first."""
    got = npf(got) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    big = float(np.max(np.abs(ref)))
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.where(np.abs(ref) > tol['atol_rel'] * big / max(tol['rtol'], 1e-300), err / np.abs(ref), 0.0)
    print('%-58s max|err|/max|ref| %.2e   max rel.err (entries above the atol floor) %.2e'
          % (what, float(np.nanmax(err)) / max(big, 1e-300), float(np.nanmax(rel))))
    np.testing.assert_allclose(got, ref, rtol=tol['rtol'], atol=tol['atol_rel'] * big, err_msg=what)


def bits_equal(a, b):
    """Bit-for-bit equality that also holds for NaN payloads and signed zeros."""
    it = torch.int64 if a.dtype == F64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def hyper(rng, b, q):
    """Per-kernel hyperparameters, all distinct: gamma log-normal / max(1, Q/4) (so that gram entries stay O(1e-3..1)),
    alpha and beta log-normal."""
    gam = r32(np.exp(0.5 * rng.standard_normal((b, q))) / max(1.0, q / 4.0))
    al = r32(np.exp(0.3 * rng.standard_normal((b, 1))) * (1.0 + 0.25 * np.arange(b))[:, None])
    be = r32(np.exp(0.3 * rng.standard_normal((b, 1))) * (2.0 + 0.5 * np.arange(b))[:, None])
    return gam, al, be


# ---------------------------------------------------------------------------------------------------------------
# gram: tile and store edges
# ---------------------------------------------------------------------------------------------------------------
GRAM_SHAPES = [(1, 1), (1, 5), (3, 64), (4, 4), (63, 65), (64, 64), (65, 63), (64, 128), (129, 68), (131, 131)]
GRAM_QS = [1, 2, 3, 4, 5, 29, 30]


@functools.lru_cache(maxsize=None)
def gram_case(n0, n1, q, b):
    rng = np.random.default_rng(100000 * n0 + 1000 * n1 + 10 * q + b)
    x0, x1 = r32(rng.standard_normal((n0, q))), r32(rng.standard_normal((n1, q)))
    gam, al, be = hyper(rng, b, q)
    ref01, _ = gram_ld(x0, x1, gam, al)
    sym = None
    if n0 == n1:
        ref00, _ = gram_ld(x0, x0, gam, al)
        sym = {fl: gram_ld(x0, None, gam, al, be, fl[0], fl[1], JITTER)[0] for fl in FLAGS}
        sym['same'] = ref00
    return x0, x1, gam, al, be, ref01, sym


@pytest.mark.parametrize('dt', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('b', [1, 3])
@pytest.mark.parametrize('shape', GRAM_SHAPES, ids=lambda s: '%dx%d' % s)
def test_gram_tile_and_store_edges(dev, shape, b, dt):
    """N0, N1 of 1, below 4, on and one past the 64-wide tile; Q below 4 (idle fill groups) and at 29 / 30; leading dimensions
    that are multiples of 4 with a ragged last tile (vector against element stores); distinct alpha / beta per kernel and a
    non-default jitter.  With x1 given nothing is added to the diagonal, flags set or not, even when x1 is x0 itself."""
    n0, n1 = shape
    for q in GRAM_QS:
        x0, x1, gam, al, be, ref01, sym = gram_case(n0, n1, q, b)
        tx0, tx1, tg, ta, tb = (T(a, dt, dev) for a in (x0, x1, gam, al, be))
        tag = 'gram %dx%d Q=%d B=%d ' % (n0, n1, q, b)
        check(ops.ard_rbf_gram(tx0, tx1, tg, ta, tb, jitter=JITTER), ref01, TOL[dt], tag + 'x1')
        check(ops.ard_rbf_gram(tx0, tx1, tg, ta, tb, True, True, jitter=JITTER), ref01, TOL[dt], tag + 'x1, flags set')
        if sym is not None:
            for fl in FLAGS:
                check(ops.ard_rbf_gram(tx0, None, tg, ta, tb, fl[0], fl[1], jitter=JITTER), sym[fl], TOL[dt],
                      tag + 'x1=None n%d j%d' % fl)
            check(ops.ard_rbf_gram(tx0, tx0, tg, ta, tb, jitter=JITTER), sym['same'], TOL[dt], tag + 'x1 is x0')
            check(ops.ard_rbf_gram(tx0, tx0, tg, ta, tb, True, True, jitter=JITTER), sym['same'], TOL[dt],
                  tag + 'x1 is x0, flags set')


@pytest.mark.parametrize('dt', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('n,q', [(4, 1), (5, 3), (64, 30), (65, 4), (131, 29)])
def test_gram_exact_properties(dev, n, q, dt):
    """x1=None: exactly symmetric; the diagonal is alpha_b without flags and alpha_b + 1/beta_b + jitter, evaluated in the
    tensor's type in that order (the reference adds the noise matrix, then the jitter matrix), with them; two duplicated
    rows give exactly alpha_b off the diagonal; two calls are bit-identical."""
    b = 3
    rng = np.random.default_rng(7000 + 10 * n + q)
    x = r32(rng.standard_normal((n, q)))
    x[n - 1] = x[0]                                                                # duplicated rows 0 and n-1
    gam, al, be = hyper(rng, b, q)
    tx, tg, ta, tb = (T(a, dt, dev) for a in (x, gam, al, be))
    al_t, be_t = ta.reshape(-1).cpu(), tb.reshape(-1).cpu()
    jit_t = torch.tensor(JITTER, dtype=dt)
    for noise, jit in FLAGS:
        k = ops.ard_rbf_gram(tx, None, tg, ta, tb, noise, jit, jitter=JITTER)
        k2 = ops.ard_rbf_gram(tx, None, tg, ta, tb, noise, jit, jitter=JITTER)
        assert bits_equal(k, k2), 'two calls differ'
        assert torch.equal(k, k.transpose(1, 2)), 'gram is not exactly symmetric'
        want = al_t.clone()
        if noise:
            want = want + 1.0 / be_t
        if jit:
            want = want + jit_t
        diag = torch.diagonal(k, dim1=1, dim2=2).cpu()
        dev_ulp = float(((diag - want[:, None]).abs() / want[:, None]).max()) / float(torch.finfo(dt).eps)
        print('gram N=%d Q=%d n%d j%d: diagonal off by %.2f eps' % (n, q, noise, jit, dev_ulp))
        assert torch.equal(diag, want[:, None].expand(b, n)), 'diagonal != alpha (+ 1/beta) (+ jitter) in that order'
        if n > 1:
            assert torch.equal(k[:, 0, n - 1].cpu(), al_t), 'duplicated rows must give exactly alpha'


# ---------------------------------------------------------------------------------------------------------------
# gram: exponent range
# ---------------------------------------------------------------------------------------------------------------
SWEEP_DEPTH = {F64: 765.0, F32: 95.0}     # natural-log units: just past 2^-1100 (762.5) and 2^-126 (87.3)


@functools.lru_cache(maxsize=None)
def sweep_case(q, deep):
    """Rows of x0 / x1 scaled by a ramp, then all of it rescaled so that the most negative exponent is -deep."""
    n0, n1, b = 130, 67, 2
    rng = np.random.default_rng(4200 + q)
    x0 = rng.standard_normal((n0, q)) * np.sqrt(np.linspace(0.0, 1.0, n0))[:, None]
    x1 = rng.standard_normal((n1, q)) * np.sqrt(np.linspace(0.0, 1.0, n1))[:, None]
    gam, al, _ = hyper(rng, b, q)
    _, xe = gram_ld(x0, x1, gam, al)
    f = np.sqrt(deep / float(np.max(-xe)))
    x0, x1 = r32(f * x0), r32(f * x1)
    ref, xe = gram_ld(x0, x1, gam, al)
    return x0, x1, gam, al, ref, xe


def sweep_f32_constant(q):
    """2 x the worst  err / (2^-24 max(1, |x_e|))  of the fp32 emulation of the kernel's arithmetic against gram_ld."""
    x0, x1, gam, al, ref, xe = sweep_case(q, SWEEP_DEPTH[F32])
    emu = gram_emulated(x0, x1, gam, al, np.float32).astype(np.float64)
    ok = ref >= 1e-37
    worst = float(np.max((np.abs(emu - ref) / ref / (2.0 ** -24 * np.maximum(1.0, np.abs(xe))))[ok]))
    return worst, 2.0 * worst


@pytest.mark.parametrize('q', [1, 10, 30])
def test_gram_exponent_sweep_f64(dev, q):
    """Exponents from 0 down to -765 (2^-1104: past the -1100 clamp of dpgp_exp2_tab): rtol 1e-10 per entry wherever the
    reference is >= 2^-1000, the file's atol below; every output finite and >= 0."""
    x0, x1, gam, al, ref, xe = sweep_case(q, SWEEP_DEPTH[F64])
    got = npf(ops.ard_rbf_gram(*(T(a, F64, dev) for a in (x0, x1, gam, al, al))))
    assert np.isfinite(got).all() and (got >= 0).all()
    atol = TOL[F64]['atol_rel'] * float(ref.max())
    big = ref >= 2.0 ** -1000
    rel = np.abs(got - ref)[big] / ref[big]
    print('gram sweep f64 Q=%d: exponents %.1f..%.1f, %d of %d entries >= 2^-1000, max rel.err %.2e, max |err| below %.2e'
          % (q, xe.min(), xe.max(), int(big.sum()), big.size, rel.max(), float(np.abs(got - ref)[~big].max(initial=0.0))))
    assert int((~big).sum()) > 0 and float(xe.min()) < -1100 * np.log(2.0), 'the sweep must pass the clamp'
    assert rel.max() <= 1e-10
    assert (np.abs(got - ref)[~big] <= atol).all()


@pytest.mark.parametrize('q', [1, 10, 30])
def test_gram_exponent_sweep_f32(dev, q):
    """Exponents from 0 down to -95 (2^-137: past the 2^-126 flush of v_exp_f32).  A relative error delta of the argument x_e
    becomes |x_e| delta in exp(x_e), so the bound per entry with reference >= 1e-37 is  2e-5 + c 2^-24 |x_e|  relative, with
    c = 2 x the worst err / (2^-24 max(1, |x_e|)) of the NumPy float32 emulation of the kernel's arithmetic (gram_emulated)
    on these same inputs, computed here on the CPU.  Measured for the committed inputs:
        Q = 1: emulation 7.61, c = 15.2;   Q = 10: emulation 6.49, c = 13.0;   Q = 30: emulation 8.32, c = 16.6.
    Everything is finite and >= 0; entries whose reference is below 1e-37 only have to be below 2e-37."""
    x0, x1, gam, al, ref, xe = sweep_case(q, SWEEP_DEPTH[F32])
    worst, c = sweep_f32_constant(q)
    got = npf(ops.ard_rbf_gram(*(T(a, F32, dev) for a in (x0, x1, gam, al, al))))
    assert np.isfinite(got).all() and (got >= 0).all()
    ok = ref >= 1e-37
    rel = np.abs(got - ref)[ok] / ref[ok]
    bound = 2e-5 + c * 2.0 ** -24 * np.abs(xe)[ok]
    print('gram sweep f32 Q=%d: exponents %.1f..%.1f, emulation %.3f -> c = %.3f; max rel.err %.2e, max err / bound %.3f'
          % (q, xe.min(), xe.max(), worst, c, rel.max(), float((rel / bound).max())))
    assert float(xe.min()) < -126 * np.log(2.0) and int((~ok).sum()) > 0, 'the sweep must pass the flush threshold'
    assert (rel <= bound).all()
    assert (got[~ok] <= 2e-37).all()


@pytest.mark.parametrize('dt', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('sep', [2000.0, 1e8])
def test_gram_past_the_clamp(dev, sep, dt):
    """Two clusters 2000 and 1e8 length scales apart along the first latent dimension (gamma = 1, Q = 3, 70 points a side):
    arguments of about -3e6 and -7e15.  Cross-cluster entries are exactly 0, nothing is NaN or inf.  Within a cluster the
    pre-scale by sqrt(1) and the differences of neighbouring numbers are exact, so the offset costs nothing and the file's
    tolerance holds against gram_ld on the inputs as stored in the tensor's type."""
    rng = np.random.default_rng(int(sep) % 1000 + 11)
    n, q, b = 70, 3, 2
    far = np.arange(n) % 2 == 1                                                    # alternate rows: both clusters in every tile
    x0, x1 = rng.standard_normal((n, q)), rng.standard_normal((n, q))
    x0[far, 0] += sep
    x1[far, 0] += sep
    x0, x1 = (a.astype(NP_OF[dt]).astype(np.float64) for a in (x0, x1))
    gam = np.ones((b, q))
    _, al, be = hyper(rng, b, q)
    tg, ta, tb = (T(a, dt, dev) for a in (gam, al, be))
    cross = far[:, None] != far[None, :]
    for tag, xb in (('x1', x1), ('x1=None', None)):
        ref, xe = gram_ld(x0, xb, gam, al)
        got = npf(ops.ard_rbf_gram(T(x0, dt, dev), None if xb is None else T(xb, dt, dev), tg, ta, tb))
        assert np.isfinite(got).all()
        print('gram clusters %g apart (%s): cross-cluster exponents down to %.2e' % (sep, tag, xe[:, cross].min()))
        assert (got[:, cross] == 0.0).all(), 'cross-cluster entries must be exactly 0'
        check(got[:, ~cross], ref[:, ~cross], TOL[dt], 'gram clusters %g apart (%s), within clusters' % (sep, tag))


@functools.lru_cache(maxsize=None)
def shift_case(q):
    """Points on a 2^-20 grid, so that adding 100 or 1e4 is exact in fp64: the shifted and the unshifted problem are the same
    problem, and gram_ld of either is the one reference."""
    n0, n1, b = 130, 67, 2
    rng = np.random.default_rng(900 + q)
    x0 = np.round(rng.standard_normal((n0, q)) * 2.0 ** 20) / 2.0 ** 20
    x1 = np.round(rng.standard_normal((n1, q)) * 2.0 ** 20) / 2.0 ** 20
    gam, al, _ = hyper(rng, b, q)
    ref, _ = gram_ld(x0, x1, gam, al)
    return x0, x1, gam, al, ref


@pytest.mark.parametrize('q', [1, 10, 30])
@pytest.mark.parametrize('shift', [100.0, 1e4])
def test_gram_far_from_origin_f64(dev, shift, q):
    """All points shifted by 100 / 1e4, compared with gram_ld (not the oracle, whose expanded form loses 2e-11 / 1e-7 of the
    largest entry there).  Tolerance: 8 x the error (relative to the largest entry) of the fp64 emulation of the kernel's
    arithmetic (gram_emulated) against gram_ld on the same inputs, computed here on the CPU; that error must itself be below
    the expanded form's.  The shifted result agrees with the unshifted one at the same tolerance.  Measured emulation /
    expanded-form errors for the committed inputs:
        shift 100: Q = 1  8.4e-15 / 2.6e-12,   Q = 10  1.1e-14 / 1.1e-11,   Q = 30  9.1e-15 / 1.4e-11
        shift 1e4: Q = 1  1.1e-12 / 4.0e-08,   Q = 10  1.0e-12 / 9.2e-08,   Q = 30  7.7e-13 / 1.4e-07"""
    x0, x1, gam, al, ref = shift_case(q)
    assert np.array_equal((x0 + shift) - shift, x0) and np.array_equal((x1 + shift) - shift, x1)
    big = float(ref.max())
    emu_err = float(np.abs(gram_emulated(x0 + shift, x1 + shift, gam, al, np.float64) - ref).max()) / big
    exp_err = float(np.abs(orc.ard_rbf_gram(x0 + shift, x1 + shift, gam, al, None) - ref).max()) / big
    tg, ta = T(gam, F64, dev), T(al, F64, dev)
    got = npf(ops.ard_rbf_gram(T(x0 + shift, F64, dev), T(x1 + shift, F64, dev), tg, ta, ta))
    got0 = npf(ops.ard_rbf_gram(T(x0, F64, dev), T(x1, F64, dev), tg, ta, ta))
    err, err0 = float(np.abs(got - ref).max()) / big, float(np.abs(got - got0).max()) / big
    print('gram shifted by %g Q=%d: emulation %.2e, expanded form %.2e; kernel %.2e vs reference, %.2e vs unshifted'
          % (shift, q, emu_err, exp_err, err, err0))
    assert emu_err < exp_err
    assert err <= 8.0 * emu_err
    assert err0 <= 8.0 * emu_err


@pytest.mark.parametrize('dt', DTYPES, ids=['f64', 'f32'])
def test_gram_nan_in_one_entry(dev, dt):
    """A NaN in one entry of x0: exactly that row of every kernel's output is NaN (and the column when x1=None); everything
    else equals the clean call bit for bit."""
    rng = np.random.default_rng(31)
    n0, n1, q, b, row = 70, 67, 5, 2, 65
    x0, x1 = r32(rng.standard_normal((n0, q))), r32(rng.standard_normal((n1, q)))
    gam, al, be = hyper(rng, b, q)
    bad = x0.copy()
    bad[row, 2] = np.nan
    tg, ta, tb = (T(a, dt, dev) for a in (gam, al, be))
    for xb in (T(x1, dt, dev), None):
        clean = ops.ard_rbf_gram(T(x0, dt, dev), xb, tg, ta, tb, True, True, jitter=JITTER)
        got = ops.ard_rbf_gram(T(bad, dt, dev), xb, tg, ta, tb, True, True, jitter=JITTER)
        want = torch.zeros_like(got, dtype=torch.bool)
        want[:, row, :] = True
        if xb is None:
            want[:, :, row] = True
        assert torch.equal(torch.isnan(got), want), 'NaN pattern'
        assert not bool(torch.isnan(clean).any())
        assert bits_equal(torch.where(want, torch.zeros_like(got), got), torch.where(want, torch.zeros_like(got), clean))


def test_q_above_the_maximum_is_refused(dev):
    """Q = 31 > DPGP_MAX_Q: a ValueError that names argument #4, for gram, psi1 and psi1T_y."""
    q, dt = 31, F64
    x = torch.zeros(5, q, dtype=dt, device=dev)
    s = torch.ones(5, q, dtype=dt, device=dev)
    g, a = torch.ones(2, q, dtype=dt, device=dev), torch.ones(2, 1, dtype=dt, device=dev)
    y = torch.zeros(5, 2, dtype=dt, device=dev)
    with pytest.raises(ValueError, match='#4'):
        ops.ard_rbf_gram(x, None, g, a, a)
    with pytest.raises(ValueError, match='#4'):
        ops.psi1(x, x, s, g, a)
    with pytest.raises(ValueError, match='#4'):
        ops.psi1T_y(x, x, s, g, a, y)


@pytest.mark.parametrize('dt', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('b', [1, 3, 300])
def test_diag_and_psi0_exact(dev, b, dt):
    """ard_rbf_diag and psi0 (B = 300: more than one 256-thread block of psi0) equal the oracle's expression evaluated in
    the tensor's type, exactly, for all flags, distinct alpha / beta and a non-default jitter."""
    ft = NP_OF[dt]
    rng = np.random.default_rng(50 + b)
    al = np.exp(0.3 * rng.standard_normal((b, 1))).astype(ft)
    be = (1.0 + np.exp(0.3 * rng.standard_normal((b, 1)))).astype(ft)
    ta, tb = T(al, dt, dev), T(be, dt, dev)
    for n in (1, 255, 257, 1000):
        for noise, jit in FLAGS:
            want = al * np.ones((1, n), dtype=ft)
            if noise:
                want = want + ft(1) / be
            if jit:
                want = want + ft(JITTER)
            assert want.dtype == ft
            got = ops.ard_rbf_diag(n, ta, tb, noise, jit, jitter=JITTER).cpu().numpy()
            assert got.dtype == ft and np.array_equal(got, want), ('diag', b, n, noise, jit)
        got0 = ops.psi0(n, ta).cpu().numpy()
        assert np.array_equal(got0, al * ft(n)), ('psi0', b, n)
    print('diag / psi0 B=%d %s: exact' % (b, ft.__name__))


# ---------------------------------------------------------------------------------------------------------------
# psi1
# ---------------------------------------------------------------------------------------------------------------

def psi_inputs(rng, b, n, m, q):
    """As test_psi_statistics_vs_oracle_ragged (within the f16 range of the fp32 Psi1^T y kernel), rounded to fp32."""
    z, mu = r32(rng.standard_normal((m, q))), r32(rng.standard_normal((n, q)))
    s = r32(np.exp(0.5 * rng.standard_normal((n, q))))
    gam = r32(np.exp(0.3 * rng.standard_normal((b, q))))
    al = r32(np.exp(0.3 * rng.standard_normal((b, 1))) * (1.0 + 0.25 * np.arange(b))[:, None])
    y = r32(rng.standard_normal((n, b)))
    return z, mu, s, gam, al, y


_P1_NS, _P1_MS, _P1_QS, _P1_BS = [1, 31, 32, 33, 65], [1, 3, 4, 63, 64, 65, 68, 129, 130], [1, 7, 30], [1, 3]
PSI1_SHAPES = [(_P1_BS[(i + k) % 2], _P1_NS[(i + k) % 5], m, _P1_QS[(i + 2 * k) % 3])
               for i, m in enumerate(_P1_MS) for k in range(3)] + [(3, 1, 1, 1), (1, 32, 64, 30), (3, 65, 130, 30)]


@functools.lru_cache(maxsize=None)
def psi1_case(shape):
    b, n, m, q = shape
    arrs = psi_inputs(np.random.default_rng(sum(shape) + 1000 * q), b, n, m, q)
    return arrs, psi1_ld(*arrs[:5])[0]


@pytest.mark.parametrize('dt', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('shape', PSI1_SHAPES, ids=lambda s: 'B%d-N%d-M%d-Q%d' % s)
def test_psi1_edges(dev, shape, dt):
    """N around the 32-row workgroup, M around the 64-row z chunk and the 4-wide vector store (M % 4 == 0 with and without a
    ragged chunk), Q = 1, 7, 30, distinct alpha per kernel."""
    arrs, ref = psi1_case(shape)
    check(ops.psi1(*(T(a, dt, dev) for a in arrs[:5])), ref, TOL[dt], 'psi1 B=%d N=%d M=%d Q=%d' % shape)


def test_psi1_far_inducing_points_f64(dev):
    """Half the inducing points sit 3000 length scales away: the argument of dpgp_exp2 is below its -1022 clamp, those entries
    are exactly 0, everything is finite and the near half stays within the file's tolerance."""
    b, n, m, q = 2, 65, 68, 3
    z, mu, s, gam, al, _ = psi_inputs(np.random.default_rng(77), b, n, m, q)
    gam = np.ones_like(gam)
    far = np.arange(m) % 2 == 1
    z[far, 1] += 3000.0
    ref, ex = psi1_ld(z, mu, s, gam, al)
    got = npf(ops.psi1(*(T(a, F64, dev) for a in (z, mu, s, gam, al))))
    print('psi1 far: far exponents (base 2) %.3g .. %.3g' % (ex[:, :, far].min() * LOG2E, ex[:, :, far].max() * LOG2E))
    assert ex[:, :, far].max() * LOG2E < -1022.0
    assert np.isfinite(got).all()
    assert (got[:, :, far] == 0.0).all()
    check(got[:, :, ~far], ref[:, :, ~far], TOL[F64], 'psi1 far, the near half')


@pytest.mark.parametrize('dt', DTYPES, ids=['f64', 'f32'])
def test_psi1_nan_and_variance_extremes_stay_in_their_rows(dev, dt):
    """A NaN in one mu entry makes that output row NaN for every kernel and inducing point; variances of 1e-12 and 1e6 in
    single rows stay within tolerance; in both cases all other rows equal the clean call bit for bit (the factors and the
    log-term are per row)."""
    b, n, m, q = 3, 65, 68, 3
    z, mu, s, gam, al, _ = psi_inputs(np.random.default_rng(78), b, n, m, q)
    tz, tg, ta = (T(a, dt, dev) for a in (z, gam, al))
    clean = ops.psi1(tz, T(mu, dt, dev), T(s, dt, dev), tg, ta)
    assert not bool(torch.isnan(clean).any())
    row = 33
    bad = mu.copy()
    bad[row, 1] = np.nan
    got = ops.psi1(tz, T(bad, dt, dev), T(s, dt, dev), tg, ta)
    want = torch.zeros_like(got, dtype=torch.bool)
    want[:, row, :] = True
    assert torch.equal(torch.isnan(got), want), 'NaN pattern'
    keep = [i for i in range(n) if i != row]
    assert bits_equal(got[:, keep], clean[:, keep])
    s2 = s.copy()
    s2[31], s2[32] = 1e-12, 1e6
    s2 = s2.astype(NP_OF[dt]).astype(np.float64)
    got = ops.psi1(tz, T(mu, dt, dev), T(s2, dt, dev), tg, ta)
    keep = [i for i in range(n) if i not in (31, 32)]
    assert bits_equal(got[:, keep], clean[:, keep]), 'neighbouring rows disturbed'
    ref, _ = psi1_ld(z, mu, s2, gam, al)
    check(got, ref, TOL[dt], 'psi1 with s = 1e-12 / 1e6 rows')
    for r in (31, 32):   # the rows themselves, on their own scale
        check(got[:, r], ref[:, r], TOL[dt], 'psi1 row with s = %g' % s2[r, 0])


# ---------------------------------------------------------------------------------------------------------------
# psi1T_y
# ---------------------------------------------------------------------------------------------------------------
TOL_P1Y = {F64: TOL[F64], F32: dict(TOL[F32], atol_rel=2e-5)}      # fp32: a signed sum over n of fp32 terms (test_gpu_kernels)

_PY_MS, _PY_NS = [1, 64, 65, 127, 128, 129, 257], [1, 31, 33, 129, 257, 300]
P1Y_SHAPES_F64 = [([1, 3][(i + k) % 2], _PY_NS[(2 * i + 3 * k) % 6], m, [1, 30][(i + k + 1) % 2])
                  for i, m in enumerate(_PY_MS) for k in range(2)] + [(3, 300, 257, 30), (1, 129, 128, 1)]
P1Y_QS_F32 = [5, 6, 10, 11, 15, 16, 21, 22, 26, 27, 30]                 # both edges of every KF1 = ceil((6 Q + 2) / 32) = 1..6
P1Y_MS_F32 = [40, 64, 65, 130]                                          # NJ = 4 (M <= 64) / NJ = 8 and their boundary


@functools.lru_cache(maxsize=None)
def p1y_case(shape):
    b, n, m, q = shape
    arrs = psi_inputs(np.random.default_rng(sum(shape) + 77 * q), b, n, m, q)
    return arrs, psi1T_y_ld(*arrs)


@pytest.mark.parametrize('shape', P1Y_SHAPES_F64, ids=lambda s: 'B%d-N%d-M%d-Q%d' % s)
def test_psi1T_y_edges_f64(dev, shape):
    """M around the 128-column chunk (two columns per lane), N around the 32-row tile and the split boundaries."""
    arrs, ref = p1y_case(shape)
    check(ops.psi1T_y(*(T(a, F64, dev) for a in arrs)), ref, TOL_P1Y[F64], 'psi1T_y f64 B=%d N=%d M=%d Q=%d' % shape)


@pytest.mark.parametrize('m', [65, 257])
def test_psi1T_y_split_count_f64(dev, m, monkeypatch):
    """N = 300: one split (DPGP_PSI1_NS=1) against the library's own count (3 here): both within tolerance of the reference
    and equal to 1e-13 of the largest entry."""
    shape = (3, 300, m, 30)
    arrs, ref = p1y_case(shape)
    targs = [T(a, F64, dev) for a in arrs]
    monkeypatch.delenv('DPGP_PSI1_NS', raising=False)
    own = ops.psi1T_y(*targs)
    monkeypatch.setenv('DPGP_PSI1_NS', '1')
    one = ops.psi1T_y(*targs)
    check(own, ref, TOL_P1Y[F64], 'psi1T_y f64 M=%d, library split count' % m)
    check(one, ref, TOL_P1Y[F64], 'psi1T_y f64 M=%d, one split' % m)
    dif = float((own - one).abs().max()) / float(np.abs(ref).max())
    print('psi1T_y f64 M=%d: one split vs library split count %.2e of the largest entry' % (m, dif))
    assert dif <= 1e-13


@pytest.mark.parametrize('m', P1Y_MS_F32)
@pytest.mark.parametrize('q', P1Y_QS_F32)
def test_psi1T_y_every_k_step_count_f32(dev, q, m):
    """The f16-operand kernel at both edges of each of its six K-step instantiations and both column-tile variants."""
    shape = (3, 200, m, q)
    arrs, ref = p1y_case(shape)
    check(ops.psi1T_y(*(T(a, F32, dev) for a in arrs)), ref, TOL_P1Y[F32], 'psi1T_y f32 B=%d N=%d M=%d Q=%d' % shape)


@pytest.mark.parametrize('dt', DTYPES, ids=['f64', 'f32'])
def test_psi1T_y_leading_dimension_above_b(dev, dt):
    """The C ABI with y inside a [N, B + 3] buffer whose padding columns are NaN (ldy = B + 3): bit-identical to the operator
    on the contiguous copy."""
    from dp_gp_lvm_amd import _lib
    b, n, m, q = 3, 200, 65, 7
    arrs, _ = p1y_case((b, n, m, q))
    z, mu, s, gam, al, y = (T(a, dt, dev) for a in arrs)
    want = ops.psi1T_y(z, mu, s, gam, al, y)
    assert not bool(torch.isnan(want).any())
    pad = torch.full((n, b + 3), float('nan'), dtype=dt, device=dev)
    pad[:, :b] = y
    l = _lib.lib()
    wsb = l.dpgp_psi1T_y_workspace_bytes(b, n, m)
    ws = torch.empty(max(int(wsb), 256), dtype=torch.uint8, device=dev)
    out = torch.empty((b, m), dtype=dt, device=dev)
    name = 'dpgp_psi1T_y_' + ('f64' if dt == F64 else 'f32')
    al1 = al.reshape(-1).contiguous()
    _lib.check(getattr(l, name)(b, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gam.data_ptr(), al1.data_ptr(),
                                pad.data_ptr(), b + 3, out.data_ptr(), ws.data_ptr(), wsb,
                                torch.cuda.current_stream().cuda_stream), name)
    assert bits_equal(out, want)


def test_psi1T_y_far_observations_f64(dev):
    """Observations 3000 length scales from every inducing point contribute exactly nothing (the result equals, bit for bit,
    the one with their y set to 0); the result is finite and within tolerance."""
    b, n, m, q = 3, 300, 129, 3
    z, mu, s, gam, al, y = psi_inputs(np.random.default_rng(91), b, n, m, q)
    gam = np.ones_like(gam)
    far = np.arange(n) % 3 == 1
    mu[far, 2] -= 3000.0
    y0 = y.copy()
    y0[far] = 0.0
    targs = [T(a, F64, dev) for a in (z, mu, s, gam, al)]
    got, got0 = ops.psi1T_y(*targs, T(y, F64, dev)), ops.psi1T_y(*targs, T(y0, F64, dev))
    assert bool(torch.isfinite(got).all())
    assert bits_equal(got, got0), 'far observations contributed'
    check(got, psi1T_y_ld(z, mu, s, gam, al, y), TOL_P1Y[F64], 'psi1T_y f64 with far observations')


@pytest.mark.parametrize('dt', DTYPES, ids=['f64', 'f32'])
def test_psi1T_y_nan_in_one_y_entry(dev, dt):
    """A NaN in y[n, b]: exactly kernel b's row of the result is NaN, the other rows equal the clean call bit for bit."""
    b, n, m, q = 3, 200, 130, 7
    arrs, _ = p1y_case((b, n, m, q))
    targs = [T(a, dt, dev) for a in arrs[:5]]
    clean = ops.psi1T_y(*targs, T(arrs[5], dt, dev))
    bad = arrs[5].copy()
    bad[150, 1] = np.nan
    got = ops.psi1T_y(*targs, T(bad, dt, dev))
    want = torch.zeros_like(got, dtype=torch.bool)
    want[1] = True
    assert not bool(torch.isnan(clean).any())
    assert torch.equal(torch.isnan(got), want), 'NaN pattern'
    assert bits_equal(got[[0, 2]], clean[[0, 2]])


# ---------------------------------------------------------------------------------------------------------------
# KL
# ---------------------------------------------------------------------------------------------------------------
KL_SHAPES = [(1, 1), (255, 1), (257, 3), (10001, 30)]


def kl_inputs(n, q, ft):
    """mu standard normal, s log-normal with sigma = 2, as stored in type ft."""
    rng = np.random.default_rng(13 * n + q)
    mu, s = rng.standard_normal((n, q)), np.exp(2.0 * rng.standard_normal((n, q)))
    return mu.astype(ft).astype(np.float64), s.astype(ft).astype(np.float64)


@pytest.mark.parametrize('dt', DTYPES, ids=['f64', 'f32'])
@pytest.mark.parametrize('shape', KL_SHAPES, ids=lambda s: '%dx%d' % s)
def test_kl_sizes(dev, shape, dt):
    """One element, around the 256-thread block, and 300 030 elements through the single-block loop; every term is >= 0, so
    the sum is well conditioned (tests/test_elementwise_refs.py checks the tolerance on the oracle's own fp64 sum)."""
    mu, s = kl_inputs(shape[0], shape[1], NP_OF[dt])
    ref = kl_ld(mu, s)
    got = float(ops.kl_qx(T(mu, dt, dev), T(s, dt, dev)))
    print('kl %dx%d %s: rel.err %.2e' % (shape[0], shape[1], NP_OF[dt].__name__, abs(got - ref) / abs(ref)))
    np.testing.assert_allclose(got, ref, rtol=1e-12 if dt == F64 else 1e-6)
