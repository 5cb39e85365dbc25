"""
GPU tests of the forward Psi2 kernels (csrc/psi2.hip: psi2_mfma_kernel in fp64 and exact fp32, psi2_f16_kernel = the
per-observation patch kernel, psi2_plain_kernel; csrc/psi2_pairs.hip: the pair-tile kernel; csrc/psi2_consts.h) at every
K-step instantiation, n-split, chunk, tile-range and tile edge of their dispatch, at their range guards and over the whole
exponent range.

The reference is psi2_ld: the literal formula of oracle.psi2 with differences, products, logs and sums in np.longdouble
(tests/test_psi2_refs.py pins it against the oracle and the golden fixtures on the CPU).  Every random input is rounded to
fp32 first, so that the fp64 and the fp32 operators see the same numbers and share one reference.  Every sweep calls the
operator through the C ABI with a workspace of exactly dpgp_psi2_workspace_bytes bytes that is pre-filled with NaN
(psi2_call): a slab entry that is read before it is written shows as NaN, not as whatever the allocator left there.

"All algorithms" is ALGOS below.  Tolerances at ordinary geometry are test_gpu_kernels.TOL_PSI2.  Far from the centre the
f16-split kernels are held to their documented accuracy model (pairs_emulated, patch_emulated: CPU emulations of their
operand arithmetic, pinned by the CPU sibling of this file).  Each case prints its observed maximum error.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from conftest import golden  # noqa: F401  (the golden inputs are used by the CPU sibling of this file)
from dp_gp_lvm_amd import _lib, ops
from test_gpu_kernels import TOL_PSI2

pytestmark = pytest.mark.gpu

LD = np.longdouble
F64, F32 = torch.float64, torch.float32
f32, f16 = np.float32, np.float16
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
ALGOS = [(F64, 'auto'), (F64, 'plain'), (F32, 'auto'), (F32, 'mfma_f32'), (F32, 'patch_f16'), (F32, 'plain')]
SUFFIX = {F64: 'f64', F32: 'f32'}
PAIR_GUARD, PATCH_GUARD = 8192.0, 30000.0        # psi2_pairs.hip: oor |= !(cc >= -8192); psi2.hip: the +-30000 clamps
PAIR_MODEL = LN2 * 2.0 ** -21                     # relative error per unit of max|c''|: "exponent good to ~|c''| 2^-21"


def tag(dt, algo):
    return '%s %-9s' % (SUFFIX[dt], algo)


# ---------------------------------------------------------------------------------------------------------------
# reference (NumPy, longdouble)
# ---------------------------------------------------------------------------------------------------------------

def r32(a):
    """Rounded to fp32 and back: the fp64 and fp32 operators then see identical inputs."""
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _psi2_ld(key):
    z, mu, s, gamma, alpha = (np.frombuffer(buf, dtype=np.float64).reshape(shape).astype(LD) for shape, buf in key)
    alpha = alpha.reshape(-1)
    b_, n_, m_ = gamma.shape[0], mu.shape[0], z.shape[0]
    i, j = np.tril_indices(m_)
    zbar = (z[i] + z[j]) / LD(2)                                                   # [P,Q]
    zdif2 = np.square(z[i] - z[j])
    c = np.sum(z, axis=0) / LD(m_)
    acc = np.zeros((b_, len(i)), dtype=LD)                                         # lower-triangle pairs, summed over n
    cmax = np.zeros(b_)
    log2e = LD(1) / np.log(LD(2))
    chunk = max(1, min(n_, 4000000 // (len(i) * z.shape[1])))
    for n0 in range(0, n_, chunk):
        num = np.square(mu[n0:n0 + chunk, None, :] - zbar[None])                   # [c,P,Q]
        for b in range(b_):
            g = gamma[b][None, :]
            den = LD(2) * g * s[n0:n0 + chunk] + LD(1)                             # [c,Q]
            w = g / den
            e = np.einsum('cpq,cq->cp', num, w)
            lp = LD(2) * np.log(alpha[b]) - (LD(0.5) * np.sum(np.log(den), axis=-1)[:, None]
                                             + LD(0.25) * np.sum(zdif2 * g, axis=-1)[None, :] + e)
            acc[b] += np.sum(np.exp(lp), axis=0)
            cpp = -np.sum(w * np.square(mu[n0:n0 + chunk] - c[None, :]) * log2e + LD(0.5) * np.log(den) * log2e, axis=-1)
            cmax[b] = max(cmax[b], float(np.max(np.abs(cpp))))
    out = np.zeros((b_, m_, m_))
    out[:, i, j] = acc.astype(np.float64)
    out[:, j, i] = out[:, i, j]
    out.setflags(write=False)
    cmax.setflags(write=False)
    return out, cmax


def psi2_ld(z, mu, s, gamma, alpha):
    """The literal formula of oracle.psi2 (log psi2[b,n,m,m'] = 2 log alpha_b - sum_q (1/2 log den + gamma (z_m - z_m')^2 / 4
    + gamma (mu_n - (z_m + z_m') / 2)^2 / den), den = 2 gamma s + 1, summed over n) with differences, products, logs and sums
    in longdouble -> (psi2 [B,M,M] fp64, max_n |c''_n| per b), c''_n = -sum_q (w (mu - c)^2 log2e + 1/2 log2 den), w = gamma /
    den, c the column mean of z (the row constant of the pair-tile kernel: header of psi2_pairs.hip).  Memoised on the inputs'
    bytes; the results are read-only."""
    arrs = [np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (z, mu, s, np.atleast_2d(gamma), alpha)]
    return _psi2_ld(tuple((a.shape, a.tobytes()) for a in arrs))


# ---------------------------------------------------------------------------------------------------------------
# CPU emulations of the f16-split kernels' operand arithmetic (one output dim)
# ---------------------------------------------------------------------------------------------------------------

def _split2(x):
    h = x.astype(f16)
    return h, (x - h.astype(f32)).astype(f16)


def _exact_exponent(z, mu, s, g):
    """log2 of psi2[n, p] / (alpha^2 exp2(beta_p)) for the lower-triangle pairs p, in longdouble from the given inputs."""
    i, j = np.tril_indices(z.shape[0])
    zl, mul, sl, gl = (np.asarray(a, dtype=np.float64).astype(LD) for a in (z, mu, s, g))
    den = LD(2) * gl * sl + LD(1)
    zbar = (zl[i] + zl[j]) / LD(2)
    log2e = LD(1) / np.log(LD(2))
    ex = -(np.sum(LD(0.5) * np.log(den) * log2e, axis=1)[:, None]
           + log2e * np.einsum('npq,nq->np', np.square(mul[:, None, :] - zbar[None]), gl / den))
    return ex.astype(np.float64), i, j


def pairs_emulated(z, mu, s, g):
    """The pair-tile kernel's exponent E[n, p] = c''_n + sum_q (a_nq s_pq^2 + b_nq s_pq) as psi2_pairs.hip and psi2_consts.h
    build it: fp32 for the column means, a, b and c''; the row operands {ah, ah, al | bh, bh, bl} against the pair features
    {f1h, f1l, f1h | f2h, f2l, f2h} with f1 = s^2 / 64 (and 64 a on the other side), f2 = s; c'' in three f16 pieces where
    6Q + 2 slots leave one free, in two (22 bits) where they do not (Q = 5 and Q = 21); exact products, a wide sum, one
    rounding to fp32 (the fp32 accumulation order inside the MFMA is not modelled).
    -> dict(err: max |E - exact| over the terms with exact E > -40, cmax: max_n |c''_n|, ratio: err / (cmax 2^-21), three)."""
    z, mu, s, g = (np.asarray(a, dtype=np.float64).astype(f32) for a in (z, mu, s, g))
    n_, q_ = mu.shape
    zc = z.astype(np.float64).mean(0).astype(f32)
    mc = (mu - zc).astype(f32)
    den = (f32(2) * g * s + f32(1)).astype(f32)
    w = (g / den).astype(f32)
    a = (f32(-0.25 * LOG2E * 64) * w).astype(f32)
    bb = ((f32(LOG2E) * w).astype(f32) * mc).astype(f32)
    cc = np.zeros(n_, f32)
    for q in range(q_):
        cc = (cc - ((bb[:, q] * mc[:, q]).astype(f32) + (f32(0.5) * np.log2(den[:, q]).astype(f32)).astype(f32)).astype(f32)).astype(f32)
    ks = (6 * q_ + 2 + 15) // 16
    ks = 2 if ks <= 2 else 4 if ks <= 4 else 6 if ks <= 6 else 8
    three = 6 * q_ + 2 < 16 * ks
    ch = cc.astype(f16)
    r1 = (cc - ch.astype(f32)).astype(f32)
    cm = r1.astype(f16)
    cl = (r1 - cm.astype(f32)).astype(f16)
    d = np.float64
    cparts = ch.astype(d) + cm.astype(d) + (cl.astype(d) if three else 0.0)
    ex, i, j = _exact_exponent(z, mu, s, g)
    zcent = (z - zc).astype(f32)
    sq = (zcent[i] + zcent[j]).astype(f32)                                         # [P,Q]
    f1 = ((sq * sq).astype(f32) * f32(1 / 64)).astype(f32)
    ah, al = _split2(a)
    bh, bl = _split2(bb)
    f1h, f1l = _split2(f1)
    f2h, f2l = _split2(sq)
    dot = lambda x, y: np.einsum('nq,pq->np', x.astype(d), y.astype(d))
    e = (dot(ah, f1h) + dot(ah, f1l) + dot(al, f1h) + dot(bh, f2h) + dot(bh, f2l) + dot(bl, f2h)
         + cparts[:, None]).astype(f32).astype(d)
    sel = ex > -40
    err = float(np.abs(e - ex)[sel].max())
    cmax = float(np.abs(cc).max())
    return dict(err=err, cmax=cmax, ratio=err / (cmax * 2.0 ** -21), three=three, ks=ks)


def patch_emulated(z, mu, s, g):
    """The patch kernel's exponent (psi2.hip, psi2_patch_f16p): P[n, m] = c'_n + sum_q (a_nq z_mq^2 + b_nq z_mq) on the matrix
    pipe — row operands {ah, ah, al | bh, bh, bl} against {hi, lo, hi} of z^2 and z, c' in two f16 pieces — rounded to fp32 and
    split into (hi, lo) f16 words; then E[n, m, m'] = P[n, m] + P[n, m'] + sum_q X_nq z_mq z_m'q with the fp32 products X z
    split two ways against the two-way split of z.  Exact products, wide sums, one rounding to fp32 per GEMM.
    -> dict(err: max |E - exact| over the lower-triangle terms with exact E > -40, pmax: max |P|, cprime: max_n |c'_n|)."""
    z, mu, s, g = (np.asarray(a, dtype=np.float64).astype(f32) for a in (z, mu, s, g))
    d = np.float64
    zc = z.astype(d).mean(0).astype(f32)
    zs = (z - zc).astype(f32)
    mc = (mu - zc).astype(f32)
    den = (f32(2) * g * s + f32(1)).astype(f32)
    w = (g / den).astype(f32)
    vx = (f32(-0.5 * LOG2E) * w).astype(f32)
    a = (f32(-0.25 * LOG2E) * w).astype(f32)
    bb = ((f32(LOG2E) * w).astype(f32) * mc).astype(f32)
    cq = ((((f32(-0.5 * LOG2E) * w).astype(f32) * mc).astype(f32) * mc).astype(f32)
          - (f32(0.25) * np.log2(den).astype(f32)).astype(f32)).astype(f32)
    cp = np.zeros(mu.shape[0], f32)
    for q in range(mu.shape[1]):
        cp = (cp + cq[:, q]).astype(f32)
    ch, cl = _split2(cp)
    ah, al = _split2(a)
    bh, bl = _split2(bb)
    z2h, z2l = _split2((zs * zs).astype(f32))
    z1h, z1l = _split2(zs)
    dot = lambda x, y: np.einsum('nq,mq->nm', x.astype(d), y.astype(d))
    p = (dot(ah, z2h) + dot(ah, z2l) + dot(al, z2h) + dot(bh, z1h) + dot(bh, z1l) + dot(bl, z1h)
         + (ch.astype(d) + cl.astype(d))[:, None]).astype(f32)                     # [N,M]
    ph, pl = _split2(p)
    psum = ph.astype(d) + pl.astype(d)
    ex, i, j = _exact_exponent(z, mu, s, g)
    xz = (vx[:, None, :] * zs[None, :, :]).astype(f32)                             # [N,M,Q]  A side: X z_m, split
    xh, xl = _split2(xz)
    xh, xl = xh.astype(d), xl.astype(d)
    zh, zl = z1h.astype(d), z1l.astype(d)
    e = (np.einsum('npq,pq->np', xh[:, i, :], zh[j]) + np.einsum('npq,pq->np', xh[:, i, :], zl[j])
         + np.einsum('npq,pq->np', xl[:, i, :], zh[j]) + psum[:, i] + psum[:, j]).astype(f32).astype(d)
    sel = ex > -40
    return dict(err=float(np.abs(e - ex)[sel].max()), pmax=float(np.abs(p).max()), cprime=float(np.abs(cp).max()))


# ---------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------

def T(a, dt, dev):
    return torch.as_tensor(np.asarray(a), dtype=dt, device=dev)


def npf(t):
    return t.detach().cpu().numpy().astype(np.float64)


def bits_equal(a, b):
    """Bit-for-bit equality that also holds for NaN payloads and signed zeros."""
    it = torch.int64 if a.dtype == F64 else torch.int32
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def psi2_raw(dev, dt, b, n, m, q, tensors, algo_id, short=0):
    """dpgp_psi2_f32 / _f64 through the C ABI on a workspace of exactly dpgp_psi2_workspace_bytes - short bytes, pre-filled
    with NaN -> (return code, out)."""
    l = _lib.lib()
    wsb = int(l.dpgp_psi2_workspace_bytes(b, n, m, q, 8 if dt == F64 else 4))
    assert wsb > 0 and wsb % 4 == 0
    ws = torch.full((wsb // 4,), float('nan'), dtype=F32, device=dev)          # (two NaN words are an fp64 NaN as well)
    out = torch.full((b, m, m), float('nan'), dtype=dt, device=dev)
    z, mu, s, gam, al = tensors
    rc = getattr(l, 'dpgp_psi2_' + SUFFIX[dt])(b, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gam.data_ptr(),
                                               al.data_ptr(), out.data_ptr(), ws.data_ptr(), ctypes.c_size_t(wsb - short),
                                               algo_id, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def psi2_call(dev, dt, algo, z, mu, s, gamma, alpha):
    """The operator on NumPy inputs through psi2_raw; a non-zero return code is an error."""
    z, mu, s = (np.asarray(a, dtype=np.float64) for a in (z, mu, s))
    gamma = np.atleast_2d(np.asarray(gamma, dtype=np.float64))
    alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
    ts = [T(np.ascontiguousarray(a), dt, dev) for a in (z, mu, s, gamma, alpha)]
    rc, out = psi2_raw(dev, dt, gamma.shape[0], mu.shape[0], z.shape[0], z.shape[1], ts, _lib.ALGO[algo])
    assert rc == 0, ('dpgp_psi2_' + SUFFIX[dt], algo, rc)
    return out


def check(got, ref, rtol, atol_rel, what):
    """|got - ref| <= rtol_b |ref| + atol_rel max|ref_b| per output dim b (rtol a number or one per b), printing the observed
    errors first.  NaN in got fails."""
    got = npf(got) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    rt = np.broadcast_to(np.asarray(rtol, dtype=np.float64).reshape(-1), (ref.shape[0],))
    worst, worst_rel = 0.0, 0.0
    for b in range(ref.shape[0]):
        big = float(np.max(np.abs(ref[b])))
        err = np.abs(got[b] - ref[b])
        with np.errstate(divide='ignore', invalid='ignore'):
            rel = np.where(np.abs(ref[b]) > atol_rel * big / max(rt[b], 1e-300), err / np.abs(ref[b]), 0.0)
        worst = max(worst, float(np.nanmax(err)) / max(big, 1e-300))
        worst_rel = max(worst_rel, float(np.nanmax(rel)))
    print('%-64s max|err|/max|ref| %.2e   max rel.err (entries above the atol floor) %.2e   (rtol %.2e)'
          % (what, worst, worst_rel, float(rt.max())))
    for b in range(ref.shape[0]):
        np.testing.assert_allclose(got[b], ref[b], rtol=rt[b], atol=atol_rel * float(np.max(np.abs(ref[b]))),
                                   err_msg='%s, output dim %d' % (what, b))
    return worst_rel


def check_tol(got, ref, dt, what):
    return check(got, ref, TOL_PSI2[dt]['rtol'], TOL_PSI2[dt]['atol_rel'], what)


@functools.lru_cache(maxsize=None)
def ordinary_case(b, n, m, q):
    """Ordinary geometry: z, mu ~ N(0, 1), s = exp(0.5 N), gamma and alpha = exp(0.3 N), alpha distinct per b."""
    rng = np.random.default_rng(1000003 * b + 10007 * n + 101 * m + q)
    z, mu = r32(rng.standard_normal((m, q))), r32(rng.standard_normal((n, q)))
    s = r32(np.exp(0.5 * rng.standard_normal((n, q))))
    gam = r32(np.exp(0.3 * rng.standard_normal((b, q))))
    al = r32(np.exp(0.3 * rng.standard_normal((b, 1))) * (1.0 + 0.25 * np.arange(b))[:, None])
    return z, mu, s, gam, al


def ordinary_ref(b, n, m, q):
    return psi2_ld(*ordinary_case(b, n, m, q))[0]


def all_algorithms(dev, case, ref, what, also=None):
    for dt, algo in ALGOS:
        got = psi2_call(dev, dt, algo, *case)
        check_tol(got, ref, dt, '%s %s' % (what, tag(dt, algo)))
        if also is not None:
            also(dt, algo, got)


# ---------------------------------------------------------------------------------------------------------------
# the caller itself
# ---------------------------------------------------------------------------------------------------------------

def test_caller_agrees_with_ops(dev):
    """psi2_call (C ABI, exact NaN-filled workspace) and ops.psi2 run the same operator: bitwise equal results."""
    case = ordinary_case(2, 70, 40, 6)
    for dt, algo in ALGOS:
        got = psi2_call(dev, dt, algo, *case)
        via_ops = ops.psi2(*[T(a, dt, dev) for a in case], algo=algo)
        assert bits_equal(got, via_ops), tag(dt, algo)


# ---------------------------------------------------------------------------------------------------------------
# 1. every Q
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('q', list(range(1, 31)))
def test_every_latent_dimension(dev, q):
    """Q = 1 .. 30 at B = 2, N = 70, M = 40: all eight K-step instantiations of the fp64 and the exact-fp32 MFMA kernel (KS =
    ceil((Q + 2) / 4)), all eight of the patch kernel (KB = ceil(Q / 4)), the four of the pair-tile kernel (KS 2, 4, 6, 8 with
    Q = 5 and Q = 21, where c'' has two f16 pieces only) and the pair -> patch handover at Q = 22.  Exactly symmetric;
    two calls bitwise equal."""
    case = ordinary_case(2, 70, 40, q)
    ref = ordinary_ref(2, 70, 40, q)

    def also(dt, algo, got):
        assert torch.equal(got, got.transpose(1, 2)), 'psi2 must be exactly symmetric: ' + tag(dt, algo)
        assert bits_equal(got, psi2_call(dev, dt, algo, *case)), 'two calls differ: ' + tag(dt, algo)
    all_algorithms(dev, case, ref, 'Q=%d' % q, also)


def test_refusals(dev):
    """Q = 31 is refused (by ops.psi2 and with -4 by the C ABI); a workspace one byte short gives -12, an algorithm id out of
    range -13; the output is not touched."""
    z, mu, s, gam, al = ordinary_case(2, 70, 40, 6)
    for dt in (F64, F32):
        ts = [T(a, dt, dev) for a in (z, mu, s, gam, al.reshape(-1))]
        for kw, want in ((dict(algo_id=0, short=1), -12), (dict(algo_id=4), -13), (dict(algo_id=-1), -13)):
            rc, out = psi2_raw(dev, dt, 2, 70, 40, 6, ts, **kw)
            assert rc == want and bool(torch.isnan(out).all()), (SUFFIX[dt], kw, rc)
        rng = np.random.default_rng(31)
        z31, mu31 = rng.standard_normal((40, 31)), rng.standard_normal((70, 31))
        t31 = [T(a, dt, dev) for a in (z31, mu31, np.ones((70, 31)), np.ones((2, 31)), np.ones(2))]
        with pytest.raises(Exception):
            ops.psi2(*t31)
        l = _lib.lib()
        ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
        out = torch.full((2, 40, 40), float('nan'), dtype=dt, device=dev)
        rc = getattr(l, 'dpgp_psi2_' + SUFFIX[dt])(2, 70, 40, 31, *[t.data_ptr() for t in t31], out.data_ptr(), ws.data_ptr(),
                                                   ctypes.c_size_t(ws.numel()), 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == -4 and bool(torch.isnan(out).all())


# ---------------------------------------------------------------------------------------------------------------
# 2. M and N edges
# ---------------------------------------------------------------------------------------------------------------
M_EDGES = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65]
N_EDGES = [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 129]


@pytest.mark.parametrize('m', M_EDGES)
def test_inducing_point_edges(dev, m):
    """M on, one below and one past 16 (Mp rounding), 32 (the fp64 patch), 48 and 64 (the fp32 patch): diagonal and
    off-diagonal patches, ragged last pair tile.  N = 37, B = 2, Q in {2, 7}, all algorithms."""
    for q in (2, 7):
        all_algorithms(dev, ordinary_case(2, 37, m, q), ordinary_ref(2, 37, m, q), 'M=%d Q=%d' % (m, q))


@pytest.mark.parametrize('n', N_EDGES)
def test_observation_edges(dev, n):
    """N of 1, around 4 (the four-wave row ownership n = nbeg + w + 4 j), around the 8-row wave chunks and the 32-row tiles
    (31 .. 33, 63 .. 65, 127, 129).  M = 17, B = 2, Q in {2, 7}, all algorithms."""
    for q in (2, 7):
        all_algorithms(dev, ordinary_case(2, n, 17, q), ordinary_ref(2, n, 17, q), 'N=%d Q=%d' % (n, q))


def test_many_output_dims(dev):
    """B = 130, N = 260, M = 17, Q = 3: the B >= 128 branch of psi2_nsplit."""
    all_algorithms(dev, ordinary_case(130, 260, 17, 3), ordinary_ref(130, 260, 17, 3), 'B=130')


# ---------------------------------------------------------------------------------------------------------------
# 3. pair-tile grouping
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('m', [40, 56, 64])
@pytest.mark.parametrize('q', [3, 10, 13, 20])
def test_pair_tile_grouping(dev, q, m, monkeypatch):
    """The pair-tile kernel's tile loops (groups of G = 6, 6, 4, 2 resident tiles at KS = 2, 4, 6, 8, then groups of 2 and 1)
    depend on the tiles per range modulo 4 G.  B = 1, N = 40; M = 40, 56, 64 are 26, 50 and 65 tiles.  Default ranges (M = 64:
    3 ranges of 22 tiles: two waves run one full group, the others 2 + 2 + 1), one range (M = 64: 16 - 17 tiles per wave: two
    full groups with the next group's operands fetched beneath the epilogue, then remainders) and five ranges.  The ranges
    partition the pairs and never change a sum's order: bitwise equal results."""
    case = ordinary_case(1, 40, m, q)
    ref = ordinary_ref(1, 40, m, q)
    monkeypatch.delenv('DPGP_PP_RANGES', raising=False)
    base = psi2_call(dev, F32, 'auto', *case)
    check_tol(base, ref, F32, 'pairs Q=%d M=%d default ranges' % (q, m))
    for nr in (1, 5):
        monkeypatch.setenv('DPGP_PP_RANGES', str(nr))
        got = psi2_call(dev, F32, 'auto', *case)
        check_tol(got, ref, F32, 'pairs Q=%d M=%d %d range(s)' % (q, m, nr))
        assert bits_equal(got, base), 'tile ranges changed the result: Q=%d M=%d ranges=%d' % (q, m, nr)


# ---------------------------------------------------------------------------------------------------------------
# 4. n-splits
# ---------------------------------------------------------------------------------------------------------------
NS_VALUES = [1, 2, 3, 5, 8]


def reorder_tol(dt, n):
    """Two summation orders of n non-negative terms differ by at most 2 (n + 2) units in the last place relatively (each
    order is within (n - 1) u of the exact sum; the slabs are summed in fp64 and rounded once more)."""
    return 2.0 * (n + 2) * (2.0 ** -53 if dt == F64 else 2.0 ** -24)


@pytest.mark.parametrize('q', [4, 22])
@pytest.mark.parametrize('n', [57, 64, 65, 100])
def test_forced_n_splits(dev, n, q, monkeypatch):
    """DPGP_PSI2_NS in {1, 2, 3, 5, 8} at B = 2, M = 33, all algorithms.  The kernels round the rows per split differently (32
    for the MFMA kernels, 4 for the patch kernel, none for the pair-tile kernel): for these N no pair-path split is empty, the
    32-rounded MFMA path does get empty splits and must write zeros for them.  Held to the reference, and to the NS = 1 result
    within the sum-reordering tolerance."""
    case = ordinary_case(2, n, 33, q)
    ref = ordinary_ref(2, n, 33, q)
    one = {}
    for ns in NS_VALUES:
        assert (ns - 1) * -(-n // ns) < n
        monkeypatch.setenv('DPGP_PSI2_NS', str(ns))
        for dt, algo in ALGOS:
            got = psi2_call(dev, dt, algo, *case)
            what = 'N=%d Q=%d NS=%d %s' % (n, q, ns, tag(dt, algo))
            check_tol(got, ref, dt, what)
            if ns == 1:
                one[(dt, algo)] = npf(got)
            else:
                check(got, one[(dt, algo)], reorder_tol(dt, n), TOL_PSI2[dt]['atol_rel'], what + ' against NS=1')


@pytest.mark.parametrize('shape', [(2, 1100, 33, 4), (2, 700, 200, 3)], ids=['N1100_M33', 'N700_M200'])
def test_automatic_n_splits(dev, shape, monkeypatch):
    """psi2_nsplit's own choice where it is more than one split (tests/test_psi2_refs.py asserts that): B = 2, M = 33, N = 1100
    (the one-round rule of the pair-tile sizes) and B = 2, M = 200, N = 700 (M > 128: the list-schedule branch)."""
    monkeypatch.delenv('DPGP_PSI2_NS', raising=False)
    all_algorithms(dev, ordinary_case(*shape), ordinary_ref(*shape), 'B=%d N=%d M=%d Q=%d' % shape)


@pytest.mark.parametrize('n,ns', [(10, 8), (20, 7)])
def test_over_split(dev, n, ns, monkeypatch):
    """More n-splits asked for than ceil(N / ns)-row splits exist: N = 10 with DPGP_PSI2_NS = 8 (rows per split 2: splits 5 - 7
    start behind the last observation), N = 20 with 7.  The pair-tile kernel stores from inside its chunk loop, so an empty
    split would leave its slab unwritten and psi2_finish_kernel would sum the NaN the workspace was filled with; psi2_nsplit
    therefore steps the override down to the largest count without an empty split."""
    monkeypatch.setenv('DPGP_PSI2_NS', str(ns))
    for q in (4, 22):
        all_algorithms(dev, ordinary_case(2, n, 33, q), ordinary_ref(2, n, 33, q), 'N=%d NS=%d Q=%d' % (n, ns, q))


# ---------------------------------------------------------------------------------------------------------------
# 5. chunks
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('q', [3, 10, 13, 20])
def test_several_chunks_per_workgroup(dev, q, monkeypatch):
    """The pair-tile kernel with a 10 KB LDS budget (DPGP_PP_LDS_KB = 10) at N = 200, M = 24, B = 2: 3 chunks of 96, 96 and 8
    rows at KS = 2, 7 chunks of 32 (the last with 8 rows) at KS = 8 — later chunks add to what the owner stored, the last
    chunk is one partly filled tile; with three n-splits 67 rows per workgroup (KS = 8: 32 + 32 + 3)."""
    case = ordinary_case(2, 200, 24, q)
    ref = ordinary_ref(2, 200, 24, q)
    monkeypatch.setenv('DPGP_PP_LDS_KB', '10')
    for ns in (1, 3):
        monkeypatch.setenv('DPGP_PSI2_NS', str(ns))
        check_tol(psi2_call(dev, F32, 'auto', *case), ref, F32, 'pairs, 10 KB chunks, Q=%d NS=%d' % (q, ns))


def eight_against_four(dev, case, ref, what, monkeypatch):
    monkeypatch.setenv('DPGP_PSI2_NS', '1')
    monkeypatch.setenv('DPGP_PP_NW', '8')
    p8 = psi2_call(dev, F32, 'auto', *case)
    check_tol(p8, ref, F32, what + ', eight waves')
    monkeypatch.setenv('DPGP_PP_NW', '4')
    p4 = psi2_call(dev, F32, 'auto', *case)
    check_tol(p4, ref, F32, what + ', four waves')
    torch.testing.assert_close(p8, p4, rtol=1e-5, atol=1e-5 * float(p4.max()))


@pytest.mark.parametrize('q', [3, 10, 13, 20])
def test_eight_waves_single_chunk(dev, q, monkeypatch):
    """DPGP_PP_NW = 8 at N = 70 (one chunk), M = 24, B = 2, the four KS; compared with four waves as
    test_psi2_eight_wave_workgroups does."""
    eight_against_four(dev, ordinary_case(2, 70, 24, q), ordinary_ref(2, 70, 24, q), 'pairs Q=%d N=70' % q, monkeypatch)


def test_eight_waves_several_chunks(dev, monkeypatch):
    """Eight waves with several chunks at KS = 2: N = 2100, M = 24, Q = 2 (2016 rows fit the 160 KB; four waves: 3 chunks)."""
    eight_against_four(dev, ordinary_case(2, 2100, 24, 2), ordinary_ref(2, 2100, 24, 2), 'pairs Q=2 N=2100', monkeypatch)


# ---------------------------------------------------------------------------------------------------------------
# 6. accuracy far from the centre
# ---------------------------------------------------------------------------------------------------------------
FAR_N, FAR_M, FAR_B = 96, 24, 2
FAR_PATCH_QS = [1, 5, 10, 21, 30]


@functools.lru_cache(maxsize=None)
def far_case(q):
    """Two clusters: z and mu each half at +15 and half at -15 (plus N(0, 1)), length scales of order one (gamma = exp(0.3 N)),
    s = exp(0.5 N).  max_n |c''_n| is about 200 (Q = 1) to 2800 (Q = 21).  Seeded by Q alone, drawn in the order z, mu, s,
    gamma: the inputs at which the pair kernel's accuracy model was first measured."""
    rng = np.random.default_rng(q)
    z, mu = rng.standard_normal((FAR_M, q)), rng.standard_normal((FAR_N, q))
    z[:FAR_M // 2] += 15.0
    z[FAR_M // 2:] -= 15.0
    mu[:FAR_N // 2] += 15.0
    mu[FAR_N // 2:] -= 15.0
    s = np.exp(0.5 * rng.standard_normal((FAR_N, q)))
    gam = np.exp(0.3 * rng.standard_normal((FAR_B, q)))
    al = np.exp(0.3 * rng.standard_normal((FAR_B, 1))) * (1.0 + 0.25 * np.arange(FAR_B))[:, None]
    return tuple(r32(a) for a in (z, mu, s, gam, al))


@functools.lru_cache(maxsize=None)
def far_pairs_emulation(q):
    z, mu, s, gam, _ = far_case(q)
    return [pairs_emulated(z, mu, s, gam[b]) for b in range(FAR_B)]


@functools.lru_cache(maxsize=None)
def far_patch_emulation(q):
    z, mu, s, gam, _ = far_case(q)
    return [patch_emulated(z, mu, s, gam[b]) for b in range(FAR_B)]


@pytest.mark.parametrize('q', list(range(1, 22)))
def test_far_from_the_centre_pair_kernel(dev, q):
    """The pair-tile kernel (fp32 'auto', Q <= 21) at the two-cluster geometry.  Its documented model is an exponent good to
    ~|c''| 2^-21, i.e. a relative error of ln2 2^-21 max_n |c''_n| per output dim; the bound is twice that (the margin is for
    the MFMA's fp32 accumulation, which the CPU emulation — below 1x at exactly these inputs, tests/test_psi2_refs.py — does not
    model), plus the usual atol floor.  At Q = 21 that is 2 ln2 2^-21 2800 = 1.9e-3: above the suite's rtol 1e-4, which this
    kernel cannot meet here.  Q = 5 and Q = 21 carry c'' in 22 bits.  fp64 stays at TOL_PSI2."""
    case = far_case(q)
    ref, cmax = psi2_ld(*case)
    check_tol(psi2_call(dev, F64, 'auto', *case), ref, F64, 'far Q=%d f64 auto' % q)
    got = psi2_call(dev, F32, 'auto', *case)
    rel = check(got, ref, 2.0 * PAIR_MODEL * cmax, TOL_PSI2[F32]['atol_rel'], 'far Q=%d pairs (max|c\'\'| %.0f)' % (q, cmax.max()))
    print('far Q=%d pairs: max rel.err / (ln2 2^-21 max|c\'\'|) = %.2f' % (q, rel / (PAIR_MODEL * cmax.min())))


@pytest.mark.parametrize('q', FAR_PATCH_QS)
def test_far_from_the_centre_other_kernels(dev, q):
    """The other kernels at the two-cluster geometry.  patch_f16: twice the maximum exponent error of its CPU emulation on the
    same inputs (patch_emulated; measured there, in log2 units, Q = 1: 7.5e-5, 5: 2.2e-4, 10: 3.8e-4, 21: 8.6e-4, 30: 9.0e-4
    — as ln2 * that a relative error), plus the atol floor.  mfma_f32 and fp32 plain: rtol 2e-3, the project's
    far-from-origin tolerance (test_psi2_far_from_origin_is_translation_invariant).  fp64 plain: TOL_PSI2."""
    case = far_case(q)
    ref, _ = psi2_ld(*case)
    emu = far_patch_emulation(q)
    check(psi2_call(dev, F32, 'patch_f16', *case), ref, [2.0 * LN2 * e['err'] for e in emu], TOL_PSI2[F32]['atol_rel'],
          'far Q=%d patch_f16 (emulated %.1e)' % (q, max(e['err'] for e in emu)))
    for algo in ('mfma_f32', 'plain'):
        check(psi2_call(dev, F32, algo, *case), ref, 2e-3, TOL_PSI2[F32]['atol_rel'], 'far Q=%d f32 %s' % (q, algo))
    check_tol(psi2_call(dev, F64, 'plain', *case), ref, F64, 'far Q=%d f64 plain' % q)


# ---------------------------------------------------------------------------------------------------------------
# 7. range guards
# ---------------------------------------------------------------------------------------------------------------
GUARD_ROW = 7


def pair_guard_quantity(z, mu, s, g):
    """|c''_n| of every row in fp64 (psi2_pairs.hip: the row is out of range when c'' < -8192)."""
    c = z.mean(0)
    den = 2.0 * g * s + 1.0
    return np.abs(np.sum((g / den) * (mu - c) ** 2 * LOG2E + 0.5 * np.log2(den), axis=1))


def patch_guard_quantity(z, mu, s, g):
    """Per row in fp64 the largest of |c'_n| and |P[n, m]| over the patch's columns (psi2.hip, psi2_patch_f16p: out of range
    when c'_n < -30000 or |P[n, m]| > 30000), c'_n = -sum_q (1/2 w (mu - c)^2 log2e + 1/4 log2 den) = c''_n / 2,
    P[n, m] = c'_n + log2e sum_q w (z_mq - c_q) ((mu_nq - c_q) - (z_mq - c_q) / 4); padded columns have P = c'."""
    c = z.mean(0)
    den = 2.0 * g * s + 1.0
    w, mc, zs = g / den, mu - c, z - c
    cp = -np.sum(0.5 * w * mc ** 2 * LOG2E + 0.25 * np.log2(den), axis=1)
    p = cp[:, None] + LOG2E * np.einsum('nq,nmq->nm', w, zs[None] * (mc[:, None, :] - 0.25 * zs[None]))
    return np.maximum(np.abs(cp), np.abs(p).max(axis=1))


GUARDS = {'pairs': (2, 'auto', pair_guard_quantity, PAIR_GUARD), 'patch_f16': (2, 'patch_f16', patch_guard_quantity, PATCH_GUARD),
          'patch_auto_Q24': (24, 'auto', patch_guard_quantity, PATCH_GUARD)}


@functools.lru_cache(maxsize=None)
def guard_case(kernel, factor):
    """N = 40, M = 17, B = 2 (gamma = 1 for b = 0, 0.05 for b = 1); observation GUARD_ROW is moved out along the diagonal
    until its guard quantity for b = 0 is factor x the line (bisection in fp64 on the fp32-rounded inputs)."""
    q, _, quantity, line = GUARDS[kernel]
    rng = np.random.default_rng(77 + q)
    z, mu = r32(rng.standard_normal((17, q))), r32(rng.standard_normal((40, q)))
    s = r32(np.exp(0.5 * rng.standard_normal((40, q))))
    gam = r32(np.stack([np.ones(q), 0.05 * np.ones(q)]))
    al = r32([[1.1], [0.8]])

    def moved(d):
        m2 = mu.copy()
        m2[GUARD_ROW] = r32(z.mean(0) + d)
        return m2
    lo, hi = 0.0, 1000.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if quantity(z, moved(mid), s, gam[0])[GUARD_ROW] < factor * line:
            lo = mid
        else:
            hi = mid
    mu2 = moved(lo)
    got = quantity(z, mu2, s, gam[0])
    assert abs(got[GUARD_ROW] / line - factor) < 1e-4 and np.delete(got, GUARD_ROW).max() < 0.05 * line
    assert quantity(z, mu2, s, gam[1]).max() < 0.5 * line
    return z, mu2, s, gam, al


@pytest.mark.parametrize('kernel', list(GUARDS))
def test_range_guard_line(dev, kernel):
    """The range guards just inside (0.98 x) and just outside (1.02 x) their lines; the 2 % is arbitrary, five orders of
    magnitude above the fp32 rounding of the guarded quantity.
      pair-tile kernel (Q = 2, 'auto'): the row constant c''_n against the documented -8192;
      patch kernel ('patch_f16' at Q = 2, 'auto' at Q = 24): the row constant c'_n = c''_n / 2 against -30000 and every
        P[n, m] of the row against +-30000, whichever is reached first (patch_guard_quantity: here P[n, m] of the inducing
        point that lies furthest against the direction of the moved observation).
    Inside: every entry finite and within the bound of the far-from-the-centre tests (pairs: 2 ln2 2^-21 max|c''|; patch: twice
    its emulation, not below TOL_PSI2), and the far row contributes nothing measurable (the reference without it is the same).
    Outside: every entry of b = 0 is NaN, b = 1 (gamma = 0.05, far inside) is finite and correct.  fp64 and mfma_f32 have no
    such limit and are correct on both sides."""
    q, algo, _, _ = GUARDS[kernel]
    for factor in (0.98, 1.02):
        case = guard_case(kernel, factor)
        z, mu, s, gam, al = case
        ref, cmax = psi2_ld(*case)
        without, _ = psi2_ld(z, np.delete(mu, GUARD_ROW, axis=0), np.delete(s, GUARD_ROW, axis=0), gam, al)
        np.testing.assert_allclose(ref[0], without[0], rtol=1e-15, atol=0)
        what = '%s guard x%.2f ' % (kernel, factor)
        check_tol(psi2_call(dev, F64, 'auto', *case), ref, F64, what + 'f64 auto')
        check(psi2_call(dev, F32, 'mfma_f32', *case), ref, 2e-3, TOL_PSI2[F32]['atol_rel'], what + 'f32 mfma_f32')
        got = psi2_call(dev, F32, algo, *case)
        if kernel == 'pairs':
            rtol = np.maximum(2.0 * PAIR_MODEL * cmax, TOL_PSI2[F32]['rtol'])
        else:
            rtol = [max(2.0 * LN2 * patch_emulated(z, mu, s, gam[b])['err'], TOL_PSI2[F32]['rtol']) for b in range(2)]
        if factor < 1.0:
            assert bool(torch.isfinite(got).all()), what + 'inside the line: must be finite'
            check(got, ref, rtol, TOL_PSI2[F32]['atol_rel'], what + 'inside')
        else:
            assert bool(torch.isnan(got[0]).all()), what + 'outside the line: every entry of b = 0 must be NaN'
            assert bool(torch.isfinite(got[1]).all()), what + 'b = 1 is far inside and must stay finite'
            check(got[1:], ref[1:], rtol[1], TOL_PSI2[F32]['atol_rel'], what + 'outside, b = 1')


# ---------------------------------------------------------------------------------------------------------------
# 8. exponent range
# ---------------------------------------------------------------------------------------------------------------
SWEEP_T = [0, 1, 100, 125, 127, 140, 149, 151, 300, 1000, 1021, 1023, 1074, 1076, 1101, 2000]


@functools.lru_cache(maxsize=None)
def sweep_case(where, t):
    """N = 1, M = 2, Q = 1, gamma = 1, s = 1/2 (den = 2), alpha = 2^(1/4) (so that alpha^2 den^(-1/2) = 1 up to rounding).
    'beta': z = -+D/2, mu = 0 with 1/4 D^2 log2e = t: the off-diagonal entry is 2^-t through beta (the diagonal ones 2^(-t/2)
    through E).  'E': z_0 = z_1 = 0, mu = d with 1/2 d^2 log2e = t: all entries 2^-t through E (c'' = -t - 1/2)."""
    if where == 'beta':
        d = math.sqrt(4.0 * t / LOG2E)
        z, mu = r32([[-0.5 * d], [0.5 * d]]), np.zeros((1, 1))
    else:
        z, mu = np.zeros((2, 1)), r32([[math.sqrt(2.0 * t / LOG2E)]])
    return z, mu, np.full((1, 1), 0.5), np.ones((1, 1)), r32([[2.0 ** 0.25]])


@pytest.mark.parametrize('where', ['beta', 'E'])
def test_exponent_range(dev, where):
    """Results from 1 down to and past 2^-126 (fp32; v_exp_f32 flushes), 2^-1022 (fp64) and 2^-1100 (the clamp of
    dpgp_exp2_tab), once through the beta factor (the scale kernel's / epilogue's exponential) and once through E (the hot
    loop's).  Per entry, with no atol floor relative to the largest entry: where the reference is a normal number of the type
    the result is within TOL_PSI2's rtol; below that it is 0 or within rtol plus two units of the subnormal grid (2^-149 /
    2^-1074; subnormals carry fewer bits, and the result is a product of a rounded sum and rounded factors: each of up to three
    roundings on that grid is half a unit, scaled by factors up to sqrt 2).  Nothing is NaN, infinite or negative.  The E sweep stays
    inside the f16 kernels' guards up to t = 2000 (|c''| = 2000.5 < 8192)."""
    for t in SWEEP_T:
        case = sweep_case(where, t)
        ref, _ = psi2_ld(*case)
        for dt, algo in ALGOS:
            got = npf(psi2_call(dev, dt, algo, *case))[0]
            tiny, grid = (2.0 ** -1022, 2.0 ** -1074) if dt == F64 else (2.0 ** -126, 2.0 ** -149)
            rtol = TOL_PSI2[dt]['rtol']
            what = '%s sweep t=%d %s' % (where, t, tag(dt, algo))
            assert np.isfinite(got).all() and (got >= 0).all(), (what, got)
            r = ref[0]
            with np.errstate(divide='ignore', invalid='ignore'):
                rel = np.where(r >= tiny, np.abs(got - r) / r, 0.0)
            print('%-40s log2 ref %9.2f .. %9.2f   max rel.err (normal entries) %.2e   got %s'
                  % (what, np.log2(np.maximum(r.min(), 5e-324)), np.log2(np.maximum(r.max(), 5e-324)), rel.max(), got.ravel()))
            ok_normal = np.abs(got - r) <= rtol * r
            ok_small = (got == 0) | (np.abs(got - r) <= rtol * r + 2.0 * grid)
            assert np.where(r >= tiny, ok_normal, ok_small).all(), (what, got, r)


# ---------------------------------------------------------------------------------------------------------------
# 9. NaN
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('where', ['mu', 's', 'z', 'gamma', 'alpha'])
def test_nan_inputs_give_nan(dev, where):
    """One NaN input, all algorithms, B = 2, N = 37, M = 17, Q = 3.  Entries that depend on it must be NaN, never silently
    finite: mu[3, 1] or s[3, 1] -> every entry of every b (each is a sum over all observations); z[5, 1] -> at least row and
    column 5 of every b (the kernels that centre z by its column mean make everything NaN); gamma[1, 1] or alpha[1] -> every
    entry of b = 1, while b = 0 does not depend on it and stays within tolerance."""
    z, mu, s, gam, al = (np.array(a, copy=True) for a in ordinary_case(2, 37, 17, 3))
    ref = ordinary_ref(2, 37, 17, 3)
    target, index = {'mu': (mu, (3, 1)), 's': (s, (3, 1)), 'z': (z, (5, 1)), 'gamma': (gam, (1, 1)), 'alpha': (al, (1, 0))}[where]
    target[index] = np.nan
    for dt, algo in ALGOS:
        got = npf(psi2_call(dev, dt, algo, z, mu, s, gam, al))
        what = 'NaN in %s, %s' % (where, tag(dt, algo))
        if where in ('mu', 's'):
            assert np.isnan(got).all(), what
        elif where == 'z':
            assert np.isnan(got[:, 5, :]).all() and np.isnan(got[:, :, 5]).all(), what
        else:
            assert np.isnan(got[1]).all(), what
            check_tol(got[:1], ref[:1], dt, what + ', b = 0')
