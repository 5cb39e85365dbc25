"""
The four public dense operators — ops.potrf_batched, ops.trsm_batched, ops.tril_inverse_batched, ops.matmul (csrc/linalg.hip, potrf_big.hip,
potrf_persist.hip, gemm.hip, linalg_dev.h) — at every compiled form and dispatch edge, on well-conditioned matrices and on the RBF grams
with jitter that the models factor (cond ~ 1e10 in fp64), judged by componentwise backward errors against two limits: a derivable cap and
8 x LAPACK's own figure on the same case (tests/test_dense_refs.py holds the recipes, figures, limits, case tables and the dispatch mirror,
and the CPU tests that show they can be trusted).

Families: P1 potrf at every tile count to 128 (both loader paths), P2 fp32 residency to 176, P3 the multi-workgroup routine with and without
look-ahead, P4 the persistent kernels left- and right-looking and the library's own choice of them; T trsm at every chunk shape; I the
inverse, persistent and fallback; G gemm at every K-step, tile edge, layout and view; F failure reporting (info = first failing pivot + 1);
B independence of the matrices of a batch and run-to-run reproducibility; U the triangle contract (nothing above the diagonal is read);
C guard bands around every operand, output and workspace of the C ABI.  The forms are chosen through DPGP_POTRF_PERSISTENT,
DPGP_POTRF_LEFT and DPGP_POTRF_NO_LOOKAHEAD, which the library reads on every call.  Every test prints
    dense-edges <family> <case>: fig=<figure in u> ref=<LAPACK's> ratio=<fig / max(ref, 2)>
"""
import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import _lib, ops
import test_dense_refs as R

pytestmark = pytest.mark.gpu
TD = {'f64': torch.float64, 'f32': torch.float32}
VARS = (R.V_PERSIST, R.V_LEFT, R.V_NOLA)


def on(dev, a):
    return torch.as_tensor(np.array(a), device=dev)             # (a copy: the cases are read-only)


def set_form(monkeypatch, form):
    for v in VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in R.ENVS[form].items():
        monkeypatch.setenv(k, v)


def held(family, what, tiles, cap, f_ref, cap_only=False):
    """Print the figure, then hold it to both limits (cap_only: to the cap alone — R.CAP_ONLY says which cases and why)."""
    R.report(family, what, float(tiles.max()), f_ref)
    return R.judge(tiles, cap, f_ref, what, cap_only)


def ids(v):
    return '-'.join(str(x) for x in v) if isinstance(v, tuple) else str(v)


# --------------------------------------------------------------------------------------------------------------------
# P: potrf
# --------------------------------------------------------------------------------------------------------------------
def check_potrf(dev, monkeypatch, case, family):
    recipe, m, dt, algo, b, form = case
    set_form(monkeypatch, form)
    a = R.spd(recipe, m, dt, b)
    l, info = ops.potrf_batched(on(dev, a), algo=algo)
    what = '%s M=%d %s %s B=%d %s' % (recipe, m, dt, algo, b, R.potrf_form(b, m, dt, algo, R.ENVS[form]))
    assert not info.cpu().numpy().any(), (what, info)
    l = l.cpu().numpy()
    held(family, what, R.potrf_figure(a, l), R.potrf_cap(m), R.lapack_potrf(recipe, m, dt, b), R.cap_only(case))
    assert R.upper_nonzeros(l) == 0, what + ': non-zeros above the diagonal'


@pytest.mark.parametrize('algo', ['auto', 'plain'])
@pytest.mark.parametrize('dt', ['f64', 'f32'])
@pytest.mark.parametrize('m', R.P1_MS)
def test_potrf_at_every_tile_count(dev, monkeypatch, m, dt, algo):
    """P1: 1 ... 8 tile rows, M = 16 b - 15, 16 b - 14, 16 b - 1, 16 b: the resident kernel (pair loader for even M in fp64, scalar
    otherwise) and the plain cross-check path."""
    cases = [c for c in R.P1 if c[1:4] == (m, dt, algo)]
    assert cases
    for c in cases:
        check_potrf(dev, monkeypatch, c, 'P1')


@pytest.mark.parametrize('case', R.P2, ids=ids)
def test_potrf_fp32_residency(dev, monkeypatch, case):
    """P2: fp32 keeps 9 to 11 tile rows in LDS (M <= 176) and moves to the multi-workgroup routine at 177."""
    check_potrf(dev, monkeypatch, case, 'P2')


@pytest.mark.parametrize('case', R.P3, ids=ids)
def test_potrf_multi_workgroup(dev, monkeypatch, case):
    """P3: 2 to 6 blocks of 128, in place and on a padded copy, with look-ahead and without."""
    check_potrf(dev, monkeypatch, case, 'P3')


@pytest.mark.parametrize('case', R.P4, ids=ids)
def test_potrf_persistent(dev, monkeypatch, case):
    """P4: one persistent workgroup per matrix, left-looking (the default) and right-looking.  (The rows below a diagonal block are solved
    with explicit inverses of its 16 x 16 diagonal tiles, pp_trsm_tile: without its refinement step the grams gave 3e2 .. 8e3 u in the
    first tile column of those rows, where the limits are 1e2 .. 3e2 u.)"""
    check_potrf(dev, monkeypatch, case, 'P4')


def test_potrf_library_picks_the_persistent_form(dev, monkeypatch):
    """P4: no variable set, B = 128, M = 129."""
    check_potrf(dev, monkeypatch, R.P4_DEFAULT, 'P4')


# --------------------------------------------------------------------------------------------------------------------
# T, I: trsm and the inverse
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['f64', 'f32'])
@pytest.mark.parametrize('m,k', R.T_SHAPES)
def test_trsm_at_every_chunk_shape(dev, m, k, dt):
    """T: one to three chunks of 64 right-hand sides with last widths 1, 63, 64 (a narrower padded stride in the last chunk), 1 to 13
    tile rows; blocked (explicit inverses of the diagonal tiles) and plain."""
    r = R.rhs(m, k, dt, R.T_B)
    for recipe in ('gram', 'wishart'):
        l = R.factor(recipe, m, dt, R.T_B)
        cap, f_ref = R.solve_cap(l), R.lapack_trsm(recipe, m, k, dt, R.T_B)
        for algo in ('auto', 'plain'):
            x = ops.trsm_batched(on(dev, l), on(dev, r), algo=algo).cpu().numpy()
            held('T', '%s M=%d K=%d %s %s chunks=%s' % (recipe, m, k, dt, algo, R.trsm_chunks(k)), R.solve_figure(l, x, r), cap, f_ref)


@pytest.mark.parametrize('m,b', R.I_PERSISTENT + R.I_FALLBACK)
def test_inverse_persistent_and_fallback(dev, m, b):
    """I: the persistent solve on the identity (M a multiple of 128: 1, 2, 3 and 5 blocks) and the column-chunk kernel otherwise;
    exactly 0.0 above the diagonal."""
    for recipe in R.inverse_recipes(m, b):
        l = R.factor(recipe, m, 'f64', b)
        w = ops.tril_inverse_batched(on(dev, l)).cpu().numpy()
        what = '%s M=%d B=%d %s' % (recipe, m, b, 'fallback' if m % 128 else 'persistent')
        held('I', what, R.solve_figure(l, w, R.eye(m, 'f64', b)), R.solve_cap(l), R.lapack_inverse(recipe, m, 'f64', b))
        assert R.upper_nonzeros(w) == 0, what + ': non-zeros above the diagonal'
        assert not np.signbit(np.triu(w, 1)).any(), what + ': -0.0 above the diagonal'


# --------------------------------------------------------------------------------------------------------------------
# G: gemm
# --------------------------------------------------------------------------------------------------------------------
def stored_transposed(t):
    """The same logical tensor with its last two dims stored the other way round (i- / j-contiguous instead of k-contiguous)."""
    return t.transpose(-1, -2).contiguous().transpose(-1, -2)


def numpy_ref(a, b, alpha=1.0, beta=0.0, c0=None):
    c = alpha * np.matmul(a, b)
    return c if beta == 0.0 else c + beta * c0


def check_gemm(what, got, a, b, alpha=1.0, beta=0.0, c0=None):
    """got (device) against alpha a b + beta c0 (NumPy views): both limits, f_ref = NumPy's matmul of the same views."""
    k = a.shape[-1]
    ref = numpy_ref(a, b, alpha, beta, c0)
    f_ref = float(R.gemm_figure(ref, a, b, alpha, beta, c0).max())
    return held('G', what, R.gemm_figure(got.cpu().numpy(), a, b, alpha, beta, c0), R.gemm_cap(k), f_ref)


@pytest.mark.parametrize('k', R.G_KS)
def test_gemm_at_every_k_step_tile_edge_and_layout(dev, k):
    """G: k from 0 over every K-step remainder to 129, m and n on both sides of the 64-tile, each operand k-contiguous or not."""
    for m, n in R.G_MN:
        a, b, _ = R.gemm_operands(R.G_B, m, n, k)
        ta, tb = on(dev, a), on(dev, b)
        for tra, trb in R.G_LAYOUTS:
            xa, xb = stored_transposed(ta) if tra else ta, stored_transposed(tb) if trb else tb
            if k > 1 and m > 1:
                assert (xa.stride(-1) == 1) == (not tra)
            check_gemm('%dx%dx%d A%s B%s' % (m, n, k, 'ik'[tra], 'kj'[trb]), ops.matmul(xa, xb), a, b)


def test_gemm_views(dev):
    """G: 2-D operands broadcast over the batch, stride-0 expansions, sliced rows, a strided out with beta != 0, beta = 0 into NaN."""
    m, n, k = R.G_EDGE
    a, b, c0 = R.gemm_operands(R.G_B, m, n, k)
    ta, tb = on(dev, a), on(dev, b)
    check_gemm('2-D A', ops.matmul(ta[0], tb), a[0], b)
    check_gemm('2-D B', ops.matmul(ta, tb[1]), a, b[1])
    check_gemm('2-D both', ops.matmul(ta[1], tb[0]), a[1], b[0])
    check_gemm('batch-expanded A', ops.matmul(ta[1:2].expand(R.G_B, m, k), tb), np.broadcast_to(a[1:2], a.shape), b)
    check_gemm('batch-expanded B', ops.matmul(ta, tb[0:1].expand(R.G_B, k, n)), a, np.broadcast_to(b[0:1], b.shape))
    col, row = tb[:, :, 3:4].expand(R.G_B, k, n), ta[:, 5:6, :].expand(R.G_B, m, k)
    assert col.stride(-1) == 0 and row.stride(-2) == 0
    check_gemm('column-expanded B', ops.matmul(ta, col), a, np.broadcast_to(b[:, :, 3:4], b.shape))
    check_gemm('row-expanded A', ops.matmul(row, tb), np.broadcast_to(a[:, 5:6, :], a.shape), b)
    check_gemm('rows ::2 of A', ops.matmul(ta[:, ::2, :], tb), a[:, ::2, :], b)
    check_gemm('k ::2 of both', ops.matmul(ta[:, :, ::2], tb[:, ::2, :]), a[:, :, ::2], b[:, ::2, :])
    # out: a strided slice of a larger tensor, beta != 0; everything outside the view stays
    g = np.random.default_rng(11)
    big = g.standard_normal((R.G_B, m + 7, 2 * n + 9))
    tbig = on(dev, big)
    view = tbig[:, 3:3 + m, 5:5 + 2 * n:2]
    assert tuple(view.shape) == (R.G_B, m, n) and view.stride(-1) == 2
    ops.matmul(ta, tb, out=view, alpha=-0.5, beta=2.0)
    check_gemm('strided out, beta=2', view, a, b, -0.5, 2.0, big[:, 3:3 + m, 5:5 + 2 * n:2])
    after = tbig.cpu().numpy()
    outside = np.ones(big.shape, dtype=bool)
    outside[:, 3:3 + m, 5:5 + 2 * n:2] = False
    assert np.array_equal(after[outside].view(np.int64), big[outside].view(np.int64)), 'written outside the out view'
    # beta = 0 never reads out (as BLAS has it): NaN in out does not reach the result
    out = torch.full((R.G_B, m, n), float('nan'), dtype=torch.float64, device=dev)
    ops.matmul(ta, tb, out=out, alpha=1.5, beta=0.0)
    assert bool(torch.isfinite(out).all())
    check_gemm('beta=0 into NaN', out, a, b, 1.5)


def test_gemm_k_zero(dev):
    """G: k = 0 is beta C (exactly 0.0 for beta = 0, whatever out held)."""
    for m, n in R.G_MN:
        a, b, c0 = R.gemm_operands(R.G_B, m, n, 0)
        ta, tb = on(dev, a), on(dev, b)
        out = torch.full((R.G_B, m, n), float('nan'), dtype=torch.float64, device=dev)
        ops.matmul(ta, tb, out=out, alpha=3.0, beta=0.0)
        assert bool((out == 0.0).all()), 'k = 0, beta = 0'
        out = on(dev, c0)
        ops.matmul(ta, tb, out=out, alpha=3.0, beta=2.0)
        check_gemm('%dx%dx0 beta=2' % (m, n), out, a, b, 3.0, 2.0, c0)
        assert np.array_equal(out.cpu().numpy(), 2.0 * c0)


def test_gemm_batch_beyond_the_grid_limit(dev):
    """G: 65,537 matrices: the grid's z extent stops at 65,535 and the kernel loops (bz += gridDim.z), two of them a second round."""
    batch, m, n, k = R.G_HUGE
    a, b, _ = R.gemm_operands(batch, m, n, k)
    got = ops.matmul(on(dev, a), on(dev, b)).cpu().numpy()
    per = R.gemm_ratio(got, a, b).max(axis=(1, 2)).reshape(batch, 1, 1)
    f_ref = float(R.gemm_ratio(np.matmul(a, b), a, b).max())
    held('G', 'batch=%d %dx%dx%d' % R.G_HUGE, per, R.gemm_cap(k), f_ref)


# --------------------------------------------------------------------------------------------------------------------
# F: failure reporting
# --------------------------------------------------------------------------------------------------------------------
RESIDENT_FORMS = [(100, 'f64', 'auto'), (100, 'f64', 'plain'), (100, 'f32', 'auto'), (160, 'f32', 'auto')]
F_PIVOTS = {100: (0, 15, 16, 99), 160: (0, 128, 159), 300: (0, 127, 128, 255, 256, 299), 384: (0, 383)}
F_PAIRS = {100: ((15, 16), (0, 99)), 160: ((128, 159),), 300: ((127, 128), (0, 299), (128, 256)), 384: ((0, 383),)}
F_NAN_DIAG = {100: (16, 99), 160: (128,), 300: (0, 128, 299), 384: (383,)}
F_NAN_BELOW = {100: ((16, 3), (99, 98)), 160: ((130, 2),), 300: ((128, 127), (200, 3), (299, 256)), 384: ((383, 0),)}
BIG_FORM_CASES = [(m, 'f64', form) for m in (300, 384) for form in R.BIG_FORMS] + [(300, 'f32', 'multi')]


def lowered(m, dt, pivots, idx=0):
    """gram(m) with pivot p made equal to -L0[p,p]^2 for each p in pivots: the p-th diagonal entry lowered by 2 L0[p,p]^2 (L0: LAPACK's
    factor), so that the leading p x p block is untouched and the failure is as far from marginal as the pivot was."""
    a = np.array(R.spd('gram', m, dt, idx + 1)[idx])
    l0 = R.factor('gram', m, dt, idx + 1)[idx]
    for p in pivots:
        a[p, p] -= 2 * l0[p, p] ** 2
    return a


def failure_batch(m, dt):
    """(matrices [B,M,M], info wanted [B], what each is)"""
    mats, want, names = [], [], []
    for p in F_PIVOTS[m]:
        mats.append(lowered(m, dt, (p,)))
        want.append(p + 1)
        names.append('pivot %d' % p)
    for p1, p2 in F_PAIRS[m]:
        mats.append(lowered(m, dt, (p1, p2)))
        want.append(p1 + 1)
        names.append('pivots %d and %d' % (p1, p2))
    for p in F_NAN_DIAG[m]:
        a = np.array(R.spd('gram', m, dt, 1)[0])
        a[p, p] = np.nan
        mats.append(a)
        want.append(p + 1)
        names.append('NaN at (%d, %d)' % (p, p))
    for i, j in F_NAN_BELOW[m]:
        a = np.array(R.spd('gram', m, dt, 1)[0])
        a[i, j] = np.nan
        mats.append(a)
        want.append(i + 1)
        names.append('NaN at (%d, %d)' % (i, j))
    return np.stack(mats), want, names


def check_failures(dev, m, dt, algo, what):
    a, want, names = failure_batch(m, dt)
    _, info = ops.potrf_batched(on(dev, a), algo=algo)
    got = info.cpu().tolist()
    print('dense-edges F %s: info %s' % (what, got))
    bad = ['%s: info %d, not %d' % (n, g, w) for n, g, w in zip(names, got, want) if g != w]
    assert not bad, (what, bad)


@pytest.mark.parametrize('m,dt,algo', RESIDENT_FORMS, ids=ids)
def test_failure_reporting_resident(dev, monkeypatch, m, dt, algo):
    """F: a negative pivot in the first tile, at a tile's last and first row and in the last row; two failures; NaN on and below the
    diagonal — info is the first failing pivot + 1."""
    set_form(monkeypatch, 'none')
    check_failures(dev, m, dt, algo, 'M=%d %s %s' % (m, dt, algo))


@pytest.mark.parametrize('m,dt,form', BIG_FORM_CASES, ids=ids)
def test_failure_reporting_large(dev, monkeypatch, m, dt, form):
    """F: the same in block 0 of a multi-block matrix, at a 128-block's last and first row and in the padded last block."""
    set_form(monkeypatch, form)
    check_failures(dev, m, dt, 'auto', 'M=%d %s %s' % (m, dt, form))


# --------------------------------------------------------------------------------------------------------------------
# B: independence and reproducibility
# --------------------------------------------------------------------------------------------------------------------
B_FORMS = [(m, dt, algo, 'none') for m, dt, algo in RESIDENT_FORMS] + [(300, 'f64', 'auto', form) for form in R.BIG_FORMS] + [
    (256, 'f64', 'auto', form) for form in R.BIG_FORMS] + [(300, 'f32', 'auto', 'multi')]


def bits(t):
    return t.cpu().numpy().view(np.int64 if t.dtype == torch.float64 else np.int32)


@pytest.mark.parametrize('m,dt,algo,form', B_FORMS, ids=ids)
def test_matrices_of_a_batch_do_not_influence_each_other(dev, monkeypatch, m, dt, algo, form):
    """B: [good, failing, good]: the good ones come out bit-identical to their solo runs with info 0; two runs are bit-identical."""
    set_form(monkeypatch, form)
    good = R.spd('gram', m, dt, 3)
    a = np.stack([good[0], lowered(m, dt, (m // 2,), idx=1), good[2]])
    ta = on(dev, a)
    l, info = ops.potrf_batched(ta, algo=algo)
    assert info.cpu().tolist() == [0, m // 2 + 1, 0]
    for i in (0, 2):
        solo, solo_info = ops.potrf_batched(ta[i:i + 1], algo=algo)
        assert int(solo_info[0]) == 0
        assert np.array_equal(bits(l[i]), bits(solo[0])), 'matrix %d differs from its solo run' % i
    l2, info2 = ops.potrf_batched(ta, algo=algo)
    assert torch.equal(info, info2) and all(np.array_equal(bits(l[i]), bits(l2[i])) for i in (0, 2)), 'two runs differ'
    tiles = R.potrf_figure(a[[0, 2]], l[[0, 2]].cpu().numpy())
    f_ref = float(R.potrf_figure(a[[0, 2]], R.factor('gram', m, dt, 3)[[0, 2]]).max())
    held('B', 'M=%d %s %s %s' % (m, dt, algo, form), tiles, R.potrf_cap(m), f_ref)


@pytest.mark.parametrize('dt', ['f64', 'f32'])
def test_solves_are_reproducible_and_independent(dev, dt):
    """B: trsm and the inverse: a NaN matrix in the batch leaves the others bit-identical to their solo runs; two runs are bit-identical."""
    m, k = 129, 65
    l, r = np.array(R.factor('gram', m, dt, 3)), R.rhs(m, k, dt, 3)
    l[1, 70, 3] = np.nan
    tl, tr = on(dev, l), on(dev, r)
    for algo in ('auto', 'plain'):
        x = ops.trsm_batched(tl, tr, algo=algo)
        assert torch.equal(x[[0, 2]], ops.trsm_batched(tl, tr, algo=algo)[[0, 2]])
        for i in (0, 2):
            assert torch.equal(x[i], ops.trsm_batched(tl[i:i + 1], tr[i:i + 1], algo=algo)[0]), (algo, i)
    if dt == 'f64':
        for mm in (129, 256):
            l = np.array(R.factor('gram', mm, dt, 3))
            l[1, 70, 3] = np.nan
            tl = on(dev, l)
            w = ops.tril_inverse_batched(tl)
            assert torch.equal(w[[0, 2]], ops.tril_inverse_batched(tl)[[0, 2]])
            for i in (0, 2):
                assert torch.equal(w[i], ops.tril_inverse_batched(tl[i:i + 1])[0]), (mm, i)


# --------------------------------------------------------------------------------------------------------------------
# U: the triangle contract
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', ['f64', 'f32'])
def test_solves_never_read_above_the_diagonal(dev, dt):
    """U: NaN above the diagonal of L changes no bit of trsm's or the inverse's result (tf.matrix_triangular_solve ignores that triangle)."""
    for m, k in ((17, 65), (129, 65), (128, 9)):
        l, r = R.factor('gram', m, dt, 2), R.rhs(m, k, dt, 2)
        dirty = l + np.triu(np.full((m, m), np.nan, dtype=l.dtype), 1)
        for algo in ('auto', 'plain'):
            clean = ops.trsm_batched(on(dev, l), on(dev, r), algo=algo)
            assert bool(torch.isfinite(clean).all())
            assert torch.equal(clean, ops.trsm_batched(on(dev, dirty), on(dev, r), algo=algo)), (m, k, algo)
    if dt == 'f64':
        for m in (128, 129, 256, 384):
            l = R.factor('gram', m, dt, 2)
            dirty = l + np.triu(np.full((m, m), np.nan), 1)
            clean = ops.tril_inverse_batched(on(dev, l))
            assert bool(torch.isfinite(clean).all())
            assert torch.equal(clean, ops.tril_inverse_batched(on(dev, dirty))), m


U_FORMS = [(m, dt, algo, 'none') for m in (99, 100, 128) for dt, algo in (('f64', 'auto'), ('f64', 'plain'), ('f32', 'auto'))] + [
    (160, 'f32', 'auto', 'none'), (300, 'f32', 'auto', 'multi')] + [(m, 'f64', 'auto', form) for m in (256, 300) for form in R.BIG_FORMS]


@pytest.mark.parametrize('m,dt,algo,form', U_FORMS, ids=ids)
def test_potrf_reads_the_lower_triangle_only(dev, monkeypatch, m, dt, algo, form):
    """U: the strict upper triangle doubled changes no bit of L (tf.cholesky reads the lower triangle only)."""
    set_form(monkeypatch, form)
    a = R.spd('gram', m, dt, 2)
    clean, info = ops.potrf_batched(on(dev, a), algo=algo)
    other, info2 = ops.potrf_batched(on(dev, a + np.triu(a, 1)), algo=algo)
    assert not info.cpu().numpy().any() and not info2.cpu().numpy().any()
    assert torch.equal(clean, other)


# --------------------------------------------------------------------------------------------------------------------
# C: guard bands around every buffer of the C ABI
# --------------------------------------------------------------------------------------------------------------------
BAND, PATTERN = 4096, 0xA5


class Arena:
    """One device buffer; every slice of it has BAND bytes of PATTERN before and after it (bases aligned to 256 bytes)."""

    def __init__(self, dev, sizes):
        self.spans, cur = [], 0
        for n in sizes:
            cur += BAND
            self.spans.append((cur, int(n)))
            cur = R._up(cur + int(n) + BAND, 256)
        self.buf = torch.full((cur,), PATTERN, dtype=torch.uint8, device=dev)

    def view(self, i, dtype=torch.uint8):
        off, n = self.spans[i]
        return self.buf[off:off + n].view(dtype)

    def put(self, i, array):
        t = torch.as_tensor(np.array(array))
        v = self.view(i, t.dtype)
        assert v.numel() == t.numel()
        v.copy_(t.reshape(-1))
        return v

    def check(self, what):
        host = self.buf.cpu().numpy()
        live = np.zeros(host.shape, dtype=bool)
        for off, n in self.spans:
            live[off:off + n] = True
        hit = np.nonzero(~live & (host != PATTERN))[0]
        if hit.size:
            i = int(np.searchsorted([off for off, _ in self.spans], hit[0], side='right')) - 1
            where = 'before slice 0' if i < 0 else 'slice %d + %d bytes (its size: %d)' % (i, hit[0] - self.spans[i][0], self.spans[i][1])
            raise AssertionError('%s: %d guard bytes overwritten, the first at %s' % (what, hit.size, where))


def stream():
    return torch.cuda.current_stream().cuda_stream


C_POTRF = [(127, 'f64', 'auto', 'none'), (128, 'f64', 'auto', 'none'), (127, 'f32', 'auto', 'none'), (176, 'f32', 'auto', 'none'),
           (127, 'f64', 'plain', 'none'), (129, 'f64', 'plain', 'none')] + [(m, 'f64', 'auto', form) for m in (129, 256) for form in R.BIG_FORMS] + [
               (129, 'f32', 'auto', 'multi'), (256, 'f32', 'auto', 'multi')]


@pytest.mark.parametrize('m,dt,algo,form', C_POTRF, ids=ids)
def test_potrf_writes_nothing_outside_its_buffers(dev, monkeypatch, m, dt, algo, form):
    """C: the matrices, info and a workspace of exactly the queried size as slices of one buffer, 4 KiB of a fixed pattern around each."""
    set_form(monkeypatch, form)
    b, lib = 2, _lib.lib()
    a = R.spd('gram', m, dt, b)
    wsb = lib.dpgp_potrf_workspace_bytes(b, m, R.ELEM[dt])
    assert wsb == R.potrf_ws_bytes(b, m, R.ELEM[dt])
    ar = Arena(dev, [a.nbytes, 4 * b, wsb])
    ta, info, ws = ar.put(0, a), ar.view(1, torch.int32), ar.view(2)
    ar.check('before the call')
    _lib.check(getattr(lib, 'dpgp_potrf_batched_' + dt)(b, m, ta.data_ptr(), info.data_ptr(), ws.data_ptr(), wsb, _lib.ALGO[algo], stream()), 'potrf')
    torch.cuda.synchronize()
    what = 'potrf M=%d %s %s %s' % (m, dt, algo, form)
    ar.check(what)
    assert info.cpu().tolist() == [0] * b
    held('C', what, R.potrf_figure(a, ta.cpu().numpy().reshape(b, m, m)), R.potrf_cap(m), R.lapack_potrf('gram', m, dt, b))


@pytest.mark.parametrize('m,k,dt,algo', [(33, 65, 'f64', 'auto'), (33, 65, 'f64', 'plain'), (33, 65, 'f32', 'auto'), (129, 65, 'f64', 'auto'),
                                         (17, 1, 'f32', 'plain')], ids=ids)
def test_trsm_writes_nothing_outside_its_buffers(dev, m, k, dt, algo):
    b, lib = 2, _lib.lib()
    l, r = R.factor('gram', m, dt, b), R.rhs(m, k, dt, b)
    wsb = lib.dpgp_trsm_workspace_bytes(b, m, k, R.ELEM[dt])
    assert wsb == R.trsm_ws_bytes(b, m, k, R.ELEM[dt])
    ar = Arena(dev, [l.nbytes, r.nbytes, wsb])
    tl, tx, ws = ar.put(0, l), ar.put(1, r), ar.view(2)
    _lib.check(getattr(lib, 'dpgp_trsm_batched_' + dt)(b, m, k, tl.data_ptr(), tx.data_ptr(), ws.data_ptr(), wsb, _lib.ALGO[algo], stream()), 'trsm')
    torch.cuda.synchronize()
    what = 'trsm M=%d K=%d %s %s' % (m, k, dt, algo)
    ar.check(what)
    assert np.array_equal(tl.cpu().numpy().reshape(l.shape), l), 'L was modified'
    held('C', what, R.solve_figure(l, tx.cpu().numpy().reshape(r.shape), r), R.solve_cap(l), R.lapack_trsm('gram', m, k, dt, b))


@pytest.mark.parametrize('m', [128, 256])
def test_persistent_inverse_writes_nothing_outside_its_buffers(dev, m):
    b, lib = 3, _lib.lib()
    l = R.factor('gram', m, 'f64', b)
    ar = Arena(dev, [l.nbytes, l.nbytes, 8 * b])
    tl, out, ws = ar.put(0, l), ar.view(1, torch.float64), ar.view(2)
    _lib.check(lib.dpgp_trtri_lower_batched_f64(b, m, tl.data_ptr(), out.data_ptr(), ws.data_ptr(), 8 * b, stream()), 'trtri')
    torch.cuda.synchronize()
    ar.check('inverse M=%d' % m)
    assert np.array_equal(tl.cpu().numpy().reshape(l.shape), l), 'L was modified'
    w = out.cpu().numpy().reshape(l.shape)
    held('C', 'inverse M=%d' % m, R.solve_figure(l, w, R.eye(m, 'f64', b)), R.solve_cap(l), R.lapack_inverse('gram', m, 'f64', b))
    assert R.upper_nonzeros(w) == 0


def test_gemm_writes_nothing_outside_its_out_view(dev):
    """C: A, B and the tensor that encloses a strided out view as slices of one buffer; the bands and every entry of the enclosing tensor
    outside the view keep their bits."""
    m, n, k = R.G_EDGE
    a, b, _ = R.gemm_operands(R.G_B, m, n, k)
    big = np.random.default_rng(12).standard_normal((R.G_B, m + 7, 2 * n + 9))
    ar = Arena(dev, [a.nbytes, b.nbytes, big.nbytes])
    ta, tb, tbig = ar.put(0, a).view(a.shape), ar.put(1, b).view(b.shape), ar.put(2, big).view(big.shape)
    view = tbig[:, 3:3 + m, 5:5 + 2 * n:2]
    ops.matmul(ta, tb, out=view, alpha=-0.5, beta=2.0)
    torch.cuda.synchronize()
    ar.check('gemm 65 x 63 x 33')
    check_gemm('guarded strided out', view, a, b, -0.5, 2.0, big[:, 3:3 + m, 5:5 + 2 * n:2])
    after = tbig.cpu().numpy()
    outside = np.ones(big.shape, dtype=bool)
    outside[:, 3:3 + m, 5:5 + 2 * n:2] = False
    assert np.array_equal(after[outside].view(np.int64), big[outside].view(np.int64)), 'written outside the out view'
    assert np.array_equal(ta.cpu().numpy(), a) and np.array_equal(tb.cpu().numpy(), b)
