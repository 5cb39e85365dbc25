"""
Recipes, references and comparators of tests/test_gpu_chain_edges.py (the dense forward chain and stage A of the backward pass at every
tile count and launch form), and the CPU tests that show they can be trusted:
  (a) every (recipe, shape) the GPU file uses is well conditioned (cond K_uu, cond B <= 1e7, so cond * 2^-52 is far below the 1e-8
      tolerance) and none of the lower 16 x 16 tiles of the reference g_psi2 / w_kuu is small (>= 1e-4 of the largest entry: a wrong or
      skipped tile shows at >= 1e4 x the tolerance), and the two forms of the reference agree to a tenth of the tolerance there;
  (b) the autograd adjoints equal the closed forms of csrc/grad.hip's header evaluated with explicit inverses (two independent references);
  (c) the comparators fail on a zeroed tile, a transposed tile, a dropped jitter, a dropped Psi2 slab and a dirty padding entry.
The chain is plain fp64 arithmetic on K_uu, the Psi2 slabs and the Psi1^T y slabs, so the references take those pieces as arguments: the
GPU file passes what it reads back from the workspace, and the mixed-precision chain is held to the fp64 tolerance.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import dpgp_oracle as orc
from oracle import dpgp_oracle_torch as ot

TILE = 16
Q = 3
TERM_TOL = 1e-9             # forward terms, relative to the largest |term| of the problem (test_gpu_elbo.RTOL['f64'])
ADJ_TOL = 1e-8              # adjoints, relative to the largest entry of that output (test_gpu_grad.test_chain_adjoints)
COND_CAP = 1e7
TILE_FLOOR = 1e-4
# recipe -> (z_scale, jitter)
RECIPES = dict(dense=(2.0, 1e-8), jittered=(1.5, 1e-3), jittered_f32=(1.5, 1e-2))


def problem(n, d, m, q, seed, z_scale, jitter):
    """y [N,D], z [M,Q], mu [N,Q], s [N,Q], gamma [D,Q], alpha [D], beta [D] (jitter rides along for the caller)."""
    g = np.random.default_rng(seed)
    z = z_scale * g.standard_normal((m, q))
    mu = z_scale * g.standard_normal((n, q))
    s = g.uniform(0.1, 0.6, (n, q))
    gamma = g.uniform(0.5, 1.5, (d, q))
    alpha = g.uniform(0.7, 1.5, d)
    beta = g.uniform(0.5, 2.0, d)
    y = g.standard_normal((n, d))
    return dict(y=y, z=z, mu=mu, s=s, gamma=gamma, alpha=alpha, beta=beta, jitter=jitter)


def shape_of(m, n=None):
    """The GPU file's shapes: D = 3, N = 70 up to M = 128; D = 2, N = 150 above (few output dims: never the persistent-workgroup chain)."""
    return (70 if n is None else n, 3) if m <= 128 else (150 if n is None else n, 2)


# seeds: 1000 + M, except where that draw misses a condition of (a) below (then the first of 2000 + M, 3000 + M, ... that meets them all)
SEEDS = {('dense', 49, None): 3049, ('dense', 97, None): 3097, ('dense', 113, None): 5113, ('dense', 128, 1030): 2128,
         ('dense', 129, None): 6129, ('dense', 176, None): 2176, ('dense', 256, None): 4256, ('jittered', 113, None): 5113}


@functools.lru_cache(maxsize=None)
def case(recipe, m, n=None):
    """The problem of (recipe, M[, N]); cached and shared, never modified (the arrays are read-only)."""
    z_scale, jitter = RECIPES[recipe]
    seed = SEEDS.get((recipe, m, n), 1000 + m)
    n, d = shape_of(m, n)
    p = problem(n, d, m, Q, seed, z_scale, jitter)
    for a in p.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return p


_t = lambda a: torch.as_tensor(np.array(a, dtype=np.float64))


def chain_terms(k_uu, p2, v, alpha, beta, yy, n):
    """The five f_hat terms per output dim [D,5] of the chain on the given pieces (oracle: fhat_from_pieces)."""
    return ot.fhat_from_pieces(_t(k_uu), _t(p2), _t(v), _t(alpha).reshape(-1), _t(beta).reshape(-1), _t(yy), n).numpy()


def chain_adjoints_from_pieces(k_uu, p2, v, alpha, beta, yy, n, jitter):
    """What stage A must return for the given pieces, by autograd through fhat_from_pieces with respect to (K, P, v, alpha, beta); the
    dependence of K - jitter I, P and v on alpha (factors alpha, alpha^2, alpha) is added in closed form, as csrc/grad.hip's header has it."""
    kl, pl, vl, al, be = (_t(a).clone().requires_grad_(True) for a in (k_uu, p2, v, np.reshape(alpha, -1), np.reshape(beta, -1)))
    f = torch.sum(ot.fhat_from_pieces(kl, pl, vl, al, be, _t(yy), n))
    gk, gp, gv, da, db = torch.autograd.grad(f, [kl, pl, vl, al, be])
    sym = lambda a: 0.5 * (a + a.transpose(1, 2))
    gk, gp = sym(gk), sym(gp)
    k_scaled = kl.detach() - jitter * torch.eye(kl.shape[1], dtype=torch.float64)
    da = da + ((gk * k_scaled).sum(dim=(1, 2)) + 2.0 * (gp * pl.detach()).sum(dim=(1, 2)) + (gv * vl.detach()).sum(dim=1)) / al.detach()
    return dict(g_psi2=gp.numpy(), g_kuu=gk.numpy(), w_kuu=(gk * k_scaled).numpy(), g_v=gv.numpy(), d_alpha=da.numpy(), d_beta=db.numpy())


def closed_form_adjoints(k_uu, p2, v, alpha, beta, yy, n, jitter):
    """G_B, G_K, G_P, G_v, d/dalpha, d/dbeta of csrc/grad.hip's header, with explicit inverses (NumPy)."""
    k_uu, p2, v = (np.asarray(a, dtype=np.float64) for a in (k_uu, p2, v))
    al, be = np.reshape(alpha, -1), np.reshape(beta, -1)
    m = k_uu.shape[1]
    k_inv = np.linalg.inv(k_uu)
    b_inv = np.linalg.inv(k_uu + be[:, None, None] * p2)
    w = np.einsum('dij,dj->di', b_inv, v)
    vw = np.sum(v * w, axis=1)
    b3 = be[:, None, None]
    gb = -0.5 * b_inv - 0.5 * b3 * b3 * w[:, :, None] * w[:, None, :]
    gk = 0.5 * k_inv - 0.5 * b3 * (k_inv @ p2 @ k_inv) + gb
    gp = 0.5 * b3 * k_inv + b3 * gb
    gv = be[:, None] ** 2 * w
    wk = gk * (k_uu - jitter * np.eye(m))
    tr = np.sum(k_inv * p2, axis=(1, 2))
    d_beta = 0.5 * n / be + 0.5 * (tr - al * n) - 0.5 * np.asarray(yy) + be * vw + np.sum(gb * p2, axis=(1, 2))
    d_alpha = -0.5 * be * n + (wk.sum(axis=(1, 2)) + 2.0 * np.sum(gp * p2, axis=(1, 2)) + np.sum(gv * v, axis=1)) / al
    return dict(g_psi2=gp, g_kuu=gk, w_kuu=wk, g_v=gv, d_alpha=d_alpha, d_beta=d_beta)


def guard_bound(k_uu, p2, v, beta):
    """chain_b_kernel's conditioning guard: 2^-23 beta |K^-1|_F |Psi2|_F (1 + 1/2 beta^2 |L_B^-1 v|^2), per output dim."""
    be = np.reshape(beta, -1)
    out = np.empty(len(be))
    for d in range(len(be)):
        l_b = np.linalg.cholesky(k_uu[d] + be[d] * p2[d])
        c = np.linalg.solve(l_b, v[d])
        out[d] = 2.0 ** -23 * be[d] * np.linalg.norm(np.linalg.inv(k_uu[d])) * np.linalg.norm(p2[d]) * (1.0 + 0.5 * be[d] ** 2 * (c @ c))
    return out


def tiles_close(got, want, m, tol, what='', padding=True):
    """got [D, >= M, >= M] against want [D,M,M] over the lower triangle j <= i < M, one 16 x 16 tile at a time, each to tol x the largest
    |entry| of want's lower triangle; a failure names its output dim and tile.  padding: the entries of got's lower tiles outside
    j <= i < M (above the diagonal in a diagonal tile, rows and columns >= M up to 16 ceil(M / 16)) must be exactly 0.0.
    Returns the largest error as a fraction of the tolerance."""
    got, want = np.asarray(got), np.asarray(want)
    nb = (m + TILE - 1) // TILE
    mp = nb * TILE
    assert want.shape[1:] == (m, m) and got.shape[0] == want.shape[0]
    assert got.shape[1] >= (mp if padding else m) and got.shape[2] >= (mp if padding else m), (what, got.shape, m)
    i, j = np.meshgrid(np.arange(mp), np.arange(mp), indexing='ij')
    live = (j <= i) & (i < m)
    atol = tol * np.abs(want[:, live[:m, :m]]).max()
    worst = 0.0
    for d in range(want.shape[0]):
        for ti in range(nb):
            for tj in range(ti + 1):
                r, c = slice(TILE * ti, TILE * (ti + 1)), slice(TILE * tj, TILE * (tj + 1))
                lv = live[r, c][:min(TILE, m - TILE * ti), :min(TILE, m - TILE * tj)]
                g, w = got[d, r, c], want[d, r, c]                 # (want is cut at M by the slice; got may be)
                err = np.abs(g[:lv.shape[0], :lv.shape[1]] - w)[lv]
                e = float(err.max()) if np.isfinite(err).all() else np.inf
                assert e <= atol, '%s: output dim %d, tile (%d, %d): error %.3e > %.3e' % (what, d, ti, tj, e, atol)
                worst = max(worst, e / atol)
                if padding:
                    dead = g[~live[r, c]]
                    assert (dead == 0.0).all(), '%s: output dim %d, tile (%d, %d): %d padding entries are not 0.0 (largest %.3e)' % (
                        what, d, ti, tj, int((dead != 0.0).sum()), float(np.nanmax(np.abs(dead))))
    return worst


def terms_close(got, want, tol, what=''):
    """The f_hat terms [D,5], each to tol x the largest |term| of the problem; a failure names output dim and term.  Returns the largest
    error as a fraction of the tolerance."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    atol = tol * np.abs(want).max()
    err = np.abs(got - want)
    err[~np.isfinite(err)] = np.inf
    d, k = np.unravel_index(int(np.argmax(err)), err.shape)
    assert err[d, k] <= atol, '%s: output dim %d, term %d: %.17g against %.17g (error %.3e > %.3e)' % (
        what, d, k, got[d, k], want[d, k], err[d, k], atol)
    return float(err.max() / atol)


def vector_close(got, want, tol, what=''):
    got, want = np.asarray(got), np.asarray(want)
    atol = tol * np.abs(want).max()
    err = np.abs(got - want)
    assert np.isfinite(err).all() and err.max() <= atol, '%s: error %.3e > %.3e' % (what, float(np.nanmax(err)), atol)
    return float(err.max() / atol)


def smallest_tile(a, m):
    """The smallest max-|entry| among the lower 16 x 16 tiles of a [D,M,M] (lower triangle only), relative to the largest lower entry."""
    nb = (m + TILE - 1) // TILE
    low = np.tril(np.ones((m, m), dtype=bool))
    top = np.abs(a[:, low]).max()
    small = np.inf
    for ti in range(nb):
        for tj in range(ti + 1):
            r, c = slice(TILE * ti, min(m, TILE * (ti + 1))), slice(TILE * tj, min(m, TILE * (tj + 1)))
            small = min(small, np.abs(a[:, r, c][:, low[r, c]]).max(axis=1).min())
    return small / top


@functools.lru_cache(maxsize=None)
def oracle(recipe, m, n=None):
    """The full oracle at a case (cached, shared between the tests; never modified): ot.chain_adjoints — autograd through the oracle's own
    Psi statistics — with w_kuu, and the five terms of the NumPy oracle."""
    p = case(recipe, m, n)
    args = [np.array(p[k]) for k in ('y', 'z', 'mu', 's', 'gamma', 'alpha', 'beta')]
    ref = ot.chain_adjoints(*args, jitter=p['jitter'])
    ref['w_kuu'] = ref['g_kuu'] * (ref['k_uu'] - p['jitter'] * np.eye(m))
    ref['terms'] = oracle_terms(recipe, m, n)
    return ref


@functools.lru_cache(maxsize=None)
def oracle_terms(recipe, m, n=None):
    """The five f_hat terms per output dim of the NumPy oracle at a case (cached)."""
    p = case(recipe, m, n)
    return orc.fhat_terms(*[p[k] for k in ('y', 'z', 'mu', 's', 'gamma', 'alpha', 'beta')], jitter=p['jitter'])


def chain_terms_f32(k_uu, p2, v, alpha, beta, yy, n):
    """The chain in float32 on the CPU (LAPACK Cholesky and triangular solves on float32 copies of the pieces; the logarithms and the
    final products in fp64): what rounding every matrix entry to 24 bits costs, whatever the order of the sums."""
    import scipy.linalg as sla
    al, be = np.reshape(alpha, -1), np.reshape(beta, -1)
    out = np.empty((len(be), 5))
    for d in range(len(be)):
        k, p, vv = (np.asarray(a[d], dtype=np.float32) for a in (k_uu, p2, v))
        l_k = np.linalg.cholesky(k)
        l_b = np.linalg.cholesky(k + np.float32(be[d]) * p)
        assert l_k.dtype == np.float32 and l_b.dtype == np.float32
        x = sla.solve_triangular(l_k, p, lower=True)
        tr = np.trace(sla.solve_triangular(l_k, x.T, lower=True), dtype=np.float32)
        c = sla.solve_triangular(l_b, vv, lower=True)
        ld = np.sum(np.log(np.diag(l_b).astype(np.float64))) - np.sum(np.log(np.diag(l_k).astype(np.float64)))
        out[d] = [0.5 * n * (np.log(be[d]) - ot.LOG_2PI), -ld, 0.5 * be[d] * (float(tr) - al[d] * n), -0.5 * be[d] * yy[d],
                  0.5 * be[d] ** 2 * float(np.dot(c, c))]
    return out


# ---- the case tables of tests/test_gpu_chain_edges.py (kept here so that (a) below walks exactly what the GPU file runs) ----
TILE_COUNT_MS = [v for nb in range(1, 9) for v in (16 * nb - 15, 16 * nb - 1, 16 * nb)]     # F1 / A1: M = 1, 15, 16, 17, 31, 32, ... 128
LDS_FORM_MS = [129, 144, 176, 177, 192, 208]                  # F2: fp64 workspace — K_uu out of LDS from 129, B one per CU, B global from 177
PLAIN_MS = [17, 129, 193]                                     # F3
SLAB_MS = [33, 128, 144]                                      # F4 (N = 1030: eight splits of the observations are admissible)
SLAB_N = 1030
F32_MS = [128, 176, 177, 192, 256, 257]                       # F6: fp32 workspace — K_uu resident to 176, B two / one per CU / global
FAIL_MS = [40, 144, 192]                                      # F7
JITTER_MS = [17, 64, 113, 128]                                # A2
BIG_MS = [129, 177, 200, 256]                                 # A4
REPRO_MS = [31, 128, 256]                                     # A5
ADJOINT_CASES = sorted(set([('dense', m, None) for m in TILE_COUNT_MS + BIG_MS + REPRO_MS] + [('jittered', m, None) for m in JITTER_MS] +
                           [('dense', m, SLAB_N) for m in SLAB_MS[:2]]), key=str)
FORWARD_ONLY_CASES = sorted(set([('dense', m, None) for m in LDS_FORM_MS + PLAIN_MS + FAIL_MS] + [('dense', SLAB_MS[2], SLAB_N)] +
                                [('jittered_f32', m, None) for m in F32_MS]) - set(ADJOINT_CASES), key=str)


def reference_disagreement(recipe, m, n=None):
    """The largest difference between the autograd and the closed-form adjoints at a case, relative to the largest entry of each output."""
    p, ref = case(recipe, m, n), oracle(recipe, m, n)
    args = (ref['k_uu'], ref['psi2'], ref['v'], p['alpha'], p['beta'], np.sum(p['y'] ** 2, axis=0), p['y'].shape[0], p['jitter'])
    auto, closed = chain_adjoints_from_pieces(*args), closed_form_adjoints(*args)
    return max(float(np.abs(auto[k] - closed[k]).max() / np.abs(closed[k]).max()) for k in ('g_psi2', 'w_kuu', 'g_v', 'd_alpha', 'd_beta'))


def pieces_of(recipe, m, n):
    p = case(recipe, m, n)
    t = lambda k: _t(p[k])
    k_uu, p2, v = ot.psi_pieces(t('y'), t('z'), t('mu'), t('s'), t('gamma'), t('alpha'), jitter=p['jitter'], chunk=16)
    return p, k_uu.numpy(), p2.numpy(), v.numpy()


# --------------------------------------------------------------------------------------------------------------------
# (a) input conditions
# --------------------------------------------------------------------------------------------------------------------
def _conds(k_uu, p2, beta):
    b = k_uu + np.reshape(beta, -1)[:, None, None] * p2
    return np.linalg.cond(k_uu).max(), np.linalg.cond(b).max()


@pytest.mark.parametrize('recipe,m,n', ADJOINT_CASES, ids=lambda v: str(v))
def test_adjoint_cases_are_well_conditioned_and_have_no_small_tile(recipe, m, n):
    ref = oracle(recipe, m, n)
    ck, cb = _conds(ref['k_uu'], ref['psi2'], case(recipe, m, n)['beta'])
    tg, tw = smallest_tile(ref['g_psi2'], m), smallest_tile(ref['w_kuu'], m)
    print('%s M = %d: cond K_uu %.2e, cond B %.2e, smallest tile of g_psi2 %.2e, of w_kuu %.2e' % (recipe, m, ck, cb, tg, tw))
    assert ck <= COND_CAP and cb <= COND_CAP
    assert tg >= TILE_FLOOR and tw >= TILE_FLOOR
    # ... and the reference resolves the tolerance it judges by: its two forms (autograd through Cholesky factors, closed forms through
    # explicit inverses; both LAPACK fp64) agree to a tenth of it.  cond B <= 1e7 alone does not ensure that: the draw of seed 2256 at
    # M = 256 (cond B = 7.7e6) left them 1.4e-8 apart, each 0.7 to 1.0e-8 from the same formulas in extended precision.
    rd = reference_disagreement(recipe, m, n)
    print('    the two forms of the reference differ by %.2e of the largest entry' % rd)
    assert rd <= 0.1 * ADJ_TOL


@pytest.mark.parametrize('recipe,m,n', FORWARD_ONLY_CASES, ids=lambda v: str(v))
def test_forward_cases_are_well_conditioned(recipe, m, n):
    p, k_uu, p2, _ = pieces_of(recipe, m, n)
    ck, cb = _conds(k_uu, p2, p['beta'])
    print('%s M = %d: cond K_uu %.2e, cond B %.2e' % (recipe, m, ck, cb))
    assert ck <= COND_CAP and cb <= COND_CAP


def test_case_tables_cover_every_tile_count_and_form():
    assert TILE_COUNT_MS[:7] == [1, 15, 16, 17, 31, 32, 33] and TILE_COUNT_MS[-3:] == [113, 127, 128] and len(TILE_COUNT_MS) == 24
    assert sorted(set((m + 15) // 16 for m in TILE_COUNT_MS)) == list(range(1, 9))
    # the LDS arithmetic of csrc/linalg_dev.h / linalg.hip (tiles of 16 x 17 elements, 128 bytes of header): K_uu resident within 80 KB and
    # <= 12 tile rows; B (with its border vector) resident within 150 KB, two workgroups per compute unit within 80 KB
    tsz, ldt, hdr = 16 * 17, 17, 128
    k_res = lambda m, e: (lambda nb: nb <= 12 and hdr + e * tsz * (1 + nb * (nb + 1) // 2) <= 80 * 1024)((m + 15) // 16)
    b_bytes = lambda m, e: (lambda nb: hdr + e * (tsz * (1 + nb * (nb + 1) // 2) + nb * ldt))((m + 15) // 16)
    form = lambda m, e: 2 if b_bytes(m, e) <= 80 * 1024 else 1 if b_bytes(m, e) <= 150 * 1024 else 0
    assert [k_res(m, 8) for m in (128, 129)] == [True, False] and [k_res(m, 4) for m in (176, 177)] == [True, False]
    assert [form(m, 8) for m in [128] + LDS_FORM_MS] == [2, 1, 1, 1, 0, 0, 0]
    assert [form(m, 4) for m in F32_MS] == [2, 2, 1, 1, 1, 0]


# --------------------------------------------------------------------------------------------------------------------
# (b) reference consistency
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('recipe,m', [('dense', 17), ('dense', 128), ('jittered', 64), ('jittered', 113), ('dense', 200)])
def test_autograd_adjoints_equal_the_closed_forms(recipe, m):
    p = case(recipe, m)
    ref = oracle(recipe, m)
    n = p['y'].shape[0]
    yy = np.sum(p['y'] ** 2, axis=0)
    args = (ref['k_uu'], ref['psi2'], ref['v'], p['alpha'], p['beta'], yy, n, p['jitter'])
    auto, closed = chain_adjoints_from_pieces(*args), closed_form_adjoints(*args)
    for k in ('g_psi2', 'g_kuu', 'w_kuu', 'g_v', 'd_alpha', 'd_beta'):
        np.testing.assert_allclose(auto[k], closed[k], rtol=0, atol=1e-9 * np.abs(closed[k]).max(), err_msg=k)
    # ... and the pieces form of the reference is the oracle's own chain_adjoints (same autograd, Psi statistics passed in)
    for k in ('g_psi2', 'g_kuu', 'w_kuu', 'g_v', 'd_alpha', 'd_beta'):
        np.testing.assert_allclose(auto[k], ref[k], rtol=0, atol=1e-12 * np.abs(ref[k]).max(), err_msg=k)
    np.testing.assert_allclose(chain_terms(*args[:7]), ref['terms'], rtol=0, atol=TERM_TOL * np.abs(ref['terms']).max())
    # the guard formula against its parts written out another way
    l_b = np.linalg.cholesky(ref['k_uu'][0] + p['beta'][0] * ref['psi2'][0])
    quad = ref['v'][0] @ np.linalg.solve(l_b @ l_b.T, ref['v'][0])
    want = 2.0 ** -23 * p['beta'][0] * np.sqrt(np.sum(np.linalg.inv(ref['k_uu'][0]) ** 2) * np.sum(ref['psi2'][0] ** 2)) * (
        1.0 + 0.5 * p['beta'][0] ** 2 * quad)
    np.testing.assert_allclose(guard_bound(ref['k_uu'], ref['psi2'], ref['v'], p['beta'])[0], want, rtol=1e-9)


# --------------------------------------------------------------------------------------------------------------------
# (c) comparator sensitivity
# --------------------------------------------------------------------------------------------------------------------
def _padded(a, m):
    mp = TILE * ((m + TILE - 1) // TILE)
    out = np.zeros((a.shape[0], mp, mp))
    out[:, :m, :m] = np.tril(a)                                 # what stage A writes: the lower triangle, zeros in the rest of its tiles
    return out


def test_comparators_fail_on_each_corruption():
    m = 113                                                      # (8 tile rows, the last one a single row)
    p, ref = case('jittered', m), oracle('jittered', m)
    n, jitter = p['y'].shape[0], p['jitter']
    yy = np.sum(p['y'] ** 2, axis=0)
    nb = (m + TILE - 1) // TILE
    for name in ('g_psi2', 'w_kuu'):
        clean = _padded(ref[name], m)
        assert tiles_close(clean, ref[name], m, ADJ_TOL, name) == 0.0
        # the lower tile with the smallest entries, zeroed: the hardest one to see
        low = np.tril(np.ones((m, m), dtype=bool))
        sizes = {(ti, tj): np.abs(ref[name][:, TILE * ti:TILE * (ti + 1), TILE * tj:TILE * (tj + 1)]).max()
                 for ti in range(nb) for tj in range(ti)}
        ti, tj = min(sizes, key=sizes.get)
        r, c = slice(TILE * ti, TILE * (ti + 1)), slice(TILE * tj, TILE * (tj + 1))
        bad = clean.copy()
        bad[1, r, c] = 0.0
        with pytest.raises(AssertionError, match=r'output dim 1, tile \(%d, %d\)' % (ti, tj)):
            tiles_close(bad, ref[name], m, ADJ_TOL, name)
        bad = clean.copy()                                       # a full off-diagonal tile, transposed in place
        bad[0, 32:48, 16:32] = clean[0, 32:48, 16:32].T
        with pytest.raises(AssertionError, match=r'output dim 0, tile \(2, 1\)'):
            tiles_close(bad, ref[name], m, ADJ_TOL, name)
        for i, j in ((m, 3), (m - 1, m), (5, 9), (TILE * nb - 1, TILE * nb - 1)):     # below M, right of M, above the diagonal, the corner
            bad = clean.copy()
            bad[2, i, j] = 1e-3
            with pytest.raises(AssertionError, match='padding'):
                tiles_close(bad, ref[name], m, ADJ_TOL, name)
        bad = clean.copy()
        bad[2, m, 3] = np.nan
        with pytest.raises(AssertionError, match='padding'):
            tiles_close(bad, ref[name], m, ADJ_TOL, name)
        bad = clean.copy()
        bad[0, 40, 7] = np.nan
        with pytest.raises(AssertionError, match=r'tile \(2, 0\)'):
            tiles_close(bad, ref[name], m, ADJ_TOL, name)
        tiles_close(clean[:, :m, :m] + np.triu(clean[:, :m, :m].transpose(0, 2, 1), 1), ref[name], m, ADJ_TOL, name, padding=False)
    # jitter dropped from the diagonal of K_uu - jitter I
    bad = _padded(ref['g_kuu'] * ref['k_uu'], m)
    with pytest.raises(AssertionError, match=r'tile \(\d, \d\)'):
        tiles_close(bad, ref['w_kuu'], m, ADJ_TOL, 'w_kuu')
    # one of eight Psi2 slabs dropped (slabs of unequal weight, as the splits of the observations are)
    wts = np.arange(1.0, 9.0) / 36.0
    slabs = wts[:, None, None, None] * ref['psi2'][None]
    args = lambda p2: (ref['k_uu'], p2, ref['v'], p['alpha'], p['beta'], yy, n)
    full = chain_adjoints_from_pieces(*args(slabs.sum(axis=0)), jitter)
    assert terms_close(chain_terms(*args(slabs.sum(axis=0))), ref['terms'], TERM_TOL) <= 1.0
    assert tiles_close(_padded(full['g_psi2'], m), ref['g_psi2'], m, ADJ_TOL) <= 1.0
    for drop in (0, 7):
        short = np.delete(slabs, drop, axis=0).sum(axis=0)
        with pytest.raises(AssertionError, match='term'):
            terms_close(chain_terms(*args(short)), ref['terms'], TERM_TOL)
        lost = chain_adjoints_from_pieces(*args(short), jitter)
        for name in ('g_psi2', 'w_kuu'):
            with pytest.raises(AssertionError, match='tile'):
                tiles_close(_padded(lost[name], m), ref[name], m, ADJ_TOL, name)
        with pytest.raises(AssertionError):
            vector_close(lost['g_v'], ref['g_v'], ADJ_TOL, 'g_v')
    # a term that is NaN, and one that is off by 2e-9 of the largest
    t = ref['terms'].copy()
    t[1, 4] = np.nan
    with pytest.raises(AssertionError, match='output dim 1, term 4'):
        terms_close(t, ref['terms'], TERM_TOL)
    t = ref['terms'].copy()
    t[2, 1] += 2e-9 * np.abs(t).max()
    with pytest.raises(AssertionError, match='output dim 2, term 1'):
        terms_close(t, ref['terms'], TERM_TOL)
    assert terms_close(ref['terms'].copy(), ref['terms'], TERM_TOL) == 0.0
