"""
Recipes, figures, limits, case tables and dispatch mirror of tests/test_gpu_dense_edges.py (the four public dense operators: ops.potrf_batched,
ops.trsm_batched, ops.tril_inverse_batched, ops.matmul; csrc/linalg.hip, potrf_big.hip, potrf_persist.hip, gemm.hip, linalg_dev.h), and the
CPU tests that show they can be trusted:
  (a) the case tables reach every compiled form, loader path, tile-row count, block count, chunk shape and K-step (dispatch mirror, held
      equal to the library's own host-side workspace queries);
  (b) LAPACK's own result passes both limits at every case, and no input can fail to factor legitimately;
  (c) the comparators fail on a moved entry, a transposed tile, a zeroed tile, a dropped k-term and a non-zero above the diagonal.

Inputs.  wishart(m) = a a^T + 0.5 m I (cond ~ 10, what tests/test_gpu_kernels.py uses); gram(m) = exp(-1/2 |z_i - z_j|^2) + jitter I with
z ~ N(0, I_2): what the models factor (jitter 1e-8 in fp64: cond 5e9 .. 3e10 for M >= 127; 1e-3 in fp32: cond <= 2e5).  At that conditioning
an entrywise comparison of L says nothing, so every result is judged by its componentwise BACKWARD error, in units of the operand type's unit
roundoff u (2^-53, 2^-24), with the residual products formed in np.longdouble:
    potrf              max_{i >= j} |L L^T - A|_ij / (|L| |L|^T)_ij / u
    trsm, inverse      max |L X - B|_ij / (|L| |X|)_ij / u          (entries with a zero denominator must have residual exactly 0)
    gemm               max |C - (alpha A B + beta C0)|_ij / (|alpha| |A| |B| + |beta C0|)_ij / u
over the whole batch, one 16 x 16 tile at a time (a failure names its matrix and tile).  A figure is held to two limits:
    cap    potrf M + 4 (Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3: gamma_{M+1}; + 3 for pivots by rsq and two Newton
           steps instead of a correctly rounded root); trsm / inverse (M + 2) max_k kappa_inf(L_kk) over the 16 x 16 diagonal tiles of L
           (Thm 8.5's gamma_M, times the condition number of a diagonal tile because the kernels apply its explicit inverse); gemm k + 2
    gate   GATE x max(f_ref, 2), f_ref = the same figure of LAPACK (np.linalg.cholesky, scipy.linalg.solve_triangular; NumPy's matmul of
           the same views for gemm) on the same case in the same type.  GATE = 8 was fixed before the first GPU run and is never raised.
"""
import functools

import numpy as np
import pytest
import scipy.linalg as sla

LD = np.longdouble
TILE = 16
NP = {'f64': np.float64, 'f32': np.float32}
U = {'f64': 2.0 ** -53, 'f32': 2.0 ** -24}
ELEM = {'f64': 8, 'f32': 4}
JITTER = {'f64': 1e-8, 'f32': 1e-3}
GATE, GATE_FLOOR = 8.0, 2.0
PIVOT_MARGIN = 4.0          # smallest squared pivot >= 4 x (eps M max|A|): 8 x the (M + 1) u max|A| a computed pivot can be off by


# --------------------------------------------------------------------------------------------------------------------
# recipes (seeded, cached, read-only)
# --------------------------------------------------------------------------------------------------------------------
def _frozen(a):
    a.setflags(write=False)
    return a


def _one(recipe, m, dt, idx):
    if recipe == 'wishart':
        a = np.random.default_rng([1, m, idx]).standard_normal((m, m + 3))
        return a @ a.T + 0.5 * m * np.eye(m)
    assert recipe == 'gram'
    z = np.random.default_rng([2, m, idx]).standard_normal((m, 2))
    d = ((z[:, None, :] - z[None, :, :]) ** 2).sum(-1)
    return np.exp(-0.5 * d) + JITTER[dt] * np.eye(m)


@functools.lru_cache(maxsize=None)
def spd(recipe, m, dt, b):
    """[b,m,m] symmetric positive definite matrices of the recipe in the operand type dt ('f64' / 'f32')."""
    return _frozen(np.stack([_one(recipe, m, dt, i) for i in range(b)]).astype(NP[dt]))


@functools.lru_cache(maxsize=None)
def factor(recipe, m, dt, b):
    """LAPACK's Cholesky factors of spd(...) in the operand type: the reference of potrf, the operand of trsm and the inverse."""
    l = np.linalg.cholesky(spd(recipe, m, dt, b))
    assert l.dtype == NP[dt]
    return _frozen(l)


@functools.lru_cache(maxsize=None)
def rhs(m, k, dt, b):
    return _frozen(np.random.default_rng([3, m, k]).standard_normal((b, m, k)).astype(NP[dt]))


def eye(m, dt, b):
    return np.broadcast_to(np.eye(m, dtype=NP[dt]), (b, m, m))


def solve(l, r):
    """scipy.linalg.solve_triangular per matrix, in the operand type."""
    x = np.stack([sla.solve_triangular(l[i], r[i], lower=True) for i in range(l.shape[0])])
    assert x.dtype == l.dtype
    return x


# --------------------------------------------------------------------------------------------------------------------
# figures: [B, tile rows, tile columns] of backward errors in units of u
# --------------------------------------------------------------------------------------------------------------------
def _ratio(res, den, u):
    res, den = np.asarray(res, dtype=np.float64), np.asarray(den, dtype=np.float64)
    q = np.zeros(den.shape)
    pos = den > 0
    q[pos] = res[pos] / den[pos] / u
    q[~pos & (res != 0)] = np.inf                 # (NaN != 0: a NaN anywhere is an infinite figure)
    q[~np.isfinite(q)] = np.inf
    return q


def tile_max(q):
    b, r, c = q.shape
    rp, cp = -(-r // TILE) * TILE, -(-c // TILE) * TILE
    pad = np.zeros((b, rp, cp))
    pad[:, :r, :c] = q
    return pad.reshape(b, rp // TILE, TILE, cp // TILE, TILE).max(axis=(2, 4))


def _u(a):
    return U['f64' if a.dtype == np.float64 else 'f32']


def potrf_figure(a, l):
    """a, l [B,M,M] in the operand type; only the lower triangle of l enters (upper_nonzeros judges the rest)."""
    assert a.shape == l.shape and a.dtype == l.dtype
    lo = np.tril(l)
    ll = lo.astype(LD)
    res = np.abs(ll @ ll.transpose(0, 2, 1) - a.astype(LD))
    al = np.abs(lo.astype(np.float64))
    q = _ratio(res, al @ al.transpose(0, 2, 1), _u(a))
    return tile_max(np.tril(q))


def solve_figure(l, x, r):
    """l [B,M,M] (lower triangle), x, r [B,M,K] in the operand type: L X = R."""
    assert x.shape == r.shape and x.dtype == l.dtype
    lo = np.tril(l)
    res = np.abs(lo.astype(LD) @ x.astype(LD) - np.asarray(r).astype(LD))
    return tile_max(_ratio(res, np.abs(lo.astype(np.float64)) @ np.abs(x.astype(np.float64)), _u(l)))


def gemm_ratio(c, a, b, alpha=1.0, beta=0.0, c0=None):
    """c [batch,m,n] against alpha a b + beta c0 (a, b: any views NumPy's matmul broadcasts to c's shape; fp64): per entry, in u."""
    c = np.asarray(c)
    c = c.reshape((-1,) + c.shape[-2:])
    want = LD(alpha) * (np.asarray(a).astype(LD) @ np.asarray(b).astype(LD))
    den = abs(alpha) * (np.abs(a) @ np.abs(b))
    if beta != 0.0:
        want = want + LD(beta) * np.asarray(c0).astype(LD)
        den = den + np.abs(beta * np.asarray(c0))
    want, den = (np.broadcast_to(v, c.shape[:1] + v.shape[-2:]) if v.ndim == 2 else v for v in (want, den))
    return _ratio(np.abs(c.astype(LD) - want), den, U['f64'])


def gemm_figure(c, a, b, alpha=1.0, beta=0.0, c0=None):
    return tile_max(gemm_ratio(c, a, b, alpha, beta, c0))


def upper_nonzeros(x):
    """How many entries strictly above the diagonal of [B,M,M] are not exactly 0.0 (NaN counts)."""
    x = np.asarray(x)
    return int((np.triu(x, 1) != 0).sum())


def tile_kappa(l):
    """max over the batch and the 16 x 16 diagonal tiles of kappa_inf(L_kk)."""
    l = np.asarray(l, dtype=np.float64)
    m = l.shape[1]
    return max(float(np.linalg.cond(np.tril(l[i, k:k + TILE, k:k + TILE]), np.inf)) for i in range(l.shape[0]) for k in range(0, m, TILE))


def potrf_cap(m):
    return m + 4.0


def solve_cap(l):
    return (l.shape[1] + 2.0) * tile_kappa(l)


def gemm_cap(k):
    return k + 2.0


def judge(tiles, cap, f_ref, what, cap_only=False):
    """The figure (largest tile) against min(cap, GATE max(f_ref, GATE_FLOOR)) — cap alone for a family DESIGN.md names; returns it."""
    gate = GATE * max(f_ref, GATE_FLOOR)
    limit = cap if cap_only else min(cap, gate)
    b, ti, tj = np.unravel_index(int(np.argmax(tiles)), tiles.shape)
    worst = float(tiles[b, ti, tj])
    assert worst <= limit, '%s: matrix %d, tile (%d, %d): figure %.4g u > %.4g u (cap %.4g, LAPACK %.3g, gate %.4g)' % (
        what, b, ti, tj, worst, limit, cap, f_ref, gate)
    return worst


def report(family, what, fig, ref):
    print('dense-edges %s %s: fig=%.3g ref=%.3g ratio=%.3g' % (family, what, fig, ref, fig / max(ref, GATE_FLOOR)))


# LAPACK's own figures (cached: the reference gate of every form of a case, and test (b) below)
@functools.lru_cache(maxsize=None)
def lapack_potrf(recipe, m, dt, b):
    return float(potrf_figure(spd(recipe, m, dt, b), factor(recipe, m, dt, b)).max())


@functools.lru_cache(maxsize=None)
def lapack_trsm(recipe, m, k, dt, b):
    l, r = factor(recipe, m, dt, b), rhs(m, k, dt, b)
    return float(solve_figure(l, solve(l, r), r).max())


@functools.lru_cache(maxsize=None)
def lapack_inverse(recipe, m, dt, b):
    l, r = factor(recipe, m, dt, b), eye(m, dt, b)
    return float(solve_figure(l, solve(l, r), r).max())


# --------------------------------------------------------------------------------------------------------------------
# dispatch mirror
# --------------------------------------------------------------------------------------------------------------------
LDS_HDR, TSZ, K_LDS_MAX, PW, TRSM_KC, GM_T, GM_KC = 128, 16 * 17, 80 * 1024, 128, 64, 64, 32
V_PERSIST, V_LEFT, V_NOLA = 'DPGP_POTRF_PERSISTENT', 'DPGP_POTRF_LEFT', 'DPGP_POTRF_NO_LOOKAHEAD'
# what the GPU file sets (every other variable of the three is unset): form wanted -> environment
ENVS = {'none': {}, 'multi': {V_PERSIST: '0'}, 'nola': {V_PERSIST: '0', V_NOLA: '1'}, 'left': {V_PERSIST: '1'},
        'right': {V_PERSIST: '1', V_LEFT: '0'}}
BIG_FORMS = ('multi', 'nola', 'left', 'right')


def _up(x, q):
    return -(-x // q) * q


def k_resident(m, elem):
    """chain_k_resident of the padded size (linalg_dev.h:904-910): <= 12 tile rows and dinv + the lower tiles within 80 KB of LDS."""
    nb = _up(m, 16) // 16
    return nb <= 12 and LDS_HDR + elem * TSZ * (1 + nb * (nb + 1) // 2) <= K_LDS_MAX


def potrf_form(b, m, dt, algo='auto', env=None):
    """Which compiled form dpgp_potrf_batched_* runs (potrf_api, linalg.hip:572-604; launch_potrf_big, potrf_big.hip:236-264;
    potrf_persist_applicable, potrf_persist.hip:837; launch_potrf_persist, potrf_persist.hip:839-860):
      'resident'  potrf_batched_lds_kernel + potrf_lds        'plain'  potrf_batched_kernel + potrf_plain
      'multi'     pbig_diag / pbig_panel / pbig_update with look-ahead       'nola'  the same, diagonal blocks as launches of their own
      'left'      pleft_persistent_kernel                     'right'  pbig_persistent_kernel
    The else-branch of potrf_batched_kernel (potrf_blocked, linalg.hip:441) is NOT reachable from potrf_api: it launches that kernel only
    with plain = 1 (linalg.hip:593 returns first for every other algo), so no test of the public operator can cover it."""
    env = env or {}
    elem = ELEM[dt]
    if algo != 'plain' and k_resident(m, elem):
        return 'resident'
    if algo == 'plain':
        return 'plain'
    if elem == 8:
        pe = env.get(V_PERSIST)
        if (pe[:1] == '1') if pe is not None else (m > 128 and b >= 128):
            return 'right' if env.get(V_LEFT, '')[:1] == '0' else 'left'
    return 'nola' if env.get(V_NOLA, '')[:1] == '1' else 'multi'


def potrf_loader(m, dt):
    """The resident kernel's loader / store path (linalg.hip:461-512): 16-byte pairs for even M in fp64, scalars otherwise."""
    return 'pair' if (m % 2 == 0 and dt == 'f64') else 'scalar'


def big_blocks(m):
    """(128-wide block count, factored in place on the caller's array?) of the large-M forms (potrf_big.hip:237-238)."""
    return _up(m, PW) // PW, m % PW == 0


def _align256(x):
    return _up(x, 256)


def potrf_ws_bytes(b, m, elem):
    """dpgp_potrf_workspace_bytes (linalg.hip:558-564; potrf_big_ws_elems, potrf_big.hip:230-233)."""
    mp, mw = _up(m, 16), _up(m, PW)
    return _align256(elem * max(b * mp * mp, b * (mw * mw + PW * PW + (PW // 16) * 256 + mw * PW)))


def trsm_chunks(k):
    """(chunk count, padded chunk stride Kcp, width of the last chunk, its padded stride Kp) — trsm_api (linalg.hip:614-638) and
    trsm_batched_kernel (linalg.hip:526-527)."""
    nchunk = -(-k // TRSM_KC) if k > TRSM_KC else 1
    kcp = _up(k, 16) if nchunk == 1 else TRSM_KC
    last = k - (nchunk - 1) * TRSM_KC if nchunk > 1 else k
    return nchunk, kcp, last, _up(last, 16)


def trsm_ws_bytes(b, m, k, elem):
    """dpgp_trsm_workspace_bytes (linalg.hip:565-570)."""
    mp = _up(m, 16)
    nchunk, kcp, _, _ = trsm_chunks(k)
    return _align256(elem * b * nchunk * (mp * mp + mp * kcp + (mp // 16) * 256))


def gemm_steps(k):
    """(K-steps of 32 staged through LDS, width of the last one) — gemm_strided_f64_kernel (gemm.hip:75-90)."""
    return -(-k // GM_KC), (k - 1) % GM_KC + 1 if k else 0


# --------------------------------------------------------------------------------------------------------------------
# case tables: (recipe, M, dtype, algo, B, form wanted)
# --------------------------------------------------------------------------------------------------------------------
P1_MS = [v for nb in range(1, 9) for v in (16 * nb - 15, 16 * nb - 14, 16 * nb - 1, 16 * nb)]
P1 = [(r, m, dt, algo, 3, 'none') for m in P1_MS for dt in ('f64', 'f32') for algo in ('auto', 'plain')
      for r in (('wishart', 'gram') if m >= 17 else ('wishart',))]
P2_MS = [129, 143, 144, 145, 160, 175, 176, 177]
P2 = [('gram', m, 'f32', 'auto', 3, 'none') for m in P2_MS] + [('gram', m, 'f32', 'plain', 3, 'none') for m in (129, 177)]
BIG_MS = [129, 130, 191, 192, 193, 255, 256, 257, 383, 384, 385, 512, 640, 641]
BOTH_MS = (129, 256, 257, 384)


def _big(ms, dt, form, b=2):
    return [(r, m, dt, 'auto', b, form) for m in ms for r in (('gram', 'wishart') if m in BOTH_MS else ('gram',))]


# (512, 640 and 641 without look-ahead and 512, 640 right-looking are not in the issue's lists: one matrix each, so that every large-M form
# meets every block count from 2 to 6)
P3 = (_big(BIG_MS, 'f64', 'multi') + _big([177, 256, 257, 384, 641], 'f32', 'multi') + _big([256, 300, 384], 'f64', 'nola') +
      [('gram', m, 'f64', 'auto', 1, 'nola') for m in (512, 640, 641)])
P4 = (_big(BIG_MS, 'f64', 'left') + _big([129, 256, 300, 384, 641], 'f64', 'right') +
      [('gram', m, 'f64', 'auto', 1, 'right') for m in (512, 640)])
P4_DEFAULT = ('gram', 129, 'f64', 'auto', 128, 'none')          # the smallest shape at which the library picks the persistent form itself
POTRF_CASES = P1 + P2 + P3 + P4 + [P4_DEFAULT]


def cap_only(case):
    """The one family held to its cap alone: fp32 in the multi-workgroup routine on the well-conditioned recipe.  Measured 17 .. 23 u on
    the diagonal tiles of the last 128-block against a gate of 16 u (LAPACK 1.6 .. 1.7 u) and caps of 260 .. 388 u: a diagonal entry of the
    residual is a sum of M squares, all of one sign, that the fp32 matrix pipe adds one after the other through every block step
    (error ~ sqrt(M) u, 16 .. 20 u at M = 256 .. 384), where LAPACK's sgemm adds them in short vector lanes.  (The grams pass the gate.)"""
    recipe, m, dt, algo, b, form = case
    return recipe == 'wishart' and dt == 'f32' and potrf_form(b, m, dt, algo, ENVS[form]) == 'multi'

T_KS, T_MS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129], [1, 15, 16, 17, 127, 128, 129, 200]
T_SHAPES = sorted(set([(m, k) for m in (17, 129) for k in T_KS] + [(m, k) for m in T_MS for k in (1, 9, 65)]))
T_B = 2
I_PERSISTENT = [(m, b) for m in (128, 256, 384, 640) for b in (1, 3)]
I_FALLBACK = [(m, 2) for m in (1, 17, 127, 129, 200, 300)]


def inverse_recipes(m, b):
    """Both recipes, but the well-conditioned one only at the smaller batch of the persistent sizes (the host-side residual of three
    640 x 640 matrices is seconds)."""
    return ('gram', 'wishart') if (m % 128 or b == 1) else ('gram',)


G_KS = [0, 1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 128, 129]      # (2 is not in the issue's list: every remainder of the MFMA's k = 4)
G_MN = [(1, 129), (63, 65), (64, 64), (65, 63), (129, 1)]
G_LAYOUTS = [(ta, tb) for ta in (False, True) for tb in (False, True)]     # operand stored transposed (then i- / j-contiguous)?
G_B = 2
G_EDGE = (65, 63, 33)                                             # the shape of the view cases
G_HUGE = (65537, 2, 2, 3)


@functools.lru_cache(maxsize=None)
def gemm_operands(batch, m, n, k):
    g = np.random.default_rng([4, batch, m, n, k])
    return _frozen(g.standard_normal((batch, m, k))), _frozen(g.standard_normal((batch, k, n))), _frozen(g.standard_normal((batch, m, n)))


# --------------------------------------------------------------------------------------------------------------------
# (a) coverage
# --------------------------------------------------------------------------------------------------------------------
def _form(c):
    r, m, dt, algo, b, want = c
    return potrf_form(b, m, dt, algo, ENVS[want])


def test_potrf_tables_reach_every_form_loader_tile_row_and_block_count():
    assert P1_MS[:8] == [1, 2, 15, 16, 17, 18, 31, 32] and P1_MS[-4:] == [113, 114, 127, 128] and len(P1_MS) == 32
    for c in POTRF_CASES:                                        # the environment a case asks for gives the form it is named after
        if c[5] != 'none':
            assert _form(c) == c[5], c
    forms = {(_form(c), c[2]) for c in POTRF_CASES}
    assert forms == {('resident', 'f64'), ('resident', 'f32'), ('plain', 'f64'), ('plain', 'f32'), ('multi', 'f64'), ('multi', 'f32'),
                     ('nola', 'f64'), ('left', 'f64'), ('right', 'f64')}
    assert all(_form(c) == 'resident' for c in P1 if c[3] == 'auto') and all(_form(c) == 'plain' for c in P1 + P2 if c[3] == 'plain')
    assert _form(P4_DEFAULT) == 'left' and potrf_form(127, 129, 'f64') == 'multi' and potrf_form(128, 128, 'f64') == 'resident'
    # residency edges: fp64 to 128, fp32 to 176 (9 to 11 tile rows are fp32's alone)
    assert [k_resident(m, 8) for m in (128, 129)] == [True, False] and [k_resident(m, 4) for m in (176, 177)] == [True, False]
    assert [_form(c) for c in P2 if c[3] == 'auto'] == ['resident'] * 7 + ['multi']
    rows = {_up(c[1], 16) // 16 for c in POTRF_CASES if _form(c) == 'resident' and c[2] == 'f32'}
    assert rows == set(range(1, 12))
    assert {_up(c[1], 16) // 16 for c in POTRF_CASES if _form(c) == 'resident' and c[2] == 'f64'} == set(range(1, 9))
    # both loader paths, and the pair path at M = 2 (mod 16): its last pair of a row is the first of a tile
    res64 = [c[1] for c in POTRF_CASES if _form(c) == 'resident' and c[2] == 'f64']
    assert {potrf_loader(m, 'f64') for m in res64} == {'pair', 'scalar'} and potrf_loader(64, 'f32') == 'scalar'
    assert {m % 16 for m in res64} == {1, 2, 15, 0}
    # 2 to 6 blocks of 128, factored in place and on a padded copy, in every large-M form
    for form in BIG_FORMS:
        ms = {c[1] for c in POTRF_CASES if _form(c) == form and c[2] == 'f64'}
        assert {big_blocks(m)[0] for m in ms} >= {2, 3, 4, 5, 6}, form
        assert {big_blocks(m)[1] for m in ms} == {True, False}, form
    assert {big_blocks(c[1]) for c in P3 if c[2] == 'f32'} >= {(2, False), (2, True), (3, True), (6, False)}


def test_trsm_inverse_and_gemm_tables_reach_every_chunk_and_step():
    shapes = {trsm_chunks(k)[:1] + trsm_chunks(k)[2:3] for m, k in T_SHAPES}
    assert shapes >= {(1, 1), (1, 63), (1, 64), (2, 1), (2, 63), (2, 64), (3, 1)}
    # the last chunk's padded stride differs from the full chunks' (what a kernel that mixes them up gets wrong)
    assert [trsm_chunks(k) for k in (64, 65, 127, 129)] == [(1, 64, 64, 64), (2, 64, 1, 16), (2, 64, 63, 64), (3, 64, 1, 16)]
    assert {_up(m, 16) // 16 for m, _ in T_SHAPES} == {1, 2, 8, 9, 13}
    assert all(m % 128 == 0 for m, _ in I_PERSISTENT) and all(m % 128 for m, _ in I_FALLBACK)
    assert {m // 128 for m, _ in I_PERSISTENT} == {1, 2, 3, 5}                      # odd and even block counts
    steps = {gemm_steps(k) for k in G_KS}
    assert steps >= {(0, 0), (1, 1), (1, 31), (1, 32), (2, 1), (2, 31), (2, 32), (3, 1), (4, 32), (5, 1)}
    assert {k % 4 for k in G_KS if k} == {0, 1, 2, 3}
    assert {(-(-m // GM_T), m % GM_T) for mn in G_MN for m in mn} == {(1, 1), (1, 63), (1, 0), (2, 1), (3, 1)}
    assert G_HUGE[0] > 65535 and G_HUGE[0] % 65535 != 0                             # the bz += gridDim.z loop, with a ragged last round


def test_dispatch_mirror_equals_the_librarys_workspace_queries():
    from dp_gp_lvm_amd import _lib
    lib = _lib.lib()
    ms = sorted(set(P1_MS + P2_MS + BIG_MS + T_MS + [300]))
    for elem in (4, 8):
        for b in (1, 2, 3, 128):
            for m in ms:
                assert lib.dpgp_potrf_workspace_bytes(b, m, elem) == potrf_ws_bytes(b, m, elem), (b, m, elem)
        for m, k in T_SHAPES + [(200, 512), (33, 192), (33, 193)]:
            assert lib.dpgp_trsm_workspace_bytes(T_B, m, k, elem) == trsm_ws_bytes(T_B, m, k, elem), (m, k, elem)
    assert lib.dpgp_potrf_workspace_bytes(0, 5, 8) == 0 and lib.dpgp_trsm_workspace_bytes(1, 5, 0, 8) == 0


# --------------------------------------------------------------------------------------------------------------------
# (b) LAPACK passes both limits at every case; no input can fail legitimately
# --------------------------------------------------------------------------------------------------------------------
POTRF_INPUTS = sorted({(c[0], c[1], c[2], c[4]) for c in POTRF_CASES})


@pytest.mark.parametrize('recipe,m,dt,b', POTRF_INPUTS, ids=lambda v: str(v))
def test_lapack_cholesky_passes_both_limits_and_no_pivot_is_marginal(recipe, m, dt, b):
    a, l = spd(recipe, m, dt, b), factor(recipe, m, dt, b)
    f = lapack_potrf(recipe, m, dt, b)
    assert judge(potrf_figure(a, l), potrf_cap(m), f, 'LAPACK') == f and f <= potrf_cap(m)
    piv = float((np.diagonal(l, axis1=1, axis2=2).astype(np.float64) ** 2).min())
    margin = piv / (np.finfo(NP[dt]).eps * m * float(np.abs(a).max()))
    print('%s M = %d %s: LAPACK %.3g u (cap %g), smallest squared pivot %.3g = %.3g x eps M max|A|' % (recipe, m, dt, f, m + 4, piv, margin))
    assert margin >= PIVOT_MARGIN


@pytest.mark.parametrize('m,k', T_SHAPES)
@pytest.mark.parametrize('dt', ['f64', 'f32'])
def test_lapack_triangular_solve_passes_both_limits(m, k, dt):
    for recipe in ('gram', 'wishart'):
        l = factor(recipe, m, dt, T_B)
        f, cap = lapack_trsm(recipe, m, k, dt, T_B), solve_cap(l)
        print('%s M = %d K = %d %s: LAPACK %.3g u, cap %.4g (tile kappa %.3g)' % (recipe, m, k, dt, f, cap, tile_kappa(l)))
        assert f <= cap and f <= GATE * max(f, GATE_FLOOR)


@pytest.mark.parametrize('m,b', I_PERSISTENT + I_FALLBACK)
def test_lapack_inverse_passes_both_limits(m, b):
    for recipe in inverse_recipes(m, b):
        l = factor(recipe, m, 'f64', b)
        f, cap = lapack_inverse(recipe, m, 'f64', b), solve_cap(l)
        print('%s M = %d B = %d: LAPACK %.3g u, cap %.4g' % (recipe, m, b, f, cap))
        assert f <= cap
        assert upper_nonzeros(solve(l, eye(m, 'f64', b))) == 0


@pytest.mark.parametrize('k', G_KS)
def test_numpy_matmul_passes_both_limits(k):
    for m, n in G_MN:
        a, b, c0 = gemm_operands(G_B, m, n, k)
        f = float(gemm_figure(a @ b, a, b).max())
        f2 = float(gemm_figure(-0.5 * (a @ b) + 2.0 * c0, a, b, -0.5, 2.0, c0).max())
        print('gemm %d x %d x %d: NumPy %.3g u, with alpha, beta %.3g u (cap %g)' % (m, n, k, f, f2, k + 2))
        assert f <= gemm_cap(k) and f2 <= gemm_cap(k)


# --------------------------------------------------------------------------------------------------------------------
# (c) comparator trust
# --------------------------------------------------------------------------------------------------------------------
MOVE = {'f64': 1e-10, 'f32': 1e-4}


def _fails(tiles, cap, f_ref, match):
    with pytest.raises(AssertionError, match=match):
        judge(tiles, cap, f_ref, 'corrupted')


@pytest.mark.parametrize('dt', ['f64', 'f32'])
def test_potrf_comparator_fails_on_each_corruption(dt):
    m, b = 113, 3
    for recipe in ('wishart', 'gram'):
        a, l, f = spd(recipe, m, dt, b), factor(recipe, m, dt, b), lapack_potrf(recipe, m, dt, b)
        cap = potrf_cap(m)
        assert judge(potrf_figure(a, l), cap, f, 'clean') == f
        # one entry moved: any entry of the well-conditioned factor; of the gram factor one of the first column, where the entry is the whole
        # of its denominator (deep inside, a pivot of 1e-8 moved by 1e-10 of itself is no backward error at all, and rightly passes)
        for i, j in ((0, 0), (m - 1, 0), (40, 0)) + (((57, 22), (m - 1, m - 1)) if recipe == 'wishart' else ()):
            bad = l.copy()
            bad[1, i, j] *= NP[dt](1.0 + MOVE[dt])
            _fails(potrf_figure(a, bad), cap, f, r'matrix 1, tile \(%d, %d\)' % (i // 16, j // 16))
        bad = l.copy()
        bad[2, 32:48, 16:32] = l[2, 32:48, 16:32].T
        _fails(potrf_figure(a, bad), cap, f, 'matrix 2')
        bad = l.copy()
        bad[0, 96:112, 0:16] = 0
        _fails(potrf_figure(a, bad), cap, f, r'matrix 0, tile \(6, 0\)')
        bad = l.copy()
        bad[0, 112:, 112:] = 0                                   # the last (single-row) diagonal tile
        _fails(potrf_figure(a, bad), cap, f, r'matrix 0, tile \(7, 7\)')
        bad = l.copy()
        bad[1, 70, 3] = np.nan
        _fails(potrf_figure(a, bad), cap, f, 'matrix 1')
        assert upper_nonzeros(l) == 0
        bad = l.copy()
        bad[1, 3, 70] = 1e-30
        assert upper_nonzeros(bad) == 1
        bad[1, 5, 9] = np.nan
        assert upper_nonzeros(bad) == 2


@pytest.mark.parametrize('dt', ['f64', 'f32'])
def test_solve_comparator_fails_on_each_corruption(dt):
    m, k, b = 129, 65, T_B
    for recipe in ('wishart', 'gram'):
        l, r = factor(recipe, m, dt, b), rhs(m, k, dt, b)
        x, f, cap = solve(l, r), lapack_trsm(recipe, m, k, dt, b), solve_cap(factor(recipe, m, dt, b))
        assert judge(solve_figure(l, x, r), cap, f, 'clean') == f
        for i, j in ((0, 0), (0, 64)) + (((77, 30), (m - 1, 64)) if recipe == 'wishart' else ()):
            bad = x.copy()
            bad[1, i, j] *= NP[dt](1.0 + MOVE[dt])
            _fails(solve_figure(l, bad, r), cap, f, 'matrix 1')
        bad = x.copy()
        bad[0, 32:48, 16:32] = x[0, 32:48, 16:32].T
        _fails(solve_figure(l, bad, r), cap, f, 'matrix 0')
        bad = x.copy()
        bad[1, 128:, 64:] = 0                                    # the 1 x 1 corner tile
        _fails(solve_figure(l, bad, r), cap, f, r'matrix 1, tile \(8, 4\)')
    # the inverse: a non-zero above the diagonal is a residual over a zero denominator (the rows above it hold nothing else)
    l = factor('wishart', 100, 'f64', 1)
    w = solve(l, eye(100, 'f64', 1))
    f, cap = lapack_inverse('wishart', 100, 'f64', 1), solve_cap(l)
    assert judge(solve_figure(l, w, eye(100, 'f64', 1)), cap, f, 'clean') == f
    bad = w.copy()
    bad[0, 3, 70] = 1e-20
    assert upper_nonzeros(bad) == 1
    _fails(solve_figure(l, bad, eye(100, 'f64', 1)), cap, f, r'tile \(0, 4\)')
    bad = w.copy()
    bad[0, 48:64, 16:32] = 0
    _fails(solve_figure(l, bad, eye(100, 'f64', 1)), cap, f, r'tile \(3, 1\)')


def test_gemm_comparator_fails_on_each_corruption():
    m, n, k = G_EDGE
    a, b, c0 = gemm_operands(G_B, m, n, k)
    c = -0.5 * (a @ b) + 2.0 * c0
    f, cap = float(gemm_figure(c, a, b, -0.5, 2.0, c0).max()), gemm_cap(k)
    judge(gemm_figure(c, a, b, -0.5, 2.0, c0), cap, f, 'clean')
    i, j = np.unravel_index(int(np.argmax(np.abs(c[1]))), c[1].shape)
    bad = c.copy()
    bad[1, i, j] *= 1.0 + MOVE['f64']
    _fails(gemm_figure(bad, a, b, -0.5, 2.0, c0), cap, f, r'matrix 1, tile \(%d, %d\)' % (i // 16, j // 16))
    bad = c.copy()
    bad[0, 16:32, 32:48] = c[0, 16:32, 32:48].T
    _fails(gemm_figure(bad, a, b, -0.5, 2.0, c0), cap, f, r'matrix 0, tile \(1, 2\)')
    bad = c.copy()
    bad[1, 64:, 48:] = 0                                         # the 1 x 15 corner tile
    _fails(gemm_figure(bad, a, b, -0.5, 2.0, c0), cap, f, r'matrix 1, tile \(4, 3\)')
    for drop in (0, 31, 32):                                     # one k-term dropped: the first, the last of a K-step, the lone one of the next
        keep = [t for t in range(k) if t != drop]
        _fails(gemm_figure(-0.5 * (a[:, :, keep] @ b[:, keep, :]) + 2.0 * c0, a, b, -0.5, 2.0, c0), cap, f, 'matrix')
    _fails(gemm_figure(-0.5 * (a @ b), a, b, -0.5, 2.0, c0), cap, f, 'matrix')          # beta C0 dropped
    # k = 0: the denominator is |beta C0| alone, or zero — then anything but an exact 0 fails
    a0, b0 = a[:, :, :0], b[:, :0, :]
    assert gemm_figure(np.zeros_like(c0), a0, b0).max() == 0.0 and gemm_figure(2.0 * c0, a0, b0, 1.0, 2.0, c0).max() == 0.0
    bad = np.zeros_like(c0)
    bad[0, 5, 5] = 1e-300
    _fails(gemm_figure(bad, a0, b0), gemm_cap(0), 0.0, r'matrix 0, tile \(0, 0\)')
