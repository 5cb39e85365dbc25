"""
Recipes, references, plan mirror and comparators of tests/test_gpu_qx_psi_edges.py (the q(X) Psi operators of csrc/qx_psi.hip at every
tile, chunk, slab and LDS edge), and the CPU tests that show they can be trusted:
  (a) the fp64 torch-autograd references (the restatements of test_gpu_qx_psi_grouped.py, test_gpu_predict_masked.py and
      test_gpu_train_masked.py, imported) agree with a 40-digit mpmath evaluation of all seven outputs to 1e-14 of each output's largest
      entry: two decades of margin under the operators' 1e-12;
  (b) a Python mirror of the host plans (qp_/qg_ stats, adjoint and parameter-adjoint plans, the LDS formulas, the KQ / PC dispatch, and
      the two overrides DPGP_QP_N_SLABS / DPGP_QP_PAIR_SLABS) gives the library's workspace size for every case of every family under
      every override the family uses: the library took the override, and the mirror may be used to reason about coverage;
  (c) the case lists together reach every register-width instantiation, every (PC, NW) switch of the grouped adjoint's LDS budget, the
      48 KiB dynamic-LDS attribute boundary of each kernel, and the slab shapes that the natural plans never produce at test sizes;
  (d) with both overrides unset the workspace queries return what they returned before the overrides existed (three recorded shapes).
The families (E1 .. E7) are described where their case lists are built.
"""
import collections
import functools
import zlib

import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import _lib
from test_gpu_predict_masked import restated as restated_latent
from test_gpu_qx_psi_grouped import restated as restated_grouped
from test_gpu_train_masked import restated_param

TOL = 1e-12                  # the operators' tolerance (test_gpu_predict_b1.close: rtol, and atol relative to the largest entry)
REF_TOL = 1e-14              # what the autograd references are held to against mpmath
N_KNOB, PAIR_KNOB = 'DPGP_QP_N_SLABS', 'DPGP_QP_PAIR_SLABS'
OUTPUTS = ('psi1', 'psi2', 'd_mu', 'd_s', 'd_z', 'd_gamma', 'd_alpha')
ALL_OPS = ('stats', 'adjoint', 'param')
OUTPUTS_OF = dict(stats=('psi1', 'psi2'), adjoint=('d_mu', 'd_s'), param=('d_z', 'd_gamma', 'd_alpha'))

# form: 'plain' (B kernels, no weights), 'weighted' (B kernels, wt [B,N]) or 'grouped' (K = b kernels x p weight rows [P,N]);
# wkind: how the weights are drawn (weights_of); recipe: how the inputs are drawn (inputs); gmode: 'both', 'g1' (g2 = 0) or 'g2' (g1 = 0)
Case = collections.namedtuple('Case', 'family form wkind b p m n q recipe gmode')


def mk(family, form, wkind, b, p, m, n, q, recipe='std', gmode='both'):
    return Case(family, form, wkind if form != 'plain' else 'none', b, p if form == 'grouped' else 1, m, n, q, recipe, gmode)


def case_id(c):
    tail = ('' if c.recipe == 'std' else '-' + c.recipe) + ('' if c.gmode == 'both' else '-' + c.gmode)
    shape = ('K%dP%d' % (c.b, c.p)) if c.form == 'grouped' else 'B%d' % c.b
    return '%s-%s-%s-%s-M%d-N%d-Q%d%s' % (c.family, c.form, c.wkind, shape, c.m, c.n, c.q, tail)


# ------------------------------------------------------------------------------------------------------------------------ the families
FORMS = (('plain', 'none'), ('weighted', 'binary'), ('weighted', 'real'), ('grouped', 'mixed'))
UNSET = ()


def _forms(family, b, p, m, n, q, **kw):
    return [mk(family, form, wkind, b, p, m, n, q, **kw) for form, wkind in FORMS]


# E1: M at the 32-tile edges (rows and columns past M in the last tile add nothing; a multiple of 32 has no empty tile)
E1 = [c for m in (31, 32, 33, 63, 64, 65, 96, 97) for c in _forms('E1', 2, 3, m, 33, 3)]
# E2: N at the staging (32) and wave (64) edges; stats and the parameter adjoint under DPGP_QP_N_SLABS unset / 1 / 2 / 3.  For the grouped
# adjoint N = 64 / 65 and 128 / 129 switch NW; at N = 129 the fourth wave is past N and the third has one live lane
E2 = [c for n in (31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129) for c in _forms('E2', 2, 3, 33, n, 5)]
E2_ENVS = [UNSET] + [((N_KNOB, str(v)),) for v in (1, 2, 3)]
# E3: every register width: KQ of the adjoint (1, 2, 4, 8; the chunk-is-everything path up to Q = 8; a last chunk of one dim at 9 and 17),
# KQ of the parameter adjoint (1, 2, 4; a last chunk of one dim at 5, 9, 17), each with PC = 1, 2, 4, 8 (P = 1, 2, 4, 5)
E3_Q = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17)
E3 = [mk('E3', form, wkind, 3, 1, 40, 70, q) for q in E3_Q for form, wkind in FORMS[:3]] + \
     [mk('E3', 'grouped', 'mixed', 2, p, 40, 70, q) for q in E3_Q for p in (1, 2, 4, 5)]
# E4: the pair-slab loop of the adjoint under DPGP_QP_PAIR_SLABS: several tiles per workgroup, slabs that cross a block row of the
# triangle, and the Psi1 term exactly once (g1 alone and g2 alone under every split).  M = 130: 15 tiles, T = 5; M = 97: 10 tiles
E4_FORMS = [('plain', 'none', 'both'), ('plain', 'none', 'g1'), ('plain', 'none', 'g2'), ('weighted', 'binary', 'both'),
            ('weighted', 'real', 'both'), ('weighted', 'real', 'g1'), ('weighted', 'real', 'g2'), ('grouped', 'mixed', 'both'),
            ('grouped', 'mixed', 'g1'), ('grouped', 'mixed', 'g2')]
E4 = [mk('E4', form, wkind, 1 if m == 130 or form == 'grouped' else 2, 3, m, 65, 10, gmode=gmode)
      for m in (130, 97) for form, wkind, gmode in E4_FORMS]


def e4_envs(c):
    tiles = qp_tiles(c.m)
    return [UNSET] + [((PAIR_KNOB, str(v)),) for v in (1, 2, 4, 6, tiles)]


# E5: the LDS switch points.  Grouped adjoint, M = 33: NW 4 -> 2 at Q = 14 / 15 and 2 -> 1 at 26 / 27 (PC = 8), PC 8 -> 4 at 46 / 47 and
# 4 -> 2 at 63 / 64; at each Q also P = PC and PC + 1 of the width the plan picks.  The 48 KiB attribute boundary: 19 / 20 (adjoint and
# parameter adjoint, Psi2 term), 24 / 25 (parameter adjoint, Psi1 term), 47 / 48 (stats); Q = 64 for the three plain operators
E5_SWITCHES = [((14, 15), 5, 257, ((8, 4), (8, 2))), ((26, 27), 5, 129, ((8, 2), (8, 1))), ((46, 47), 5, 70, ((8, 1), (4, 1))),
               ((63, 64), 3, 70, ((4, 1), (2, 1)))]          # (Q pair), P, N, the (PC, NW) on either side


def _e5_grouped():
    out = []
    for qs, p, n, _ in E5_SWITCHES:
        for q in qs:
            pc = qg_adj_plan(1, p, n, 33, q, {})['pc']
            for pp in sorted({p, pc, pc + 1}):
                out.append(mk('E5', 'grouped', 'mixed', 1, pp, 33, n, q))
    return out


E5_PLAIN_Q = (19, 20, 24, 25, 47, 48, 64)
E6_N, E6_M, E6_Q = 256, 65, 10
# E7: range.  shift50: z and mu moved by +50 in every latent dim (tolerance x 51: see tol_of); s0: s = 0 exactly in a third of the rows;
# gs1e4: gamma s up to 1e4; far: a third of the points 40 units from every inducing input in every dim (every exponential underflows)
E7 = [c for recipe in ('shift50', 's0', 'gs1e4', 'far') for c in _forms('E7', 2, 3, 33, 65, 10, recipe=recipe)]


def tol_of(c):
    """shift50: inputs near 50 carry rounding 50 times larger relative to the unit-size differences mu - z the operators depend on, and
    the results are linear in that to first order: 1e-12 (1 + 50).  Everything else: 1e-12."""
    return TOL * 51.0 if c.recipe == 'shift50' else TOL


# --------------------------------------------------------------------------------------------------------------------- the plan mirror
QP_TILE, QP_HSTRIDE, QP_NT, QP_SN, QP_QCHUNK, QP_PCHUNK, QP_TARGET_WGS = 32, 33, 64, 32, 8, 4, 1024
QG_LDS_BUDGET, LDS_ATTR = 160 * 1024, 48 * 1024


def cdiv(a, b):
    return (a + b - 1) // b


def qp_tiles(m):
    t = cdiv(m, QP_TILE)
    return t * (t + 1) // 2


def forced(env, name, hi):
    """dpgp_env_plan(name, 1, hi) of csrc/internal.h: 0 when unset or below 1 (the natural value stands), else the value clamped to hi."""
    if name not in env:
        return 0
    v = int(env[name])
    return 0 if v < 1 else min(v, hi)


def _clamp(v, hi):
    return 1 if v < 1 else min(v, hi)


def qp_stats_plan(b, n, m, env):
    tiles, chunks = qp_tiles(m), cdiv(n, QP_SN)
    sl = forced(env, N_KNOB, chunks) or cdiv(QP_TARGET_WGS // 2, tiles * b)
    n_per_slab = cdiv(chunks, _clamp(sl, chunks)) * QP_SN
    return dict(T=cdiv(m, QP_TILE), tiles=tiles, n_per_slab=n_per_slab, slabs=cdiv(n, n_per_slab))


def _pair_slabs(base, tiles, env):
    sl = forced(env, PAIR_KNOB, tiles) or cdiv(QP_TARGET_WGS, base)
    tiles_per_slab = cdiv(tiles, _clamp(sl, tiles))
    return dict(tiles_per_slab=tiles_per_slab, slabs=cdiv(tiles, tiles_per_slab))


def qp_adj_plan(b, n, m, q, env):
    p = dict(T=cdiv(m, QP_TILE), tiles=qp_tiles(m), nt=cdiv(n, QP_NT), qchunks=cdiv(q, QP_QCHUNK))
    p.update(_pair_slabs(p['nt'] * b * p['qchunks'], p['tiles'], env))
    return p


def qp_param_plan(b, n, m, q, env):
    p = dict(T=cdiv(m, QP_TILE), tiles=qp_tiles(m), qchunks=cdiv(q, QP_PCHUNK))
    chunks = cdiv(n, QP_SN)
    f = forced(env, N_KNOB, chunks)
    sl = f or cdiv(QP_TARGET_WGS // 2, p['tiles'] * b * p['qchunks'])
    p['n_per_slab'] = cdiv(chunks, _clamp(sl, chunks)) * QP_SN
    p['slabs'] = cdiv(n, p['n_per_slab'])
    sl = f or cdiv(QP_TARGET_WGS // 2, p['T'] * b)
    p['n_per_slab1'] = cdiv(chunks, _clamp(sl, chunks)) * QP_SN
    p['slabs1'] = cdiv(n, p['n_per_slab1'])
    return p


def qg_pow2_width(p):
    return 8 if p >= 5 else 4 if p >= 3 else 2 if p >= 2 else 1


def qp_stats_lds(q):
    return 8 * (2 * QP_SN * q + QP_SN + 2 * QP_TILE * q + q)


def qp_adj_lds(q):
    return 8 * (3 * q * QP_NT + 2 * QP_TILE * q + QP_TILE * QP_HSTRIDE + q)


def qp_param_lds(q):
    return 8 * (4 * QP_SN * q + QP_SN + 2 * QP_TILE * (q | 1) + q + 2 * QP_TILE * QP_HSTRIDE + 256)


def qp_param_psi1_lds(q):
    return 8 * (3 * QP_SN * q + QP_SN + QP_TILE * (q | 1) + q + QP_SN * QP_HSTRIDE + 2 * QP_TILE * q + 256)


def qg_adj_lds(q, pc, nw):
    return 8 * (3 * q * QP_NT * nw + 2 * QP_TILE * q + pc * QP_TILE * QP_HSTRIDE + q)


def qg_stats_plan(k, p, n, m, env):
    pc = qg_pow2_width(p)
    out = dict(pc=pc, pchunks=cdiv(p, pc))
    out.update(qp_stats_plan(k * out['pchunks'], n, m, env))
    return out


def qg_adj_plan(k, p, n, m, q, env):
    pc = qg_pow2_width(p)
    while pc > 1 and qg_adj_lds(q, pc, 1) > QG_LDS_BUDGET:
        pc //= 2
    nw = 4 if n > 2 * QP_NT else 2 if n > QP_NT else 1
    while nw > 1 and qg_adj_lds(q, pc, nw) > QG_LDS_BUDGET:
        nw //= 2
    out = dict(pc=pc, pchunks=cdiv(p, pc), nw=nw, T=cdiv(m, QP_TILE), tiles=qp_tiles(m), nt=cdiv(n, QP_NT * nw), qchunks=cdiv(q, QP_QCHUNK))
    out.update(_pair_slabs(out['nt'] * k * out['qchunks'] * out['pchunks'], out['tiles'], env))
    return out


def qg_param_plan(k, p, n, m, q, env):
    pc = qg_pow2_width(p)
    out = dict(pc=pc, pchunks=cdiv(p, pc))
    out.update(qp_param_plan(k * out['pchunks'], n, m, q, env))
    k1 = qp_param_plan(k, n, m, q, env)                          # (the Psi1 term: once per kernel)
    out.update(slabs1=k1['slabs1'], n_per_slab1=k1['n_per_slab1'])
    return out


def adjoint_kq(q):
    w = min(q, QP_QCHUNK)
    return 1 if w <= 1 else 2 if w <= 2 else 4 if w <= 4 else 8


def param_kq(q):
    return 1 if q <= 1 else 2 if q <= 2 else QP_PCHUNK


def plan_of(op, c, env):
    env = dict(env)
    if c.form == 'grouped':
        return dict(stats=lambda: qg_stats_plan(c.b, c.p, c.n, c.m, env), adjoint=lambda: qg_adj_plan(c.b, c.p, c.n, c.m, c.q, env),
                    param=lambda: qg_param_plan(c.b, c.p, c.n, c.m, c.q, env))[op]()
    return dict(stats=lambda: qp_stats_plan(c.b, c.n, c.m, env), adjoint=lambda: qp_adj_plan(c.b, c.n, c.m, c.q, env),
                param=lambda: qp_param_plan(c.b, c.n, c.m, c.q, env))[op]()


def workspace_bytes(op, c, env):
    """The mirror's dpgp_qx_psi_{stats,adjoint,param_adjoint}[_grouped]_workspace_bytes."""
    p = plan_of(op, c, env)
    slots = c.b * (c.p if c.form == 'grouped' else 1)             # Psi2 slots of the stats workspace
    cols = c.b * p.get('pchunks', 1)                              # workgroup columns of the two adjoints
    if op == 'stats':
        return 8 * p['slabs'] * slots * c.m * c.m
    if op == 'adjoint':
        return 8 * p['slabs'] * cols * 2 * c.q * c.n
    cell, cell1 = 2 * QP_TILE * c.q + c.q + 1, QP_TILE * c.q + c.q + 1
    return 8 * (p['slabs'] * cols * p['tiles'] * cell + p['slabs1'] * c.b * p['T'] * cell1)


def library_workspace_bytes(op, c):
    stem = dict(stats='dpgp_qx_psi_stats', adjoint='dpgp_qx_psi_adjoint', param='dpgp_qx_psi_param_adjoint')[op]
    if c.form == 'grouped':
        return getattr(_lib.lib(), stem + '_grouped_workspace_bytes')(c.b, c.p, c.n, c.m, c.q)
    return getattr(_lib.lib(), stem + '_workspace_bytes')(c.b, c.n, c.m, c.q)


def lds_of(op, c, env=UNSET):
    """{kernel: dynamic LDS bytes} of the launches of (op, case)."""
    if c.form == 'grouped':
        if op == 'stats':
            return {'qg_psi2': qp_stats_lds(c.q) + 8 * QP_SN * qg_pow2_width(c.p)}
        if op == 'adjoint':
            p = plan_of(op, c, env)
            return {'qg_adjoint': qg_adj_lds(c.q, p['pc'], p['nw'])}
        return {'qg_param': qp_param_lds(c.q) + 8 * QP_SN * qg_pow2_width(c.p), 'qp_param_psi1': qp_param_psi1_lds(c.q)}
    if op == 'stats':
        return {'qp_psi2': qp_stats_lds(c.q)}
    if op == 'adjoint':
        return {'qp_adjoint': qp_adj_lds(c.q)}
    return {'qp_param': qp_param_lds(c.q), 'qp_param_psi1': qp_param_psi1_lds(c.q)}


# ------------------------------------------------------------------------------------------------------------- inputs and references
def _seed(c):
    return zlib.crc32(repr(tuple(c._replace(gmode='both'))).encode())      # (the g1-alone / g2-alone variants share the case's draw)


def weights_of(c, rs):
    """None (plain), [B,N] (weighted) or [P,N] (grouped).  binary: 0 / 1 with about 40 % zeros; real: any reals; mixed: even rows binary,
    odd rows real; the E6 kinds switch whole waves, staged steps, n slabs or pattern chunks off."""
    if c.form == 'plain':
        return None
    rows = c.b if c.form == 'weighted' else c.p
    binary, real = (rs.random((rows, c.n)) >= 0.4).astype(np.float64), rs.standard_normal((rows, c.n))
    kind = c.wkind
    if kind == 'binary':
        return binary
    w = real.copy()
    if kind == 'mixed' or kind.endswith('_mixed'):
        w[0::2] = binary[0::2]
    off = dict(wave1=(64, 128), step1=(32, 64), slab1=(96, 192), all=(0, c.n)).get(kind.split('_')[0])
    if off:
        w[:, off[0]:off[1]] = 0.0
    if kind == 'chunk0_off':                                      # (P = 9, PC = 8: patterns 0 .. 7 are chunk 0, which owns the Psi1 term)
        w[:8] = 0.0
    if kind == 'chunk1_off':
        w[8:] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def inputs(c):
    """The case's arrays as fp64 CPU tensors: z [B,M,Q], mu, s [N,Q], gamma [B,Q], alpha [B], g1 [B,N,M], g2 [B,M,M] or [K,P,M,M], w (or
    None).  Cached and shared: never modified."""
    rs = np.random.default_rng(_seed(c))
    b, m, n, q = c.b, c.m, c.n, c.q
    z, mu = rs.standard_normal((b, m, q)), rs.standard_normal((n, q))
    s = rs.uniform(0.1, 1.5, (n, q))
    gamma, alpha = rs.uniform(0.2, 2.0, (b, q)), rs.uniform(0.5, 2.0, b)
    g1 = rs.standard_normal((b, n, m))
    g2 = rs.standard_normal((b, c.p, m, m) if c.form == 'grouped' else (b, m, m))      # (not symmetric)
    w = weights_of(c, rs)
    if c.recipe == 'shift50':
        z, mu = z + 50.0, mu + 50.0
    elif c.recipe == 's0':
        s[0::3] = 0.0
    elif c.recipe == 'gs1e4':
        s = s * 10.0 ** rs.uniform(-2.0, 4.0, (n, 1))
        s *= 1e4 / (gamma.max(axis=0) * s).max()                  # (the largest gamma s is 1e4)
    elif c.recipe == 'far':
        mu[0::3] += 40.0
    else:
        assert c.recipe == 'std', c.recipe
    if c.gmode == 'g1':
        g2 = np.zeros_like(g2)
    elif c.gmode == 'g2':
        g1 = np.zeros_like(g1)
    out = dict(z=z, mu=mu, s=s, gamma=gamma, alpha=alpha, g1=g1, g2=g2, w=w)
    return {k: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64) for k, a in out.items()}


@functools.lru_cache(maxsize=None)
def _reference(c, half):
    t = inputs(c)
    if c.form == 'grouped':
        r = restated_grouped(t)
        return {k: r[k].detach().numpy() for k in OUTPUTS}
    w = torch.ones((c.b, c.n), dtype=torch.float64) if t['w'] is None else t['w']
    args = (t['z'], t['mu'], t['s'], t['gamma'], t['alpha'], t['g1'], t['g2'], w)
    if half == 'latent':
        return {k: a.detach().numpy() for k, a in zip(('psi1', 'psi2', 'd_mu', 'd_s'), restated_latent(*args))}
    return {k: a.detach().numpy() for k, a in zip(('d_z', 'd_gamma', 'd_alpha'), restated_param(*args))}


def reference(c, outputs=OUTPUTS):
    """{output: fp64 array} of the case by torch autograd of the plain restatements, cached per case (the slot forms in two halves, so
    that a family that runs one operator pays for one)."""
    out = {}
    for name in outputs:
        half = 'all' if c.form == 'grouped' else ('latent' if name in ('psi1', 'psi2', 'd_mu', 'd_s') else 'param')
        out[name] = _reference(c, half)[name]
    return out


# ------------------------------------------------------------------------------------------------------------------------ comparators
def close_frac(have, want, tol, what=''):
    """test_gpu_predict_b1.close at tol, returning the largest error as a fraction of the bound."""
    have, want = np.asarray(have, dtype=np.float64).reshape(np.shape(want)), np.asarray(want, dtype=np.float64)
    bound = tol * max(1.0, np.abs(want).max()) + tol * np.abs(want)
    err = np.abs(have - want)
    assert np.isfinite(have).all(), what + ': not finite'
    frac = float((err / bound).max()) if err.size else 0.0
    assert frac <= 1.0, '%s: largest error %.3e of the bound at index %s (have %r, want %r)' % (
        what, frac, np.unravel_index(np.argmax(err / bound), err.shape), have.flat[np.argmax(err / bound)], want.flat[np.argmax(err / bound)])
    return frac


def tiles_close_frac(have, want, tol, what='', axes=(-2, -1)):
    """close_frac one 32-block at a time along the given axes (psi2: 32 x 32 tiles; d_z: blocks of 32 rows), the bound of the whole
    array: a failure names its tile."""
    have, want = np.asarray(have, dtype=np.float64).reshape(np.shape(want)), np.asarray(want, dtype=np.float64)
    assert np.isfinite(have).all(), what + ': not finite'
    bound = tol * max(1.0, np.abs(want).max()) + tol * np.abs(want)
    ratio = np.abs(have - want) / bound
    worst = 0.0
    blocks = [range(0, want.shape[a], QP_TILE) for a in axes]
    for origin in np.array(np.meshgrid(*blocks, indexing='ij')).reshape(len(axes), -1).T:
        sl = [slice(None)] * want.ndim
        for a, o in zip(axes, origin):
            sl[a] = slice(int(o), int(o) + QP_TILE)
        frac = float(ratio[tuple(sl)].max())
        assert frac <= 1.0, '%s: tile %s: largest error %.3e of the bound' % (what, tuple(int(o) // QP_TILE for o in origin), frac)
        worst = max(worst, frac)
    return worst


def compare(name, have, want, tol, what=''):
    if name == 'psi2':
        return tiles_close_frac(have, want, tol, what + ' psi2')
    if name == 'd_z':
        return tiles_close_frac(have, want, tol, what + ' d_z', axes=(-2,))
    return close_frac(have, want, tol, what + ' ' + name)


# ----------------------------------------------------------------------------------------------------- what the GPU file runs, per family
def e6_cases():
    """(case, operators): idle and dead waves of the (mu, S) adjoints; a skipped staged step and a skipped n slab of stats / parameter
    adjoint (the latter under DPGP_QP_N_SLABS = 3: slabs of 96 points, the second one all zero weights)."""
    n, m, q = E6_N, E6_M, E6_Q
    out = collections.OrderedDict()

    def add(c, ops):
        out[c] = tuple(op for op in ALL_OPS if op in ops or op in out.get(c, ()))

    for gmode in ('both', 'g1', 'g2'):
        for kind in ('wave1_mixed', 'all_off'):
            add(mk('E6', 'grouped', kind, 1, 5, m, n, q, gmode=gmode), ('adjoint',))
        for kind in ('wave1_real', 'all_off'):
            add(mk('E6', 'weighted', kind, 1, 1, m, n, q, gmode=gmode), ('adjoint',))
    for kind in ('chunk0_off', 'chunk1_off'):
        add(mk('E6', 'grouped', kind, 1, 9, m, n, q), ALL_OPS)
    for form, p in (('weighted', 1), ('grouped', 5)):
        for kind in ('step1_mixed', 'slab1_mixed', 'all_off'):
            add(mk('E6', form, kind, 1, p, m, n, q), ('stats', 'param'))
        add(mk('E6', form, 'all_off', 1, p, m, n, q, gmode='g2'), ('param',))
    return list(out.items())


E6 = e6_cases()
E6_CASES = [c for c, _ in E6]
E5 = _e5_grouped() + [mk('E5', form, wkind, 2, 1, 33, 70, q) for q in E5_PLAIN_Q for form, wkind in FORMS[:3]]


def runs_of(c):
    """[(operator, env)] the GPU file runs for the case; env: a tuple of (name, value), () for the natural plan."""
    if c.family == 'E2':
        return [(op, env) for op in ('stats', 'param') for env in E2_ENVS] + [('adjoint', UNSET)]
    if c.family == 'E4':
        return [('adjoint', env) for env in e4_envs(c)]
    if c.family == 'E6':
        ops = dict(E6)[c]
        envs = [UNSET, ((N_KNOB, '3'),)] if 'stats' in ops else [UNSET]
        return [(op, env) for op in ops for env in (envs if op != 'adjoint' else [UNSET])]
    return [(op, UNSET) for op in ALL_OPS]


FAMILIES = dict(E1=E1, E2=E2, E3=E3, E4=E4, E5=E5, E6=E6_CASES, E7=E7)
ALL_CASES = [c for fam in FAMILIES.values() for c in fam]
ALL_RUNS = [(c, op, env) for c in ALL_CASES for op, env in runs_of(c)]


def set_env(monkeypatch, env):
    for name in (N_KNOB, PAIR_KNOB):
        monkeypatch.delenv(name, raising=False)
    for name, value in env:
        monkeypatch.setenv(name, value)


# ============================================================================================================================ CPU tests
def test_case_lists_are_sound():
    assert len(set(ALL_CASES)) == len(ALL_CASES), 'a case is listed twice'
    for c in ALL_CASES:
        size = c.b * c.n * c.m * c.m * c.q
        assert size <= 2.3e7, (case_id(c), size)                 # (about 2e7: the reference takes about a second)
        assert 1 <= c.q <= 64
    # E6's slab-off kind is one whole slab of DPGP_QP_N_SLABS = 3
    for op in ('stats', 'param'):
        for c in (x for x in E6_CASES if x.wkind.startswith('slab1')):
            p = plan_of(op, c, ((N_KNOB, '3'),))
            assert (p['n_per_slab'], p['slabs']) == (96, 3) and (op == 'stats' or (p['n_per_slab1'], p['slabs1']) == (96, 3))
            assert not inputs(c)['w'][:, 96:192].any() and inputs(c)['w'][:, :96].any() and inputs(c)['w'][:, 192:].any()


def test_mirror_equals_the_library_workspace_queries(monkeypatch):
    """For every (case, operator, override) the GPU file runs: the library's workspace query, with the override in the environment,
    equals the mirror's.  The queries are host code and read the overrides where the launches do."""
    seen = set()
    for c, op, env in ALL_RUNS:
        key = (op, c.form, c.b, c.p, c.m, c.n, c.q, env)
        if key in seen:
            continue
        seen.add(key)
        set_env(monkeypatch, env)
        assert library_workspace_bytes(op, c) == workspace_bytes(op, c, env), (case_id(c), op, env)
    # the overrides change something, are clamped as the natural value is, and values below 1 leave the natural plan
    c = mk('E2', 'plain', 'none', 2, 1, 33, 97, 5)
    natural = {op: workspace_bytes(op, c, UNSET) for op in ALL_OPS}
    for value, slabs in (('1', 1), ('2', 2), ('1000', 4), ('0', None), ('-3', None), ('x', None)):
        env = ((N_KNOB, value),)
        set_env(monkeypatch, env)
        for op in ('stats', 'param'):
            have = library_workspace_bytes(op, c)
            if slabs is None:
                assert have == natural[op], (op, value)
            else:
                assert have == workspace_bytes(op, c, (((N_KNOB, str(slabs))),)), (op, value)
        assert library_workspace_bytes('adjoint', c) == natural['adjoint']
    c = mk('E4', 'plain', 'none', 1, 1, 130, 65, 10)
    for value, slabs in (('1', 1), ('4', 4), ('99', 15), ('0', 15), ('-1', 15)):            # (the natural plan: one tile per slab)
        set_env(monkeypatch, ((PAIR_KNOB, value),))
        assert library_workspace_bytes('adjoint', c) == 8 * slabs * 2 * 10 * 65, value
        assert library_workspace_bytes('stats', c) == workspace_bytes('stats', c, UNSET)


def test_unset_overrides_leave_the_recorded_workspace_sizes(monkeypatch):
    """Three shapes recorded before the overrides existed: (B or (K, P), N, M, Q) -> stats, adjoint, parameter adjoint."""
    set_env(monkeypatch, UNSET)
    lib = _lib.lib()
    for (b, n, m, q), want in PARENT_PLAIN.items():
        have = (lib.dpgp_qx_psi_stats_workspace_bytes(b, n, m, q), lib.dpgp_qx_psi_adjoint_workspace_bytes(b, n, m, q),
                lib.dpgp_qx_psi_param_adjoint_workspace_bytes(b, n, m, q))
        assert have == want, (b, n, m, q)
    for (k, p, n, m, q), want in PARENT_GROUPED.items():
        have = (lib.dpgp_qx_psi_stats_grouped_workspace_bytes(k, p, n, m, q), lib.dpgp_qx_psi_adjoint_grouped_workspace_bytes(k, p, n, m, q),
                lib.dpgp_qx_psi_param_adjoint_grouped_workspace_bytes(k, p, n, m, q))
        assert have == want, (k, p, n, m, q)


PARENT_PLAIN = {(5, 2000, 100, 10): (4400000, 6400000, 2153760), (2, 97, 33, 5): (69696, 46560, 83840),
                (1, 65, 130, 10): (405600, 156000, 274080)}
PARENT_GROUPED = {(3, 5, 300, 200, 23): (24000000, 9273600, 3287424), (1, 9, 256, 65, 10): (2433600, 491520, 563520),
                  (2, 3, 129, 33, 27): (261360, 334368, 564160)}


def _facts():
    """What the mirror says each (case, operator, override) of the GPU file runs."""
    facts = []
    for c, op, env in ALL_RUNS:
        p = plan_of(op, c, env)
        f = dict(case=c, op=op, env=env, plan=p, lds=lds_of(op, c, env), weighted=c.form == 'weighted', grouped=c.form == 'grouped')
        if op == 'adjoint':
            f['kq'] = adjoint_kq(c.q)
            f['pc'], f['nw'] = p.get('pc'), p.get('nw')
        elif op == 'param':
            f['kq'] = param_kq(c.q)
            f['pc'] = p.get('pc')
        facts.append(f)
    return facts


def test_the_case_lists_reach_every_instantiation_and_edge():
    facts = _facts()
    adj = [f for f in facts if f['op'] == 'adjoint']
    par = [f for f in facts if f['op'] == 'param']
    sta = [f for f in facts if f['op'] == 'stats']
    # every adjoint instantiation, and the two paths inside KQ = 8 (chunk = every dim; a last chunk of one dim)
    slot = {(f['kq'], f['weighted']) for f in adj if not f['grouped']}
    assert slot == {(kq, wt) for kq in (1, 2, 4, 8) for wt in (False, True)}, slot
    assert {(f['kq'], f['pc']) for f in adj if f['grouped']} >= {(kq, pc) for kq in (1, 2, 4, 8) for pc in (1, 2, 4, 8)}
    for form in ('plain', 'weighted', 'grouped'):
        qs = {f['case'].q for f in adj if f['case'].form == form}
        assert qs & {5, 6, 7, 8} and {9, 17} <= qs, (form, 'the one path at KQ = 8; a last chunk of one dim')
        assert {5, 9} <= {f['case'].q for f in par if f['case'].form == form}, form
    # every parameter-adjoint instantiation
    slot = {(f['kq'], f['weighted']) for f in par if not f['grouped']}
    assert slot == {(kq, wt) for kq in (1, 2, 4) for wt in (False, True)}, slot
    assert {(f['kq'], f['pc']) for f in par if f['grouped']} >= {(kq, pc) for kq in (1, 2, 4) for pc in (1, 2, 4, 8)}
    assert {f['plan']['pc'] for f in sta if f['grouped']} == {1, 2, 4, 8}
    assert {f['nw'] for f in adj if f['grouped']} == {1, 2, 4}
    # the LDS switch points of the grouped adjoint, both sides, inside the budget; P = PC and PC + 1 at each
    for (qa, qb), p, n, (sa, sb) in E5_SWITCHES:
        for q, want in ((qa, sa), (qb, sb)):
            hit = [f for f in adj if f['grouped'] and f['case'].q == q and f['case'].n == n and f['case'].m == 33]
            assert any((f['pc'], f['nw']) == want and f['case'].p == p for f in hit), (q, want)
            assert {want[0], want[0] + 1} <= {f['case'].p for f in hit if f['pc'] == want[0]}, (q, 'P = PC and PC + 1')
    for f in facts:
        for kernel, lds in f['lds'].items():
            assert lds <= QG_LDS_BUDGET, (case_id(f['case']), kernel, lds)
    # the 48 KiB attribute boundary, both sides at neighbouring Q, per kernel (slot forms) and for the grouped adjoint
    for kernel, op in (('qp_adjoint', 'adjoint'), ('qp_param', 'param'), ('qp_param_psi1', 'param'), ('qp_psi2', 'stats')):
        for weighted in (False, True):
            by_q = {f['case'].q: f['lds'][kernel] for f in facts if f['op'] == op and not f['grouped'] and f['weighted'] == weighted}
            assert any(by_q[q] <= LDS_ATTR < by_q.get(q + 1, 0) for q in by_q), (kernel, weighted)
    # pair slabs: one tile per slab, every tile in one slab, and >= 3 tiles per slab with a slab that starts inside a block row
    for form in ('plain', 'weighted', 'grouped'):
        fs = [f for f in adj if f['case'].form == form]
        assert any(f['plan']['tiles'] > 1 and f['plan']['tiles_per_slab'] == 1 for f in fs), form
        assert any(f['plan']['tiles'] >= 10 and f['plan']['tiles_per_slab'] == f['plan']['tiles'] for f in fs), form
        assert any(f['plan']['tiles_per_slab'] >= 3 and _splits_a_block_row(f['plan']) for f in fs), form
    # n slabs, for both terms of the parameter adjoint and for stats: one staged step per slab; one slab longer than N; a slab of
    # several steps whose last step is ragged
    for form in ('plain', 'weighted', 'grouped'):
        for op, key, skey in (('stats', 'n_per_slab', 'slabs'), ('param', 'n_per_slab', 'slabs'), ('param', 'n_per_slab1', 'slabs1')):
            fs = [f for f in facts if f['op'] == op and f['case'].form == form]
            assert any(f['plan'][key] == QP_SN and f['plan'][skey] >= 3 for f in fs), (form, op, key)
            assert any(f['plan'][skey] == 1 and f['plan'][key] > f['case'].n and f['plan'][key] >= 2 * QP_SN for f in fs), (form, op, key)
            assert any(_ragged_multi_step(f['case'].n, f['plan'][key], f['plan'][skey]) for f in fs), (form, op, key)
    # E2: the dead fourth wave and the one live lane of the third at N = 129
    assert any(f['grouped'] and f['case'].n == 129 and f['nw'] == 4 for f in adj)


def _splits_a_block_row(p):
    starts, t, at = set(), p['T'], 0
    for i in range(t):
        starts.add(at)
        at += t - i
    return any(s * p['tiles_per_slab'] not in starts for s in range(1, p['slabs']))


def _ragged_multi_step(n, n_per_slab, slabs):
    last = n - (slabs - 1) * n_per_slab                            # points of the last slab
    return slabs >= 2 and last > QP_SN and last % QP_SN != 0


def test_comparators_fail_on_a_wrong_tile():
    want = np.random.default_rng(1).standard_normal((2, 70, 70))
    assert tiles_close_frac(want.copy(), want, TOL) == 0.0
    bad = want.copy()
    bad[1, 64:, 32:64] *= 1.0 + 1e-10
    with pytest.raises(AssertionError, match=r'tile \(2, 1\)'):
        tiles_close_frac(bad, want, TOL, 'psi2')
    bad = want.copy()
    bad[0, 40, 3] += 3e-12 * np.abs(want).max()
    with pytest.raises(AssertionError, match=r'tile \(1,\)'):
        tiles_close_frac(bad, want, TOL, 'd_z', axes=(-2,))
    with pytest.raises(AssertionError):
        close_frac(bad, want, TOL)
    bad = want.copy()
    bad[0, 0, 0] = np.nan
    with pytest.raises(AssertionError, match='not finite'):
        close_frac(bad, want, TOL)
    assert 0.4 < close_frac(want + 0.5e-12 * np.abs(want).max(), want, TOL) <= 1.0


# ----------------------------------------------------------------------------------------------- how far the reference itself is off
def _mp_loss(mp, t, x):
    """sum_k <g1_k, Psi1_k> + sum_kp <g2_kp, Psi2_kp> in mpmath (rbf_kernel.py:135-199 restated once more), x: {name: nested lists};
    also returns psi1 [K][N][M] and psi2 [K][P][M][M]."""
    z, mu, s, gamma, alpha = x['z'], x['mu'], x['s'], x['gamma'], x['alpha']
    w, g1, g2 = t['w'], t['g1'], t['g2']
    kk, m, q, n, pp = len(z), len(z[0]), len(mu[0]), len(mu), len(w)
    half, quarter = mp.mpf(1) / 2, mp.mpf(1) / 4
    loss = mp.mpf(0)
    psi1 = [[[None] * m for _ in range(n)] for _ in range(kk)]
    psi2 = [[[[mp.mpf(0)] * m for _ in range(m)] for _ in range(pp)] for _ in range(kk)]
    for k in range(kk):
        for i in range(n):
            for a in range(m):
                e = mp.mpf(0)
                c = mp.mpf(1)
                for d in range(q):
                    w1 = gamma[k][d] * s[i][d] + 1
                    e += gamma[k][d] * (mu[i][d] - z[k][a][d]) ** 2 / w1
                    c *= w1
                psi1[k][i][a] = alpha[k] * mp.exp(-half * e) / mp.sqrt(c)
                loss += g1[k][i][a] * psi1[k][i][a]
        for a in range(m):
            for b in range(m):
                for i in range(n):
                    e = mp.mpf(0)
                    c = mp.mpf(1)
                    for d in range(q):
                        w2 = 2 * gamma[k][d] * s[i][d] + 1
                        zbar = (z[k][a][d] + z[k][b][d]) / 2
                        e += quarter * gamma[k][d] * (z[k][a][d] - z[k][b][d]) ** 2 + gamma[k][d] * (mu[i][d] - zbar) ** 2 / w2
                        c *= w2
                    term = alpha[k] ** 2 * mp.exp(-e) / mp.sqrt(c)
                    for p in range(pp):
                        psi2[k][p][a][b] = psi2[k][p][a][b] + w[p][i] * term
                for p in range(pp):
                    loss += g2[k][p][a][b] * psi2[k][p][a][b]
    return loss, psi1, psi2


def test_the_autograd_reference_against_mpmath():
    """A tiny general case (K = 2, P = 2, M = 3, N = 4, Q = 2, real weights, g2 not symmetric): the statistics evaluated with 40 digits,
    the five gradients as central differences of the 40-digit loss with step 1e-13 (truncation ~1e-26, rounding ~1e-27: exact for this
    purpose).  The autograd reference must agree within 1e-14 x max(1, max |value|) per output: the GPU tolerance of 1e-12 then has two
    decades over the reference's own error.  Prints the measured ratios."""
    import mpmath
    mp = mpmath.mp
    c = mk('ref', 'grouped', 'real', 2, 2, 3, 4, 2)
    t = inputs(c)
    assert not torch.equal(t['g2'], t['g2'].transpose(2, 3))
    ref = _reference(c, 'all')
    saved = mp.dps
    mp.dps = 40
    try:
        conv = lambda a: None if a is None else _to_mp(mp, a.numpy())
        tm = {k: conv(a) for k, a in t.items()}
        x = {k: tm[k] for k in ('z', 'mu', 's', 'gamma', 'alpha')}
        _, psi1, psi2 = _mp_loss(mp, tm, x)
        want = dict(psi1=psi1, psi2=psi2)
        h = mp.mpf(10) ** -13
        for out, name in (('d_mu', 'mu'), ('d_s', 's'), ('d_z', 'z'), ('d_gamma', 'gamma'), ('d_alpha', 'alpha')):
            flat_shape = np.shape(t[name].numpy())
            grad = np.empty(flat_shape, dtype=object)
            for idx in np.ndindex(*flat_shape):
                vals = []
                for sign in (1, -1):
                    xs = dict(x)
                    xs[name] = _bumped(x[name], idx, sign * h)
                    vals.append(_mp_loss(mp, tm, xs)[0])
                grad[idx] = (vals[0] - vals[1]) / (2 * h)
            want[out] = grad
        for name in OUTPUTS:
            w_arr = np.array(want[name], dtype=object)
            have = ref[name].reshape(w_arr.shape)
            scale = max(1.0, max(abs(float(v)) for v in w_arr.flat))
            err = max(abs(float(mp.mpf(float(hv)) - wv)) for hv, wv in zip(have.flat, w_arr.flat))
            print('%s: reference against mpmath: max |err| %.3e = %.3f of %.0e x %.3g' % (name, err, err / (REF_TOL * scale), REF_TOL, scale))
            assert err <= REF_TOL * scale, name
    finally:
        mp.dps = saved


def _to_mp(mp, a):
    return [_to_mp(mp, r) for r in a] if np.ndim(a) else mp.mpf(float(a))


def _bumped(nested, idx, by):
    if len(idx) == 0:
        return nested + by
    out = list(nested)
    out[idx[0]] = _bumped(nested[idx[0]], idx[1:], by)
    return out
