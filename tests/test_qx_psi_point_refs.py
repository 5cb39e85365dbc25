"""
Case lists, references, plan mirror and comparators of tests/test_gpu_qx_psi_point_edges.py (the per-point Psi operators of
csrc/qx_psi_point.hip and csrc/qx_psi_point_adjoint.hip at every tile, chunk, slab and Q edge), and the CPU tests that show they can
be trusted:
  (a) the fp64 references (restated / moments_of of the feature tests, torch autograd for (d_mu, d_s)) agree with a 40-digit mpmath
      evaluation to 1e-14 max(1, max |value|) per output: two decades under the operators' 1e-12.  With z and mu moved by 50 the
      reference is measured the same way; tol_of says what that measurement means for the range cases;
  (b) a Python mirror of pw_plan, pm_plan, pa_plan, pw_lds, pm_lds, pa_lds, the CT / FT / MT / QREG dispatch and the three overrides
      DPGP_PW_PAIR_SLABS, DPGP_PA_K_SLABS, DPGP_PA_PAIR_SLABS gives the library's workspace size for every case under every override the
      GPU file runs, and for plan-only shapes of production size that are never launched;
  (c) the case lists reach every instantiation, both sides of every Q switch and of the 48 KiB dynamic-LDS attribute boundary of every
      kernel, and the slab / chunk shapes the natural plans never produce at test sizes;
  (d) with the overrides unset the workspace queries return what they returned before the overrides existed (recorded shapes).
"""
import collections
import functools
import zlib

import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import _lib
from test_gpu_qx_psi_point_moments import gidx_of, moments_of
from test_gpu_qx_psi_pointwise import restated
from test_pointwise_adjoint_refs import adjoint_case, closed_form

TOL = 1e-12                   # forward: the project's operator figure; adjoint against autograd: DESIGN 7.16 / 7.17
REF_TOL = 1e-14               # what the references are held to against mpmath
PW_KNOB, PA_K_KNOB, PA_PAIR_KNOB = 'DPGP_PW_PAIR_SLABS', 'DPGP_PA_K_SLABS', 'DPGP_PA_PAIR_SLABS'
KNOBS = (PW_KNOB, PA_K_KNOB, PA_PAIR_KNOB)
GIDX_KINDS = ('random', 'mixed')
MODES = ('all', 'h', 'gqgt')  # the adjoints that are not zero: all three; h alone (the Psi1 phase); gq and gt alone (the Psi2 phase)
UNSET = ()

# recipe: how the inputs are changed (inputs);  zero: which adjoints are zero ('wave': the points 16..31 and 64..127; 'kmid': kernel 1)
Case = collections.namedtuple('Case', 'family k g j m q n recipe zero')


def mk(family, k, g, j, m, q, n, recipe='std', zero=''):
    return Case(family, k, g, j, m, q, n, recipe, zero)


def case_id(c):
    tail = ('' if c.recipe == 'std' else '-' + c.recipe) + ('-' + c.zero if c.zero else '')
    return '%s-K%dG%dJ%d-M%d-Q%d-N%d%s' % (c.family, c.k, c.g, c.j, c.m, c.q, c.n, tail)


# ------------------------------------------------------------------------------------------------------------------------ the families
# P1: M at the 32-tile edges: the diagonal tile's skipped steps (s_lo = rr >> 2), ragged nr / nc, steps past M
P1 = [mk('P1', 2, 2, 3, m, 3, 33) for m in (1, 31, 32, 33, 63, 64, 65, 96, 97)]
# P2: N at the 16-point wave edges and the 64-point workgroup edges; J = 3 finishes with plain FMAs, J = 17 on the matrix pipe.  N = 17:
# wave 1 has one live lane and waves 2, 3 are wholly past N beside live ones; N = 129: a third workgroup with one live lane
P2 = [mk('P2', 2, 2, j, 33, 5, n) for n in (1, 15, 16, 17, 48, 49, 63, 64, 65, 128, 129) for j in (3, 17)]
# P3: column edges.  C = G + J around 16, 32, 64, 128 at Q = 10 and around 32, 64 at Q = 33 (G = 3); 6 and 7 column tiles inside CT = 8
# (C = 90, 100); G = 16 and 32 (no 16-tile mixes tr and quad); G = 130 (a chunk of tr columns only; tiles16 = 9: the last chunk is
# narrower than the planned one); J of the finishing kernels (G = 2), and their m loop at M = 31, 32, 33, 65
P3_C10, P3_C33 = (15, 16, 17, 31, 32, 33, 63, 64, 65, 90, 100, 127, 128, 129, 130), (31, 32, 33, 63, 64, 65, 66)
P3_J = (1, 4, 5, 15, 16, 17, 31, 32, 48, 49, 64, 65, 129)
P3 = [mk('P3', 1, 3, cc - 3, 33, 10, 33) for cc in P3_C10] + [mk('P3', 1, 3, cc - 3, 33, 33, 33) for cc in P3_C33] + \
     [mk('P3', 1, 16, 5, 33, 10, 33), mk('P3', 1, 32, 17, 33, 10, 33), mk('P3', 1, 16, 16, 33, 10, 33), mk('P3', 1, 130, 3, 33, 10, 33)] + \
     [mk('P3', 1, 2, j, 33, 10, 33) for j in P3_J] + [mk('P3', 1, 2, j, m, 10, 33) for j in (5, 17, 49) for m in (31, 32, 65)]
# P4: Q edges at M = 40, N = 70.  Column layouts a .. d give pw CT = 1, 2, 4, 8 (4 for Q > 32), pa CT = 2, 2, 4, 4 (2 for Q > 32) and the
# finishing kernels fma, mfma<1>, mfma<2>, mfma<4>.  Every layout at the Q switches; each layout at the Q pairs where one of its kernels
# crosses 48 KiB of dynamic LDS (the table in test_the_case_lists_reach_every_instantiation_and_edge)
P4_LAYOUT = dict(a=(2, 5), b=(2, 16), c=(3, 31), d=(2, 70))
P4_SWITCH_Q = (7, 8, 15, 16, 17, 23, 24, 32, 33, 39, 40, 64)
P4_LDS_Q = dict(a=(11, 12, 18, 19, 21, 22), b=(12, 13, 31), c=(2, 3, 6, 28, 29), d=(22,))
P4 = [mk('P4', 1, g, j, 40, q, 70) for name, (g, j) in P4_LAYOUT.items() for q in sorted(set(P4_SWITCH_Q) | set(P4_LDS_Q[name]))]
# P5: forced slabs.  M = 130: 15 tiles, T = 5;  M = 97: 10 tiles, T = 4.  K = 5: k slabs of 1, 5 and a ragged 3 + 2.  N = 40: the third
# wave is ragged and the fourth wholly past N
P5 = [mk('P5', 5, 2, 3, m, 5, 40) for m in (130, 97)]
# P6: idle and skipped work.  'wave': a wave (16..31) and a workgroup (64..127) of zero adjoints beside busy ones.  The zero points
# leave out a live workgroup's first point: the adjoint kernel centres mu and z on it, so its mu is an input of its neighbours' rounding.
# 'kmid': kernel 1 of 3 has zero adjoints (the k loop of one workgroup under DPGP_PA_K_SLABS = 1)
P6 = [mk('P6', 2, 2, 17, 65, 10, 130, zero='wave'), mk('P6', 3, 2, 3, 65, 10, 70, zero='kmid')]
# P7: range.  s0: s = 0 in a third of the rows;  gs1e4: gamma s up to 1e4;  far: a third of the points (0, 3, ..) 40 units away in every
# dim, the first point of each workgroup, on which the adjoint kernel centres mu and z, among them;  far1: the points 1, 4, .. instead (the
# centre stays among the inducing inputs);  shift50: z and mu moved by 50.  Register path (Q = 10) and LDS path (Q = 17)
P7 = [mk('P7', 2, 3, 17, 33, q, 65, recipe=recipe) for recipe in ('s0', 'gs1e4', 'far', 'far1', 'shift50') for q in (10, 17)]

FAMILIES = dict(P1=P1, P2=P2, P3=P3, P4=P4, P5=P5, P6=P6, P7=P7)
ALL_CASES = [c for fam in FAMILIES.values() for c in fam]


def tol_of(c):
    """1e-12 for every case, the range cases included.  DESIGN 7.17 widened its shifted cases by (1 + offset) because its references
    lost digits there; here test_the_references_against_mpmath measures the reference with z and mu moved by 50 at 0.18 of
    1e-14 max(1, max |value|) (0.07 without the offset: under three times that, and nearly three decades under 1e-12), so the reference
    needs no factor and the kernels get none."""
    return TOL


# --------------------------------------------------------------------------------------------------------------------- the plan mirror
TILE, NP, FSTRIDE, WPAD, QREG_MAX, TARGET_WGS, PM_MAXFT, PA_APAD, EXP2_TAB = 32, 64, 33, 16, 16, 512, 4, 4, 64
LDS_ATTR, LDS_MAX = 48 * 1024, 160 * 1024


def cdiv(a, b):
    return (a + b - 1) // b


def forced(env, name, hi):
    """dpgp_env_plan(name, 1, hi) of csrc/internal.h: 0 when unset or below 1 (the natural value stands), else the value clamped to hi."""
    env = dict(env)
    if name not in env:
        return 0
    v = int(env[name])
    return 0 if v < 1 else min(v, hi)


def _clamp(v, hi):
    return 1 if v < 1 else min(v, hi)


def _columns(g, j, ctmax):
    tiles16 = (g + j + 15) // 16
    nct = cdiv(tiles16, cdiv(tiles16, ctmax))
    return tiles16, nct, cdiv(tiles16, nct)


def pw_plan(k, g, j, n, m, q, env=UNSET):
    t = cdiv(m, TILE)
    p = dict(T=t, tiles=t * (t + 1) // 2, ntn=cdiv(n, NP), qreg=q <= QREG_MAX)
    p['tiles16'], p['nct'], p['nchunks'] = _columns(g, j, 8 if q <= 32 else 4)
    p['ct'] = 1 if p['nct'] <= 1 else 2 if p['nct'] <= 2 else 4 if p['nct'] <= 4 else 8
    sl = forced(env, PW_KNOB, p['tiles']) or cdiv(TARGET_WGS, p['ntn'] * k * p['nchunks'])
    p['tiles_per_slab'] = cdiv(p['tiles'], _clamp(sl, p['tiles']))
    p['slabs'] = cdiv(p['tiles'], p['tiles_per_slab'])
    return p


def pm_plan(j):
    tiles16 = cdiv(j, 16)
    nft = cdiv(tiles16, cdiv(tiles16, PM_MAXFT))
    return dict(mfma=j >= 16, nft=nft, nchunks=cdiv(tiles16, nft), ft=1 if nft <= 1 else 2 if nft <= 2 else 4)


def pa_plan(k, g, j, n, m, q, env=UNSET):
    t = cdiv(m, TILE)
    p = dict(T=t, tiles=t * (t + 1) // 2, ntn=cdiv(n, NP), qreg=q <= QREG_MAX)
    p['tiles16'], p['nct'], p['nchunks'] = _columns(g, j, 4 if q <= 32 else 2)
    p['ct'] = 2 if p['nct'] <= 2 else 4
    mt = cdiv(1 + 2 * q, 16)
    p['mt'] = 2 if mt <= 2 else 3 if mt <= 3 else 5 if mt <= 5 else 9
    base = p['ntn'] * p['nchunks']
    ks = forced(env, PA_K_KNOB, k) or cdiv(TARGET_WGS, base)
    p['k_per_slab'] = cdiv(k, _clamp(ks, k))
    p['kslabs'] = cdiv(k, p['k_per_slab'])
    ps = forced(env, PA_PAIR_KNOB, p['tiles']) or cdiv(TARGET_WGS, base * p['kslabs'])
    p['tiles_per_slab'] = cdiv(p['tiles'], _clamp(ps, p['tiles']))
    p['pslabs'] = cdiv(p['tiles'], p['tiles_per_slab'])
    return p


# pw_lds, pm_lds, pa_lds: copies of the formulas of the two .hip files.  No library query returns an LDS size (the workspace sizes do not
# depend on them), so nothing here checks the copies against the library: the 48 KiB and 160 KiB coverage assertions hold as far as these
# lines equal pw_lds / pm_lds / pa_lds / pa_fixed there, and whoever changes those changes these.
def pw_lds(q, ct):
    return 8 * (2 * q * NP + NP + 2 * TILE * q + q + TILE * FSTRIDE + TILE * (16 * ct + WPAD) + TILE * 16 * ct)


def pm_lds(q, f):
    return 8 * (2 * q * NP + NP + TILE * q + (TILE * (16 * f['ft'] + WPAD) if f['mfma'] else TILE * 16 + NP * FSTRIDE))


def pa_lds(q, ct, mt):
    stage = 2 * TILE * q + TILE * FSTRIDE + TILE * (16 * mt + WPAD) + TILE * (16 * ct + PA_APAD)
    return 8 * (2 * q * NP + NP + 2 * q + EXP2_TAB + max(stage, NP * (16 * mt + 1)))


def shape_of(c):
    return c.k, c.g, c.j, c.n, c.m, c.q              # (the operators take K, G, J, N, M, Q)


def workspace_bytes(op, shape, env=UNSET):
    """The mirror's dpgp_qx_psi_pointwise / point_moments ('fwd') and pointwise_adjoint ('adj') _workspace_bytes."""
    k, g, j, n, m, q = shape
    if op == 'fwd':
        return 8 * pw_plan(*shape, env)['slabs'] * k * n * (g + j)
    p = pa_plan(*shape, env)
    return 8 * p['kslabs'] * p['pslabs'] * p['nchunks'] * 2 * n * q


def library_workspace_bytes(op, shape):
    lib = _lib.lib()
    if op == 'fwd':
        a, b = lib.dpgp_qx_psi_pointwise_workspace_bytes(*shape), lib.dpgp_qx_psi_point_moments_workspace_bytes(*shape)
        assert a == b, 'the moments operator plans differently'
        return a
    return lib.dpgp_qx_psi_pointwise_adjoint_workspace_bytes(*shape)


def kernels_of(op, shape, env=UNSET):
    """{kernel instantiation: dynamic LDS bytes} of the launches of (op, shape)."""
    k, g, j, n, m, q = shape
    if op == 'fwd':
        p, f = pw_plan(*shape, env), pm_plan(j)
        fin = 'pm_finish_mfma<%d>' % f['ft'] if f['mfma'] else 'pm_finish_fma'
        return {'pw<%d,%s>' % (p['ct'], p['qreg']): pw_lds(q, p['ct']), fin: pm_lds(q, f)}
    p = pa_plan(*shape, env)
    assert p['ct'] == 2 or p['mt'] != 9, 'pa_dispatch has no <4,9>'
    return {'pa<%d,%d,%s>' % (p['ct'], p['mt'], p['qreg']): pa_lds(q, p['ct'], p['mt'])}


def set_env(monkeypatch, env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in env:
        monkeypatch.setenv(name, value)


# ----------------------------------------------------------------------------------------------- what the GPU file runs, per family
def _slab_values(tiles):
    return [None, 1, 2, 4, 6, tiles]


def fwd_envs(c):
    if c.family == 'P5':
        return [UNSET if v is None else ((PW_KNOB, str(v)),) for v in _slab_values(pw_plan(*shape_of(c))['tiles'])]
    return [UNSET, ((PW_KNOB, '2'),)] if c.family == 'P6' else [UNSET]


def adj_envs(c):
    if c.family == 'P5':
        tiles = pa_plan(*shape_of(c))['tiles']
        return [tuple(([(PA_PAIR_KNOB, str(ps))] if ps else []) + ([(PA_K_KNOB, str(ks))] if ks else []))
                for ps in _slab_values(tiles) for ks in (None, 1, 2, c.k)]
    return [UNSET, ((PA_K_KNOB, '1'),)] if c.family == 'P6' else [UNSET]


def modes_of(c):
    return MODES if c.family in ('P5', 'P6') else ('all',)


def all_runs():
    """[(op, shape, env)] of every launch plan of the GPU file."""
    out = []
    for c in ALL_CASES:
        out += [('fwd', shape_of(c), env) for env in fwd_envs(c)] + [('adj', shape_of(c), env) for env in adj_envs(c)]
    k, g, j, n, m, q = shape_of(P6[1])
    out += [('adj', (kk, g, j, n, m, q), ((PA_K_KNOB, '1'),)) for kk in (k - 1, 1)]     # (P6 'kmid': the calls without / with only the zero kernel)
    out += [('adj', shape_of(P6[0]), env) for env in adj_envs(P6[0])]                  # (P6 'wave': the calls with (mu, s) moved)
    return out


# ------------------------------------------------------------------------------------------------------------- inputs and references
@functools.lru_cache(maxsize=None)
def inputs(c):
    """The case's fp64 CPU tensors: z, mu, s, gamma, alpha, c, r (inputs_of through adjoint_case), beta, the adjoints h, gq, gt.  Cached and
    shared: never modified."""
    t, (h, gq, gt) = adjoint_case((c.k, c.g, c.j, c.m, c.q, c.n))
    rs = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    t['beta'] = torch.as_tensor(rs.uniform(0.5, 20.0, c.k))
    if c.recipe == 'shift50':
        t['z'], t['mu'] = t['z'] + 50.0, t['mu'] + 50.0
    elif c.recipe == 's0':
        t['s'][0::3] = 0.0
    elif c.recipe == 'gs1e4':
        s = t['s'] * torch.as_tensor(10.0 ** rs.uniform(-2.0, 4.0, (c.n, 1)))
        t['s'] = s * (1e4 / float((t['gamma'].max(dim=0).values * s).max()))          # (the largest gamma s is 1e4)
    elif c.recipe in ('far', 'far1'):
        t['mu'][(0 if c.recipe == 'far' else 1)::3] += 40.0
    else:
        assert c.recipe == 'std', c.recipe
    if c.zero == 'wave':
        for a in (h, gq, gt):
            a[:, 16:32] = 0.0
            a[:, 64:128] = 0.0
    elif c.zero == 'kmid':
        for a in (h, gq, gt):
            a[1] = 0.0
    else:
        assert c.zero == '', c.zero
    t.update(h=h, gq=gq, gt=gt)
    return {name: a.contiguous() for name, a in t.items()}


def adjoints(t, mode):
    """(h, gq, gt) of the mode: 'h' leaves only the Psi1 phase of the adjoint kernel something to do, 'gqgt' only the Psi2 phase."""
    h, gq, gt = t['h'], t['gq'], t['gt']
    return (h if mode != 'gqgt' else torch.zeros_like(h), gq if mode != 'h' else torch.zeros_like(gq), gt if mode != 'h' else torch.zeros_like(gt))


@functools.lru_cache(maxsize=None)
def reference(c):
    """{'tr', 'quad': restated;  ('mean', kind), ('var', kind), ('top', kind): moments_of;  ('d_mu', mode), ('d_s', mode): autograd of
    L = sum h (psi1 r) + sum gq quad + sum gt tr}: read-only numpy arrays, computed once per case."""
    t = inputs(c)
    mu, s = t['mu'].clone().requires_grad_(True), t['s'].clone().requires_grad_(True)
    w = restated(dict(t, mu=mu, s=s))
    mean = torch.matmul(w['psi1'], t['r'])
    out = {}
    for mode in modes_of(c):
        h, gq, gt = adjoints(t, mode)
        loss = torch.sum(h * mean) + torch.sum(gq * w['quad']) + torch.sum(gt * w['tr'])
        out[('d_mu', mode)], out[('d_s', mode)] = torch.autograd.grad(loss, (mu, s), retain_graph=True)
    plain = {name: w[name].detach() for name in ('tr', 'quad', 'psi1')}
    out.update(tr=plain['tr'], quad=plain['quad'])
    for kind in GIDX_KINDS:
        out[('mean', kind)], out[('var', kind)], _ = moments_of(t, plain, gidx_of(kind, c.k, c.g, c.j))
    out = {name: a.detach().numpy() for name, a in out.items()}
    for a in out.values():
        a.flags.writeable = False
    return out


# ------------------------------------------------------------------------------------------------------------------------ comparators
def blocks_close_frac(have, want, tol, what='', cols=None):
    """test_gpu_predict_b1.close at tol, one block at a time: per leading index (kernel k) where want has three dims, per 64 rows (points)
    and, with cols, per that many columns.  The bound of a block is tol (max(1, max |want| of the block) + |want|).  Returns the largest
    error as a fraction of its bound; a failure names its block."""
    have, want = np.asarray(have, dtype=np.float64).reshape(np.shape(want)), np.asarray(want, dtype=np.float64)
    assert np.isfinite(have).all(), what + ': not finite'
    if want.ndim == 2:
        have, want = have[None], want[None]
    worst = 0.0
    for k in range(want.shape[0]):
        for n0 in range(0, want.shape[1], NP):
            for c0 in range(0, want.shape[2], cols or want.shape[2]):
                sl = (k, slice(n0, n0 + NP), slice(c0, c0 + (cols or want.shape[2])))
                top = max(1.0, np.abs(want[sl]).max())
                ratio = np.abs(have[sl] - want[sl]) / (tol * top + tol * np.abs(want[sl]))
                frac = float(ratio.max())
                if frac > 1.0:
                    i = np.unravel_index(np.argmax(ratio), ratio.shape)
                    raise AssertionError('%s: block (k %d, points %d.., columns %d..): largest error %.3e of the bound (have %r, want %r)' %
                                         (what, k, n0, c0, frac, have[sl][i], want[sl][i]))
                worst = max(worst, frac)
    return worst


# ============================================================================================================================ CPU tests
def test_case_lists_are_sound():
    assert len(set(ALL_CASES)) == len(ALL_CASES), 'a case is listed twice'
    for c in ALL_CASES:
        assert c.m <= 130 and c.n <= 256 and c.k <= 5 and c.g + c.j <= 140 and 1 <= c.q <= 64, case_id(c)
        assert c.k * c.n * c.m * c.m * c.q <= 2e7, case_id(c)                   # (the reference takes a second at the most)
    assert [c.m for c in P1] == [1, 31, 32, 33, 63, 64, 65, 96, 97]
    assert sorted({c.n for c in P2}) == [1, 15, 16, 17, 48, 49, 63, 64, 65, 128, 129]
    assert {c.j for c in P3 if c.g == 2 and c.m == 33} == set(P3_J)
    assert {c.m for c in P3 if c.g == 2} == {31, 32, 33, 65}
    assert [pw_plan(*shape_of(c))['tiles'] for c in P5] == [15, 10]
    t = inputs(P6[0])
    for a in (t['h'], t['gq'], t['gt']):
        assert not a[:, 16:32].any() and not a[:, 64:128].any() and a[:, :16].all() and a[:, 32:64].all() and a[:, 128:].all()
    assert not inputs(P6[1])['gt'][1].any() and inputs(P6[1])['gt'][0].all() and inputs(P6[1])['gt'][2].all()
    for c in P7:
        t = inputs(c)
        if c.recipe == 's0':
            assert not t['s'][0::3].any() and t['s'][1::3].all()
        if c.recipe == 'gs1e4':
            assert abs(float((t['gamma'].max(dim=0).values * t['s']).max()) - 1e4) < 1e-6
        if c.recipe == 'shift50':
            assert float(t['mu'].min()) > 45.0 and float(t['z'].min()) > 45.0


# plan-only shapes: production sizes whose plans do not clamp the slab counts, so that the workspace depends on every plan field; never
# launched by a test (K = 512 over-D columns; the Q = 32 | 33 chunk switch with more workgroups than PW_TARGET_WGS / tiles)
PLAN_ONLY = [(512, 1, 1, 3000, 100, 10), (512, 1, 1, 100, 50, 10), (5, 3, 62, 256, 130, 32), (5, 3, 62, 256, 130, 33), (5, 3, 126, 300, 200, 33),
             (3, 2, 40, 2000, 130, 17), (40, 4, 130, 70, 200, 23), (2, 130, 3, 1000, 97, 64)]


def test_mirror_equals_the_library_workspace_queries(monkeypatch):
    """For every (operator, shape, override) the GPU file runs, and for the plan-only shapes under a grid of overrides: the library's
    workspace query, with the override in the environment, equals the mirror's."""
    runs = all_runs()
    for shape in PLAN_ONLY:
        for ps in (None, 1, 3, 7, 1000):
            runs.append(('fwd', shape, () if ps is None else ((PW_KNOB, str(ps)),)))
            for ks in (None, 1, 2, 3, 1000):
                runs.append(('adj', shape, tuple(([(PA_PAIR_KNOB, str(ps))] if ps else []) + ([(PA_K_KNOB, str(ks))] if ks else []))))
    for op, shape, env in sorted(set(runs)):
        set_env(monkeypatch, env)
        have = library_workspace_bytes(op, shape)
        assert have > 0 and have == workspace_bytes(op, shape, env), (op, shape, env)
    # the nchunks of the Q = 32 | 33 switch is visible in a workspace size
    assert workspace_bytes('fwd', PLAN_ONLY[2]) != workspace_bytes('fwd', PLAN_ONLY[3])
    assert pw_plan(*PLAN_ONLY[2])['nchunks'] == 1 and pw_plan(*PLAN_ONLY[3])['nchunks'] == 2
    # clamped as the natural value is; a value below 1 or no number leaves the natural plan; each knob moves only its own operator
    shape = shape_of(P5[0])
    k, g, j, n, m, q = shape
    natural = {op: workspace_bytes(op, shape) for op in ('fwd', 'adj')}
    assert natural == dict(fwd=8 * 15 * k * n * (g + j), adj=8 * 5 * 15 * 2 * n * q)          # (one tile and one kernel per slab)
    for value, slabs in (('1', 1), ('4', 4), ('6', 5), ('99', 15), ('0', 15), ('-1', 15), ('x', 15)):
        set_env(monkeypatch, ((PW_KNOB, value),))
        assert library_workspace_bytes('fwd', shape) == 8 * slabs * k * n * (g + j), value
        assert library_workspace_bytes('adj', shape) == natural['adj']
        set_env(monkeypatch, ((PA_PAIR_KNOB, value),))
        assert library_workspace_bytes('adj', shape) == 8 * 5 * slabs * 2 * n * q, value
        assert library_workspace_bytes('fwd', shape) == natural['fwd']
    for value, slabs in (('1', 1), ('2', 2), ('3', 3), ('4', 3), ('5', 5), ('99', 5), ('0', 5), ('-2', 5)):
        set_env(monkeypatch, ((PA_K_KNOB, value),))
        assert library_workspace_bytes('adj', shape) == 8 * slabs * 15 * 2 * n * q, value
        assert library_workspace_bytes('fwd', shape) == natural['fwd']


# (K, G, J, N, M, Q) -> (pointwise = point_moments, pointwise_adjoint) workspace bytes, recorded before the overrides existed
PARENT = {(512, 1, 1, 3000, 100, 10): (24576000, 5280000), (3, 2, 40, 130, 65, 17): (786240, 636480), (1, 1, 5, 33, 200, 10): (44352, 147840),
          (5, 3, 126, 300, 200, 33): (10836000, 19800000), (2, 3, 17, 65, 33, 10): (62400, 62400)}


def test_unset_overrides_leave_the_recorded_workspace_sizes(monkeypatch):
    set_env(monkeypatch, UNSET)
    for shape, want in PARENT.items():
        assert (library_workspace_bytes('fwd', shape), library_workspace_bytes('adj', shape)) == want, shape


def _facts():
    facts = []
    for op, shape, env in sorted(set(all_runs())):
        plan = (pw_plan if op == 'fwd' else pa_plan)(*shape, env)
        facts.append(dict(op=op, shape=shape, env=env, plan=plan, kernels=kernels_of(op, shape, env), q=shape[5], fin=pm_plan(shape[2])))
    return facts


def _splits_a_block_row(p, slabs):
    starts, at = set(), 0
    for i in range(p['T']):
        starts.add(at)
        at += p['T'] - i
    return any(s * p['tiles_per_slab'] not in starts for s in range(1, slabs))


# kernel instantiation -> (last Q at or below 48 KiB of dynamic LDS, first Q above); pw CT = 8 is always above
LDS_EDGES = {'pw<1,': (18, 19), 'pw<2,': (12, 13), 'pw<4,': (2, 3), 'pa<2,2,': (11, 12), 'pa<4,2,': (6, 7), 'pm_finish_fma': (21, 22),
             'pm_finish_mfma<1>': (31, 32), 'pm_finish_mfma<2>': (28, 29), 'pm_finish_mfma<4>': (22, 23)}


def test_the_case_lists_reach_every_instantiation_and_edge():
    facts = _facts()
    fwd, adj = [f for f in facts if f['op'] == 'fwd'], [f for f in facts if f['op'] == 'adj']
    names = {name for f in facts for name in f['kernels']}
    want = {'pw<%d,%s>' % (ct, qr) for ct in (1, 2, 4, 8) for qr in (True, False)} | {'pm_finish_fma'} | \
           {'pm_finish_mfma<%d>' % ft for ft in (1, 2, 4)} | \
           {'pa<%d,%d,%s>' % x for x in ((2, 2, True), (4, 2, True), (2, 3, True), (4, 3, True), (2, 3, False), (4, 3, False), (2, 5, False),
                                         (4, 5, False), (2, 9, False))}
    assert names == want, names ^ want
    assert {f['fin']['nft'] for f in fwd if f['fin']['mfma']} == {1, 2, 3, 4}
    assert {(f['fin']['ft'], f['fin']['nft']) for f in fwd if f['fin']['mfma']} >= {(1, 1), (2, 2), (4, 3), (4, 4)}
    assert any(f['fin']['mfma'] and f['fin']['nchunks'] == 3 for f in fwd)
    # both sides of every Q switch, for each operator and each chunk width of P4
    for op, fs in (('fwd', fwd), ('adj', adj)):
        for layout, (g, j) in P4_LAYOUT.items():
            qs = {f['q'] for f in fs if f['shape'][1:3] == (g, j) and f['shape'][4] == 40}
            assert set(P4_SWITCH_Q) <= qs, (op, layout)
    for (g, j), (ct_lo, ct_hi) in (((2, 70), (8, 4)),):                       # the chunk-width switch at Q = 32 | 33
        assert pw_plan(1, g, j, 70, 40, 32)['ct'] == ct_lo and pw_plan(1, g, j, 70, 40, 33)['ct'] == ct_hi
        assert pa_plan(1, g, j, 70, 40, 32)['ct'] == 4 and pa_plan(1, g, j, 70, 40, 33)['ct'] == 2
    assert [pa_plan(1, 2, 5, 70, 40, q)['mt'] for q in (7, 8, 15, 16, 23, 24, 39, 40)] == [2, 2, 2, 3, 3, 5, 5, 9]
    # every LDS size inside 160 KiB; both sides of 48 KiB for every kernel instantiation, at neighbouring Q
    for f in facts:
        for name, lds in f['kernels'].items():
            assert lds <= LDS_MAX, (f['shape'], name, lds)
    for stem, (lo, hi) in LDS_EDGES.items():
        by_q = {}
        for f in facts:
            for name, lds in f['kernels'].items():
                if name.startswith(stem):
                    by_q.setdefault(f['q'], set()).add(lds)
        assert lo in by_q and hi in by_q and max(by_q[lo]) <= LDS_ATTR < min(by_q[hi]), (stem, sorted(by_q))
        assert all((max(v) <= LDS_ATTR) == (q <= lo) for q, v in by_q.items()), stem
    assert all(lds > LDS_ATTR for f in fwd for name, lds in f['kernels'].items() if name.startswith('pw<8,'))
    # the register / LDS point path on both sides of Q = 16 | 17, in every chunk width
    for ct in (1, 2, 4, 8):
        assert {16, 17} <= {f['q'] for f in fwd if f['plan']['ct'] == ct}, ct
    for ct in (2, 4):
        assert {16, 17} <= {f['q'] for f in adj if f['plan']['ct'] == ct}, ct
    # slabs of pair tiles: one tile per slab, every tile in one slab, >= 3 tiles per slab with a slab that starts inside a block row
    for fs, key in ((fwd, 'slabs'), (adj, 'pslabs')):
        assert any(f['plan']['tiles'] > 1 and f['plan']['tiles_per_slab'] == 1 for f in fs)
        assert any(f['plan']['tiles'] >= 10 and f['plan']['tiles_per_slab'] == f['plan']['tiles'] for f in fs)
        assert any(f['plan']['tiles_per_slab'] >= 3 and f['plan'][key] >= 2 and _splits_a_block_row(f['plan'], f['plan'][key]) for f in fs)
    # slabs of kernels: one per slab, all in one slab, ragged (K = 5 in 2 slabs: 3 + 2); each with several tiles per slab too
    for per, slabs in ((1, 5), (5, 1), (3, 2)):
        hit = [f for f in adj if f['shape'][0] == 5 and (f['plan']['k_per_slab'], f['plan']['kslabs']) == (per, slabs)]
        assert any(f['plan']['tiles_per_slab'] == 1 for f in hit) and any(f['plan']['tiles_per_slab'] >= 3 for f in hit), (per, slabs)
    # columns: a last chunk narrower than the planned one (tiles16 = 9); 6 and 7 tiles inside CT = 8; chunks of tr columns only, of quad
    # columns only, a 16-tile that mixes both and G a multiple of 16 (none does)
    for fs in (fwd, adj):
        assert any(f['plan']['tiles16'] % f['plan']['nct'] for f in fs if f['plan']['tiles16'] == (9 if fs is fwd else 5))    # (5 + 4; 3 + 2)
        kinds = set()
        for f in fs:
            g, c, width = f['shape'][1], f['shape'][1] + f['shape'][2], 16 * f['plan']['nct']
            for ch in range(f['plan']['nchunks']):
                lo, hi = ch * width, min(c, (ch + 1) * width)
                kinds.add('tr' if hi <= g else 'quad' if lo >= g else 'both')
            kinds.add('mixed tile' if g % 16 else 'tile edge')
        assert kinds == {'tr', 'quad', 'both', 'mixed tile', 'tile edge'}, kinds
    assert {6, 7} <= {f['plan']['nct'] for f in fwd if f['plan']['ct'] == 8}
    assert any(f['shape'][1] > 128 for f in fwd)
    # a chunk exactly full and one column more: 128 | 129 forward, 64 | 65 adjoint; at Q > 32 64 | 65 and 32 | 33
    for fs, q, cs in ((fwd, 10, (128, 129)), (adj, 10, (64, 65)), (fwd, 33, (64, 65)), (adj, 33, (32, 33))):
        chunks = {f['shape'][1] + f['shape'][2]: f['plan']['nchunks'] for f in fs if f['q'] == q and f['shape'][4] == 33 and f['shape'][1] == 3}
        assert chunks[cs[0]] == 1 and chunks[cs[1]] == 2, (q, cs)


def test_comparator_fails_on_one_wrong_block():
    want = np.random.default_rng(1).standard_normal((2, 130, 40))
    want[1, 64:128] *= 1e-3                                                   # (a small block beside large ones)
    assert blocks_close_frac(want.copy(), want, TOL, cols=16) == 0.0
    bad = want.copy()
    bad[1, 70, 33] += 3e-12                                                   # (3e-12 of the largest entry: passes `close` on the whole array)
    np.testing.assert_allclose(bad, want, rtol=3e-12, atol=3e-12 * np.abs(want).max())
    with pytest.raises(AssertionError, match=r'k 1, points 64.., columns 32..'):
        blocks_close_frac(bad, want, TOL, 'x', cols=16)
    bad = want[0].copy()
    bad[129, 0] = np.nan
    with pytest.raises(AssertionError, match='not finite'):
        blocks_close_frac(bad, want[0], TOL)
    assert 0.4 < blocks_close_frac(want[0] + 0.5e-12 * np.maximum(1.0, np.abs(want[0]).max()), want[0], TOL) <= 1.0


def test_closed_form_against_the_references():
    """The algebra the adjoint kernel implements (closed_form of test_pointwise_adjoint_refs) against autograd at one case per family
    and mode, blockwise: both are fp64, so 1e-12 here says the references of the modes and recipes are the quantity the kernel forms.
    The closed form expands (mu - z)^2 into moments of z, so for shift50 it is given z - 50 and mu - 50 (exact subtractions; only mu - z
    enters), as the kernel centres both on a point of the workgroup; handed the offset itself it sits at 1.03 of this bound."""
    for c in (P1[3], P2[7], P5[1], P6[0], P6[1], P7[0], P7[2], P7[4], P7[8]):
        t, ref = inputs(c), reference(c)
        if c.recipe == 'shift50':
            t = dict(t, z=t['z'] - 50.0, mu=t['mu'] - 50.0)
        for mode in modes_of(c):
            have = closed_form(t, adjoints(t, mode))
            for name, hv in zip(('d_mu', 'd_s'), have):
                blocks_close_frac(hv.numpy(), ref[(name, mode)], tol_of(c), '%s %s %s' % (case_id(c), mode, name))


# ----------------------------------------------------------------------------------------------- how far the references themselves are off
def _mp_forward(mp, x, adj):
    """tr [K][N][G], quad, psi1r [K][N][J] and L = sum h psi1r + sum gq quad + sum gt tr in mpmath; x: {name: nested lists of mpf}."""
    z, mu, s, gamma, alpha, cm, r = (x[k] for k in ('z', 'mu', 's', 'gamma', 'alpha', 'c', 'r'))
    h, gq, gt = adj
    kk, m, q, n, g, j = len(z), len(z[0]), len(mu[0]), len(mu), len(cm[0]), len(r[0][0])
    half, quarter, loss = mp.mpf(1) / 2, mp.mpf(1) / 4, mp.mpf(0)
    tr = [[[mp.mpf(0)] * g for _ in range(n)] for _ in range(kk)]
    quad = [[[mp.mpf(0)] * j for _ in range(n)] for _ in range(kk)]
    p1r = [[[mp.mpf(0)] * j for _ in range(n)] for _ in range(kk)]
    for k in range(kk):
        for i in range(n):
            for a in range(m):
                e, w = mp.mpf(0), mp.mpf(1)
                for d in range(q):
                    w1 = gamma[k][d] * s[i][d] + 1
                    e += gamma[k][d] * (mu[i][d] - z[k][a][d]) ** 2 / w1
                    w *= w1
                psi1 = alpha[k] * mp.exp(-half * e) / mp.sqrt(w)
                for jj in range(j):
                    p1r[k][i][jj] += psi1 * r[k][a][jj]
                for b in range(m):
                    e, w = mp.mpf(0), mp.mpf(1)
                    for d in range(q):
                        w2 = 2 * gamma[k][d] * s[i][d] + 1
                        e += quarter * gamma[k][d] * (z[k][a][d] - z[k][b][d]) ** 2 + gamma[k][d] * (mu[i][d] - (z[k][a][d] + z[k][b][d]) / 2) ** 2 / w2
                        w *= w2
                    psi2 = alpha[k] ** 2 * mp.exp(-e) / mp.sqrt(w)
                    for gg in range(g):
                        tr[k][i][gg] += cm[k][gg][a][b] * psi2
                    for jj in range(j):
                        quad[k][i][jj] += r[k][a][jj] * r[k][b][jj] * psi2
            for jj in range(j):
                loss += h[k][i][jj] * p1r[k][i][jj] + gq[k][i][jj] * quad[k][i][jj]
            for gg in range(g):
                loss += gt[k][i][gg] * tr[k][i][gg]
    return loss, tr, quad, p1r


def _to_mp(mp, a):
    return [_to_mp(mp, r) for r in a] if np.ndim(a) else mp.mpf(float(a))


def _bumped(nested, idx, by):
    if len(idx) == 0:
        return nested + by
    out = list(nested)
    out[idx[0]] = _bumped(nested[idx[0]], idx[1:], by)
    return out


def reference_error_against_mpmath(c):
    """{output: max |reference - 40-digit value| / (1e-14 max(1, max |value|))} of a tiny case: tr, quad, mean, var directly, (d_mu, d_s)
    as central differences of the 40-digit loss with step 1e-13 (truncation ~1e-26)."""
    import mpmath
    mp = mpmath.mp
    t, ref = inputs(c), reference(c)
    saved, mp.dps = mp.dps, 40
    try:
        x = {k: _to_mp(mp, t[k].numpy()) for k in ('z', 'mu', 's', 'gamma', 'alpha', 'c', 'r', 'beta')}
        adj = tuple(_to_mp(mp, t[k].numpy()) for k in ('h', 'gq', 'gt'))
        _, tr, quad, p1r = _mp_forward(mp, x, adj)
        want = {'tr': tr, 'quad': quad}
        for kind in GIDX_KINDS:
            gidx = gidx_of(kind, c.k, c.g, c.j).numpy()
            want[('mean', kind)] = p1r
            want[('var', kind)] = [[[x['alpha'][k] + 1 / x['beta'][k] - (tr[k][i][gidx[k, jj]] if 0 <= gidx[k, jj] < c.g else 0) + quad[k][i][jj]
                                     - p1r[k][i][jj] ** 2 for jj in range(c.j)] for i in range(c.n)] for k in range(c.k)]
        step = mp.mpf(10) ** -13
        for out, name in (('d_mu', 'mu'), ('d_s', 's')):
            grad = np.empty((c.n, c.q), dtype=object)
            for idx in np.ndindex(c.n, c.q):
                up, dn = (_mp_forward(mp, dict(x, **{name: _bumped(x[name], idx, sign * step)}), adj)[0] for sign in (1, -1))
                grad[idx] = (up - dn) / (2 * step)
            want[(out, 'all')] = grad
        fracs = {}
        for name, w in want.items():
            w = np.array(w, dtype=object)
            have = ref[name].reshape(w.shape)
            scale = max(1.0, max(abs(float(v)) for v in w.flat))
            err = max(abs(float(mp.mpf(float(hv)) - wv)) for hv, wv in zip(have.flat, w.flat))
            fracs[name] = err / (REF_TOL * scale)
        return fracs
    finally:
        mp.dps = saved


MP_CASE = mk('ref', 2, 2, 3, 3, 2, 4, recipe='s0')                # (K = 2, G = 2, J = 3, M = 3, N = 4, Q = 2; rows 0 and 3 have s = 0)
MP_SHIFTED = [MP_CASE._replace(recipe='shift50'), mk('ref', 1, 2, 3, 3, 8, 2, recipe='shift50')]      # (the second: more dims to sum over)


def test_the_references_against_mpmath():
    """One general small case, c not symmetric, rows with s = 0: every reference output within 1e-14 max(1, max |value|) of the 40-digit
    value, so that the GPU tolerance of 1e-12 keeps two decades over the reference's own error.  With z and mu moved by 50 (s as drawn;
    also at Q = 8) the same bound holds: the range cases need no wider tolerance (tol_of).  Prints the measured fractions."""
    t = inputs(MP_CASE)
    assert not torch.equal(t['c'], t['c'].transpose(2, 3)) and not t['s'][0].any() and t['s'][1].all()
    for c in [MP_CASE] + MP_SHIFTED:
        fracs = reference_error_against_mpmath(c)
        for name, frac in fracs.items():
            print('%s Q=%d %s: reference against mpmath: %.3f of 1e-14 max(1, max |value|)' % (c.recipe, c.q, name, frac))
        print('%s Q=%d: largest %.3f' % (c.recipe, c.q, max(fracs.values())))
        assert max(fracs.values()) <= 1.0, (c.recipe, fracs)
