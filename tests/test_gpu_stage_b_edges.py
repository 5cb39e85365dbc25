"""
GPU tests of the pair-tile stage B (csrc/psi2_pairs_grad.hip: the operand images, pg_pass_kernel's two Psi2 passes and two Psi1
passes, the finishing kernels) at every edge of its dispatch: K-steps and feature blocks, resident column tiles per wave G, the
LDS ring's chunk boundaries, column tails, the output-dim chunks of the finishing kernels, the power-of-two scale factors, and
the split training step.

Reference (stage_b_reference): torch fp64 autograd on the CPU of

    L = sum_d <G2_d, Psi2_d> + sum_d sum_m gv[d, m] (Psi1_d^T y_d)[m] + sum_d <GK_d, K_d>

with respect to (mu, S, z, gamma), the formulas of oracle/dpgp_oracle_torch.py:psi_pieces with Psi2 taken over the pairs m' <= m
(G2 is symmetric) and the squares expanded into matrix products, chunked over the observations, memoised per case.  The CPU
sibling tests/test_stage_b_refs.py pins it against ot.fhat_input_gradients and ot.psi_pieces.

Inputs (problem): z = 2 N(0,1) (4 N(0,1) for M > 128), mu = 1.5 N(0,1), S = exp(0.3 N(0,1)), gamma = exp(0.3 N(0,1)) 2 / Q,
alpha = exp(0.2 N(0,1)), G2_d = +-(1 + 0.1 N(0,1)) exp(-0.1 |z_m - z_m'|^2) (smooth and definite, a random sign per d), gv and y
N(0,1), GK = 0 unless the case says 'gk'.  The seed is the CRC-32 of the case tuple (d, n, m, q, mod, bump).  bump is 0; where a
draw fails the tail-visibility condition below it is the smallest positive integer whose draw passes (BUMPS).

Call (call_stage_b): dpgp_elbo_grad_psi_ex through ctypes with a workspace of exactly dpgp_elbo_grad_psi_workspace_bytes_ex bytes
pre-filled with NaN bytes and followed, in the same allocation, by 1 MiB of 0xA5 that must come back unchanged; the four outputs
pre-filled with NaN; every result finite.

Comparison: check_cols (tests/test_gpu_grad_psi_full_adjoint.py), 'mixed' at the mixed stage-B tolerance GRAD_TOL = 5e-4 of each
column's largest entry (tests/test_gpu_scales.py), 'mixed_fast' at its stated 2e-3 (tests/test_gpu_grad.py: FAST_GRAD_TOL).

Tail visibility (tail_visibility; asserted for every case by the CPU sibling): the reference entries of the last observation (in
d mu or d S), of the last inducing point (d z) and of the last output dim (d gamma) reach 0.05 of their column's largest entry in
at least one column, so that a dropped tail row, point or dim shows at 5e-4.

Which kernel ran (passes): the cost rule of pg_launch_pass and the ring size of pg_ring_tiles mirrored in Python, with the
experiment switches DPGP_PG_G (2 / 3 / 4 at KS <= 4, 1 / 2 at KS = 8), DPGP_PG_G1 and DPGP_PG_NTB, which the library reads on every
call.  Every pass of every case is labelled (KS, G, WLO, row tiles, column tiles, NTb); test_case_table_reaches_every_variant fails
if the table does not reach each (KS, G) in pass 1 and in pass 2 on this device.

The case table, (D, N, M, Q):
  1. K-steps and feature blocks (KSTEP_CASES): (3, 70, 17, Q), Q = 1, 5, 6, 10, 11, 15, 16, 20, 21 (KS = 2, 2, 4, 4, 6, 6, 8, 8, 8;
     Q = 5, 21: no third piece of the row constant; Q >= 16: two feature blocks), 'mixed' and 'mixed_fast'; Q = 21 is the rank-1
     Psi1 term through pg_finish_m1_kernel<64, 24>.  (3, 37, 65, 22): the handover to the patch form and grad.hip's Psi1 kernels.
  2. Column groups (GROUP_CASES): forced at D = 2, for (KS, Q, G) in (2, 3, 2|3|4), (4, 7, 2|3|4), (6, 12, 2), (8, 17, 1|2), with
     c = 1, 8 G, 8 G + 1 column tiles on BOTH sides: N = 31, 32 * 8 G, 32 * 8 G + 1 and the largest M with at most c pair tiles,
     ceil(M (M + 1) / 64) (M = 7; 22, 31, 38, 44; 23, 32, 39, 45; 32 pair tiles do not exist: M = 44 has 31 and M = 45 has 33).
     Natural picks on 256 compute units (NATURAL_CASES): (129, 513, 32, 3) -> G = 3, (129, 769, 39, 7) -> G = 4,
     (129, 257, 23, 16) -> G = 2 at KS = 8, in both passes.
  3. Ring (RING_CASES): row tiles r = 1, NTb, NTb + 1, 2 NTb + 1, 3 NTb, 3 NTb + 1, 4 NTb + 1 at NTb = 8 / 6 / 5 / 3 (KS = 2 / 4 / 6 / 8,
     Q = 4 / 8 / 13 / 18), D = 2: (N = 32 r, the largest M with at most r pair tiles) and (N = 32 (r - 1) + 1, the smallest M with at
     least r) — r observation tiles as rows of pass 1, r (or its nearest neighbours) pair tiles as rows of pass 2.  KS <= 4 also at
     G = 4 and KS = 8 also at G = 2 (one register set for the exponent operand); KS = 8 at G = 1 from the third chunk on takes the
     register-staged fills.  Inducing points as rows (the Psi1 back pass, MROW_CASES): (2, 40, 97, 16) and (2, 40, 289, 16) at KS = 8
     (4 = NTb + 1 and 10 = 3 NTb + 1 row tiles), and (2, 40, M, 4 | 8 | 13), M = 32, 33, 65, 97, 200 under DPGP_PG_NTB = 1 and 2.
  4. Output-dim chunks (DIM_CASES): (D, 33, 17, 3), D = 1, 2, 9, 16, 17, 64, 65, 257, 513, and (65, 33, 17, 16).
  5. Scale edges (SCALE_CASES) at (4, 70, 20, 4): G2 / gv / one y column of output dim 1 all zero; the largest |u_dp| (= |G2| alpha^2
     exp(-1/4 sum gamma dz^2), doubled off the diagonal; the G2 of these cases has its off-diagonal entries halved, so the maximum is
     the diagonal's), |alpha gv| or |y| of every output dim exactly 2^k, k = -20, 0, 20 (alpha = 1, one tensor at a time,
     the other term's adjoint scaled by 2^k with it so that both terms stay visible in the sums);
     gamma = 1e-6 on every other latent dim; one NaN in y must come back as NaN in all four outputs.
  6. The split step (SPLIT_CASES): (3, 70, 40, 4), (2, 40, 257, 16) (M Q > 4096: pg_u_scale_kernel reads z from memory) and
     (2, 40, 40, 21) (the step's own pieces at the largest Q: pg_u_scale_kernel, Psi2 out of feature 42 of pass 1, the Psi1^T y
     epilogue) through ops.elbo_fhat_step + ops.elbo_grad_psi_step with GK != 0, twice on the same buffers.  The fused ops.elbo_step
     at M = 128, Q = 20 is the shape (150, 4, 128, 20) of test_gpu_grad.test_training_step_equals_the_three_calls.
"""
import collections
import functools
import zlib

import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import _lib, ops
from test_gpu_grad import FAST_GRAD_TOL
from test_gpu_grad_psi_full_adjoint import check_cols
from test_gpu_scales import GRAD_TOL, TERM_TOL

pytestmark = pytest.mark.gpu

JITTER = 1e-8
TOL = {'mixed': GRAD_TOL, 'mixed_fast': FAST_GRAD_TOL}
GUARD_BYTES, GUARD_BYTE = 1 << 20, 0xA5
SWITCHES = ('DPGP_PG_G', 'DPGP_PG_G1', 'DPGP_PG_NTB', 'DPGP_GRAD_PATCH', 'DPGP_GRAD_PLAIN', 'DPGP_PSI1_PLAIN')
NAMES = ('d mu', 'd S', 'd z', 'd gamma')

Case = collections.namedtuple('Case', 'd n m q mod bump', defaults=('', 0))
# (d, n, m, q, mod) -> bump, where bump = 0 fails the tail-visibility condition: the smallest bump whose draw passes (the CPU sibling
# checks both halves of that).  The large ones are M >= 200 inducing points spread by 4 N(0,1) around 40 observations: the last one has
# to land near the data to carry any gradient at all.
BUMPS = {(2, 1, 1, 18, ''): 1, (2, 31, 7, 12, ''): 1, (2, 32, 7, 18, ''): 1, (2, 40, 33, 8, ''): 1, (2, 40, 65, 13, ''): 2,
         (2, 40, 97, 16, ''): 1, (2, 40, 200, 4, ''): 1, (2, 40, 200, 8, ''): 14, (2, 40, 200, 13, ''): 14, (2, 40, 289, 16, ''): 11,
         (2, 161, 18, 8, ''): 1, (2, 225, 21, 4, ''): 2, (2, 449, 30, 13, ''): 2, (2, 512, 31, 3, ''): 1, (2, 641, 36, 13, ''): 1,
         (2, 800, 39, 8, ''): 1, (2, 1025, 45, 3, ''): 1, (3, 70, 40, 4, 'gk'): 1, (4, 70, 20, 4, 'gvpow20'): 1,
         (17, 33, 17, 3, ''): 1}


def case(d, n, m, q, mod=''):
    return Case(d, n, m, q, mod, BUMPS.get((d, n, m, q, mod), 0))


def case_id(c):
    return 'D%d_N%d_M%d_Q%d%s' % (c.d, c.n, c.m, c.q, '_' + c.mod if c.mod else '')


def env_id(env):
    return '-'.join('%s%s' % (k.replace('DPGP_PG_', ''), v) for k, v in env) or 'auto'


# ---------------------------------------------------------------------------------------------------------------
# the dispatch of psi2_pairs_grad.hip, mirrored
# ---------------------------------------------------------------------------------------------------------------

NTB_DEFAULT = {2: 8, 4: 6, 6: 5, 8: 3}        # pg_ring_tiles: 160 KB / (3 chunks x (KS + pg_xp) KB)
VARIANTS = [(2, 2), (2, 3), (2, 4), (4, 2), (4, 3), (4, 4), (6, 2), (8, 1), (8, 2)]     # (KS, G) instances of pg_pass_kernel


def ceil_div(a, b):
    return -(-a // b)


def ksteps(q):
    """psi2_pairs_ksteps: 6 Q + 2 slots in K-steps of 16, an even number of them."""
    return 2 * ceil_div(6 * q + 2, 32)


def pgrad_supported(m, q):
    ks = ksteps(q)
    return ks <= 8 and 2 * q + 1 <= (48 if ks >= 8 else 32) and 1 <= m <= 4096


def pair_tiles(m):
    return ceil_div(m * (m + 1) // 2, 32)


def pick_g(ks, d, col_tiles, ncu, env=()):
    """pg_launch_pass: resident column tiles per wave for a pass of D output dims x col_tiles column tiles on ncu compute units."""
    env = dict(env)
    cost = lambda g, permille: ceil_div(d * ceil_div(col_tiles, 8 * g), ncu) * g * permille
    force = int(env['DPGP_PG_G']) if 'DPGP_PG_G' in env else None
    if ks <= 4:
        if force is not None:
            return force if force in (3, 4) else 2
        c2, c3, c4 = cost(2, 1000), cost(3, 945), cost(4, 940)
        return 4 if (c4 < c3 and c4 < c2) else (3 if c3 < c2 else 2)
    if ks == 6:
        return 2
    if force == 2:
        return 2
    return 2 if (force != 1 and 'DPGP_PG_G1' not in env and cost(2, 920) <= cost(1, 1000)) else 1


def ring_tiles(ks, env=()):
    """pg_ring_tiles: row tiles per chunk of the LDS ring (DPGP_PG_NTB shrinks it; not below 2 at KS = 8)."""
    ntb = NTB_DEFAULT[ks]
    v = int(dict(env).get('DPGP_PG_NTB', 0))
    return v if (2 if ks == 8 else 1) <= v <= ntb else ntb


def passes(c, prec, env, ncu):
    """The four launches of pg_pass_kernel behind one call, as (name, KS, G, WLO, row tiles, column tiles, NTb)."""
    if not pgrad_supported(c.m, c.q) or prec == 'mixed_patch':
        return []
    ks, nt, pt, mt = ksteps(c.q), ceil_div(c.n, 32), pair_tiles(c.m), ceil_div(c.m, 32)
    wlo, ntb = prec != 'mixed_fast', ring_tiles(ks, env)
    return [(name, ks, pick_g(ks, c.d, cols, ncu, env), wlo, rows, cols, ntb)
            for name, rows, cols in (('psi2 pass 1', nt, pt), ('psi2 pass 2', pt, nt), ('psi1 pass 1', nt, mt), ('psi1 pass 2', mt, nt))]


# ---------------------------------------------------------------------------------------------------------------
# inputs and reference
# ---------------------------------------------------------------------------------------------------------------

def problem(c):
    d, n, m, q = c.d, c.n, c.m, c.q
    mods = c.mod.split('+') if c.mod else []
    rng = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    z = (4.0 if m > 128 else 2.0) * rng.standard_normal((m, q))
    mu = 1.5 * rng.standard_normal((n, q))
    s = np.exp(0.3 * rng.standard_normal((n, q)))
    gamma = np.exp(0.3 * rng.standard_normal((d, q))) * 2.0 / q
    alpha = np.exp(0.2 * rng.standard_normal(d))
    dist = ((z[:, None, :] - z[None, :, :]) ** 2).sum(-1)
    sign = np.where(rng.random(d) < 0.5, -1.0, 1.0)
    g2 = (sign * (1.0 + 0.1 * rng.standard_normal(d)))[:, None, None] * np.exp(-0.1 * dist)[None]
    gv = rng.standard_normal((d, m))
    y = rng.standard_normal((n, d))
    gk = rng.standard_normal((d, m, m))
    gk = 0.5 * (gk + gk.transpose(0, 2, 1)) if 'gk' in mods else np.zeros((d, m, m))
    beta = np.exp(0.2 * rng.standard_normal(d)) * 2.0                   # (the split step's forward half only)
    for mod in mods:
        if mod == 'g2zero':
            g2[1] = 0.0
        elif mod == 'gvzero':
            gv[1] = 0.0
        elif mod == 'yzero':
            y[:, 1] = 0.0
        elif mod == 'tinygamma':
            gamma[:, ::2] = 1e-6
        elif mod == 'ynan':
            y[5, 2] = np.nan
        elif 'pow' in mod:                                              # <g2 | gv | y>pow<k>: that tensor's largest entry per output dim = 2^k
            what, k = mod.split('pow')[0], int(mod.split('pow')[1])
            alpha[:] = 1.0
            if what == 'g2':
                # u_dp = fold g2 alpha^2 exp(-1/4 sum_q gamma (z_m - z_m')^2) with fold = 2 off the diagonal (pg_u_kernel): off-diagonal
                # entries at HALF the smooth form's, so that every folded one stays below the diagonal's 2^k exp(0) = 2^k exactly
                g2 = sign[:, None, None] * 2.0 ** k * (np.exp(-0.1 * dist) * (0.5 + 0.5 * np.eye(m)))[None]
                gv = gv * 2.0 ** k
            elif what == 'gv':
                gv = gv / np.abs(gv).max(axis=1, keepdims=True) * 2.0 ** k
                g2 = g2 * 2.0 ** k
            else:
                y = y / np.abs(y).max(axis=0, keepdims=True) * 2.0 ** k
                g2 = g2 * 2.0 ** k
            # (the other term follows by 2^k — its own maximum is no power of two —, so that the Psi2 and the Psi1 term both stay visible
            # in the sums at k = -20 and 20: a wrong kap, kap1 or ky then shows at the tolerance)
        elif mod != 'gk':
            raise ValueError(mod)
    return dict(z=z, mu=mu, s=s, gamma=gamma, alpha=alpha, g2=g2, gv=gv, y=y, gk=gk, beta=beta)


def stage_b_reference(z, mu, s, gamma, alpha, y, g2, gk, gv, jitter=JITTER):
    """dL / d(mu, S, z, gamma) by fp64 autograd (NumPy in / out; g2 [D,M,M] symmetric, gk [D,M,M], gv [D,M]), and K - jitter I."""
    f64 = torch.float64
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=f64)
    n, q = mu.shape
    m, d = z.shape[0], gamma.shape[0]
    zt, gt, al = t(z).requires_grad_(True), t(gamma).requires_grad_(True), t(alpha)
    ii, jj = np.tril_indices(m)
    g2f = t(g2[:, ii, jj] * np.where(ii == jj, 1.0, 2.0)[None])                    # the adjoint folded onto the pairs m' <= m
    gvt = t(gv)
    ii, jj = torch.as_tensor(ii), torch.as_tensor(jj)
    dmu, ds = np.zeros((n, q)), np.zeros((n, q))
    # K_uu (rbf_kernel.py:58-93; ot.psi_pieces without the constant jitter I)
    zd = zt[:, None, :] - zt[None, :, :]
    k_uu = al[:, None, None] * torch.exp(-0.5 * torch.einsum('dq,ijq->dij', gt, zd * zd))
    a, b = torch.autograd.grad(torch.sum(t(gk) * k_uu), [zt, gt])
    dz, dg = a.numpy().copy(), b.numpy().copy()
    chunk = max(1, min(n, 4000000 // (d * ii.numel())))
    for n0 in range(0, n, chunk):
        mu_c, s_c = t(mu[n0:n0 + chunk]).requires_grad_(True), t(s[n0:n0 + chunk]).requires_grad_(True)
        y_c = t(y[n0:n0 + chunk])
        # Psi2 (rbf_kernel.py:164-199) over the pairs: sum_q w (mu - zbar)^2 = sum w mu^2 - 2 (w mu) . zbar + w . zbar^2
        zbar, zdp = 0.5 * (zt[ii] + zt[jj]), zt[ii] - zt[jj]
        den2 = 2.0 * gt[:, None, :] * s_c[None] + 1.0                               # [D,c,Q]
        w = gt[:, None, :] / den2
        e2 = torch.sum(w * mu_c * mu_c, dim=-1)[:, :, None] - 2.0 * (w * mu_c) @ zbar.T + w @ (zbar * zbar).T
        lp = 2.0 * torch.log(al)[:, None, None] - (0.5 * torch.sum(torch.log(den2), dim=-1)[:, :, None]
                                                   + 0.25 * (gt @ (zdp * zdp).T)[:, None, :] + e2)
        loss = torch.sum(g2f * torch.sum(torch.exp(lp), dim=1))
        # Psi1^T y (rbf_kernel.py:135-161 contracted with y)
        den1 = gt[:, None, :] * s_c[None] + 1.0
        w1 = gt[:, None, :] / den1
        e1 = torch.sum(w1 * mu_c * mu_c, dim=-1)[:, :, None] - 2.0 * (w1 * mu_c) @ zt.T + w1 @ (zt * zt).T \
            + torch.sum(torch.log(den1), dim=-1)[:, :, None]
        p1 = al[:, None, None] * torch.exp(-0.5 * e1)                               # [D,c,M]
        loss = loss + torch.sum(gvt * torch.einsum('dcm,cd->dm', p1, y_c))
        a, b, e, f = torch.autograd.grad(loss, [mu_c, s_c, zt, gt])
        dmu[n0:n0 + chunk], ds[n0:n0 + chunk] = a.numpy(), b.numpy()
        dz += e.numpy()
        dg += f.numpy()
    return (dmu, ds, dz, dg), k_uu.detach().numpy()


@functools.lru_cache(maxsize=None)
def reference(c):
    """(problem, K - jitter I, (d mu, d S, d z, d gamma)) of a case; computed once, shared, never modified."""
    p = problem(c)
    want, k_scaled = stage_b_reference(p['z'], p['mu'], p['s'], p['gamma'], p['alpha'], p['y'], p['g2'], p['gk'], p['gv'])
    for a in want + (k_scaled,) + tuple(p.values()):
        a.setflags(write=False)
    return p, k_scaled, want


def tail_visibility(c, want):
    """Largest |entry| / column maximum over the columns of: the last observation (d mu, d S), the last inducing point (d z), the
    last output dim (d gamma)."""
    dmu, ds, dz, dg = want
    frac = lambda g: float((np.abs(g[-1]) / np.abs(g).max(axis=0)).max())
    return {'observation': max(frac(dmu), frac(ds)), 'inducing point': frac(dz), 'output dim': frac(dg)}


# ---------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------

def m_at_most(r):
    """The largest M with at most r pair tiles."""
    m = 1
    while pair_tiles(m + 1) <= r:
        m += 1
    return m


def m_at_least(r):
    """The smallest M with at least r pair tiles."""
    m = 1
    while pair_tiles(m) < r:
        m += 1
    return m


G_ENV = lambda g: (('DPGP_PG_G', str(g)),)

KSTEP_CASES = [(case(3, 70, 17, q), prec, ()) for q in (1, 5, 6, 10, 11, 15, 16, 20, 21) for prec in ('mixed', 'mixed_fast')] \
    + [(case(3, 37, 65, 22), 'mixed', ())]

GROUP_VARIANTS = [(2, 3, 2), (2, 3, 3), (2, 3, 4), (4, 7, 2), (4, 7, 3), (4, 7, 4), (6, 12, 2), (8, 17, 1), (8, 17, 2)]   # (KS, Q, G)
GROUP_CASES = [(case(2, n, m_at_most(c), q), 'mixed', G_ENV(g))
               for ks, q, g in GROUP_VARIANTS for c, n in ((1, 31), (8 * g, 32 * 8 * g), (8 * g + 1, 32 * 8 * g + 1))]
NATURAL_CASES = [(case(129, 513, 32, 3), 'mixed', ()), (case(129, 769, 39, 7), 'mixed', ()), (case(129, 257, 23, 16), 'mixed', ())]
NATURAL_PICKS_256 = [(2, 3, 17), (4, 4, 25), (8, 2, 9)]                  # (KS, G, column tiles of both Psi2 passes) on 256 compute units

RING_Q = {2: 4, 4: 8, 6: 13, 8: 18}
RING_CASES = []
for _ks, _q in RING_Q.items():
    _ntb = NTB_DEFAULT[_ks]
    _envs = [(), G_ENV(4)] if _ks <= 4 else [(), G_ENV(2)] if _ks == 8 else [()]
    for _r in (1, _ntb, _ntb + 1, 2 * _ntb + 1, 3 * _ntb, 3 * _ntb + 1, 4 * _ntb + 1):
        for _c in (case(2, 32 * _r, m_at_most(_r), _q), case(2, 32 * (_r - 1) + 1, m_at_least(_r), _q)):
            RING_CASES += [(_c, 'mixed', _e) for _e in _envs]
MROW_CASES = [(case(2, 40, 97, 16), 'mixed', ()), (case(2, 40, 289, 16), 'mixed', ())] \
    + [(case(2, 40, m, q), 'mixed', (('DPGP_PG_NTB', str(ntb)),)) for q in (4, 8, 13) for ntb in (1, 2) for m in (32, 33, 65, 97, 200)]

DIM_CASES = [(case(d, 33, 17, 3), 'mixed', ()) for d in (1, 2, 9, 16, 17, 64, 65, 257, 513)] + [(case(65, 33, 17, 16), 'mixed', ())]

SCALE_SHAPE = (4, 70, 20, 4)
SCALE_MODS = ['g2zero', 'gvzero', 'yzero', 'tinygamma'] + ['%spow%d' % (w, k) for w in ('g2', 'gv', 'y') for k in (-20, 0, 20)]
SCALE_CASES = [(case(*SCALE_SHAPE, mod), 'mixed', ()) for mod in SCALE_MODS]
NAN_CASE = case(*SCALE_SHAPE, 'ynan')

SPLIT_CASES = [case(3, 70, 40, 4, 'gk'), case(2, 40, 257, 16, 'gk'), case(2, 40, 40, 21, 'gk')]

AUTOGRAD_CASES = KSTEP_CASES + GROUP_CASES + NATURAL_CASES + RING_CASES + MROW_CASES + DIM_CASES + SCALE_CASES
ALL_CASES = sorted(set(c for c, _, _ in AUTOGRAD_CASES) | set(SPLIT_CASES))    # every case with a reference (not NAN_CASE)

_ids = lambda cases: ['%s-%s-%s' % (case_id(c), prec, env_id(env)) for c, prec, env in cases]


# ---------------------------------------------------------------------------------------------------------------
# the call
# ---------------------------------------------------------------------------------------------------------------

def set_switches(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)


def call_stage_b(dev, c, prec, k_scaled=None, p=None):
    """dpgp_elbo_grad_psi_ex on the case's inputs: exact NaN-filled workspace + guard band, NaN-filled outputs.  Returns the four
    gradients as NumPy arrays (the guard band is checked here, finiteness by the caller)."""
    if p is None:
        p, k_scaled, _ = reference(c)
    d, n, m, q = c.d, c.n, c.m, c.q
    mp = 16 * ceil_div(m, 16)
    f64 = torch.float64
    t = lambda a: torch.as_tensor(np.array(a), dtype=f64, device=dev)     # (a copy: the memoised arrays are read-only)
    pad2 = lambda a: np.pad(a, ((0, 0), (0, mp - m), (0, mp - m)))
    z, mu, s, gamma, alpha, y = (t(p[k]) for k in ('z', 'mu', 's', 'gamma', 'alpha', 'y'))
    g_psi2, w_kuu, g_v = t(pad2(p['g2'])), t(pad2(p['gk'] * k_scaled)), t(np.pad(p['gv'], ((0, 0), (0, mp - m))))
    l = _lib.lib()
    wsb = int(l.dpgp_elbo_grad_psi_workspace_bytes_ex(d, n, m, q, _lib.PREC[prec]))
    assert wsb > 0
    buf = torch.empty(wsb + GUARD_BYTES, dtype=torch.uint8, device=dev)
    buf[:wsb] = 0xFF                                                     # (all-ones: NaN as f16, fp32 and fp64)
    buf[wsb:] = GUARD_BYTE
    out = [torch.full(shape, float('nan'), dtype=f64, device=dev) for shape in ((n, q), (n, q), (m, q), (d, q))]
    _lib.check(l.dpgp_elbo_grad_psi_ex(d, n, m, q, y.data_ptr(), y.stride(0), z.data_ptr(), mu.data_ptr(), s.data_ptr(),
                                       gamma.data_ptr(), alpha.data_ptr(), g_psi2.data_ptr(), w_kuu.data_ptr(), g_v.data_ptr(), None,
                                       _lib.PREC[prec], buf.data_ptr(), wsb, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                       out[3].data_ptr(), ops._stream()), 'dpgp_elbo_grad_psi_ex')
    torch.cuda.synchronize()
    assert bool((buf[wsb:] == GUARD_BYTE).all()), 'the guard band behind the workspace was written (%s)' % case_id(c)
    return [o.cpu().numpy() for o in out]


_RESULTS = {}                                 # (case, prec) -> {env: gradients}: the differences between forced variants are logged


def run_case(dev, c, prec, env, monkeypatch, record_property):
    set_switches(monkeypatch, env)
    _, _, want = reference(c)
    got = call_stage_b(dev, c, prec)
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    record_property('passes', '; '.join('%s: KS %d G %d WLO %d rows %d cols %d NTb %d' % ps for ps in passes(c, prec, env, ncu)))
    for name, g in zip(NAMES, got):
        assert np.isfinite(g).all(), '%s: non-finite entries (%s, %s, %s)' % (name, case_id(c), prec, env_id(env))
    errs = []                                  # every figure before any is judged
    for name, g, w in zip(NAMES, got, want):
        scale = np.abs(w).max(axis=0)
        errs.append(float((np.abs(g - w).max(axis=0) / np.where(scale > 0, scale, 1.0)).max()))
    record_property('col_rel_err', ' '.join('%s %.2e' % kv for kv in zip(NAMES, errs)))
    print('%s %s %s:' % (case_id(c), prec, env_id(env)), ' '.join('%s %.2e' % kv for kv in zip(NAMES, errs)))
    others = _RESULTS.setdefault((c, prec), {})
    diffs = [float(np.abs(g - o).max() / max(np.abs(w).max(), 1e-300)) for e, other in others.items() if e != env
             for g, o, w in zip(got, other, want)]
    if diffs:
        record_property('max_diff_to_other_variants', max(diffs))
    others[env] = got
    worst = 0.0
    for name, g, w in zip(NAMES, got, want):
        worst = max(worst, check_cols(g, w, TOL[prec], '%s (%s, %s, %s)' % (name, case_id(c), prec, env_id(env))))
    record_property('max_col_rel_err', worst)


# ---------------------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------------------

def test_case_table_reaches_every_variant(dev, record_property):
    """Every (KS, G) instance of pg_pass_kernel is reached by the case table on this device, in pass 1 (rows = observations) and in
    pass 2 (rows = pairs) of the Psi2 term — by the cost rule's own pick or by DPGP_PG_G."""
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    seen = {'psi2 pass 1': set(), 'psi2 pass 2': set(), 'psi1 pass 1': set(), 'psi1 pass 2': set()}
    natural = set()
    for c, prec, env in AUTOGRAD_CASES:
        for name, ks, g, wlo, rows, cols, ntb in passes(c, prec, env, ncu):
            seen[name].add((ks, g))
            if not env:
                natural.add((name, ks, g))
    record_property('compute_units', ncu)
    record_property('natural_picks', str(sorted(natural)))
    for name in ('psi2 pass 1', 'psi2 pass 2'):
        missing = [v for v in VARIANTS if v not in seen[name]]
        assert not missing, '%s: (KS, G) never reached on %d compute units: %s' % (name, ncu, missing)
    # KS = 8 over at least 7 row tiles (three chunks and more): G = 1 takes the register-staged fills there, G = 2 the one register set
    long_ks8 = set(g for c, prec, env in AUTOGRAD_CASES for name, ks, g, wlo, rows, cols, ntb in passes(c, prec, env, ncu)
                   if ks == 8 and rows >= 7)
    assert long_ks8 == {1, 2}, long_ks8


@pytest.mark.parametrize('c,prec,env', KSTEP_CASES, ids=_ids(KSTEP_CASES))
def test_ksteps_and_feature_blocks(dev, c, prec, env, monkeypatch, record_property):
    """Family 1.  Q = 21 with the rank-1 Psi1 term could not pass before PG_QP_SWITCH had its QP = 24 arm: pg_finish_m1_kernel<64, 20>
    summed the latent dims q < 20 and added red[w][40 .. 41] — another wave's partial sums of q = 0 — into dz[:, 20]."""
    run_case(dev, c, prec, env, monkeypatch, record_property)


@pytest.mark.parametrize('c,prec,env', GROUP_CASES + NATURAL_CASES, ids=_ids(GROUP_CASES + NATURAL_CASES))
def test_column_groups(dev, c, prec, env, monkeypatch, record_property):
    """Family 2: every G with 1, 8 G and 8 G + 1 column tiles (the last group's surplus tiles repeat the last one and are not stored)."""
    run_case(dev, c, prec, env, monkeypatch, record_property)


@pytest.mark.parametrize('c,prec,env', RING_CASES + MROW_CASES, ids=_ids(RING_CASES + MROW_CASES))
def test_ring_chunk_boundaries(dev, c, prec, env, monkeypatch, record_property):
    """Family 3: row tile counts on and around the chunk boundaries of the LDS ring, for each of the three kinds of rows."""
    run_case(dev, c, prec, env, monkeypatch, record_property)


@pytest.mark.parametrize('c,prec,env', DIM_CASES, ids=_ids(DIM_CASES))
def test_output_dim_chunks(dev, c, prec, env, monkeypatch, record_property):
    """Family 4: the output-dim chunks of pg_finish_pairs_kernel (16 chunks, 32 dims per LDS trip), pg_finish_obs_kernel (64 chunks,
    8 per trip) and pg_finish_m1_kernel (threads stride D by 256)."""
    run_case(dev, c, prec, env, monkeypatch, record_property)


@pytest.mark.parametrize('c,prec,env', SCALE_CASES, ids=_ids(SCALE_CASES))
def test_scale_factor_edges(dev, c, prec, env, monkeypatch, record_property):
    """Family 5: kap, kap1, ky and kg (powers of two from frexp) at an all-zero adjoint, an all-zero y column, maxima that are exact
    powers of two, and gamma = 1e-6 (those columns are held to their own largest entry, as every column is)."""
    run_case(dev, c, prec, env, monkeypatch, record_property)


def test_nan_in_y_poisons_the_outputs(dev, monkeypatch):
    """One NaN in y: pg_ky_kernel's fmax drops it, the image kernel flags it, pg_poison_kernel writes NaN into all four outputs."""
    set_switches(monkeypatch, ())
    p = problem(NAN_CASE)
    got = call_stage_b(dev, NAN_CASE, 'mixed', k_scaled=np.zeros((NAN_CASE.d, NAN_CASE.m, NAN_CASE.m)), p=p)
    for name, g in zip(NAMES, got):
        assert np.isnan(g).any(), '%s carries no NaN' % name


@pytest.mark.parametrize('c', SPLIT_CASES, ids=case_id)
def test_split_training_step(dev, c, monkeypatch, record_property):
    """Family 6: dpgp_elbo_fhat_step, then dpgp_elbo_grad_psi_step on this file's own adjoints — the only way the step runs for
    M > 128, and the only caller of pg_u_scale_kernel without z in LDS (M Q > 4096)."""
    set_switches(monkeypatch, ())
    p, k_scaled, want = reference(c)
    d, n, m, q = c.d, c.n, c.m, c.q
    mp = 16 * ceil_div(m, 16)
    t = lambda a: torch.as_tensor(np.array(a), dtype=torch.float64, device=dev)
    pad2 = lambda a: np.pad(a, ((0, 0), (0, mp - m), (0, mp - m)))
    args = [t(p[k]) for k in ('y', 'z', 'mu', 's', 'gamma', 'alpha', 'beta')]
    g_psi2, w_kuu, g_v = t(pad2(p['g2'])), t(pad2(p['gk'] * k_scaled)), t(np.pad(p['gv'], ((0, 0), (0, mp - m))))
    w64 = ops.ElboWorkspace(d, n, m, q, 'f64', dev)
    terms64, _, info64 = ops.elbo_fhat(*args, prec='f64', workspace=w64)
    assert int(info64.abs().max()) == 0, 'the fp64 evaluation flags an output dim: %s' % info64.tolist()
    terms64 = terms64.cpu().numpy()
    w, b = ops.ElboWorkspace(d, n, m, q, 'mixed', dev), ops.ElboStepBuffers(d, n, m, q, dev)
    for rep in range(2):                                                 # (twice: the buffers are reused by every step)
        terms, _, info = ops.elbo_fhat_step(*args, workspace=w, buffers=b)
        got = ops.elbo_grad_psi_step(*args[:6], g_psi2, w_kuu, g_v, workspace=w, buffers=b)
        terms, got = terms.cpu().numpy(), [g.cpu().numpy() for g in got]
        terr = float(np.abs(terms - terms64).max() / np.abs(terms64).max())
        record_property('terms_rel_err_%d' % rep, terr)
        print('%s rep %d: terms %.2e' % (case_id(c), rep, terr))
        assert np.isfinite(terms).all()
        np.testing.assert_allclose(terms, terms64, rtol=0, atol=TERM_TOL * np.abs(terms64).max())
        worst = 0.0
        for name, g, wnt in zip(NAMES, got, want):
            worst = max(worst, check_cols(g, wnt, GRAD_TOL, '%s (%s, split step, call %d)' % (name, case_id(c), rep)))
        record_property('max_col_rel_err_%d' % rep, worst)

