"""
CPU checks of what tests/test_gpu_stage_b_edges.py judges the pair-tile stage B by: its fp64 autograd reference against the
oracle (ot.fhat_input_gradients on the stored gradient fixtures, ot.psi_pieces at an odd shape), the tail-visibility condition
for every case of its table, its Python mirror of pg_launch_pass's cost rule and of the ring size against hand-computed picks,
and the shape of the case table itself.
"""
import time

import numpy as np
import pytest
import torch

from oracle import dpgp_oracle_torch as ot
import test_gpu_grad
import test_gpu_stage_b_edges as B


@pytest.mark.parametrize('fixture', ['grad_ref_40_6_12_3_T4', 'grad_ref_60_10_15_4_T5'])
def test_reference_agrees_with_the_oracle_on_the_gradient_fixtures(fixture):
    """With the oracle's own stage-A adjoints (G2 = d f_hat / d Psi2, GK = d f_hat / d K_uu, gv = d f_hat / d Psi1^T y) the reference's
    four gradients are d f_hat / d (mu, S, z, gamma) of the oracle."""
    p = test_gpu_grad.point(fixture)
    args = [p[k] for k in ('y', 'z', 'mu', 's', 'gamma', 'alpha', 'beta')]
    adj = ot.chain_adjoints(*args)
    want = ot.fhat_input_gradients(*args)
    got, k_scaled = B.stage_b_reference(p['z'], p['mu'], p['s'], p['gamma'], p['alpha'], p['y'], adj['g_psi2'], adj['g_kuu'], adj['g_v'])
    for name, g, w in zip(B.NAMES, got, (want['d_mu'], want['d_s'], want['d_z'], want['d_gamma'])):
        np.testing.assert_allclose(g, w, rtol=0, atol=1e-11 * np.abs(w).max(), err_msg=name)
    m = p['z'].shape[0]
    np.testing.assert_allclose(k_scaled, adj['k_uu'] - B.JITTER * np.eye(m), rtol=1e-13, atol=0)


def test_reference_agrees_with_autograd_of_psi_pieces():
    """The expanded squares and the fold onto the pairs against the oracle's literal formulas, at a case of the table with GK != 0
    and more than one chunk of observations."""
    c = B.SPLIT_CASES[0]
    p, k_scaled, got = B.reference(c)
    assert B.reference(c)[2] is got, 'memoised'
    f64 = torch.float64
    t = lambda a: torch.as_tensor(np.array(a), dtype=f64)
    z, mu, s, gamma = (t(p[k]).requires_grad_(True) for k in ('z', 'mu', 's', 'gamma'))
    k_uu, p2, v = ot.psi_pieces(t(p['y']), z, mu, s, gamma, t(p['alpha']), jitter=B.JITTER, chunk=16)
    loss = torch.sum(t(p['g2']) * p2) + torch.sum(t(p['gv']) * v) + torch.sum(t(p['gk']) * k_uu)
    want = torch.autograd.grad(loss, [mu, s, z, gamma])
    for name, g, w in zip(B.NAMES, got, want):
        np.testing.assert_allclose(g, w.numpy(), rtol=0, atol=1e-11 * float(w.abs().max()), err_msg=name)


def test_inputs_are_what_the_cases_say():
    for k in (-20, 0, 20):
        # what kap's frexp sees (pg_u_kernel): u_dp = fold G2 alpha^2 exp(-1/4 sum_q gamma dz^2), fold = 2 off the diagonal; its largest
        # entry per output dim is exactly 2^k (the diagonal) and every off-diagonal pair is strictly below it
        p = B.problem(B.case(*B.SCALE_SHAPE, 'g2pow%d' % k))
        dz2 = (p['z'][:, None, :] - p['z'][None, :, :]) ** 2
        m = p['z'].shape[0]
        u = (2.0 - np.eye(m))[None] * p['g2'] * (p['alpha'] ** 2)[:, None, None] * np.exp(-0.25 * np.einsum('dq,ijq->dij', p['gamma'], dz2))
        assert (np.abs(u).max(axis=(1, 2)) == 2.0 ** k).all() and (p['alpha'] == 1.0).all()
        assert (np.abs(u.astype(np.float32)).max(axis=(1, 2)) == np.float32(2.0 ** k)).all()
        off = np.abs(u)[:, ~np.eye(m, dtype=bool)]
        assert off.max() < 0.999 * 2.0 ** k and off.max() > 0.25 * 2.0 ** k        # (below the diagonal, yet of its order)
    # in every power-of-two case the other term follows by 2^k: the Psi2 term alone (gv = 0) and the Psi1 term alone (G2 = 0) each carry
    # at least 1 % of the largest entry of d mu, d S and d z (each scale factor is undone in the finishing kernel of each of these; the Psi1
    # term's share of d gamma is naturally about 1 % and is not held to this).  A scale factor that is off by a binade moves its term by half or more: 5e-3 of the
    # largest entry, ten times the tolerance — neither kap nor kap1 / ky can be wrong unseen
    for mod in B.SCALE_MODS:
        if 'pow' in mod:
            c = B.case(*B.SCALE_SHAPE, mod)
            p, total = B.problem(c), B.reference(c)[2]
            for zeroed in ('gv', 'g2'):
                q = dict(p, **{zeroed: np.zeros_like(p[zeroed])})
                part = B.stage_b_reference(q['z'], q['mu'], q['s'], q['gamma'], q['alpha'], q['y'], q['g2'], q['gk'], q['gv'])[0]
                assert all(np.abs(a).max() >= 0.01 * np.abs(t).max() for a, t in zip(part[:3], total[:3])), (mod, zeroed)
    p = B.problem(B.case(*B.SCALE_SHAPE, 'gvpow20'))
    assert (np.abs(p['gv']).max(axis=1) == 2.0 ** 20).all() and (p['alpha'] == 1.0).all()
    p = B.problem(B.case(*B.SCALE_SHAPE, 'ypow0'))
    assert (np.abs(p['y']).max(axis=0) == 1.0).all()
    assert not B.problem(B.case(*B.SCALE_SHAPE, 'g2zero'))['g2'][1].any() and B.problem(B.case(*B.SCALE_SHAPE, 'g2zero'))['g2'][0].any()
    assert not B.problem(B.case(*B.SCALE_SHAPE, 'gvzero'))['gv'][1].any()
    assert not B.problem(B.case(*B.SCALE_SHAPE, 'yzero'))['y'][:, 1].any()
    assert (B.problem(B.case(*B.SCALE_SHAPE, 'tinygamma'))['gamma'][:, ::2] == 1e-6).all()
    assert np.isnan(B.problem(B.NAN_CASE)['y']).sum() == 1
    for c in B.ALL_CASES:
        p = B.problem(c)
        assert (p['g2'] == p['g2'].transpose(0, 2, 1)).all() and (p['gk'] == p['gk'].transpose(0, 2, 1)).all()
        assert p['gk'].any() == ('gk' in c.mod)
        for a in (p['y'], p['gv']):                                # mixed signs (an array of a handful of draws may have one)
            assert a.size < 16 or ((a > 0).any() and (a < 0).any())
        assert abs(np.abs(p['z']).max() / (4.0 if c.m > 128 else 2.0)) < 6.0


def test_tails_are_visible_in_every_case():
    """The last observation, inducing point and output dim carry at least 0.05 of their column's largest entry in one column of a
    gradient they appear in — in every case of the table, at the seed the table gives it.  Also times the references."""
    slowest = (0.0, None)
    for c in B.ALL_CASES:
        t0 = time.perf_counter()
        _, _, want = B.reference(c)
        slowest = max(slowest, (time.perf_counter() - t0, c))
        assert all(np.isfinite(w).all() for w in want)
        vis = B.tail_visibility(c, want)
        assert min(vis.values()) >= 0.05, (c, vis)
        # the bump rule: the smallest bump that passes, so bump > 0 only where every smaller one fails
        for b in range(c.bump):
            w_b = B.reference(c._replace(bump=b))[2]
            assert min(B.tail_visibility(c, w_b).values()) < 0.05, (c, b)
    print('slowest reference: %.2f s (%s); %d cases' % (slowest[0], B.case_id(slowest[1]), len(B.ALL_CASES)))


def test_cost_rule_mirror_against_hand_computed_picks():
    """pick_g(KS, D, column tiles, compute units): cost = ceil(D ceil(tiles / 8 G) / CUs) x G x permille (1000 / 945 / 940 for
    G = 2 / 3 / 4 at KS <= 4; 1000 / 920 for G = 1 / 2 at KS = 8), worked by hand."""
    hand = [
        # D = 129 on 256 CUs.  17 tiles: G = 2 -> 2 groups, 258 workgroups, 2 rounds x 2 x 1000 = 4000; G = 3 -> 1 group, 1 x 3 x 945 = 2835;
        # G = 4 -> 1 x 4 x 940 = 3760
        (2, 129, 17, 256, 3), (4, 129, 17, 256, 3),
        # 25 tiles: G = 2 -> 2 groups: 4000; G = 3 -> 2 groups, 2 rounds x 3 x 945 = 5670; G = 4 -> 1 group: 3760
        (2, 129, 25, 256, 4), (4, 129, 25, 256, 4),
        # KS = 8, 9 tiles: G = 1 -> 2 groups, 2 rounds x 1000 = 2000; G = 2 -> 1 group, 1 x 2 x 920 = 1840
        (8, 129, 9, 256, 2),
        # 8 tiles: one group either way: 1000 against 1840
        (8, 129, 8, 256, 1),
        # few output dims: one round whatever G: 2000 / 2835 / 3760, and 1000 / 1840
        (2, 2, 33, 256, 2), (4, 3, 1, 256, 2), (8, 2, 17, 256, 1),
        # D = 64, 63 observation tiles: G = 2 -> 4 groups, 256 workgroups, 1 round: 2000; G = 3 -> 2835; G = 4 -> 3760
        (4, 64, 63, 256, 2),
        # D = 512, 258 pair tiles: G = 2 -> 17 groups, 8704 workgroups, 34 rounds: 68000; G = 3 -> 11 groups, 5632, 22 rounds x 3 x 945 =
        # 62370; G = 4 -> 9 groups, 4608, 18 rounds x 4 x 940 = 67680
        (4, 512, 258, 256, 3),
        # KS = 8, D = 512, 63 tiles: G = 1 -> 8 groups, 4096 workgroups, 16 rounds: 16000; G = 2 -> 4 groups, 8 rounds x 2 x 920 = 14720
        (8, 512, 63, 256, 2),
        # another chip: 129 output dims on 128 CUs, 17 tiles: G = 2 -> 258, 3 rounds: 6000; G = 3 -> 129, 2 rounds x 3 x 945 = 5670;
        # G = 4 -> 2 rounds x 4 x 940 = 7520
        (2, 129, 17, 128, 3),
        # KS = 6 has one instance
        (6, 129, 17, 256, 2), (6, 2, 1, 256, 2),
    ]
    for ks, d, tiles, ncu, want in hand:
        assert B.pick_g(ks, d, tiles, ncu) == want, (ks, d, tiles, ncu)
    # the switches: DPGP_PG_G at KS <= 4 (2 / 3 / 4; anything else: 2) and at KS = 8 (1 / 2; anything else: the rule), DPGP_PG_G1 at KS = 8
    for g in (2, 3, 4):
        assert B.pick_g(2, 129, 17, 256, B.G_ENV(g)) == g and B.pick_g(4, 2, 1, 256, B.G_ENV(g)) == g
        assert B.pick_g(6, 2, 1, 256, B.G_ENV(g)) == 2
    assert B.pick_g(4, 129, 17, 256, B.G_ENV(1)) == 2
    assert B.pick_g(8, 2, 1, 256, B.G_ENV(2)) == 2 and B.pick_g(8, 129, 9, 256, B.G_ENV(1)) == 1
    assert B.pick_g(8, 129, 9, 256, B.G_ENV(3)) == 2 and B.pick_g(8, 129, 8, 256, B.G_ENV(4)) == 1
    assert B.pick_g(8, 129, 9, 256, (('DPGP_PG_G1', '1'),)) == 1
    # the ring: 160 KB / (3 x (KS + 4 | 6) KB), DPGP_PG_NTB only downwards and not below 2 at KS = 8
    assert [160 // (3 * (ks + (6 if ks == 8 else 4))) for ks in (2, 4, 6, 8)] == [8, 6, 5, 3] == [B.NTB_DEFAULT[ks] for ks in (2, 4, 6, 8)]
    ntb = lambda ks, v: B.ring_tiles(ks, (('DPGP_PG_NTB', str(v)),))
    assert [ntb(2, 1), ntb(2, 2), ntb(2, 8), ntb(2, 9), ntb(6, 1), ntb(8, 1), ntb(8, 2), ntb(8, 4)] == [1, 2, 8, 8, 1, 3, 2, 3]
    assert [B.ksteps(q) for q in (1, 5, 6, 10, 11, 15, 16, 20, 21)] == [2, 2, 4, 4, 6, 6, 8, 8, 8]
    assert B.pgrad_supported(17, 21) and not B.pgrad_supported(17, 22) and not B.pgrad_supported(4097, 3)
    assert [B.pair_tiles(m) for m in (1, 7, 8, 23, 32, 39, 44, 45)] == [1, 1, 2, 9, 17, 25, 31, 33]


def test_case_table_has_the_shapes_it_promises():
    """On 256 compute units: the natural picks, every (KS, G) in both Psi2 passes, the column tile counts 1 / 8 G / 8 G + 1 on both
    sides, the ring's row tile counts for each kind of rows."""
    ncu = 256
    for (c, prec, env), (ks, g, tiles) in zip(B.NATURAL_CASES, B.NATURAL_PICKS_256):
        ps = {name: rest for name, *rest in B.passes(c, prec, env, ncu)}
        assert not env and ps['psi2 pass 1'][:2] == [ks, g] and ps['psi2 pass 2'][:2] == [ks, g]
        assert ps['psi2 pass 1'][4] == tiles and ps['psi2 pass 2'][4] == tiles
    seen = {}
    for c, prec, env in B.AUTOGRAD_CASES:
        for name, ks, g, wlo, rows, cols, ntb in B.passes(c, prec, env, ncu):
            seen.setdefault((name, ks, g), []).append((rows, cols, ntb, wlo))
    for ks, g in B.VARIANTS:
        for name in ('psi2 pass 1', 'psi2 pass 2'):
            cols = set(v[1] for v in seen[(name, ks, g)])
            # (32 pair tiles do not exist: 31 and 33)
            want = {1, 8 * g + 1} | ({31, 33} if (8 * g == 32 and name == 'psi2 pass 1') else {8 * g})
            assert want <= cols, (name, ks, g, sorted(cols))
    assert any(not wlo for v in seen.values() for _, _, _, wlo in v)
    for ks, ntb in B.NTB_DEFAULT.items():
        edges = [1, ntb, ntb + 1, 2 * ntb + 1, 3 * ntb, 3 * ntb + 1, 4 * ntb + 1]
        for g in ([2, 4] if ks <= 4 else [1, 2] if ks == 8 else [2]):
            obs_rows = set(v[0] for v in seen[('psi2 pass 1', ks, g)] if v[2] == ntb)
            pair_rows = sorted(set(v[0] for v in seen[('psi2 pass 2', ks, g)] if v[2] == ntb))
            assert set(edges) <= obs_rows, (ks, g, sorted(obs_rows))
            for r in edges:                                        # r itself, or the nearest attainable count on each side of it
                assert r in pair_rows or (max(x for x in pair_rows if x < r) == B.pair_tiles(B.m_at_most(r))
                                          and min(x for x in pair_rows if x > r) == B.pair_tiles(B.m_at_least(r))), (ks, g, r, pair_rows)
    # inducing points as rows (the Psi1 back pass): naturally at KS = 8, under a shrunk ring elsewhere
    m_rows = set((ks, v[0], v[2]) for (name, ks, g), vs in seen.items() if name == 'psi1 pass 2' for v in vs)
    assert {(8, 4, 3), (8, 10, 3)} <= m_rows
    for ks in (2, 4, 6):
        for ntb in (1, 2):
            assert {(ks, r, ntb) for r in (1, 2, 3, 4, 7)} <= m_rows
    assert [c.d for c, _, _ in B.DIM_CASES] == [1, 2, 9, 16, 17, 64, 65, 257, 513, 65]
    assert all(B.pgrad_supported(c.m, c.q) for c in B.ALL_CASES if c.q != 22)
    assert len(set(B._ids(B.AUTOGRAD_CASES))) == len(B.AUTOGRAD_CASES)
    zl = lambda c: c.m * c.q * 8 <= 32 * 1024                      # pg_u_scale_kernel: z in LDS
    assert [zl(c) for c in B.SPLIT_CASES] == [True, False, True] and [c.q for c in B.SPLIT_CASES] == [4, 16, 21]
