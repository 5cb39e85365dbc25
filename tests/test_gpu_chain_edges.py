"""
The dense half of the fused ELBO at every tile count and launch form, against fp64 references of the same operation
(tests/test_chain_refs.py holds the recipes, references and comparators, and the CPU tests that show they can be trusted).

Forward chain (chain_k_body, chain_b_kernel, potrf_lds / potrf_blocked / potrf_plain; csrc/linalg.hip, csrc/linalg_dev.h) and stage A of the
backward pass (chain_grad_kernel, csrc/grad.hip; M > 128: csrc/chain_grad_big.hip and ops._elbo_grad_chain_large_composed).  The chain is
fp64 arithmetic on K_uu, the Psi2 slabs and the Psi1^T y slabs; the slabs are read back from the workspace (dpgp_elbo_workspace_layout), the
reference chain is evaluated on them, and so the mixed-precision instantiation (fp32 slabs, fp64 chain) is held to the fp64 tolerances:
    forward terms                     1e-9 x the largest |term| of the problem     (test_gpu_elbo.RTOL['f64'])
    g_psi2, w_kuu, g_v                1e-8 x the largest entry of that output     (test_gpu_grad.test_chain_adjoints)
    d_alpha, d_beta                   rtol 1e-8
The matrices are compared one 16 x 16 tile at a time over the lower triangle (a wrong tile is named), the rest of the lower tiles must be
exactly 0.0.  Families: F1 every tile count, F2 the LDS forms of an fp64 workspace, F3 the plain cross-check path, F4 slab sums, F5 the
conditioning guard (inside F1 / F2), F6 the fp32 chain, F7 failure reporting; A1 every tile count, A2 jitter, A3 slabs, A4 M > 128,
A5 reproducibility.  Every test prints its largest error as a fraction of its tolerance.
"""
import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import ops
from oracle import dpgp_oracle as orc
import test_chain_refs as R

pytestmark = pytest.mark.gpu
PRECS = ['f64', 'mixed']
GUARD_REL = 2.0e-3                                               # DPGP_GUARD_REL, include/dpgp.h
ILL_CONDITIONED = -2                                             # DPGP_INFO_ILL_CONDITIONED
NAMES = ('y', 'z', 'mu', 's', 'gamma', 'alpha', 'beta')


def on_device(dev, p, **changed):
    q = dict(p, **changed)
    return [torch.as_tensor(np.array(q[k], dtype=np.float64), device=dev) for k in NAMES]     # (copies: the cases are read-only)


def forward(dev, p, prec, algo='auto', **changed):
    """One ops.elbo_fhat on a workspace of its own: (workspace, device arguments, terms, sums, info) — the last three as NumPy copies."""
    args = on_device(dev, p, **changed)
    (n, d), (m, q) = p['y'].shape, p['z'].shape
    w = ops.ElboWorkspace(d, n, m, q, prec, dev)
    terms, sums, info = ops.elbo_fhat(*args, jitter=p['jitter'], prec=prec, algo=algo, workspace=w)
    torch.cuda.synchronize()
    return w, args, terms.cpu().numpy().copy(), sums.cpu().numpy().copy(), info.cpu().numpy().copy()


def own_pieces(w, p, psi2_slabs=None, **changed):
    """K_uu (CPU oracle formula with the case's jitter) and what the evaluation left in its workspace: Psi2 = the slabs (fp32 or fp64 lower
    patches) summed in fp64 and symmetrised from the lower triangle, Psi1^T y and y^T y = their slabs summed."""
    q = dict(p, **changed)
    d, n, m, _ = w.shape
    off_p2, ns2, esz, mp, off_v, ns1, off_yy, nyy = w.layout[:8]
    ns2 = ns2 if psi2_slabs is None else psi2_slabs
    f64 = torch.float64
    slabs = w.ws[off_p2:off_p2 + esz * ns2 * d * mp * mp].view(torch.float32 if esz == 4 else f64).view(ns2, d, mp, mp)
    # (only the lower patches are written: whatever else the allocation holds is cut away before anything is converted or summed)
    low = torch.tril(slabs[:, :, :m, :m]).cpu().numpy().astype(np.float64).sum(axis=0)
    p2 = low + np.tril(low, -1).transpose(0, 2, 1)
    v = w.ws[off_v:off_v + 8 * ns1 * d * m].view(f64).view(ns1, d, m).cpu().numpy().sum(axis=0)
    yy = w.ws[off_yy:off_yy + 8 * nyy * d].view(f64).view(nyy, d).cpu().numpy().sum(axis=0)
    k_uu = orc.ard_rbf_gram(q['z'], None, q['gamma'], q['alpha'], q['beta'], include_noise=False, include_jitter=True, jitter=p['jitter'])
    return k_uu, p2, v, q['alpha'], q['beta'], yy, n


def report(family, what, **ratios):
    print('chain-edges %s %s: %s' % (family, what, ' '.join('%s=%.3g' % kv for kv in ratios.items())))


def check_forward(dev, key, prec, family, algo='auto', guard=False):
    """Terms against the chain on the evaluation's own pieces (and, fp64, against the full oracle), f_hat = their sum, info, guard."""
    p = R.case(*key)
    w, _, terms, sums, info = forward(dev, p, prec, algo)
    own = own_pieces(w, p)
    what = '%s M=%d N=%d %s %s' % (key[0], key[1], own[6], prec, algo)
    ratios = dict(own=R.terms_close(terms, R.chain_terms(*own), R.TERM_TOL, what + ' (own pieces)'))
    if prec == 'f64':
        ratios['oracle'] = R.terms_close(terms, R.oracle_terms(*key), R.TERM_TOL, what + ' (oracle)')
        assert not info.any(), (what, info)
    np.testing.assert_allclose(sums[0], terms.sum(), rtol=1e-12, err_msg=what)
    assert np.isin(info, (0, ILL_CONDITIONED)).all(), (what, info)
    if guard:
        got, want = w.guard.cpu().numpy(), R.guard_bound(*own[:3], own[4])
        np.testing.assert_allclose(got, want, rtol=1e-6, err_msg=what + ': guard')
        ratios['guard'] = float(np.abs(got / want - 1.0).max() / 1e-6)
        if prec == 'mixed':
            for d, b in enumerate(want):
                if abs(b / (GUARD_REL * own[6]) - 1.0) > 0.01:
                    assert (info[d] == ILL_CONDITIONED) == (b > GUARD_REL * own[6]), (what, d, b, info[d])
    report(family, what, **ratios)
    return w


# --------------------------------------------------------------------------------------------------------------------
# forward chain
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('m', R.TILE_COUNT_MS)
def test_forward_at_every_tile_count(dev, m, prec):
    """F1 (+ F5): nb = 1 ... 8 tile rows, M = 16 nb - 15, 16 nb - 1, 16 nb."""
    check_forward(dev, ('dense', m, None), prec, 'F1', guard=True)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('m', R.LDS_FORM_MS)
def test_forward_lds_forms_of_an_fp64_workspace(dev, m, prec):
    """F2 (+ F5): K_uu leaves LDS at M = 129; B in LDS with one workgroup per compute unit to M = 176, in global memory from 177."""
    check_forward(dev, ('dense', m, None), prec, 'F2', guard=True)


@pytest.mark.parametrize('m', R.PLAIN_MS)
def test_forward_plain_cross_check_path(dev, m):
    """F3: algo = 'plain' (potrf_plain, chain_k as a launch of its own)."""
    check_forward(dev, ('dense', m, None), 'f64', 'F3', algo='plain')


def set_splits(monkeypatch, ns2, ns1):
    monkeypatch.setenv('DPGP_PSI2_NS', str(ns2))
    monkeypatch.setenv('DPGP_PSI1_NS', str(ns1))


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('ns1', [1, 3])
@pytest.mark.parametrize('ns2', [2, 8])
@pytest.mark.parametrize('m', R.SLAB_MS)
def test_forward_slab_sums(dev, m, ns2, ns1, prec, monkeypatch):
    """F4: the sums over the Psi2 and Psi1^T y slabs (mixed: the loader with two passes in flight; fp64: the generic one)."""
    set_splits(monkeypatch, ns2, ns1)
    w = check_forward(dev, ('dense', m, R.SLAB_N), prec, 'F4 ns2=%d ns1=%d' % (ns2, ns1))
    assert (w.layout[1], w.layout[5]) == (ns2, ns1), 'the split counts were not taken'


@pytest.mark.parametrize('m', R.F32_MS)
def test_forward_fp32_chain(dev, m):
    """F6: prec = 'f32' (fp32 workspace: K_uu LDS-resident to M = 176; B two per compute unit to 176, one to 256, global memory from 257),
    jitter 1e-2, against the fp64 chain on the evaluation's own pieces.  Bound: max(5e-4, 4 x the deviation of the same chain run in
    float32 on the CPU), both relative to the largest term.  Measured on the MI355X (GPU / CPU float32 deviation):
    M = 128: 9.1e-6 / 3.4e-6, 176: 1.1e-5 / 4.3e-6, 177: 5.7e-6 / 9.5e-6, 192: 4.8e-6 / 2.2e-6, 256: 1.2e-5 / 2.2e-5, 257: 1.5e-5 / 6.4e-6:
    the 5e-4 governs everywhere."""
    key = ('jittered_f32', m, None)
    p = R.case(*key)
    w, _, terms, sums, info = forward(dev, p, 'f32')
    own = own_pieces(w, p)
    assert w.layout[2] == 4
    want = R.chain_terms(*own)
    top = np.abs(want).max()
    dev_cpu = float(np.abs(R.chain_terms_f32(*own) - want).max() / top)
    dev_gpu = float(np.abs(terms - want).max() / top)
    bound = max(5e-4, 4.0 * dev_cpu)
    print('chain-edges F6 M=%d: gpu=%.3g cpu_float32=%.3g bound=%.3g ratio=%.3g' % (m, dev_gpu, dev_cpu, bound, dev_gpu / bound))
    assert np.isin(info, (0, ILL_CONDITIONED)).all(), info
    assert np.isfinite(terms).all() and dev_gpu <= bound
    np.testing.assert_allclose(sums[0], terms.sum(), rtol=1e-12)


@pytest.mark.parametrize('m,algo', [(m, 'auto') for m in R.FAIL_MS] + [(R.FAIL_MS[0], 'plain')])
def test_failures_are_reported_in_every_form(dev, m, algo):
    """F7: numerical failure flags of the LDS-resident, one-per-compute-unit, global-memory and plain forms (fp64)."""
    p = R.case('dense', m, None)
    clean = forward(dev, p, 'f64', algo)[2]
    bad = 1
    others = np.arange(len(p['beta'])) != bad
    beta = np.array(p['beta'])
    beta[bad] = -500.0                                           # B = K - 500 Psi2 is indefinite for this output dim only
    _, _, terms, _, info = forward(dev, p, 'f64', algo, beta=beta)
    assert info[bad] > m and not info[others].any(), info
    assert np.isnan(terms[bad, [1, 2, 4]]).all()
    np.testing.assert_array_equal(terms[others], clean[others])
    alpha = np.array(p['alpha'])
    alpha[bad] = -1.0                                            # K_uu itself is not positive definite
    _, _, terms, _, info = forward(dev, p, 'f64', algo, alpha=alpha)
    assert 0 < info[bad] <= m and not info[others].any(), info
    assert np.isfinite(terms[others]).all()
    np.testing.assert_allclose(terms[others], clean[others], rtol=1e-12, atol=0)


# --------------------------------------------------------------------------------------------------------------------
# stage A
# --------------------------------------------------------------------------------------------------------------------
def compare_adjoints(got, want, m, what, padding):
    gp, wk, gv, dab, info = (a.cpu().numpy() for a in got)
    assert not info.any(), (what, info)
    if not padding:
        gp, wk = gp[:, :m, :m], wk[:, :m, :m]
    ratios = dict(g_psi2=R.tiles_close(gp, want['g_psi2'], m, R.ADJ_TOL, what + ': g_psi2', padding=padding),
                  w_kuu=R.tiles_close(wk, want['w_kuu'], m, R.ADJ_TOL, what + ': w_kuu', padding=padding),
                  g_v=R.vector_close(gv[:, :m], want['g_v'], R.ADJ_TOL, what + ': g_v'))
    assert (gv[:, m:] == 0.0).all(), what + ': g_v beyond M'
    for k, name in enumerate(('d_alpha', 'd_beta')):
        np.testing.assert_allclose(dab[:, k], want[name], rtol=1e-8, atol=0, err_msg=what + ': ' + name)
        ratios[name] = float(np.abs(dab[:, k] / want[name] - 1.0).max() / 1e-8)
    return ratios


def check_stage_a(dev, key, prec, family, with_oracle=True, step=False):
    """ops.elbo_grad_chain after ops.elbo_fhat (step: ops.elbo_fhat_step) on the same workspace, against autograd through the chain on the
    evaluation's own pieces (and, fp64, against the full oracle's chain_adjoints)."""
    p = R.case(*key)
    m = key[1]
    w, args, _, _, _ = forward(dev, p, prec)                     # (step: every Psi2 slab now holds a partial sum of an earlier evaluation)
    slabs = None
    if step:
        (n, d), q = p['y'].shape, p['z'].shape[1]
        buf = ops.ElboStepBuffers(d, n, m, q, dev)
        terms = ops.elbo_fhat_step(*args, w, buf, jitter=p['jitter'])[0]
        torch.cuda.synchronize()
        slabs = 1
    own = own_pieces(w, p, psi2_slabs=slabs)
    what = '%s M=%d N=%d %s%s' % (key[0], m, own[6], prec, ' after elbo_fhat_step' if step else '')
    if step:
        report(family, what, terms=R.terms_close(terms.cpu().numpy(), R.chain_terms(*own), R.TERM_TOL, what))
    big = m > 128
    got = ops.elbo_grad_chain(args[5], args[6], w, jitter=p['jitter'], z=args[1] if big else None, gamma=args[4] if big else None,
                              psi2_slabs=slabs)
    torch.cuda.synchronize()
    ratios = compare_adjoints(got, R.chain_adjoints_from_pieces(*own, p['jitter']), m, what + ' (own pieces)', padding=not big)
    if prec == 'f64' and with_oracle:
        ro = compare_adjoints(got, R.oracle(*key), m, what + ' (oracle)', padding=not big)
        ratios.update({'oracle_' + k: v for k, v in ro.items()})
    report(family, what, **ratios)
    return w, args, got


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('m', R.TILE_COUNT_MS)
def test_stage_a_at_every_tile_count(dev, m, prec):
    """A1: nb = 1 ... 8 — the wave-to-tile-row ownership of both passes of K^-1 P K^-1 changes with nb (odd nb: the middle wave owns one
    row twice over)."""
    check_stage_a(dev, ('dense', m, None), prec, 'A1')


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('m', R.JITTER_MS)
def test_stage_a_jitter(dev, m, prec):
    """A2: jitter = 1e-3 — the - jitter I in w_kuu = G_K .* (K_uu - jitter I) is 1e5 tolerances on the diagonal."""
    check_stage_a(dev, ('jittered', m, None), prec, 'A2')


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('ns1', [1, 3])
@pytest.mark.parametrize('ns2', [2, 8])
@pytest.mark.parametrize('m', R.SLAB_MS[:2])
def test_stage_a_slab_sums(dev, m, ns2, ns1, prec, monkeypatch):
    """A3: the slab sums of chain_grad_kernel."""
    set_splits(monkeypatch, ns2, ns1)
    w, _, _ = check_stage_a(dev, ('dense', m, R.SLAB_N), prec, 'A3 ns2=%d ns1=%d' % (ns2, ns1))
    assert (w.layout[1], w.layout[5]) == (ns2, ns1), 'the split counts were not taken'


@pytest.mark.parametrize('ns2', [2, 8])
@pytest.mark.parametrize('m', R.SLAB_MS[:2])
def test_stage_a_after_the_forward_half_of_a_step(dev, m, ns2, monkeypatch):
    """A3: after ops.elbo_fhat_step the workspace holds ONE Psi2 slab (psi2_slabs = 1), whatever the layout's count; the slabs behind it
    still hold an earlier evaluation's partial sums and must not be read."""
    set_splits(monkeypatch, ns2, 3)
    check_stage_a(dev, ('dense', m, R.SLAB_N), 'mixed', 'A3 step ns2=%d' % ns2, step=True)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('m,composed', [(m, False) for m in R.BIG_MS] + [(R.BIG_MS[-1], True)])
def test_stage_a_beyond_128_inducing_points(dev, m, composed, prec, monkeypatch):
    """A4: M = 129, 177, 200 composed from the batched operators; M = 256 dpgp_elbo_grad_chain_big, and composed (DPGP_STAGE_A_COMPOSED)."""
    if composed:
        monkeypatch.setenv('DPGP_STAGE_A_COMPOSED', '1')
    else:
        monkeypatch.delenv('DPGP_STAGE_A_COMPOSED', raising=False)
    check_stage_a(dev, ('dense', m, None), prec, 'A4 composed' if composed or m % 128 else 'A4 one call')


def same_bits(a, b, m, what):
    """Bit-identical, over what stage A writes (M <= 128: the lower tiles; above: everything)."""
    for name, x, y in zip(('g_psi2', 'w_kuu', 'g_v', 'd_alpha_beta', 'info'), a, b):
        x, y = x.cpu().numpy(), y.cpu().numpy()
        if x.ndim == 3 and m <= 128:
            i, j = np.meshgrid(np.arange(x.shape[1]), np.arange(x.shape[2]), indexing='ij')
            x, y = x[:, i // 16 >= j // 16], y[:, i // 16 >= j // 16]
        assert x.tobytes() == y.tobytes(), '%s: %s differs between two calls' % (what, name)


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('m', R.REPRO_MS)
def test_stage_a_is_reproducible_on_a_reused_workspace(dev, m, prec):
    """A5: two calls on one workspace, and a second forward + stage A round on it (stage A overwrites the Kb / Wb regions of the forward
    workspace: the forward has to rebuild them), give the same bits."""
    key = ('dense', m, None)
    p = R.case(*key)
    w, args, first = check_stage_a(dev, key, prec, 'A5', with_oracle=False)
    big = dict(z=args[1], gamma=args[4]) if m > 128 else {}
    chain = lambda: ops.elbo_grad_chain(args[5], args[6], w, jitter=p['jitter'], **big)
    same_bits(first, chain(), m, 'second call')
    terms0 = w.terms.cpu().numpy().copy()
    terms, _, _ = ops.elbo_fhat(*args, jitter=p['jitter'], prec=prec, workspace=w)
    assert terms.cpu().numpy().tobytes() == terms0.tobytes(), 'the forward terms differ on the reused workspace'
    same_bits(first, chain(), m, 'second round')
