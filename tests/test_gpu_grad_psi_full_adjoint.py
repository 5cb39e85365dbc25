"""GPU tests of stage B with a full adjoint of Psi1 (dpgp_elbo_grad_psi_ex with g_psi1 != NULL): the path of the over-T model and
its one-atom wrappers (bayesian_gp_lvm, manifold_relevance_determination), which reached it before only through the small reference
fixtures.  Against torch fp64 autograd of

    L = sum_d <G1_d, Psi1_d> + <G2_d, Psi2_d> + <GK_d, K_d>

with respect to (mu, S, z, gamma), Psi2 and K from the oracle's formulas (oracle/dpgp_oracle_torch.py:psi_pieces), alpha constant.
The inputs are laid out as _fhat_backward passes them: G2 and GK symmetric, w_kuu = GK .* (K - jitter I), g_psi2 / w_kuu
[D, Mp, Mp] and g_psi1 [D, N, Mp] zero-padded.  The shapes cross the kernels' branches: psi1_grad_z_kernel's 64 / 128 lanes
(Mp <= 64), its QP = 4 ... 32 instances, psi1_grad_n_kernel over more than one workgroup (N > 256), the M > 128 path, the pair-tile
limit of the Psi2 term (Q <= 21; the patch form above it and always for 'mixed_patch') and the LDS > 48 KB launches (M = 512, Q = 21).
Tolerance: the mixed stage-B tolerance, 5e-4 of each column's largest entry (tests/test_gpu_scales.py: GRAD_TOL, check_cols)."""
import functools

import numpy as np
import pytest
import torch

from dp_gp_lvm_amd import ops
from oracle import dpgp_oracle_torch as ot

pytestmark = pytest.mark.gpu
GRAD_TOL = 5e-4
JITTER = 1e-8

# (D, N, M, Q): D = 1 / 3 / 8; N = 1, 37, 256, 257, 700; M = 1, 16, 17, 64, 65, 128, 129, 200; Q = 1 ... 30 around the pair-tile limit
CASES = [(1, 37, 1, 1), (3, 1, 17, 4), (8, 37, 16, 5), (1, 256, 64, 4), (3, 257, 65, 5), (8, 700, 17, 13), (3, 256, 128, 13),
         (1, 257, 129, 20), (3, 700, 200, 5), (8, 257, 64, 21), (3, 37, 65, 22), (1, 700, 128, 30), (8, 256, 129, 4),
         (3, 257, 17, 20), (1, 37, 200, 13), (8, 1, 65, 30), (3, 700, 16, 1), (1, 257, 200, 22), (8, 37, 128, 1), (3, 256, 1, 21)]
LDS_CASE = (1, 300, 512, 21)          # psi1_grad_n_kernel / kuu_grad_kernel above 48 KB of LDS; G2 = 0 (the reference skips Psi2)
TINY_GAMMA_CASE = (3, 257, 65, 8)     # gamma = 1e-6 on every other latent dim


def _problem(case, tiny_gamma=False, zero_g2=False):
    d, n, m, q = case
    rng = np.random.default_rng(1000 * d + 7 * n + 3 * m + q)
    z = 2.0 * rng.standard_normal((m, q))
    mu = 1.5 * rng.standard_normal((n, q))
    s = np.exp(0.3 * rng.standard_normal((n, q)))
    gamma = np.exp(0.3 * rng.standard_normal((d, q))) * 2.0 / q          # (sum over q of gamma (mu - z)^2 of order ten)
    if tiny_gamma:
        gamma[:, ::2] = 1e-6
    alpha = np.exp(0.2 * rng.standard_normal(d))
    g1 = rng.standard_normal((d, n, m))                                  # mixed signs, and some all-zero rows
    g1[:, ::7, :] = 0.0
    dist = ((z[:, None, :] - z[None, :, :]) ** 2).sum(-1)
    sign = np.where(rng.random(d) < 0.5, -1.0, 1.0)
    g2 = (sign * (1.0 + 0.1 * rng.standard_normal(d)))[:, None, None] * np.exp(-0.1 * dist)[None]     # smooth, definite
    if zero_g2:
        g2[:] = 0.0
    gk = rng.standard_normal((d, m, m))
    gk = 0.5 * (gk + gk.transpose(0, 2, 1))
    return dict(z=z, mu=mu, s=s, gamma=gamma, alpha=alpha, g1=g1, g2=g2, gk=gk)


def _psi1(z, mu, s, gamma, alpha):
    """Psi1 [D, c, M] (rbf_kernel.py:135-161; the expression of ot.psi_pieces before its contraction with y)."""
    den1 = gamma[:, None, :] * s[None] + 1.0
    e1 = torch.einsum('cmq,dcq->dcm', (mu[:, None, :] - z[None]) ** 2, gamma[:, None, :] / den1) \
        + torch.sum(torch.log(den1), dim=-1)[:, :, None]
    return alpha[:, None, None] * torch.exp(-0.5 * e1)


@functools.lru_cache(maxsize=None)
def _reference(case, tiny_gamma=False, zero_g2=False):
    """dL/d(mu, S, z, gamma) by fp64 autograd, L summed over chunks of 64 observations (L is a sum over n of the Psi terms
    plus the K term), so that the taped graph holds one chunk at a time."""
    p = _problem(case, tiny_gamma, zero_g2)
    d, n, m, q = case
    f64 = torch.float64
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=f64)
    z, gamma, alpha = t(p['z']).requires_grad_(True), t(p['gamma']).requires_grad_(True), t(p['alpha'])
    g1, g2, gk = t(p['g1']), t(p['g2']), t(p['gk'])
    dmu, ds = np.zeros((n, q)), np.zeros((n, q))
    dz, dg = np.zeros((m, q)), np.zeros((d, q))
    none = torch.zeros((0, d), dtype=f64)
    k_uu, _, _ = ot.psi_pieces(none, z, t(p['mu'])[:0], t(p['s'])[:0], gamma, alpha, jitter=JITTER)
    a, b = torch.autograd.grad(torch.sum(gk * k_uu), [z, gamma])
    dz += a.numpy()
    dg += b.numpy()
    for n0 in range(0, n, 64):
        mu_c = t(p['mu'][n0:n0 + 64]).requires_grad_(True)
        s_c = t(p['s'][n0:n0 + 64]).requires_grad_(True)
        c = mu_c.shape[0]
        loss = torch.sum(g1[:, n0:n0 + c] * _psi1(z, mu_c, s_c, gamma, alpha))
        if not zero_g2:
            _, p2, _ = ot.psi_pieces(torch.zeros((c, d), dtype=f64), z, mu_c, s_c, gamma, alpha, jitter=JITTER)
            loss = loss + torch.sum(g2 * p2)
        a, b, e, f = torch.autograd.grad(loss, [mu_c, s_c, z, gamma])
        dmu[n0:n0 + c], ds[n0:n0 + c] = a.numpy(), b.numpy()
        dz += e.numpy()
        dg += f.numpy()
    with torch.no_grad():
        k_scaled = (k_uu - JITTER * torch.eye(m, dtype=f64)).numpy()
    return p, k_scaled, (dmu, ds, dz, dg)


def check_cols(got, want, tol, what):
    """|got - want| <= tol * max |want[:, j]| for every column j (a [N|M|D, Q] gradient: per latent dim); returns the largest
    error as a fraction of its column's largest entry."""
    got, want = np.asarray(got), np.asarray(want)
    assert np.isfinite(got).all(), '%s: non-finite entries' % what
    scale = np.abs(want).max(axis=0)
    err = np.abs(got - want).max(axis=0)
    bad = err > tol * scale
    assert not bad.any(), '%s: columns %s off by %s of their largest entry (tolerance %g)' % (
        what, np.flatnonzero(bad).tolist(), (err / np.where(scale > 0, scale, 1.0))[bad].tolist(), tol)
    return float((err / np.where(scale > 0, scale, 1.0)).max()) if err.size else 0.0


def _run(dev, case, prec, tiny_gamma=False, zero_g2=False):
    p, k_scaled, want = _reference(case, tiny_gamma, zero_g2)
    d, n, m, q = case
    mp = 16 * ((m + 15) // 16)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    pad2 = lambda a: np.pad(a, ((0, 0), (0, mp - m), (0, mp - m)))
    g_psi2, w_kuu = t(pad2(p['g2'])), t(pad2(p['gk'] * k_scaled))
    g_psi1 = t(np.pad(p['g1'], ((0, 0), (0, 0), (0, mp - m))))
    got = ops.elbo_grad_psi(None, t(p['z']), t(p['mu']), t(p['s']), t(p['gamma']), t(p['alpha']), g_psi2, w_kuu, None, prec=prec,
                            g_psi1=g_psi1)
    worst = 0.0
    for name, g, w in zip(('d mu', 'd S', 'd z', 'd gamma'), got, want):
        worst = max(worst, check_cols(g.cpu().numpy(), w, GRAD_TOL, '%s (%s, D N M Q = %s)' % (name, prec, case)))
    return worst


@pytest.mark.parametrize('prec', ['mixed', 'mixed_patch'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'D%d_N%d_M%d_Q%d' % c)
def test_full_psi1_adjoint_against_autograd(dev, case, prec, record_property):
    record_property('max_col_rel_err', _run(dev, case, prec))


@pytest.mark.parametrize('prec', ['mixed', 'mixed_patch'])
def test_full_psi1_adjoint_beyond_48k_of_lds(dev, prec, record_property):
    """M = 512, Q = 21: psi1_grad_n_kernel and kuu_grad_kernel take the hipFuncSetAttribute branch (M QP 4 B > 48 KB)."""
    record_property('max_col_rel_err', _run(dev, LDS_CASE, prec, zero_g2=True))


@pytest.mark.parametrize('m', [40, 129])
def test_kuu_term_with_a_dominant_diagonal(dev, m, record_property):
    """The K_uu term alone (G1 = G2 = 0) where the diagonal of GK .* K dominates each row: well separated inducing inputs and a
    large diagonal in GK, as behind a small noise precision (beta ~ 1 / var(y)).  The diagonal contributes nothing to d/dz and
    d/dgamma; kuu_grad_kernel used to add it into fp32 row sums whose difference it then took (1e-3 of the largest entry off)."""
    d, n, q = 2, 33, 4
    rng = np.random.default_rng(m)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    z = 3.0 * rng.standard_normal((m, q))
    gamma = np.exp(0.3 * rng.standard_normal((d, q))) * 0.7
    alpha = np.exp(0.2 * rng.standard_normal(d))
    gk = 0.1 * rng.standard_normal((d, m, m))
    gk = 0.5 * (gk + gk.transpose(0, 2, 1)) + 1e3 * np.eye(m)[None]
    zt, gt = t(z).cpu().requires_grad_(True), t(gamma).cpu().requires_grad_(True)
    k_uu, _, _ = ot.psi_pieces(torch.zeros((0, d), dtype=torch.float64), zt, zt[:0], zt[:0], gt, t(alpha).cpu(), jitter=JITTER)
    want_z, want_g = (a.numpy() for a in torch.autograd.grad(torch.sum(torch.as_tensor(gk) * k_uu), [zt, gt]))
    mp = 16 * ((m + 15) // 16)
    w_kuu = np.pad(gk * (k_uu.detach().numpy() - JITTER * np.eye(m)), ((0, 0), (0, mp - m), (0, mp - m)))
    mu, s = rng.standard_normal((n, q)), np.exp(0.3 * rng.standard_normal((n, q)))
    _, _, dz, dg = ops.elbo_grad_psi(None, t(z), t(mu), t(s), t(gamma), t(alpha), t(np.zeros((d, mp, mp))), t(w_kuu), None,
                                     prec='mixed', g_psi1=t(np.zeros((d, n, mp))))
    e = check_cols(dz.cpu().numpy(), want_z, GRAD_TOL, 'd z')
    record_property('max_col_rel_err', max(e, check_cols(dg.cpu().numpy(), want_g, GRAD_TOL, 'd gamma')))


@pytest.mark.parametrize('prec', ['mixed', 'mixed_patch'])
def test_full_psi1_adjoint_with_tiny_ard_weights(dev, prec, record_property):
    """gamma = 1e-6 on every other latent dim: the gradients of those columns are ~1e-6 of the others and are held to their own
    largest entry."""
    record_property('max_col_rel_err', _run(dev, TINY_GAMMA_CASE, prec, tiny_gamma=True))
