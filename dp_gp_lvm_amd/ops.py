"""
Torch-tensor front-end of the C ABI (include/dpgp.h).  PyTorch is plumbing here: device memory, the current HIP stream
and (in models/) torch.distributed.  Every function takes CUDA (ROCm) tensors, enqueues HIP kernels on the current
stream and returns device tensors; nothing here computes on the host and there is no fallback.
"""
import ctypes

import torch

from . import _lib

_SUFFIX = {torch.float32: 'f32', torch.float64: 'f64'}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _prep(t, dtype, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor' % name)
    if not t.is_cuda:
        raise RuntimeError('%s must live on the GPU: dp_gp_lvm_amd runs its operators in HIP only' % name)
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _dtype_of(*ts):
    dt = ts[0].dtype
    if dt not in _SUFFIX:
        raise TypeError('expected float32 or float64 tensors, got %s' % dt)
    return dt


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _hyp(gamma, alpha, beta, dt):
    gamma = _prep(gamma, dt, 'gamma')
    assert gamma.dim() == 2, 'gamma must be [B x Q]'
    b = gamma.shape[0]
    alpha = _prep(alpha, dt, 'alpha').reshape(-1)
    assert alpha.numel() == b, 'alpha must be [B x 1]'
    if beta is not None:
        beta = _prep(beta, dt, 'beta').reshape(-1)
        assert beta.numel() == b, 'beta must be [B x 1]'
    return gamma, alpha, beta, b


def ard_rbf_gram(x0, x1, gamma, alpha, beta, include_noise=False, include_jitter=False, jitter=1e-8):
    """Kernel.covariance_matrix -> [B,N0,N1]  (reference: src/kernels/rbf_kernel.py:58-93)."""
    dt = _dtype_of(x0)
    x0 = _prep(x0, dt, 'input_0')
    gamma, alpha, beta, b = _hyp(gamma, alpha, beta, dt)
    q = gamma.shape[1]
    assert x0.dim() == 2 and x0.shape[1] == q, 'input_0 must be [N0 x Q]'
    n0 = x0.shape[0]
    n1 = n0
    x1p = None
    if x1 is not None:
        x1 = _prep(x1, dt, 'input_1')
        assert x1.dim() == 2 and x1.shape[1] == q, 'input_1 must be [N1 x Q]'
        n1, x1p = x1.shape[0], x1.data_ptr()
    out = torch.empty((b, n0, n1), dtype=dt, device=x0.device)
    flags = (_lib.FLAG_NOISE if include_noise else 0) | (_lib.FLAG_JITTER if include_jitter else 0)
    name = 'dpgp_ard_rbf_gram_' + _SUFFIX[dt]
    _lib.check(getattr(_lib.lib(), name)(b, n0, n1, q, x0.data_ptr(), x1p, gamma.data_ptr(), alpha.data_ptr(),
                                         beta.data_ptr(), flags, float(jitter), out.data_ptr(), _stream()), name)
    return out


def ard_rbf_gram_grad(x, gamma, alpha, w):
    """The gram-gradient contraction of dpgp_ard_rbf_gram_grad_f64 (fp64): with G = w * (noise-free ARD-RBF gram of x),
    returns r = G.sum(1) [N], sx[i,q] = sum_j G_ij (x_iq - x_jq) [N,Q] and sq[i,q] = sum_j G_ij (x_iq - x_jq)^2 [N,Q].
    x [N,Q], gamma [1,Q] or [Q], alpha one element, w [N,N] (any; a row-sliced view with unit column stride is used in place)."""
    f64 = torch.float64
    x = _prep(x, f64, 'x')
    assert x.dim() == 2, 'x must be [N x Q]'
    n, q = x.shape
    gamma = _prep(gamma, f64, 'gamma').reshape(-1)
    alpha = _prep(alpha, f64, 'alpha').reshape(-1)
    assert gamma.numel() == q and alpha.numel() == 1, 'gamma must be [1 x Q], alpha [1 x 1]'
    if not isinstance(w, torch.Tensor) or not w.is_cuda:
        raise RuntimeError('w must live on the GPU: dp_gp_lvm_amd runs its operators in HIP only')
    assert w.dim() == 2 and tuple(w.shape) == (n, n), 'w must be [N x N]'
    w = w.to(f64)
    if w.stride(1) != 1 or w.stride(0) < max(1, n):
        w = w.contiguous()
    r = torch.empty(n, dtype=f64, device=x.device)
    sx = torch.empty((n, q), dtype=f64, device=x.device)
    sq = torch.empty((n, q), dtype=f64, device=x.device)
    if n == 0:
        return r, sx, sq
    l = _lib.lib()
    wsb = l.dpgp_ard_rbf_gram_grad_workspace_bytes(n, q)
    ws = _ws(wsb, x.device)
    _lib.check(l.dpgp_ard_rbf_gram_grad_f64(n, q, x.data_ptr(), gamma.data_ptr(), alpha.data_ptr(), w.data_ptr(), w.stride(0),
                                            r.data_ptr(), sx.data_ptr(), sq.data_ptr(), ws.data_ptr(), wsb, _stream()),
               'dpgp_ard_rbf_gram_grad_f64')
    return r, sx, sq


def ard_rbf_gram_grad_batched(x, gamma, alpha, w):
    """ard_rbf_gram_grad for B kernels in one launch pair (dpgp_ard_rbf_gram_grad_batched_f64, fp64): x [B,N,Q], gamma [B,Q],
    alpha [B], w [B,N,N] (any; a view with unit column stride, e.g. big[:, :N, :N], is used in place).  Returns r [B,N],
    sx [B,N,Q], sq [B,N,Q]: for every b what ard_rbf_gram_grad returns for b's own inputs."""
    f64 = torch.float64
    x = _prep(x, f64, 'x')
    assert x.dim() == 3, 'x must be [B x N x Q]'
    b, n, q = x.shape
    gamma = _prep(gamma, f64, 'gamma')
    alpha = _prep(alpha, f64, 'alpha').reshape(-1)
    assert gamma.numel() == b * q and alpha.numel() == b, 'gamma must be [B x Q], alpha [B]'
    gamma = gamma.reshape(b, q)
    if not isinstance(w, torch.Tensor) or not w.is_cuda:
        raise RuntimeError('w must live on the GPU: dp_gp_lvm_amd runs its operators in HIP only')
    assert w.dim() == 3 and tuple(w.shape) == (b, n, n), 'w must be [B x N x N]'
    w = w.to(f64)
    if w.stride(2) != 1 or w.stride(1) < max(1, n) or (b > 1 and w.stride(0) < (n - 1) * w.stride(1) + n):
        w = w.contiguous()
    r = torch.empty((b, n), dtype=f64, device=x.device)
    sx = torch.empty((b, n, q), dtype=f64, device=x.device)
    sq = torch.empty((b, n, q), dtype=f64, device=x.device)
    if b == 0 or n == 0:
        return r, sx, sq
    l = _lib.lib()
    wsb = l.dpgp_ard_rbf_gram_grad_batched_workspace_bytes(b, n, q)
    ws = _ws(wsb, x.device)
    _lib.check(l.dpgp_ard_rbf_gram_grad_batched_f64(b, n, q, x.data_ptr(), gamma.data_ptr(), alpha.data_ptr(), w.data_ptr(),
                                                    w.stride(1), w.stride(0), r.data_ptr(), sx.data_ptr(), sq.data_ptr(),
                                                    ws.data_ptr(), wsb, _stream()),
               'dpgp_ard_rbf_gram_grad_batched_f64')
    return r, sx, sq


def _qx_args(z, mu, s, gamma, alpha, zfac):
    f64 = torch.float64
    z, mu, s = _prep(z, f64, 'z'), _prep(mu, f64, 'mu'), _prep(s, f64, 's')
    assert z.dim() == 3, 'z must be [B x M x Q]'
    b, m, q = z.shape
    assert mu.dim() == 2 and mu.shape[1] == q and s.shape == mu.shape, 'mu and s must be [N* x Q]'
    gamma = _prep(gamma, f64, 'gamma').reshape(b, -1)
    alpha = _prep(alpha, f64, 'alpha').reshape(-1)
    assert gamma.shape[1] == q and alpha.numel() == b, 'gamma must be [B x Q], alpha [B]'
    if zfac is not None:
        zfac = _prep(zfac, f64, 'zfac')
        assert tuple(zfac.shape) == (b, m, m), 'zfac must be [B x M x M]'
    return z, mu, s, gamma, alpha, zfac, b, mu.shape[0], m, q


def _qx_weights(weights, b, n, ref):
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float64 or not weights.is_contiguous():
        raise TypeError('weights must be a contiguous float64 torch.Tensor')
    if weights.device != ref.device:
        raise RuntimeError('weights must live on the device of the inputs')
    assert tuple(weights.shape) == (b, n), 'weights must be [B x N*]'
    return weights


def qx_pair_factor(z, gamma, alpha):
    """The q(X*)-independent factor of Psi2 per kernel, alpha_b^2 exp(-1/4 sum_q gamma_bq (z_bm - z_bm')^2) [B,M,M], as the gram
    of z_b with gamma_b / 2 and alpha_b^2 (one dpgp_ard_rbf_gram_f64 per kernel; formed once while Z is frozen)."""
    f64 = torch.float64
    z = _prep(z, f64, 'z')
    gamma = _prep(gamma, f64, 'gamma').reshape(z.shape[0], -1)
    alpha = _prep(alpha, f64, 'alpha').reshape(-1)
    one = torch.ones(1, 1, dtype=f64, device=z.device)
    return torch.cat([ard_rbf_gram(z[b], None, 0.5 * gamma[b:b + 1], (alpha[b] * alpha[b]).reshape(1, 1), one)
                      for b in range(z.shape[0])]).contiguous()


def qx_psi_stats_batched(z, mu, s, gamma, alpha, zfac=None, weights=None):
    """Psi1 [B,N*,M] and Psi2 [B,M,M] of q(X*) = (mu, s) [N*,Q] for B kernels with their own inducing inputs z [B,M,Q],
    gamma [B,Q], alpha [B] (rbf_kernel.py:135-199), fp64 (dpgp_qx_psi_stats_batched_f64).  zfac: qx_pair_factor(z, gamma, alpha)
    or None (computed in the kernels).  weights: None, or [B,N*] fp64 contiguous on the inputs' device: Psi2_b becomes
    sum_n weights[b,n] (test point n's term) (dpgp_qx_psi_stats_weighted_f64; Psi1 is not weighted)."""
    z, mu, s, gamma, alpha, zfac, b, n, m, q = _qx_args(z, mu, s, gamma, alpha, zfac)
    psi_1 = torch.empty((b, n, m), dtype=torch.float64, device=mu.device)
    psi_2 = torch.empty((b, m, m), dtype=torch.float64, device=mu.device)
    l = _lib.lib()
    wsb = l.dpgp_qx_psi_stats_workspace_bytes(b, n, m, q)
    ws = _ws(wsb, mu.device)
    if weights is not None:
        weights = _qx_weights(weights, b, n, mu)
        _lib.check(l.dpgp_qx_psi_stats_weighted_f64(b, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                                    alpha.data_ptr(), None if zfac is None else zfac.data_ptr(),
                                                    weights.data_ptr(), psi_1.data_ptr(), psi_2.data_ptr(), ws.data_ptr(), wsb,
                                                    _stream()), 'dpgp_qx_psi_stats_weighted_f64')
        return psi_1, psi_2
    _lib.check(l.dpgp_qx_psi_stats_batched_f64(b, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                               alpha.data_ptr(), None if zfac is None else zfac.data_ptr(), psi_1.data_ptr(),
                                               psi_2.data_ptr(), ws.data_ptr(), wsb, _stream()),
               'dpgp_qx_psi_stats_batched_f64')
    return psi_1, psi_2


def qx_psi_adjoint(z, mu, s, gamma, alpha, g1, g2, zfac=None, weights=None):
    """(d_mu, d_s) [N*,Q]: the adjoints g1 = dF/dPsi1 [B,N*,M] and g2 = dF/dPsi2 [B,M,M] of the B kernels of
    qx_psi_stats_batched contracted with dPsi/d(mu, s), summed over the kernels (dpgp_qx_psi_adjoint_f64; fixed summation
    order, the same bits on every run).  weights: as qx_psi_stats_batched; the Psi2 part of test point n from kernel b is
    multiplied by weights[b,n], the Psi1 part is governed by g1 alone (dpgp_qx_psi_adjoint_weighted_f64)."""
    z, mu, s, gamma, alpha, zfac, b, n, m, q = _qx_args(z, mu, s, gamma, alpha, zfac)
    g1, g2 = _prep(g1, torch.float64, 'g1'), _prep(g2, torch.float64, 'g2')
    assert tuple(g1.shape) == (b, n, m) and tuple(g2.shape) == (b, m, m), 'g1 must be [B x N* x M], g2 [B x M x M]'
    d_mu = torch.empty((n, q), dtype=torch.float64, device=mu.device)
    d_s = torch.empty_like(d_mu)
    l = _lib.lib()
    wsb = l.dpgp_qx_psi_adjoint_workspace_bytes(b, n, m, q)
    ws = _ws(wsb, mu.device)
    if weights is not None:
        weights = _qx_weights(weights, b, n, mu)
        _lib.check(l.dpgp_qx_psi_adjoint_weighted_f64(b, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                                      alpha.data_ptr(), None if zfac is None else zfac.data_ptr(),
                                                      weights.data_ptr(), g1.data_ptr(), g2.data_ptr(), d_mu.data_ptr(),
                                                      d_s.data_ptr(), ws.data_ptr(), wsb, _stream()),
                   'dpgp_qx_psi_adjoint_weighted_f64')
        return d_mu, d_s
    _lib.check(l.dpgp_qx_psi_adjoint_f64(b, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                         alpha.data_ptr(), None if zfac is None else zfac.data_ptr(), g1.data_ptr(),
                                         g2.data_ptr(), d_mu.data_ptr(), d_s.data_ptr(), ws.data_ptr(), wsb, _stream()),
               'dpgp_qx_psi_adjoint_f64')
    return d_mu, d_s


def qx_psi_param_adjoint(z, mu, s, gamma, alpha, g1, g2, zfac=None, weights=None):
    """(d_z [B,M,Q], d_gamma [B,Q], d_alpha [B]): the adjoints g1 [B,N*,M] and g2 [B,M,M] of qx_psi_adjoint contracted with
    dPsi/d(z_b, gamma_b, alpha_b) of the (weighted) statistics, PER KERNEL b, not summed over the kernels
    (dpgp_qx_psi_param_adjoint_weighted_f64; the derivative of the complete Psi2, pair factor included: zfac is only its cached
    value; fixed summation order, the same bits on every run).  weights: as qx_psi_stats_batched (None: all ones)."""
    z, mu, s, gamma, alpha, zfac, b, n, m, q = _qx_args(z, mu, s, gamma, alpha, zfac)
    g1, g2 = _prep(g1, torch.float64, 'g1'), _prep(g2, torch.float64, 'g2')
    assert tuple(g1.shape) == (b, n, m) and tuple(g2.shape) == (b, m, m), 'g1 must be [B x N* x M], g2 [B x M x M]'
    d_z = torch.empty((b, m, q), dtype=torch.float64, device=mu.device)
    d_gamma = torch.empty((b, q), dtype=torch.float64, device=mu.device)
    d_alpha = torch.empty(b, dtype=torch.float64, device=mu.device)
    l = _lib.lib()
    wsb = l.dpgp_qx_psi_param_adjoint_workspace_bytes(b, n, m, q)
    ws = _ws(wsb, mu.device)
    if weights is not None:
        weights = _qx_weights(weights, b, n, mu)
    _lib.check(l.dpgp_qx_psi_param_adjoint_weighted_f64(b, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                                        alpha.data_ptr(), None if zfac is None else zfac.data_ptr(),
                                                        None if weights is None else weights.data_ptr(), g1.data_ptr(),
                                                        g2.data_ptr(), d_z.data_ptr(), d_gamma.data_ptr(), d_alpha.data_ptr(),
                                                        ws.data_ptr(), wsb, _stream()), 'dpgp_qx_psi_param_adjoint_weighted_f64')
    return d_z, d_gamma, d_alpha


def _qx_grouped_args(z, mu, s, gamma, alpha, weights, zfac):
    z, mu, s, gamma, alpha, zfac, k, n, m, q = _qx_args(z, mu, s, gamma, alpha, zfac)
    if not isinstance(weights, torch.Tensor) or weights.dim() != 2:
        raise TypeError('weights must be a [P x N] float64 torch.Tensor (required by the grouped operators)')
    weights = _qx_weights(weights, weights.shape[0], n, mu)
    assert weights.shape[0] >= 1, 'weights must hold at least one row'
    return z, mu, s, gamma, alpha, zfac, weights, k, weights.shape[0], n, m, q


def qx_psi_stats_grouped(z, mu, s, gamma, alpha, weights, zfac=None):
    """Psi1 [K,N,M] (once per kernel, not weighted) and Psi2 [K,P,M,M] = sum_n weights[p,n] psi2_kn of q(X) = (mu, s) [N,Q] for K
    kernels z [K,M,Q], gamma [K,Q], alpha [K] and P weight rows [P,N] shared by the kernels (dpgp_qx_psi_stats_grouped_f64):
    what qx_psi_stats_batched(weights=) gives for the K P slots (k, p), with every exponential evaluated once per chunk of
    patterns.  weights: fp64 contiguous on the inputs' device, required."""
    z, mu, s, gamma, alpha, zfac, weights, k, p, n, m, q = _qx_grouped_args(z, mu, s, gamma, alpha, weights, zfac)
    psi_1 = torch.empty((k, n, m), dtype=torch.float64, device=mu.device)
    psi_2 = torch.empty((k, p, m, m), dtype=torch.float64, device=mu.device)
    l = _lib.lib()
    wsb = l.dpgp_qx_psi_stats_grouped_workspace_bytes(k, p, n, m, q)
    ws = _ws(wsb, mu.device)
    _lib.check(l.dpgp_qx_psi_stats_grouped_f64(k, p, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                               alpha.data_ptr(), None if zfac is None else zfac.data_ptr(), weights.data_ptr(),
                                               psi_1.data_ptr(), psi_2.data_ptr(), ws.data_ptr(), wsb, _stream()),
               'dpgp_qx_psi_stats_grouped_f64')
    return psi_1, psi_2


def _qx_grouped_adjoints(g1, g2, k, p, n, m):
    g1, g2 = _prep(g1, torch.float64, 'g1'), _prep(g2, torch.float64, 'g2')
    assert tuple(g1.shape) == (k, n, m) and tuple(g2.shape) == (k, p, m, m), 'g1 must be [K x N x M], g2 [K x P x M x M]'
    return g1, g2


def qx_psi_adjoint_grouped(z, mu, s, gamma, alpha, g1, g2, weights, zfac=None):
    """(d_mu, d_s) [N,Q] of sum_k <g1_k, Psi1_k> + sum_kp <g2_kp, Psi2_kp> for the statistics of qx_psi_stats_grouped: g1 [K,N,M]
    (already summed over the patterns), g2 [K,P,M,M] (any matrices) (dpgp_qx_psi_adjoint_grouped_f64; fixed summation order)."""
    z, mu, s, gamma, alpha, zfac, weights, k, p, n, m, q = _qx_grouped_args(z, mu, s, gamma, alpha, weights, zfac)
    g1, g2 = _qx_grouped_adjoints(g1, g2, k, p, n, m)
    d_mu = torch.empty((n, q), dtype=torch.float64, device=mu.device)
    d_s = torch.empty_like(d_mu)
    l = _lib.lib()
    wsb = l.dpgp_qx_psi_adjoint_grouped_workspace_bytes(k, p, n, m, q)
    ws = _ws(wsb, mu.device)
    _lib.check(l.dpgp_qx_psi_adjoint_grouped_f64(k, p, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                                 alpha.data_ptr(), None if zfac is None else zfac.data_ptr(), weights.data_ptr(),
                                                 g1.data_ptr(), g2.data_ptr(), d_mu.data_ptr(), d_s.data_ptr(), ws.data_ptr(), wsb,
                                                 _stream()), 'dpgp_qx_psi_adjoint_grouped_f64')
    return d_mu, d_s


def qx_psi_param_adjoint_grouped(z, mu, s, gamma, alpha, g1, g2, weights, zfac=None):
    """(d_z [K,M,Q], d_gamma [K,Q], d_alpha [K]) of the same sum, per kernel, summed over that kernel's patterns; the derivative
    of the complete Psi2, pair factor included (dpgp_qx_psi_param_adjoint_grouped_f64; fixed summation order)."""
    z, mu, s, gamma, alpha, zfac, weights, k, p, n, m, q = _qx_grouped_args(z, mu, s, gamma, alpha, weights, zfac)
    g1, g2 = _qx_grouped_adjoints(g1, g2, k, p, n, m)
    d_z = torch.empty((k, m, q), dtype=torch.float64, device=mu.device)
    d_gamma = torch.empty((k, q), dtype=torch.float64, device=mu.device)
    d_alpha = torch.empty(k, dtype=torch.float64, device=mu.device)
    l = _lib.lib()
    wsb = l.dpgp_qx_psi_param_adjoint_grouped_workspace_bytes(k, p, n, m, q)
    ws = _ws(wsb, mu.device)
    _lib.check(l.dpgp_qx_psi_param_adjoint_grouped_f64(k, p, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                                       alpha.data_ptr(), None if zfac is None else zfac.data_ptr(),
                                                       weights.data_ptr(), g1.data_ptr(), g2.data_ptr(), d_z.data_ptr(),
                                                       d_gamma.data_ptr(), d_alpha.data_ptr(), ws.data_ptr(), wsb, _stream()),
               'dpgp_qx_psi_param_adjoint_grouped_f64')
    return d_z, d_gamma, d_alpha


def _qx_point_args(c, r, k, m, mu):
    for name, a in (('c', c), ('r', r)):
        if not isinstance(a, torch.Tensor) or a.dtype != torch.float64:
            raise TypeError('%s must be a float64 torch.Tensor' % name)
        if a.device != mu.device:
            raise RuntimeError('%s must live on the device of the inputs' % name)
    if c.dim() != 4 or c.shape[0] != k or c.shape[1] < 1 or tuple(c.shape[2:]) != (m, m):
        raise ValueError('c must be [K x G x M x M] with G >= 1, got %s' % (tuple(c.shape),))
    if r.dim() != 3 or r.shape[0] != k or r.shape[1] != m or r.shape[2] < 1:
        raise ValueError('r must be [K x M x J] with J >= 1, got %s' % (tuple(r.shape),))
    return c.contiguous(), r.contiguous()


def qx_psi_point_moments(z, mu, s, gamma, alpha, c, r, gidx, beta, zfac=None):
    """Per-entry predictive moments (dpgp_qx_psi_point_moments_f64): with psi1_kn [M], psi2_kn [M,M] test point n's own
    statistics of kernel k at q(X) = (mu, s) [N,Q] (kernels, c [K,G,M,M] and r [K,M,J] as in qx_psi_pointwise), returns
        mean [K,N,J] = sum_m psi1_kn[m] r[k,m,j]
        var [K,N,J]  = alpha_k + 1/beta_k - <c[k,gidx[k,j]], psi2_kn> + r_kj^T psi2_kn r_kj - mean^2
    from one operator call; neither psi1 [K,N,M] nor psi2_kn is formed in memory.  gidx [K,J]: an int32 tensor, any value outside
    [0, G) means no trace term; beta [K] fp64.  Fixed summation order, the same bits on every run."""
    z, mu, s, gamma, alpha, zfac, k, n, m, q = _qx_args(z, mu, s, gamma, alpha, zfac)
    c, r = _qx_point_args(c, r, k, m, mu)
    g, j = c.shape[1], r.shape[2]
    if not isinstance(gidx, torch.Tensor) or gidx.dtype != torch.int32:
        raise TypeError('gidx must be an int32 torch.Tensor')
    if not isinstance(beta, torch.Tensor) or beta.dtype != torch.float64:
        raise TypeError('beta must be a float64 torch.Tensor')
    if gidx.device != mu.device or beta.device != mu.device:
        raise RuntimeError('gidx and beta must live on the device of the inputs')
    if tuple(gidx.shape) != (k, j):
        raise ValueError('gidx must be [K x J], got %s' % (tuple(gidx.shape),))
    if tuple(beta.shape) != (k,):
        raise ValueError('beta must be [K], got %s' % (tuple(beta.shape),))
    gidx, beta = gidx.contiguous(), beta.contiguous()
    mean = torch.empty((k, n, j), dtype=torch.float64, device=mu.device)
    var = torch.empty_like(mean)
    l = _lib.lib()
    wsb = l.dpgp_qx_psi_point_moments_workspace_bytes(k, g, j, n, m, q)
    ws = _ws(wsb, mu.device)
    _lib.check(l.dpgp_qx_psi_point_moments_f64(k, g, j, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                               alpha.data_ptr(), None if zfac is None else zfac.data_ptr(), c.data_ptr(),
                                               r.data_ptr(), gidx.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr(),
                                               ws.data_ptr(), wsb, _stream()), 'dpgp_qx_psi_point_moments_f64')
    return mean, var


def qx_psi_pointwise(z, mu, s, gamma, alpha, c, r, zfac=None):
    """Per-point Psi2 contractions (dpgp_qx_psi_pointwise_f64): with psi2_kn [M,M] test point n's own term of kernel k's Psi2 at
    q(X) = (mu, s) [N,Q] (kernels z [K,M,Q], gamma [K,Q], alpha [K] as in qx_psi_stats_grouped), returns
        tr [K,N,G]   = sum_{m,m'} c[k,g,m,m'] psi2_kn[m,m']            c [K,G,M,M], any matrices
        quad [K,N,J] = sum_{m,m'} r[k,m,j] r[k,m',j] psi2_kn[m,m']     r [K,M,J]
    without forming psi2_kn in memory; fixed summation order, the same bits on every run.  c and r: float64 tensors on the
    inputs' device (TypeError otherwise), of these shapes (ValueError otherwise)."""
    z, mu, s, gamma, alpha, zfac, k, n, m, q = _qx_args(z, mu, s, gamma, alpha, zfac)
    c, r = _qx_point_args(c, r, k, m, mu)
    g, j = c.shape[1], r.shape[2]
    tr = torch.empty((k, n, g), dtype=torch.float64, device=mu.device)
    quad = torch.empty((k, n, j), dtype=torch.float64, device=mu.device)
    l = _lib.lib()
    wsb = l.dpgp_qx_psi_pointwise_workspace_bytes(k, g, j, n, m, q)
    ws = _ws(wsb, mu.device)
    _lib.check(l.dpgp_qx_psi_pointwise_f64(k, g, j, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                           alpha.data_ptr(), None if zfac is None else zfac.data_ptr(), c.data_ptr(), r.data_ptr(),
                                           tr.data_ptr(), quad.data_ptr(), ws.data_ptr(), wsb, _stream()),
               'dpgp_qx_psi_pointwise_f64')
    return tr, quad


def _qx_point_adjoint(a, name, shape, mu):
    if not isinstance(a, torch.Tensor) or a.dtype != torch.float64:
        raise TypeError('%s must be a float64 torch.Tensor' % name)
    if a.device != mu.device:
        raise RuntimeError('%s must live on the device of the inputs' % name)
    if tuple(a.shape) != shape:
        raise ValueError('%s must be %s, got %s' % (name, list(shape), tuple(a.shape)))
    return a.contiguous()


def qx_psi_pointwise_adjoint(z, mu, s, gamma, alpha, c, r, h, gq, gt, zfac=None):
    """(d_mu, d_s) [N,Q] of  L = sum_knj h (psi1_kn . r_kj) + sum_knj gq (r_kj^T psi2_kn r_kj) + sum_kng gt <c_kg, psi2_kn>
    (dpgp_qx_psi_pointwise_adjoint_f64): the latent adjoint of qx_psi_pointwise's two outputs (adjoints gt [K,N,G] of tr, gq [K,N,J]
    of quad) and of psi1 . r (adjoint h [K,N,J]), summed over the kernels; inputs as qx_psi_pointwise.  Derivatives with respect to
    the variances s.  The adjoint of psi2_kn is formed before it meets the exponentials: one exponential per (k, n, pair) whatever
    G + J is; nothing of size N M M is formed.  Fixed summation order, the same bits on every run; a zero adjoint gives exactly 0."""
    z, mu, s, gamma, alpha, zfac, k, n, m, q = _qx_args(z, mu, s, gamma, alpha, zfac)
    c, r = _qx_point_args(c, r, k, m, mu)
    g, j = c.shape[1], r.shape[2]
    h = _qx_point_adjoint(h, 'h', (k, n, j), mu)
    gq = _qx_point_adjoint(gq, 'gq', (k, n, j), mu)
    gt = _qx_point_adjoint(gt, 'gt', (k, n, g), mu)
    d_mu = torch.empty((n, q), dtype=torch.float64, device=mu.device)
    d_s = torch.empty_like(d_mu)
    l = _lib.lib()
    wsb = l.dpgp_qx_psi_pointwise_adjoint_workspace_bytes(k, g, j, n, m, q)
    ws = _ws(wsb, mu.device)
    _lib.check(l.dpgp_qx_psi_pointwise_adjoint_f64(k, g, j, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                                   alpha.data_ptr(), None if zfac is None else zfac.data_ptr(), c.data_ptr(),
                                                   r.data_ptr(), h.data_ptr(), gq.data_ptr(), gt.data_ptr(), d_mu.data_ptr(),
                                                   d_s.data_ptr(), ws.data_ptr(), wsb, _stream()),
               'dpgp_qx_psi_pointwise_adjoint_f64')
    return d_mu, d_s


def point_moments_adjoints(gidx, g, mean, g_mean, g_var):
    """The adjoints (h, gq, gt) of (psi1 . r, quad, tr) that the combination step of qx_psi_point_moments passes back:
    mean = psi1 . r,  var = const - tr[gidx] + quad - mean^2.  gidx [K,J] int, g the number of trace columns; a gidx outside
    [0, g) has no trace term and contributes nothing.  Plain tensor algebra on the tensors' device; the gather's transpose is a
    product with the one-hot matrix of gidx, not index_add, whose atomic adds on the GPU would not give the same bits twice."""
    h = g_mean - 2.0 * mean * g_var
    onehot = (gidx.to(torch.int64)[:, :, None] == torch.arange(g, device=gidx.device)[None, None, :]).to(g_var.dtype)
    gt = -torch.bmm(g_var, onehot)
    return h, g_var, gt


def qx_psi_point_moments_adjoint(z, mu, s, gamma, alpha, c, r, gidx, beta, mean, g_mean, g_var, zfac=None):
    """The vector-Jacobian product of qx_psi_point_moments with respect to q(X) = (mu, s): (d_mu, d_s) [N,Q] of
    sum g_mean . mean + sum g_var . var, with mean [K,N,J] the operator's first output at the same inputs and g_mean, g_var
    [K,N,J] fp64.  A host composition on qx_psi_pointwise_adjoint: h = g_mean - 2 mean g_var, gq = g_var, gt[k,n,g] = -sum of
    g_var[k,n,j] over the columns with gidx[k,j] = g.  beta enters var as a constant only and is accepted for symmetry."""
    if not isinstance(gidx, torch.Tensor) or gidx.dtype != torch.int32:
        raise TypeError('gidx must be an int32 torch.Tensor')
    if not isinstance(c, torch.Tensor) or c.dim() != 4:
        raise ValueError('c must be [K x G x M x M]')
    for name, a in (('mean', mean), ('g_mean', g_mean), ('g_var', g_var)):
        if not isinstance(a, torch.Tensor) or a.dtype != torch.float64:
            raise TypeError('%s must be a float64 torch.Tensor' % name)
        if a.shape != g_var.shape or a.dim() != 3:
            raise ValueError('mean, g_mean and g_var must be [K x N x J]')
    if tuple(gidx.shape) != (g_var.shape[0], g_var.shape[2]):
        raise ValueError('gidx must be [K x J], got %s' % (tuple(gidx.shape),))
    h, gq, gt = point_moments_adjoints(gidx, c.shape[1], mean, g_mean, g_var)
    return qx_psi_pointwise_adjoint(z, mu, s, gamma, alpha, c, r, h, gq, gt, zfac=zfac)


def psi_latent_adjoint(z, mu, s, gamma, alpha, y, g_v, g_psi2, weights=None):
    """(d_mu, d_s) [N*,Q] of  L = sum_b <g_psi2_b, sum_n weights[b,n] psi2_bn> + sum_b g_v_b . (Psi1_b^T y_b)  for B kernels
    (gamma [B,Q], alpha [B]) that share the inducing inputs z [M,Q] and q(X*) = (mu, s) [N*,Q] (dpgp_psi_latent_adjoint_f64, fp64):
    y [N*,B] zero-filled data (column b for kernel b; row stride free), g_v [B,M], g_psi2 [B,M,M] (any matrices), weights None
    (all ones) or [B,N*] fp64 contiguous.  Derivatives with respect to the variances s.  Nothing of size B N* M or N* M M is
    formed; fixed summation order, the same bits on every run."""
    f64 = torch.float64
    z, mu, s = _prep(z, f64, 'z'), _prep(mu, f64, 'mu'), _prep(s, f64, 's')
    assert z.dim() == 2, 'z must be [M x Q]'
    m, q = z.shape
    assert mu.dim() == 2 and mu.shape[1] == q and s.shape == mu.shape, 'mu and s must be [N* x Q]'
    n = mu.shape[0]
    gamma = _prep(gamma, f64, 'gamma')
    assert gamma.dim() == 2 and gamma.shape[1] == q, 'gamma must be [B x Q]'
    b = gamma.shape[0]
    alpha = _prep(alpha, f64, 'alpha').reshape(-1)
    assert alpha.numel() == b, 'alpha must be [B]'
    if not isinstance(y, torch.Tensor):
        raise TypeError('y must be a torch.Tensor')
    if y.dtype != f64 or not y.is_cuda or y.dim() != 2 or y.stride(1) != 1 or y.stride(0) < b:
        y = _prep(y, f64, 'y')
    assert tuple(y.shape) == (n, b), 'y must be [N* x B]'
    g_v, g_psi2 = _prep(g_v, f64, 'g_v'), _prep(g_psi2, f64, 'g_psi2')
    assert tuple(g_v.shape) == (b, m) and tuple(g_psi2.shape) == (b, m, m), 'g_v must be [B x M], g_psi2 [B x M x M]'
    if weights is not None:
        weights = _qx_weights(weights, b, n, mu)
    d_mu = torch.empty((n, q), dtype=f64, device=mu.device)
    d_s = torch.empty_like(d_mu)
    l = _lib.lib()
    wsb = l.dpgp_psi_latent_adjoint_workspace_bytes(b, n, m, q)
    ws = _ws(wsb, mu.device)
    _lib.check(l.dpgp_psi_latent_adjoint_f64(b, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                             alpha.data_ptr(), y.data_ptr(), y.stride(0), None if weights is None else weights.data_ptr(),
                                             g_v.data_ptr(), g_psi2.data_ptr(), d_mu.data_ptr(), d_s.data_ptr(), ws.data_ptr(), wsb,
                                             _stream()), 'dpgp_psi_latent_adjoint_f64')
    return d_mu, d_s


def _point_metric_args(z, x, gamma, alpha, a, name, what, dirs=None, max_q=None, prior=None, frame=None):
    """The checks of the six point operators below: float64 tensors (TypeError), of the stated shapes (ValueError), on one GPU
    (RuntimeError), in this order; `a` is the last operand (`name`: p [K,M,M], r [K,M,J] or c [K,G,M,M], `what` its wording);
    dirs: the directions v [N,Q] of ard_rbf_point_energy / ard_rbf_point_christoffel (a one-element tuple), or (v, dx, dv) of
    ard_rbf_point_christoffel_tangent, checked in their place after x; max_q: an operator's own limit on Q (ValueError, after the
    shapes); prior: the constant diagonal metric [Q] of geodesic_shoot, checked after `a`; frame: the vectors w [N,F,Q] of
    ard_rbf_point_transport, checked after the directions, and Q + 1 + F <= 64 where max_q is."""
    dirs = () if dirs is None else tuple(zip(('v', 'dx', 'dv'), dirs))
    wdir = () if frame is None else (('w', frame),)
    args = (('z', z), ('x', x)) + dirs + wdir + (('gamma', gamma), ('alpha', alpha), (name, a)) + (() if prior is None else (('prior', prior),))
    for nm, v in args:
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float64:
            raise TypeError('%s must be a float64 torch.Tensor' % nm)
    if z.dim() != 3 or min(z.shape) < 1:
        raise ValueError('z must be [K x M x Q], got %s' % (tuple(z.shape),))
    k, m, q = z.shape
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] != q:
        raise ValueError('x must be [N x Q] with Q = %d, got %s' % (q, tuple(x.shape)))
    for nm, v in dirs:
        if tuple(v.shape) != tuple(x.shape):
            raise ValueError('%s must be [N x Q] as x, got %s' % (nm, tuple(v.shape)))
    if frame is not None and (frame.dim() != 3 or frame.shape[0] != x.shape[0] or frame.shape[1] < 1 or frame.shape[2] != q):
        raise ValueError('w must be [N x F x Q] with N, Q as x and F >= 1, got %s' % (tuple(frame.shape),))
    if tuple(gamma.shape) != (k, q):
        raise ValueError('gamma must be [K x Q], got %s' % (tuple(gamma.shape),))
    if alpha.numel() != k:
        raise ValueError('alpha must be [K], got %s' % (tuple(alpha.shape),))
    if name == 'c':
        bad = a.dim() != 4 or a.shape[0] != k or a.shape[1] < 1 or a.shape[2] != m or a.shape[3] != m
    else:
        bad = a.dim() != 3 or a.shape[0] != k or a.shape[1] != m or a.shape[2] < 1 or (name == 'p' and a.shape[2] != m)
    if bad:
        raise ValueError('%s must be %s, got %s' % (name, what, tuple(a.shape)))
    if prior is not None and tuple(prior.shape) != (q,):
        raise ValueError('prior must be [Q], got %s' % (tuple(prior.shape),))
    if max_q is not None and q > max_q:
        raise ValueError('z must have Q <= %d, got Q = %d' % (max_q, q))
    if frame is not None and q + 1 + frame.shape[1] > 64:
        raise ValueError('z and w must have Q + 1 + F <= 64, got Q = %d, F = %d' % (q, frame.shape[1]))
    for nm, v in args:
        if not v.is_cuda or v.device != z.device:
            raise RuntimeError('%s must live on the GPU of z: dp_gp_lvm_amd runs its operators in HIP only' % nm)
    return z.contiguous(), x.contiguous(), gamma.contiguous(), alpha.reshape(-1).contiguous(), a.contiguous(), k, x.shape[0], m, q


def _point_call(op, dims, ins, outs):
    """dpgp_ard_rbf_point_<op>_f64(*dims, *ins, *outs, ws, ws_bytes, stream) with the workspace that its query asks for."""
    l = _lib.lib()
    wsb = getattr(l, 'dpgp_ard_rbf_point_%s_workspace_bytes' % op)(*dims)
    ws = _ws(wsb, ins[0].device)
    fn = 'dpgp_ard_rbf_point_%s_f64' % op
    _lib.check(getattr(l, fn)(*dims, *(t.data_ptr() for t in ins + outs), ws.data_ptr(), wsb, _stream()), fn)


def ard_rbf_point_metric(z, x, gamma, alpha, p):
    """The quadratic form of the derivative features at deterministic latent points (dpgp_ard_rbf_point_metric_f64): with
    b_kmq(x_n) = d k_km(x_n) / d x_q = -gamma_kq (x_nq - z_kmq) alpha_k exp(-1/2 sum_q gamma_kq (x_nq - z_kmq)^2) of the kernels
    z [K,M,Q], gamma [K,Q], alpha [K] at the points x [N,Q], returns
        g [K,N,Q,Q] = sum_{m,m'} p[k,m,m'] b_kmq(x_n) b_km'q'(x_n)          p [K,M,M], used as given (not symmetrised)
    The alpha diag(gamma) term of the expected metric is the caller's.  The features [K,N,M,Q] are never formed in memory; fixed
    summation order, the same bits on every run.  float64 tensors (TypeError) of these shapes (ValueError) on one GPU
    (RuntimeError)."""
    z, x, gamma, alpha, p, k, n, m, q = _point_metric_args(z, x, gamma, alpha, p, 'p', '[K x M x M]')
    g = torch.empty((k, n, q, q), dtype=torch.float64, device=z.device)
    _point_call('metric', (k, n, m, q), (z, x, gamma, alpha, p), (g,))
    return g


def ard_rbf_point_jacobian(z, x, gamma, alpha, r):
    """The derivative features contracted with weights (dpgp_ard_rbf_point_jacobian_f64): b as in ard_rbf_point_metric,
        jac [K,N,J,Q] = sum_m b_kmq(x_n) r[k,m,j]                            r [K,M,J]
    the Jacobian of the predictive means sum_m k_km(x_n) r[k,m,j] with respect to x_n.  Same rules as ard_rbf_point_metric."""
    z, x, gamma, alpha, r, k, n, m, q = _point_metric_args(z, x, gamma, alpha, r, 'r', '[K x M x J] with J >= 1')
    j = r.shape[2]
    jac = torch.empty((k, n, j, q), dtype=torch.float64, device=z.device)
    _point_call('jacobian', (k, j, n, m, q), (z, x, gamma, alpha, r), (jac,))
    return jac


def ard_rbf_point_energy(z, x, v, gamma, alpha, p):
    """The quadratic form of ard_rbf_point_metric along the directions v [N,Q] at the points x [N,Q], with both gradients
    (dpgp_ard_rbf_point_energy_f64): with b as there, c_knm = sum_q b_kmq(x_n) v_nq, returns (e, dx, dv),
        e [K,N] = sum_{m,m'} p[k,m,m'] c_knm c_knm' = v_n^T g[k,n] v_n,     dx [K,N,Q] = de/dx_n,     dv [K,N,Q] = de/dv_n
    p [K,M,M] is any matrix; the results depend on its symmetric part only.  The alpha diag(gamma) term of the expected metric
    is the caller's.  One launch, nothing of size N M in memory; fixed summation order, the same bits on every run.  float64
    tensors (TypeError) of these shapes (ValueError) on one GPU (RuntimeError)."""
    z, x, gamma, alpha, p, k, n, m, q = _point_metric_args(z, x, gamma, alpha, p, 'p', '[K x M x M]', dirs=(v,))
    v = v.contiguous()
    e = torch.empty((k, n), dtype=torch.float64, device=z.device)
    dx = torch.empty((k, n, q), dtype=torch.float64, device=z.device)
    dv = torch.empty_like(dx)
    _point_call('energy', (k, n, m, q), (z, x, v, gamma, alpha, p), (e, dx, dv))
    return e, dx, dv


def ard_rbf_point_christoffel(z, x, v, gamma, alpha, p):
    """The metric of ard_rbf_point_metric and its contracted Christoffel symbol along the velocities v [N,Q] at the points x [N,Q]
    (dpgp_ard_rbf_point_christoffel_f64): with b as there, k_km the kernel values and
        d_knm = v_n^T (d^2 k_km / dx dx)(x_n) v_n = k_km(x_n) [(sum_q gamma_kq (x_nq - z_kmq) v_nq)^2 - sum_q gamma_kq v_nq^2]
    returns (g, gam),
        g [K,N,Q,Q] = sum_{m,m'} p[k,m,m'] b_kmq(x_n) b_km'q'(x_n)           exactly ard_rbf_point_metric's quantity
        gam [K,N,Q] = sum_{m,m'} b_kmq(x_n) p[k,m,m'] d_knm'
    p [K,M,M] is used as given (not symmetrised).  For a SYMMETRIC p, gam is the Christoffel symbol of the first kind of g
    contracted twice with v, gam = (D_v g) v - 1/2 grad_x (v^T g v), so that a geodesic of G = G0 + sum_k g_k with constant G0
    obeys G x'' = -sum_k gam_k; for a non-symmetric p it is the sum above and no more.  One launch, nothing of size N M in
    memory; fixed summation order, the same bits on every run.  Q <= 63 (ValueError).  float64 tensors (TypeError) of these
    shapes (ValueError) on one GPU (RuntimeError)."""
    z, x, gamma, alpha, p, k, n, m, q = _point_metric_args(z, x, gamma, alpha, p, 'p', '[K x M x M]', dirs=(v,), max_q=63)
    v = v.contiguous()
    g = torch.empty((k, n, q, q), dtype=torch.float64, device=z.device)
    gam = torch.empty((k, n, q), dtype=torch.float64, device=z.device)
    _point_call('christoffel', (k, n, m, q), (z, x, v, gamma, alpha, p), (g, gam))
    return g, gam


def ard_rbf_point_christoffel_tangent(z, x, v, dx, dv, gamma, alpha, p):
    """ard_rbf_point_christoffel's pair and its derivative along a direction (dx, dv) [N,Q] of the state (x, v)
    (dpgp_ard_rbf_point_christoffel_tangent_f64): with u_q = gamma_kq (x_nq - z_kmq), k, b, d as there, a = sum_q u_q v_q and
        e = sum_q u_q dx_q,   f = sum_q u_q dv_q,   c1 = sum_q gamma_kq dx_q v_q,   c2 = sum_q gamma_kq v_q dv_q
        db_q = k (e u_q - gamma_kq dx_q),           dd = k (-e (a^2 - sum_q gamma_kq v_q^2) + 2 a (c1 + f) - 2 c2)
    returns (g, gam, dg, dgam),
        g [K,N,Q,Q], gam [K,N,Q]     the bits of ard_rbf_point_christoffel(z, x, v, gamma, alpha, p)
        dg [K,N,Q,Q] = db^T p b + b^T p db,        dgam [K,N,Q] = db^T p d + b^T p dd
    p [K,M,M] is used as given (not symmetrised); dg is symmetric for a symmetric p up to rounding.  One launch, all four results
    from one product over the feature block [b | d | db | dd]; nothing of size N M in memory; fixed summation order, the same
    bits on every run; exact zeros for a zero direction.  Q <= 31 (ValueError).  float64 tensors (TypeError) of these shapes
    (ValueError) on one GPU (RuntimeError)."""
    z, x, gamma, alpha, p, k, n, m, q = _point_metric_args(z, x, gamma, alpha, p, 'p', '[K x M x M]', dirs=(v, dx, dv), max_q=31)
    v, dx, dv = v.contiguous(), dx.contiguous(), dv.contiguous()
    g = torch.empty((k, n, q, q), dtype=torch.float64, device=z.device)
    gam = torch.empty((k, n, q), dtype=torch.float64, device=z.device)
    dg, dgam = torch.empty_like(g), torch.empty_like(gam)
    _point_call('christoffel_tangent', (k, n, m, q), (z, x, v, dx, dv, gamma, alpha, p), (g, gam, dg, dgam))
    return g, gam, dg, dgam


def ard_rbf_point_transport(z, x, v, w, gamma, alpha, p):
    """ard_rbf_point_christoffel's pair and the Christoffel symbols that move a frame of F vectors w [N,F,Q] along the velocities
    v [N,Q] (dpgp_ard_rbf_point_transport_f64): with u_q = gamma_kq (x_nq - z_kmq), k, b as there, a_v = sum_q u_q v_q and
        a_w = sum_q u_q w_q,     d(v, w) = v^T (d^2 k / dx dx) w = k (a_v a_w - sum_q gamma_kq v_q w_q)
    returns (g, gam, tgam),
        g [K,N,Q,Q], gam [K,N,Q]     the bits of ard_rbf_point_christoffel(z, x, v, gamma, alpha, p)
        tgam [K,N,F,Q] = sum_{m,m'} b_kmq(x_n) p[k,m,m'] d_knm'(v, w_r)
    p [K,M,M] is used as given (not symmetrised); for a SYMMETRIC p, tgam is the Christoffel symbol of the first kind of g
    contracted with v and w_r, so that parallel transport along a geodesic of G = G0 + sum_k g_k with velocity v obeys
    G w_r' = -sum_k tgam_k[r].  One launch, all three results from one product over the feature block [b | d(v,v) | d(v,w_1) ..
    d(v,w_F)]; nothing of size N M in memory; fixed summation order, the same bits on every run.  A vector's tgam depends
    neither on F, nor on its place in the frame, nor on the other vectors; for w_r = v it has the bits of gam; exact zeros for
    w_r = 0.  Q + 1 + F <= 64 (ValueError).  float64 tensors (TypeError) of these shapes (ValueError) on one GPU (RuntimeError)."""
    z, x, gamma, alpha, p, k, n, m, q = _point_metric_args(z, x, gamma, alpha, p, 'p', '[K x M x M]', dirs=(v,), frame=w)
    v, w = v.contiguous(), w.contiguous()
    f = w.shape[1]
    g = torch.empty((k, n, q, q), dtype=torch.float64, device=z.device)
    gam = torch.empty((k, n, q), dtype=torch.float64, device=z.device)
    tgam = torch.empty((k, n, f, q), dtype=torch.float64, device=z.device)
    _point_call('transport', (k, n, m, q, f), (z, x, v, w, gamma, alpha, p), (g, gam, tgam))
    return g, gam, tgam


def _accel_args(args):
    """The checks of geodesic_accel / geodesic_accel_tangent / geodesic_transport on (('g', g), ('gam', gam)[, ('dg', dg),
    ('dgam', dgam) or ('tgam', tgam)], ('prior', prior), ('v', v)): contiguous tensors in that order and (K, N, Q)."""
    for nm, t in args:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
            raise TypeError('%s must be a float64 torch.Tensor' % nm)
    g = args[0][1]
    if g.dim() != 4 or min(g.shape) < 1 or g.shape[2] != g.shape[3] or g.shape[3] > 64:
        raise ValueError('g must be [K x N x Q x Q] with Q <= 64, got %s' % (tuple(g.shape),))
    k, n, q = g.shape[0], g.shape[1], g.shape[2]
    want = dict(gam=((k, n, q), '[K x N x Q] as g'), dg=((k, n, q, q), '[K x N x Q x Q] as g'), dgam=((k, n, q), '[K x N x Q] as g'),
                prior=((q,), '[Q]'), v=((n, q), '[N x Q]'))
    for nm, t in args[1:]:
        if nm == 'tgam':
            if t.dim() != 4 or tuple(t.shape[:2]) != (k, n) or not 1 <= t.shape[2] <= 63 or t.shape[3] != q:
                raise ValueError('tgam must be [K x N x F x Q] with K, N, Q as g and 1 <= F <= 63, got %s' % (tuple(t.shape),))
        elif tuple(t.shape) != want[nm][0]:
            raise ValueError('%s must be %s, got %s' % (nm, want[nm][1], tuple(t.shape)))
    for nm, t in args:
        if not t.is_cuda or t.device != g.device:
            raise RuntimeError('%s must live on the GPU of g: dp_gp_lvm_amd runs its operators in HIP only' % nm)
    return [t.contiguous() for _, t in args], k, n, q


def geodesic_accel_tangent(g, gam, dg, dgam, prior, v):
    """geodesic_accel and its derivative from ard_rbf_point_christoffel_tangent's four results (dpgp_geodesic_accel_tangent_f64):
    returns (a, da, speed, info); a, speed and info carry the bits of geodesic_accel(g, gam, prior, v), and with the same factor
        da [N,Q] = -G_n^-1 (sum_k dgam[k,n] + (sum_k dg[k,n]) a_n)            (k ascending; the constant prior drops out)
    the derivative of the acceleration along the direction that dg, dgam were taken in.  info[n] != 0: a[n, :] and da[n, :] are
    NaN and the other points are unaffected.  dg [K,N,Q,Q], dgam [K,N,Q]; everything else as geodesic_accel."""
    (g, gam, dg, dgam, prior, v), k, n, q = _accel_args((('g', g), ('gam', gam), ('dg', dg), ('dgam', dgam), ('prior', prior),
                                                          ('v', v)))
    a = torch.empty((n, q), dtype=torch.float64, device=g.device)
    da = torch.empty_like(a)
    speed = torch.empty((n,), dtype=torch.float64, device=g.device)
    info = torch.empty((n,), dtype=torch.int32, device=g.device)
    _lib.check(_lib.lib().dpgp_geodesic_accel_tangent_f64(k, n, q, g.data_ptr(), gam.data_ptr(), dg.data_ptr(), dgam.data_ptr(),
                                                          prior.data_ptr(), v.data_ptr(), a.data_ptr(), da.data_ptr(),
                                                          speed.data_ptr(), info.data_ptr(), _stream()),
               'dpgp_geodesic_accel_tangent_f64')
    return a, da, speed, info


def geodesic_transport(g, gam, tgam, prior, v):
    """geodesic_accel and the rates of a frame in parallel transport from ard_rbf_point_transport's three results
    (dpgp_geodesic_transport_f64): returns (a, dw, speed, info); a, speed and info carry the bits of
    geodesic_accel(g, gam, prior, v), and with the same factor
        dw [N,F,Q] = -G_n^-1 sum_k tgam[k,n,r]                                (k ascending; the constant prior enters G only)
    all 1 + F right-hand sides in one pair of substitutions.  Where tgam[:, n, r] has the bits of gam[:, n], dw[n, r] has the
    bits of a[n].  info[n] != 0: a[n, :] and dw[n, :, :] are NaN and the other points are unaffected.  tgam [K,N,F,Q] with
    F <= 63; everything else as geodesic_accel."""
    (g, gam, tgam, prior, v), k, n, q = _accel_args((('g', g), ('gam', gam), ('tgam', tgam), ('prior', prior), ('v', v)))
    f = tgam.shape[2]
    a = torch.empty((n, q), dtype=torch.float64, device=g.device)
    dw = torch.empty((n, f, q), dtype=torch.float64, device=g.device)
    speed = torch.empty((n,), dtype=torch.float64, device=g.device)
    info = torch.empty((n,), dtype=torch.int32, device=g.device)
    _lib.check(_lib.lib().dpgp_geodesic_transport_f64(k, n, q, f, g.data_ptr(), gam.data_ptr(), tgam.data_ptr(), prior.data_ptr(),
                                                      v.data_ptr(), a.data_ptr(), dw.data_ptr(), speed.data_ptr(), info.data_ptr(),
                                                      _stream()), 'dpgp_geodesic_transport_f64')
    return a, dw, speed, info


def geodesic_accel(g, gam, prior, v):
    """The acceleration of the geodesic equation from ard_rbf_point_christoffel's pair (dpgp_geodesic_accel_f64): per point, with
    G_n = sum_k g[k,n] + diag(prior) (k ascending), returns (a, speed, info),
        a [N,Q] = -G_n^-1 sum_k gam[k,n],     speed [N] = v_n^T G_n v_n,     info [N] int32
    by one Cholesky factorisation per point (the lower triangle of G_n is read) in one launch.  info[n] = 0, or the 1-based index
    of the first pivot that is not positive: a[n, :] is then NaN and the other points are unaffected.  g [K,N,Q,Q], gam [K,N,Q],
    prior [Q], v [N,Q] with Q <= 64.  No atomics, nothing read on the host, the same bits on every run.  float64 tensors
    (TypeError) of these shapes (ValueError) on one GPU (RuntimeError)."""
    (g, gam, prior, v), k, n, q = _accel_args((('g', g), ('gam', gam), ('prior', prior), ('v', v)))
    a = torch.empty((n, q), dtype=torch.float64, device=g.device)
    speed = torch.empty((n,), dtype=torch.float64, device=g.device)
    info = torch.empty((n,), dtype=torch.int32, device=g.device)
    _lib.check(_lib.lib().dpgp_geodesic_accel_f64(k, n, q, g.data_ptr(), gam.data_ptr(), prior.data_ptr(), v.data_ptr(),
                                                  a.data_ptr(), speed.data_ptr(), info.data_ptr(), _stream()),
               'dpgp_geodesic_accel_f64')
    return a, speed, info


def _shoot(parts, prior, states, num_steps, tangent):
    """The checks and the call of geodesic_shoot / geodesic_shoot_tangent.  parts: a non-empty list (TypeError; at most 64,
    ValueError) of (z [K_i,M_i,Q], gamma [K_i,Q], alpha [K_i], p [K_i,M_i,M_i]), each checked as
    ard_rbf_point_christoffel[_tangent] checks it next to the states (x, v[, dx, dv]) [C,Q] and prior [Q]; num_steps >= 1
    (ValueError)."""
    if not isinstance(parts, (list, tuple)) or not parts or any(not isinstance(pt, (list, tuple)) or len(pt) != 4 for pt in parts):
        raise TypeError('parts must be a non-empty list of (z, gamma, alpha, p)')
    if len(parts) > 64:
        raise ValueError('parts must have at most 64 entries, got %d' % len(parts))
    num_steps = int(num_steps)
    if num_steps < 1:
        raise ValueError('num_steps must be >= 1, got %d' % num_steps)
    if prior is None:
        raise TypeError('prior must be a float64 torch.Tensor')
    x, dirs = states[0], tuple(states[1:])
    kept, ks, ms, off_gpu = [], [], [], None
    for z, gamma, alpha, p in parts:
        try:
            z, xc, gamma, alpha, p, k, c, m, q = _point_metric_args(z, x, gamma, alpha, p, 'p', '[K x M x M]', dirs=dirs,
                                                                    max_q=31 if tangent else 63, prior=prior)
        except RuntimeError as err:          # (the types and shapes of the later parts come before any part's device)
            off_gpu = off_gpu or err
            continue
        kept.append((z, gamma, alpha, p))
        ks.append(k)
        ms.append(m)
    if off_gpu is not None:
        raise off_gpu
    if any(pt[0].device != xc.device for pt in kept):
        raise RuntimeError('every part must live on the GPU of x: dp_gp_lvm_amd runs its operators in HIP only')
    prior = prior.contiguous()
    states = [xc] + [d.contiguous() for d in dirs]
    rows = [torch.empty((c, num_steps + 1, q), dtype=torch.float64, device=xc.device) for _ in states]
    bad = torch.empty((c,), dtype=torch.int32, device=xc.device)
    speed0 = [torch.empty((c,), dtype=torch.float64, device=xc.device)] if tangent else []
    n = len(kept)
    ints = ctypes.c_int * n
    ptrs = ctypes.c_void_p * n
    ka, ma = ints(*ks), ints(*ms)
    lists = [ptrs(*(pt[j].data_ptr() for pt in kept)) for j in range(4)]
    l = _lib.lib()
    wsb = l.dpgp_geodesic_shoot_workspace_bytes(n, ka, ma, q, c, int(tangent))
    ws = _ws(wsb, xc.device)
    fn = 'dpgp_geodesic_shoot_tangent_f64' if tangent else 'dpgp_geodesic_shoot_f64'
    _lib.check(getattr(l, fn)(n, ka, ma, q, c, num_steps, *lists, prior.data_ptr(), *(t.data_ptr() for t in states),
                              *(t.data_ptr() for t in rows), bad.data_ptr(), *(t.data_ptr() for t in speed0), ws.data_ptr(), wsb,
                              _stream()), fn)
    return tuple(rows) + (bad,) + tuple(speed0)


def geodesic_shoot(parts, prior, x, v, num_steps):
    """The exponential map on the device (dpgp_geodesic_shoot_f64): the classical RK4 solution of (x', v') = (v, -G^-1 Gamma) on
    t in [0, 1] at step 1 / num_steps for the C curves from x [C,Q] with the velocities v [C,Q], under the metric
    G = sum over parts and their kernels of g + diag(prior): parts is a list of (z [K_i,M_i,Q], gamma [K_i,Q], alpha [K_i],
    p [K_i,M_i,M_i]), the operands of ard_rbf_point_christoffel, prior [Q].  Returns (curve, vel [C,S+1,Q], bad [C] int32): the
    BITS of models/geodesic.exp_map's loop on ard_rbf_point_christoffel (the parts' slabs concatenated) and geodesic_accel;
    bad counts the stages whose metric failed to factor (NaN in that curve from there on, the others unaffected).  One C call:
    4 S (parts + 1) launches, nothing allocated or added by torch between stages, nothing read on the host.  Q <= 63.  float64
    tensors (TypeError) of these shapes (ValueError) on one GPU (RuntimeError)."""
    return _shoot(parts, prior, (x, v), num_steps, False)


def geodesic_shoot_tangent(parts, prior, x, v, dx, dv, num_steps):
    """geodesic_shoot with its tangent-linear solution from (dx, dv) [C,Q] (dpgp_geodesic_shoot_tangent_f64): returns
    (curve, vel, dcurve, dvel [C,S+1,Q], bad [C] int32, speed0 [C]), the BITS of models/geodesic._rk4_tangent on
    ard_rbf_point_christoffel_tangent and geodesic_accel_tangent; speed0 = v^T G(x) v at the start.  Q <= 31; everything else as
    geodesic_shoot."""
    return _shoot(parts, prior, (x, v, dx, dv), num_steps, True)


def ard_rbf_point_cov(z, x, gamma, alpha, c):
    """The joint posterior covariance at deterministic latent points (dpgp_ard_rbf_point_cov_f64): with the features
    k_km(x_n) = alpha_k exp(-1/2 sum_q gamma_kq (x_nq - z_kmq)^2) of the kernels z [K,M,Q], gamma [K,Q], alpha [K] at the points
    x [N,Q], returns
        out [K,G,N,N] = alpha_k exp(-1/2 sum_q gamma_kq (x_iq - x_jq)^2) - sum_{m,m'} k_km(x_i) c[k,g,m,m'] k_km'(x_j)
    c [K,G,M,M] with G >= 1 is any set of matrices; the result depends on their symmetric parts only and is exactly symmetric in
    (i, j).  One launch, the features shared by the G patterns of a kernel, nothing of size N M in memory; fixed summation order,
    the same bits on every run.  N <= 46340.  float64 tensors (TypeError) of these shapes (ValueError) on one GPU (RuntimeError)."""
    z, x, gamma, alpha, c, k, n, m, q = _point_metric_args(z, x, gamma, alpha, c, 'c', '[K x G x M x M] with G >= 1')
    g = c.shape[1]
    out = torch.empty((k, g, n, n), dtype=torch.float64, device=z.device)
    _point_call('cov', (k, g, n, m, q), (z, x, gamma, alpha, c), (out,))
    return out


def ard_rbf_diag(n, alpha, beta, include_noise=False, include_jitter=False, jitter=1e-8):
    """Kernel.covariance_diag -> [B,N]  (rbf_kernel.py:96-116)."""
    dt = _dtype_of(alpha)
    alpha = _prep(alpha, dt, 'alpha').reshape(-1)
    beta = _prep(beta, dt, 'beta').reshape(-1)
    b = alpha.numel()
    out = torch.empty((b, int(n)), dtype=dt, device=alpha.device)
    flags = (_lib.FLAG_NOISE if include_noise else 0) | (_lib.FLAG_JITTER if include_jitter else 0)
    name = 'dpgp_ard_rbf_diag_' + _SUFFIX[dt]
    _lib.check(getattr(_lib.lib(), name)(b, int(n), alpha.data_ptr(), beta.data_ptr(), flags, float(jitter),
                                         out.data_ptr(), _stream()), name)
    return out


def psi0(n, alpha):
    """Kernel.psi_0 -> [B,1]  (rbf_kernel.py:119-132)."""
    dt = _dtype_of(alpha)
    alpha = _prep(alpha, dt, 'alpha').reshape(-1)
    out = torch.empty((alpha.numel(), 1), dtype=dt, device=alpha.device)
    name = 'dpgp_psi0_' + _SUFFIX[dt]
    _lib.check(getattr(_lib.lib(), name)(alpha.numel(), int(n), alpha.data_ptr(), out.data_ptr(), _stream()), name)
    return out


def _zms(z, mu, s, gamma, alpha):
    dt = _dtype_of(mu)
    z, mu, s = _prep(z, dt, 'inducing_input'), _prep(mu, dt, 'latent_input_mean'), _prep(s, dt, 'latent variance')
    gamma, alpha, _, b = _hyp(gamma, alpha, None, dt)
    q = gamma.shape[1]
    assert z.dim() == 2 and z.shape[1] == q, 'inducing_input must be [M x Q]'
    assert mu.dim() == 2 and mu.shape[1] == q, 'latent_input_mean must be [N x Q]'
    assert s.shape == mu.shape, 'latent variances must be [N x Q]'
    return dt, z, mu, s, gamma, alpha, b, mu.shape[0], z.shape[0], q


def psi1(z, mu, s, gamma, alpha):
    """Kernel.psi_1 -> [B,N,M]  (rbf_kernel.py:135-161)."""
    dt, z, mu, s, gamma, alpha, b, n, m, q = _zms(z, mu, s, gamma, alpha)
    out = torch.empty((b, n, m), dtype=dt, device=mu.device)
    name = 'dpgp_psi1_' + _SUFFIX[dt]
    _lib.check(getattr(_lib.lib(), name)(b, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                         alpha.data_ptr(), out.data_ptr(), _stream()), name)
    return out


def psi1T_y(z, mu, s, gamma, alpha, y):
    """Psi1_b^T y_b -> [B,M] without materialising Psi1 (dp_gp_lvm.py:132-145)."""
    dt, z, mu, s, gamma, alpha, b, n, m, q = _zms(z, mu, s, gamma, alpha)
    y = _prep(y, dt, 'y')
    assert y.shape == (n, b), 'y must be [N x B]'
    out = torch.empty((b, m), dtype=dt, device=mu.device)
    l = _lib.lib()
    wsb = l.dpgp_psi1T_y_workspace_bytes(b, n, m)
    ws = _ws(wsb, mu.device)
    name = 'dpgp_psi1T_y_' + _SUFFIX[dt]
    _lib.check(getattr(l, name)(b, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                alpha.data_ptr(), y.data_ptr(), y.stride(0), out.data_ptr(), ws.data_ptr(), wsb,
                                _stream()), name)
    return out


def psi2(z, mu, s, gamma, alpha, algo='auto', weights=None):
    """Kernel.psi_2 -> [B,M,M]  (rbf_kernel.py:164-199), streamed over n on the matrix cores.
    weights [B,N] (fp64 only; algo 'auto' or 'plain'): out[b] = sum_n weights[b,n] psi2_bn (dpgp_psi2_weighted_f64).  The weights
    must be >= 0 and finite — behaviour for negative weights is unspecified; a weight of 0 contributes exactly 0.0."""
    dt, z, mu, s, gamma, alpha, b, n, m, q = _zms(z, mu, s, gamma, alpha)
    out = torch.empty((b, m, m), dtype=dt, device=mu.device)
    l = _lib.lib()
    wsb = l.dpgp_psi2_workspace_bytes(b, n, m, q, out.element_size())
    ws = _ws(wsb, mu.device)
    if weights is not None:
        assert dt == torch.float64, 'weighted Psi2 is an fp64 operator'
        weights = _qx_weights(weights, b, n, mu)
        _lib.check(l.dpgp_psi2_weighted_f64(b, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                            alpha.data_ptr(), weights.data_ptr(), out.data_ptr(), ws.data_ptr(), wsb,
                                            _lib.ALGO[algo], _stream()), 'dpgp_psi2_weighted_f64')
        return out
    name = 'dpgp_psi2_' + _SUFFIX[dt]
    _lib.check(getattr(l, name)(b, n, m, q, z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(),
                                alpha.data_ptr(), out.data_ptr(), ws.data_ptr(), wsb, _lib.ALGO[algo], _stream()), name)
    return out


def potrf_batched(a, algo='auto'):
    """tf.cholesky on [B,M,M] -> (L [B,M,M] lower, info [B] int32)  (dp_gp_lvm.py:116,127)."""
    dt = _dtype_of(a)
    assert a.dim() == 3 and a.shape[1] == a.shape[2], 'a must be [B x M x M]'
    l_ = _prep(a, dt, 'a').clone()
    b, m = l_.shape[0], l_.shape[1]
    info = torch.empty(b, dtype=torch.int32, device=a.device)
    l = _lib.lib()
    wsb = l.dpgp_potrf_workspace_bytes(b, m, l_.element_size())
    ws = _ws(wsb, a.device)
    name = 'dpgp_potrf_batched_' + _SUFFIX[dt]
    _lib.check(getattr(l, name)(b, m, l_.data_ptr(), info.data_ptr(), ws.data_ptr(), wsb, _lib.ALGO[algo], _stream()),
               name)
    return l_, info


def trsm_batched(l_, rhs, algo='auto'):
    """tf.matrix_triangular_solve(l, rhs, lower=True) on [B,M,M], [B,M,K] -> [B,M,K]  (dp_gp_lvm.py:118-121)."""
    dt = _dtype_of(l_)
    l_ = _prep(l_, dt, 'l')
    x = _prep(rhs, dt, 'rhs').clone()
    assert l_.dim() == 3 and x.dim() == 3 and l_.shape[0] == x.shape[0] and l_.shape[1] == l_.shape[2] == x.shape[1]
    b, m, k = x.shape
    l = _lib.lib()
    wsb = l.dpgp_trsm_workspace_bytes(b, m, k, x.element_size())
    ws = _ws(wsb, x.device)
    name = 'dpgp_trsm_batched_' + _SUFFIX[dt]
    _lib.check(getattr(l, name)(b, m, k, l_.data_ptr(), x.data_ptr(), ws.data_ptr(), wsb, _lib.ALGO[algo], _stream()),
               name)
    return x


def tril_inverse_batched(l_):
    """tf.matrix_triangular_solve(l, eye, lower=True) on [B,M,M] fp64 -> L^-1 [B,M,M] (lower, zeros above the diagonal).  M a multiple
    of 128: one persistent-workgroup launch (dpgp_trtri_lower_batched_f64); otherwise dpgp_trsm_batched on the identity."""
    f64 = torch.float64
    l_ = _prep(l_, f64, 'l')
    b, m = l_.shape[0], l_.shape[1]
    assert l_.dim() == 3 and l_.shape[2] == m
    if m % 128 != 0:
        return trsm_batched(l_, torch.eye(m, dtype=f64, device=l_.device).expand(b, m, m).contiguous())
    out = torch.empty_like(l_)
    ws = _ws(8 * b, l_.device)
    _lib.check(_lib.lib().dpgp_trtri_lower_batched_f64(b, m, l_.data_ptr(), out.data_ptr(), ws.data_ptr(), 8 * b, _stream()),
               'dpgp_trtri_lower_batched_f64')
    return out


def matmul(a, b, out=None, alpha=1.0, beta=0.0):
    """tf.matmul on fp64 device tensors of 2 or 3 dimensions (batch broadcast as in TensorFlow / torch.matmul), through the
    library's strided batched MFMA kernel (dpgp_gemm_strided_f64): transposed or sliced VIEWS are passed by their strides, no
    copies and no rocBLAS.  The reference's call sites: dp_gp_lvm.py:657-658 and the composed chains around it.
    out (optional, [batch, m, n] or [m, n]): out = alpha a b + beta out."""
    f64 = torch.float64
    for t, name in ((a, 'a'), (b, 'b')):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != f64:
            raise TypeError('%s must be a float64 tensor on the GPU (dp_gp_lvm_amd has no host path)' % name)
        if t.dim() not in (2, 3):
            raise ValueError('%s must have 2 or 3 dimensions' % name)
    m, k, n = a.shape[-2], a.shape[-1], b.shape[-1]
    if b.shape[-2] != k:
        raise ValueError('inner dimensions differ: %s x %s' % (tuple(a.shape), tuple(b.shape)))
    ba = a.shape[0] if a.dim() == 3 else 1
    bb = b.shape[0] if b.dim() == 3 else 1
    if ba != bb and ba != 1 and bb != 1:
        raise ValueError('batch dimensions differ: %s x %s' % (tuple(a.shape), tuple(b.shape)))
    batch = max(ba, bb)
    three = a.dim() == 3 or b.dim() == 3
    if out is None:
        if beta != 0.0:
            raise ValueError('beta needs out')
        out = torch.empty((batch, m, n) if three else (m, n), dtype=f64, device=a.device)
    else:
        assert out.dtype == f64 and out.is_cuda and tuple(out.shape) == ((batch, m, n) if three else (m, n))
    if m == 0 or n == 0:
        return out
    a_sb = a.stride(0) if (a.dim() == 3 and ba > 1) else 0
    b_sb = b.stride(0) if (b.dim() == 3 and bb > 1) else 0
    c_sb = out.stride(0) if three else 0
    _lib.check(_lib.lib().dpgp_gemm_strided_f64(batch, m, n, k, float(alpha), a.data_ptr(), a_sb, a.stride(-2), a.stride(-1),
                                                b.data_ptr(), b_sb, b.stride(-2), b.stride(-1), float(beta), out.data_ptr(),
                                                c_sb, out.stride(-2), out.stride(-1), _stream()), 'dpgp_gemm_strided_f64')
    return out


def kl_qx(mu, s):
    """calculate_kl_divergence_standard_prior -> 0-d fp64 tensor  (gp_expressions.py:10-24)."""
    dt = _dtype_of(mu)
    mu, s = _prep(mu, dt, 'x_mean'), _prep(s, dt, 'x_var')
    assert mu.shape == s.shape and mu.dim() == 2
    out = torch.empty(1, dtype=torch.float64, device=mu.device)
    name = 'dpgp_kl_qx_' + _SUFFIX[dt]
    _lib.check(getattr(_lib.lib(), name)(mu.shape[0], mu.shape[1], mu.data_ptr(), s.data_ptr(), out.data_ptr(),
                                         _stream()), name)
    return out[0]


class ElboWorkspace:
    """Caller-owned scratch + outputs of the fused ELBO for one (D,N,M,Q,prec): allocate once, evaluate many times."""

    def __init__(self, d, n, m, q, prec='mixed', device='cuda'):
        self.shape, self.prec = (d, n, m, q), prec
        l = _lib.lib()
        self.nbytes = l.dpgp_elbo_workspace_bytes(d, n, m, q, _lib.PREC[prec])
        self.ws = _ws(self.nbytes, device)
        # (before the first evaluation: NaN terms and zero flags, not whatever the allocator hands out)
        self.terms = torch.full((d, 5), float('nan'), dtype=torch.float64, device=device)
        self.sums = torch.full((2,), float('nan'), dtype=torch.float64, device=device)
        self.info = torch.zeros(d, dtype=torch.int32, device=device)
        self.exec = _lib.ExecResources()
        # second stream + fork / join events: Psi1^T y beside the psi2 launch (include/dpgp.h, dpgp_exec_t.stream_aux).
        # Opt-in (DPGP_PARALLEL_BRANCH=1): measured on MI355X it is SLOWER than one stream — config 2: 0.263 vs 0.253 ms per
        # evaluation, config 3: 1.371 vs 1.298, replayed from a HIP graph 0.345 — the two event hand-offs cost more than the
        # 12 us (D = 64) the branch could hide, and the psi2 launch fills the chip on its own.
        import os
        if os.environ.get('DPGP_PARALLEL_BRANCH', '0') == '1':
            self.exec.stream_aux, self.exec.ev_fork, self.exec.ev_join = l.dpgp_stream_create(), l.dpgp_event_create(), l.dpgp_event_create()
        import ctypes
        lay = (ctypes.c_size_t * 10)()
        _lib.check(l.dpgp_elbo_workspace_layout(d, n, m, q, _lib.PREC[prec], ctypes.cast(lay, ctypes.c_void_p)),
                   'dpgp_elbo_workspace_layout')
        self.layout = tuple(int(v) for v in lay)
        # guard[d]: bound on what the rounding of an fp32 Psi2 can do to output dim d's terms (include/dpgp.h,
        # DPGP_INFO_ILL_CONDITIONED); a view into the workspace, valid after an evaluation
        self.guard = self.ws[self.layout[8]:self.layout[8] + 8 * d].view(torch.float64)
        flay = (ctypes.c_size_t * 6)()
        _lib.check(l.dpgp_elbo_workspace_front_layout(d, n, m, q, _lib.PREC[prec], ctypes.cast(flay, ctypes.c_void_p)),
                   'dpgp_elbo_workspace_front_layout')
        self.front_layout = tuple(int(v) for v in flay)

    def kuu(self):
        """K_uu + jitter I [D,M,M] as the front launch of the last ``elbo_fhat`` left it: a strided view into the workspace."""
        d, _, m, _ = self.shape
        off, stride, elem, mp, _, _ = self.front_layout
        dt = torch.float32 if elem == 4 else torch.float64
        flat = self.ws[off:off + stride * d].view(dt)
        return flat.as_strided((d, m, m), (stride // elem, mp, 1))

    def pair_factors(self):
        """The pair factors alpha_d^2 exp(-r^2 / 4) the last ``elbo_fhat`` (algo 'auto') left for the pair-tile Psi2 kernel, unpacked
        from its table to [D,M,M] fp32 (entries m' <= m; zeros above the diagonal), or None where that kernel does not run (fp64
        Psi2, Q > 21)."""
        d, _, m, _ = self.shape
        off, ppad = self.front_layout[4], self.front_layout[5]
        if ppad == 0:
            return None
        tab = self.ws[off:off + 4 * d * ppad].view(torch.float32).view(d, ppad)
        rows, cols = torch.tril_indices(m, m, device=self.ws.device)
        out = torch.zeros((d, m, m), dtype=torch.float32, device=self.ws.device)
        out[:, rows, cols] = tab[:, rows * (rows + 1) // 2 + cols]
        return out

    def __del__(self):
        try:
            l = _lib.lib()
            if self.exec.stream_aux:
                l.dpgp_stream_destroy(self.exec.stream_aux)
                l.dpgp_event_destroy(self.exec.ev_fork)
                l.dpgp_event_destroy(self.exec.ev_join)
                self.exec.stream_aux = None
        except Exception:                                        # (interpreter shutdown)
            pass


def elbo_fhat(y, z, mu, s, gamma, alpha, beta, jitter=1e-8, prec='mixed', algo='auto', workspace=None, events=None,
              model_tail=None):
    """
    The fused per-output ELBO reduction of dp_gp_lvm.py:108-148 for the D output dims in ``y`` [N,D] (a column slice of
    the full data when D is sharded over GPUs).  All inputs fp64 device tensors.
    Returns (terms [D,5], sums [2] = (f_hat, KL), info [D]) — device tensors, no host synchronisation.
    """
    f64 = torch.float64
    z, mu, s = _prep(z, f64, 'z'), _prep(mu, f64, 'mu'), _prep(s, f64, 's')
    gamma, alpha, beta, d = _hyp(gamma, alpha, beta, f64)
    if not y.is_cuda:
        raise RuntimeError('y must live on the GPU')
    if y.dtype != f64 or y.stride(1) != 1:
        y = y.to(f64).contiguous()
    n, m, q = mu.shape[0], z.shape[0], z.shape[1]
    assert y.shape == (n, d), 'y must be [N x D]'
    assert mu.shape == (n, q) and s.shape == (n, q) and gamma.shape == (d, q)
    w = workspace if workspace is not None else ElboWorkspace(d, n, m, q, prec, y.device)
    assert w.shape == (d, n, m, q) and w.prec == prec, 'workspace was sized for another problem'
    ev0, ev1 = events if events is not None else (None, None)     # optional hipEvent handles around the psi2 kernel
    w.exec.ev_psi2_begin, w.exec.ev_psi2_end = ev0, ev1
    # model_tail = (scal, pack, out) device tensors (out may be None): fold dpgp_model_pack / _finalize into the last launch
    w.exec.model_scal, w.exec.model_pack, w.exec.model_out = (
        (None, None, None) if model_tail is None else
        tuple(None if t_ is None else t_.data_ptr() for t_ in model_tail))
    import ctypes
    _lib.check(_lib.lib().dpgp_elbo_fhat_ex(d, n, m, q, y.data_ptr(), y.stride(0), z.data_ptr(), mu.data_ptr(),
                                            s.data_ptr(), gamma.data_ptr(), alpha.data_ptr(), beta.data_ptr(),
                                            float(jitter), _lib.PREC[prec], _lib.ALGO[algo], w.terms.data_ptr(),
                                            w.sums.data_ptr(), w.info.data_ptr(), w.ws.data_ptr(), w.nbytes,
                                            _stream(), ctypes.cast(ctypes.pointer(w.exec), ctypes.c_void_p)),
               'dpgp_elbo_fhat_ex')
    return w.terms, w.sums, w.info


class ElboTWorkspace:
    """Device buffers of ``elbo_fhat_t`` for one problem shape (allocated once, reused by every evaluation)."""

    def __init__(self, t, d, n, m, q, prec, device):
        nbytes = int(_lib.lib().dpgp_elbo_fhat_t_workspace_bytes(t, d, n, m, q, _lib.PREC[prec]))
        if nbytes == 0:
            raise ValueError('elbo_fhat_t: unsupported shape / precision (T=%d D=%d N=%d M=%d Q=%d %s)' % (t, d, n, m, q, prec))
        self.shape, self.prec, self.nbytes = (t, d, n, m, q), prec, nbytes
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.per_t = torch.empty(t, dtype=torch.float64, device=device)
        self.quad = torch.empty((t, d), dtype=torch.float64, device=device)
        self.sums = torch.empty(2, dtype=torch.float64, device=device)
        self.info = torch.empty(t, dtype=torch.int32, device=device)
        # second stream + fork / join events: Psi1 and Psi1^T Y beside the fused reduction on the atoms (include/dpgp.h);
        # DPGP_PARALLEL_BRANCH_T=0 keeps one stream
        import os
        l = _lib.lib()
        self.aux = (l.dpgp_stream_create(), l.dpgp_event_create(), l.dpgp_event_create()) \
            if os.environ.get('DPGP_PARALLEL_BRANCH_T', '1') != '0' else (None, None, None)

    def __del__(self):
        try:
            if self.aux[0]:
                l = _lib.lib()
                l.dpgp_stream_destroy(self.aux[0])
                l.dpgp_event_destroy(self.aux[1])
                l.dpgp_event_destroy(self.aux[2])
                self.aux = (None, None, None)
        except Exception:
            pass


def elbo_fhat_t_supported(m):
    """dpgp_elbo_fhat_t keeps the factors L_B,t in LDS (first version): M <= 128."""
    return 16 * ((int(m) + 15) // 16) <= 128


def elbo_fhat_t(y, yy, z, mu, s, gamma_atoms, alpha_atoms, beta_atoms, phit, jitter=1e-8, prec='mixed', workspace=None,
                model_tail=None):
    """
    f_hat of the over-T model (reference dp_gp_lvm.py:608-676) for the D output dims in ``y`` [N,D]: T atoms, each solved against
    all D columns, weighted by ``phit`` [T,D] (any strides: phi[D,T].t() is read in place).  ``yy`` [D] = column sums of y^2.
    All inputs fp64 device tensors.  model_tail = (scal, pack, out) as for ``elbo_fhat``.
    Returns (per_t [T], quad [T,D], sums [2] = (f_hat, KL), info [T]) — device tensors, no host synchronisation (nine launches).
    """
    f64 = torch.float64
    z, mu, s = _prep(z, f64, 'z'), _prep(mu, f64, 'mu'), _prep(s, f64, 's')
    gamma, alpha, beta, t = _hyp(gamma_atoms, alpha_atoms, beta_atoms, f64)
    if not y.is_cuda:
        raise RuntimeError('y must live on the GPU')
    if y.dtype != f64 or y.stride(1) != 1:
        y = y.to(f64).contiguous()
    n, d = y.shape
    m, q = z.shape
    yy = _prep(yy, f64, 'yy').reshape(-1)
    if not phit.is_cuda or phit.dtype != f64:
        raise RuntimeError('phit must be an fp64 GPU tensor')
    assert mu.shape == (n, q) and s.shape == (n, q) and gamma.shape == (t, q)
    assert yy.numel() == d and phit.shape == (t, d), 'yy must be [D], phit [T x D]'
    w = workspace if workspace is not None else ElboTWorkspace(t, d, n, m, q, prec, y.device)
    assert w.shape == (t, d, n, m, q) and w.prec == prec, 'workspace was sized for another problem'
    tail = (None, None, None) if model_tail is None else tuple(None if t_ is None else t_.data_ptr() for t_ in model_tail)
    _lib.check(_lib.lib().dpgp_elbo_fhat_t(t, d, n, m, q, y.data_ptr(), y.stride(0), yy.data_ptr(), z.data_ptr(), mu.data_ptr(),
                                           s.data_ptr(), gamma.data_ptr(), alpha.data_ptr(), beta.data_ptr(), phit.data_ptr(),
                                           phit.stride(0), phit.stride(1), float(jitter), _lib.PREC[prec], w.per_t.data_ptr(),
                                           w.quad.data_ptr(), w.sums.data_ptr(), w.info.data_ptr(), w.ws.data_ptr(), w.nbytes,
                                           _stream(), *tail, *w.aux),
               'dpgp_elbo_fhat_t')
    return w.per_t, w.quad, w.sums, w.info


def elbo_step_supported(m, q):
    """Where the models take dpgp_elbo_step: B_d in LDS (M <= 128) and Q <= 20.  The Q bound is this function's choice (the step was
    tuned and measured up to the BASELINE configs' Q = 20), not the kernels' limit: the pair-tile form of stage B, and with it
    dpgp_elbo_step, takes Q <= 21 (psi2_pgrad_supported, csrc/psi2_pairs_grad.hip); at Q = 21 the models take the three calls."""
    return 16 * ((int(m) + 15) // 16) <= 128 and int(q) <= 20


class ElboStepBuffers:
    """Outputs and stage-B workspace of ``elbo_step`` for one problem shape (allocated once: the workspace holds the operand images
    and the results of the two passes, ~1.6 GB at N=2000, D=512, M=128, Q=10)."""

    def __init__(self, d, n, m, q, device):
        f64 = torch.float64
        mp = 16 * ((m + 15) // 16)
        self.shape = (d, n, m, q)
        if mp <= 128:                                            # (stage A outputs of the one-call step; M > 128: the caller's)
            self.gp = torch.empty((d, mp, mp), dtype=f64, device=device)
            self.wk = torch.empty((d, mp, mp), dtype=f64, device=device)
            self.gv = torch.empty((d, mp), dtype=f64, device=device)
            self.dab = torch.empty((d, 2), dtype=f64, device=device)
            self.info = torch.empty(d, dtype=torch.int32, device=device)
        self.nbytes = int(_lib.lib().dpgp_elbo_grad_psi_workspace_bytes_ex(d, n, m, q, _lib.PREC['mixed']))
        self.ws = _ws(self.nbytes, device)
        self.dmu, self.ds = torch.empty((n, q), dtype=f64, device=device), torch.empty((n, q), dtype=f64, device=device)
        self.dz, self.dg = torch.empty((m, q), dtype=f64, device=device), torch.empty((d, q), dtype=f64, device=device)
        # second stream + fork / join events of the one-call step: Psi1^T y and the K_uu branch (in a step the latter is a launch of its
        # own) run beside the image build and the head of pass 1.  DPGP_STEP_AUX=0 keeps one stream.
        import os
        self.aux = None
        if mp <= 128 and os.environ.get('DPGP_STEP_AUX', '1') != '0':
            l = _lib.lib()
            self.aux = (l.dpgp_stream_create(), l.dpgp_event_create(), l.dpgp_event_create())

    def __del__(self):
        try:
            if self.aux:
                l = _lib.lib()
                l.dpgp_stream_destroy(self.aux[0])
                l.dpgp_event_destroy(self.aux[1])
                l.dpgp_event_destroy(self.aux[2])
                self.aux = None
        except Exception:                                        # (interpreter shutdown)
            pass


def elbo_step(y, z, mu, s, gamma, alpha, beta, workspace, buffers, jitter=1e-8, model_tail=None, stage_b='mixed'):
    """One training step's worth of the fused reduction in mixed precision (dpgp_elbo_step): the f_hat terms of ``elbo_fhat``
    and the gradients of ``elbo_grad_chain`` + ``elbo_grad_psi`` from ONE call, the Psi2 exponentials evaluated twice instead of
    three times (dp_gp_lvm.py:108-145 and its tf.gradients, test/synthetic_data_hard_test.py:143-155).
    workspace: ElboWorkspace(..., 'mixed'); buffers: ElboStepBuffers.  All inputs fp64 device tensors (as ``elbo_fhat``).
    stage_b: 'mixed', or 'mixed_fast' (DPGP_PREC_MIXED_FAST, include/dpgp.h: 11-bit exponentials in the second products of stage B).
    Returns (terms, sums, info), (d_mu, d_s, d_z, d_gamma, d_alpha_beta, info_grad) — tensors of the two buffer objects."""
    import ctypes
    w, b = workspace, buffers
    d, n, m, q = w.shape
    assert b.shape == w.shape and w.prec == 'mixed', 'buffers were sized for another problem'
    assert y.is_cuda and y.dtype == torch.float64 and y.stride(1) == 1 and y.shape == (n, d)
    w.exec.ev_psi2_begin, w.exec.ev_psi2_end = None, None
    w.exec.model_scal, w.exec.model_pack, w.exec.model_out = (
        (None, None, None) if model_tail is None else tuple(None if t_ is None else t_.data_ptr() for t_ in model_tail))
    own = (w.exec.stream_aux, w.exec.ev_fork, w.exec.ev_join)
    if b.aux and not own[0]:
        w.exec.stream_aux, w.exec.ev_fork, w.exec.ev_join = b.aux
    try:
        _lib.check(_lib.lib().dpgp_elbo_step(
            d, n, m, q, y.data_ptr(), y.stride(0), z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(), alpha.data_ptr(),
            beta.data_ptr(), float(jitter), _lib.PREC[stage_b], w.terms.data_ptr(), w.sums.data_ptr(), w.info.data_ptr(), w.ws.data_ptr(),
            w.nbytes, b.gp.data_ptr(), b.wk.data_ptr(), b.gv.data_ptr(), b.dab.data_ptr(), b.info.data_ptr(), b.ws.data_ptr(), b.nbytes,
            b.dmu.data_ptr(), b.ds.data_ptr(), b.dz.data_ptr(), b.dg.data_ptr(), _stream(),
            ctypes.cast(ctypes.pointer(w.exec), ctypes.c_void_p)), 'dpgp_elbo_step')
    finally:
        w.exec.stream_aux, w.exec.ev_fork, w.exec.ev_join = own
    return (w.terms, w.sums, w.info), (b.dmu, b.ds, b.dz, b.dg, b.dab, b.info)


def elbo_fhat_step(y, z, mu, s, gamma, alpha, beta, workspace, buffers, jitter=1e-8, model_tail=None):
    """The forward half of ``elbo_step`` as a call of its own (dpgp_elbo_fhat_step; any M): as ``elbo_fhat`` in mixed precision, Psi2
    out of the first pass of stage B, whose results stay in ``buffers.ws`` for ``elbo_grad_psi_step``.  The forward workspace then
    holds ONE Psi2 slab (``elbo_grad_chain(..., psi2_slabs=1)``)."""
    import ctypes
    w, b = workspace, buffers
    d, n, m, q = w.shape
    assert b.shape == w.shape and w.prec == 'mixed'
    assert y.is_cuda and y.dtype == torch.float64 and y.stride(1) == 1 and y.shape == (n, d)
    w.exec.ev_psi2_begin, w.exec.ev_psi2_end = None, None
    w.exec.model_scal, w.exec.model_pack, w.exec.model_out = (
        (None, None, None) if model_tail is None else tuple(None if t_ is None else t_.data_ptr() for t_ in model_tail))
    _lib.check(_lib.lib().dpgp_elbo_fhat_step(
        d, n, m, q, y.data_ptr(), y.stride(0), z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(), alpha.data_ptr(),
        beta.data_ptr(), float(jitter), w.terms.data_ptr(), w.sums.data_ptr(), w.info.data_ptr(), w.ws.data_ptr(), w.nbytes,
        b.ws.data_ptr(), b.nbytes, _stream(), ctypes.cast(ctypes.pointer(w.exec), ctypes.c_void_p)), 'dpgp_elbo_fhat_step')
    return w.terms, w.sums, w.info


def elbo_grad_psi_step(y, z, mu, s, gamma, alpha, g_psi2, w_kuu, g_v, workspace, buffers, stage_b='mixed'):
    """The rest of stage B after ``elbo_fhat_step`` on the same workspace / buffers (dpgp_elbo_grad_psi_step)."""
    w, b = workspace, buffers
    d, n, m, q = w.shape
    _lib.check(_lib.lib().dpgp_elbo_grad_psi_step(
        d, n, m, q, y.data_ptr(), y.stride(0), z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(), alpha.data_ptr(),
        g_psi2.data_ptr(), w_kuu.data_ptr(), g_v.data_ptr(), _lib.PREC[stage_b], w.ws.data_ptr(), w.nbytes, b.ws.data_ptr(), b.nbytes,
        b.dmu.data_ptr(), b.ds.data_ptr(), b.dz.data_ptr(), b.dg.data_ptr(), _stream()), 'dpgp_elbo_grad_psi_step')
    return b.dmu, b.ds, b.dz, b.dg


def elbo_grad_chain(alpha, beta, workspace, jitter=1e-8, z=None, gamma=None, psi2_slabs=None):
    """Backward pass, stage A: adjoints of the per-output dense algebra from the workspace of a finished ``elbo_fhat`` call
    (dp_gp_lvm.py:108-145 differentiated; prec mixed / f64).  M <= 128: one HIP kernel per output dim with B in LDS
    (dpgp_elbo_grad_chain_ex).  M > 128 (needs z and gamma, mixed only downstream): composed here from the library's batched
    Cholesky / triangular solves and plain fp64 GEMMs (``_elbo_grad_chain_large``).
    psi2_slabs: the number of Psi2 partial slabs the forward evaluation left (1 after ``elbo_fhat_step``; default: the layout's).
    Returns (g_psi2 [D,Mp,Mp], w_kuu [D,Mp,Mp], g_v [D,Mp], d_alpha_beta [D,2], info [D]); see include/dpgp.h."""
    f64 = torch.float64
    d, n, m, q = workspace.shape
    alpha = _prep(alpha, f64, 'alpha').reshape(-1)
    beta = _prep(beta, f64, 'beta').reshape(-1)
    assert alpha.numel() == d and beta.numel() == d
    mp = 16 * ((m + 15) // 16)
    if mp > 128 and z is not None and gamma is not None:
        return _elbo_grad_chain_large(alpha, beta, workspace, jitter, z, gamma, psi2_slabs)
    dev = workspace.ws.device
    gp = torch.empty((d, mp, mp), dtype=f64, device=dev)
    wk = torch.empty((d, mp, mp), dtype=f64, device=dev)
    gv = torch.empty((d, mp), dtype=f64, device=dev)
    dab = torch.empty((d, 2), dtype=f64, device=dev)
    info = torch.empty(d, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().dpgp_elbo_grad_chain_ex(d, n, m, q, alpha.data_ptr(), beta.data_ptr(), float(jitter),
                                                  _lib.PREC[workspace.prec], workspace.ws.data_ptr(), workspace.nbytes,
                                                  0 if psi2_slabs is None else int(psi2_slabs), gp.data_ptr(), wk.data_ptr(),
                                                  gv.data_ptr(), dab.data_ptr(), info.data_ptr(), _stream()), 'dpgp_elbo_grad_chain_ex')
    return gp, wk, gv, dab, info


def _elbo_grad_chain_large(alpha, beta, workspace, jitter, z, gamma, psi2_slabs=None):
    """Stage A for M > 128.  M a multiple of 128: ONE library call, dpgp_elbo_grad_chain_big (csrc/chain_grad_big.hip: persistent Cholesky
    and solve, five strided MFMA products, three streaming kernels); other M (or DPGP_STAGE_A_COMPOSED=1, the cross-check): composed here
    from the batched operators (``_elbo_grad_chain_large_composed``)."""
    import os
    d, n, m, q = workspace.shape
    if m % 128 != 0 or workspace.prec not in ('mixed', 'f64') or os.environ.get('DPGP_STAGE_A_COMPOSED', '0') == '1':
        return _elbo_grad_chain_large_composed(alpha, beta, workspace, jitter, z, gamma, psi2_slabs)
    f64 = torch.float64
    dev = workspace.ws.device
    l = _lib.lib()
    z, gamma = _prep(z, f64, 'z'), _prep(gamma, f64, 'gamma')
    wsb = int(l.dpgp_elbo_grad_chain_big_workspace_bytes(d, m))
    ws = _ws(wsb, dev)
    gp, wk = torch.empty((d, m, m), dtype=f64, device=dev), torch.empty((d, m, m), dtype=f64, device=dev)
    gv, dab = torch.empty((d, m), dtype=f64, device=dev), torch.empty((d, 2), dtype=f64, device=dev)
    info = torch.empty(d, dtype=torch.int32, device=dev)
    _lib.check(l.dpgp_elbo_grad_chain_big(d, n, m, q, z.data_ptr(), gamma.data_ptr(), alpha.data_ptr(), beta.data_ptr(), float(jitter),
                                          _lib.PREC[workspace.prec], workspace.ws.data_ptr(), workspace.nbytes,
                                          0 if psi2_slabs is None else int(psi2_slabs), ws.data_ptr(), wsb, gp.data_ptr(), wk.data_ptr(),
                                          gv.data_ptr(), dab.data_ptr(), info.data_ptr(), _stream()), 'dpgp_elbo_grad_chain_big')
    return gp, wk, gv, dab, info


def _elbo_grad_chain_large_composed(alpha, beta, workspace, jitter, z, gamma, psi2_slabs=None):
    """Stage A for M > 128 (first version): the same adjoints as chain_grad_kernel (grad.hip), with B^-1 and K^-1 formed
    explicitly from the library's Cholesky factors — L^-1 by dpgp_trsm_batched on the identity, the M x M products as plain
    fp64 GEMMs (the library's strided MFMA kernel, ``matmul`` above), element-wise work in torch.  Reads Psi2, Psi1^T y and y^T y from the
    workspace of the forward evaluation (dpgp_elbo_workspace_layout); K_uu is rebuilt (one gram launch).
        G_B = -1/2 B^-1 - 1/2 beta^2 w w^T,  w = B^-1 v;   G_K = 1/2 K^-1 - 1/2 beta K^-1 P K^-1 + G_B;
        G_P = 1/2 beta K^-1 + beta G_B;   G_v = beta^2 w;   d/dalpha, d/dbeta complete (see chain_grad_kernel)."""
    import ctypes
    f64 = torch.float64
    d, n, m, q = workspace.shape
    dev = workspace.ws.device
    off_p2, ns2, esz, mp, off_v, ns1, off_yy, nyy = workspace.layout[:8]
    ns2 = ns2 if psi2_slabs is None else int(psi2_slabs)        # (after elbo_fhat_step: one slab)
    raw = workspace.ws
    pdt = torch.float32 if esz == 4 else f64
    p2 = raw[off_p2:off_p2 + esz * ns2 * d * mp * mp].view(pdt).view(ns2, d, mp, mp).sum(dim=0, dtype=f64)[:, :m, :m]
    p2 = torch.tril(p2) + torch.tril(p2, -1).transpose(1, 2)                    # (lower patches are what the kernel writes)
    v = raw[off_v:off_v + 8 * ns1 * d * m].view(f64).view(ns1, d, m).sum(dim=0)
    yy = raw[off_yy:off_yy + 8 * nyy * d].view(f64).view(nyy, d).sum(dim=0)
    k_uu = ard_rbf_gram(_prep(z, f64, 'z'), None, gamma, alpha, beta, include_noise=False, include_jitter=True, jitter=jitter)
    l_k, info_k = potrf_batched(k_uu)
    l_b, info_b = potrf_batched(k_uu + beta[:, None, None] * p2)
    li = tril_inverse_batched(l_k)
    k_inv = matmul(li.transpose(1, 2), li)
    li = tril_inverse_batched(l_b)
    b_inv = matmul(li.transpose(1, 2), li)
    del li
    w = matmul(b_inv, v[:, :, None])[:, :, 0]
    vw = torch.sum(v * w, dim=1)
    x = matmul(matmul(k_inv, p2), k_inv)
    be = beta[:, None, None]
    gb = -0.5 * b_inv - 0.5 * be * be * w[:, :, None] * w[:, None, :]
    gk = 0.5 * k_inv - 0.5 * be * x + gb
    gp_ = 0.5 * be * k_inv + be * gb
    wk_ = gk * (k_uu - float(jitter) * torch.eye(m, dtype=f64, device=dev))
    s_k, s_p = wk_.sum(dim=(1, 2)), (gp_ * p2).sum(dim=(1, 2))
    s_gbp, tr = (gb * p2).sum(dim=(1, 2)), (k_inv * p2).sum(dim=(1, 2))
    dab = torch.stack([-0.5 * beta * n + (s_k + 2.0 * s_p + beta * beta * vw) / alpha,
                       0.5 * n / beta + 0.5 * (tr - alpha * n) - 0.5 * yy + beta * vw + s_gbp], dim=1).contiguous()
    pad = (0, mp - m, 0, mp - m)
    gp = torch.nn.functional.pad(gp_, pad).contiguous()
    wk = torch.nn.functional.pad(wk_, pad).contiguous()
    gv = torch.nn.functional.pad(beta[:, None] ** 2 * w, (0, mp - m)).contiguous()
    return gp, wk, gv, dab, torch.maximum(info_k, info_b)


def elbo_grad_psi(y, z, mu, s, gamma, alpha, g_psi2, w_kuu, g_v, prec='mixed', g_psi1=None, weights=None):
    """Backward pass, stage B: d f_hat / d (mu [N,Q], s [N,Q], z [M,Q], gamma [D,Q]) from the stage-A adjoints
    (rbf_kernel.py:58-199 differentiated).  g_psi1 [D,N,Mp] (mixed precision only): a full adjoint of Psi1 in place of the
    rank-1 form g_v[d,a] y[n,d] — then y and g_v may be None.
    weights [D,N] (prec='f64' only, AssertionError otherwise): the Psi2 term becomes <g_psi2_d, sum_n weights[d,n] psi2_dn>
    (dpgp_elbo_grad_psi_weighted_f64); the Psi1 term is governed by y alone (zero-fill it), the K_uu term is unweighted.  The
    weights must be >= 0 and finite — behaviour for negative weights is unspecified; a weight of 0 contributes exactly 0.0."""
    assert weights is None or (prec == 'f64' and g_psi1 is None), 'weights are taken by the fp64 stage B only'
    f64 = torch.float64
    z, mu, s = _prep(z, f64, 'z'), _prep(mu, f64, 'mu'), _prep(s, f64, 's')
    gamma, alpha, _, d = _hyp(gamma, alpha, None, f64)
    n, m, q = mu.shape[0], z.shape[0], z.shape[1]
    if y is not None and (y.dtype != f64 or y.stride(1) != 1):
        y = y.to(f64).contiguous()
    if g_psi1 is not None:
        g_psi1 = _prep(g_psi1, f64, 'g_psi1')
        assert g_psi1.shape == (d, n, g_psi2.shape[1])
    dev = mu.device
    if prec == 'f64' and m > 128:
        if g_psi1 is not None:
            raise ValueError('a full Psi1 adjoint is taken in mixed precision only')
        return _elbo_grad_psi_f64_blocks(y, z, mu, s, gamma, alpha, g_psi2, w_kuu, g_v, weights)
    l = _lib.lib()
    wsb = l.dpgp_elbo_grad_psi_workspace_bytes_ex(d, n, m, q, _lib.PREC[prec])
    ws = _ws(wsb, dev)
    dmu, ds = torch.empty((n, q), dtype=f64, device=dev), torch.empty((n, q), dtype=f64, device=dev)
    dz, dg = torch.empty((m, q), dtype=f64, device=dev), torch.empty((d, q), dtype=f64, device=dev)
    if weights is not None:
        weights = _qx_weights(weights, d, n, mu)
        _lib.check(l.dpgp_elbo_grad_psi_weighted_f64(d, n, m, q, y.data_ptr(), y.stride(0), z.data_ptr(), mu.data_ptr(),
                                                     s.data_ptr(), gamma.data_ptr(), alpha.data_ptr(), weights.data_ptr(),
                                                     g_psi2.data_ptr(), w_kuu.data_ptr(), g_v.data_ptr(), ws.data_ptr(), wsb,
                                                     dmu.data_ptr(), ds.data_ptr(), dz.data_ptr(), dg.data_ptr(), _stream()),
                   'dpgp_elbo_grad_psi_weighted_f64')
        return dmu, ds, dz, dg
    _lib.check(l.dpgp_elbo_grad_psi_ex(d, n, m, q, y.data_ptr() if y is not None else None, y.stride(0) if y is not None else 0,
                                       z.data_ptr(), mu.data_ptr(), s.data_ptr(), gamma.data_ptr(), alpha.data_ptr(),
                                       g_psi2.data_ptr(), w_kuu.data_ptr(), g_v.data_ptr() if g_v is not None else None,
                                       g_psi1.data_ptr() if g_psi1 is not None else None, _lib.PREC[prec], ws.data_ptr(), wsb,
                                       dmu.data_ptr(), ds.data_ptr(), dz.data_ptr(), dg.data_ptr(), _stream()),
               'dpgp_elbo_grad_psi_ex')
    return dmu, ds, dz, dg


def _elbo_grad_psi_f64_blocks(y, z, mu, s, gamma, alpha, g_psi2, w_kuu, g_v, weights=None):
    """Stage B in fp64 for M > 128.  The fp64 kernel keeps the M x M adjoint of one output dim in LDS (M <= 128); every term
    of stage B is a sum over PAIRS of inducing points (Psi2 and K_uu terms) or over single ones (Psi1 term), so the sum is
    split over the nb (nb - 1) / 2 unordered pairs {I, J} of blocks of <= 64 inducing points: pair {I, J} runs the same
    kernel on the 128 points z_I, z_J with the adjoint blocks [[G_II / (nb - 1), G_IJ], [G_JI, G_JJ / (nb - 1)]] (a diagonal
    block and a single point belong to nb - 1 pairs).  Exact in exact arithmetic, fp64 throughout, the same work as one
    pass over the M x M square; the training configuration (precision='f64', backward_precision='mixed') does not come
    here — this is the reference-precision check of it."""
    f64 = torch.float64
    dev = mu.device
    d, (n, q), m = gamma.shape[0], mu.shape, z.shape[0]
    nb = -(-m // 64)
    blocks = [b.to(dev) for b in torch.tensor_split(torch.arange(m), nb)]
    wd = 1.0 / (nb - 1)
    dmu, ds = torch.zeros((n, q), dtype=f64, device=dev), torch.zeros((n, q), dtype=f64, device=dev)
    dz, dg = torch.zeros((m, q), dtype=f64, device=dev), torch.zeros((d, q), dtype=f64, device=dev)
    for i in range(nb):
        for j in range(i + 1, nb):
            idx = torch.cat([blocks[i], blocks[j]])
            ni, ms = blocks[i].numel(), idx.numel()
            mps = 16 * ((ms + 15) // 16)
            scale = torch.ones((ms, ms), dtype=f64, device=dev)
            scale[:ni, :ni] = wd
            scale[ni:, ni:] = wd
            pad2 = (0, mps - ms, 0, mps - ms)
            gs = torch.nn.functional.pad(g_psi2[:, idx][:, :, idx] * scale, pad2).contiguous()
            ws_ = torch.nn.functional.pad(w_kuu[:, idx][:, :, idx] * scale, pad2).contiguous()
            gvs = torch.nn.functional.pad(g_v[:, idx] * wd, (0, mps - ms)).contiguous() if g_v is not None else None
            a, b, c, e = elbo_grad_psi(y, z[idx].contiguous(), mu, s, gamma, alpha, gs, ws_, gvs, prec='f64', weights=weights)
            dmu += a
            ds += b
            dz.index_add_(0, idx, c)
            dg += e
    return dmu, ds, dz, dg
