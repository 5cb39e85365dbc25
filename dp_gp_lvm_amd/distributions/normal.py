"""Multivariate normal scoring of predictions (reference: src/distributions/normal.py:14-36), on the library's batched
Cholesky / triangular-solve operators (dpgp_potrf_batched, dpgp_trsm_batched) instead of tf.cholesky /
tf.matrix_triangular_solve.  Used as in test/frey_faces_prediction.py:232-238: log-likelihood of the held-out ground truth
under the predictive mean / covariance that predict_missing_data returns."""
import math

import torch

from .. import ops
from ..utils.types import TORCH_DTYPE


def _chol(covariance):
    c = torch.as_tensor(covariance, dtype=TORCH_DTYPE)
    while c.dim() > 2 and c.shape[0] == 1:
        c = c[0]                                                  # tf.squeeze
    assert c.dim() == 2 and c.shape[0] == c.shape[1], 'covariance must be [D x D]'
    l_, info = ops.potrf_batched(c[None].contiguous())
    return l_, info


def mvn_log_pdf(x, mean, covariance):
    """Log-likelihood of the rows of x [B x D] under N(mean [1 x D], covariance [D x D]); returns a B-vector.
    A covariance that is not positive definite gives NaN (tf.cholesky raises there)."""
    x = torch.as_tensor(x, dtype=TORCH_DTYPE, device=covariance.device if torch.is_tensor(covariance) else None)
    mean = torch.as_tensor(mean, dtype=TORCH_DTYPE, device=x.device)
    l_, info = _chol(covariance)
    num_dims = l_.shape[-1]
    diff = (x - mean).transpose(0, 1).contiguous()                # [D x B]
    alpha = ops.trsm_batched(l_, diff[None].contiguous())[0].transpose(0, 1)          # [B x D]
    beta = torch.sum(torch.log(torch.diagonal(l_[0])))
    out = -0.5 * (torch.sum(alpha * alpha, dim=-1) + num_dims * math.log(2.0 * math.pi)) - beta
    return torch.where(info[0] == 0, out, torch.full_like(out, float('nan')))


def _mat(t, device, name):
    t = torch.as_tensor(t, dtype=TORCH_DTYPE, device=device)
    while t.dim() > 2 and t.shape[0] == 1:
        t = t[0]                                                  # (leading batch of one, as tf.squeeze would drop it)
    assert t.dim() == 2, '%s must be a matrix' % name
    return t


def mvn_conditional_mean_covar(b, mean_a, mean_b, covar_aa, covar_bb, covar_ab, reference_compat=True):
    """Conditional mean [N x D_a] and covariance [D_a x D_a] of 'a' given the samples b [N x D_b] (reference:
    src/distributions/normal.py:39-70), on dpgp_potrf_batched, dpgp_trsm_batched and the fp64 MFMA product:
        mean  = mean_a + covar_ab^T alpha,   covar = covar_aa - v^T v,   v = L^-1 covar_ab,   L = chol(covar_bb)
    with covar_ab given as [D_b x D_a] (the orientation the reference's solve uses).  Its matrices keep two dimensions
    throughout, so D_a = 1 works (the reference squeezes covar_ab to a vector there and fails).
    reference_compat=True (default) reproduces the reference's alpha = diag(L)^-1 L^-1 (b - mean_b): its second solve is
    tf.matrix_triangular_solve(L^T, ., lower=True), which reads only the lower triangle of L^T, i.e. its diagonal.
    reference_compat=False gives the textbook alpha = covar_bb^-1 (b - mean_b) = L^-T L^-1 (b - mean_b).
    A covar_bb that is not positive definite gives NaN (tf.cholesky raises there)."""
    device = covar_bb.device if torch.is_tensor(covar_bb) else None
    kbb = _mat(covar_bb, device, 'covar_bb')
    device = kbb.device
    kab = _mat(covar_ab, device, 'covar_ab')
    kaa = _mat(covar_aa, device, 'covar_aa')
    diff = _mat(b, device, 'b') - _mat(mean_b, device, 'mean_b')
    l_, info = ops.potrf_batched(kbb[None].contiguous())
    t = ops.trsm_batched(l_, diff[None].contiguous())[0]
    if reference_compat:
        alpha = t / torch.diagonal(l_[0])[:, None]
    else:
        alpha = ops.matmul(ops.tril_inverse_batched(l_)[0].transpose(0, 1), t)
    v = ops.trsm_batched(l_, kab[None].contiguous())[0]
    mean = _mat(mean_a, device, 'mean_a') + ops.matmul(kab.transpose(0, 1), alpha)
    covar = ops.matmul(v.transpose(0, 1), v, out=kaa.clone(), alpha=-1.0, beta=1.0)
    ok = info[0] == 0
    nan = torch.full((), float('nan'), dtype=TORCH_DTYPE, device=device)
    return torch.where(ok, mean, nan), torch.where(ok, covar, nan)
