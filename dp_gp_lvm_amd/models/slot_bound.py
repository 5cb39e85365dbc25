"""
Test-point slots over K frozen kernels that each have their own inducing inputs (the per-entry masks of
manifold_relevance_determination at test time): a _TestBound whose slot b uses kernel kern[b].
"""
import numpy as np
import torch

from ..utils.types import TORCH_DTYPE
from .test_bound import _TestBound


def kernel_slots(z, gamma, alpha, beta, kern, y, dims, weights, device):
    """B slots over K kernels (lists of K: z [M,Q], gamma, alpha, beta, as _TestBound takes them); kern [B]: slot b's kernel.
    y [B,N*,Dmax] (zero where unobserved and in the padding columns), dims [B], weights [B,N*] as _TestBound.slots.  K_uu, L,
    L^-1, K_uu^-1 and the pair factor are formed once per kernel (as _TestBound.__init__ forms them) and gathered to the
    slots; the returned object evaluates as any _TestBound with weights."""
    f64 = TORCH_DTYPE
    per = _TestBound(z, gamma, alpha, beta, [torch.zeros((1, 1), dtype=f64, device=device)] * len(z), device)
    self = _TestBound.__new__(_TestBound)
    idx = torch.as_tensor(np.asarray(kern, dtype=np.int64), device=device)
    take = lambda t: t.index_select(0, idx).contiguous()
    self.z, self.gamma, self.alpha, self.beta = take(per.z), take(per.gamma), take(per.alpha), take(per.beta)
    self.l_uu, self.info_uu, self.li, self.kinv, self.zfac = (take(t) for t in (per.l_uu, per.info_uu, per.li, per.kinv, per.zfac))
    self.m, self.device, self.n_t, self.eye = per.m, device, y.shape[1], per.eye
    self.dims = torch.as_tensor(np.asarray(dims, dtype=np.float64), dtype=f64, device=device)
    self.y = y.detach().to(device=device, dtype=f64).contiguous()
    self.yy = torch.sum(self.y * self.y, dim=(1, 2))
    self.terms = None
    self.weights = weights.detach().to(device=device, dtype=f64).contiguous()
    self.n_w = torch.sum(self.weights, dim=1)
    return self
