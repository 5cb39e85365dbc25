"""
The collapsed sparse-GP bound of one batch slot, its backward pass and its posterior, in fp64 on the device: the algebra shared
by the masked training bounds (masked_bound*.py), the frozen test bounds (frozen_bound*.py) and the predictive moments
(marginals.py, frozen_bound_t._MomentsT).  This is the only module under models/ that factorises A; the callers choose the batch
layout, the Psi operators, the reductions over slots and the parameter adjoints.

Per slot b, with K = K_uu + jitter I = L L^T, the (weighted) statistic Psi2, the noise precision beta, v = Psi1^T Y [M, J] (Y zero
where unobserved), N_w observed rows, a multiplier D (the number of columns that share the slot; sum_j phi_j over-T; 1 over-D)
and optional column weights phi [J] (over-T; 1 otherwise):

    T = L^-1 Psi2 L^-T,   A = beta T + I = L_A L_A^T,   R0 = L_A^-1 L^-1,   u = R0 v,   P = R0^T R0 = (K + beta Psi2)^-1
    f = 1/2 N_w D (log beta - log 2 pi) - D log|L_A| + 1/2 D beta (tr T - alpha N_w) + 1/2 beta^2 sum_j phi_j |u_j|^2
        - 1/2 beta sum_j phi_j |y_j|^2

(log|L_A| = 1/2 log|A| = 1/2 log|K + beta Psi2| - 1/2 log|K|, |u_j|^2 = v_j^T P v_j).  Backward pass, with r = R0^T u = P v,
RR = (r phi) r^T and KP = K^-1 Psi2:

    df/dv    = beta^2 r phi
    df/dPsi2 = G2 = 1/2 D beta (K^-1 - P) - 1/2 beta^3 RR                               the difference form
                  = 1/2 D beta^2 sym(KP P) - 1/2 beta^3 RR                              the product form
    df/dK    = GK = -1/2 D beta^2 sym(KP P KP^T) - 1/2 beta^2 RR
    df/dbeta      = 1/2 N_w D / beta - 1/2 D <P, Psi2> + 1/2 D (tr T - alpha N_w) + beta sum_j phi_j |u_j|^2
                    - 1/2 beta^2 <RR, Psi2> - 1/2 sum_j phi_j |y_j|^2

The two forms of G2 are one matrix, K^-1 - P = beta K^-1 Psi2 P.  The difference cancels when beta |Psi2| is small against |K|
(a slot with few observed rows), so the training bounds, whose G2 also drives (Z, gamma, alpha), use the product; the frozen
test bounds of bayesian_gp_lvm, MRD and dp_gp_lvm keep the difference, which needs no further product.  GK is the explicit
K-derivative 1/2 D (K^-1 - P) - 1/2 D beta K^-1 Psi2 K^-1 - 1/2 beta^2 RR in its product form.  Posterior: the weights
rhs = beta P v of the predictive mean and C = K^-1 - P of the predictive variance.

No host synchronisation anywhere: every function is safe under graph capture.
"""
import torch

from .. import ops
from ..utils.constants import GP_DEFAULT_JITTER
from ..utils.types import TORCH_DTYPE


def factors(k_uu):
    """K_uu [K,M,M] -> (L^-1 [K,M,M], the potrf info [K])."""
    l_uu, info = ops.potrf_batched(k_uu)
    return ops.tril_inverse_batched(l_uu), info


def k_inverse(li):
    """K_uu^-1 = L^-T L^-1."""
    return ops.matmul(li.transpose(1, 2), li)


def shared_z_kernels(z, gamma, alpha):
    """K kernels (gamma [K,Q], alpha [K]) on ONE set of inducing inputs z [M,Q]: (L^-1, K_uu^-1, info, pair factor of Psi2), one
    gram call each for K_uu and the pair factor."""
    ones = torch.ones_like(alpha)                                   # the noise precision: not read without include_noise
    li, info = factors(ops.ard_rbf_gram(z, None, gamma, alpha, ones, include_noise=False, include_jitter=True,
                                        jitter=GP_DEFAULT_JITTER))
    return li, k_inverse(li), info, ops.ard_rbf_gram(z, None, 0.5 * gamma, alpha * alpha, ones)


def own_z_kernels(z, gamma, alpha):
    """K kernels with their own inducing inputs z [K,M,Q] (gamma [K,Q], alpha [K]): as shared_z_kernels, one gram call per
    kernel and ops.qx_pair_factor."""
    one = torch.ones_like(alpha[:1])
    li, info = factors(torch.cat([ops.ard_rbf_gram(z[k], None, gamma[k:k + 1], alpha[k:k + 1], one, include_noise=False,
                                                   include_jitter=True, jitter=GP_DEFAULT_JITTER) for k in range(z.shape[0])]))
    return li, k_inverse(li), info, ops.qx_pair_factor(z, gamma, alpha)


def precision(r0):
    """P = R0^T R0 = (K_uu + beta Psi2)^-1."""
    return ops.matmul(r0.transpose(1, 2), r0)


def posterior(r0, kinv, beta, v):
    """(rhs = beta P v [B,M,J], C = K_uu^-1 - P): the predictive mean's weights and the predictive variance's matrix; beta [B] or
    one element."""
    p = precision(r0)
    return beta.reshape(-1)[:, None, None] * ops.matmul(p, v), kinv - p


class Chain:
    """The forward pass of B slots from li = L^-1 [B,M,M], psi_2 [B,M,M] and beta ([B], or one element for all slots): tm = T,
    l_a = L_A, info (potrf's, [B]) and r0; project(v) adds u, logdet = log|L_A| and tr = tr T."""

    def __init__(self, li, psi_2, beta, eye=None):
        if eye is None:
            eye = torch.eye(li.shape[1], dtype=TORCH_DTYPE, device=li.device)
        self.li, self.psi_2, self.beta = li, psi_2, beta.reshape(-1)
        self.tm = ops.matmul(ops.matmul(li, psi_2), li.transpose(1, 2))
        self.l_a, self.info = ops.potrf_batched(self.beta[:, None, None] * self.tm + eye)
        self.r0 = ops.matmul(ops.tril_inverse_batched(self.l_a), li)

    def project(self, v):
        """v [B,M,J]; returns self."""
        self.u = ops.matmul(self.r0, v)
        self.logdet = torch.sum(torch.log(torch.diagonal(self.l_a, dim1=-2, dim2=-1)), dim=-1)
        self.tr = torch.diagonal(self.tm, dim1=-2, dim2=-1).sum(-1)
        return self


def _sym(a):
    return 0.5 * (a + a.transpose(1, 2))


def _times(a, d):
    """a D; D = None stands for 1 and costs no launch."""
    return a if d is None else a * d


class Adjoint:
    """The backward pieces of a projected Chain: r [B,M,J], rphi = r phi, p = P, rr = RR, then G2, GK and the beta summand on
    request.  dd [B]: the multiplier D (None: 1); phi [B,J] or None; outer: the product forming RR from (rphi, r^T), ops.matmul,
    or torch.mul for J = 1 (the broadcast product is that outer product without a gemm launch)."""

    def __init__(self, chain, dd=None, phi=None, outer=ops.matmul):
        self.chain, self.dd = chain, dd
        self.d3 = None if dd is None else dd[:, None, None]
        self.b3 = chain.beta[:, None, None]
        self.r = ops.matmul(chain.r0.transpose(1, 2), chain.u)
        self.rphi = self.r if phi is None else self.r * phi[:, None, :]
        self.p = precision(chain.r0)
        self.rr = outer(self.rphi, self.r.transpose(1, 2))

    def g2_difference(self, kinv):
        return (_times(0.5, self.dd) * self.chain.beta)[:, None, None] * (kinv - self.p) - (0.5 * self.b3 ** 3) * self.rr

    def g2_product(self, kinv):
        """Also keeps kp = KP and kpp = KP P for gk()."""
        b3 = self.b3
        self.kp = ops.matmul(kinv, self.chain.psi_2)
        self.kpp = ops.matmul(self.kp, self.p)
        return _times(0.5 * b3 * b3, self.d3) * _sym(self.kpp) - (0.5 * b3 ** 3) * self.rr

    def gk(self):
        """GK per slot [B,M,M] (after g2_product)."""
        b3 = self.b3
        return _times(-0.5 * b3 * b3, self.d3) * _sym(ops.matmul(self.kpp, self.kp.transpose(1, 2))) - (0.5 * b3 * b3) * self.rr

    def d_beta(self, n_w, alpha, uu, yy):
        """The beta summand per slot [B]: n_w [B], alpha ([B] or one element), uu = sum_j phi_j |u_j|^2, yy = sum_j phi_j |y_j|^2."""
        c, be, dd = self.chain, self.chain.beta, self.dd
        return _times(0.5 * n_w, dd) / be - _times(0.5, dd) * torch.sum(self.p * c.psi_2, dim=(1, 2)) \
            + _times(0.5, dd) * (c.tr - alpha * n_w) + be * uu - (0.5 * be * be) * torch.sum(self.rr * c.psi_2, dim=(1, 2)) - 0.5 * yy
