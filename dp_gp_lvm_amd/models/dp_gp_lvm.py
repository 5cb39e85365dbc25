"""
DP-GP-LVM — mirror of the reference's ``dp_gp_lvm`` factory (src/models/dp_gp_lvm.py:22-510) with the same signature,
assertions and accessors; ``.objective`` is evaluated by the HIP library (libdpgp_hip.so):

    dpgp_model_prepare  ->  dpgp_elbo_fhat  ->  [one packed all-reduce when D is sharded]  ->  dpgp_model_finalize

i.e. five kernel launches and at most one collective per evaluation, with no host arithmetic in between.
Where the reference returns lazy TensorFlow nodes, accessors here return torch tensors computed from the current
parameter values, and ``objective`` re-evaluates on every access.

Multi-GPU: the per-output-dimension terms are independent given (q(X), Z, atoms), so the D outputs are sharded over the
ranks of ``process_group`` (rank r keeps columns r*D/W .. (r+1)*D/W of Y and the matching rows of phi); q(X), Z and the
atoms are replicated.  The only exchange per evaluation is a sum all-reduce of the two scalars (f_hat, DP objective).
The same holds for a model trained with observed= (its bound runs on the local columns observed somewhere, possibly none), for the
per-entry moments and for the shared-inducing test bound, whose sums over columns are completed by one all-reduce each
(DESIGN.md section 7.15).
"""
import contextlib
import functools
import gc
import os
import numpy as np
import torch
import torch.nn.functional as F

from .. import _lib, ops
from ..kernels.interfaces.kernel import KernelHyperparameters
from ..kernels.rbf_kernel import k_ard_rbf
from ..utils.constants import GP_LVM_DEFAULT_LATENT_DIMENSIONS, GP_LVM_DEFAULT_NUM_INDUCING_POINTS, \
    DP_DEFAULT_TRUNCATION_LEVEL, DP_DEFAULT_ALPHA_PRIOR_PARAMS, GP_INIT_GAMMA, GP_INIT_ALPHA, GP_INIT_BETA, \
    GP_DEFAULT_JITTER
from ..utils.expressions import principal_component_analysis as pca
from ..utils import missing as _missing
from ..utils.types import TORCH_DTYPE, create_positive_variable, default_device, register_variable
from .dirichlet_process import dirichlet_process
from .interfaces.trainable import Trainable
from . import collapsed, marginals as _marginals, predictor as _predictor, test_latents as _latents
from .latent_geometry import LatentGeometry
from .masked_bound_d import _MaskedBoundD
from .masked_bound_t import _MaskedBoundT
from .frozen_bound import _TestBound
from .frozen_bound_d import _ShardedTestBoundD, _TestBoundD
from .frozen_bound_t import _MomentsT, _TestBoundT


def shard_bounds(num_dimensions, rank, world_size):
    """Contiguous, balanced split of the D output dims: rank r owns [lo, hi)."""
    base, rem = divmod(num_dimensions, world_size)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def weighted_shard_bounds(costs, rank, world_size, align=1):
    """Contiguous split of the D = len(costs) output dims by cost: rank r owns [lo, hi), every bound a multiple of `align` (or D),
    and the largest share's cost is the smallest any contiguous aligned split into world_size shares can have.  Exact dynamic
    programme over the D / align units (prefix sums; O(world_size units^2), host only, deterministic: every rank computes the same
    bounds).  Among the splits with that largest share it prefers a small sum of squared shares, then late cuts, which for equal
    costs is shard_bounds.  No share is empty while world_size <= ceil(D / align); beyond that the first units get a rank each."""
    costs = np.asarray(costs, dtype=np.float64).reshape(-1)
    d, align = costs.size, int(align)
    assert align >= 1 and world_size >= 1 and 0 <= rank < world_size and d >= 1 and (costs >= 0).all(), \
        'weighted_shard_bounds: costs must be non-negative, 0 <= rank < world_size, align >= 1'
    units = -(-d // align)
    if world_size >= units:
        cuts = [min(k, units) for k in range(world_size + 1)]
    else:
        prefix = np.concatenate([[0.0], np.cumsum(np.add.reduceat(costs, np.arange(0, d, align)))])
        # best[k][i]: (largest share, sum of squares, first cut) of the units i.. split into k non-empty shares
        best = [[None] * (units + 1) for _ in range(world_size + 1)]
        for i in range(units):
            c = prefix[units] - prefix[i]
            best[1][i] = (c, c * c, units)
        for k in range(2, world_size + 1):
            for i in range(units - k + 1):
                pick = None
                for c in range(i + 1, units - k + 2):
                    head, rest = prefix[c] - prefix[i], best[k - 1][c]
                    cand = (max(head, rest[0]), head * head + rest[1], c)
                    if pick is None or cand[:2] <= pick[:2]:
                        pick = cand                      # (ties: the later cut)
                best[k][i] = pick
        cuts = [0]
        for k in range(world_size, 0, -1):
            cuts.append(best[k][cuts[-1]][2])
    return min(cuts[rank] * align, d), min(cuts[rank + 1] * align, d)


@contextlib.contextmanager
def _graph_capture(graph):
    """torch.cuda.graph(graph) with Python's cyclic garbage collector held off for the length of the capture.  A model that went out of
    use inside a reference cycle keeps its torch.cuda.CUDAGraph until a collection, torch no longer collects on entry, and a collection
    that falls inside a capture destroys that graph there: destroying a graph is not permitted while a stream is capturing, the
    destructor throws and the process aborts.  So: collect first, then capture with the collector disabled."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            yield
    finally:
        if was_enabled:
            gc.enable()


def _adam(params, learning_rate):
    """torch.optim.Adam on the raw variables (plumbing: it only applies the update).  The fused implementation where this build of
    torch has it for fp64 device tensors — one launch instead of a dozen element-wise ones per iteration (DPGP_FUSED_ADAM=0: the default
    one)."""
    if os.environ.get('DPGP_FUSED_ADAM', '1') != '0':
        try:
            return torch.optim.Adam(params, lr=learning_rate, fused=True)
        except (RuntimeError, TypeError, ValueError):
            pass
    return torch.optim.Adam(params, lr=learning_rate)


def dp_gp_lvm(y_train,
              num_latent_dims=GP_LVM_DEFAULT_LATENT_DIMENSIONS,
              num_inducing_points=GP_LVM_DEFAULT_NUM_INDUCING_POINTS,
              truncation_level=DP_DEFAULT_TRUNCATION_LEVEL,
              alpha_prior_params=DP_DEFAULT_ALPHA_PRIOR_PARAMS,
              mask_size=1,
              device=None, precision=None, process_group=None, initial_values=None, backward_precision=None,
              psi_algo='auto', _shard_of=None, observed=None, shard_by='count'):
    """
    :param y_train: [N x D] numpy array, columns normalised to zero mean / unit variance (dp_gp_lvm.py:30-32).
    :param num_latent_dims: Q.  :param num_inducing_points: M.  :param truncation_level: T.
    :param alpha_prior_params: Gamma prior (s_1, s_2) on the DP concentration.  :param mask_size: see the reference.
    Extensions (keyword-only in spirit, all optional):
    :param device: torch device of the parameters (default: current GPU).
    :param precision: 'mixed' (psi-statistics fp32 on the matrix cores, Cholesky chain fp64), 'f64' or 'f32'.
    :param process_group: torch.distributed group over which the D output dims are sharded (None: single GPU).
    :param backward_precision: precision of the streaming stage (B) of the backward pass; default: `precision`.  'mixed' with
           precision='f64' = fp64 forward and dense adjoints (accurate B^-1, K^-1 however ill-conditioned K_uu is), the
           streaming stage on the matrix pipe (gradients to ~1e-4): the training configuration (see optimise()).
    :param psi_algo: 'auto' (fp32 psi-statistics on f16 hi/lo-split MFMA operands), 'mfma_f32' (exact fp32 products on
           v_mfma_f32_16x16x4_f32: no f16 range limit, slower) or 'plain' (VALU cross-check kernels); forward evaluation only.
    :param initial_values: dict of post-initialisation parameter VALUES (x_mean, x_var, x_u, phi_logits, gamma_atoms,
           alpha_atoms, beta_atoms, gamma_1, gamma_2, w_1, w_2) that replace the random/PCA initialisation — used by the
           parity tests and the benchmark, which must not depend on PCA sign conventions or NumPy's global RNG.
    :param observed: (extension) a boolean [N x D] mask of the entries of y_train that were measured, any pattern with at least one
           True (entries where it is False are ignored and may be NaN; utils.missing.observed_mask makes the mask of a NaN-filled
           array).  f_hat is then the sum over the columns d observed somewhere of the unmasked model's five terms on the rows R_d
           at which d was measured (N -> N_d, Psi2_d and y_d^T y_d over R_d, Psi1_d^T y_d on the zero-filled column): the fp64
           operators of the unmasked precision='f64' model with a 0 / 1 weight per (column, row) on the Psi2 sum and its adjoint
           (models/masked_bound_d.py), evaluated eagerly — precision and backward_precision None or 'f64'.
           KL(q(X)) runs over all N rows, the DP objective over all D columns, the hyper-prior over the T
           atoms; a column never observed contributes its DP terms only, a row never observed its KL only.  x_mean defaults to the
           PCA of the column-mean-filled data.  impute_training_data() fills the gaps with the posterior mean.
           With process_group every rank is given the full y_train and the full mask and keeps its columns of both; the bound runs
           on the local columns observed somewhere, which may be none (such a rank contributes f_hat = 0 and zero partial
           derivatives and still joins every collective); the exchanges are the unmasked model's.
    :param shard_by: how the D columns are split over the ranks: 'count' (shard_bounds: equal numbers of columns) or, with observed
           only, 'observed' (weighted_shard_bounds on a cost of 1 + the number of observed rows per column, aligned to mask_size).
    """
    num_samples, num_dimensions = np.shape(y_train)
    train_obs = None
    assert shard_by in ('count', 'observed'), "shard_by must be 'count' or 'observed'"
    assert shard_by == 'count' or observed is not None, "shard_by='observed' splits by the mask: it needs observed="
    if observed is not None:
        assert precision in (None, 'f64'), "with observed, precision must be None or 'f64' (the masked model is fp64)"
        assert backward_precision in (None, 'f64'), "with observed, backward_precision must be None or 'f64' (the masked model is fp64)"
        if process_group is not None:
            import torch.distributed as dist_
            assert isinstance(process_group, dist_.ProcessGroup), 'process_group must be a torch.distributed process group'
        train_obs = _missing.check_observed(observed, (num_samples, num_dimensions))
        assert train_obs.any(), 'observed must hold at least one True entry'
        y_train = _missing.zero_filled(y_train, train_obs)
        precision = backward_precision = 'f64'
    assert 0 < num_latent_dims <= num_dimensions, \
        'Number of latent dimensions must be postive and less than the dimensionality of the observed data.'
    assert 0 < num_inducing_points <= num_samples, \
        'Number of inducing points must be positive and less than the number of observations in the observed data.'
    assert 0 < truncation_level <= min(num_samples, num_dimensions), \
        'The truncation level must be positive and less than the dimensionality of the observed data and ' \
        'less than the number of observations.'
    if precision is None:
        # the default-constructed model is the one that trains like the reference (fp64 arithmetic, src/utils/types.py:13-14):
        # fp64 forward pass and dense adjoints, the streaming stage of the backward pass on the matrix pipe.
        # precision='mixed' (fp32 psi-statistics) is the fast scoring mode: its conditioning guard stops a long Adam run.
        precision, backward_precision = 'f64', (backward_precision or 'mixed')
    assert precision in ('f32', 'mixed', 'f64'), "precision must be one of 'f32', 'mixed', 'f64'"
    assert backward_precision in (None, 'mixed', 'f64', 'mixed_fast'), "backward_precision must be None, 'mixed', 'mixed_fast' or 'f64'"
    # stage B behind an fp64 forward pass (the training configuration): the patch form of the Psi2 term, which keeps its accuracy
    # where the adjoints cancel (include/dpgp.h, DPGP_PREC_MIXED_PATCH); behind a mixed forward pass the faster pair-tile form
    # precision='f32' (the psi-statistics as exact fp32 products, fp32 chain) is a scoring precision: its gradients are those of the
    # mixed evaluation — the same function to the mixed tolerance, fp64 dense adjoints — on a second, lazily built workspace
    grad_precision = 'mixed' if precision == 'f32' else precision
    stage_b_precision = backward_precision or grad_precision
    if precision == 'f64' and backward_precision == 'mixed':
        stage_b_precision = 'mixed_patch'
    assert psi_algo in _lib.ALGO, 'psi_algo must be one of %s' % sorted(_lib.ALGO)
    assert truncation_level <= 64, 'truncation levels above 64 are not supported by the HIP model kernels (PREP_MAX_T)'
    device = default_device() if device is None else torch.device(device)
    iv = dict(initial_values or {})

    def _t(a):
        return torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=TORCH_DTYPE, device=device).contiguous()

    def _raw_pos(name, init, shape):
        if name in iv:
            v = np.asarray(iv[name], dtype=np.float64).reshape(shape)
            return _t(np.log(np.expm1(v)))
        return create_positive_variable(init, shape, device=device)

    # ---- variational parameters (dp_gp_lvm.py:62-74) ----
    if 'x_mean' in iv:
        x_init = np.asarray(iv['x_mean'], dtype=np.float64)
    else:
        x_init = pca(np.asarray(y_train) if train_obs is None else _missing.column_mean_filled(y_train, train_obs),
                     num_latent_dimensions=num_latent_dims)
    x_mean = _t(x_init)                                                        # [N x Q]
    x_var_raw = _raw_pos('x_var', 1.0, (num_samples, num_latent_dims))         # softplus(raw) = diag of q(X) covariance
    if 'x_u' in iv:
        x_u = _t(iv['x_u'])
    else:
        x_u = _t(np.random.permutation(x_init)[:num_inducing_points] +
                 np.random.normal(loc=0.0, scale=0.01, size=(num_inducing_points, num_latent_dims)))   # [M x Q]

    # ---- DP over the D output dims (:77-80) and the atoms of the kernel hyper-parameters (:84-94) ----
    dp_model = dirichlet_process(num_samples=num_dimensions, alpha_prior_params=alpha_prior_params,
                                 truncation_level=truncation_level, mask_size=mask_size, device=device)
    for key, name in (('logits', 'phi_logits'), ('gamma_1', 'gamma_1'), ('gamma_2', 'gamma_2')):
        if name in iv:
            v = np.asarray(iv[name], dtype=np.float64)
            dp_model.raw[key].copy_(_t(v if key == 'logits' else np.log(np.expm1(v))).reshape(dp_model.raw[key].shape))
    for i, name in enumerate(('w_1', 'w_2')):
        if name in iv:
            dp_model.raw['w'][i] = float(np.log(np.expm1(float(iv[name]))))
    gamma_atoms_raw = _raw_pos('gamma_atoms', GP_INIT_GAMMA, (truncation_level, num_latent_dims))
    sig_var_atoms_raw = _raw_pos('alpha_atoms', GP_INIT_ALPHA, (truncation_level, 1))
    beta_atoms_raw = _raw_pos('beta_atoms', GP_INIT_BETA, (truncation_level, 1))

    # the reference's creation order of its trainable tf.Variables (dp_gp_lvm.py:63-94, dirichlet_process.py:40-59)
    for v_ in (x_mean, x_var_raw, x_u, dp_model.raw['logits'], dp_model.raw['gamma_1'], dp_model.raw['gamma_2'],
               dp_model.raw['w'], gamma_atoms_raw, sig_var_atoms_raw, beta_atoms_raw):
        register_variable(v_, trainable=True)

    # ---- D-sharding ----
    if process_group is not None:
        import torch.distributed as dist
        rank, world = dist.get_rank(process_group), dist.get_world_size(process_group)
    elif _shard_of is not None:
        # test hook: behave as rank r of w WITHOUT a communicator — objective terms / gradients come back as this
        # rank's PARTIAL values (what would enter the all-reduce), so that one GPU can check the sharding arithmetic
        dist, (rank, world) = None, _shard_of
    else:
        dist, rank, world = None, 0, 1
    sharded = process_group is not None          # (a 1-rank group still goes through pack -> all_reduce -> finalize)
    if shard_by == 'observed':
        d_lo, d_hi = weighted_shard_bounds(train_obs.sum(axis=0) + 1, rank, world, mask_size)
    else:
        d_lo, d_hi = shard_bounds(num_dimensions, rank, world)
    d_local = d_hi - d_lo
    assert d_local > 0, 'more ranks than output dimensions'
    split = sharded or world > 1                 # (this object holds a share of the columns: prediction assembles over the ranks)
    y_local = _t(np.asarray(y_train)[:, d_lo:d_hi])                            # [N x D_local]

    # ---- device buffers of one objective evaluation (allocated once) ----
    f64 = dict(dtype=TORCH_DTYPE, device=device)
    buf = dict(gamma=torch.empty((d_local, num_latent_dims), **f64), alpha=torch.empty((d_local, 1), **f64),
               beta=torch.empty((d_local, 1), **f64), s=torch.empty((num_samples, num_latent_dims), **f64),
               phi=torch.empty((d_local, truncation_level), **f64),
               scal=torch.zeros(_lib.lib().dpgp_model_scal_count(d_local), **f64),
               red=torch.zeros(2, **f64), out=torch.zeros(5, **f64))
    # observed=: f_hat and its derivatives come from models/masked_bound_d.py; nothing of the fused pipeline is used (no workspace)
    # (sharded: the bound of the local columns; a share with no observed column is an empty batch)
    masked = _MaskedBoundD(np.asarray(y_train, dtype=np.float64)[:, d_lo:d_hi], train_obs[:, d_lo:d_hi], device) \
        if train_obs is not None else None
    workspace = ops.ElboWorkspace(d_local, num_samples, num_inducing_points, num_latent_dims, precision, device) \
        if masked is None else None
    s_1, s_2 = dp_model.prior

    # one training step through dpgp_elbo_step (mixed precision, where ops.elbo_step_supported offers it: M <= 128 and, by choice,
    # Q <= 20): the forward's psi2 dispatch is
    # replaced by the first pass of stage B (DPGP_FUSED_STEP=0: the three separate calls, e.g. for bench.py's per-stage breakdown)
    # fp64 forward + 'mixed' stage B: pair-tile or patch form by the conditioning of K_uu (see _gradients; DPGP_ADAPTIVE_STAGE_B=0: always
    # the patch form)
    DPGP_GUARD_REL = 2.0e-3                                  # (include/dpgp.h)
    adaptive_stage_b = (precision == 'f64' and backward_precision == 'mixed' and num_latent_dims <= 20 and
                        os.environ.get('DPGP_ADAPTIVE_STAGE_B', '1') != '0')
    step_ok = (grad_precision == 'mixed' and stage_b_precision in ('mixed', 'mixed_fast') and psi_algo == 'auto' and
               num_latent_dims <= 20 and os.environ.get('DPGP_FUSED_STEP', '1') != '0')
    fused_step = step_ok and ops.elbo_step_supported(num_inducing_points, num_latent_dims)
    split_step = step_ok and not fused_step            # (M > 128: the two halves of the step around the host-composed stage A)
    step_state = {}

    def grad_workspace():
        if precision != 'f32':
            return workspace
        if 'ws_mixed' not in step_state:
            step_state['ws_mixed'] = ops.ElboWorkspace(d_local, num_samples, num_inducing_points, num_latent_dims, 'mixed', device)
        return step_state['ws_mixed']

    def evaluate(events=None, out=None, _local_part_only=False, _step=False, _half_step=False, _grad=False):
        """One objective evaluation; returns the device tensor out[5] = (objective, f_hat, KL, DP objective, hyper-prior).
        Five launches: prepare, front (KL, y'y, K_uu tiles, operand constants, pair factors), psi1T_y,
        psi2 (+ the K_uu tasks), chain_b (+ the final reduction: sum, pack, finalize); D sharded: the all-reduce and the
        finalising launch follow."""
        lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
        r = dp_model.raw
        out = buf['out'] if out is None else out
        if masked is not None:
            return _evaluate_masked(out)[0]
        _lib.check(lib.dpgp_model_prepare(
            d_local, truncation_level, num_latent_dims, num_samples, d_lo, mask_size, r['logits'].data_ptr(),
            gamma_atoms_raw.data_ptr(), sig_var_atoms_raw.data_ptr(), beta_atoms_raw.data_ptr(), x_var_raw.data_ptr(),
            r['gamma_1'].data_ptr(), r['gamma_2'].data_ptr(), r['w'].data_ptr(), s_1, s_2, 1 if rank == 0 else 0,
            buf['gamma'].data_ptr(), buf['alpha'].data_ptr(), buf['beta'].data_ptr(), buf['s'].data_ptr(),
            buf['phi'].data_ptr(), buf['scal'].data_ptr(), st), 'dpgp_model_prepare')
        red = buf['red']
        # single GPU: the last kernel of the fused ELBO also packs and finalises; sharded: it packs, then one all-reduce
        if (_step or _half_step) and 'buf' not in step_state:
            step_state['buf'] = ops.ElboStepBuffers(d_local, num_samples, num_inducing_points, num_latent_dims, device)
        ws_ = grad_workspace() if (_step or _half_step or _grad) else workspace
        if _half_step:
            ops.elbo_fhat_step(y_local, x_u, x_mean, buf['s'], buf['gamma'], buf['alpha'], buf['beta'], ws_, step_state['buf'],
                               jitter=GP_DEFAULT_JITTER, model_tail=(buf['scal'], red, None if sharded else out))
        elif _step:
            step_state['grads'] = ops.elbo_step(y_local, x_u, x_mean, buf['s'], buf['gamma'], buf['alpha'], buf['beta'], ws_,
                                                step_state['buf'], jitter=GP_DEFAULT_JITTER,
                                                model_tail=(buf['scal'], red, None if sharded else out),
                                                stage_b=stage_b_precision)[1]
        else:
            ops.elbo_fhat(y_local, x_u, x_mean, buf['s'], buf['gamma'], buf['alpha'], buf['beta'],
                          jitter=GP_DEFAULT_JITTER, prec=grad_precision if _grad else precision, algo=psi_algo, workspace=ws_, events=events,
                          model_tail=(buf['scal'], red, None if sharded else out))
        if sharded and not _local_part_only:
            _exchange_and_finalise(out, ws_)
        return out

    def _evaluate_masked(out, grad=False):
        """observed=: prepare (the mixed gamma_d, alpha_d, beta_d, S, phi, scal as in the unmasked evaluation), the masked f_hat of the
        columns observed somewhere (models/masked_bound_d.py), KL over all rows, then pack and finalize: out[5] as evaluate().
        Launched eagerly, no host synchronisation.  Returns (out, stage-A/B derivatives or None)."""
        lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
        r = dp_model.raw
        _lib.check(lib.dpgp_model_prepare(
            d_local, truncation_level, num_latent_dims, num_samples, d_lo, mask_size, r['logits'].data_ptr(),
            gamma_atoms_raw.data_ptr(), sig_var_atoms_raw.data_ptr(), beta_atoms_raw.data_ptr(), x_var_raw.data_ptr(),
            r['gamma_1'].data_ptr(), r['gamma_2'].data_ptr(), r['w'].data_ptr(), s_1, s_2, 1 if rank == 0 else 0,
            buf['gamma'].data_ptr(), buf['alpha'].data_ptr(), buf['beta'].data_ptr(), buf['s'].data_ptr(), buf['phi'].data_ptr(),
            buf['scal'].data_ptr(), st), 'dpgp_model_prepare')
        with torch.no_grad():
            gam = masked.take(buf['gamma']).contiguous()
            al, be = masked.take(buf['alpha']).reshape(-1).contiguous(), masked.take(buf['beta']).reshape(-1).contiguous()
            res = masked.evaluate(x_u.detach(), x_mean.detach(), buf['s'], gam, al, be, grad=grad)
            f, grads = res if grad else (res, None)
            kl = ops.kl_qx(x_mean.detach(), buf['s']).reshape(1)
        _lib.check(lib.dpgp_model_pack(d_local, f.data_ptr(), buf['scal'].data_ptr(), buf['red'].data_ptr(), st), 'dpgp_model_pack')
        if sharded:                                         # the only exchange: (f_hat, DP objective) of the local columns
            dist.all_reduce(buf['red'], op=dist.ReduceOp.SUM, group=process_group)
        _lib.check(lib.dpgp_model_finalize(buf['red'].data_ptr(), kl.data_ptr(), buf['scal'][1:2].data_ptr(), out.data_ptr(), st),
                   'dpgp_model_finalize')
        return out, grads

    def _exchange_and_finalise(out, ws_=None):
        lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
        dist.all_reduce(buf['red'], op=dist.ReduceOp.SUM, group=process_group)    # the only exchange: 2 fp64 scalars
        _lib.check(lib.dpgp_model_finalize(buf['red'].data_ptr(), (ws_ or workspace).sums[1:2].data_ptr(), buf['scal'][1:2].data_ptr(),
                                           out.data_ptr(), st), 'dpgp_model_finalize')

    graph_state = {}

    def _evaluate_graph(out=None):
        """evaluate() replayed from a HIP graph (captured on first use): one hipGraphLaunch instead of five kernel launches
        and their argument marshalling on the host — at small per-GPU shares (D / 8 output dims) the host side of the eager
        path is as long as the kernels.  The graph reads the raw variables in place, so optimiser updates are seen.  With a
        process group the graph holds this rank's part (prepare ... pack); the 2-scalar all-reduce and the finalising kernel
        follow as ordinary calls (a collective inside a captured graph is transport-specific; this form works with any).
        Returns the same device tensor as evaluate(); `out` (optional, [5]) receives a copy on the stream."""
        if masked is not None:                           # (the masked path is launched eagerly: no capture)
            res = evaluate()
            if out is not None:
                out.copy_(res, non_blocking=True)
            return res
        if 'graph' not in graph_state:
            evaluate()                                   # (first call outside the capture: function attributes, warm-up)
            torch.cuda.synchronize()
            gph = torch.cuda.CUDAGraph()
            with _graph_capture(gph):
                evaluate(_local_part_only=True)
            graph_state['graph'] = gph
        graph_state['graph'].replay()
        if sharded:
            _exchange_and_finalise(buf['out'])
        if out is not None:
            out.copy_(buf['out'], non_blocking=True)
        return buf['out']

    grad_names = ('x_mean', 'x_var', 'x_u', 'dp_logits', 'dp_gamma_1', 'dp_gamma_2', 'dp_w', 'gamma_atoms', 'alpha_atoms',
                  'beta_atoms')

    grad_state = {}

    def _gradients(events=None):
        """d objective / d (raw trainable variables) — what tf.gradients(objective, trainable variables) gives the
        reference's optimiser (test/synthetic_data_hard_test.py:143-155).  dpgp_elbo_step (one call: forward, stage A, stage B;
        mixed precision, where ops.elbo_step_supported offers it: M <= 128, Q <= 20) or one forward evaluation, then
        dpgp_elbo_grad_chain and dpgp_elbo_grad_psi; then
        dpgp_model_backward; sharded over D, the per-GPU
        partial gradients are packed into one buffer and sum-all-reduced.  Returns {name: tensor} keyed like ``raw``.
        events: optional list of 4 torch.cuda.Event(enable_timing=True), recorded after the forward evaluation, stage A,
        stage B and the chain rule to the raw variables (bench.py's breakdown)."""
        lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
        gws = grad_workspace() if masked is None else None
        mark = (lambda i: events[i].record()) if events is not None else (lambda i: None)
        r = dp_model.raw
        info = gws.info if masked is None else None
        if masked is not None:
            # observed=: forward, dense adjoints and the weighted stage B of the columns observed somewhere; a never-observed
            # column's rows of d_gamma and d_alpha_beta are zero (its DP terms reach the logits through dpgp_model_backward)
            _, (dmu, ds, dz, dg, dab) = _evaluate_masked(buf['out'], grad=True)
            mark(0), mark(1)
            dg, dab, info = masked.scatter(dg), masked.scatter(dab), masked.info
            mark(2)
        elif fused_step and events is None:
            evaluate(_step=True)
            dmu, ds, dz, dg, dab, _ = step_state['grads']
        elif split_step and events is None:
            evaluate(_half_step=True)
            gp, wk, gv, dab, _ = ops.elbo_grad_chain(buf['alpha'], buf['beta'], gws, jitter=GP_DEFAULT_JITTER, z=x_u,
                                                     gamma=buf['gamma'], psi2_slabs=1)
            dmu, ds, dz, dg = ops.elbo_grad_psi_step(y_local, x_u, x_mean, buf['s'], buf['gamma'], buf['alpha'], gp, wk, gv, gws,
                                                     step_state['buf'], stage_b=stage_b_precision)
        else:
            evaluate(_grad=True)
            mark(0)
            gp, wk, gv, dab, _ = ops.elbo_grad_chain(buf['alpha'], buf['beta'], gws, jitter=GP_DEFAULT_JITTER, z=x_u,
                                                     gamma=buf['gamma'])
            mark(1)
            form = stage_b_precision
            if adaptive_stage_b:
                # the training configuration (fp64 forward, matrix-pipe stage B): the pair-tile form of the Psi2 term (4.6 ms at config 3)
                # while K_uu is well conditioned, the patch form (7.5 ms) once it is not — the pair form accumulates the a'- and b-weighted
                # exponentials separately and loses accuracy where they cancel (include/dpgp.h, DPGP_PREC_MIXED_PATCH: 7e-3 against 2e-3 of
                # the largest gradient entry at the ill-conditioned fixture, whose guard bound is 80 x the threshold).  The measure is the
                # conditioning-guard bound the forward evaluation computes in every precision (one host read per step: 10 ms of fp64
                # forward pass are in front of it); the switch sits at a tenth of the threshold a mixed forward pass is flagged at.
                bound = float(gws.guard.max())
                form = 'mixed' if bound <= 0.1 * DPGP_GUARD_REL * num_samples else 'mixed_patch'
                grad_state['stage_b_form'] = form
            dmu, ds, dz, dg = ops.elbo_grad_psi(y_local, x_u, x_mean, buf['s'], buf['gamma'], buf['alpha'], gp, wk, gv,
                                                prec=form)
            mark(2)
        rows = r['logits'].shape[0]
        sizes = [num_samples * num_latent_dims, num_samples * num_latent_dims, num_inducing_points * num_latent_dims,
                 rows * truncation_level, max(truncation_level - 1, 1), max(truncation_level - 1, 1), 2,
                 truncation_level * num_latent_dims, truncation_level, truncation_level]
        flat = torch.zeros(sum(sizes) + 1, **f64)          # (+1: this rank's trouble flag, summed over ranks with the rest)
        parts = list(torch.split(flat, sizes + [1]))[:-1]
        t_ = truncation_level
        _lib.check(lib.dpgp_model_backward(
            d_local, t_, num_latent_dims, num_samples, num_inducing_points, d_lo, mask_size, rows, r['logits'].data_ptr(),
            gamma_atoms_raw.data_ptr(), sig_var_atoms_raw.data_ptr(), beta_atoms_raw.data_ptr(), x_var_raw.data_ptr(),
            r['gamma_1'].data_ptr(), r['gamma_2'].data_ptr(), r['w'].data_ptr(), x_mean.data_ptr(), buf['phi'].data_ptr(),
            s_1, s_2, 1 if rank == 0 else 0, dmu.data_ptr(), ds.data_ptr(), dz.data_ptr(), dg.data_ptr(), dab.data_ptr(),
            *[p_.data_ptr() for p_ in parts], st), 'dpgp_model_backward')
        mark(3)
        # trouble flag of the LOCAL output dims (a Cholesky / conditioning flag of the forward evaluation or a non-finite
        # partial gradient), reduced with the gradients: every rank sees the same decision (optimise() branches on it)
        _lib.check(lib.dpgp_trouble_flag(flat.numel() - 1, flat.data_ptr(), info.numel(), info.data_ptr(),
                                         flat[-1:].data_ptr(), st), 'dpgp_trouble_flag')
        if sharded:
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=process_group)      # one packed exchange (N Q x 2 + M Q + ...)
        grad_state['flag'] = flat[-1]
        shapes = [x_mean.shape, x_var_raw.shape, x_u.shape, r['logits'].shape, r['gamma_1'].shape, r['gamma_2'].shape,
                  r['w'].shape, gamma_atoms_raw.shape, sig_var_atoms_raw.shape, beta_atoms_raw.shape]
        return {k: p_[:int(np.prod(sh))].reshape(sh) for k, p_, sh in zip(grad_names, parts, shapes)}

    def _optimise(num_iterations, learning_rate=0.01, callback=None):
        """Adam on the raw variables with the HIP gradients (the reference: tf.train.AdamOptimizer(...).minimize(objective),
        test/synthetic_data_hard_test.py:143-155).  torch.optim.Adam only applies the update (plumbing).

        Every iteration checks the flags of the evaluation — failed factorisation, the conditioning guard of the fp32 Psi2
        (DPGP_INFO_ILL_CONDITIONED, include/dpgp.h), non-finite gradients — as ONE value that travels with the packed gradient
        all-reduce, so all ranks of a sharded run take the same branch, and raises FloatingPointError (the reference's
        tf.cholesky raises InvalidArgumentError there) instead of updating parameters with meaningless gradients.
        precision='mixed' carries Psi2 in fp32: once training drives K_uu towards singularity (long length scales: its small
        eigenvalues approach the 1e-8 jitter) that is no longer the reference's objective and the guard fires (DESIGN.md
        section 5).  The training configuration that follows the reference's fp64 arithmetic all the way is
        precision='f64', backward_precision='mixed': fp64 forward and dense adjoints, the streaming stage of the backward pass
        on the matrix pipe.  Returns {'iterations', 'precision', 'backward_precision'}."""
        params = dict(x_mean=x_mean, x_var=x_var_raw, x_u=x_u, dp_logits=dp_model.raw['logits'],
                      dp_gamma_1=dp_model.raw['gamma_1'], dp_gamma_2=dp_model.raw['gamma_2'], dp_w=dp_model.raw['w'],
                      gamma_atoms=gamma_atoms_raw, alpha_atoms=sig_var_atoms_raw, beta_atoms=beta_atoms_raw)
        opt = _adam(list(params.values()), learning_rate)
        for it in range(num_iterations):
            g = _gradients()
            if float(grad_state['flag']) != 0.0:                                 # identical on every rank
                raise FloatingPointError(
                    'iteration %d: failed Cholesky factorisation, ill-conditioning flag or non-finite gradient in '
                    'precision=%r (info codes of this rank: %s).  The fp32 psi-statistics of precision="mixed" stop being a '
                    'substitute for the reference\'s fp64 once K_uu is nearly singular: build the model with '
                    'precision="f64", backward_precision="mixed".'
                    % (it, precision, sorted(set((workspace.info if masked is None else masked.info).unique().tolist()) - {0})))
            for k, p_ in params.items():
                p_.grad = g[k].reshape(p_.shape)                                 # (views of this step's own packed buffer: no copy)
            opt.step()
            if callback is not None:
                callback(it)
        return {'iterations': num_iterations, 'precision': precision,
                'backward_precision': backward_precision or precision}

    def _mixed():
        phi = dp_model.assignments                                               # [D x T], all output dims
        return (phi @ F.softplus(gamma_atoms_raw), phi @ F.softplus(sig_var_atoms_raw), phi @ F.softplus(beta_atoms_raw))

    pred_state = {}

    def _start(y_test, use_pca, x_test_mean, x_test_var, neighbour):
        """q(X*) as dp_gp_lvm.py:246-262 (models/test_latents.start), registered as prediction variables."""
        xt_, st__ = _latents.start(y_test.shape[0], num_latent_dims, device, x_test_mean, x_test_var, use_pca, y_test, neighbour)
        # q(X*): the reference creates these two as NON-trainable tf.Variables (dp_gp_lvm.py:258-262), which is what
        # get_prediction_variables() hands to the test-time optimiser (test/frey_faces_prediction.py:165-171)
        pred_state['x_test_mean'] = register_variable(xt_, trainable=False)
        pred_state['x_test_var_raw'] = register_variable(torch.log(torch.expm1(st__)), trainable=False)
        return xt_, st__

    def _first_columns_start(y_test, do, use_pca, x_test_mean, x_test_var):
        """The start for test points observed in their first `do` output dims: nearest neighbour over those columns."""
        return _start(y_test, use_pca, x_test_mean, x_test_var,
                      lambda: _latents.l2_neighbour(np.asarray(y_train)[:, :do], y_test, x_mean.detach().cpu().numpy()))

    def _fhat_on(y_t, xt, st_, dims=None):
        """f_hat (fused ELBO, dpgp_elbo_fhat) of the first `dims` output dims on (y_t, q(X*)) with the trained kernel and
        inducing inputs, and KL(q(X*) || p(X*)); uses the mixed hyper-parameters of the last evaluate()."""
        dd = num_dimensions if dims is None else dims
        ws_t = ops.ElboWorkspace(dd, y_t.shape[0], num_inducing_points, num_latent_dims, precision, device)
        terms_t, sums, info = ops.elbo_fhat(y_t, x_u, xt, st_, buf['gamma'][:dd].contiguous(), buf['alpha'][:dd].contiguous(),
                                      buf['beta'][:dd].contiguous(), jitter=GP_DEFAULT_JITTER, prec=precision, workspace=ws_t)
        pred_state['terms'] = terms_t.clone()
        return sums[0].clone(), sums[1].clone()

    ONE_GPU = "on a model sharded over a process group the test-time paths run the shared-inducing masked bound only: pass " \
              "observed= with form='shared' (form='slots' and the reference's own forms of the prediction paths run on one GPU)"

    def _masked(y_test, observed, predict=False, reference_compat=False, form='shared'):
        assert not split or form == 'shared', ONE_GPU
        return _missing.masked_arguments(y_test, observed, num_dimensions, predict, reference_compat)

    def _masked_bound(y0, obs, form='slots'):
        """The fp64 test bound with one slot per output dim that has an observed entry: that dim's mixed (gamma, alpha, beta) of
        this evaluate() and the shared inducing inputs.  Returns (bound, the training-side evaluation out[5]).
        form='shared': the same bound on ONE copy of the inducing inputs (models/frozen_bound_d.py), no slots.
        A sharded model ('shared' only): the bound of the local columns that have an observed test entry, wrapped so that one
        evaluation is one packed all-reduce (frozen_bound_d._ShardedTestBoundD); `out` is the global training-side evaluation."""
        out = evaluate().clone()
        if split:
            assert form == 'shared', ONE_GPU
            here = np.flatnonzero(obs[:, d_lo:d_hi].any(axis=0))                 # local indices
            idx = torch.as_tensor(here, device=device)
            local = _TestBoundD(x_u.detach(), buf['gamma'][idx], buf['alpha'][idx, 0], buf['beta'][idx, 0], _t(y0[:, d_lo + here]),
                                _t(obs[:, d_lo + here].T), device) if here.size else None
            pred_state['missing_columns'] = _missing.missing_columns(obs)
            return _ShardedTestBoundD(local, obs.shape[0], num_latent_dims, device, process_group if sharded else None), out
        cols = np.flatnonzero(obs.any(axis=0))
        idx = torch.as_tensor(cols, device=device)
        if form == 'shared':
            bound = _TestBoundD(x_u.detach(), buf['gamma'][idx], buf['alpha'][idx, 0], buf['beta'][idx, 0], _t(y0[:, cols]),
                                _t(obs[:, cols].T), device)
            pred_state['missing_columns'] = _missing.missing_columns(obs)
            return bound, out
        bound = _TestBound.slots(x_u.detach(), buf['gamma'][idx], buf['alpha'][idx, 0], buf['beta'][idx, 0],
                                 _t(y0[:, cols].T[:, :, None]), np.ones(cols.size), _t(obs[:, cols].T), device)
        pred_state['missing_columns'] = _missing.missing_columns(obs)
        return bound, out

    def _masked_init(y0, obs, use_pca, x_test_mean, x_test_var):
        """The start of q(X*) on the full y_train and the full masks (every rank holds them).  A start the caller did not supply
        draws np.random.normal noise: sharded, rank 0's is broadcast once, so that the replicas of q(X*) start bit-identical."""
        xt, st_ = _masked_init_local(y0, obs, use_pca, x_test_mean, x_test_var)
        if sharded and x_test_mean is None:
            dist.broadcast(xt, src=dist.get_global_rank(process_group, 0), group=process_group)
        return xt, st_

    def _masked_init_local(y0, obs, use_pca, x_test_mean, x_test_var):
        return _start(y0, use_pca, x_test_mean, x_test_var,
                      lambda: _latents.masked_neighbour(np.asarray(y_train), train_obs, y0, obs, x_mean.detach().cpu().numpy()))

    def _predictive_moments(cols, xt, st_):
        """Predictive mean [N* x Du] and covariance [Du x N* x N*] of the output dims `cols` at q(X*) (dp_gp_lvm.py:426-498)."""
        num_test_points, m_ = xt.shape[0], num_inducing_points
        idx = torch.as_tensor(np.asarray(cols), device=device)
        gu, au, bu = buf['gamma'][idx].contiguous(), buf['alpha'][:, 0][idx].contiguous(), buf['beta'][:, 0][idx].contiguous()
        s_train = F.softplus(x_var_raw)
        psi_1 = ops.psi1(x_u, x_mean, s_train, gu, au)                          # [Du x N x M]
        psi_2 = ops.psi2(x_u, x_mean, s_train, gu, au)
        psi_1t = ops.psi1(x_u, xt, st_, gu, au)                                  # [Du x N* x M]
        psi_2t = ops.psi2(x_u, xt, st_, gu, au)
        k_uu = ops.ard_rbf_gram(x_u, None, gu, au, bu, include_noise=False, include_jitter=True, jitter=GP_DEFAULT_JITTER)
        l_uu, _ = ops.potrf_batched(k_uu)
        h = ops.trsm_batched(l_uu, psi_2)
        a_mat = bu[:, None, None] * ops.trsm_batched(l_uu, h.transpose(1, 2).contiguous()).transpose(1, 2) + \
            torch.eye(m_, dtype=TORCH_DTYPE, device=device)
        l_a, _ = ops.potrf_batched(a_mat.contiguous())
        c = ops.trsm_batched(l_a, ops.trsm_batched(l_uu, psi_1.transpose(1, 2).contiguous()))          # [Du x M x N]
        c_pred = ops.trsm_batched(l_a, ops.trsm_batched(l_uu, psi_1t.transpose(1, 2).contiguous()))   # [Du x M x N*]
        y_u = _t(np.asarray(y_train)[:, np.asarray(cols)]).transpose(0, 1).contiguous()[:, :, None]    # [Du x N x 1]
        cy = ops.matmul(c, y_u)                                                # [Du x M x 1]
        predicted_mean = (bu[:, None] * ops.matmul(c_pred.transpose(1, 2), cy)[:, :, 0]).transpose(0, 1)   # [N* x Du]
        eye = torch.eye(m_, dtype=TORCH_DTYPE, device=device).expand(len(cols), m_, m_).contiguous()
        l_uu_inv, l_a_inv = ops.trsm_batched(l_uu, eye), ops.trsm_batched(l_a, eye)
        ainv = ops.matmul(l_a_inv.transpose(1, 2), l_a_inv)                    # A^-1
        g = psi_2t - ops.matmul(psi_1t.transpose(1, 2), psi_1t)               # [Du x M x M]
        scale_yu = ops.matmul(ops.matmul(ops.matmul(l_uu_inv.transpose(1, 2), ops.matmul(ainv, l_uu_inv)),
                                         psi_1.transpose(1, 2)), y_u)       # [Du x M x 1]
        yu_var = bu * bu * ops.matmul(scale_yu.transpose(1, 2), ops.matmul(g, scale_yu))[:, 0, 0]
        tr_term = torch.diagonal(ops.matmul(ops.matmul(l_uu_inv.transpose(1, 2), ops.matmul(eye - ainv, l_uu_inv)),
                                            psi_2t), dim1=-2, dim2=-1).sum(-1)
        psi_0t = ops.psi0(num_test_points, au)[:, 0]
        predicted_covar = yu_var[:, None, None] + (psi_0t + 1.0 / bu + tr_term)[:, None, None] * \
            torch.eye(num_test_points, dtype=TORCH_DTYPE, device=device)
        return predicted_mean, predicted_covar

    def _marginals_at(cols, xt, st_):
        """Per-entry predictive moments (mean, var) [N* x len(cols)] of the output dims `cols` at q(X*): every column is its own
        mixed kernel (gamma_d, alpha_d, beta_d of the last evaluation), so the operator runs in its K = len(cols), G = J = 1
        layout: c_d = K_d^-1 - P_d, P_d = (K_d + beta_d Psi2_d)^-1, r_d = beta_d P_d Psi1_d^T y_d; no Psi1* [K, N*, M] is formed.
        The trace term enters with the derived sign, - tr((K_d^-1 - P_d) Psi2*(n)).  _predictive_moments' tr_term is the same
        quantity, + tr((K_d^-1 - P_d) Psi2*) summed over the test points, and is ADDED there (following the reference), so
            sum_n var(n,d) = predicted_covar[d,0,0] + (N* - 1)/beta_d - 2 tr_term_d."""
        if masked is not None:
            return _marginals_at_masked(cols, xt, st_)
        idx = torch.as_tensor(np.asarray(cols) - d_lo, device=device)           # (cols: global, within this rank's [d_lo, d_hi))
        f64 = lambda a: a.to(TORCH_DTYPE).contiguous()
        gu, au, bu = f64(buf['gamma'][idx]), f64(buf['alpha'][:, 0][idx]), f64(buf['beta'][:, 0][idx])
        z, mu, s_train = f64(x_u.detach()), f64(x_mean.detach()), f64(F.softplus(x_var_raw).detach())
        psi_1 = ops.psi1(z, mu, s_train, gu, au)                                 # [K x N x M] (training)
        psi_2 = ops.psi2(z, mu, s_train, gu, au)
        k_uu = ops.ard_rbf_gram(z, None, gu, au, bu, include_noise=False, include_jitter=True, jitter=GP_DEFAULT_JITTER)
        li, _ = collapsed.factors(k_uu)
        r0 = collapsed.Chain(li, psi_2, bu).r0
        y_u = _t(np.asarray(y_train)[:, np.asarray(cols)]).to(TORCH_DTYPE).transpose(0, 1).contiguous()[:, :, None]
        r, c = collapsed.posterior(r0, collapsed.k_inverse(li), bu, ops.matmul(psi_1.transpose(1, 2), y_u))      # r [K x M x 1]
        gidx = torch.zeros((len(cols), 1), dtype=torch.int32, device=device)
        mean, var = ops.qx_psi_point_moments(z[None].expand(len(cols), -1, -1).contiguous(), f64(xt), f64(st_), gu, au,
                                             c[:, None].contiguous(), r.contiguous(), gidx, bu)
        return mean[:, :, 0].transpose(0, 1).contiguous(), var[:, :, 0].transpose(0, 1).contiguous()

    def _marginals_at_masked(cols, xt, st_):
        """_marginals_at on a model trained with observed=: Psi2_d is the weighted sum over the rows at which column d was measured and
        Psi1_d^T y_d comes from ops.psi1T_y on the zero-filled data (no [K, N, M] array); a column never observed has no posterior:
        mean 0, variance alpha_d + 1/beta_d."""
        cols = np.asarray(cols) - d_lo                                     # (given global, within this rank's [d_lo, d_hi))
        pos = np.searchsorted(masked.cols_np, cols)
        seen = np.isin(cols, masked.cols_np)                               # (masked.cols_np may be empty: a share never observed)
        idx = torch.as_tensor(cols, device=device)
        au, bu = buf['alpha'][:, 0][idx].contiguous(), buf['beta'][:, 0][idx].contiguous()
        prior_var = (au + 1.0 / bu)[None, :].expand(xt.shape[0], -1)
        mean, var = torch.zeros((xt.shape[0], cols.size), dtype=TORCH_DTYPE, device=device), prior_var.clone()
        if seen.any():
            here = torch.as_tensor(np.flatnonzero(seen), device=device)
            sel = torch.as_tensor(pos[seen], dtype=torch.long, device=device)
            gu, a_, b_ = buf['gamma'][idx[here]].contiguous(), au[here].contiguous(), bu[here].contiguous()
            z = x_u.detach()
            c, rhs = masked.posterior(z, x_mean.detach(), F.softplus(x_var_raw).detach(), gu, a_, b_, sel=sel)
            k_ = int(sel.numel())
            gidx = torch.zeros((k_, 1), dtype=torch.int32, device=device)
            mn, vr = ops.qx_psi_point_moments(z[None].expand(k_, -1, -1).contiguous(), xt.contiguous(), st_.contiguous(), gu, a_,
                                              c[:, None].contiguous(), rhs[:, :, None].contiguous(), gidx, b_)
            mean[:, here], var[:, here] = mn[:, :, 0].transpose(0, 1), vr[:, :, 0].transpose(0, 1)
        return mean, var

    def _frozen_columns(cols):
        """The training side of _marginals_at / _marginals_at_masked of the output dims `cols`, formed once: the arguments of
        predictor.of_columns (z, gamma [K,Q], alpha [K], beta [K], c [K,M,M], r [K,M], here, prior_var [J], scatter) for the K
        columns of `cols` that were observed in training, at the places `here`."""
        cols = np.asarray(cols)
        idx = torch.as_tensor(cols, device=device)
        f64 = lambda a: a.to(TORCH_DTYPE).contiguous()
        z, mu, s_train = f64(x_u.detach()), f64(x_mean.detach()), f64(F.softplus(x_var_raw).detach())
        if masked is None:
            gu, au, bu = f64(buf['gamma'][idx]), f64(buf['alpha'][:, 0][idx]), f64(buf['beta'][:, 0][idx])
            psi_1 = ops.psi1(z, mu, s_train, gu, au)
            psi_2 = ops.psi2(z, mu, s_train, gu, au)
            k_uu = ops.ard_rbf_gram(z, None, gu, au, bu, include_noise=False, include_jitter=True, jitter=GP_DEFAULT_JITTER)
            li, _ = collapsed.factors(k_uu)
            r0 = collapsed.Chain(li, psi_2, bu).r0
            y_u = _t(np.asarray(y_train)[:, cols]).to(TORCH_DTYPE).transpose(0, 1).contiguous()[:, :, None]
            r, c = collapsed.posterior(r0, collapsed.k_inverse(li), bu, ops.matmul(psi_1.transpose(1, 2), y_u))
            here = torch.arange(cols.size, device=device)
            return z, gu, au, bu, c.contiguous(), r[:, :, 0].contiguous(), here, au + 1.0 / bu, False
        pos, seen = np.searchsorted(masked.cols_np, cols), np.isin(cols, masked.cols_np)
        au, bu = buf['alpha'][:, 0][idx].contiguous(), buf['beta'][:, 0][idx].contiguous()
        here = torch.as_tensor(np.flatnonzero(seen), dtype=torch.long, device=device)
        gu, a_, b_ = buf['gamma'][idx[here]].contiguous(), au[here].contiguous(), bu[here].contiguous()
        c = rhs = None
        if seen.any():
            sel = torch.as_tensor(pos[seen], dtype=torch.long, device=device)
            c, rhs = masked.posterior(x_u.detach(), x_mean.detach(), F.softplus(x_var_raw).detach(), gu, a_, b_, sel=sel)
            c, rhs = f64(c), f64(rhs)
        return z, f64(gu), f64(a_), f64(b_), c, rhs, here, f64(au + 1.0 / bu), True

    def _frozen_predictor(cols):
        """_frozen_columns as a predictor.FrozenPredictor (its forward is _marginals_at's operator call on the same arrays)."""
        return _predictor.of_columns(*_frozen_columns(cols), device)

    def _latent_geometry(cols):
        """The pieces of the Jacobian and the metric of the output dims `cols`: the observed columns as the K kernels of a
        marginals._Marginals with one column each (None when no column of `cols` was observed in training), their places `here`,
        and sum_d alpha_d diag(gamma_d) [Q x Q] over the columns never observed (the prior of their Jacobian rows)."""
        z, gu, au, bu, c, r, here, _, _ = _frozen_columns(cols)
        idx = torch.as_tensor(np.asarray(cols), device=device)
        prior = buf['alpha'][:, 0][idx].to(TORCH_DTYPE)[:, None] * buf['gamma'][idx].to(TORCH_DTYPE)              # [J, Q]
        unseen = torch.ones(len(cols), dtype=torch.bool, device=device)
        unseen[here] = False
        prior_unseen = torch.diag_embed(torch.sum(prior[unseen], dim=0))
        k = int(here.numel())
        if not k:
            return None, here, prior_unseen
        marg = _marginals._Marginals(z[None].expand(k, -1, -1), gu, au, bu, None, c[:, None], r[:, :, None],
                                     torch.zeros((k, 1), dtype=torch.int32, device=device))
        return marg, here, prior_unseen

    def _column_marginals(cols):
        """The output dims `cols` as the K = len(cols) kernels of a marginals._Marginals with one column and one pattern each
        (every column is its own mixed kernel): only these kernels are gathered, never all D.  A column never observed in
        training keeps c = 0 and r = 0: its posterior is its prior."""
        z, gu, au, bu, c, r, here, _, _ = _frozen_columns(cols)
        idx = torch.as_tensor(np.asarray(cols), device=device)
        k, m = len(cols), z.shape[0]
        f64 = lambda a: a.to(TORCH_DTYPE).contiguous()
        g_all, a_all, b_all = f64(buf['gamma'][idx]), f64(buf['alpha'][:, 0][idx]), f64(buf['beta'][:, 0][idx])
        c_all = torch.zeros((k, m, m), dtype=TORCH_DTYPE, device=device)
        r_all = torch.zeros((k, m), dtype=TORCH_DTYPE, device=device)
        if int(here.numel()):
            c_all[here], r_all[here] = c, r
        return _marginals._Marginals(z[None].expand(k, -1, -1), g_all, a_all, b_all, None, c_all[:, None], r_all[:, :, None],
                                     torch.zeros((k, 1), dtype=torch.int32, device=device), all_seen=True)

    def _geometry_columns(columns):
        cols = np.arange(num_dimensions) if columns is None else np.asarray(columns, dtype=np.int64).reshape(-1)
        assert cols.size >= 1 and cols.min() >= 0 and cols.max() < num_dimensions, 'columns must be output dims in [0, D)'
        return cols

    def _require_unsharded(name):
        assert not split, '%s is not built for a model sharded over a process group' % name

    def _metric_under(columns, name):
        """latent_geometry's hook: the marginals.Metric under latent_metric(., columns), _latent_geometry's kernels with their
        (P, prior) and the prior of the columns never observed, formed once; that prior alone when no chosen column was
        observed in training."""
        _require_unsharded(name)
        cols = _geometry_columns(columns)
        evaluate()
        with torch.no_grad():
            marg, _, prior_unseen = _latent_geometry(cols)
            parts = [] if marg is None else [(marg,) + marg._metric_operands(None, None)]
            return _marginals.Metric(parts, prior_unseen[None])

    def _assembled_marginals(cols, xt, st_):
        """_marginals_at of the GLOBAL output dims `cols` (any order) on a sharded model: this rank computes the columns it owns
        into a zero-filled [2 x N* x len(cols)] buffer, one sum all-reduce completes it; every rank returns the same (mean, var).
        Without a communicator (_shard_of) the other ranks' columns stay zero."""
        cols = np.asarray(cols, dtype=np.int64).reshape(-1)
        pair = torch.zeros((2, xt.shape[0], cols.size), dtype=TORCH_DTYPE, device=device)
        own = np.flatnonzero((cols >= d_lo) & (cols < d_hi))
        if own.size:
            mean, var = _marginals_at(cols[own], xt, st_)
            at = torch.as_tensor(own, device=device)
            pair[0].index_copy_(1, at, mean)
            pair[1].index_copy_(1, at, var)
        if sharded:
            dist.all_reduce(pair, op=dist.ReduceOp.SUM, group=process_group)
        return pair[0], pair[1]

    def _reference_form_not_built(name, how):
        raise NotImplementedError("%s: the reference's form of this call is not built for a model trained with observed=: %s"
                                  % (name, how))

    def _form_arg(form, observed):
        assert form in ('slots', 'shared'), "form must be 'slots' or 'shared'"
        assert form == 'slots' or observed is not None, "form='shared' is the masked test bound: it needs observed="

    class DP_GP_LVM(LatentGeometry, Trainable):
        """Accessors as in the reference (dp_gp_lvm.py:161-231,502-508).  The latent-geometry methods are
        models/latent_geometry.LatentGeometry's, every column under its own mixed kernel: an operator call runs over
        K = len(columns) kernels and is summed over them in blocks of points; with the columns of one discovered group they show
        that group's own energy, the paths it considers short and where its manifold takes a motion.  Not built for a model
        sharded over a process group: AssertionError."""
        _latent_dims, _device = num_latent_dims, device
        _metric_of, _require_built = staticmethod(_metric_under), staticmethod(_require_unsharded)
        raw = dict(x_mean=x_mean, x_var=x_var_raw, x_u=x_u, gamma_atoms=gamma_atoms_raw, alpha_atoms=sig_var_atoms_raw,
                   beta_atoms=beta_atoms_raw, **{'dp_' + k: v for k, v in dp_model.raw.items()})
        shard = (d_lo, d_hi)

        @property
        def assignments(self):
            return dp_model.assignments

        @property
        def dp(self):
            return dp_model

        @property
        def dp_atoms(self):
            return F.softplus(gamma_atoms_raw), F.softplus(sig_var_atoms_raw), F.softplus(beta_atoms_raw)

        @property
        def kernel(self):
            g, a, b = _mixed()
            return k_ard_rbf(gamma=g, alpha=a, beta=b)                           # batch size D (:105)

        @property
        def ard_weights(self):
            return _mixed()[0]

        @property
        def signal_variance(self):
            return _mixed()[1]

        @property
        def noise_precision(self):
            return _mixed()[2]

        @property
        def inducing_input(self):
            return x_u

        @property
        def q_x(self):
            return x_mean, torch.diag_embed(F.softplus(x_var_raw))               # mean [N x Q], covariance [N x Q x Q]

        @property
        def objective(self):
            """dp.objective - (f_hat - KL) - hyper-prior (dp_gp_lvm.py:154): 0-d fp64 device tensor."""
            return evaluate()[0].clone()

        @property
        def objective_terms(self):
            """(objective, f_hat, KL, DP objective, hyper-prior log-likelihood) of one evaluation, as a device tensor."""
            return evaluate().clone()

        @property
        def per_dimension_terms(self):
            """[D_local x 5] f_hat terms and the info flags of the last evaluation (0 fine, > 0 failed factorisation,
            DPGP_INFO_ILL_CONDITIONED = -2: fp32 Psi2 no longer trustworthy for this output dim).  A model trained with observed=:
            [D_local x 5] and [D_local], zero rows for the columns never observed."""
            if masked is not None:
                if masked.terms is None:
                    evaluate()
                return masked.scatter(masked.terms), masked.scatter(masked.info)
            return workspace.terms, workspace.info

        @property
        def conditioning_guard(self):
            """[D_local] bound on what the rounding of an fp32 Psi2 can move each output dim's f_hat terms by (last
            evaluation; computed in every precision mode; flagged in info when > DPGP_GUARD_REL * N in mixed / f32); None for a model
            trained with observed= (fp64 throughout, no fused evaluation)."""
            return None if masked is not None else workspace.guard

        @property
        def last_stage_b_form(self):
            """'mixed' (pair-tile form) or 'mixed_patch' (patch form): what the last gradients() of the training configuration
            (precision='f64', backward_precision='mixed') chose for the Psi2 term by the conditioning-guard bound; None otherwise."""
            return grad_state.get('stage_b_form')

        evaluate_ = staticmethod(evaluate)
        evaluate_graph = staticmethod(_evaluate_graph)

        @staticmethod
        def partial_pack():
            """(f_hat, DP objective) shares of the local output dims after one evaluation: the 2-vector that is
            sum-all-reduced when D is sharded (tests of the sharding arithmetic)."""
            evaluate()
            return buf['red'].clone()

        gradients = staticmethod(_gradients)
        optimise = staticmethod(_optimise)

        @property
        def prediction_terms(self):
            """[D* x 5] f_hat terms of the test points in the last predict_* call (the observed dims for missing data; with
            `observed`: [slots x 5], one slot per output dim that has an observed entry, ascending).  On a sharded model it stays
            local: the slots of this rank's columns ([0 x 5] where none of them has an observed test entry)."""
            return pred_state.get('terms')

        @property
        def missing_columns(self):
            """The output dims whose moments the last predict_missing_data returned (ascending), or None."""
            return pred_state.get('missing_columns')

        @staticmethod
        def _reference_defect(num_test_points):
            """What the reference's own prediction bounds contain on top of the bound (dp_gp_lvm.py:292, :409): there
            `tf.trace(...)` is [D] while psi_0_test and beta are [D x 1], so beta * (trace - psi_0) broadcasts to [D x D] and the
            reduce_sum adds  1/2 sum_ij beta_i (tr_j - psi0_i) - 1/2 sum_i beta_i (tr_i - psi0_i)."""
            terms_t = pred_state['terms']
            dd = terms_t.shape[0]
            al, be = buf['alpha'][:dd, 0], buf['beta'][:dd, 0]
            psi0 = al * num_test_points
            tr = 2.0 * terms_t[:, 2] / be + psi0                                  # term 2 = beta/2 (tr - alpha N*)
            return 0.5 * torch.sum(be[:, None] * (tr[None, :] - psi0[:, None])) - 0.5 * torch.sum(be * (tr - psi0))

        @staticmethod
        def predict_new_latent_variables(y_test, use_pca=False, x_test_mean=None, x_test_var=None, reference_compat=False,
                                         observed=None):
            """Mirror of dp_gp_lvm.py:233-309: q(X*) for fully observed test data y_test [N* x D] and the prediction lower bound
                f_hat + f_hat_test - KL(q(X)) - KL(q(X*)),    test log-likelihood = f_hat_test - KL(q(X*)),
            (without the reference's broadcasting defect in its beta (trace - psi_0) term, dp_gp_lvm.py:292 — see
            oracle/gen_golden_predict.py; `reference_compat=True` returns the reference's own numbers, defect included)
            where f_hat_test is the SAME fused ELBO evaluated on (y_test, q(X*)) with the trained kernel and inducing inputs
            (one more dpgp_elbo_fhat call).  Returns (prediction_lower_bound, x_test_mean [N* x Q], x_test_covar [N* x Q x Q],
            test_log_likelihood) at the initial q(X*): nearest training neighbour + N(0, 0.01^2) noise, or PCA of y_test
            (`use_pca`), or the given x_test_mean / x_test_var (values; what a caller's optimiser of q(X*) passes back in).

            On a model trained with observed=: the call takes observed=, a boolean [N* x D] mask as in predict_missing_data
            (utils.missing.observed_mask(y_test) for gaps marked by NaN, all True for complete rows); f_hat_test is the
            shared-inducing masked test bound (models/frozen_bound_d.py) with every measured entry counting, the training-side f_hat
            the model's own masked one, q(X*) starts at the nearest training neighbour over the jointly observed columns.
            Without observed= it is the reference's call, which such a model does not take: NotImplementedError.  AssertionError
            for reference_compat=True; observed= is taken by such a model and by a sharded model only.

            On a model sharded over a process group (trained on complete data or with observed=) the call takes observed= in the
            same way: each rank evaluates the shared-inducing bound on its columns, ONE packed all-reduce sums f_hat*, KL(q(X*)) is
            added once on every rank; a start of q(X*) that was not supplied is rank 0's, broadcast.  Without observed=:
            AssertionError (the reference's form runs on one GPU)."""
            if masked is not None or (split and observed is not None):
                if observed is None:
                    _reference_form_not_built('predict_new_latent_variables', 'pass observed=, the mask of the measured entries of '
                                              'y_test [N* x D] (utils.missing.observed_mask(y_test) reads it off the NaNs)')
                y0, obs = _masked(y_test, observed, reference_compat=reference_compat)
                xt, st_ = _masked_init(y0, obs, use_pca, x_test_mean, x_test_var)
                bound, out = _masked_bound(y0, obs, 'shared')
                f_hat_test, kl_test = _latents.bound_at(bound, xt, st_)
                pred_state['terms'] = bound.terms
                with torch.no_grad():
                    test_ll = f_hat_test - kl_test
                    return out[1] - out[2] + test_ll, xt, torch.diag_embed(st_), test_ll
            assert observed is None, 'observed= is taken by a model trained with observed='
            assert not split, ONE_GPU
            y_test = np.asarray(y_test, dtype=np.float64)
            num_test_points, test_dims = np.shape(y_test)
            assert test_dims == num_dimensions, \
                'Observed dimensionality for prediction must be equal to the dimensionality of the training data.'
            xt, st_ = _first_columns_start(y_test, num_dimensions, use_pca, x_test_mean, x_test_var)
            out = evaluate().clone()                                                 # (objective, f_hat, KL, DP, hyper)
            f_hat_test, kl_test = _fhat_on(_t(y_test), xt, st_)
            lower_bound = out[1] + f_hat_test - out[2] - kl_test
            test_ll = f_hat_test - kl_test
            if reference_compat:                                                 # the reference's own numbers (see _reference_defect)
                extra = DP_GP_LVM._reference_defect(num_test_points)
                lower_bound, test_ll = lower_bound + extra, test_ll + extra
            return lower_bound, xt, torch.diag_embed(st_), test_ll

        @staticmethod
        def test_latent_gradients(y_test, x_test_mean, x_test_var, observed=None, form='slots'):
            """d (f_hat_test - KL(q(X*))) / d (x_test_mean, x_test_var) with the trained model fixed — what TensorFlow's autograd
            gives a caller of the reference who optimises q(X*) on the bounds returned by predict_*; y_test [N* x Do], Do <= D
            (the first Do output dims).  Uses the backward pass of the fused ELBO (stages A and B) on the test points.
            observed: as predict_missing_data (y_test [N* x D]; True everywhere is allowed here): the gradient of the masked
            bound, fp64, by the weighted test-point operators.  form (with observed only, AssertionError otherwise): 'slots', one
            slot with its own copy of Z, Psi1* and adjoint per output dim, or 'shared', the same bound on one copy of Z with no
            [D x N* x M] array (models/frozen_bound_d.py, ops.psi_latent_adjoint).
            On a model sharded over a process group: observed= with form='shared' only (AssertionError otherwise); each rank
            evaluates its columns, ONE all-reduce of the packed (f_hat*, d mu*, d S*) — 1 + 2 N* Q fp64 values — sums them, the KL
            gradient is added once on every rank; prediction_terms then holds this rank's columns only."""
            _form_arg(form, observed)
            if observed is not None:
                y0, obs = _masked(y_test, observed, form=form)
                bound, _ = _masked_bound(y0, obs, form)
                with torch.no_grad():
                    grads = _latents.ascent_gradient(bound, _latents.latent_values(x_test_mean, device, num_latent_dims, y0.shape[0]),
                                                     _latents.latent_values(x_test_var, device, num_latent_dims, y0.shape[0]))
                    pred_state['terms'] = bound.terms
                return grads
            assert not split, ONE_GPU
            y_t = _t(np.asarray(y_test, dtype=np.float64))
            dd = y_t.shape[1]
            xt, st_ = _latents.latent_values(x_test_mean, device, num_latent_dims, y_t.shape[0]), \
                _latents.latent_values(x_test_var, device, num_latent_dims, y_t.shape[0])
            evaluate()
            gam, al, be = buf['gamma'][:dd].contiguous(), buf['alpha'][:dd].contiguous(), buf['beta'][:dd].contiguous()
            ws_t = ops.ElboWorkspace(dd, y_t.shape[0], num_inducing_points, num_latent_dims, precision, device)
            ops.elbo_fhat(y_t, x_u, xt, st_, gam, al, be, jitter=GP_DEFAULT_JITTER, prec=precision, workspace=ws_t)
            gp, wk, gv, _, _ = ops.elbo_grad_chain(al, be, ws_t, jitter=GP_DEFAULT_JITTER, z=x_u, gamma=gam)
            dmu, ds, _, _ = ops.elbo_grad_psi(y_t, x_u, xt, st_, gam, al, gp, wk, gv, prec=precision)
            k_mu, k_s = _latents.kl_gradient(xt, st_)
            return dmu - k_mu, ds - k_s

        @staticmethod
        def optimise_test_latents(y_test, num_iterations=200, learning_rate=0.01, use_pca=False, x_test_mean=None,
                                  x_test_var=None, observed=None, form='slots'):
            """Adam on q(X*) (mean and softplus-parametrised variances) maximising f_hat_test - KL(q(X*)) for test points
            observed in their first Do output dims; returns (x_test_mean, x_test_var) to hand to predict_*.  observed: as
            predict_missing_data; the slots' factors are formed once, no host synchronisation inside the loop.  form: as
            test_latent_gradients.  On a model sharded over a process group (observed= with form='shared' only): one packed
            all-reduce per iteration; a start that is not supplied is rank 0's, broadcast once, and every rank applies the same
            reduced gradient, so the ranks' q(X*) stay bit-identical."""
            _form_arg(form, observed)
            if observed is not None:
                y0, obs = _masked(y_test, observed, form=form)
                xt, st_ = _masked_init(y0, obs, use_pca, x_test_mean, x_test_var)
                bound, _ = _masked_bound(y0, obs, form)
                with torch.no_grad():
                    fitted = _latents.fit(functools.partial(_latents.ascent_gradient, bound), xt, st_, num_iterations, learning_rate)
                    pred_state['terms'] = bound.terms
                    return fitted
            assert not split, ONE_GPU
            y_test = np.asarray(y_test, dtype=np.float64)
            xt, st_ = _first_columns_start(y_test, y_test.shape[1], use_pca, x_test_mean, x_test_var)
            # (every iteration is one public test_latent_gradients call: an evaluate(), a workspace and a host round trip of q(X*))
            return _latents.fit(functools.partial(DP_GP_LVM.test_latent_gradients, y_test), xt, st_, num_iterations, learning_rate)

        @staticmethod
        def predictive_marginals(x_test_mean, x_test_var, columns=None):
            """(mean, var), each [N* x len(columns)]: the per-entry predictive moments of the output dims `columns` (default: all
            D) at q(X*) = (x_test_mean, x_test_var [N* x Q]) under each column's mixed kernel of this evaluation, observation
            noise 1/beta_d included; one call of ops.qx_psi_point_moments (see _marginals_at for the formulas and for the sign
            of the trace term against predict_missing_data's array).  fp64, torch.no_grad.  On a model sharded over a process
            group (any precision, with or without observed=): `columns` are global, each rank computes those it owns and one sum
            all-reduce assembles the pair in the caller's column order, the same tensors on every rank."""
            cols = _geometry_columns(columns)
            val = lambda a: _t(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
            evaluate()
            with torch.no_grad():
                return (_assembled_marginals if split else _marginals_at)(cols, val(x_test_mean), val(x_test_var))

        @staticmethod
        def frozen_predictor(columns=None):
            """A models/predictor.FrozenPredictor of the output dims `columns` (default: all D): p(x_mean, x_var) gives the bits of
            predictive_marginals, differentiably in q(X*); p.vjp is its vector-Jacobian product (ops.psi_latent_adjoint: the
            columns' kernels share Z and q(X*)).  The training side is built once, here, at the model's current parameters: stale
            after further training.  Not built for a model sharded over a process group: AssertionError."""
            _require_unsharded('frozen_predictor')
            cols = _geometry_columns(columns)
            evaluate()
            with torch.no_grad():
                return _frozen_predictor(cols)

        @staticmethod
        def predictive_jacobian(x, columns=None):
            """[N* x len(columns) x Q]: the mean of the Jacobian d f_d / d x of the noise-free map of the output dims `columns`
            (default: all D) at the DETERMINISTIC latent points x [N* x Q] (numpy or torch), b_d(x)^T r_d under each column's
            mixed kernel of this evaluation: the derivative of predictive_marginals' mean at x_test_var = 0.  One call of
            ops.ard_rbf_point_jacobian with every column its own kernel; the features [D, N*, M, Q] are never formed.  A column
            never observed in training has a zero row.  The training side is built once per call.  fp64, torch.no_grad.  Not
            built for a model sharded over a process group: AssertionError."""
            _require_unsharded('predictive_jacobian')
            cols = _geometry_columns(columns)
            xp = _marginals.points_arg(x, num_latent_dims, device)
            evaluate()
            with torch.no_grad():
                marg, here, _ = _latent_geometry(cols)
                out = torch.zeros((xp.shape[0], cols.size, num_latent_dims), dtype=TORCH_DTYPE, device=device)
                if marg is not None:
                    out[:, here] = marg.jacobian(xp)[:, :, 0].transpose(0, 1)
                return out

        @staticmethod
        def latent_metric(x, columns=None):
            """[N* x Q x Q]: the expected Riemannian metric G(x) = sum_d E[J_d J_d^T] of the map from latent space to the output
            dims `columns` (default: all D) at the latent points x [N* x Q] (Tosi et al., UAI 2014; formulas in
            models/marginals.py), every column under its own mixed kernel: one call of ops.ard_rbf_point_metric over
            K = len(columns) kernels, summed over them in blocks of points.  With the columns of one discovered group it shows which region and which
            latent directions that group uses.  A column never observed in training contributes alpha_d diag(gamma_d).  fp64.
            Not built for a model sharded over a process group: AssertionError."""
            _require_unsharded('latent_metric')
            cols = _geometry_columns(columns)
            xp = _marginals.points_arg(x, num_latent_dims, device)
            evaluate()
            with torch.no_grad():
                marg, _, prior_unseen = _latent_geometry(cols)
                g = prior_unseen[None].expand(xp.shape[0], -1, -1)
                return g.clone() if marg is None else marg.metric_total(xp) + g

        @staticmethod
        def predictive_covariance(x, columns=None, noise=False):
            """[len(columns) x N* x N*]: the joint posterior covariance of the noise-free functions of the output dims `columns`
            (default: all D) at the DETERMINISTIC latent points x [N* x Q] (numpy or torch), every column under its own mixed
            kernel,
                cov_d(x, x') = alpha_d exp(-1/2 sum_q gamma_dq (x_q - x'_q)^2) - k_d(x)^T (K_d^-1 - P_d) k_d(x')
            (models/marginals.py): one call of ops.ard_rbf_point_cov over K = len(columns) kernels; only the chosen columns'
            kernels are formed.  Its diagonal plus 1/beta_d is predictive_marginals(x, 0)'s variance; noise=True adds 1/beta_d
            on the diagonal.  A column never observed in training gets its prior gram.  Exactly symmetric.  The array is
            J N*^2 doubles (here every column has its own matrix; in the other models columns of one (kernel, pattern) repeat the
            same one).  Works on a model trained on complete data and on one trained with observed=.  fp64, torch.no_grad.  Not
            built for a model sharded over a process group: AssertionError."""
            _require_unsharded('predictive_covariance')
            cols = _geometry_columns(columns)
            xp = _marginals.points_arg(x, num_latent_dims, device)
            evaluate()
            with torch.no_grad():
                marg = _column_marginals(cols)
                cov = marg.covariance(xp)[:, 0]
                return _marginals.with_noise(cov, 1.0 / marg.beta) if noise else cov

        @staticmethod
        def sample_functions(x, num_samples=1, columns=None, noise=False, jitter=_marginals.DEFAULT_SAMPLE_JITTER, seed=0,
                             draws=None):
            """[S x N* x len(columns)]: S joint draws of the output dims `columns` (default: all D) at the latent points x
            [N* x Q]: mean + L_d xi with L_d L_d^T = predictive_covariance_d + jitter alpha_d I (+ 1/beta_d I with noise), xi
            standard normal from a device torch.Generator seeded with `seed`, or given as `draws` [S x N* x len(columns)].  One
            ops.potrf_batched call and one ops.matmul over the columns' kernels, whatever their number; one host read,
            potrf's info at the end: FloatingPointError if a factorisation failed (raise `jitter` or set noise=True).  The
            default jitter, 1e-6 alpha_d, is a choice, not a measurement: the gram of nearby points has its smallest eigenvalue
            below rounding and the factorisation needs a shift well above eps N* lambda_max ~ 1e-12 alpha; 1e-6 alpha is far
            above that and far below any 1/beta the models train to.  fp64, torch.no_grad.  Not built for a model sharded over a
            process group: AssertionError."""
            _require_unsharded('sample_functions')
            cols = _geometry_columns(columns)
            xp = _marginals.points_arg(x, num_latent_dims, device)
            evaluate()
            with torch.no_grad():
                xi = _marginals.standard_draws(draws, num_samples, xp.shape[0], cols.size, _marginals.draw_generator(seed, device),
                                               device)
                f, info = _column_marginals(cols).sample(xp, xi.permute(2, 0, 1)[:, :, :, None], None, noise, jitter)
                _marginals.raise_if_not_factorised(info)
                return f[:, :, :, 0].permute(1, 2, 0).contiguous()

        @staticmethod
        def predict_missing_data(y_test, use_pca=False, x_test_mean=None, x_test_var=None, reference_compat=False,
                                 observed=None, marginal_variance=False, form='slots'):
            """Mirror of dp_gp_lvm.py:311-500: y_test [N* x Do] holds the FIRST Do output dims of the test points; returns
            (missing_data_lower_bound, x_test_mean, x_test_covar, predicted_mean [N* x Du], predicted_covar [Du x N* x N*])
            for the remaining Du = D - Do dims at the initial q(X*) (see predict_new_latent_variables).  Composed of the
            library's operators (Psi statistics at q(X*), batched Cholesky / triangular solves) and plain fp64 GEMMs.

            observed (extension): a boolean [N* x D] mask of the entries of y_test [N* x D] that were measured, any pattern
            (entries where it is False are ignored and may be NaN).  The bound is f_hat + f_hat*(masked) - KL(q(X)) - KL(q(X*)):
            output dim d enters f_hat* with the test points at which it was measured, as one slot of the weighted test-point
            operators (fp64 whatever `precision` is; the training-side f_hat and KL are the model's own evaluation);
            KL(q(X*)) runs over all N* rows.  The Du predicted dims are the columns with at least one unobserved entry,
            ascending (property missing_columns); q(X*) starts at the masked nearest neighbour (a row with nothing observed
            at 0).  AssertionError for a non-boolean mask, a shape mismatch, a mask that is True everywhere, or
            reference_compat=True.

            marginal_variance=True (extension): the last entry is the per-entry variance [N* x Du] of predictive_marginals on
            the predicted dims in place of the [Du x N* x N*] array.

            form (with observed only, AssertionError otherwise): 'slots' or 'shared', as test_latent_gradients: how f_hat* is evaluated.

            On a model trained with observed=: y_test is [N* x D] (the reference's first-Do-columns form, a narrower y_test without
            observed=, is not built for such a model: NotImplementedError), observed defaults to utils.missing.observed_mask(y_test)
            (NaN = missing); f_hat* is always the shared-inducing bound, the training-side f_hat the model's own masked one, and the
            last two entries are the per-entry moments of predictive_marginals on missing_columns, predicted_mean [N* x Du] and
            predicted_var [N* x Du] — per entry whatever marginal_variance says (no [Du x N* x N*] array is built for such a
            model).  AssertionError for reference_compat=True.

            On a model sharded over a process group: observed= with form='shared' (a mask-trained model always runs that bound);
            the bound is global — the training-side f_hat and KL of the sharded evaluation, f_hat* summed over the ranks by ONE
            packed all-reduce, KL(q(X*)) subtracted once — and the last two entries are predictive_marginals' per-entry moments
            [N* x Du] of the global missing_columns, assembled by one sum all-reduce, whatever marginal_variance says; every rank
            returns the same tensors.  prediction_terms stays local: this rank's columns only."""
            _form_arg(form, observed if masked is None else True)
            if split and masked is None:
                assert observed is not None and form == 'shared', ONE_GPU
            if masked is not None or split:
                if observed is None and np.ndim(y_test) == 2 and np.shape(y_test)[1] != num_dimensions:
                    _reference_form_not_built('predict_missing_data', 'pass y_test [N* x D] with NaN at the missing entries, or with observed=')
                y0, obs = _masked(y_test, _missing.observed_mask(y_test) if observed is None else observed, predict=True,
                                  reference_compat=reference_compat)
                xt, st_ = _masked_init(y0, obs, use_pca, x_test_mean, x_test_var)
                bound, out = _masked_bound(y0, obs, 'shared')
                f_hat_test, kl_test = _latents.bound_at(bound, xt, st_)
                pred_state['terms'] = bound.terms
                with torch.no_grad():
                    lower_bound = out[1] + f_hat_test - out[2] - kl_test
                    predicted_mean, predicted_var = (_assembled_marginals if split else _marginals_at_masked)(
                        pred_state['missing_columns'], xt, st_)
                return lower_bound, xt, torch.diag_embed(st_), predicted_mean, predicted_var
            if observed is not None:
                y0, obs = _masked(y_test, observed, predict=True, reference_compat=reference_compat)
                xt, st_ = _masked_init(y0, obs, use_pca, x_test_mean, x_test_var)
                bound, out = _masked_bound(y0, obs, form)
                f_hat_test, kl_test = _latents.bound_at(bound, xt, st_)
                pred_state['terms'] = bound.terms
                with torch.no_grad():
                    lower_bound = out[1] + f_hat_test - out[2] - kl_test
                    predicted_mean, predicted_covar = _predictive_moments(pred_state['missing_columns'], xt, st_)
                    if marginal_variance:
                        predicted_covar = _marginals_at(pred_state['missing_columns'], xt, st_)[1]
                return lower_bound, xt, torch.diag_embed(st_), predicted_mean, predicted_covar
            assert not split, ONE_GPU
            y_test = np.asarray(y_test, dtype=np.float64)
            num_test_points, num_observed_dims = np.shape(y_test)
            assert num_observed_dims < num_dimensions, \
                'Observed dimensionality for missing data scenario must be less than total ' \
                'dimensionality of training data.'
            do = num_observed_dims
            xt, st_ = _first_columns_start(y_test, do, use_pca, x_test_mean, x_test_var)
            out = evaluate().clone()
            f_hat_test, kl_test = _fhat_on(_t(y_test), xt, st_, dims=do)
            lower_bound = out[1] + f_hat_test - out[2] - kl_test
            if reference_compat:
                lower_bound = lower_bound + DP_GP_LVM._reference_defect(num_test_points)
            # predictive mean / covariance of the unobserved dims (:426-498), output dims do .. D-1 only
            pred_state['missing_columns'] = np.arange(do, num_dimensions)
            predicted_mean, predicted_covar = _predictive_moments(pred_state['missing_columns'], xt, st_)
            if marginal_variance:
                with torch.no_grad():
                    predicted_covar = _marginals_at(pred_state['missing_columns'], xt, st_)[1]
            return lower_bound, xt, torch.diag_embed(st_), predicted_mean, predicted_covar

        @staticmethod
        def impute_training_data(return_variance=False):
            """A model trained with observed=: y_train [N x D] with every unobserved entry (n, d) replaced by the posterior mean
            beta_d Psi1_d[n,:] (K_d + beta_d Psi2_d)^-1 Psi1_d^T y_d (Psi2_d and y_d over the rows at which d was observed); observed
            entries as given, a never-observed column 0.  fp64 device tensor.  return_variance=True: (filled, var), var [N x D] the
            per-entry variance of predictive_marginals at the training q(X) at the unobserved entries and 0 at the observed ones;
            filled is the same tensor either way.  On a model sharded over a process group each rank computes its columns and one
            sum all-reduce assembles them: filled (and var) are [N x D] and the same on every rank."""
            assert masked is not None, 'impute_training_data needs a model trained with observed='
            evaluate()
            with torch.no_grad():
                mean, var = (_assembled_marginals if split else _marginals_at_masked)(
                    np.arange(num_dimensions), x_mean.detach(), F.softplus(x_var_raw).detach())
                obs = torch.as_tensor(train_obs, device=device)
                filled = torch.where(obs, _t(y_train) if split else y_local, mean)
                return (filled, torch.where(obs, torch.zeros_like(var), var)) if return_variance else filled

    return DP_GP_LVM()


def dp_gp_lvm_t(y_train,
                num_latent_dims=GP_LVM_DEFAULT_LATENT_DIMENSIONS,
                num_inducing_points=GP_LVM_DEFAULT_NUM_INDUCING_POINTS,
                truncation_level=DP_DEFAULT_TRUNCATION_LEVEL,
                alpha_prior_params=DP_DEFAULT_ALPHA_PRIOR_PARAMS,
                mask_size=1,
                seed=0,
                device=None, precision=None, initial_values=None, _view_of_many=False, process_group=None, observed=None):
    """
    Over-T formulation — mirror of the reference's ``dp_gp_lvm_t`` factory (src/models/dp_gp_lvm.py:513-676), SURVEY.md
    §8(f) row 3: the kernel batch is the T atoms, the mixture weights phi [T x D] enter outside the kernel, so an evaluation
    needs T Psi2's instead of D.  A different objective from ``dp_gp_lvm`` away from equal atoms (equal at the reference's
    initialisation, test/unittests/dpgplvm_unitttests.py:544-548).  Objective and gradients, composed of the library's
    operators in the B_t = K_t + beta_t Psi2_t algebra of DESIGN.md §2:

        Psi1 [T,N,M], Psi2 [T,M,M], K_uu [T,M,M]       dpgp_psi1 / dpgp_psi2 / dpgp_ard_rbf_gram      (:611-620)
        L_K, L_B = chol(K), chol(K + beta Psi2)         dpgp_potrf_batched                             (:620,633)
        <K^-1, Psi2> by two triangular solves           dpgp_trsm_batched                              (:622-629)
        V = Psi1^T Y  [T,M,D]                           dpgp_gemm_strided_f64 (fp64 MFMA, ops.matmul)
        C = L_B^-1 V, 1/2 sum_td phi_td beta_t^2 |C_td|^2   dpgp_trsm_batched                          (:638-658)

    precision: 'f64', or 'mixed' = the Psi statistics in fp32 (f16-split MFMA kernels), everything after them in fp64.
    process_group: a torch.distributed group -> the D output dims are sharded over its ranks as in ``dp_gp_lvm``
    (shard_bounds): the T-atom chain is replicated (it does not depend on D), V = Psi1^T Y, the solves and every sum over d
    run on the local columns; an evaluation exchanges ONE scalar (the local f_hat), a gradient evaluation ONE packed
    all-reduce of all raw-variable gradients plus the trouble flag of optimise().
    observed (extension): a boolean [N x D] mask of the entries of y_train that were measured, any pattern with at least one True
    (entries where it is False are ignored and may be NaN).  f_hat is then the sum over the columns d observed somewhere of
    -1/2 N_d log 2 pi + sum_t phi_td F_t(y_d on its rows R_d): T x P slots, P the number of distinct row patterns
    (models/masked_bound_t.py), fp64 (precision None or 'f64'), one GPU (process_group None).  KL(q(X)) runs over all N rows, the
    DP objective over all D columns, the hyper-prior over the T atoms; a column never observed contributes its DP terms only, a
    row never observed its KL only.  x_mean defaults to the PCA of the column-mean-filled data.  impute_training_data() fills
    the gaps with the mixture's posterior mean.  DPGP_GROUPED_PSI=0 runs the Psi statistics and their adjoints in the slot form
    on the weighted operators (cross-checks only).
    """
    num_samples, num_dimensions = np.shape(y_train)
    # (_view_of_many: one view of a multi-view model, whose own check is against the views' total dimensionality)
    assert 0 < num_latent_dims < num_dimensions or _view_of_many, \
        'Number of latent dimensions must be postive and less than the dimensionality of the observed data.'
    assert 0 < num_inducing_points <= num_samples, \
        'Number of inducing points must be positive and less than or equal to the number of observations in the ' \
        'observed data.'
    assert 0 < truncation_level <= min(num_samples, num_dimensions), \
        'The truncation level must be positive and less than or equal to the dimensionality of the observed data and ' \
        'less than or equal to the number of observations.'
    assert isinstance(seed, int) and seed >= 0, 'Seed must be a 32-bit unsigned integer, i.e., 0 <= seed <= 2^32 - 1.'
    train_obs = None
    if observed is not None:
        assert precision in (None, 'f64'), "with observed, precision must be None or 'f64' (the masked model is fp64)"
        assert process_group is None, 'with observed, process_group must be None (the masked model is not sharded)'
        train_obs = _missing.check_observed(observed, (num_samples, num_dimensions))
        assert train_obs.any(), 'observed must hold at least one True entry'
        y_train = _missing.zero_filled(y_train, train_obs)
    precision = 'f64' if precision is None else precision     # (default: the reference's arithmetic, as in dp_gp_lvm)
    assert precision in ('mixed', 'f64'), "precision must be 'mixed' or 'f64'"
    np.random.seed(seed=seed)
    device = default_device() if device is None else torch.device(device)
    iv = dict(initial_values or {})

    def _t(a):
        return torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=TORCH_DTYPE, device=device).contiguous()

    def _raw_pos(name, init, shape):
        if name in iv:
            return _t(np.log(np.expm1(np.asarray(iv[name], dtype=np.float64).reshape(shape))))
        return create_positive_variable(init, shape, device=device)

    x_init = np.asarray(iv['x_mean'], dtype=np.float64) if 'x_mean' in iv else \
        pca(np.asarray(y_train) if train_obs is None else _missing.column_mean_filled(y_train, train_obs),
            num_latent_dimensions=num_latent_dims)
    x_mean = _t(x_init)
    x_var_raw = _raw_pos('x_var', 1.0, (num_samples, num_latent_dims))
    x_u = _t(iv['x_u']) if 'x_u' in iv else \
        _t(np.random.permutation(x_init)[:num_inducing_points] +
           np.random.normal(loc=0.0, scale=0.01, size=(num_inducing_points, num_latent_dims)))
    dp_model = dirichlet_process(num_samples=num_dimensions, alpha_prior_params=alpha_prior_params,
                                 truncation_level=truncation_level, mask_size=mask_size, device=device)
    for key, name in (('logits', 'phi_logits'), ('gamma_1', 'gamma_1'), ('gamma_2', 'gamma_2')):
        if name in iv:
            v = np.asarray(iv[name], dtype=np.float64)
            dp_model.raw[key].copy_(_t(v if key == 'logits' else np.log(np.expm1(v))).reshape(dp_model.raw[key].shape))
    for i, name in enumerate(('w_1', 'w_2')):
        if name in iv:
            dp_model.raw['w'][i] = float(np.log(np.expm1(float(iv[name]))))
    gamma_atoms_raw = _raw_pos('gamma_atoms', GP_INIT_GAMMA, (truncation_level, num_latent_dims))
    sig_var_atoms_raw = _raw_pos('alpha_atoms', GP_INIT_ALPHA, (truncation_level, 1))
    beta_atoms_raw = _raw_pos('beta_atoms', GP_INIT_BETA, (truncation_level, 1))
    sharded = process_group is not None
    if sharded:
        import torch.distributed as dist
        rank, world = dist.get_rank(process_group), dist.get_world_size(process_group)
        assert world <= num_dimensions, 'more ranks than output dimensions'
    else:
        rank, world = 0, 1
    d_lo, d_hi = shard_bounds(num_dimensions, rank, world)
    y_dev = _t(np.asarray(y_train)[:, d_lo:d_hi])                              # the local columns
    yy = torch.sum(y_dev * y_dev, dim=0)                                       # [D_local]
    from ..distributions.log_normal import log_pdf as log_normal_log_pdf
    from ..distributions.beta import entropy as beta_dist_entropy
    from ..distributions.gamma import entropy as gamma_dist_entropy
    from ..distributions.multinomial import entropy as multinomial_dist_entropy
    s_1, s_2 = dp_model.prior
    n_, d_, m_ = num_samples, d_hi - d_lo, num_inducing_points             # (d_: the LOCAL output dims; the sums over d are local)
    mp_ = 16 * ((m_ + 15) // 16)
    last_info = [torch.zeros((), dtype=torch.int32, device=device)]
    # the fused forward pass (csrc/elbo.hip, dpgp_elbo_fhat_t): M <= 128 and at least T local output dims; otherwise, and
    # whenever gradients are wanted, f_hat is composed of the library's operators (_FHatT)
    fused_t = ops.ElboTWorkspace(truncation_level, d_, n_, m_, num_latent_dims, precision, device) \
        if (ops.elbo_fhat_t_supported(m_) and d_ >= truncation_level and device.type == 'cuda' and train_obs is None
            and os.environ.get('DPGP_FUSED_T', '1') != '0') else None       # (DPGP_FUSED_T=0: cross-checks only)
    # observed=: f_hat and its derivatives come from the T x P slot bound (models/masked_bound_t.py); everything around them
    # (transforms, KL, DP objective, hyper-prior, chain rule to the raw variables) is the unmasked model's
    masked = _MaskedBoundT(np.asarray(y_train, dtype=np.float64), train_obs, truncation_level, device) \
        if train_obs is not None else None

    def _chain(x_u_, x_mean_, s_, gat, aat, bat):
        """Psi statistics and the Cholesky factors of the T atoms (library operators)."""
        pt = torch.float32 if precision == 'mixed' else TORCH_DTYPE
        cast = lambda a: a.to(pt).contiguous()
        psi_1 = ops.psi1(cast(x_u_), cast(x_mean_), cast(s_), cast(gat), cast(aat)).to(TORCH_DTYPE)   # [T x N x M]
        psi_2 = ops.psi2(cast(x_u_), cast(x_mean_), cast(s_), cast(gat), cast(aat)).to(TORCH_DTYPE)   # [T x M x M]
        k_uu = ops.ard_rbf_gram(x_u_, None, gat, aat, bat, include_noise=False, include_jitter=True,
                                jitter=GP_DEFAULT_JITTER)                                              # [T x M x M]
        l_k, info_k = ops.potrf_batched(k_uu)
        l_b, info_b = ops.potrf_batched(k_uu + bat[:, None, None] * psi_2)
        last_info[0] = torch.maximum(info_k.abs().max(), info_b.abs().max())
        return psi_1, psi_2, k_uu, l_k, l_b

    def _fhat_forward(x_mean_, s_, x_u_, gat, aat, bat, phit, for_backward=True):
        """f_hat of dp_gp_lvm.py:617-667 from the library's operators; returns (f_hat, what the backward pass needs).
        for_backward: K^-1 and B^-1 are formed once here (two inverses of the triangular factors + two products) and serve the trace,
        the solve against V and the whole backward pass — six latency-bound batched solves of T small matrices otherwise."""
        psi_1, psi_2, k_uu, l_k, l_b = _chain(x_u_, x_mean_, s_, gat, aat, bat)
        v = ops.matmul(psi_1.transpose(1, 2), y_dev)                       # [T x M x D]
        k_inv = b_inv = None
        if for_backward:
            li = ops.tril_inverse_batched(l_k)                             # (M a multiple of 128: the persistent solve, one launch)
            k_inv = ops.matmul(li.transpose(1, 2), li)
            li = ops.tril_inverse_batched(l_b)
            b_inv = ops.matmul(li.transpose(1, 2), li)
            tr = torch.sum(k_inv * psi_2, dim=(1, 2))                        # tr(L^-1 Psi2 L^-T) = <K^-1, Psi2>
            c = ops.matmul(li, v)                                          # L_B^-1 V
        else:
            h = ops.trsm_batched(l_k, psi_2)
            tr = torch.diagonal(ops.trsm_batched(l_k, h.transpose(1, 2).contiguous()), dim1=-2, dim2=-1).sum(-1)
            c = ops.trsm_batched(l_b, v)
        logdet = torch.log(torch.diagonal(l_b, dim1=-2, dim2=-1)).sum(-1) - \
            torch.log(torch.diagonal(l_k, dim1=-2, dim2=-1)).sum(-1)
        quad = bat[:, None] ** 2 * torch.sum(c * c, dim=1)                   # [T x D]
        per_t = 0.5 * (n_ * torch.log(bat) + bat * (tr - n_ * aat)) - logdet
        f_hat = -0.5 * n_ * d_ * np.log(2.0 * np.pi) + torch.sum(phit * per_t[:, None]) \
            - 0.5 * torch.sum(phit * bat[:, None] * yy[None, :]) + 0.5 * torch.sum(phit * quad)
        return f_hat, (x_mean_, s_, x_u_, gat, aat, bat, phit, psi_2, k_uu, k_inv, b_inv, v, per_t, quad, tr)

    def _fhat_backward(saved):
        """d f_hat / d (x_mean, S, x_u, gamma atoms, alpha atoms, beta atoms, phi^T): the adjoints of the per-atom dense algebra
        (torch on [T, M, M] arrays, T small) and the library's streaming stage B (dpgp_elbo_grad_psi_ex: Psi2 term on the matrix
        pipe, Psi1 term with the full adjoint beta^2 Y diag(phi_t) W_t^T, K_uu term)."""
        x_mean_, s_, x_u_, gat, aat, bat, phit, p2, k_uu, k_inv, b_inv, v, per_t, quad, tr = saved
        eye = torch.eye(m_, dtype=TORCH_DTYPE, device=device)
        st = phit.sum(dim=1)[:, None, None]                                  # s_t = sum_d phi_td
        be = bat[:, None, None]
        w = ops.matmul(b_inv, v)                                           # [T x M x D]
        wphi = w * phit[:, None, :]
        vwphi = torch.sum(v * wphi, dim=(1, 2))                              # sum_d phi_td v_td^T B^-1 v_td
        ww = ops.matmul(wphi, w.transpose(1, 2))
        gb = -0.5 * st * b_inv - 0.5 * be * be * ww
        # gk = 1/2 s_t (K^-1 - B^-1 - beta K^-1 Psi2 K^-1) + .. and gp = 1/2 s_t beta (K^-1 - B^-1) + .. from K^-1 - B^-1 = beta K^-1 Psi2 B^-1
        # as products: the differences cancel to O(beta |Psi2| / |K_uu|) of |K^-1| (a small noise precision, beta ~ 1 / var(y) for y far
        # from unit scale, left 1e-3 of d/dx_u in their rounding)
        kp = ops.matmul(k_inv, p2)                                         # K^-1 Psi2
        kpb = ops.matmul(kp, b_inv)                                        # K^-1 Psi2 B^-1 (symmetric in exact arithmetic)
        sym = lambda a: 0.5 * (a + a.transpose(1, 2))
        gk = sym(-0.5 * st * be * be * ops.matmul(kp, kpb)) - 0.5 * be * be * ww
        gp = sym(0.5 * st * be * be * kpb) - 0.5 * be * be * be * ww
        wk = gk * (k_uu - GP_DEFAULT_JITTER * eye)
        g1 = be * be * ops.matmul(y_dev, wphi.transpose(1, 2))             # [T x N x M] adjoint of Psi1
        pad2 = (0, mp_ - m_, 0, mp_ - m_)
        dmu, ds, dz, dgam = ops.elbo_grad_psi(None, x_u_, x_mean_, s_, gat, aat,
                                              torch.nn.functional.pad(gp, pad2).contiguous(),
                                              torch.nn.functional.pad(wk, pad2).contiguous(), None,
                                              prec='mixed_patch' if precision == 'f64' else 'mixed',
                                              g_psi1=torch.nn.functional.pad(g1, (0, mp_ - m_)).contiguous())
        s_k, s_p = wk.sum(dim=(1, 2)), (gp * p2).sum(dim=(1, 2))
        s_gbp = (gb * p2).sum(dim=(1, 2))
        stv = st[:, 0, 0]
        d_alpha = -0.5 * bat * n_ * stv + (s_k + 2.0 * s_p + bat * bat * vwphi) / aat
        d_beta = stv * (0.5 * n_ / bat + 0.5 * (tr - aat * n_)) - 0.5 * torch.sum(phit * yy[None, :], dim=1) \
            + bat * vwphi + s_gbp
        d_phit = per_t[:, None] - 0.5 * bat[:, None] * yy[None, :] + 0.5 * quad
        return dmu, ds, dz, dgam, d_alpha, d_beta, d_phit

    class _FHatT(torch.autograd.Function):
        """f_hat as a differentiable function of (x_mean, S, x_u, gamma / alpha / beta atoms, phi^T) for torch autograd (the
        cross-check path of the gradients, DPGP_T_AUTOGRAD=1, and the objective's graph): _fhat_forward / _fhat_backward."""

        @staticmethod
        def forward(ctx, x_mean_, s_, x_u_, gat, aat, bat, phit):
            f_hat, saved = _fhat_forward(x_mean_, s_, x_u_, gat, aat, bat, phit, for_backward=any(ctx.needs_input_grad))
            ctx.save_for_backward(*[a for a in saved if a is not None])
            ctx.with_inverses = saved[9] is not None
            return f_hat

        @staticmethod
        def backward(ctx, g_out):
            assert ctx.with_inverses
            return tuple(g_out * g for g in _fhat_backward(ctx.saved_tensors))

    def _dp_objective(phi, g1, g2, w1, w2):
        """-ELBO of the DP (dirichlet_process.py:64-88) as a function of its arguments (for autograd)."""
        t_ = truncation_level
        dg12 = torch.digamma(g1 + g2)
        tail = (torch.flip(torch.cumsum(torch.flip(phi, [-1]), dim=-1), [-1]) - phi)[:, 0:-1]
        ev_z = torch.sum(phi[:, 0:-1] * (torch.digamma(g1) - dg12) + tail * (torch.digamma(g2) - dg12))
        ev_v = (t_ - 1.0) * (torch.digamma(w1) - torch.log(w2)) + ((w1 / w2) - 1.0) * torch.sum(torch.digamma(g2) - dg12)
        ev_a = s_1 * np.log(s_2) - float(torch.lgamma(torch.tensor(s_1, dtype=TORCH_DTYPE))) + \
            (s_1 - 1.0) * (torch.digamma(w1) - torch.log(w2)) - s_2 * (w1 / w2)
        return -(ev_z + ev_v + ev_a + torch.sum(multinomial_dist_entropy(phi)) + torch.sum(beta_dist_entropy(g1, g2)) +
                 gamma_dist_entropy(w1, w2))

    def _objective_of(r):
        """(objective, f_hat, KL, DP objective, hyper-prior) from a dict of raw variables (torch graph when they require grad)."""
        gat, aat, bat = F.softplus(r['gamma_atoms']), F.softplus(r['alpha_atoms'])[:, 0], F.softplus(r['beta_atoms'])[:, 0]
        s = F.softplus(r['x_var'])
        phi = torch.softmax(r['dp_logits'], dim=-1)
        if mask_size != 1:
            phi = torch.repeat_interleave(phi, mask_size, dim=0)
        phit = phi[d_lo:d_hi].transpose(0, 1).contiguous()                                        # local dims
        mu = r['x_mean']
        if masked is not None:                                                                    # (values only: no torch graph)
            f_hat = masked.evaluate(r['x_u'], mu, s, gat, aat, bat, phit)
            last_info[0] = masked.info
        else:
            f_hat = _FHatT.apply(mu, s, r['x_u'], gat, aat, bat, phit)
        kl = 0.5 * (torch.sum(mu * mu) + torch.sum(s - torch.log(s)) - mu.shape[0] * mu.shape[1])     # gp_expressions.py:10-24
        hyper = torch.sum(log_normal_log_pdf(gat)) + torch.sum(log_normal_log_pdf(aat)) + torch.sum(log_normal_log_pdf(bat))
        w = F.softplus(r['dp_w'])
        dp_obj = _dp_objective(phi, F.softplus(r['dp_gamma_1']), F.softplus(r['dp_gamma_2']), w[0], w[1])
        return torch.stack([dp_obj - (f_hat - kl) - hyper, f_hat, kl, dp_obj, hyper])

    raw_vars = dict(x_mean=x_mean, x_var=x_var_raw, x_u=x_u, gamma_atoms=gamma_atoms_raw, alpha_atoms=sig_var_atoms_raw,
                    beta_atoms=beta_atoms_raw, **{'dp_' + k: v for k, v in dp_model.raw.items()})

    def _exchange(out):
        """Sharded: out[1] is the f_hat of the local output dims; everything else is replicated."""
        if sharded:
            f_tot = out[1].clone()
            dist.all_reduce(f_tot, op=dist.ReduceOp.SUM, group=process_group)
            out = torch.stack([out[3] - (f_tot - out[2]) - out[4], f_tot, out[2], out[3], out[4]])
        return out

    tbuf = {}
    if fused_t is not None:
        t_, q_ = truncation_level, num_latent_dims
        tbuf = dict(s=torch.empty((n_, q_), dtype=TORCH_DTYPE, device=device),
                    phi=torch.empty((d_, t_), dtype=TORCH_DTYPE, device=device),
                    atoms=torch.empty(t_ * q_ + 2 * t_, dtype=TORCH_DTYPE, device=device),
                    scal=torch.zeros(_lib.lib().dpgp_model_scal_count(d_), dtype=TORCH_DTYPE, device=device),
                    red=torch.zeros(2, dtype=TORCH_DTYPE, device=device), out=torch.zeros(5, dtype=TORCH_DTYPE, device=device))

    def _evaluate_fused(finish=True):
        """dpgp_model_prepare_t -> dpgp_elbo_fhat_t (the model-level tail rides in its last launch) -> [one packed all-reduce
        and dpgp_model_finalize when D is sharded]: eleven launches, no host arithmetic (round 2: ~200 launches of library
        operators and torch element-wise kernels)."""
        lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
        r = dp_model.raw
        t_, q_ = truncation_level, num_latent_dims
        _lib.check(lib.dpgp_model_prepare_t(
            d_, t_, q_, n_, d_lo, mask_size, r['logits'].data_ptr(), gamma_atoms_raw.data_ptr(), sig_var_atoms_raw.data_ptr(),
            beta_atoms_raw.data_ptr(), x_var_raw.data_ptr(), r['gamma_1'].data_ptr(), r['gamma_2'].data_ptr(), r['w'].data_ptr(),
            s_1, s_2, 1 if rank == 0 else 0, tbuf['s'].data_ptr(), tbuf['phi'].data_ptr(), tbuf['atoms'].data_ptr(),
            tbuf['scal'].data_ptr(), st), 'dpgp_model_prepare_t')
        at = tbuf['atoms']
        _, _, sums_t, info_t = ops.elbo_fhat_t(
            y_dev, yy, x_u, x_mean, tbuf['s'], at[:t_ * q_].view(t_, q_), at[t_ * q_:t_ * q_ + t_], at[t_ * q_ + t_:],
            tbuf['phi'].t(), jitter=GP_DEFAULT_JITTER, prec=precision, workspace=fused_t,
            model_tail=(tbuf['scal'], tbuf['red'], None if sharded else tbuf['out']))
        last_info[0] = info_t                 # (per atom; cholesky_info reduces it when asked: no launch per evaluation)
        return _finish_fused() if finish else tbuf['out']

    def _finish_fused():
        if sharded:
            lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
            dist.all_reduce(tbuf['red'], op=dist.ReduceOp.SUM, group=process_group)     # (f_hat, DP objective): 2 fp64 scalars
            _lib.check(lib.dpgp_model_finalize(tbuf['red'].data_ptr(), fused_t.sums[1:2].data_ptr(),
                                               tbuf['scal'][1:2].data_ptr(), tbuf['out'].data_ptr(), st), 'dpgp_model_finalize')
        return tbuf['out']

    def evaluate():
        with torch.no_grad():
            out = _evaluate_fused() if fused_t is not None else _exchange(_objective_of(raw_vars))
        return out, last_info[0]

    graph = {}

    def _objective_terms_graph():
        """The same evaluation replayed from a HIP graph (torch.cuda.CUDAGraph = hipGraph on ROCm): this composed objective
        is ~200 small launches, i.e. launch-bound; capturing them once removes the per-launch host cost.  The raw variables
        are read in place, so updates by an optimiser are seen by the replay.  With observed= the evaluation is launched eagerly,
        as in gradients() and optimise(): the masked bound is not captured."""
        if masked is not None:
            return evaluate()[0].clone()
        if 'g' not in graph:
            cur = torch.cuda.current_stream()
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                for _ in range(2):
                    evaluate()
            cur.wait_stream(side)
            g_ = torch.cuda.CUDAGraph()
            with _graph_capture(g_):
                with torch.no_grad():
                    graph['out'] = _evaluate_fused(finish=False) if fused_t is not None else _objective_of(raw_vars)
            graph['g'] = g_
        graph['g'].replay()
        if fused_t is not None:
            return _finish_fused().clone()
        return _exchange(graph['out'].clone())              # (the all-reduce of a sharded model runs eagerly behind the replay)

    def _local_flat_autograd():
        """This rank's packed gradient (all raw variables, then the trouble flag) — everything in front of the exchange — by torch
        autograd over the whole objective (~540 launches: the DP / KL / prior terms and their derivatives are ~400 of them)."""
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in raw_vars.items()}
        terms = _objective_of(leaves)
        # sharded: this rank's share of the objective = -(local f_hat) + (replicated terms) / world; the shares sum to it
        obj = terms[0] if not sharded else -terms[1] + (terms[3] + terms[2] - terms[4]) / world
        grads = torch.autograd.grad(obj, list(leaves.values()), allow_unused=True)
        grads = [torch.zeros_like(v) if g is None else g for v, g in zip(leaves.values(), grads)]
        flat = torch.cat([g.reshape(-1) for g in grads] + [torch.zeros(1, dtype=TORCH_DTYPE, device=device)])
        # trouble flag (failed factorisation / non-finite local gradient), reduced with the gradients: a collective decision
        flat[-1] = ((last_info[0] != 0) | ~torch.isfinite(flat[:-1]).all()).to(TORCH_DTYPE)
        return flat

    hbuf = {}

    def _local_flat():
        """The same with the model-level ends in the HIP library: dpgp_model_prepare_t (softplus / softmax transforms, phi), f_hat and
        its derivatives with respect to (x_mean, S, x_u, atoms, phi) from the library's operators (_fhat_forward / _fhat_backward),
        dpgp_model_backward_t (chain rule to the raw variables, KL, DP objective, hyper-prior): ~200 launches instead of ~540.
        Sharded: the replicated terms are added on rank 0 only (add_constants); the ranks' packed gradients sum to the gradient."""
        if os.environ.get('DPGP_T_AUTOGRAD', '0') == '1' and masked is None:
            return _local_flat_autograd()
        lib, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
        r = dp_model.raw
        t_, q_ = truncation_level, num_latent_dims
        if not hbuf:
            f64 = dict(dtype=TORCH_DTYPE, device=device)
            hbuf.update(s=torch.empty((n_, q_), **f64), phi=torch.empty((d_, t_), **f64), atoms=torch.empty(t_ * q_ + 2 * t_, **f64),
                        scal=torch.zeros(_lib.lib().dpgp_model_scal_count(d_), **f64))
        with torch.no_grad():
            _lib.check(lib.dpgp_model_prepare_t(
                d_, t_, q_, n_, d_lo, mask_size, r['logits'].data_ptr(), gamma_atoms_raw.data_ptr(), sig_var_atoms_raw.data_ptr(),
                beta_atoms_raw.data_ptr(), x_var_raw.data_ptr(), r['gamma_1'].data_ptr(), r['gamma_2'].data_ptr(), r['w'].data_ptr(),
                s_1, s_2, 1 if rank == 0 else 0, hbuf['s'].data_ptr(), hbuf['phi'].data_ptr(), hbuf['atoms'].data_ptr(),
                hbuf['scal'].data_ptr(), st), 'dpgp_model_prepare_t')
            at = hbuf['atoms']
            gat, aat, bat = at[:t_ * q_].view(t_, q_), at[t_ * q_:t_ * q_ + t_], at[t_ * q_ + t_:]
            if masked is not None:
                _, g = masked.evaluate(x_u, x_mean, hbuf['s'], gat, aat, bat, hbuf['phi'].t().contiguous(), grad=True)
                last_info[0] = masked.info
                dmu, ds, dz, dgam, d_alpha, d_beta, d_phit = (g[k] for k in ('mu', 's', 'z', 'gamma', 'alpha', 'beta', 'phit'))
            else:
                _, saved = _fhat_forward(x_mean, hbuf['s'], x_u, gat, aat, bat, hbuf['phi'].t().contiguous())
                dmu, ds, dz, dgam, d_alpha, d_beta, d_phit = _fhat_backward(saved)
            dab = torch.stack([d_alpha, d_beta], dim=1).contiguous()
            dphi = d_phit.t().contiguous()
            sizes = {k: v.numel() for k, v in raw_vars.items()}
            flat = torch.zeros(sum(sizes.values()) + 1, dtype=TORCH_DTYPE, device=device)
            parts, o = {}, 0
            for k, nel in sizes.items():
                parts[k] = flat[o:o + nel]
                o += nel
            rows = r['logits'].shape[0]
            _lib.check(lib.dpgp_model_backward_t(
                d_, t_, q_, n_, m_, d_lo, mask_size, rows, r['logits'].data_ptr(), gamma_atoms_raw.data_ptr(),
                sig_var_atoms_raw.data_ptr(), beta_atoms_raw.data_ptr(), x_var_raw.data_ptr(), r['gamma_1'].data_ptr(),
                r['gamma_2'].data_ptr(), r['w'].data_ptr(), x_mean.data_ptr(), hbuf['phi'].data_ptr(), s_1, s_2, 1 if rank == 0 else 0,
                dmu.contiguous().data_ptr(), ds.contiguous().data_ptr(), dz.contiguous().data_ptr(), dgam.contiguous().data_ptr(),
                dab.data_ptr(), dphi.data_ptr(), parts['x_mean'].data_ptr(), parts['x_var'].data_ptr(), parts['x_u'].data_ptr(),
                parts['dp_logits'].data_ptr(), parts['dp_gamma_1'].data_ptr(), parts['dp_gamma_2'].data_ptr(), parts['dp_w'].data_ptr(),
                parts['gamma_atoms'].data_ptr(), parts['alpha_atoms'].data_ptr(), parts['beta_atoms'].data_ptr(), st),
                'dpgp_model_backward_t')
            flat[-1] = ((last_info[0] != 0) | ~torch.isfinite(flat[:-1]).all()).to(TORCH_DTYPE)
        return flat

    grad_graph = {}

    def _gradients(graph=None):
        """d objective / d raw variable for all raw variables: torch autograd around the library-backed f_hat (above).
        graph=True (the default of optimise(); DPGP_GRAPH_T=0 turns it off): the local part — ~250 launches of library operators,
        element-wise kernels and their autograd, host-bound at ~4.6 ms per call whatever the problem size — is captured ONCE into a
        HIP graph (torch.cuda.CUDAGraph) and replayed; the raw variables are read in place, so optimiser updates are seen."""
        use_graph = bool(graph) and os.environ.get('DPGP_GRAPH_T', '1') != '0' and masked is None   # (observed=: launched eagerly)
        if use_graph:
            if 'g' not in grad_graph:
                cur = torch.cuda.current_stream()
                side = torch.cuda.Stream()
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    for _ in range(2):
                        _local_flat()
                cur.wait_stream(side)
                g_ = torch.cuda.CUDAGraph()
                with _graph_capture(g_):
                    grad_graph['flat'] = _local_flat()
                grad_graph['g'] = g_
            grad_graph['g'].replay()
            flat = grad_graph['flat'].clone()
        else:
            flat = _local_flat()
        if sharded:
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=process_group)       # ONE packed exchange
        grad_flag[0] = flat[-1]
        out, o = {}, 0
        for (k, v) in raw_vars.items():
            out[k] = flat[o:o + v.numel()].reshape(v.shape)
            o += v.numel()
        return out

    grad_flag = [torch.zeros((), dtype=TORCH_DTYPE, device=device)]

    def _optimise(num_iterations, learning_rate=0.01, callback=None):
        """Adam on the raw variables (the reference: tf.train.AdamOptimizer(...).minimize(objective))."""
        opt = torch.optim.Adam(list(raw_vars.values()), lr=learning_rate)
        for it in range(num_iterations):
            g = _gradients(graph=True)
            # potrf replaces a failing pivot by 1 and goes on: a failed factorisation would give finite, meaningless
            # gradients.  The reference's tf.cholesky raises; so does this.
            bad = (grad_flag[0] != 0) | ~torch.stack([torch.isfinite(v).all() for v in g.values()]).all()
            if bool(bad):
                raise FloatingPointError('iteration %d: failed Cholesky factorisation or non-finite gradient (precision=%r); '
                                         'use precision="f64"' % (it, precision))
            for k, p_ in raw_vars.items():
                p_.grad = g[k].reshape(p_.shape)
            opt.step()
            if callback is not None:
                callback(it)

    def _impute_training_data(return_variance=False):
        """A model trained with observed=: y_train [N x D] with every unobserved entry (n, d) replaced by the mixture's posterior mean
        sum_t phi_td beta_t Psi1_t[n,:] (K_t + beta_t Psi2_{t,p(d)})^-1 Psi1_t^T y_d (Psi2 and y_d over the rows at which d was
        observed); observed entries as given; a column never observed gets 0.  return_variance=True: (filled, var), var [N x D]
        the per-entry variance of predictive_marginals at the training q(X) at the unobserved entries and 0 at the observed ones;
        filled is the same tensor either way."""
        assert masked is not None, 'impute_training_data needs a model trained with observed='
        if return_variance:
            filled = _impute_training_data()
            with torch.no_grad():
                _, var = _moments().at(x_mean.detach(), F.softplus(x_var_raw).detach(), _columns_arg(None))
                return filled, torch.where(torch.as_tensor(train_obs, device=device), torch.zeros_like(var), var)
        with torch.no_grad():
            gat, aat, bat = F.softplus(gamma_atoms_raw), F.softplus(sig_var_atoms_raw)[:, 0], F.softplus(beta_atoms_raw)[:, 0]
            phi = torch.softmax(dp_model.raw['logits'], dim=-1)
            if mask_size != 1:
                phi = torch.repeat_interleave(phi, mask_size, dim=0)
            means = masked.posterior_means(x_u, x_mean, F.softplus(x_var_raw), gat, aat, bat, phi.transpose(0, 1).contiguous())
            return torch.where(torch.as_tensor(train_obs, device=device), y_dev, means)

    # ---- prediction (models/frozen_bound_t.py): fp64, one GPU; the reference's own over-T predict_* raise NameError, so there is
    # nothing to mirror: the bound is the model's own masked bound on the test rows with everything trained held fixed
    pred_state = {}

    def _frozen():
        """The trained values the prediction paths hold fixed: (gamma [T,Q], alpha [T], beta [T], phi^T [T,D], S [N,Q])."""
        assert precision == 'f64' and not sharded, 'prediction paths of dp_gp_lvm_t run in fp64 on one GPU'
        with torch.no_grad():
            phi = torch.softmax(dp_model.raw['logits'], dim=-1)
            if mask_size != 1:
                phi = torch.repeat_interleave(phi, mask_size, dim=0)
            return (F.softplus(gamma_atoms_raw), F.softplus(sig_var_atoms_raw)[:, 0].contiguous(),
                    F.softplus(beta_atoms_raw)[:, 0].contiguous(), phi.transpose(0, 1).contiguous(), F.softplus(x_var_raw))

    def _test_arguments(y_test, observed, predict=False):
        """(y_test zero-filled [N* x D], mask): `observed` given -> the checks of utils.missing.masked_arguments; None -> y_test
        holds the first Do <= D output dims of every test point."""
        assert precision == 'f64' and not sharded, 'prediction paths of dp_gp_lvm_t run in fp64 on one GPU'
        if observed is not None:
            return _missing.masked_arguments(y_test, observed, num_dimensions, predict)
        y_test = np.asarray(y_test, dtype=np.float64)
        assert y_test.ndim == 2 and y_test.shape[0] >= 1 and 1 <= y_test.shape[1] <= num_dimensions, \
            'y_test must be [N* x Do] with 1 <= Do <= D'
        if predict:
            assert y_test.shape[1] < num_dimensions, \
                'Observed dimensionality for missing data scenario must be less than total dimensionality of training data.'
        obs = np.zeros((y_test.shape[0], num_dimensions), dtype=bool)
        obs[:, :y_test.shape[1]] = True
        y0 = np.zeros(obs.shape)
        y0[:, :y_test.shape[1]] = y_test
        return y0, obs

    def _test_bound(y0, obs):
        gat, aat, bat, phit, _ = _frozen()
        return _TestBoundT(x_u.detach(), gat, aat, bat, phit, y0, obs, device)

    def _start(y0, obs, use_pca, x_test_mean, x_test_var):
        """q(X*) at the start: the given values, or the PCA of the zero-filled test rows, or the training latent mean of the
        nearest training row over the jointly observed columns plus N(0, 0.01^2) noise; variances 1 unless given."""
        return _latents.start(
            y0.shape[0], num_latent_dims, device, x_test_mean, x_test_var, use_pca, y0,
            lambda: _latents.masked_neighbour(np.asarray(y_train), train_obs, y0, obs, x_mean.detach().cpu().numpy()))

    def _moments():
        """The training side of the predictive moments (frozen_bound_t._MomentsT), formed once per call."""
        gat, aat, bat, phit, s = _frozen()
        train = masked if masked is not None else \
            _MaskedBoundT(np.asarray(y_train, dtype=np.float64), np.ones((num_samples, num_dimensions), dtype=bool),
                          truncation_level, device)
        with torch.no_grad():
            return _MomentsT(train, x_u.detach(), x_mean.detach(), s, gat, aat, bat, phit)

    def _columns_arg(columns):
        return _marginals.columns_arg(columns, num_dimensions, device)

    def _metric_under(columns, name):
        """latent_geometry's hook: the marginals.Metric under latent_metric(., columns), the training side and the atoms'
        (P, prior), phi as weights, formed once."""
        cols = _columns_arg(columns)
        with torch.no_grad():
            return _marginals.Metric([_moments().metric_part(cols)])

    class DP_GP_LVM_T(LatentGeometry, Trainable):
        """Accessors as in the reference (dp_gp_lvm.py:679-740); the kernel has batch size T here.  The latent-geometry methods
        are models/latent_geometry.LatentGeometry's: an operator call runs on the T atoms, the weights phi included; with the
        columns of one discovered group they show that group's own energy, the paths it considers short and where its manifold
        takes a motion."""
        _latent_dims, _device, _metric_of = num_latent_dims, device, staticmethod(_metric_under)
        raw = dict(x_mean=x_mean, x_var=x_var_raw, x_u=x_u, gamma_atoms=gamma_atoms_raw, alpha_atoms=sig_var_atoms_raw,
                   beta_atoms=beta_atoms_raw, **{'dp_' + k: v for k, v in dp_model.raw.items()})

        @property
        def assignments(self):
            return dp_model.assignments

        @property
        def dp(self):
            return dp_model

        @property
        def dp_atoms(self):
            return F.softplus(gamma_atoms_raw), F.softplus(sig_var_atoms_raw), F.softplus(beta_atoms_raw)

        @property
        def kernel(self):
            return k_ard_rbf(gamma=F.softplus(gamma_atoms_raw), alpha=F.softplus(sig_var_atoms_raw),
                             beta=F.softplus(beta_atoms_raw))

        @property
        def inducing_input(self):
            return x_u

        @property
        def q_x(self):
            return x_mean, torch.diag_embed(F.softplus(x_var_raw))

        @property
        def objective(self):
            return evaluate()[0][0].clone()

        @property
        def objective_terms(self):
            # (a copy: the fused path evaluates into one persistent buffer, which the next evaluation overwrites)
            return evaluate()[0].clone()

        @property
        def cholesky_info(self):
            info = evaluate()[1]
            return info.abs().max() if info.dim() else info

        shard = (d_lo, d_hi)

        objective_terms_graph = staticmethod(_objective_terms_graph)
        gradients = staticmethod(_gradients)
        optimise = staticmethod(_optimise)
        impute_training_data = staticmethod(_impute_training_data)

        @property
        def prediction_terms(self):
            """F_t(d) [T P x Dmax] of the test bound in the last prediction call (slot t P + p, the places of pattern p's columns;
            the layout of masked_bound_t._MaskedBoundT), or None."""
            return pred_state.get('terms')

        @property
        def missing_columns(self):
            """The output dims whose moments the last predict_missing_data returned (ascending), or None."""
            return pred_state.get('missing_columns')

        @staticmethod
        def predict_new_latent_variables(y_test, use_pca=False, x_test_mean=None, x_test_var=None):
            """q(X*) for fully observed test data y_test [N* x D] and the prediction lower bound
                f_hat + f_hat* - KL(q(X)) - KL(q(X*)),    test log-likelihood = f_hat* - KL(q(X*)),
            f_hat* the model's own bound on (y_test, q(X*)) with everything trained held fixed (models/frozen_bound_t.py).  Returns
            (prediction_lower_bound, x_test_mean [N* x Q], x_test_covar [N* x Q x Q], test_log_likelihood) at the initial q(X*):
            nearest training neighbour + N(0, 0.01^2) noise, or PCA of y_test (`use_pca`), or the given values; variances 1.
            fp64 and one GPU (AssertionError for a 'mixed' or sharded model)."""
            y0, obs = _test_arguments(y_test, None)
            assert np.shape(y_test)[1] == num_dimensions, \
                'Observed dimensionality for prediction must be equal to the dimensionality of the training data.'
            xt, st_ = _start(y0, obs, use_pca, x_test_mean, x_test_var)
            out = evaluate()[0].clone()                                           # (objective, f_hat, KL, DP, hyper)
            bound = _test_bound(y0, obs)
            f_hat_test, kl_test = _latents.bound_at(bound, xt, st_)
            pred_state['terms'] = bound.terms
            test_ll = f_hat_test - kl_test
            return out[1] - out[2] + test_ll, xt, torch.diag_embed(st_), test_ll

        @staticmethod
        def test_latent_gradients(y_test, x_test_mean, x_test_var, observed=None):
            """d (f_hat* - KL(q(X*))) / d (x_test_mean, x_test_var) with the trained model fixed.  y_test [N* x Do] (the first
            Do <= D output dims), or [N* x D] with a boolean mask `observed` of any pattern (entries where it is False are ignored
            and may be NaN; True everywhere is allowed here)."""
            y0, obs = _test_arguments(y_test, observed)
            bound = _test_bound(y0, obs)
            with torch.no_grad():
                grads = _latents.ascent_gradient(bound, _latents.latent_values(x_test_mean, device, num_latent_dims, y0.shape[0]),
                                                 _latents.latent_values(x_test_var, device, num_latent_dims, y0.shape[0]))
                pred_state['terms'] = bound.terms
            return grads

        @staticmethod
        def optimise_test_latents(y_test, num_iterations=200, learning_rate=0.01, use_pca=False, x_test_mean=None,
                                  x_test_var=None, observed=None):
            """Adam on q(X*) (mean and softplus-parametrised variances) maximising f_hat* - KL(q(X*)); returns (x_test_mean,
            x_test_var) to hand to predict_*.  The frozen bound is formed once and nothing is read back on the host inside the
            loop.  observed: as test_latent_gradients; the start is then the masked nearest neighbour."""
            y0, obs = _test_arguments(y_test, observed)
            xt, st_ = _start(y0, obs, use_pca, x_test_mean, x_test_var)
            bound = _test_bound(y0, obs)
            with torch.no_grad():
                fitted = _latents.fit(functools.partial(_latents.ascent_gradient, bound), xt, st_, num_iterations, learning_rate)
                pred_state['terms'] = bound.terms
                return fitted

        @staticmethod
        def predictive_marginals(x_test_mean, x_test_var, columns=None):
            """(mean, var), each [N* x len(columns)]: the per-entry moments of the mixture sum_t phi_td N(mean_t, var_t) of the
            output dims `columns` (default: all D) at q(X*) = (x_test_mean, x_test_var [N* x Q]); formulas in
            models/frozen_bound_t._MomentsT, the Psi2 parts by ops.qx_psi_pointwise.  A column never observed in training has mean
            0 and variance sum_t phi_td (alpha_t + 1 / beta_t)."""
            cols = _columns_arg(columns)
            with torch.no_grad():
                return _moments().at(_latents.latent_values(x_test_mean, device, num_latent_dims),
                                     _latents.latent_values(x_test_var, device, num_latent_dims), cols)

        @staticmethod
        def frozen_predictor(columns=None):
            """A models/predictor.FrozenPredictor of the output dims `columns` (default: all D): p(x_mean, x_var) gives the bits of
            predictive_marginals, differentiably in q(X*); p.vjp is its vector-Jacobian product (the mixture's on the host, then
            ops.qx_psi_point_moments_adjoint on the T atoms).  The training side is built once, here, at the model's current
            parameters: stale after further training.  Not built for a sharded model: AssertionError."""
            cols = _columns_arg(columns)
            return _predictor.of_mixture(_moments(), cols, device)

        @staticmethod
        def predictive_jacobian(x, columns=None):
            """[N* x len(columns) x Q]: the mean of the Jacobian d f_d / d x of the noise-free map of the output dims `columns`
            (default: all D) at the DETERMINISTIC latent points x [N* x Q] (numpy or torch), sum_t phi_td b_t(x)^T r_td: the
            derivative of predictive_marginals' mean at x_test_var = 0 (ops.ard_rbf_point_jacobian on the T atoms).  The training
            side is built once per call.  fp64, torch.no_grad."""
            cols = _columns_arg(columns)
            with torch.no_grad():
                return _moments().jacobian(_marginals.points_arg(x, num_latent_dims, device), cols)

        @staticmethod
        def latent_metric(x, columns=None):
            """[N* x Q x Q]: the expected Riemannian metric of the map from latent space to the output dims `columns` (default:
            all D) at the latent points x [N* x Q] (Tosi et al., UAI 2014), the mixture's second moment over the atoms
            (frozen_bound_t._MomentsT.metric; one call of ops.ard_rbf_point_metric on the T atoms).  With the columns of one
            discovered group it shows which region and which latent directions that group uses.  A column never observed in
            training contributes sum_t phi_td alpha_t diag(gamma_t).  fp64."""
            cols = _columns_arg(columns)
            with torch.no_grad():
                return _moments().metric(_marginals.points_arg(x, num_latent_dims, device), cols)

        @staticmethod
        def predictive_covariance(x, columns=None, noise=False):
            """[len(columns) x N* x N*]: the covariance of the output dims `columns` (default: all D) at the DETERMINISTIC latent
            points x [N* x Q] (numpy or torch) under the mixture over the atoms,
                sum_t phi_td (cov_t,p(d) + m_td m_td^T) - m_d m_d^T
            with cov_t,p the joint posterior covariance of the noise-free function under atom t and training row pattern p
            (frozen_bound_t._MomentsT.covariance; one call of ops.ard_rbf_point_cov on the T atoms).  noise=True adds 1/beta_t to
            every atom's diagonal; the diagonal is then predictive_marginals(x, 0)'s variance.  A column never observed in
            training gets the mixture of the atoms' prior grams.  The array is J N*^2 doubles (and T times that while it is
            formed); under one atom the columns of one pattern repeat the same matrix.  Works on a model trained on complete data
            and on one trained with observed=.  fp64, torch.no_grad."""
            cols = _columns_arg(columns)
            with torch.no_grad():
                return _moments().covariance(_marginals.points_arg(x, num_latent_dims, device), cols, noise)

        @staticmethod
        def sample_functions(x, num_samples=1, columns=None, noise=False, jitter=_marginals.DEFAULT_SAMPLE_JITTER, seed=0,
                             draws=None, atoms=None):
            """[S x N* x len(columns)]: S joint draws of the output dims `columns` (default: all D) at the latent points x
            [N* x Q].  Every (sample, column) first draws its atom t from phi_:d (a device torch.Generator seeded with `seed`), or
            takes it from `atoms` [S x len(columns)] (long), then draws from that atom's posterior: m_td + L xi with
            L L^T = cov_t,p(d) + jitter alpha_t I (+ 1/beta_t I with noise), xi standard normal from the same generator, or
            given as `draws` [S x N* x len(columns)].  One ops.potrf_batched call over the (atom, pattern) pairs and one
            ops.matmul, whatever the number of columns; one host read, potrf's info at the end: FloatingPointError if a
            factorisation failed (raise `jitter` or set noise=True).  The default jitter, 1e-6 alpha_t, is a choice, not a
            measurement: the gram of nearby points has its smallest eigenvalue below rounding and the factorisation needs a
            shift well above eps N* lambda_max ~ 1e-12 alpha; 1e-6 alpha is far above that and far below any 1/beta the models
            train to.  fp64, torch.no_grad."""
            cols = _columns_arg(columns)
            with torch.no_grad():
                xp = _marginals.points_arg(x, num_latent_dims, device)
                gen = _marginals.draw_generator(seed, device)
                if atoms is not None:
                    at = np.asarray(atoms.detach().cpu() if torch.is_tensor(atoms) else atoms, dtype=np.int64)
                    assert at.ndim == 2 and at.shape[1] == cols.numel() and at.min() >= 0 and at.max() < truncation_level, \
                        'atoms must be [S x len(columns)] atom indices in [0, T)'
                    atoms = torch.as_tensor(at, device=device)
                mom = _moments()
                if atoms is None:                                         # (the atoms first, then the normal draws: one stream)
                    count = int(num_samples) if draws is None else len(draws)
                    assert count >= 1, 'num_samples must be at least 1'
                    phi = mom.phit.index_select(1, cols)
                    atoms = torch.multinomial(phi.transpose(0, 1).contiguous(), count, replacement=True,
                                              generator=gen).transpose(0, 1)
                xi = _marginals.standard_draws(draws, atoms.shape[0], xp.shape[0], cols.numel(), gen, device)
                assert atoms.shape[0] == xi.shape[0], 'atoms and draws must hold the same number of samples'
                f, info = mom.sample(xp, xi, cols, atoms, noise, jitter)
                _marginals.raise_if_not_factorised(info)
                return f

        @staticmethod
        def predict_missing_data(y_test, use_pca=False, x_test_mean=None, x_test_var=None, observed=None):
            """y_test [N* x Do] holds the first Do < D output dims of the test points, or, with `observed` (a boolean [N* x D]
            mask of any pattern, not True everywhere; unobserved entries are ignored and may be NaN), y_test is [N* x D].
            Returns (lower_bound, x_test_mean, x_test_covar [N* x Q x Q], predicted_mean [N* x Du], predicted_var [N* x Du]) at
            the initial q(X*) (see predict_new_latent_variables; with a mask the masked nearest neighbour) for the Du dims
            Do .. D-1, or, with `observed`, the columns with at least one unobserved test entry, ascending (missing_columns).
            lower_bound = f_hat + f_hat* - KL(q(X)) - KL(q(X*)).

            predicted_var is the PER-ENTRY marginal variance of the mixture over the atoms (observation noise 1 / beta_t
            included), not the [Du x N* x N*] array the other models return in the reference's shape.  That array is built from
            Psi2* summed over all test points: one scalar per output dim plus a diagonal, the same for every test point, so it
            cannot say how sure the model is about one filled-in value.  The per-entry variance needs each test point's own
            Psi2*, contracted on the fly by ops.qx_psi_pointwise; the reference has no working over-T prediction to mirror."""
            y0, obs = _test_arguments(y_test, observed, predict=True)
            xt, st_ = _start(y0, obs, use_pca, x_test_mean, x_test_var)
            out = evaluate()[0].clone()
            bound = _test_bound(y0, obs)
            pred_state['missing_columns'] = _missing.missing_columns(obs)
            f_hat_test, kl_test = _latents.bound_at(bound, xt, st_)
            pred_state['terms'] = bound.terms
            with torch.no_grad():
                lower_bound = out[1] + f_hat_test - out[2] - kl_test
                mean, var = _moments().at(xt, st_, _columns_arg(pred_state['missing_columns']))
            return lower_bound, xt, torch.diag_embed(st_), mean, var

    return DP_GP_LVM_T()
