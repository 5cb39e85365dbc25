"""Child process of tests/test_gpu_sharded_masked.py: one rank of a D-sharded dp_gp_lvm on the visible GPU, trained with
observed= or on complete data.
    python tests/_sharded_masked_worker.py <case> <out.npz>
RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT come from the environment; the transport is gloo (see tests/_sharded_worker.py).
`collect` is also what the parent test runs on the single-process model: the same calls in the same order on both sides.

A case is  <fixture>:<mask kind or 'complete'>:<shard_by>:<sections, '+'-separated>  with the sections
    train    objective, objective terms, shard, all gradients, per-dimension flags, then (last) a 5-step Adam run
    impute   impute_training_data(return_variance=True) (mask-trained only) and predictive_marginals, all columns and a permuted subset
    test     the shared-inducing test bound: gradients, a 5-step q(X*) fit from a start that is not supplied, predict_missing_data,
             predict_new_latent_variables(observed=)
    flag     the columns of rank 1 of 2 on an atom with ARD weights x 1e-5; optimise(3) must raise on every rank
    args     the argument checks of a sharded model
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

SEED = 4321
# The 'flag' case.  ARD weights x 1e-5 alone flag nothing on the fp64 masked path (measured on two ranks: no rank raised, no info
# entry set): the 1e-8 jitter keeps K_uu factorisable in fp64 and A = I + beta T stays positive definite; the mixed-precision model
# of tests/_sharded_worker.py is flagged there by its conditioning guard, which the fp64 path does not have.  So the atom of rank
# 1's columns also gets this signal variance: its square overflows in Psi2, A is not finite and its factorisation fails (info > 0).
FLAG_ALPHA = 1e200


def mask_of(kind, n, d):
    """rand30 / edge: tests/test_gpu_train_masked_d.masks.  empty01: rand30 at another seed with columns 0 and 1 never observed
    (rank 0 of 3 at D = 6 owns no observed column)."""
    from test_gpu_train_masked_d import masks
    if kind == 'complete':
        return None
    if kind == 'empty01':
        obs = np.random.default_rng(2).random((n, d)) >= 0.3
        obs[:, :2] = False
        return obs
    return masks(n, d)[kind]


def points_for_test(g, empty_head=False):
    """N* = 6 points near training points; the test mask has column 2 unobserved everywhere and row 1 fully unobserved;
    empty_head: columns 0 and 1 unobserved as well (the first of three ranks at D = 6 then has no observed test entry)."""
    from test_gpu_train_masked_d import points_near_training
    y_t, o_t, xm, xv = points_near_training(g, 11)
    o_t[1, :] = False
    if empty_head:
        o_t[:, :2] = False
    return np.where(o_t, y_t, np.nan), o_t, xm, xv


def subset_of(d):
    return [7, 2, 5, 4, 0] if d == 10 else [4, 0, 3, 1]           # permuted, on both sides of every shard boundary


def flagged_fixture(g):
    """tests/_sharded_worker.py's 'flag' recipe: the first half of the output dims on atom 0, the second half on atom 1, whose ARD
    weights are scaled by 1e-5.  The logits are +-800, so that the other atoms' assignment probabilities are exactly 0 and nothing
    of atom 1 reaches the first half (see FLAG_ALPHA)."""
    bad = {k: np.array(v) for k, v in g.items()}
    d = bad['y'].shape[1]
    logits = np.full_like(bad['dp_logits'], -800.0)
    logits[: d // 2, 0] = 800.0
    logits[d // 2:, 1] = 800.0
    bad['dp_logits'] = logits
    sp = np.logaddexp(0.0, bad['gamma_atoms_raw'])
    sp[1] *= 1e-5
    bad['gamma_atoms_raw'] = np.log(np.expm1(sp))
    return bad


def build(g, dev, kind, shard_by='count', **kw):
    from test_gpu_train_masked_d import build_fixture
    n, d = g['y'].shape
    obs = mask_of(kind, n, d)
    if shard_by != 'count':
        kw['shard_by'] = shard_by
    if obs is None:
        return build_fixture(g, dev, None, precision='f64', backward_precision='f64', **kw)
    return build_fixture(g, dev, obs, y=np.where(obs, g['y'], np.nan), **kw)


def collect(model, g, kind, sections, noise_seed=SEED, empty_head=False, single=False, calls=None):
    """The numbers of the sections as a dict of arrays.  single: the one-GPU model the ranks are compared with.  calls: a list that
    grows by one entry per collective call of this process (the children count them: 'n_*' is the number of collectives of one
    call of the model)."""
    import torch
    res = {}
    num = lambda a: a.detach().cpu().numpy()
    d = g['y'].shape[1]
    complete = kind == 'complete'
    if 'train' in sections:
        before = len(calls or [])
        res['objective'] = float(model.objective)
        res['n_objective'] = len(calls or []) - before
        res['terms'] = num(model.objective_terms)
        res['shard'] = np.array(model.shard)
        res['pack'] = num(model.partial_pack())
        before = len(calls or [])
        grads = model.gradients()
        res['n_gradients'] = len(calls or []) - before
        for k, v in grads.items():
            res['grad_' + k] = num(v)
        terms, info = model.per_dimension_terms
        res['per_dim'], res['info'] = num(terms), num(info)
    if 'impute' in sections:
        _, _, xm, xv = points_for_test(g)
        if not complete:
            filled, var = model.impute_training_data(return_variance=True)
            res['filled'], res['filled_var'] = num(filled), num(var)
            res['filled_plain'] = num(model.impute_training_data())
        res['marg_mean'], res['marg_var'] = (num(a) for a in model.predictive_marginals(xm, xv))
        res['sub_mean'], res['sub_var'] = (num(a) for a in model.predictive_marginals(xm, xv, columns=subset_of(d)))
    if 'test' in sections:
        y_nan, o_t, xm, xv = points_for_test(g, empty_head)
        before = len(calls or [])
        res['tg_mu'], res['tg_s'] = (num(a) for a in model.test_latent_gradients(y_nan, xm, xv, observed=o_t, form='shared'))
        res['n_test_gradients'] = len(calls or []) - before
        np.random.seed(noise_seed)
        before = len(calls or [])
        fit_mu, fit_s = model.optimise_test_latents(y_nan, num_iterations=5, observed=o_t, form='shared')
        res['n_fit'] = len(calls or []) - before
        res['fit_mu'], res['fit_s'] = num(fit_mu), num(fit_s)
        bound, q_mu, q_cov, mean, var = model.predict_missing_data(y_nan, x_test_mean=fit_mu, x_test_var=fit_s, observed=o_t,
                                                                   form='shared', marginal_variance=True)
        res['pmd_bound'], res['pmd_mu'], res['pmd_cov'] = float(bound), num(q_mu), num(q_cov)
        res['pmd_cols'], res['pmd_mean'], res['pmd_var'] = np.asarray(model.missing_columns), num(mean), num(var)
        res['pmd_slots'] = int(model.prediction_terms.shape[0])
        if complete and single:
            # one GPU, complete data: the mean of this call is the [Du x N* x N*] path's; predictive_marginals is the per-entry pin
            res['pmd_mean'] = num(model.predictive_marginals(q_mu, fit_s, columns=model.missing_columns)[0])
        np.random.seed(noise_seed)
        if complete and single:
            # one GPU, complete data: predict_new_latent_variables takes no observed=; the same bound at the same seeded start
            lb, n_mu, n_cov, _, _ = model.predict_missing_data(y_nan, observed=o_t, form='shared', marginal_variance=True)
            terms = model.objective_terms
            ll = lb - (terms[1] - terms[2])
        else:
            lb, n_mu, n_cov, ll = model.predict_new_latent_variables(y_nan, observed=o_t)
        res['new_bound'], res['new_ll'], res['new_mu'], res['new_cov'] = float(lb), float(ll), num(n_mu), num(n_cov)
    if 'train' in sections:
        model.optimise(5, learning_rate=0.01)
        res['after'] = float(model.objective)
        res['x_u_after'] = num(model.raw['x_u'])
    return res


def main():
    case, out = sys.argv[1:3]
    fixture, kind, shard_by, sections = case.split(':')
    sections = sections.split('+')
    import pytest
    import torch
    import torch.distributed as dist
    from conftest import golden
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    dist.init_process_group('gloo', rank=rank, world_size=world)
    dev = torch.device('cuda:0')
    g = golden(fixture)
    pg = dist.group.WORLD
    res = dict(rank=rank)
    calls = []
    for name in ('all_reduce', 'broadcast'):                       # count this process's collectives (dist.barrier is ours)
        def counted(*a, _f=getattr(dist, name), _n=name, **kw):
            calls.append(_n)
            return _f(*a, **kw)
        setattr(dist, name, counted)
    if 'flag' in sections:
        model = build(flagged_fixture(g), dev, kind, process_group=pg)
        with torch.no_grad():
            model.raw['alpha_atoms'][1, 0] = FLAG_ALPHA                                # (softplus(x) = x out there)
        at = []
        try:
            model.optimise(3, callback=at.append)
            res['raised'] = 0
        except FloatingPointError:
            res['raised'] = 1
        res['iterations_done'] = len(at)
        res['shard'] = np.array(model.shard)
        res['local_flags'] = int((model.per_dimension_terms[1] != 0).sum())
    elif 'args' in sections:
        y_nan, o_t, xm, xv = points_for_test(g)
        refused = []
        for kind_ in (kind, 'complete'):
            model = build(g, dev, kind_, process_group=pg)
            calls = [lambda: model.test_latent_gradients(y_nan, xm, xv, observed=o_t, form='slots'),
                     lambda: model.test_latent_gradients(y_nan, xm, xv, observed=o_t),            # (the default form is 'slots')
                     lambda: model.optimise_test_latents(y_nan, num_iterations=1, observed=o_t, form='slots'),
                     lambda: model.test_latent_gradients(g['y'][:3, :4], xm[:3], xv[:3])]         # the reference's form
            if kind_ == 'complete':
                calls += [lambda: model.predict_missing_data(y_nan, observed=o_t, form='slots'),
                          lambda: model.predict_missing_data(g['y'][:3, :4]),
                          lambda: model.predict_new_latent_variables(g['y'][:3]),
                          lambda: model.optimise_test_latents(g['y'][:3, :4], num_iterations=1)]
            for call in calls:
                with pytest.raises(AssertionError, match="observed= with form='shared'"):
                    call()
                refused.append(1)
        with pytest.raises(AssertionError, match='needs observed='):
            build(g, dev, 'complete', process_group=pg, shard_by='observed')
        refused.append(1)
        res['refused'] = len(refused)
        res.update(collect(build(g, dev, kind, process_group=pg), g, kind, ['train'], calls=calls))           # (a 1-rank group: pack -> all-reduce -> finalize)
    else:
        model = build(g, dev, kind, shard_by, process_group=pg)
        res.update(collect(model, g, kind, sections, noise_seed=SEED if rank == 0 else 1000 + rank,
                           empty_head=world == 3, calls=calls))
    np.savez(out, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
