"""dp_gp_lvm trained with observed= (and, for the prediction paths, on complete data) D-sharded over two or three ranks: fresh
child processes on the one GPU of the test box, gloo transport (tests/_sharded_masked_worker.py), against the single-process
model, which tests/test_gpu_train_masked_d.py pins to the fp64 oracle.  Training (objective, terms, all gradients, a 5-step Adam
run), uneven and empty shares, the _shard_of arithmetic without a communicator, the collective trouble flag, imputation and
per-entry moments, the shared-inducing test bound, the argument checks and the split that follows the mask.

Tolerances (tests/test_gpu_sharded.py's: fp64, the same kernels on the same inputs, only the order of the sum over d differs):
1e-12 relative on objective, terms and bounds; gradients atol = 1e-9 max|want|; 1e-7 after the 5-step runs; moments 1e-12."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import golden
from _sharded_masked_worker import build, collect, mask_of, points_for_test

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
D6, D10 = 'grad_ref_40_6_12_3_T4', 'grad_ref_60_10_15_4_T5'
SINGLE = {}


def _run_ranks(tmp_path, case, world):
    assert world <= 3
    port = 31200 + os.getpid() % 1500
    procs, outs = [], []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY='0')
        out = str(tmp_path / ('rank%d.npz' % rank))
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, '_sharded_masked_worker.py'), case, out],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for pr in procs:
        try:
            log, _ = pr.communicate(timeout=300)
        except subprocess.TimeoutExpired:          # a rank left waiting in a collective: kill exactly our children
            for q in procs:
                q.kill()
            pytest.fail('a rank hung (collective mismatch between the ranks)')
        logs.append(log.decode(errors='replace'))
    for pr, log in zip(procs, logs):
        assert pr.returncode == 0, log[-3000:]
    return [dict(np.load(o)) for o in outs]


def single_of(dev, fixture, kind, sections, empty_head=False):
    """The single-process model's numbers for a case, computed once and shared."""
    key = (fixture, kind, tuple(sections), empty_head)
    if key not in SINGLE:
        g = golden(fixture)
        SINGLE[key] = collect(build(g, dev, kind), g, kind, sections, empty_head=empty_head, single=True)
    return SINGLE[key]


def rel(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    top = max(np.abs(want).max(), 1e-300)
    print('%s: max |err| %.3e of %.3e (bound %.0e of that)' % (what, np.abs(got - want).max(), top, tol))
    np.testing.assert_allclose(got, want, rtol=tol, atol=tol * top, err_msg=what)


def absolute(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    top = max(np.abs(want).max(), 1e-300)
    print('%s: max |err| %.3e of %.3e (bound %.0e of that)' % (what, np.abs(got - want).max(), top, tol))
    np.testing.assert_allclose(got, want, rtol=0, atol=tol * top, err_msg=what)


def moments(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    print('%s: max |err| %.3e of %.3e (bound 1e-12)' % (what, np.abs(got - want).max(), np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * max(1.0, np.abs(want).max()), err_msg=what)


def check_training(ranks, one, bounds):
    assert [tuple(r['shard']) for r in ranks] == bounds
    for r in ranks:
        tag = 'rank %d ' % int(r['rank'])
        # one evaluation: one all-reduce (the 2 scalars); one gradient evaluation: that one and the packed gradients + flag
        assert (int(r['n_objective']), int(r['n_gradients'])) == (1, 2)
        rel(r['objective'], one['objective'], 1e-12, tag + 'objective')
        rel(r['terms'], one['terms'], 1e-12, tag + 'terms')
        for k in one:
            if k.startswith('grad_'):
                absolute(r[k], one[k], 1e-9, tag + k)
        # per_dimension_terms is local: this rank's rows of the single-process array, zero rows for never-observed columns
        d_lo, d_hi = (int(v) for v in r['shard'])
        assert r['per_dim'].shape == (d_hi - d_lo, 5) and r['info'].shape == (d_hi - d_lo,) and not r['info'].any()
        rel(r['per_dim'], one['per_dim'][d_lo:d_hi], 1e-12, tag + 'per-dimension terms')
        assert np.array_equal(np.abs(r['per_dim']).sum(axis=1) == 0, np.abs(one['per_dim'][d_lo:d_hi]).sum(axis=1) == 0)
        rel(r['after'], one['after'], 1e-7, tag + 'objective after 5 Adam steps')
        absolute(r['x_u_after'], one['x_u_after'], 1e-7, tag + 'x_u after 5 Adam steps')
        # partial_pack() on a model with a process group: the reduced (f_hat, DP objective), as on the unmasked sharded model
        rel(r['pack'], one['pack'], 1e-12, tag + '(f_hat, DP objective) after the all-reduce')
    rel(sum(r['per_dim'].sum() for r in ranks), one['per_dim'].sum(), 1e-12, 'f_hat as the sum of the ranks\' per-dimension terms')
    for r in ranks[1:]:                                                                   # replicas stay bit-identical
        np.testing.assert_array_equal(r['x_u_after'], ranks[0]['x_u_after'])
        np.testing.assert_array_equal(r['terms'], ranks[0]['terms'])
        for k in one:
            if k.startswith('grad_'):
                np.testing.assert_array_equal(r[k], ranks[0][k], err_msg=k)


def check_imputation(ranks, one, complete=False):
    names = ['marg_mean', 'marg_var', 'sub_mean', 'sub_var'] + ([] if complete else ['filled', 'filled_var', 'filled_plain'])
    for r in ranks:
        for k in names:
            assert r[k].shape == one[k].shape, k
            moments(r[k], one[k], 'rank %d %s' % (int(r['rank']), k))
            np.testing.assert_array_equal(r[k], ranks[0][k], err_msg=k)              # every rank returns the same tensors
        if not complete:
            np.testing.assert_array_equal(r['filled'], r['filled_plain'])


def check_test_time(ranks, one, slots):
    for r in ranks:
        tag = 'rank %d ' % int(r['rank'])
        # collectives: the training-side evaluation (1) and ONE per evaluation of the test bound; the 5-step fit adds the broadcast
        assert (int(r['n_test_gradients']), int(r['n_fit'])) == (2, 1 + 1 + 5)
        absolute(r['tg_mu'], one['tg_mu'], 1e-9, tag + 'd bound / d mean')
        absolute(r['tg_s'], one['tg_s'], 1e-9, tag + 'd bound / d var')
        absolute(r['fit_mu'], one['fit_mu'], 1e-7, tag + 'q(X*) mean after 5 steps')
        absolute(r['fit_s'], one['fit_s'], 1e-7, tag + 'q(X*) var after 5 steps')
        # (the bound is evaluated at each side's own fitted q(X*): the 5-step bound)
        rel(r['pmd_bound'], one['pmd_bound'], 1e-7, tag + 'predict_missing_data bound')
        absolute(r['pmd_mu'], one['pmd_mu'], 1e-7, tag + 'predict_missing_data q(X*) mean')
        absolute(r['pmd_cov'], one['pmd_cov'], 1e-7, tag + 'predict_missing_data q(X*) covariance')
        np.testing.assert_array_equal(r['pmd_cols'], one['pmd_cols'])
        absolute(r['pmd_mean'], one['pmd_mean'], 1e-7, tag + 'predicted mean')
        absolute(r['pmd_var'], one['pmd_var'], 1e-7, tag + 'predicted variance')
        # predict_new_latent_variables at the seeded start that rank 0 made and broadcast: no optimiser in between
        rel(r['new_bound'], one['new_bound'], 1e-12, tag + 'predict_new_latent_variables bound')
        rel(r['new_ll'], one['new_ll'], 1e-12, tag + 'test log-likelihood')
        np.testing.assert_array_equal(r['new_mu'], one['new_mu'])
        np.testing.assert_array_equal(r['new_cov'], one['new_cov'])
        for k in ('fit_mu', 'fit_s', 'pmd_mu', 'pmd_mean', 'pmd_var', 'new_mu', 'tg_mu', 'tg_s'):     # bit-identical over the ranks
            np.testing.assert_array_equal(r[k], ranks[0][k], err_msg=k)
    assert [int(r['pmd_slots']) for r in ranks] == slots                        # prediction_terms is local


def slots_of(fixture, bounds, empty_head=False):
    o_t = points_for_test(golden(fixture), empty_head)[1]
    return [int(o_t[:, lo:hi].any(axis=0).sum()) for lo, hi in bounds]


@pytest.mark.parametrize('kind', ['rand30', 'edge'])
def test_two_ranks_equal_one(dev, tmp_path, kind):
    """Training, imputation, moments and the test-time paths of a mask-trained model on two ranks (one set of children)."""
    one = single_of(dev, D10, kind, ['train', 'impute', 'test'])
    ranks = _run_ranks(tmp_path, '%s:%s:count:train+impute+test' % (D10, kind), 2)
    check_training(ranks, one, [(0, 5), (5, 10)])
    check_imputation(ranks, one)
    check_test_time(ranks, one, slots_of(D10, [(0, 5), (5, 10)]))


def test_three_ranks_with_an_empty_share(dev, tmp_path):
    """D = 6, columns 0 and 1 never observed: rank 0 of 3 owns no observed column, in training and at test time."""
    one = single_of(dev, D6, 'empty01', ['train', 'impute', 'test'], empty_head=True)
    ranks = _run_ranks(tmp_path, '%s:empty01:count:train+impute+test' % D6, 3)
    check_training(ranks, one, [(0, 2), (2, 4), (4, 6)])
    assert ranks[0]['per_dim'].shape == (2, 5) and not ranks[0]['per_dim'].any()      # rank 0: f_hat share 0
    check_imputation(ranks, one)
    slots = slots_of(D6, [(0, 2), (2, 4), (4, 6)], empty_head=True)
    assert slots[0] == 0 and min(slots[1:]) >= 1
    check_test_time(ranks, one, slots)


def test_three_ranks_uneven_shares(dev, tmp_path):
    one = single_of(dev, D10, 'rand30', ['train'])
    ranks = _run_ranks(tmp_path, '%s:rand30:count:train' % D10, 3)
    check_training(ranks, one, [(0, 4), (4, 7), (7, 10)])


def odd_shape_model(dev, **kw):
    """tests/test_gpu_train_masked_d.test_odd_shapes_match_the_oracle's (70, 9, 33, 9, 3, 3): mask_size = 3."""
    from test_gpu_train_masked_d import build as build_raw
    n, d, m, q, t, mask = 70, 9, 33, 9, 3, 3
    rng = np.random.default_rng(n + d)
    y = rng.standard_normal((n, d))
    y = (y - y.mean(0)) / y.std(0)
    raw = dict(x_mean=rng.standard_normal((n, q)), x_var_raw=0.3 * rng.standard_normal((n, q)),
               x_u=rng.standard_normal((m, q)), dp_logits=rng.standard_normal((d // mask, t)),
               gamma_1_raw=rng.standard_normal(max(t - 1, 0)), gamma_2_raw=rng.standard_normal(max(t - 1, 0)),
               w_1_raw=np.array(0.4), w_2_raw=np.array(0.7), gamma_atoms_raw=0.5 * rng.standard_normal((t, q)),
               alpha_atoms_raw=0.5 * rng.standard_normal((t, 1)), beta_atoms_raw=0.5 * rng.standard_normal((t, 1)) + 1.0)
    obs = np.random.default_rng(7).random((n, d)) >= 0.3
    return build_raw(raw, np.where(obs, y, np.nan), dev, obs, mask_size=mask, **kw)


@pytest.mark.parametrize('case', ['D6 rand30', 'D6 empty01', 'odd shape, mask_size 3'])
def test_shard_of_partial_values_sum_to_the_whole(dev, case):
    """_shard_of=(r, w), no communicator: partial_pack() and the partial gradients of the w shares sum to the single-process values;
    w = D is one column per share, and with empty01 two of those shares have no observed column."""
    if case.startswith('D6'):
        g, kind = golden(D6), case.split()[1]
        make = lambda **kw: build(g, dev, kind, **kw)
        worlds = (2, 3, 6)
    else:
        make = lambda **kw: odd_shape_model(dev, **kw)
        worlds = (2, 3, 9)                    # (w = 2: shares of 5 and 4 columns, not aligned to mask_size)
    whole = make()
    pack, grads = whole.partial_pack().cpu().numpy(), {k: v.cpu().numpy() for k, v in whole.gradients().items()}
    for w in worlds:
        parts = [make(_shard_of=(r, w)) for r in range(w)]
        rel(sum(p.partial_pack().cpu().numpy() for p in parts), pack, 1e-12, 'w = %d: partial_pack' % w)
        got = [p.gradients() for p in parts]
        for k, want in grads.items():
            absolute(sum(gr[k].cpu().numpy() for gr in got), want, 1e-9, 'w = %d: %s' % (w, k))
        assert [p.shard[1] - p.shard[0] for p in parts] == [tuple(p.per_dimension_terms[0].shape)[0] for p in parts]


def test_a_flag_on_one_rank_stops_both(dev, tmp_path):
    """The columns of rank 1 sit on an atom whose ARD weights are scaled by 1e-5 (tests/_sharded_worker.py's 'flag' recipe) and
    whose signal variance is 1e200: the factorisation of their A fails, the flag travels with the packed gradients, both ranks
    raise FloatingPointError in the same iteration and only rank 1 saw the trouble itself.  The ARD scale alone flags nothing in
    fp64 (measured: no rank raised, no info entry set; _sharded_masked_worker.FLAG_ALPHA says why), so it cannot show this."""
    ranks = _run_ranks(tmp_path, '%s:rand30:count:flag' % D10, 2)
    print('raised %s, iterations done %s, local flags %s' % ([int(r['raised']) for r in ranks], [int(r['iterations_done']) for r in ranks],
                                                             [int(r['local_flags']) for r in ranks]))
    assert all(int(r['raised']) == 1 for r in ranks)
    assert int(ranks[0]['iterations_done']) == int(ranks[1]['iterations_done'])
    assert int(ranks[0]['local_flags']) == 0 and int(ranks[1]['local_flags']) >= 1


def test_complete_data_model_two_ranks(dev, tmp_path):
    """A sharded precision='f64' model trained on complete data: predictive_marginals and the shared-inducing test-time paths."""
    one = single_of(dev, D10, 'complete', ['impute', 'test'])
    ranks = _run_ranks(tmp_path, '%s:complete:count:impute+test' % D10, 2)
    check_imputation(ranks, one, complete=True)
    check_test_time(ranks, one, slots_of(D10, [(0, 5), (5, 10)]))


def test_complete_data_model_three_ranks_with_an_empty_test_share(dev, tmp_path):
    one = single_of(dev, D6, 'complete', ['test'], empty_head=True)
    ranks = _run_ranks(tmp_path, '%s:complete:count:test' % D6, 3)
    slots = slots_of(D6, [(0, 2), (2, 4), (4, 6)], empty_head=True)
    assert slots[0] == 0 and min(slots[1:]) >= 1
    check_test_time(ranks, one, slots)


def test_argument_checks_and_a_one_rank_group(dev, tmp_path):
    """On a sharded model form='slots', the reference's forms and shard_by='observed' without observed= raise AssertionError (in the
    child); a 1-rank group goes through pack -> all-reduce -> finalize and gives the single-process numbers."""
    one = single_of(dev, D6, 'rand30', ['train'])
    ranks = _run_ranks(tmp_path, '%s:rand30:count:args' % D6, 1)
    assert int(ranks[0]['refused']) == 13
    check_training(ranks, one, [(0, 6)])
    from dp_gp_lvm_amd.models.dp_gp_lvm import dp_gp_lvm
    with pytest.raises(AssertionError, match='needs observed='):
        dp_gp_lvm(golden(D6)['y'], device=dev, shard_by='observed')
    with pytest.raises(AssertionError, match='shard_by must be'):
        build(golden(D6), dev, 'rand30', shard_by='rows')


def test_shard_by_observed(dev, tmp_path):
    """Two ranks on the edge mask (columns 0 and 1 cost 1 and 2): bounds other than the equal-count ones, the same numbers."""
    from dp_gp_lvm_amd.models.dp_gp_lvm import shard_bounds, weighted_shard_bounds
    one = single_of(dev, D10, 'edge', ['train'])
    obs = mask_of('edge', *golden(D10)['y'].shape)
    bounds = [weighted_shard_bounds(obs.sum(axis=0) + 1, r, 2) for r in range(2)]
    assert bounds != [shard_bounds(10, r, 2) for r in range(2)] and bounds[0][1] == bounds[1][0]
    ranks = _run_ranks(tmp_path, '%s:edge:observed:train' % D10, 2)
    check_training(ranks, one, bounds)
