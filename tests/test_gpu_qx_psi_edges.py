"""
GPU tests of the q(X) Psi operators of csrc/qx_psi.hip (statistics, (mu, S) adjoint and parameter adjoint, each in the plain, weighted and
pattern-grouped form) at the edges their feature tests never reach: every register-width instantiation, the multi-tile slab loop of the
adjoint, the (PC, NW) switches of the grouped adjoint's LDS budget, the 48 KiB dynamic-LDS boundary, idle and dead waves, the 32 / 64
edges of M and N, ragged and forced n slabs, and the range of the inputs.  The case lists, the fp64 autograd references, the comparators
and the proof that the lists reach those edges are in tests/test_qx_psi_refs.py (CPU).

Every check: the operator with zfac = None and with the precomputed pair factor, run twice (bit equality), compared with
test_gpu_predict_b1.close's bound at 1e-12 (rtol 1e-12, atol 1e-12 x max(1, max |want|)); psi2 and d_z one 32-block at a time so that a
failure names its tile; psi2 exactly symmetric.  A launch that fails raises in dp_gp_lvm_amd.ops (the return code is not DPGP_OK).  The
forced plans (DPGP_QP_N_SLABS, DPGP_QP_PAIR_SLABS) are read by the library on every call.  Each test prints its largest error as a
fraction of its tolerance (DESIGN.md records them per family).
"""
import pytest
import torch

import test_qx_psi_refs as R

pytestmark = pytest.mark.gpu


def on_device(c, dev):
    t = {k: None if a is None else a.to(dev).contiguous() for k, a in R.inputs(c).items()}
    z, gamma, alpha = t['z'], t['gamma'], t['alpha']
    dz = z[:, :, None, :] - z[:, None, :, :]
    t['zfac'] = ((alpha * alpha)[:, None, None] * torch.exp(-0.25 * torch.sum(gamma[:, None, None, :] * dz * dz, dim=-1))).contiguous()
    return t


def call(op, c, t, zf):
    from dp_gp_lvm_amd import ops
    base = (t['z'], t['mu'], t['s'], t['gamma'], t['alpha'])
    if c.form == 'grouped':
        if op == 'stats':
            return ops.qx_psi_stats_grouped(*base, t['w'], zfac=zf)
        fn = ops.qx_psi_adjoint_grouped if op == 'adjoint' else ops.qx_psi_param_adjoint_grouped
        return fn(*base, t['g1'], t['g2'], t['w'], zfac=zf)
    if op == 'stats':
        return ops.qx_psi_stats_batched(*base, zfac=zf, weights=t['w'])
    fn = ops.qx_psi_adjoint if op == 'adjoint' else ops.qx_psi_param_adjoint
    return fn(*base, t['g1'], t['g2'], zfac=zf, weights=t['w'])


def run_case(dev, c, monkeypatch, record_property):
    """Every (operator, forced plan) of the case against the reference; returns {(op, env, with zfac): outputs} and the largest error as a
    fraction of the tolerance."""
    t, tol, worst, results = on_device(c, dev), R.tol_of(c), 0.0, {}
    for op, env in R.runs_of(c):
        R.set_env(monkeypatch, env)
        names = R.OUTPUTS_OF[op]
        want = R.reference(c, names)
        # the plan that is launched is the one the coverage conditions of test_qx_psi_refs.py were worked out for
        assert R.library_workspace_bytes(op, c) == R.workspace_bytes(op, c, env), '%s %s %s: the plan differs' % (R.case_id(c), op, dict(env))
        for zf in (None, t['zfac']):
            tag = '%s %s %s zfac=%s:' % (R.case_id(c), op, dict(env), zf is not None)
            have, again = call(op, c, t, zf), call(op, c, t, zf)
            for name, h, a in zip(names, have, again):
                assert torch.equal(h, a), tag + ' ' + name + ': two calls differ'
                worst = max(worst, R.compare(name, h.cpu().numpy(), want[name], tol, tag))
            if op == 'stats':
                assert torch.equal(have[1], have[1].transpose(-1, -2)), tag + ' psi2 is not exactly symmetric'
            results[(op, env, zf is not None)] = have
    print('qx_psi_edges %s %s: largest error %.2e of the tolerance %.1e' % (c.family, R.case_id(c), worst, tol))
    record_property('fraction_of_tolerance', worst)
    return results, worst


@pytest.mark.parametrize('c', R.E1, ids=R.case_id)
def test_e1_m_tile_edges(dev, c, monkeypatch, record_property):
    run_case(dev, c, monkeypatch, record_property)


@pytest.mark.parametrize('c', R.E2, ids=R.case_id)
def test_e2_n_edges_and_forced_n_slabs(dev, c, monkeypatch, record_property):
    results, _ = run_case(dev, c, monkeypatch, record_property)
    # a forced number of n slabs only changes the order of additions
    for (op, env, zf), have in results.items():
        if env != R.UNSET:
            for name, h, n in zip(R.OUTPUTS_OF[op], have, results[(op, R.UNSET, zf)]):
                R.compare(name, h.cpu().numpy(), n.cpu().numpy(), R.TOL, '%s %s %s against the natural plan:' % (R.case_id(c), op, dict(env)))


@pytest.mark.parametrize('c', R.E3, ids=R.case_id)
def test_e3_register_widths(dev, c, monkeypatch, record_property):
    run_case(dev, c, monkeypatch, record_property)


@pytest.mark.parametrize('c', R.E4, ids=R.case_id)
def test_e4_pair_slabs(dev, c, monkeypatch, record_property):
    """The adjoint under every forced number of pair slabs against autograd and against the natural plan (1e-12, not bitwise: the order
    of additions differs).  g1 alone and g2 alone pin the Psi1 term to exactly one slab per diagonal tile."""
    results, _ = run_case(dev, c, monkeypatch, record_property)
    for (op, env, zf), have in results.items():
        if env != R.UNSET:
            for name, h, n in zip(R.OUTPUTS_OF[op], have, results[(op, R.UNSET, zf)]):
                R.close_frac(h.cpu().numpy(), n.cpu().numpy(), R.TOL, '%s %s %s against the natural plan' % (R.case_id(c), name, dict(env)))


@pytest.mark.parametrize('c', R.E5, ids=R.case_id)
def test_e5_lds_switch_points(dev, c, monkeypatch, record_property):
    run_case(dev, c, monkeypatch, record_property)


@pytest.mark.parametrize('c', R.E6_CASES, ids=R.case_id)
def test_e6_idle_and_dead_waves(dev, c, monkeypatch, record_property):
    results, _ = run_case(dev, c, monkeypatch, record_property)
    w = R.inputs(c)['w']
    for (op, env, zf), have in results.items():
        tag = '%s %s %s zfac=%s: ' % (R.case_id(c), op, dict(env), zf)
        if op == 'stats':                                           # a weight row (kernel or pattern) of zeros: psi2 exactly 0.0
            rows = [int(i) for i in torch.nonzero((w == 0.0).all(dim=1)).flatten()]
            psi2 = have[1] if c.form == 'grouped' else have[1][None]      # [K, weight row, M, M]
            if c.wkind in ('all_off', 'chunk0_off', 'chunk1_off'):
                assert rows, tag + 'no all-zero weight row'
            for p in rows:
                assert bool((psi2[:, p] == 0.0).all()), tag + 'psi2 of the all-zero weight row %d is not exactly 0.0' % p
        elif c.wkind == 'all_off' and c.gmode == 'g2':             # no weight and no g1: exactly nothing
            for name, h in zip(R.OUTPUTS_OF[op], have):
                assert bool((h == 0.0).all()), tag + name + ' is not exactly 0.0'


@pytest.mark.parametrize('form,kind,p', [('grouped', 'all_off', 5), ('weighted', 'all_off', 1)])
def test_e6_all_zero_weights_leave_the_psi1_part_alone(dev, form, kind, p, monkeypatch):
    """Every point at weight 0: off-diagonal tiles are skipped, and what g2 would add is exactly 0.0, so g1 with any g2 gives the bits of
    g1 alone."""
    R.set_env(monkeypatch, R.UNSET)
    both, g1 = (R.mk('E6', form, kind, 1, p, R.E6_M, R.E6_N, R.E6_Q, gmode=g) for g in ('both', 'g1'))
    assert both in R.E6_CASES and g1 in R.E6_CASES
    tb, t1 = on_device(both, dev), on_device(g1, dev)
    assert torch.equal(tb['g1'], t1['g1']) and torch.equal(tb['z'], t1['z']) and bool((tb['g2'] != 0.0).any())
    for zf in (None, tb['zfac']):
        for hb, h1 in zip(call('adjoint', both, tb, zf), call('adjoint', g1, t1, zf)):
            assert torch.equal(hb, h1) and bool((hb != 0.0).any())


OFF_CASES = [c for c in R.E6_CASES if c.wkind.split('_')[0] in ('wave1', 'step1', 'slab1') and c.gmode == 'both']


@pytest.mark.parametrize('c', OFF_CASES, ids=R.case_id)
def test_e6_zero_weight_points_add_exactly_nothing(dev, c, monkeypatch):
    """Other values of (mu, s) at the points whose every weight is 0 (a whole wave, a whole staged step, a whole n slab) leave psi2 and the
    g1 = 0 adjoints bit for bit what they were: their Psi2-term contribution is exactly 0.0, not merely small."""
    t = on_device(c, dev)
    off = (t['w'] == 0.0).all(dim=0)
    lo, hi = dict(wave1=(64, 128), step1=(32, 64), slab1=(96, 192))[c.wkind.split('_')[0]]
    assert bool(off[lo:hi].all()) and not bool(off.all())
    moved = dict(t)
    moved['mu'], moved['s'] = t['mu'].clone(), t['s'].clone()
    moved['mu'][off] = 0.5 * t['mu'][off] + 0.3
    moved['s'][off] = 2.0 * t['s'][off]
    for d in (t, moved):
        d['g1'] = torch.zeros_like(t['g1'])
    ops_of = dict(R.E6)[c]
    for env in (R.UNSET, ((R.N_KNOB, '3'),)):
        R.set_env(monkeypatch, env)
        for zf in (None, t['zfac']):
            if 'stats' in ops_of:
                assert torch.equal(call('stats', c, t, zf)[1], call('stats', c, moved, zf)[1]), (env, 'psi2')
            if 'param' in ops_of:
                for name, a, b in zip(R.OUTPUTS_OF['param'], call('param', c, t, zf), call('param', c, moved, zf)):
                    assert torch.equal(a, b) and bool((a != 0.0).any()), (env, name)
            if 'adjoint' in ops_of:
                for name, a, b in zip(R.OUTPUTS_OF['adjoint'], call('adjoint', c, t, zf), call('adjoint', c, moved, zf)):
                    assert bool((a[off] == 0.0).all()) and bool((b[off] == 0.0).all()), (env, name, 'rows of the zero-weight points')
                    assert torch.equal(a[~off], b[~off]) and bool((a[~off] != 0.0).any()), (env, name)


@pytest.mark.parametrize('c', R.E7, ids=R.case_id)
def test_e7_range(dev, c, monkeypatch, record_property):
    """Shifted inputs (tolerance x 51, see test_qx_psi_refs.tol_of), s = 0 rows, gamma s up to 1e4, and points so far from every inducing
    input that every exponential underflows: finite (the comparators check it) and within the tolerance."""
    run_case(dev, c, monkeypatch, record_property)
    t = R.inputs(c)
    if c.recipe == 's0':
        assert bool((t['s'][0::3] == 0.0).all())
    if c.recipe == 'gs1e4':
        assert abs(float((t['gamma'].max(dim=0).values * t['s']).max()) - 1e4) < 1e-6
    if c.recipe == 'far':
        assert float(R.reference(c, ('psi1',))['psi1'][:, 0::3].max()) == 0.0      # (underflow, in the reference too)
