"""
GPU tests of the per-point Psi operators (csrc/qx_psi_point.hip: ops.qx_psi_pointwise, ops.qx_psi_point_moments;
csrc/qx_psi_point_adjoint.hip: ops.qx_psi_pointwise_adjoint) at the edges their feature tests never reach: several pair tiles and several
kernels k inside one workgroup (the forced plans DPGP_PW_PAIR_SLABS, DPGP_PA_K_SLABS, DPGP_PA_PAIR_SLABS, read by the library on every
call), every CT / FT / MT / QREG instantiation, both sides of every Q switch and of the 48 KiB dynamic-LDS boundary, the 32 / 16 / 64
edges of M, the columns and N, idle waves and skipped phases, and the range of the inputs.  The case lists, the references (torch fp64
and autograd, held to 1e-14 against mpmath), the plan mirror and the proof that the lists reach those edges are in
tests/test_qx_psi_point_refs.py (CPU).

Every check: zfac = None and the precomputed pair factor, each run twice (bit equality), compared at 1e-12 with
test_gpu_predict_b1.close's bound taken per kernel k, per block of 64 points and (forward) per 16 columns, so that no block hides behind
a larger one; var is held to that bound like the other outputs.  Before each launch the library's workspace query is compared with the
mirror's: the plan that runs is the one the coverage conditions were worked out for.  Each test prints its largest error as a fraction
of its tolerance (DESIGN.md records them per family).
"""
import pytest
import torch

import test_qx_psi_point_refs as R
from test_gpu_qx_psi_point_moments import gidx_of
from test_gpu_qx_psi_pointwise import pair_factor

pytestmark = pytest.mark.gpu


def on_device(case, dev, **replace):
    t = {name: a.to(dev).contiguous() for name, a in dict(R.inputs(case), **replace).items()}
    t['zfac'] = pair_factor(t)
    return t


def base_args(t):
    return t['z'], t['mu'], t['s'], t['gamma'], t['alpha'], t['c'], t['r']


def shape_of_inputs(t):
    k, m, q = t['z'].shape
    return k, t['c'].shape[1], t['r'].shape[2], t['mu'].shape[0], m, q


def planned(op, t, env, monkeypatch):
    """Sets the overrides and checks that the library plans what the mirror plans."""
    R.set_env(monkeypatch, env)
    shape = shape_of_inputs(t)
    assert R.library_workspace_bytes(op, shape) == R.workspace_bytes(op, shape, env), '%s %s %s: the plan differs' % (op, shape, dict(env))


def forward(t, zf, kinds=R.GIDX_KINDS):
    """{'tr', 'quad', ('mean', kind), ('var', kind)}: both forward operators, each called twice."""
    from dp_gp_lvm_amd import ops
    out = {}
    tr, quad = ops.qx_psi_pointwise(*base_args(t), zfac=zf)
    tr_b, quad_b = ops.qx_psi_pointwise(*base_args(t), zfac=zf)
    assert torch.equal(tr, tr_b) and torch.equal(quad, quad_b), 'qx_psi_pointwise: two calls differ'
    out.update(tr=tr, quad=quad)
    k, g, j = shape_of_inputs(t)[:3]
    for kind in kinds:
        gidx = t.get('gidx_' + kind, gidx_of(kind, k, g, j)).to(tr.device)
        mean, var = ops.qx_psi_point_moments(*base_args(t), gidx, t['beta'], zfac=zf)
        mean_b, var_b = ops.qx_psi_point_moments(*base_args(t), gidx, t['beta'], zfac=zf)
        assert torch.equal(mean, mean_b) and torch.equal(var, var_b), 'qx_psi_point_moments: two calls differ'
        out[('mean', kind)], out[('var', kind)] = mean, var
    return out


def adjoint(t, mode, zf):
    from dp_gp_lvm_amd import ops
    adj = tuple(a.contiguous() for a in R.adjoints(t, mode))
    have, again = (ops.qx_psi_pointwise_adjoint(*base_args(t), *adj, zfac=zf) for _ in range(2))
    assert torch.equal(have[0], again[0]) and torch.equal(have[1], again[1]), 'qx_psi_pointwise_adjoint: two calls differ'
    return {('d_mu', mode): have[0], ('d_s', mode): have[1]}


def compare(c, have, want, tag):
    """Every output of `have` against `want` ({name: array}), blockwise; returns the largest fraction of the tolerance."""
    worst = 0.0
    for name, hv in have.items():
        forward_output = name in ('tr', 'quad') or name[0] in ('mean', 'var')
        wv = want[name]
        wv = wv.cpu().numpy() if torch.is_tensor(wv) else wv
        worst = max(worst, R.blocks_close_frac(hv.cpu().numpy(), wv, R.tol_of(c), '%s %s' % (tag, name), cols=16 if forward_output else None))
    return worst


def run_forward(dev, c, monkeypatch):
    t, ref, worst, results = on_device(c, dev), R.reference(c), 0.0, {}
    for env in R.fwd_envs(c):
        planned('fwd', t, env, monkeypatch)
        for zf in (None, t['zfac']):
            tag = '%s fwd %s zfac=%s:' % (R.case_id(c), dict(env), zf is not None)
            have = forward(t, zf)
            worst = max(worst, compare(c, have, ref, tag))
            if env != R.UNSET:
                compare(c, have, results[(R.UNSET, zf is not None)], tag + ' against the natural plan:')
            results[(env, zf is not None)] = have
    return results, worst


def run_adjoint(dev, c, monkeypatch, modes=None):
    t, ref, worst, results = on_device(c, dev), R.reference(c), 0.0, {}
    for env in R.adj_envs(c):
        planned('adj', t, env, monkeypatch)
        for mode in modes or R.modes_of(c):
            for zf in (None, t['zfac']):
                tag = '%s adj %s %s zfac=%s:' % (R.case_id(c), dict(env), mode, zf is not None)
                have = adjoint(t, mode, zf)
                worst = max(worst, compare(c, have, ref, tag))
                if env != R.UNSET:
                    compare(c, have, results[(R.UNSET, mode, zf is not None)], tag + ' against the natural plan:')
                results[(env, mode, zf is not None)] = have
    return results, worst


def report(c, what, worst, record_property):
    print('qx_psi_point_edges %s %s %s: largest error %.2e of the tolerance %.1e' % (c.family, R.case_id(c), what, worst, R.tol_of(c)))
    record_property('fraction_of_tolerance', worst)


def run_both(dev, c, monkeypatch, record_property):
    fwd, wf = run_forward(dev, c, monkeypatch)
    adj, wa = run_adjoint(dev, c, monkeypatch)
    report(c, 'forward %.2e adjoint %.2e' % (wf, wa), max(wf, wa), record_property)
    return fwd, adj


@pytest.mark.parametrize('c', R.P1, ids=R.case_id)
def test_p1_m_tile_edges(dev, c, monkeypatch, record_property):
    run_both(dev, c, monkeypatch, record_property)


@pytest.mark.parametrize('c', R.P2, ids=R.case_id)
def test_p2_n_edges(dev, c, monkeypatch, record_property):
    run_both(dev, c, monkeypatch, record_property)


@pytest.mark.parametrize('c', R.P3, ids=R.case_id)
def test_p3_column_edges(dev, c, monkeypatch, record_property):
    run_both(dev, c, monkeypatch, record_property)


@pytest.mark.parametrize('c', R.P4, ids=R.case_id)
def test_p4_q_edges(dev, c, monkeypatch, record_property):
    run_both(dev, c, monkeypatch, record_property)


@pytest.mark.parametrize('c', R.P5, ids=R.case_id)
def test_p5_forced_pair_slabs_forward(dev, c, monkeypatch, record_property):
    """DPGP_PW_PAIR_SLABS unset, 1, 2, 4, 6, tiles: each plan against the reference and against the natural plan (1e-12, not bitwise: the
    order of additions differs), through the slab reduction of both second launches."""
    results, worst = run_forward(dev, c, monkeypatch)
    assert len({env for env, _ in results}) == 6
    report(c, 'forward', worst, record_property)


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('c', R.P5, ids=R.case_id)
def test_p5_forced_slabs_adjoint(dev, c, mode, monkeypatch, record_property):
    """DPGP_PA_PAIR_SLABS unset, 1, 2, 4, 6, tiles x DPGP_PA_K_SLABS unset, 1, 2, K.  h alone pins the Psi1 phase to pair slab 0 (run in
    every slab it would come out pslabs times too large), gq + gt alone the Psi2 phase to each tile exactly once."""
    results, worst = run_adjoint(dev, c, monkeypatch, modes=(mode,))
    assert len({env for env, _, _ in results}) == 24
    report(c, 'adjoint ' + mode, worst, record_property)


def test_p6_zero_adjoint_waves(dev, monkeypatch, record_property):
    """Points 16..31 (a wave beside busy ones) and 64..127 (a workgroup) have h = gq = gt = 0: their rows are exactly 0.0 in every mode
    and plan, and other values of (mu, s) at those points change no bit of the other rows."""
    c = R.P6[0]
    results, worst = run_adjoint(dev, c, monkeypatch)
    report(c, 'adjoint', worst, record_property)
    off = torch.zeros(c.n, dtype=torch.bool)
    off[16:32] = True
    off[64:128] = True
    t = R.inputs(c)
    mu, s = t['mu'].clone(), t['s'].clone()
    mu[off] = 0.5 * mu[off] + 0.3
    s[off] = 2.0 * s[off]
    moved = on_device(c, dev, mu=mu, s=s)
    for (env, mode, zf), have in results.items():
        planned('adj', moved, env, monkeypatch)
        other = adjoint(moved, mode, moved['zfac'] if zf else None)
        for name, a in have.items():
            a, b = a.cpu(), other[name].cpu()
            assert bool((a[off] == 0.0).all()) and bool((b[off] == 0.0).all()), (env, mode, name, 'rows of the zero-adjoint points')
            assert torch.equal(a[~off], b[~off]) and bool((a[~off] != 0.0).all()), (env, mode, name)


def test_p6_zero_adjoint_kernel_inside_the_k_loop(dev, monkeypatch, record_property):
    """Kernel 1 of 3 has zero adjoints.  Under DPGP_PA_K_SLABS = 1 one workgroup walks all three: kernel 1 adds exactly 0.0 (alone: an
    all-zero result), and kernels 0 and 2 give the bits of a call that holds only them, at the same plan."""
    c = R.P6[1]
    results, worst = run_adjoint(dev, c, monkeypatch)
    report(c, 'adjoint', worst, record_property)
    env = ((R.PA_K_KNOB, '1'),)
    t = R.inputs(c)
    per_kernel = ('z', 'gamma', 'alpha', 'c', 'r', 'beta', 'h', 'gq', 'gt')
    two = on_device(c, dev, **{name: t[name][[0, 2]] for name in per_kernel})
    one = on_device(c, dev, **{name: t[name][[1]] for name in per_kernel})
    for sub in (two, one):
        planned('adj', sub, env, monkeypatch)
    assert R.pa_plan(*R.shape_of(c), env)['k_per_slab'] == 3 and R.pa_plan(2, *R.shape_of(c)[1:], env)['pslabs'] == R.pa_plan(*R.shape_of(c), env)['pslabs']
    for mode in R.MODES:
        for zf in (False, True):
            have = results[(env, mode, zf)]
            for name, a in adjoint(two, mode, two['zfac'] if zf else None).items():
                assert torch.equal(a, have[name]) and bool((a != 0.0).any()), (mode, zf, name)
            for name, a in adjoint(one, mode, one['zfac'] if zf else None).items():
                assert bool((a == 0.0).all()), (mode, zf, name)


def test_p6_zero_columns_of_r(dev, monkeypatch, record_property):
    """r = 0 in a column and gidx = -1 there: mean exactly 0.0 and var exactly alpha + 1/beta, under the natural plan and two pair slabs;
    the other columns keep their bits."""
    c = R.P6[0]
    results, worst = run_forward(dev, c, monkeypatch)
    report(c, 'forward', worst, record_property)
    zero = [0, 5, 16]
    keep = [i for i in range(c.j) if i not in zero]
    t = R.inputs(c)
    r = t['r'].clone()
    r[:, :, zero] = 0.0
    gidx = gidx_of('random', c.k, c.g, c.j).clone()
    gidx[:, zero] = -1
    full, cut = on_device(c, dev, gidx_random=gidx), on_device(c, dev, r=r, gidx_random=gidx)
    base = (full['alpha'] + 1.0 / full['beta'])[:, None, None].expand(-1, c.n, len(zero))
    for env in R.fwd_envs(c):
        planned('fwd', full, env, monkeypatch)
        for zf in (None, full['zfac']):
            a, b = forward(full, zf, kinds=('random',)), forward(cut, zf, kinds=('random',))
            assert bool((b[('mean', 'random')][:, :, zero] == 0.0).all()) and torch.equal(b[('var', 'random')][:, :, zero], base), env
            assert bool((b['quad'][:, :, zero] == 0.0).all()) and torch.equal(a['tr'], b['tr']), env
            for name in ('quad', ('mean', 'random'), ('var', 'random')):
                assert torch.equal(a[name][:, :, keep], b[name][:, :, keep]), (env, name)


@pytest.mark.parametrize('c', R.P7, ids=R.case_id)
def test_p7_range(dev, c, monkeypatch, record_property):
    """s = 0 rows, gamma s up to 1e4, a third of the points 40 units from every inducing input (with and without the workgroups' first
    points, the adjoint kernel's centres, among them), z and mu moved by 50: finite (the comparator checks it) and within 1e-12 of the
    reference, which test_qx_psi_point_refs holds to 1e-14 at that offset too.  The far points' results are 0 or tiny."""
    fwd, adj = run_both(dev, c, monkeypatch, record_property)
    if c.recipe in ('far', 'far1'):
        far = slice(0 if c.recipe == 'far' else 1, None, 3)
        for have in fwd.values():
            assert float(have['tr'][:, far].abs().max()) < 1e-100 and float(have['quad'][:, far].abs().max()) < 1e-100
            assert float(have[('mean', 'random')][:, far].abs().max()) < 1e-100
        for have in adj.values():
            assert float(have[('d_mu', 'all')][far].abs().max()) < 1e-100 and float(have[('d_s', 'all')][far].abs().max()) < 1e-100
