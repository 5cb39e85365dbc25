"""CPU tests (no GPU) of the C ABI of the geodesic-tangent operators (include/dpgp.h, csrc/ard_rbf_point_metric.hip,
csrc/geodesic_accel.hip) and of the argument checks of their ops front-ends: the entry points are exported and bound, bad
arguments come back with their negative codes in argument order and before anything is launched (every device pointer here
is a dummy: a launch would fault), the workspace query is 0 for a shape out of range (Q = 32 included: the feature block is
2 Q + 2 wide) and holds nothing of size N M, and ops raises TypeError / ValueError / RuntimeError as documented."""
import ctypes
import os
import re

import pytest
import torch

from dp_gp_lvm_amd import _lib, ops

P = ctypes.c_void_p(16)          # non-NULL, never dereferenced: every call below returns before a launch
STEM = 'dpgp_ard_rbf_point_christoffel_tangent'
ACCEL = 'dpgp_geodesic_accel_tangent_f64'
CASES = [('K', 0, -1), ('N', 0, -2), ('M', -1, -3), ('Q', 0, -4), ('z', None, -5), ('x', None, -6), ('v', None, -7),
         ('dx', None, -8), ('dv', None, -9), ('gamma', None, -10), ('alpha', None, -11), ('p', None, -12), ('g', None, -13),
         ('gam', None, -14), ('dg', None, -15), ('dgam', None, -16), ('ws', None, -17), ('ws_bytes', 7, -18)]
GOOD = dict(K=1, N=2, M=3, Q=2)
ACCEL_CASES = [('K', 0, -1), ('N', -3, -2), ('Q', 0, -3), ('g', None, -4), ('gam', None, -5), ('dg', None, -6), ('dgam', None, -7),
               ('prior', None, -8), ('v', None, -9), ('a', None, -10), ('da', None, -11), ('speed', None, -12), ('info', None, -13)]
ACCEL_GOOD = dict(K=1, N=2, Q=2)


def call(**kw):
    a = dict(GOOD, z=P, x=P, v=P, dx=P, dv=P, gamma=P, alpha=P, p=P, g=P, gam=P, dg=P, dgam=P, ws=P, ws_bytes=1 << 20)
    a.update(kw)
    return getattr(_lib.lib(), STEM + '_f64')(*a.values(), None)


def call_accel(**kw):
    a = dict(ACCEL_GOOD, g=P, gam=P, dg=P, dgam=P, prior=P, v=P, a=P, da=P, speed=P, info=P)
    a.update(kw)
    return getattr(_lib.lib(), ACCEL)(*a.values(), None)


def _header_names(header, name):
    decl = re.search(r'int %s\(([^;]*)\);' % name, header)
    assert decl is not None, name
    return [a.split()[-1].lstrip('*') for a in decl.group(1).replace('\n', ' ').split(',')]


def test_entry_points_are_exported_bound_and_declared():
    lib = _lib.lib()
    for n in (STEM + '_workspace_bytes', STEM + '_f64', ACCEL):
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES[STEM + '_workspace_bytes'][1]) == 4
    assert len(_lib.SIGNATURES[STEM + '_f64'][1]) == 4 + 12 + 3            # z, x, v, dx, dv, gamma, alpha, p, g, gam, dg, dgam; ws ..
    assert len(_lib.SIGNATURES[ACCEL][1]) == 3 + 10 + 1                    # g, gam, dg, dgam, prior, v, a, da, speed, info; stream
    assert callable(ops.ard_rbf_point_christoffel_tangent) and callable(ops.geodesic_accel_tangent)
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'dpgp.h')).read()
    assert 'size_t %s_workspace_bytes(int K, int N, int M, int Q);' % STEM in header
    assert _header_names(header, STEM + '_f64') == [name for name, _, _ in CASES] + ['stream']    # the codes' order
    assert _header_names(header, ACCEL) == [name for name, _, _ in ACCEL_CASES] + ['stream']


@pytest.mark.parametrize('fn, cases, good', [(call, CASES, GOOD), (call_accel, ACCEL_CASES, ACCEL_GOOD)], ids=['tangent', 'accel'])
def test_bad_arguments_come_back_with_their_codes_in_order(fn, cases, good):
    for name, bad, code in cases:
        assert fn(**{name: bad}) == code, name
    # with every argument bad at once the first check answers; repairing them one by one walks down the list
    bad = {name: value for name, value, _ in cases}
    for name, _, code in cases:
        assert fn(**bad) == code, name
        if name != 'ws_bytes':
            bad[name] = good.get(name, P)
    codes = [code for _, _, code in cases]
    assert codes == list(range(-1, -len(codes) - 1, -1))


def test_q_limits():
    assert call(Q=32) == -4 and call(Q=33) == -4 and call(Q=63) == -4      # 2 Q + 2 feature columns: 31 is the last Q
    assert call(Q=31, ws_bytes=0) == -18                                   # (31 passes the Q check; stopped before the launch)
    assert call_accel(Q=65) == -3
    assert call_accel(Q=64, info=None) == -13                              # (64 passes the Q check)


def test_workspace_query_holds_nothing_of_size_n_m_and_is_zero_out_of_range():
    query = getattr(_lib.lib(), STEM + '_workspace_bytes')
    for shape in [(1, 1, 1, 1), (3, 130, 200, 21), (512, 320, 128, 10), (8, 3200, 128, 10), (1, 10000, 128, 31)]:
        assert 0 < query(*shape) <= 256, shape                               # the results are written from the accumulators
        assert call(ws_bytes=query(*shape) - 1) == -18
    for shape in [(0, 2, 3, 2), (1, 0, 3, 2), (1, 2, 0, 2), (1, 2, 3, 0), (1, 2, 3, 32), (1, 2, 3, 64), (-1, 2, 3, 2), (1, -5, 3, 2)]:
        assert query(*shape) == 0, shape


def _args(k=2, n=5, m=4, q=3):
    f = torch.float64
    return dict(z=torch.zeros((k, m, q), dtype=f), x=torch.zeros((n, q), dtype=f), v=torch.zeros((n, q), dtype=f),
                dx=torch.zeros((n, q), dtype=f), dv=torch.zeros((n, q), dtype=f), gamma=torch.ones((k, q), dtype=f),
                alpha=torch.ones(k, dtype=f), p=torch.zeros((k, m, m), dtype=f))


def _run(a):
    return ops.ard_rbf_point_christoffel_tangent(a['z'], a['x'], a['v'], a['dx'], a['dv'], a['gamma'], a['alpha'], a['p'])


def test_ops_tangent_argument_errors():
    for name in ('z', 'x', 'v', 'dx', 'dv', 'gamma', 'alpha', 'p'):
        a = _args()
        a[name] = a[name].to(torch.float32)
        with pytest.raises(TypeError, match='%s must' % name):
            _run(a)
        a[name] = a[name].numpy()
        with pytest.raises(TypeError, match='%s must' % name):
            _run(a)
    f = torch.float64
    wrong = dict(z=torch.zeros((2, 4), dtype=f), x=torch.zeros((5, 4), dtype=f), v=torch.zeros((4, 3), dtype=f),
                 dx=torch.zeros((5, 2), dtype=f), dv=torch.zeros((5,), dtype=f), gamma=torch.ones((2, 4), dtype=f),
                 alpha=torch.ones(3, dtype=f), p=torch.zeros((2, 4, 3), dtype=f))
    for name, bad in wrong.items():
        a = _args()
        a[name] = bad
        with pytest.raises(ValueError, match='^%s must' % name):
            _run(a)
    with pytest.raises(ValueError, match='Q <= 31'):                         # Q = 32: well-formed, one column pair too wide
        _run(_args(q=32))
    with pytest.raises(RuntimeError, match='must live on the GPU'):          # well-formed host tensors: there is no CPU path
        _run(_args(q=31))


def _accel_args(k=2, n=5, q=3):
    f = torch.float64
    return dict(g=torch.zeros((k, n, q, q), dtype=f), gam=torch.zeros((k, n, q), dtype=f), dg=torch.zeros((k, n, q, q), dtype=f),
                dgam=torch.zeros((k, n, q), dtype=f), prior=torch.ones(q, dtype=f), v=torch.zeros((n, q), dtype=f))


def test_ops_geodesic_accel_tangent_argument_errors():
    run = lambda a: ops.geodesic_accel_tangent(a['g'], a['gam'], a['dg'], a['dgam'], a['prior'], a['v'])
    for name in ('g', 'gam', 'dg', 'dgam', 'prior', 'v'):
        a = _accel_args()
        a[name] = a[name].to(torch.float32)
        with pytest.raises(TypeError, match='^%s must' % name):
            run(a)
        a[name] = a[name].numpy()
        with pytest.raises(TypeError, match='^%s must' % name):
            run(a)
    f = torch.float64
    wrong = dict(g=torch.zeros((2, 5, 3, 2), dtype=f), gam=torch.zeros((2, 5, 2), dtype=f), dg=torch.zeros((2, 5, 3, 2), dtype=f),
                 dgam=torch.zeros((1, 5, 3), dtype=f), prior=torch.ones(4, dtype=f), v=torch.zeros((4, 3), dtype=f))
    for name, bad in wrong.items():
        a = _accel_args()
        a[name] = bad
        with pytest.raises(ValueError, match='^%s must' % name):
            run(a)
    with pytest.raises(ValueError, match='g must'):
        run(_accel_args(q=65))
    with pytest.raises(RuntimeError, match='must live on the GPU'):
        run(_accel_args(q=64))
