"""CPU tests (no GPU) of the C ABI of the parallel-transport operators (include/dpgp.h, csrc/ard_rbf_point_metric.hip,
csrc/geodesic_accel.hip) and of the argument checks of their ops front-ends: the entry points are exported and bound, bad
arguments come back with their negative codes in argument order and before anything is launched (every device pointer here
is a dummy: a launch would fault), the workspace query is 0 for a shape out of range (Q + 1 + F = 65 included: the feature block
is Q + 1 + F wide) and holds nothing of size N M, and ops raises TypeError / ValueError / RuntimeError as documented."""
import ctypes
import os
import re

import pytest
import torch

from dp_gp_lvm_amd import _lib, ops

P = ctypes.c_void_p(16)          # non-NULL, never dereferenced: every call below returns before a launch
STEM = 'dpgp_ard_rbf_point_transport'
ACCEL = 'dpgp_geodesic_transport_f64'
CASES = [('K', 0, -1), ('N', 0, -2), ('M', -1, -3), ('Q', 0, -4), ('F', 0, -5), ('z', None, -6), ('x', None, -7), ('v', None, -8),
         ('w', None, -9), ('gamma', None, -10), ('alpha', None, -11), ('p', None, -12), ('g', None, -13), ('gam', None, -14),
         ('tgam', None, -15), ('ws', None, -16), ('ws_bytes', 7, -17)]
GOOD = dict(K=1, N=2, M=3, Q=2, F=2)
ACCEL_CASES = [('K', 0, -1), ('N', -3, -2), ('Q', 0, -3), ('F', 0, -4), ('g', None, -5), ('gam', None, -6), ('tgam', None, -7),
               ('prior', None, -8), ('v', None, -9), ('a', None, -10), ('dw', None, -11), ('speed', None, -12), ('info', None, -13)]
ACCEL_GOOD = dict(K=1, N=2, Q=2, F=2)


def call(**kw):
    a = dict(GOOD, z=P, x=P, v=P, w=P, gamma=P, alpha=P, p=P, g=P, gam=P, tgam=P, ws=P, ws_bytes=1 << 20)
    a.update(kw)
    return getattr(_lib.lib(), STEM + '_f64')(*a.values(), None)


def call_accel(**kw):
    a = dict(ACCEL_GOOD, g=P, gam=P, tgam=P, prior=P, v=P, a=P, dw=P, speed=P, info=P)
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
    assert len(_lib.SIGNATURES[STEM + '_workspace_bytes'][1]) == 5
    assert len(_lib.SIGNATURES[STEM + '_f64'][1]) == 5 + 10 + 3            # z, x, v, w, gamma, alpha, p, g, gam, tgam; ws ..
    assert len(_lib.SIGNATURES[ACCEL][1]) == 4 + 9 + 1                     # g, gam, tgam, prior, v, a, dw, speed, info; stream
    assert callable(ops.ard_rbf_point_transport) and callable(ops.geodesic_transport)
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'dpgp.h')).read()
    assert 'size_t %s_workspace_bytes(int K, int N, int M, int Q, int F);' % STEM in header
    assert _header_names(header, STEM + '_f64') == [name for name, _, _ in CASES] + ['stream']    # the codes' order
    assert _header_names(header, ACCEL) == [name for name, _, _ in ACCEL_CASES] + ['stream']


@pytest.mark.parametrize('fn, cases, good', [(call, CASES, GOOD), (call_accel, ACCEL_CASES, ACCEL_GOOD)], ids=['transport', 'accel'])
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


def test_q_and_f_limits():
    assert call(Q=63, F=1) == -4 and call(Q=64, F=1) == -4                 # Q + 1 + F <= 64 with F >= 1: 62 is the last Q
    assert call(Q=62, F=2) == -5 and call(Q=10, F=54) == -5 and call(Q=1, F=63) == -5 and call(Q=10, F=-1) == -5
    for q, f in ((62, 1), (10, 53), (1, 62), (31, 32)):                    # (W = 64 passes; stopped before the launch)
        assert call(Q=q, F=f, ws_bytes=0) == -17
    assert call_accel(Q=65) == -3 and call_accel(F=64) == -4
    assert call_accel(Q=64, F=63, info=None) == -13                        # (64 and 63 pass the checks)


def test_workspace_query_holds_nothing_of_size_n_m_and_is_zero_out_of_range():
    query = getattr(_lib.lib(), STEM + '_workspace_bytes')
    for shape in [(1, 1, 1, 1, 1), (3, 130, 200, 21, 7), (512, 320, 128, 10, 5), (8, 3200, 128, 10, 10), (1, 10000, 128, 31, 32),
                  (1, 2, 3, 62, 1), (1, 2, 3, 1, 62)]:
        assert 0 < query(*shape) <= 256, shape                               # the results are written from the accumulators
        assert call(ws_bytes=query(*shape) - 1) == -17
    for shape in [(0, 2, 3, 2, 1), (1, 0, 3, 2, 1), (1, 2, 0, 2, 1), (1, 2, 3, 0, 1), (1, 2, 3, 2, 0), (1, 2, 3, 32, 32),
                  (1, 2, 3, 63, 1), (1, 2, 3, 1, 63), (1, 2, 3, 10, 54), (-1, 2, 3, 2, 1), (1, -5, 3, 2, 1), (1, 2, 3, 2, -1)]:
        assert query(*shape) == 0, shape
    assert query(1, 2, 3, 31, 33) == 0 and query(1, 2, 3, 31, 32) > 0        # Q + 1 + F = 65 | 64


def _args(k=2, n=5, m=4, q=3, f=2):
    t = torch.float64
    return dict(z=torch.zeros((k, m, q), dtype=t), x=torch.zeros((n, q), dtype=t), v=torch.zeros((n, q), dtype=t),
                w=torch.zeros((n, f, q), dtype=t), gamma=torch.ones((k, q), dtype=t), alpha=torch.ones(k, dtype=t),
                p=torch.zeros((k, m, m), dtype=t))


def _run(a):
    return ops.ard_rbf_point_transport(a['z'], a['x'], a['v'], a['w'], a['gamma'], a['alpha'], a['p'])


def test_ops_transport_argument_errors():
    for name in ('z', 'x', 'v', 'w', 'gamma', 'alpha', 'p'):
        a = _args()
        a[name] = a[name].to(torch.float32)
        with pytest.raises(TypeError, match='%s must' % name):
            _run(a)
        a[name] = a[name].numpy()
        with pytest.raises(TypeError, match='%s must' % name):
            _run(a)
    t = torch.float64
    wrong = dict(z=torch.zeros((2, 4), dtype=t), x=torch.zeros((5, 4), dtype=t), v=torch.zeros((4, 3), dtype=t),
                 w=torch.zeros((5, 3), dtype=t), gamma=torch.ones((2, 4), dtype=t), alpha=torch.ones(3, dtype=t),
                 p=torch.zeros((2, 4, 3), dtype=t))
    for name, bad in wrong.items():
        a = _args()
        a[name] = bad
        with pytest.raises(ValueError, match='^%s must' % name):
            _run(a)
    for bad in (torch.zeros((4, 2, 3), dtype=t), torch.zeros((5, 0, 3), dtype=t), torch.zeros((5, 2, 4), dtype=t)):
        with pytest.raises(ValueError, match='^w must'):
            _run(dict(_args(), w=bad))
    with pytest.raises(ValueError, match=r'Q \+ 1 \+ F <= 64'):              # W = 65: well-formed, one column too wide
        _run(_args(q=31, f=33))
    with pytest.raises(ValueError, match=r'Q \+ 1 \+ F <= 64'):
        _run(_args(q=63, f=1))
    with pytest.raises(RuntimeError, match='must live on the GPU'):          # well-formed host tensors: there is no CPU path
        _run(_args(q=31, f=32))


def _accel_args(k=2, n=5, q=3, f=2):
    t = torch.float64
    return dict(g=torch.zeros((k, n, q, q), dtype=t), gam=torch.zeros((k, n, q), dtype=t), tgam=torch.zeros((k, n, f, q), dtype=t),
                prior=torch.ones(q, dtype=t), v=torch.zeros((n, q), dtype=t))


def test_ops_geodesic_transport_argument_errors():
    run = lambda a: ops.geodesic_transport(a['g'], a['gam'], a['tgam'], a['prior'], a['v'])
    for name in ('g', 'gam', 'tgam', 'prior', 'v'):
        a = _accel_args()
        a[name] = a[name].to(torch.float32)
        with pytest.raises(TypeError, match='^%s must' % name):
            run(a)
        a[name] = a[name].numpy()
        with pytest.raises(TypeError, match='^%s must' % name):
            run(a)
    t = torch.float64
    wrong = dict(g=torch.zeros((2, 5, 3, 2), dtype=t), gam=torch.zeros((2, 5, 2), dtype=t), tgam=torch.zeros((2, 5, 3), dtype=t),
                 prior=torch.ones(4, dtype=t), v=torch.zeros((4, 3), dtype=t))
    for name, bad in wrong.items():
        a = _accel_args()
        a[name] = bad
        with pytest.raises(ValueError, match='^%s must' % name):
            run(a)
    for bad in (torch.zeros((2, 5, 0, 3), dtype=t), torch.zeros((2, 5, 64, 3), dtype=t), torch.zeros((2, 4, 2, 3), dtype=t)):
        with pytest.raises(ValueError, match='^tgam must'):
            run(dict(_accel_args(), tgam=bad))
    with pytest.raises(ValueError, match='g must'):
        run(_accel_args(q=65))
    with pytest.raises(RuntimeError, match='must live on the GPU'):
        run(_accel_args(q=64, f=63))
