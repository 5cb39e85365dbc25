"""CPU tests (no GPU) of the latent-metric operators' C ABI (include/dpgp.h, csrc/ard_rbf_point_metric.hip) and of the argument
checks of their ops front-end: the entry points are exported and bound, bad arguments come back with their negative codes in
argument order and before anything is launched (every device pointer here is a dummy: a launch would fault), the workspace
query is 0 for a shape out of range and holds no feature array, and ops raises TypeError / ValueError / RuntimeError as documented."""
import ctypes

import pytest
import torch

from dp_gp_lvm_amd import _lib, ops

P = ctypes.c_void_p(16)          # non-NULL, never dereferenced: every call below returns before a launch
METRIC, JACOBIAN = 'dpgp_ard_rbf_point_metric', 'dpgp_ard_rbf_point_jacobian'
CASES = {
    METRIC: [('K', 0, -1), ('N', 0, -2), ('M', -1, -3), ('Q', 0, -4), ('z', None, -5), ('x', None, -6), ('gamma', None, -7),
             ('alpha', None, -8), ('p', None, -9), ('g', None, -10), ('ws', None, -11), ('ws_bytes', 7, -12)],
    JACOBIAN: [('K', 0, -1), ('J', 0, -2), ('N', -2, -3), ('M', 0, -4), ('Q', 0, -5), ('z', None, -6), ('x', None, -7),
               ('gamma', None, -8), ('alpha', None, -9), ('r', None, -10), ('jac', None, -11), ('ws', None, -12),
               ('ws_bytes', 7, -13)],
}
GOOD = {METRIC: dict(K=1, N=2, M=3, Q=2), JACOBIAN: dict(K=1, J=3, N=2, M=3, Q=2)}
STEMS = (METRIC, JACOBIAN)


def call(stem, **kw):
    last = dict(p=P, g=P) if stem == METRIC else dict(r=P, jac=P)
    a = dict(GOOD[stem], z=P, x=P, gamma=P, alpha=P, **last, ws=P, ws_bytes=1 << 20)
    a.update(kw)
    return getattr(_lib.lib(), stem + '_f64')(*a.values(), None)


@pytest.mark.parametrize('stem', STEMS)
def test_entry_points_are_exported_and_bound(stem):
    lib = _lib.lib()
    for n in (stem + '_workspace_bytes', stem + '_f64'):
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    dims = len(GOOD[stem])
    assert len(_lib.SIGNATURES[stem + '_workspace_bytes'][1]) == dims
    assert len(_lib.SIGNATURES[stem + '_f64'][1]) == dims + 6 + 3       # z, x, gamma, alpha, p | r, result; ws, ws_bytes, stream
    assert callable(ops.ard_rbf_point_metric) and callable(ops.ard_rbf_point_jacobian)


@pytest.mark.parametrize('stem', STEMS)
def test_bad_arguments_come_back_with_their_codes_in_order(stem):
    for name, bad, code in CASES[stem]:
        assert call(stem, **{name: bad}) == code, name
    assert call(stem, Q=65) == CASES[stem][len(GOOD[stem]) - 1][2]
    # with every argument bad at once the first check answers; repairing them one by one walks down the list
    bad = {name: value for name, value, _ in CASES[stem]}
    for name, _, code in CASES[stem]:
        assert call(stem, **bad) == code, name
        if name != 'ws_bytes':
            bad[name] = GOOD[stem].get(name, P)
    codes = [code for _, _, code in CASES[stem]]
    assert codes == list(range(-1, -len(codes) - 1, -1))


def test_workspace_queries_hold_no_feature_array():
    lib = _lib.lib()
    metric, jacobian = lib.dpgp_ard_rbf_point_metric_workspace_bytes, lib.dpgp_ard_rbf_point_jacobian_workspace_bytes
    assert 0 < metric(4, 4096, 128, 10) < 8 * 4 * 4096 * 128 * 10 // 4
    assert 0 < jacobian(4, 60, 4096, 128, 10) < 8 * 4 * 4096 * 128 * 10 // 4
    for shape in [(1, 1, 1, 1), (3, 130, 200, 21), (512, 500, 128, 10), (1, 10000, 128, 64)]:
        assert 0 < metric(*shape) <= 256, shape                          # the results are written from the accumulators
        assert 0 < jacobian(shape[0], 7, *shape[1:]) <= 256, shape
        assert call(METRIC, ws_bytes=metric(*shape) - 1) == -12 and call(JACOBIAN, ws_bytes=metric(*shape) - 1) == -13
    for shape in [(0, 2, 3, 2), (1, 0, 3, 2), (1, 2, 0, 2), (1, 2, 3, 0), (1, 2, 3, 65), (-1, 2, 3, 2)]:
        assert metric(*shape) == 0, shape
        assert jacobian(shape[0], 1, *shape[1:]) == 0, shape
    assert jacobian(1, 0, 2, 3, 2) == 0 and jacobian(1, -4, 2, 3, 2) == 0


def _args(k=2, n=5, m=4, q=3, j=2):
    f = torch.float64
    return dict(z=torch.zeros((k, m, q), dtype=f), x=torch.zeros((n, q), dtype=f), gamma=torch.ones((k, q), dtype=f),
                alpha=torch.ones(k, dtype=f), p=torch.zeros((k, m, m), dtype=f), r=torch.zeros((k, m, j), dtype=f))


def _run(which, a):
    if which == 'metric':
        return ops.ard_rbf_point_metric(a['z'], a['x'], a['gamma'], a['alpha'], a['p'])
    return ops.ard_rbf_point_jacobian(a['z'], a['x'], a['gamma'], a['alpha'], a['r'])


@pytest.mark.parametrize('which', ['metric', 'jacobian'])
def test_ops_argument_errors(which):
    last = 'p' if which == 'metric' else 'r'
    for name in ('z', 'x', 'gamma', 'alpha', last):
        a = _args()
        a[name] = a[name].to(torch.float32)
        with pytest.raises(TypeError, match=name):
            _run(which, a)
        a[name] = a[name].numpy()
        with pytest.raises(TypeError, match=name):
            _run(which, a)
    f = torch.float64
    wrong = dict(z=torch.zeros((2, 4), dtype=f), x=torch.zeros((5, 4), dtype=f), gamma=torch.ones((2, 4), dtype=f),
                 alpha=torch.ones(3, dtype=f))
    wrong[last] = torch.zeros((2, 5, 4), dtype=f) if which == 'metric' else torch.zeros((2, 4, 0), dtype=f)
    for name, bad in wrong.items():
        a = _args()
        a[name] = bad
        with pytest.raises(ValueError, match=name):
            _run(which, a)
    if which == 'metric':
        a = _args()
        a['p'] = torch.zeros((2, 4, 3), dtype=f)                         # p must be square
        with pytest.raises(ValueError, match='p must be'):
            _run(which, a)
    with pytest.raises(RuntimeError, match='must live on the GPU'):      # well-formed host tensors: there is no CPU path
        _run(which, _args())
