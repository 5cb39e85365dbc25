"""CPU tests (no GPU) of the joint-covariance operator's C ABI (include/dpgp.h, csrc/ard_rbf_point_cov.hip) and of the argument
checks of its ops front-end: the entry points are exported and bound, bad arguments come back with their negative codes in argument
order and before anything is launched (every device pointer here is a dummy: a launch would fault), the workspace query is 0 for a
shape out of range and holds nothing of size N M, and ops raises TypeError / ValueError / RuntimeError as documented."""
import ctypes
import os
import re

import pytest
import torch

from dp_gp_lvm_amd import _lib, ops

P = ctypes.c_void_p(16)          # non-NULL, never dereferenced: every call below returns before a launch
STEM = 'dpgp_ard_rbf_point_cov'
CASES = [('K', 0, -1), ('G', 0, -2), ('N', 0, -3), ('M', -1, -4), ('Q', 0, -5), ('z', None, -6), ('x', None, -7),
         ('gamma', None, -8), ('alpha', None, -9), ('c', None, -10), ('out', None, -11), ('ws', None, -12), ('ws_bytes', 7, -13)]
GOOD = dict(K=1, G=2, N=2, M=3, Q=2)


def call(**kw):
    a = dict(GOOD, z=P, x=P, gamma=P, alpha=P, c=P, out=P, ws=P, ws_bytes=1 << 20)
    a.update(kw)
    return getattr(_lib.lib(), STEM + '_f64')(*a.values(), None)


def test_entry_points_are_exported_bound_and_declared():
    lib = _lib.lib()
    for n in (STEM + '_workspace_bytes', STEM + '_f64'):
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES[STEM + '_workspace_bytes'][1]) == 5
    assert len(_lib.SIGNATURES[STEM + '_f64'][1]) == 5 + 6 + 3             # z, x, gamma, alpha, c, out; ws, ws_bytes, stream
    assert callable(ops.ard_rbf_point_cov)
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'dpgp.h')).read()
    decl = re.search(r'int %s_f64\(([^;]*)\);' % STEM, header)
    assert decl is not None and 'size_t %s_workspace_bytes(int K, int G, int N, int M, int Q);' % STEM in header
    names = [a.split()[-1].lstrip('*') for a in decl.group(1).replace('\n', ' ').split(',')]
    assert names == [name for name, _, _ in CASES] + ['stream']            # the header's argument order is the codes' order


def test_bad_arguments_come_back_with_their_codes_in_order():
    for name, bad, code in CASES:
        assert call(**{name: bad}) == code, name
    assert call(Q=65) == -5                                                # Q is the 5th argument
    assert call(N=46341) == -3 and call(N=46340, ws=None) == -12           # N N must fit 31 bits
    # with every argument bad at once the first check answers; repairing them one by one walks down the list
    bad = {name: value for name, value, _ in CASES}
    for name, _, code in CASES:
        assert call(**bad) == code, name
        if name != 'ws_bytes':
            bad[name] = GOOD.get(name, P)
    codes = [code for _, _, code in CASES]
    assert codes == list(range(-1, -len(codes) - 1, -1))


def test_workspace_query_holds_nothing_of_size_n_m_and_is_zero_out_of_range():
    query = _lib.lib().dpgp_ard_rbf_point_cov_workspace_bytes
    for shape in [(1, 1, 1, 1, 1), (3, 2, 130, 200, 21), (512, 1, 320, 128, 10), (8, 16, 500, 128, 10), (1, 1, 2000, 128, 10),
                  (1, 1, 46340, 128, 64)]:
        assert 0 < query(*shape) <= 256, shape                               # the results are written from registers
        assert call(ws_bytes=query(*shape) - 1) == -13
    for shape in [(0, 1, 2, 3, 2), (1, 0, 2, 3, 2), (1, 1, 0, 3, 2), (1, 1, 2, 0, 2), (1, 1, 2, 3, 0), (1, 1, 2, 3, 65),
                  (-1, 1, 2, 3, 2), (1, 1, -5, 3, 2), (1, 1, 46341, 3, 2)]:
        assert query(*shape) == 0, shape


def _args(k=2, g=2, n=5, m=4, q=3):
    f = torch.float64
    return dict(z=torch.zeros((k, m, q), dtype=f), x=torch.zeros((n, q), dtype=f), gamma=torch.ones((k, q), dtype=f),
                alpha=torch.ones(k, dtype=f), c=torch.zeros((k, g, m, m), dtype=f))


def _run(a):
    return ops.ard_rbf_point_cov(a['z'], a['x'], a['gamma'], a['alpha'], a['c'])


def test_ops_argument_errors():
    for name in ('z', 'x', 'gamma', 'alpha', 'c'):
        a = _args()
        a[name] = a[name].to(torch.float32)
        with pytest.raises(TypeError, match='%s must' % name):
            _run(a)
        a[name] = a[name].numpy()
        with pytest.raises(TypeError, match='%s must' % name):
            _run(a)
    f = torch.float64
    wrong = dict(z=torch.zeros((2, 4), dtype=f), x=torch.zeros((5, 4), dtype=f), gamma=torch.ones((2, 4), dtype=f),
                 alpha=torch.ones(3, dtype=f), c=torch.zeros((2, 4, 4), dtype=f))
    for name, bad in wrong.items():
        a = _args()
        a[name] = bad
        with pytest.raises(ValueError, match='%s must' % name):
            _run(a)
    for bad in (torch.zeros((2, 0, 4, 4), dtype=f), torch.zeros((2, 2, 4, 3), dtype=f), torch.zeros((3, 2, 4, 4), dtype=f)):
        with pytest.raises(ValueError, match='c must be .K x G x M x M. with G >= 1'):
            _run(dict(_args(), c=bad))
    with pytest.raises(RuntimeError, match='must live on the GPU'):          # well-formed host tensors: there is no CPU path
        _run(_args())
