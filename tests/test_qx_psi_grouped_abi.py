"""CPU tests (no GPU) of the pattern-grouped Psi operators' C ABI (include/dpgp.h, csrc/qx_psi.hip): the six entry points are
exported and bound, bad arguments come back with their negative codes in argument order and before anything is launched
(every device pointer here is a dummy: a launch would fault), zfac is nullable and w is not, the workspace queries are 0 for a
shape out of range and a workspace one byte short is refused."""
import ctypes

import pytest

from dp_gp_lvm_amd import _lib

P = ctypes.c_void_p(16)          # non-NULL, never dereferenced: every call below returns before a launch
COMMON = [('K', 0, -1), ('P', 0, -2), ('N', -1, -3), ('M', 0, -4), ('Q', 0, -5), ('z', None, -6), ('mu', None, -7), ('s', None, -8),
          ('gamma', None, -9), ('alpha', None, -10), ('w', None, -12)]
OPS = {
    'stats': ('dpgp_qx_psi_stats_grouped', ['psi1', 'psi2']),
    'adjoint': ('dpgp_qx_psi_adjoint_grouped', ['g1', 'g2', 'd_mu', 'd_s']),
    'param': ('dpgp_qx_psi_param_adjoint_grouped', ['g1', 'g2', 'd_z', 'd_gamma', 'd_alpha']),
}


def cases_of(op):
    """[(argument, bad value, code)] in the order of the checks."""
    tail = OPS[op][1] + ['ws']
    out = COMMON + [(name, None, -13 - i) for i, name in enumerate(tail)]
    return out + [('ws_bytes', 7, -13 - len(tail))]


def call(op, **kw):
    a = dict(K=1, P=2, N=2, M=3, Q=2, z=P, mu=P, s=P, gamma=P, alpha=P, zfac=None, w=P)
    a.update({name: P for name in OPS[op][1]})
    a.update(ws=P, ws_bytes=1 << 30)
    a.update(kw)
    return getattr(_lib.lib(), OPS[op][0] + '_f64')(*a.values(), None)


def query(op):
    return getattr(_lib.lib(), OPS[op][0] + '_workspace_bytes')


def test_entry_points_are_exported_and_bound():
    lib = _lib.lib()
    for stem, outs in OPS.values():
        for n in (stem + '_workspace_bytes', stem + '_f64'):
            assert n in _lib.SIGNATURES and hasattr(lib, n), n
        assert len(_lib.SIGNATURES[stem + '_workspace_bytes'][1]) == 5
        # K, P, N, M, Q; z, mu, s, gamma, alpha, zfac, w; the operator's own pointers; ws, ws_bytes, stream
        assert len(_lib.SIGNATURES[stem + '_f64'][1]) == 5 + 7 + len(outs) + 3


@pytest.mark.parametrize('op', list(OPS))
def test_bad_arguments_come_back_with_their_codes(op):
    for name, bad, code in cases_of(op):
        assert call(op, **{name: bad}) == code, name
        assert call(op, zfac=P, **{name: bad}) == code, name
    assert call(op, Q=65) == -5
    assert call(op, P=-3) == -2


@pytest.mark.parametrize('op', list(OPS))
def test_the_checks_are_made_in_the_order_of_the_codes(op):
    # with every argument bad at once the first check answers; repairing them one by one walks down the list
    cases = cases_of(op)
    bad = {name: value for name, value, _ in cases}
    good = dict(K=1, P=2, N=2, M=3, Q=2)
    for name, _, code in cases:
        assert call(op, **bad) == code, name
        if name != 'ws_bytes':
            bad[name] = good.get(name, P)
    codes = [code for _, _, code in cases]
    assert codes == sorted(codes, reverse=True) and len(set(codes)) == len(codes)


@pytest.mark.parametrize('op', list(OPS))
def test_null_zfac_passes_null_weights_do_not_and_a_short_workspace_is_refused(op):
    need = query(op)(1, 2, 2, 3, 2)
    short_code = cases_of(op)[-1][2]
    assert need > 0
    assert call(op, zfac=None, ws_bytes=need - 1) == short_code and call(op, zfac=P, ws_bytes=need - 1) == short_code
    assert call(op, w=None, ws_bytes=need - 1) == -12


@pytest.mark.parametrize('op', list(OPS))
def test_workspace_query(op):
    q = query(op)
    for shape in [(1, 1, 1, 1, 1), (1, 2, 2, 3, 2), (3, 5, 300, 200, 23), (8, 16, 2000, 128, 10), (1, 9, 7, 33, 64), (4, 60, 200, 50, 10)]:
        assert q(*shape) > 0, shape
    for shape in [(0, 1, 2, 3, 2), (1, 0, 2, 3, 2), (1, 1, 0, 3, 2), (1, 1, 2, 0, 2), (1, 1, 2, 3, 0), (1, 1, 2, 3, 65), (-1, 1, 2, 3, 2),
                  (1, -1, 2, 3, 2)]:
        assert q(*shape) == 0, shape
    # the partial sums of a larger problem need at least as much room
    assert q(4, 16, 500, 128, 10) >= q(1, 16, 500, 128, 10) and q(1, 16, 500, 128, 10) >= q(1, 1, 500, 128, 10)
