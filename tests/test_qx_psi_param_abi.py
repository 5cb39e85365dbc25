"""CPU tests (no GPU) of the parameter adjoint of the weighted test-point Psi statistics' C ABI (include/dpgp.h,
csrc/qx_psi.hip): the two entry points are exported and bound, bad arguments come back with the negative codes of
dpgp_qx_psi_adjoint_weighted_f64 (-1 .. -12) and then -13 .. -17, in order and before anything is launched (every device
pointer here is a dummy: a launch would fault), and the workspace query is 0 for a shape out of range."""
import ctypes

import pytest

from dp_gp_lvm_amd import _lib

NAMES = ['dpgp_qx_psi_param_adjoint_workspace_bytes', 'dpgp_qx_psi_param_adjoint_weighted_f64']
P = ctypes.c_void_p(16)          # non-NULL, never dereferenced: every call below returns before a launch

CASES = [(dict(B=0), -1), (dict(N=-1), -2), (dict(M=0), -3), (dict(Q=0), -4), (dict(Q=65), -4), (dict(z=None), -5),
         (dict(mu=None), -6), (dict(s=None), -7), (dict(gamma=None), -8), (dict(alpha=None), -9), (dict(g1=None), -11),
         (dict(g2=None), -12), (dict(d_z=None), -13), (dict(d_gamma=None), -14), (dict(d_alpha=None), -15), (dict(ws=None), -16),
         (dict(ws_bytes=7), -17)]


def _param(**kw):
    a = dict(B=1, N=2, M=3, Q=2, z=P, mu=P, s=P, gamma=P, alpha=P, zfac=None, w=P, g1=P, g2=P, d_z=P, d_gamma=P, d_alpha=P, ws=P,
             ws_bytes=1 << 30)
    a.update(kw)
    return _lib.lib().dpgp_qx_psi_param_adjoint_weighted_f64(*a.values(), None)


def test_entry_points_are_exported_and_bound():
    lib = _lib.lib()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    # one more output pointer than the (mu, s) adjoint: (d_z, d_gamma, d_alpha) instead of (d_mu, d_s)
    assert len(_lib.SIGNATURES[NAMES[1]][1]) == len(_lib.SIGNATURES['dpgp_qx_psi_adjoint_weighted_f64'][1]) + 1


@pytest.mark.parametrize('w', [P, None])
@pytest.mark.parametrize('kw,code', CASES)
def test_bad_arguments_come_back_in_order(kw, code, w):
    assert _param(w=w, **kw) == code


@pytest.mark.parametrize('w', [P, None])
def test_the_checks_are_made_in_the_order_of_the_codes(w):
    # with every argument bad at once the first check answers; repairing them one by one walks down the list
    bad = {}
    for kw, _ in CASES:
        bad.update(kw)
    bad['Q'] = 0
    order = ['B', 'N', 'M', 'Q', 'z', 'mu', 's', 'gamma', 'alpha', 'g1', 'g2', 'd_z', 'd_gamma', 'd_alpha', 'ws', 'ws_bytes']
    codes = [-1, -2, -3, -4, -5, -6, -7, -8, -9, -11, -12, -13, -14, -15, -16, -17]
    good = dict(B=1, N=2, M=3, Q=2, z=P, mu=P, s=P, gamma=P, alpha=P, g1=P, g2=P, d_z=P, d_gamma=P, d_alpha=P, ws=P)
    for name, code in zip(order, codes):
        assert _param(w=w, **bad) == code, name
        if name != 'ws_bytes':
            bad[name] = good[name]


def test_null_weights_and_null_zfac_pass_every_pointer_check():
    short = _lib.lib().dpgp_qx_psi_param_adjoint_workspace_bytes(1, 2, 3, 2) - 1
    assert _param(w=None, ws_bytes=short) == -17 and _param(w=P, zfac=P, ws_bytes=short) == -17


def test_workspace_query():
    q = _lib.lib().dpgp_qx_psi_param_adjoint_workspace_bytes
    for shape in [(1, 1, 1, 1), (1, 2, 3, 2), (5, 300, 200, 23), (16, 2000, 128, 10), (1, 7, 33, 64)]:
        assert q(*shape) > 0, shape
    for shape in [(0, 2, 3, 2), (1, 0, 3, 2), (1, 2, 0, 2), (1, 2, 3, 0), (1, 2, 3, 65), (-1, 2, 3, 2)]:
        assert q(*shape) == 0, shape
    # the partial sums of a larger problem need at least as much room
    assert q(4, 500, 128, 10) >= q(1, 500, 128, 10)
