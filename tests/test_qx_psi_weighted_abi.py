"""CPU tests (no GPU) of the weighted test-point Psi operators' C ABI (include/dpgp.h, csrc/qx_psi.hip): both entry points are
exported and bound, and they refuse bad arguments with the negative codes of the unweighted functions, in the same order, before
anything is launched (every device pointer here is a dummy: a launch would fault).  The weight pointer is nullable."""
import ctypes

import pytest

from dp_gp_lvm_amd import _lib
from test_qx_psi_abi import _adjoint, _stats

NAMES = ['dpgp_qx_psi_stats_weighted_f64', 'dpgp_qx_psi_adjoint_weighted_f64']
P = ctypes.c_void_p(16)          # non-NULL, never dereferenced: every call below returns before a launch

STATS_CASES = [(dict(B=0), -1), (dict(N=0), -2), (dict(M=0), -3), (dict(Q=0), -4), (dict(Q=65), -4), (dict(z=None), -5),
               (dict(mu=None), -6), (dict(s=None), -7), (dict(gamma=None), -8), (dict(alpha=None), -9), (dict(psi1=None), -11),
               (dict(psi2=None), -12), (dict(ws=None), -13), (dict(ws_bytes=0), -14)]
ADJOINT_CASES = [(dict(B=0), -1), (dict(N=-1), -2), (dict(M=0), -3), (dict(Q=0), -4), (dict(Q=65), -4), (dict(z=None), -5),
                 (dict(mu=None), -6), (dict(s=None), -7), (dict(gamma=None), -8), (dict(alpha=None), -9), (dict(g1=None), -11),
                 (dict(g2=None), -12), (dict(d_mu=None), -13), (dict(d_s=None), -14), (dict(ws=None), -15),
                 (dict(ws_bytes=7), -16)]


def test_entry_points_are_exported_and_bound():
    lib = _lib.lib()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    # one more pointer (the weights, right after zfac) than the unweighted signatures
    for new, old in zip(NAMES, ['dpgp_qx_psi_stats_batched_f64', 'dpgp_qx_psi_adjoint_f64']):
        assert len(_lib.SIGNATURES[new][1]) == len(_lib.SIGNATURES[old][1]) + 1


def _stats_w(**kw):
    a = dict(B=1, N=2, M=3, Q=2, z=P, mu=P, s=P, gamma=P, alpha=P, zfac=None, w=P, psi1=P, psi2=P, ws=P, ws_bytes=1 << 30)
    a.update(kw)
    return _lib.lib().dpgp_qx_psi_stats_weighted_f64(*a.values(), None)


def _adjoint_w(**kw):
    a = dict(B=1, N=2, M=3, Q=2, z=P, mu=P, s=P, gamma=P, alpha=P, zfac=None, w=P, g1=P, g2=P, d_mu=P, d_s=P, ws=P,
             ws_bytes=1 << 30)
    a.update(kw)
    return _lib.lib().dpgp_qx_psi_adjoint_weighted_f64(*a.values(), None)


@pytest.mark.parametrize('w', [P, None])
@pytest.mark.parametrize('kw,code', STATS_CASES)
def test_stats_bad_arguments_have_the_unweighted_codes(kw, code, w):
    assert _stats_w(w=w, **kw) == code == _stats(**kw)


@pytest.mark.parametrize('w', [P, None])
@pytest.mark.parametrize('kw,code', ADJOINT_CASES)
def test_adjoint_bad_arguments_have_the_unweighted_codes(kw, code, w):
    assert _adjoint_w(w=w, **kw) == code == _adjoint(**kw)


def test_null_weights_and_null_zfac_pass_every_pointer_check():
    # with w = NULL and zfac = NULL every argument check passes up to the workspace size: the last one made
    lib = _lib.lib()
    short = lib.dpgp_qx_psi_stats_workspace_bytes(1, 2, 3, 2) - 1
    assert _stats_w(w=None, ws_bytes=short) == -14 and _stats_w(w=P, zfac=P, ws_bytes=short) == -14
    short = lib.dpgp_qx_psi_adjoint_workspace_bytes(1, 2, 3, 2) - 1
    assert _adjoint_w(w=None, ws_bytes=short) == -16 and _adjoint_w(w=P, zfac=P, ws_bytes=short) == -16
