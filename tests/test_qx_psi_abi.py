"""CPU tests (no GPU) of the two test-point Psi operators' C ABI (include/dpgp.h, csrc/qx_psi.hip): both entry points are
exported, their workspace queries are host-only functions, and bad arguments are refused with their negative codes before
anything is launched (every device pointer here is a dummy: a launch would fault)."""
import ctypes

import pytest

from dp_gp_lvm_amd import _lib

NAMES = ['dpgp_qx_psi_stats_workspace_bytes', 'dpgp_qx_psi_stats_batched_f64', 'dpgp_qx_psi_adjoint_workspace_bytes',
         'dpgp_qx_psi_adjoint_f64']
P = ctypes.c_void_p(16)          # non-NULL, never dereferenced: every call below returns before a launch


def test_entry_points_are_exported_and_bound():
    lib = _lib.lib()
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.SIGNATURES


def test_workspace_queries_are_host_only():
    lib = _lib.lib()
    assert lib.dpgp_qx_psi_stats_workspace_bytes(1, 1, 1, 1) >= 8
    assert lib.dpgp_qx_psi_adjoint_workspace_bytes(1, 1, 1, 1) >= 16
    big = lib.dpgp_qx_psi_adjoint_workspace_bytes(5, 300, 200, 23)
    assert big >= 8 * 2 * 23 * 300 * 5 and big % 8 == 0
    assert lib.dpgp_qx_psi_stats_workspace_bytes(5, 300, 200, 23) >= 8 * 5 * 200 * 200
    for args in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 65)):
        assert lib.dpgp_qx_psi_stats_workspace_bytes(*args) == 0
        assert lib.dpgp_qx_psi_adjoint_workspace_bytes(*args) == 0
    assert lib.dpgp_qx_psi_adjoint_workspace_bytes(1, 1, 1, 64) > 0


def _stats(**kw):
    a = dict(B=1, N=2, M=3, Q=2, z=P, mu=P, s=P, gamma=P, alpha=P, zfac=None, psi1=P, psi2=P, ws=P, ws_bytes=1 << 30)
    a.update(kw)
    return _lib.lib().dpgp_qx_psi_stats_batched_f64(*a.values(), None)


def _adjoint(**kw):
    a = dict(B=1, N=2, M=3, Q=2, z=P, mu=P, s=P, gamma=P, alpha=P, zfac=None, g1=P, g2=P, d_mu=P, d_s=P, ws=P, ws_bytes=1 << 30)
    a.update(kw)
    return _lib.lib().dpgp_qx_psi_adjoint_f64(*a.values(), None)


@pytest.mark.parametrize('kw,code', [(dict(B=0), -1), (dict(N=0), -2), (dict(M=0), -3), (dict(Q=0), -4), (dict(Q=65), -4),
                                     (dict(z=None), -5), (dict(mu=None), -6), (dict(s=None), -7), (dict(gamma=None), -8),
                                     (dict(alpha=None), -9), (dict(psi1=None), -11), (dict(psi2=None), -12),
                                     (dict(ws=None), -13), (dict(ws_bytes=0), -14)])
def test_stats_bad_arguments(kw, code):
    assert _stats(**kw) == code


@pytest.mark.parametrize('kw,code', [(dict(B=0), -1), (dict(N=-1), -2), (dict(M=0), -3), (dict(Q=0), -4), (dict(Q=65), -4),
                                     (dict(z=None), -5), (dict(mu=None), -6), (dict(s=None), -7), (dict(gamma=None), -8),
                                     (dict(alpha=None), -9), (dict(g1=None), -11), (dict(g2=None), -12),
                                     (dict(d_mu=None), -13), (dict(d_s=None), -14), (dict(ws=None), -15),
                                     (dict(ws_bytes=7), -16)])
def test_adjoint_bad_arguments(kw, code):
    assert _adjoint(**kw) == code
