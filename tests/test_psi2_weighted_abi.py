"""CPU tests (no GPU) of the two weighted fp64 Psi2 entry points' C ABI (include/dpgp.h: dpgp_psi2_weighted_f64, csrc/psi2.hip;
dpgp_elbo_grad_psi_weighted_f64, csrc/elbo.hip): both are exported and bound, and for every defect they return the code the
unweighted function returns for it — with the weights NULL and non-NULL — before anything is launched (every device pointer
here is a dummy: a launch would fault)."""
import ctypes

import pytest

from dp_gp_lvm_amd import _lib

P = ctypes.c_void_p(16)          # non-NULL, never dereferenced: every call below returns before a launch
F64 = _lib.PREC['f64']


def test_entry_points_are_exported_and_bound():
    lib = _lib.lib()
    for n in ('dpgp_psi2_weighted_f64', 'dpgp_elbo_grad_psi_weighted_f64'):
        assert hasattr(lib, n) and n in _lib.SIGNATURES


def _psi2_args(**kw):
    a = dict(B=2, N=5, M=3, Q=2, z=P, mu=P, s=P, gamma=P, alpha=P, out=P, ws=P, ws_bytes=1 << 30, algo=0)
    a.update(kw)
    return a


def _psi2(w, **kw):
    a = _psi2_args(**kw)
    v = list(a.values())
    return _lib.lib().dpgp_psi2_weighted_f64(*v[:9], w, *v[9:], None)


def _psi2_unweighted(**kw):
    return _lib.lib().dpgp_psi2_f64(*_psi2_args(**kw).values(), None)


PSI2_DEFECTS = [(dict(B=0), -1), (dict(N=0), -2), (dict(M=0), -3), (dict(Q=0), -4), (dict(Q=65), -4), (dict(z=None), -5),
                (dict(mu=None), -6), (dict(s=None), -7), (dict(gamma=None), -8), (dict(alpha=None), -9), (dict(out=None), -10),
                (dict(ws=None), -11), (dict(ws_bytes=0), -12), (dict(algo=-1), -13), (dict(algo=99), -13)]


@pytest.mark.parametrize('w', [None, P], ids=['w_null', 'w_given'])
@pytest.mark.parametrize('kw,code', PSI2_DEFECTS)
def test_psi2_weighted_bad_arguments(kw, code, w):
    assert _psi2_unweighted(**kw) == code
    assert _psi2(w, **kw) == code


@pytest.mark.parametrize('w', [None, P], ids=['w_null', 'w_given'])
@pytest.mark.parametrize('algo', ['mfma_f32', 'patch_f16'])
def test_psi2_weighted_takes_auto_and_plain_only(algo, w):
    """The other algorithms of dpgp_psi2_f64 are refused with its code for an unknown one."""
    assert _psi2(w, algo=_lib.ALGO[algo]) == _psi2_unweighted(algo=99) == -13


def test_psi2_weighted_argument_order_is_that_of_the_unweighted_function():
    """Two defects at once: the earlier one is reported."""
    for w in (None, P):
        assert _psi2(w, s=None, ws=None) == _psi2_unweighted(s=None, ws=None) == -7
        assert _psi2(w, ws_bytes=0, algo=99) == _psi2_unweighted(ws_bytes=0, algo=99) == -12


def _grad_args(**kw):
    a = dict(D=2, N=5, M=3, Q=2, y=P, ldy=2, z=P, mu=P, s=P, gamma=P, alpha=P, g_psi2=P, w_kuu=P, g_v=P, ws=P,
             ws_bytes=1 << 30, d_mu=P, d_s=P, d_z=P, d_gamma=P)
    a.update(kw)
    return a


def _grad(w, **kw):
    v = list(_grad_args(**kw).values())
    return _lib.lib().dpgp_elbo_grad_psi_weighted_f64(*v[:11], w, *v[11:], None)


def _grad_unweighted(**kw):
    v = list(_grad_args(**kw).values())
    return _lib.lib().dpgp_elbo_grad_psi(*v[:14], F64, *v[14:], None)


GRAD_DEFECTS = [(dict(D=0), -1), (dict(N=0), -2), (dict(M=0), -3), (dict(Q=0), -4), (dict(Q=65), -4), (dict(y=None), -5),
                (dict(ldy=1), -6), (dict(z=None), -7), (dict(mu=None), -8), (dict(s=None), -9), (dict(gamma=None), -10),
                (dict(alpha=None), -11), (dict(g_psi2=None), -12), (dict(w_kuu=None), -13), (dict(g_v=None), -14),
                (dict(ws=None), -16), (dict(ws_bytes=8), -17), (dict(d_mu=None), -18), (dict(d_s=None), -19),
                (dict(d_z=None), -20), (dict(d_gamma=None), -21), (dict(M=129), -30), (dict(M=200), -30)]


@pytest.mark.parametrize('w', [None, P], ids=['w_null', 'w_given'])
@pytest.mark.parametrize('kw,code', GRAD_DEFECTS)
def test_grad_psi_weighted_bad_arguments(kw, code, w):
    assert _grad_unweighted(**kw) == code
    assert _grad(w, **kw) == code


def test_grad_psi_weighted_argument_order_is_that_of_the_unweighted_function():
    for w in (None, P):
        assert _grad(w, mu=None, d_z=None) == _grad_unweighted(mu=None, d_z=None) == -8
        assert _grad(w, ws=None, M=200) == _grad_unweighted(ws=None, M=200) == -16


def test_workspace_sizes_are_those_of_the_unweighted_functions():
    """ws_bytes one short of the unweighted function's query is refused, the query itself is not the defect reported next."""
    lib = _lib.lib()
    need = lib.dpgp_psi2_workspace_bytes(2, 5, 3, 2, 8)
    for w in (None, P):
        assert _psi2(w, ws_bytes=need - 1) == -12
        assert _psi2(w, ws_bytes=need, algo=99) == -13
    need = lib.dpgp_elbo_grad_psi_workspace_bytes_ex(2, 5, 3, 2, F64)
    for w in (None, P):
        assert _grad(w, ws_bytes=need - 1) == -17
        assert _grad(w, ws_bytes=need, d_mu=None) == -18
