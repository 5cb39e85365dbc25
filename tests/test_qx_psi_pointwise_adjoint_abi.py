"""CPU tests (no GPU) of the C ABI of the per-point contractions' latent adjoint (include/dpgp.h, csrc/qx_psi_point_adjoint.hip): the
two entry points are exported and bound, bad arguments come back with their negative codes in argument order and before anything
is launched (every device pointer here is a dummy: a launch would fault), zfac is nullable, the workspace query is 0 for a shape
out of range and a workspace one byte short is refused."""
import ctypes

from dp_gp_lvm_amd import _lib

P = ctypes.c_void_p(16)          # non-NULL, never dereferenced: every call below returns before a launch
STEM = 'dpgp_qx_psi_pointwise_adjoint'
CASES = [('K', 0, -1), ('G', 0, -2), ('J', -1, -3), ('N', 0, -4), ('M', 0, -5), ('Q', 0, -6), ('z', None, -7), ('mu', None, -8),
         ('s', None, -9), ('gamma', None, -10), ('alpha', None, -11), ('c', None, -13), ('r', None, -14), ('h', None, -15),
         ('gq', None, -16), ('gt', None, -17), ('d_mu', None, -18), ('d_s', None, -19), ('ws', None, -20), ('ws_bytes', 7, -21)]
GOOD = dict(K=1, G=2, J=3, N=2, M=3, Q=2)


def call(**kw):
    a = dict(GOOD, z=P, mu=P, s=P, gamma=P, alpha=P, zfac=None, c=P, r=P, h=P, gq=P, gt=P, d_mu=P, d_s=P, ws=P, ws_bytes=1 << 30)
    a.update(kw)
    return getattr(_lib.lib(), STEM + '_f64')(*a.values(), None)


def query(*shape):
    return getattr(_lib.lib(), STEM + '_workspace_bytes')(*shape)


def test_entry_points_are_exported_and_bound():
    lib = _lib.lib()
    for n in (STEM + '_workspace_bytes', STEM + '_f64'):
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES[STEM + '_workspace_bytes'][1]) == 6
    # K, G, J, N, M, Q; z, mu, s, gamma, alpha, zfac, c, r, h, gq, gt, d_mu, d_s; ws, ws_bytes, stream
    assert len(_lib.SIGNATURES[STEM + '_f64'][1]) == 6 + 13 + 3
    from dp_gp_lvm_amd import ops
    assert callable(ops.qx_psi_pointwise_adjoint) and callable(ops.qx_psi_point_moments_adjoint)


def test_bad_arguments_come_back_with_their_codes():
    for name, bad, code in CASES:
        assert call(**{name: bad}) == code, name
        assert call(zfac=P, **{name: bad}) == code, name
    assert call(Q=65) == -6
    assert call(G=-3) == -2
    assert -12 not in [code for _, _, code in CASES]             # zfac is nullable: its place has no code


def test_the_checks_are_made_in_the_order_of_the_codes():
    # with every argument bad at once the first check answers; repairing them one by one walks down the list
    bad = {name: value for name, value, _ in CASES}
    for name, _, code in CASES:
        assert call(**bad) == code, name
        if name != 'ws_bytes':
            bad[name] = GOOD.get(name, P)
    codes = [code for _, _, code in CASES]
    assert codes == sorted(codes, reverse=True) and len(set(codes)) == len(codes)


def test_null_zfac_passes_and_a_short_workspace_is_refused():
    need = query(*GOOD.values())
    assert need > 0
    assert call(zfac=None, ws_bytes=need - 1) == -21 and call(zfac=P, ws_bytes=need - 1) == -21
    # (ws_bytes == need would launch on the dummy pointers: not tried without a GPU)


def test_workspace_query():
    #             K, G,  J,   N,   M,  Q
    for shape in [(1, 1, 1, 1, 1, 1), (1, 2, 3, 2, 3, 2), (3, 2, 40, 130, 65, 17), (8, 16, 512, 500, 128, 10), (1, 2, 15, 70, 40, 64),
                  (1, 1, 5, 33, 200, 10), (512, 1, 1, 500, 128, 10)]:
        n, q = shape[3], shape[5]
        need = query(*shape)
        # partial (d_mu, d_s) and nothing else: a whole number of [2][N][Q] slabs; nothing of size K N M or N M M is asked for
        assert need > 0 and need % (8 * 2 * n * q) == 0, shape
        assert need <= 8 * 2 * n * q * 1024, shape
    for shape in [(0, 1, 1, 2, 3, 2), (1, 0, 1, 2, 3, 2), (1, 1, 0, 2, 3, 2), (1, 1, 1, 0, 3, 2), (1, 1, 1, 2, 0, 2), (1, 1, 1, 2, 3, 0),
                  (1, 1, 1, 2, 3, 65), (-1, 1, 1, 2, 3, 2), (1, 1, -1, 2, 3, 2)]:
        assert query(*shape) == 0, shape
    # few points: the pair tiles are split over slabs; many points and one kernel: one slab per column chunk
    assert query(1, 1, 5, 33, 200, 10) > 8 * 2 * 33 * 10 and query(1, 1, 1, 50000, 128, 10) == 8 * 2 * 50000 * 10
