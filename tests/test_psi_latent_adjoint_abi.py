"""CPU tests (no GPU) of the shared-inducing latent adjoint's C ABI (include/dpgp.h, csrc/psi_latent_adjoint.hip): the two entry
points are exported and bound, bad arguments come back with their negative codes in argument order and before anything is
launched (every device pointer here is a dummy: a launch would fault), w is nullable, the workspace query is 0 for a shape out of
range and a workspace one byte short is refused."""
import ctypes

from dp_gp_lvm_amd import _lib

P = ctypes.c_void_p(16)          # non-NULL, never dereferenced: every call below returns before a launch
STEM = 'dpgp_psi_latent_adjoint'
CASES = [('B', 0, -1), ('N', 0, -2), ('M', -1, -3), ('Q', 0, -4), ('z', None, -5), ('mu', None, -6), ('s', None, -7),
         ('gamma', None, -8), ('alpha', None, -9), ('y', None, -10), ('ldy', 2, -11), ('g_v', None, -13), ('g_psi2', None, -14),
         ('d_mu', None, -15), ('d_s', None, -16), ('ws', None, -17), ('ws_bytes', 7, -18)]
GOOD = dict(B=3, N=2, M=3, Q=2)


def call(**kw):
    a = dict(GOOD, z=P, mu=P, s=P, gamma=P, alpha=P, y=P, ldy=3, w=None, g_v=P, g_psi2=P, d_mu=P, d_s=P, ws=P, ws_bytes=1 << 30)
    a.update(kw)
    return getattr(_lib.lib(), STEM + '_f64')(*a.values(), None)


def query(*shape):
    return getattr(_lib.lib(), STEM + '_workspace_bytes')(*shape)


def test_entry_points_are_exported_and_bound():
    lib = _lib.lib()
    for n in (STEM + '_workspace_bytes', STEM + '_f64'):
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES[STEM + '_workspace_bytes'][1]) == 4
    # B, N, M, Q; z, mu, s, gamma, alpha, y; ldy; w, g_v, g_psi2, d_mu, d_s; ws, ws_bytes, stream
    args = _lib.SIGNATURES[STEM + '_f64'][1]
    assert len(args) == 4 + 6 + 1 + 5 + 3 and args[10] is ctypes.c_int and args[-2] is ctypes.c_size_t


def test_bad_arguments_come_back_with_their_codes():
    for name, bad, code in CASES:
        assert call(**{name: bad}) == code, name
        assert call(w=P, **{name: bad}) == code, name
    assert call(Q=65) == -4 and call(Q=64, ws_bytes=7) == -18
    assert call(B=-3) == -1
    assert call(ldy=2) == -11 and call(ldy=0) == -11 and call(ldy=3, ws_bytes=7) == -18 and call(ldy=40, ws_bytes=7) == -18
    assert -12 not in [code for _, _, code in CASES]             # w is nullable: its place has no code


def test_the_checks_are_made_in_the_order_of_the_codes():
    # with every argument bad at once the first check answers; repairing them one by one walks down the list
    for w in (None, P):
        bad = {name: value for name, value, _ in CASES}
        for name, _, code in CASES:
            assert call(w=w, **bad) == code, name
            if name != 'ws_bytes':
                bad[name] = GOOD.get(name, 3 if name == 'ldy' else P)
    codes = [code for _, _, code in CASES]
    assert codes == sorted(codes, reverse=True) and len(set(codes)) == len(codes)


def test_null_weights_pass_and_a_short_workspace_is_refused():
    need = query(*GOOD.values())
    assert need > 0
    assert call(w=None, ws_bytes=need - 1) == -18 and call(w=P, ws_bytes=need - 1) == -18
    # (ws_bytes == need would launch on the dummy pointers: not tried without a GPU)


def test_workspace_query(monkeypatch):
    #             B,  N,   M,  Q
    for shape in [(1, 1, 1, 1), (3, 2, 3, 2), (17, 129, 130, 23), (512, 500, 128, 10), (3, 5, 17, 64), (60, 100, 50, 10)]:
        b, n, m, q = shape
        need = query(*shape)
        # partial sums of the two outputs and nothing else: a whole number of [2][N][Q] slabs
        assert need > 0 and need % (8 * 2 * n * q) == 0, shape
    for shape in [(0, 2, 3, 2), (3, 0, 3, 2), (3, 2, 0, 2), (3, 2, 3, 0), (3, 2, 3, 65), (-1, 2, 3, 2), (3, -2, 3, 2)]:
        assert query(*shape) == 0, shape
    # the forced plan (tests of the slab boundaries): one slab of columns and one of pair tiles = one slab; Q = 64 has two chunks
    monkeypatch.setenv('DPGP_PLA_COL_SLABS', '1')
    monkeypatch.setenv('DPGP_PLA_PAIR_SLABS', '1')
    assert query(17, 33, 65, 10) == 8 * 2 * 33 * 10 and query(3, 5, 17, 64) == 2 * 8 * 2 * 5 * 64
    monkeypatch.setenv('DPGP_PLA_COL_SLABS', '3')
    monkeypatch.setenv('DPGP_PLA_PAIR_SLABS', '2')
    assert query(17, 33, 65, 10) == 3 * 2 * 8 * 2 * 33 * 10
