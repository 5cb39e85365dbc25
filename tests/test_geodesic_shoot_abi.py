"""CPU tests (no GPU) of the C ABI of the integrators on the device (include/dpgp.h, csrc/geodesic_accel.hip) and of the argument
checks of ops.geodesic_shoot / ops.geodesic_shoot_tangent: the entry points are exported, bound and declared in the order of their
codes; bad arguments come back with their negative codes in declaration order and before anything is launched (every device
pointer here is a dummy: a launch would fault); the limits on Q and on the number of parts; the workspace query holds the slabs
and a few states and nothing else, is 0 out of range, and a workspace one byte short has a code of its own; ops raises TypeError /
ValueError / RuntimeError as documented."""
import ctypes
import os
import re

import pytest
import torch

from dp_gp_lvm_amd import _lib, ops

P = ctypes.c_void_p(16)          # non-NULL, never dereferenced: every call below returns before a launch
MAX_PARTS = 64
QUERY = 'dpgp_geodesic_shoot_workspace_bytes'
PLAIN = 'dpgp_geodesic_shoot_f64'
TANGENT = 'dpgp_geodesic_shoot_tangent_f64'


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def ptrs(n, value=16):
    return (ctypes.c_void_p * n)(*([value] * n))


HEAD = [('parts', 0, -1), ('K', None, -2), ('M', None, -3), ('Q', 0, -4), ('C', 0, -5), ('S', 0, -6), ('z', None, -7),
        ('gamma', None, -8), ('alpha', None, -9), ('p', None, -10), ('prior', None, -11), ('x', None, -12), ('v', None, -13)]
PLAIN_CASES = HEAD + [('curve', None, -14), ('vel', None, -15), ('bad', None, -16), ('ws', None, -17), ('ws_bytes', 7, -18)]
TANGENT_CASES = HEAD + [('dx', None, -14), ('dv', None, -15), ('curve', None, -16), ('vel', None, -17), ('dcurve', None, -18),
                        ('dvel', None, -19), ('bad', None, -20), ('speed0', None, -21), ('ws', None, -22), ('ws_bytes', 7, -23)]


def good(cases):
    a = {name: P for name, _, _ in cases}
    a.update(parts=2, K=ints(1, 3), M=ints(3, 4), Q=2, C=5, S=2, z=ptrs(2), gamma=ptrs(2), alpha=ptrs(2), p=ptrs(2), ws_bytes=1 << 24)
    return a


def call(fn, cases, **kw):
    a = good(cases)
    a.update(kw)
    assert list(a) == [name for name, _, _ in cases]
    return getattr(_lib.lib(), fn)(*a.values(), None)


def _header_names(header, name):
    decl = re.search(r'(?:int|size_t) %s\(([^;]*)\);' % name, header)
    assert decl is not None, name
    return [a.split()[-1].lstrip('*') for a in decl.group(1).replace('\n', ' ').split(',')]


def test_entry_points_are_exported_bound_and_declared():
    lib = _lib.lib()
    for n in (QUERY, PLAIN, TANGENT):
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert len(_lib.SIGNATURES[QUERY][1]) == 6
    assert len(_lib.SIGNATURES[PLAIN][1]) == len(PLAIN_CASES) + 1 and len(_lib.SIGNATURES[TANGENT][1]) == len(TANGENT_CASES) + 1
    assert callable(ops.geodesic_shoot) and callable(ops.geodesic_shoot_tangent)
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'dpgp.h')).read()
    assert _header_names(header, QUERY) == ['parts', 'K', 'M', 'Q', 'C', 'tangent']
    assert _header_names(header, PLAIN) == [name for name, _, _ in PLAIN_CASES] + ['stream']            # the codes' order
    assert _header_names(header, TANGENT) == [name for name, _, _ in TANGENT_CASES] + ['stream']


@pytest.mark.parametrize('fn, cases', [(PLAIN, PLAIN_CASES), (TANGENT, TANGENT_CASES)], ids=['plain', 'tangent'])
def test_bad_arguments_come_back_with_their_codes_in_order(fn, cases):
    for name, bad, code in cases:
        assert call(fn, cases, **{name: bad}) == code, name
    # with every argument bad at once the first check answers; repairing them one by one walks down the list
    bad = {name: value for name, value, _ in cases}
    for name, _, code in cases:
        assert call(fn, cases, **bad) == code, name
        if name != 'ws_bytes':
            bad[name] = good(cases)[name]
    codes = [code for _, _, code in cases]
    assert codes == list(range(-1, -len(codes) - 1, -1))


@pytest.mark.parametrize('fn, cases', [(PLAIN, PLAIN_CASES), (TANGENT, TANGENT_CASES)], ids=['plain', 'tangent'])
def test_an_entry_of_a_list_is_checked_as_the_list(fn, cases):
    assert call(fn, cases, K=ints(1, 0)) == -2 and call(fn, cases, K=ints(-1, 3)) == -2
    assert call(fn, cases, M=ints(3, 0)) == -3
    for i, name in enumerate(('z', 'gamma', 'alpha', 'p')):
        hole = ptrs(2)
        hole[1] = None
        assert call(fn, cases, **{name: hole}) == -7 - i, name


def test_q_limits():
    short = dict(ws_bytes=0)
    assert call(PLAIN, PLAIN_CASES, Q=64) == -4 and call(PLAIN, PLAIN_CASES, Q=63, **short) == -18        # (63 passes the Q check)
    assert call(TANGENT, TANGENT_CASES, Q=32) == -4 and call(TANGENT, TANGENT_CASES, Q=63) == -4
    assert call(TANGENT, TANGENT_CASES, Q=31, **short) == -23


def test_the_cap_on_parts():
    many = dict(K=ints(*[1] * (MAX_PARTS + 1)), M=ints(*[2] * (MAX_PARTS + 1)), z=ptrs(MAX_PARTS + 1), gamma=ptrs(MAX_PARTS + 1),
                alpha=ptrs(MAX_PARTS + 1), p=ptrs(MAX_PARTS + 1))
    assert MAX_PARTS >= 32
    for fn, cases in ((PLAIN, PLAIN_CASES), (TANGENT, TANGENT_CASES)):
        assert call(fn, cases, parts=MAX_PARTS + 1, **many) == -1
        assert call(fn, cases, parts=MAX_PARTS, ws_bytes=0, **many) == cases[-1][2]                        # (the cap itself passes)
        assert call(fn, cases, parts=-1) == -1
    query = getattr(_lib.lib(), QUERY)
    assert query(MAX_PARTS, many['K'], many['M'], 3, 5, 0) > 0 and query(MAX_PARTS + 1, many['K'], many['M'], 3, 5, 0) == 0


def test_workspace_query_and_a_workspace_one_byte_short():
    query = getattr(_lib.lib(), QUERY)
    for ks, ms, q, c in [((1,), (1,), 1, 1), ((1, 3), (3, 4), 2, 5), ((60,), (50,), 10, 10), ((8,), (128,), 10, 100), ((3, 5), (9, 20), 31, 7)]:
        k, m = ints(*ks), ints(*ms)
        slabs = sum(ks) * c * (q * q + q) * 8
        for tangent, fn, cases in ((0, PLAIN, PLAIN_CASES), (1, TANGENT, TANGENT_CASES)):
            need = query(len(ks), k, m, q, c, tangent)
            states = (12 if tangent else 6) * c * q * 8                  # two argument buffers and the sums of x, v[, dx, dv]
            assert (1 + tangent) * slabs + states <= need <= (1 + tangent) * slabs + states + 256 * 8      # (plus a token and alignment)
            kw = dict(parts=len(ks), K=k, M=m, Q=q, C=c, z=ptrs(len(ks)), gamma=ptrs(len(ks)), alpha=ptrs(len(ks)), p=ptrs(len(ks)))
            assert call(fn, cases, ws_bytes=need - 1, **kw) == cases[-1][2]
    k, m = ints(1, 3), ints(3, 4)
    for args in [(0, k, m, 2, 5, 0), (2, None, m, 2, 5, 0), (2, k, None, 2, 5, 0), (2, k, m, 0, 5, 0), (2, k, m, 2, 0, 0), (2, k, m, 64, 5, 0),
                 (2, k, m, 32, 5, 1), (2, ints(1, 0), m, 2, 5, 0), (2, k, ints(0, 4), 2, 5, 1), (2, k, m, 2, -3, 1)]:
        assert query(*args) == 0, args
    assert query(2, k, m, 63, 5, 0) > 0 and query(2, k, m, 31, 5, 1) > 0


def _args(k=2, c=5, m=4, q=3, parts=2):
    f = torch.float64
    part = lambda: [torch.zeros((k, m, q), dtype=f), torch.ones((k, q), dtype=f), torch.ones(k, dtype=f), torch.zeros((k, m, m), dtype=f)]
    return dict(parts=[part() for _ in range(parts)], prior=torch.ones(q, dtype=f), x=torch.zeros((c, q), dtype=f),
                v=torch.zeros((c, q), dtype=f), dx=torch.zeros((c, q), dtype=f), dv=torch.zeros((c, q), dtype=f))


def _run(a, tangent, num_steps=2):
    if tangent:
        return ops.geodesic_shoot_tangent(a['parts'], a['prior'], a['x'], a['v'], a['dx'], a['dv'], num_steps)
    return ops.geodesic_shoot(a['parts'], a['prior'], a['x'], a['v'], num_steps)


@pytest.mark.parametrize('tangent', [False, True], ids=['plain', 'tangent'])
def test_ops_argument_errors(tangent):
    states = ('x', 'v', 'dx', 'dv') if tangent else ('x', 'v')
    for name in states + ('prior',):
        a = _args()
        a[name] = a[name].to(torch.float32)
        with pytest.raises(TypeError, match='^%s must' % name):
            _run(a, tangent)
        a[name] = a[name].numpy()
        with pytest.raises(TypeError, match='^%s must' % name):
            _run(a, tangent)
    for j, name in enumerate(('z', 'gamma', 'alpha', 'p')):
        a = _args()
        a['parts'][1][j] = a['parts'][1][j].to(torch.float32)
        with pytest.raises(TypeError, match='^%s must' % name):
            _run(a, tangent)
    for bad in (None, [], [(1, 2, 3)], torch.zeros(3)):
        a = _args()
        a['parts'] = bad
        with pytest.raises(TypeError, match='^parts must'):
            _run(a, tangent)
    f = torch.float64
    wrong = dict(x=torch.zeros((5, 4), dtype=f), v=torch.zeros((4, 3), dtype=f), dx=torch.zeros((5, 2), dtype=f),
                 dv=torch.zeros((5,), dtype=f), prior=torch.ones(4, dtype=f))
    for name in states + ('prior',):
        a = _args()
        a[name] = wrong[name]
        with pytest.raises(ValueError, match='^%s must' % name):
            _run(a, tangent)
    wrong = [torch.zeros((2, 4), dtype=f), torch.ones((2, 4), dtype=f), torch.ones(3, dtype=f), torch.zeros((2, 4, 3), dtype=f)]
    for j, name in enumerate(('z', 'gamma', 'alpha', 'p')):
        a = _args()
        a['parts'][1][j] = wrong[j]
        with pytest.raises(ValueError, match='^%s must' % name):
            _run(a, tangent)
    with pytest.raises(ValueError, match='^parts must have at most 64'):
        _run(_args(parts=MAX_PARTS + 1), tangent)
    limit = 31 if tangent else 63
    with pytest.raises(ValueError, match='Q <= %d' % limit):
        _run(_args(q=limit + 1), tangent)
    for steps in (0, -2):
        with pytest.raises(ValueError, match='^num_steps must'):
            _run(_args(), tangent, steps)
    with pytest.raises(RuntimeError, match='must live on the GPU'):          # well-formed host tensors: there is no CPU path
        _run(_args(q=limit), tangent)
