"""CPU tests (no GPU) of the batched gram-gradient contraction's C ABI (include/dpgp.h, csrc/gram_grad.hip): the two entry
points are exported and bound, every bad argument comes back with its negative index in declaration order and before
anything is launched (every device pointer here is a dummy: a launch would fault), B == 0 / N == 0 return 0 with null
pointers, and the workspace query follows the slab plan (the 512-workgroup target divided by B) and is 0 out of range."""
import ctypes

import pytest

from dp_gp_lvm_amd import _lib

NAMES = ['dpgp_ard_rbf_gram_grad_batched_workspace_bytes', 'dpgp_ard_rbf_gram_grad_batched_f64']
P = ctypes.c_void_p(16)          # non-NULL, never dereferenced: every call below returns before a launch
ORDER = ['B', 'N', 'Q', 'x', 'gamma', 'alpha', 'w', 'ldw', 'w_stride', 'r', 'sx', 'sq', 'ws', 'ws_bytes']
GOOD = dict(B=3, N=70, Q=5, x=P, gamma=P, alpha=P, w=P, ldw=70, w_stride=70 * 70, r=P, sx=P, sq=P, ws=P, ws_bytes=1 << 30)
BAD = dict(B=-1, N=-1, Q=0, x=None, gamma=None, alpha=None, w=None, ldw=69, w_stride=70 * 70 - 1, r=None, sx=None, sq=None,
           ws=None, ws_bytes=7)


def _call(**kw):
    a = dict(GOOD)
    a.update(kw)
    assert list(a) == ORDER
    return _lib.lib().dpgp_ard_rbf_gram_grad_batched_f64(*a.values(), None)


def test_entry_points_are_exported_and_bound():
    lib = _lib.lib()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(lib, n)
    # the single-kernel arguments plus B and the batch stride of w
    assert len(_lib.SIGNATURES[NAMES[1]][1]) == len(_lib.SIGNATURES['dpgp_ard_rbf_gram_grad_f64'][1]) + 2
    assert len(_lib.SIGNATURES[NAMES[1]][1]) == len(ORDER) + 1                  # (+ the stream)


@pytest.mark.parametrize('index,name', list(enumerate(ORDER, start=1)))
def test_every_bad_argument_comes_back_with_its_index(index, name):
    assert _call(**{name: BAD[name]}) == -index


def test_the_checks_are_made_in_declaration_order():
    bad = dict(BAD)
    for index, name in enumerate(ORDER, start=1):
        assert _call(**bad) == -index, name
        bad[name] = GOOD[name]


def test_limits_and_empty_problems():
    assert _call(Q=65) == -3 and _call(Q=64, ws_bytes=7) == -14
    wsb = _lib.lib().dpgp_ard_rbf_gram_grad_batched_workspace_bytes(3, 70, 5)
    assert _call(ws_bytes=wsb - 1) == -14                                       # one byte short
    assert _call(ldw=72, w_stride=69 * 72 + 70, ws_bytes=wsb - 1) == -14       # the smallest stride of a padded w passes
    assert _call(ldw=72, w_stride=69 * 72 + 69) == -9
    assert _call(B=1, w_stride=0, ws_bytes=7) == -14                            # one kernel: the stride is not used
    null = dict(x=None, gamma=None, alpha=None, w=None, ldw=0, w_stride=0, r=None, sx=None, sq=None, ws=None, ws_bytes=0)
    assert _call(B=0, **null) == 0 and _call(N=0, **null) == 0 and _call(B=0, N=0, **null) == 0
    assert _call(B=0, Q=0, **null) == -3                                        # (Q is checked before the early return)


def test_workspace_query():
    q = _lib.lib().dpgp_ard_rbf_gram_grad_batched_workspace_bytes
    per = lambda b, n, qq: 8 * b * (1 + 2 * qq) * n                              # one slab per kernel
    for shape in [(1, 1, 1), (3, 70, 5), (20, 50, 10), (512, 128, 10), (2, 2000, 64)]:
        assert q(*shape) >= per(*shape), shape
    for shape in [(0, 5, 3), (3, 0, 3), (3, 5, 0), (3, 5, 65), (-1, 5, 3), (3, -5, 3)]:
        assert q(*shape) == 0, shape
    # the slab plan divides its workgroup target by B: one slab per kernel once B row tiles reach it, never more slabs than
    # column chunks, and for one kernel the single-kernel plan
    assert q(512, 128, 10) == per(512, 128, 10) and q(256, 128, 10) == per(256, 128, 10)
    assert q(128, 128, 10) == 2 * per(128, 128, 10)
    assert q(20, 50, 10) == per(20, 50, 10) and q(4, 128, 10) == 2 * per(4, 128, 10)
    single = _lib.lib().dpgp_ard_rbf_gram_grad_workspace_bytes
    for n, qq in [(50, 10), (777, 10), (2000, 10), (5000, 3)]:
        assert q(1, n, qq) == single(n, qq)
    assert q(3, 2000, 10) < 3 * single(2000, 10)
