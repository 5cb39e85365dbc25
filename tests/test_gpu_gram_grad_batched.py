"""GPU tests of the batched gram-gradient contraction, dpgp_ard_rbf_gram_grad_batched_f64 / ops.ard_rbf_gram_grad_batched
(csrc/gram_grad.hip): every kernel b of the batch against the dense torch-CPU restatement of test_gpu_gp_regression.py at the
project's operator tolerance (1e-12 of the result's largest entry), against the single-kernel operator on b's own inputs
(1e-13: the bits may differ where the slab plans do), run-to-run bits, views of w with even and odd padding, and model-sized
batches.  The C ABI's argument checks need no GPU: tests/test_gram_grad_batched_abi.py."""
import itertools

import numpy as np
import pytest
import torch

from test_gpu_gp_regression import dense_gram_grad

pytestmark = pytest.mark.gpu


def inputs(b, n, q, seed):
    """Every kernel its own x (far from the origin), gamma, alpha and non-symmetric w: a wrong batch offset shows."""
    rng = np.random.default_rng(seed)
    x = 100.0 + 10.0 * np.arange(b)[:, None, None] + rng.uniform(-1.5, 1.5, (b, n, q))
    gamma = rng.uniform(0.3, 1.5, (b, q)) / max(1.0, q / 4.0)
    alpha = rng.uniform(0.5, 2.0, b)
    w = rng.standard_normal((b, n, n))
    return tuple(torch.as_tensor(a) for a in (x, gamma, alpha, w))


def dense(x, gamma, alpha, w):
    per = [dense_gram_grad(x[b], gamma[b], alpha[b], w[b]) for b in range(x.shape[0])]
    return tuple(torch.stack([p[k] for p in per]) for k in range(3))


def check(got, ref, tol, tag=''):
    for name, a, r in zip(('r', 'sx', 'sq'), got, ref):
        a, r = a.cpu().numpy(), r.cpu().numpy()
        assert a.shape == r.shape, name
        print('%s %s: max |err| %.3e of %.3e' % (tag, name, np.abs(a - r).max(), np.abs(r).max()))
        np.testing.assert_allclose(a, r, rtol=0, atol=tol * np.abs(r).max(), err_msg='%s %s' % (tag, name))


@pytest.mark.parametrize('b,n,q', list(itertools.product([1, 3], [1, 17, 64, 65, 130], [1, 10, 23, 64])))
def test_matches_the_dense_restatement_and_the_single_kernel_operator(dev, b, n, q):
    from dp_gp_lvm_amd import ops
    cpu = inputs(b, n, q, 1000 * b + 10 * n + q)
    x, gamma, alpha, w = (a.to(dev) for a in cpu)
    got = ops.ard_rbf_gram_grad_batched(x, gamma, alpha, w)
    assert [tuple(a.shape) for a in got] == [(b, n), (b, n, q), (b, n, q)]
    check(got, dense(*cpu), 1e-12, 'dense')
    single = [ops.ard_rbf_gram_grad(x[i], gamma[i:i + 1], alpha[i:i + 1], w[i]) for i in range(b)]
    stacked = tuple(torch.stack([s[k] for s in single]) for k in range(3))
    if b == 1:                      # the single operator is the batched one at B = 1: the same kernel, plan and summation order
        for name, u, v in zip(('r', 'sx', 'sq'), got, stacked):
            assert torch.equal(u, v), 'single %s: not the same bits' % name
    else:                           # (the plan, and with it the slabs' summation order, may differ)
        check(got, stacked, 1e-13, 'single')
    again = ops.ard_rbf_gram_grad_batched(x, gamma, alpha, w)
    for u, v in zip(got, again):
        assert torch.equal(u, v), 'two calls differ'


@pytest.mark.parametrize('pad', [2, 3])
def test_views_of_w_with_even_and_odd_padding(dev, pad):
    """pad 2: even leading dimension (the 16-byte loads); pad 3: odd (element loads; with an odd batch stride too)."""
    from dp_gp_lvm_amd import ops
    b, n, q = 3, 130, 10
    x, gamma, alpha, w = (a.to(dev) for a in inputs(b, n, q, 7))
    want = ops.ard_rbf_gram_grad_batched(x, gamma, alpha, w)
    big = torch.full((b, n + 1, n + pad), float('nan'), dtype=torch.float64, device=dev)
    big[:, :n, :n] = w
    view = big[:, :n, :n]
    assert not view.is_contiguous() and view.stride(2) == 1
    check(ops.ard_rbf_gram_grad_batched(x, gamma, alpha, view), want, 1e-13, 'pad %d' % pad)
    # anything else is made contiguous: a transposed view
    wt = w.transpose(1, 2)
    check(ops.ard_rbf_gram_grad_batched(x, gamma, alpha, wt), ops.ard_rbf_gram_grad_batched(x, gamma, alpha, wt.contiguous()),
          1e-13, 'transposed')


@pytest.mark.parametrize('b,n,q', [(20, 50, 10), (64, 128, 10)])
def test_model_sized_batches(dev, b, n, q):
    from dp_gp_lvm_amd import ops
    cpu = inputs(b, n, q, b + n)
    got = ops.ard_rbf_gram_grad_batched(*(a.to(dev) for a in cpu))
    check(got, dense(*cpu), 1e-12, 'dense')


def test_wrapper_checks(dev):
    from dp_gp_lvm_amd import ops
    x, gamma, alpha, w = (a.to(dev) for a in inputs(2, 9, 3, 1))
    with pytest.raises(AssertionError):
        ops.ard_rbf_gram_grad_batched(x, gamma, alpha, w[:, :-1])
    with pytest.raises(AssertionError):
        ops.ard_rbf_gram_grad_batched(x, gamma[:1], alpha, w)
    with pytest.raises(RuntimeError):
        ops.ard_rbf_gram_grad_batched(x, gamma, alpha, w.cpu())
    empty = ops.ard_rbf_gram_grad_batched(x[:0], gamma[:0], alpha[:0], w[:0])
    assert [tuple(a.shape) for a in empty] == [(0, 9), (0, 9, 3), (0, 9, 3)]
