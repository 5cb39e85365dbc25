"""GPU tests of gp_regression / gp_lvm (reference src/models/gaussian_process.py:22-129) and of the operator their gradient
needs, dpgp_ard_rbf_gram_grad_f64: the contraction against a dense torch-CPU restatement, run-to-run bits, argument checks;
the models against the reference fixtures (tools/gen_golden_gp.py -> tests/golden/gpr_ref_*.npz, gplvm_ref_*.npz)."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'gpr_ref_*.npz')) +
                  glob.glob(os.path.join(GOLDEN, 'gplvm_ref_*.npz')))


def dense_gram_grad(x, gamma, alpha, w):
    out = ([], [], [])
    for i0 in range(0, x.shape[0], 256):                          # (row blocks: the [rows, N, Q] differences stay small)
        d = x[i0:i0 + 256, None, :] - x[None, :, :]
        g = w[i0:i0 + 256] * (alpha * torch.exp(-0.5 * torch.sum(gamma * d * d, dim=-1)))
        for o, v in zip(out, (g.sum(1), torch.einsum('ij,ijq->iq', g, d), torch.einsum('ij,ijq->iq', g, d * d))):
            o.append(v)
    return tuple(torch.cat(o) for o in out)


def inputs(n, q, seed):
    rng = np.random.default_rng(seed)
    x = 100.0 + rng.uniform(-1.5, 1.5, (n, q))                  # far from the origin: differences, not |x|^2 - 2 x^T x
    gamma = rng.uniform(0.3, 1.5, (1, q)) / max(1.0, q / 4.0)
    w = rng.standard_normal((n, n))                              # not symmetric
    return x, gamma, np.array([[1.7]]), w


@pytest.mark.parametrize('q', [1, 3, 10, 20, 33])
@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 200, 777, 2048])
def test_gram_grad_matches_dense_restatement(dev, n, q):
    from dp_gp_lvm_amd import ops
    x, gamma, alpha, w = inputs(n, q, 100 * n + q)
    got = ops.ard_rbf_gram_grad(*(torch.as_tensor(a, device=dev) for a in (x, gamma, alpha, w)))
    ref = dense_gram_grad(*(torch.as_tensor(a) for a in (x, gamma.reshape(-1), alpha[0, 0], w)))
    for name, a, b in zip(('r', 'sx', 'sq'), got, ref):
        b = b.numpy()
        np.testing.assert_allclose(a.cpu().numpy(), b, rtol=1e-12, atol=1e-12 * np.abs(b).max(), err_msg=name)


def test_gram_grad_same_bits_and_strided_w(dev):
    from dp_gp_lvm_amd import ops
    x, gamma, alpha, w = (torch.as_tensor(a, device=dev) for a in inputs(777, 10, 3))
    a = ops.ard_rbf_gram_grad(x, gamma, alpha, w)
    b = ops.ard_rbf_gram_grad(x, gamma, alpha, w)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    big = torch.zeros((777, 780), dtype=torch.float64, device=dev)   # ldw > N (even: the 16-byte load path)
    big[:, :777] = w
    c = ops.ard_rbf_gram_grad(x, gamma, alpha, big[:, :777])
    for u, v in zip(a, c):
        assert torch.equal(u, v)
    odd = torch.zeros((777, 779), dtype=torch.float64, device=dev)   # odd ldw: element loads
    odd[:, :777] = w
    d = ops.ard_rbf_gram_grad(x, gamma, alpha, odd[:, :777])
    for u, v in zip(a, d):
        torch.testing.assert_close(u, v, rtol=1e-13, atol=1e-13 * float(v.abs().max()))


def test_gram_grad_bad_arguments(dev):
    from dp_gp_lvm_amd import _lib
    l = _lib.lib()
    n, q = 100, 4
    wsb = l.dpgp_ard_rbf_gram_grad_workspace_bytes(n, q)
    assert wsb >= 8 * (2 * q + 1) * n
    assert l.dpgp_ard_rbf_gram_grad_workspace_bytes(n, 65) == 0
    t = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    x, gm, al, w, r, sx, sq, ws = t(n, q), t(q), t(1), t(n, n), t(n), t(n, q), t(n, q), t(wsb // 8 + 1)
    args = [n, q, x.data_ptr(), gm.data_ptr(), al.data_ptr(), w.data_ptr(), n, r.data_ptr(), sx.data_ptr(), sq.data_ptr(),
            ws.data_ptr(), wsb, None]
    assert l.dpgp_ard_rbf_gram_grad_f64(*args) == 0
    torch.cuda.synchronize()
    bad = {1: -1, 2: 0, 3: None, 4: None, 5: None, 6: None, 7: n - 1, 8: None, 9: None, 10: None, 11: None, 12: wsb - 1}
    for idx, val in bad.items():
        a = list(args)
        a[idx - 1] = val
        assert l.dpgp_ard_rbf_gram_grad_f64(*a) == -idx, idx
    a = list(args)
    a[1] = 65
    assert l.dpgp_ard_rbf_gram_grad_f64(*a) == -2
    a = [0, q, None, None, None, None, 0, None, None, None, None, 0, None]
    assert l.dpgp_ard_rbf_gram_grad_f64(*a) == 0                    # N == 0: nothing to do, no pointer is read


def build(g, dev):
    from dp_gp_lvm_amd.models.gaussian_process import gp_lvm, gp_regression
    if str(g['kind']) == 'gpr':
        model = gp_regression(g['x'], g['y'], device=dev)
    else:
        model = gp_lvm(g['y'], num_latent_dims=g['x_latent'].shape[1], device=dev,
                       initial_values=dict(x_latent=g['x_latent']))
    with torch.no_grad():
        for k, v in model.raw_variables.items():
            v.copy_(torch.as_tensor(g[k], device=dev).reshape(v.shape))
    return model


@pytest.mark.parametrize('fixture', FIXTURES)
def test_model_matches_the_reference(dev, fixture):
    g = golden(fixture)
    model = build(g, dev)
    np.testing.assert_allclose(float(model.objective.detach()), float(g['objective']), rtol=1e-10)
    np.testing.assert_allclose(model.log_likelihood.detach().cpu().numpy(), g['log_likelihood'], rtol=1e-10)
    got = model.gradients()
    assert list(got) == list(model.raw_variables)
    for k, v in got.items():
        ref = g['grad_' + k]
        np.testing.assert_allclose(v.cpu().numpy().reshape(ref.shape), ref, rtol=1e-8, atol=1e-8 * np.abs(ref).max(), err_msg=k)
    mean, covar = model.predict_mean_covar(g['x_test'])
    np.testing.assert_allclose(mean.cpu().numpy(), g['pred_mean'], rtol=1e-10, atol=1e-10 * np.abs(g['pred_mean']).max())
    np.testing.assert_allclose(covar.cpu().numpy(), g['pred_covar'], rtol=1e-10, atol=1e-10 * np.abs(g['pred_covar']).max())
    # N* = 1 (the reference cannot): the first row / entry of the full prediction
    m1, c1 = model.predict_mean_covar(g['x_test'][:1])
    assert tuple(m1.shape) == (1, g['y'].shape[1]) and tuple(c1.shape) == (1, 1)
    np.testing.assert_allclose(m1.cpu().numpy(), g['pred_mean'][:1], rtol=1e-10, atol=1e-10 * np.abs(g['pred_mean']).max())
    np.testing.assert_allclose(c1.cpu().numpy(), g['pred_covar'][:1, :1], rtol=1e-10)


@pytest.mark.parametrize('fixture', ['gpr_ref_150_4_5', 'gplvm_ref_60_8_3'])
def test_backward_equals_gradients(dev, fixture):
    model = build(golden(fixture), dev)
    want = model.gradients()
    for v in model.raw_variables.values():
        v.grad = None
    model.objective.backward()
    for k, v in model.raw_variables.items():
        torch.testing.assert_close(v.grad, want[k].reshape(v.shape), rtol=1e-10, atol=1e-10 * float(want[k].abs().max()))


def test_textbook_prediction_mean(dev):
    g = golden('gpr_ref_40_3_1')
    model = build(g, dev)
    mean, covar = model.predict_mean_covar(g['x_test'], reference_compat=False)
    gamma = np.logaddexp(0.0, g['gamma_raw'])
    alpha, beta = np.logaddexp(0.0, g['alpha_raw'])[0, 0], np.logaddexp(0.0, g['beta_raw'])[0, 0]
    k = lambda a, b: alpha * np.exp(-0.5 * np.sum(gamma * (a[:, None] - b[None]) ** 2, axis=-1))
    x, xs = g['x'], g['x_test']
    kxx = k(x, x) + (1.0 / beta + 1e-8) * np.eye(len(x))
    want = k(x, xs).T @ np.linalg.solve(kxx, g['y'])
    np.testing.assert_allclose(mean.cpu().numpy(), want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
    np.testing.assert_allclose(covar.cpu().numpy(), g['pred_covar'], rtol=1e-10, atol=1e-10 * np.abs(g['pred_covar']).max())


@pytest.mark.parametrize('kind', ['gpr', 'gplvm'])
def test_adam_lowers_the_objective(dev, kind):
    from dp_gp_lvm_amd.models.gaussian_process import gp_lvm, gp_regression
    from dp_gp_lvm_amd.kernels.rbf_kernel import k_ard_rbf
    g = golden('gpr_ref_150_4_5' if kind == 'gpr' else 'gplvm_ref_130_12_4')
    if kind == 'gpr':
        kern = k_ard_rbf(gamma=torch.full((1, 4), 0.5, dtype=torch.float64), alpha=torch.ones(1, 1, dtype=torch.float64),
                         beta=torch.full((1, 1), 2.0, dtype=torch.float64))
        model = gp_regression(g['x'], g['y'], kernel=kern, device=dev)
        np.testing.assert_allclose(torch.nn.functional.softplus(model.raw_variables['gamma_raw']).detach().cpu().numpy(),
                                   np.full((1, 4), 0.5), rtol=1e-12)
    else:
        model = gp_lvm(g['y'], num_latent_dims=4, device=dev)
        assert tuple(model.latent_input.shape) == (g['y'].shape[0], 4)
    before = float(model.objective)
    model.optimise(50, learning_rate=0.01)
    after = float(model.objective)
    assert np.isfinite(after) and after < before, (before, after)

