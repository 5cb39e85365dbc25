"""CPU tests (no GPU) of mixture_moments (models/frozen_bound_t.py): the per-entry mean and variance of the over-T model's
mixture over the atoms, sum_t phi_td N(mean_t(n,d), var_t(n,d))."""
import numpy as np
import torch

from dp_gp_lvm_amd.models.frozen_bound_t import mixture_moments


def random_case(t, n, j, seed):
    rs = np.random.default_rng(seed)
    phi = rs.random((t, j)) + 0.05
    phi /= phi.sum(axis=0, keepdims=True)
    return phi, rs.standard_normal((t, n, j)), rs.uniform(0.01, 2.0, (t, n, j))


def run(phi, mean_t, var_t):
    mean, var = mixture_moments(*(torch.as_tensor(a, dtype=torch.float64) for a in (phi, mean_t, var_t)))
    return mean.numpy(), var.numpy()


def test_one_atom_returns_its_inputs():
    _, mean_t, var_t = random_case(1, 5, 3, 0)
    mean, var = run(np.ones((1, 3)), mean_t, var_t)
    np.testing.assert_allclose(mean, mean_t[0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(var, var_t[0], rtol=1e-14, atol=1e-15)


def test_one_hot_weights_select_an_atom():
    _, mean_t, var_t = random_case(4, 6, 5, 1)
    pick = np.array([2, 0, 3, 3, 1])
    phi = np.zeros((4, 5))
    phi[pick, np.arange(5)] = 1.0
    mean, var = run(phi, mean_t, var_t)
    np.testing.assert_allclose(mean, mean_t[pick, :, np.arange(5)].T, rtol=0, atol=1e-15)
    np.testing.assert_allclose(var, var_t[pick, :, np.arange(5)].T, rtol=1e-14, atol=1e-15)


def test_the_mixture_is_at_least_as_wide_as_its_atoms_on_average():
    # var = sum_t phi var_t + (sum_t phi mean_t^2 - mean^2), and the bracket is a variance (of the atoms' means): >= 0
    phi, mean_t, var_t = random_case(5, 40, 7, 2)
    _, var = run(phi, mean_t, var_t)
    inner = np.sum(phi[:, None, :] * var_t, axis=0)
    assert np.all(var >= inner - 1e-14 * np.abs(inner))
    assert np.any(var > inner * (1.0 + 1e-6))


def test_against_a_direct_evaluation():
    for seed, (t, n, j) in enumerate([(1, 1, 1), (3, 7, 2), (8, 70, 13)]):
        phi, mean_t, var_t = random_case(t, n, j, 10 + seed)
        mean, var = run(phi, mean_t, var_t)
        want_mean, want_var = np.zeros((n, j)), np.zeros((n, j))
        for d in range(j):
            for i in range(n):
                m1 = sum(phi[a, d] * mean_t[a, i, d] for a in range(t))
                m2 = sum(phi[a, d] * (var_t[a, i, d] + mean_t[a, i, d] ** 2) for a in range(t))
                want_mean[i, d], want_var[i, d] = m1, m2 - m1 * m1
        print('max |err|: mean %.3e, var %.3e (bound 1e-14)' % (np.abs(mean - want_mean).max(), np.abs(var - want_var).max()))
        np.testing.assert_allclose(mean, want_mean, rtol=1e-14, atol=1e-14)
        np.testing.assert_allclose(var, want_var, rtol=1e-14, atol=1e-14)
