"""CPU tests (no GPU) of models/test_latents.py, the test-time fit of q(X*) that the four latent-variable models share: the start,
the Adam loop, the ascent gradient of a frozen bound and the choice between the two masked nearest-neighbour starts, each against
a literal restatement written out here.  Shapes: N = 7, N* = 3, D = 5, Q = 2, one test row with nothing observed."""
import numpy as np
import torch
import torch.nn.functional as F

from dp_gp_lvm_amd.models import test_latents as tl
from dp_gp_lvm_amd.utils import missing
from dp_gp_lvm_amd.utils.expressions import principal_component_analysis as pca

N, N_T, D, Q = 7, 3, 5, 2
CPU = torch.device('cpu')


def problem():
    rs = np.random.default_rng(11)
    y_train, y_test, x_train = rs.standard_normal((N, D)), rs.standard_normal((N_T, D)), rs.standard_normal((N, Q))
    train_obs, obs = rs.random((N, D)) >= 0.35, rs.random((N_T, D)) >= 0.3
    train_obs[:, 0] = True                              # (every training row shares a column with every observed test row)
    obs[0], obs[1] = [True, True, False, True, False], False            # row 1: nothing observed
    obs[2, 0] = True
    return y_train, y_test, x_train, train_obs, obs


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def state_after_one_draw(seed):
    np.random.seed(seed)
    np.random.normal(size=(N_T, Q))
    return np.random.get_state()


def never():
    raise AssertionError('the neighbour start must not be formed')


def test_start_takes_given_values_flat_and_draws_nothing():
    rs = np.random.default_rng(0)
    mean, var = rs.standard_normal(N_T * Q), torch.as_tensor(rs.uniform(0.1, 2.0, N_T * Q))
    np.random.seed(5)
    before = np.random.get_state()
    xt, st = tl.start(N_T, Q, CPU, mean, var, True, None, never)                       # (a given mean wins over use_pca)
    assert same_state(before, np.random.get_state())
    assert xt.dtype == st.dtype == torch.float64 and xt.is_contiguous() and st.is_contiguous()
    assert torch.equal(xt, torch.as_tensor(mean.reshape(N_T, Q))) and torch.equal(st, var.reshape(N_T, Q))
    # a given mean alone: variances 1
    xt, st = tl.start(N_T, Q, CPU, mean.reshape(N_T, Q), None, False, None, never)
    assert torch.equal(xt, torch.as_tensor(mean.reshape(N_T, Q))) and torch.equal(st, torch.ones((N_T, Q), dtype=torch.float64))
    assert same_state(before, np.random.get_state())


def test_start_by_pca_draws_nothing():
    _, y_test, _, _, _ = problem()
    var = np.full((N_T, Q), 0.25)
    np.random.seed(5)
    before = np.random.get_state()
    xt, st = tl.start(N_T, Q, CPU, None, var, True, y_test, never)
    assert same_state(before, np.random.get_state())
    assert torch.equal(xt, torch.as_tensor(pca(y_test, num_latent_dimensions=Q))) and torch.equal(st, torch.as_tensor(var))


def test_start_by_l2_neighbour_is_one_draw():
    y_train, y_test, x_train, _, _ = problem()
    do = 3
    np.random.seed(7)
    xt, st = tl.start(N_T, Q, CPU, None, None, False, y_test[:, :do],
                      lambda: tl.l2_neighbour(y_train[:, :do], y_test[:, :do], x_train))
    assert same_state(np.random.get_state(), state_after_one_draw(7))
    np.random.seed(7)
    d2 = np.array([[np.sum((y_train[i, :do] - y_test[n, :do]) ** 2) for n in range(N_T)] for i in range(N)])
    want = x_train[np.argmin(d2, axis=0)] + np.random.normal(scale=0.01, size=(N_T, Q))
    assert torch.equal(xt, torch.as_tensor(want)) and torch.equal(st, torch.ones((N_T, Q), dtype=torch.float64))


def masked_rows(y_train, train_obs, y_test, obs):
    """Per test row: the training row with the smallest MEAN squared difference over the columns observed in the test row (and,
    with a training mask, in the training row too); -1 where no column is left."""
    rows = []
    for n in range(N_T):
        best, arg = np.inf, -1
        for i in range(N):
            cols = [d for d in range(D) if obs[n, d] and (train_obs is None or train_obs[i, d])]
            if cols:
                val = np.mean([(y_train[i, d] - y_test[n, d]) ** 2 for d in cols])
                if val < best:
                    best, arg = val, i
        rows.append(arg)
    return rows


def test_masked_neighbour_picks_the_jointly_observed_form_iff_a_training_mask_is_given():
    y_train, y_test, x_train, train_obs, obs = problem()
    y_nan = np.where(obs, y_test, np.nan)
    out = {}
    for name, mask in (('complete', None), ('masked', train_obs)):
        np.random.seed(3)
        xt, st = tl.start(N_T, Q, CPU, None, None, False, y_test,
                          lambda: tl.masked_neighbour(y_train, mask, y_nan, obs, x_train))
        assert same_state(np.random.get_state(), state_after_one_draw(3))
        rows = masked_rows(y_train, mask, y_test, obs)
        assert rows[1] == -1 and min(rows[0], rows[2]) >= 0
        np.random.seed(3)
        noise = np.random.normal(scale=0.01, size=(N_T, Q))
        want = np.stack([x_train[r] if r >= 0 else np.zeros(Q) for r in rows]) + noise
        assert torch.equal(xt, torch.as_tensor(want)), name
        assert torch.equal(st, torch.ones((N_T, Q), dtype=torch.float64))
        np.random.seed(3)
        helper = missing.masked_nearest_neighbour_init(y_train, y_nan, obs, x_train) if mask is None else \
            missing.jointly_observed_nearest_neighbour_init(y_train, mask, y_nan, obs, x_train)
        assert np.array_equal(xt.numpy(), helper), name
        out[name] = rows
    assert out['complete'] != out['masked']                     # (the two forms disagree on this data: the choice is visible)


def quadratic_grad(centre, scale):
    return lambda mu, s: (-scale * (mu - centre), -0.5 * (1.0 - 1.0 / s))


def test_fit_is_the_loop_written_out_and_updates_its_start_in_place():
    rs = np.random.default_rng(2)
    centre, scale = torch.as_tensor(rs.standard_normal((N_T, Q))), torch.as_tensor(rs.uniform(0.5, 2.0, (N_T, Q)))
    grad_fn = quadratic_grad(centre, scale)
    x0 = torch.as_tensor(rs.standard_normal((N_T, Q)))
    s0 = torch.as_tensor(rs.uniform(0.2, 3.0, (N_T, Q)))
    s0[0, 0], s0[1, 1] = 1e-6, 50.0
    for iterations in (0, 1, 5):
        xt = x0.clone()
        got_x, got_s = tl.fit(grad_fn, xt, s0, iterations, 0.05)
        assert got_x is xt
        x, raw = x0.clone(), torch.log(torch.expm1(s0))
        opt = torch.optim.Adam([x, raw], lr=0.05)
        for _ in range(iterations):
            sv = F.softplus(raw)
            g_mu, g_s = grad_fn(x, sv)
            x.grad, raw.grad = -g_mu, -g_s * torch.sigmoid(raw)
            opt.step()
        assert torch.equal(got_x, x) and torch.equal(got_s, F.softplus(raw)), iterations
        assert (iterations == 0) == torch.equal(got_x, x0)
    # no iteration: the variances come back through log(expm1(.)) and softplus.  softplus(r) = log1p(e^r) carries the rounding
    # of r = log(expm1(s)) relatively as |r| eps: |r| < 14 at s = 1e-6 (3e-15); at s = 50, r = 50 to rounding and softplus(r) = r.
    _, back = tl.fit(grad_fn, x0.clone(), s0, 0, 0.05)
    assert float(((back - s0).abs() / s0).max()) <= 1e-14
    assert not s0.requires_grad and torch.equal(s0[0, 0], torch.tensor(1e-6, dtype=torch.float64))     # (the start is not touched)


def test_ascent_gradient_is_the_bounds_gradient_minus_the_kl_gradient():
    rs = np.random.default_rng(4)
    mu, s = torch.as_tensor(rs.standard_normal((N_T, Q))), torch.as_tensor(rs.uniform(0.1, 2.0, (N_T, Q)))
    d_mu, d_s = torch.as_tensor(rs.standard_normal((N_T, Q))), torch.as_tensor(rs.standard_normal((N_T, Q)))
    calls = []

    class Bound:
        def evaluate(self, mu_, s_, grad=False):
            calls.append((mu_, s_, grad))
            return torch.zeros(()), d_mu, d_s

    g_mu, g_s = tl.ascent_gradient(Bound(), mu, s)
    assert len(calls) == 1 and calls[0][0] is mu and calls[0][1] is s and calls[0][2] is True
    assert torch.equal(g_mu, d_mu - mu) and torch.equal(g_s, d_s - 0.5 * (1.0 - 1.0 / s))
    k_mu, k_s = tl.kl_gradient(mu, s)
    assert torch.equal(k_mu, mu) and torch.equal(k_s, 0.5 * (1.0 - 1.0 / s))
