"""
Discrete curves in latent space under the expected metric G(x) of models/marginals.py (Tosi et al., UAI 2014): energy, length and
geodesics.  A curve is S + 1 points c_0 .. c_S [Q]; segment i has the midpoint x_i = (c_i + c_{i+1}) / 2 and the direction
v_i = c_{i+1} - c_i, and with e_i = v_i^T G(x_i) v_i

    energy  E = S sum_i e_i            (the Riemann sum of int_0^1 |c'(t)|_G^2 dt at step 1 / S)
    length  L = sum_i sqrt(e_i)        (L^2 <= E by Cauchy-Schwarz, with equality at constant speed)
    dE / dc_j = S [ (dx_{j-1} / 2 + dv_{j-1}) + (dx_j / 2 - dv_j) ],    dx_i = de_i / dx_i,  dv_i = de_i / dv_i

(a segment moves its midpoint by half of either end and its direction by -/+ the end).  A minimiser of E between fixed ends is a
discrete geodesic.  Everything here works on `terms`, a callable (x [N,Q], v [N,Q]) -> (e [N], dx [N,Q], dv [N,Q]) that a model
builds ONCE per call from its training side (marginals.Metric.curve_terms on ops.ard_rbf_point_energy): C curves are one
call with N = C S, and an iteration of latent_geodesic is one call plus element-wise work.  fp64, no autograd.

The initial-value side: a geodesic obeys G x'' = -Gamma(x, x'), Gamma the Christoffel symbols of the first kind contracted twice
with the velocity.  exp_map integrates (x', v') = (v, -G^-1 Gamma) over t in [0, 1] by the classical Runge-Kutta scheme on `accel`,
a callable (x [N,Q], v [N,Q]) -> (a [N,Q], speed [N], info [N]) that a model builds ONCE per call
(marginals.Metric.accel on ops.ard_rbf_point_christoffel and ops.geodesic_accel): C curves are one batch, a stage is one call.

Its tangent and its inverse: exp_map_tangent integrates the tangent-linear equation beside the curve (a discrete Jacobi field, the
exact derivative of exp_map's discrete map) on `accel_tangent`, a callable (x, v, dx, dv [N,Q]) -> (a, da [N,Q], speed [N], info [N])
(marginals.Metric.accel_tangent on ops.ard_rbf_point_christoffel_tangent and ops.geodesic_accel_tangent), and log_map is Newton
shooting on it: one batched tangent shot over C Q rows per iteration.

The Runge-Kutta loops of exp_map, exp_map_tangent and log_map run here, in Python, a stage being a handful of launches; each takes
`shoot`, a callable that returns the loop's results from elsewhere: marginals.Metric.shoot / shoot_tangent, ONE call of
ops.geodesic_shoot[_tangent] per shot, with the loop's bits (a model's integrator = 'device').

Parallel transport: along a geodesic a vector w obeys G w' = -Gamma(x; x', w), the symbols contracted with the velocity and w.
parallel_transport integrates (x', v', w_1' .. w_F') for a frame of F vectors by the same Runge-Kutta scheme on `transport`, a
callable (x, v [N,Q], w [N,F,Q]) -> (a [N,Q], dw [N,F,Q], speed [N], info [N]) (marginals.Metric.transport on
ops.ard_rbf_point_transport and ops.geodesic_transport); transport_to is log_map followed by it.  Its loop always runs here: there
is no integrator on the device for it yet.

The four callables are the methods of ONE marginals.Metric, the metric that a public call runs under; the models' public methods
on them are written once, in models/latent_geometry.py.
"""
import numpy as np
import torch

from ..utils.types import TORCH_DTYPE


def curves_arg(curve, q, device, name='curve'):
    """curve [S+1 x Q] or [C x S+1 x Q] (numpy or torch) as a contiguous fp64 tensor [C x S+1 x Q] on the device, and whether it
    came as a single curve."""
    c = curve.detach() if torch.is_tensor(curve) else torch.as_tensor(np.asarray(curve, dtype=np.float64))
    c = c.to(device=device, dtype=TORCH_DTYPE)
    assert c.dim() in (2, 3) and c.shape[-1] == q and c.shape[-2] >= 2 and c.shape[0] >= 1, \
        '%s must be [S+1 x Q] or [C x S+1 x Q] with S >= 1' % name
    return (c[None] if c.dim() == 2 else c).contiguous(), c.dim() == 2


def ends_arg(x, q, device, name):
    """x [Q] or [C x Q] (numpy or torch) as a contiguous fp64 tensor [C x Q] on the device."""
    x = x.detach() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=np.float64))
    x = x.to(device=device, dtype=TORCH_DTYPE)
    assert x.dim() in (1, 2) and x.shape[-1] == q and x.shape[0] >= 1, '%s must be [Q] or [C x Q]' % name
    return (x[None] if x.dim() == 1 else x).contiguous()


def states_arg(q, device, **named):
    """(the arguments `named`, each [Q] or [C x Q], as ends_arg's [C x Q] tensors in the order given, whether the first came as
    one point [Q]); AssertionError unless all have the same shape."""
    first = next(iter(named.values()))
    single = (first.dim() if torch.is_tensor(first) else np.asarray(first).ndim) == 1
    out = [ends_arg(x, q, device, name) for name, x in named.items()]
    names = list(named)
    assert all(o.shape == out[0].shape for o in out), '%s and %s must have the same shape' % (', '.join(names[:-1]), names[-1])
    return out, single


def segments(c):
    """(midpoints x, directions v), each [C S x Q], of the curves c [C x S+1 x Q]."""
    q = c.shape[2]
    return (0.5 * (c[:, :-1] + c[:, 1:])).reshape(-1, q).contiguous(), (c[:, 1:] - c[:, :-1]).reshape(-1, q).contiguous()


def energy(e, num_curves):
    """E [C] of the segment terms e [C S]."""
    e = e.reshape(num_curves, -1)
    return e.shape[1] * torch.sum(e, dim=1)


def length(e, num_curves):
    """L [C] of the segment terms e [C S] (a term rounded below zero counts as zero)."""
    return torch.sum(torch.sqrt(torch.clamp(e.reshape(num_curves, -1), min=0.0)), dim=1)


def gradient(dx, dv, num_curves):
    """dE / dc [C x S+1 x Q] of the segment gradients dx, dv [C S x Q]."""
    q = dx.shape[1]
    dx, dv = dx.reshape(num_curves, -1, q), dv.reshape(num_curves, -1, q)
    s = dx.shape[1]
    g = torch.zeros((num_curves, s + 1, q), dtype=dx.dtype, device=dx.device)
    g[:, :-1] += 0.5 * dx - dv
    g[:, 1:] += 0.5 * dx + dv
    return s * g


def prior_terms(v, weight):
    """The terms of a constant diagonal metric diag(weight [Q]): (sum_q weight_q v_q^2, 0, 2 weight_q v_q)."""
    return torch.sum(v * v * weight, dim=1), torch.zeros_like(v), 2.0 * v * weight


def curve_energy(terms, curve, q, device, return_gradient=False):
    c, single = curves_arg(curve, q, device)
    with torch.no_grad():
        e, dx, dv = terms(*segments(c))
        en = energy(e, c.shape[0])
        if not return_gradient:
            return en
        g = gradient(dx, dv, c.shape[0])
        return en, (g[0] if single else g)


def curve_length(terms, curve, q, device):
    c, _ = curves_arg(curve, q, device)
    with torch.no_grad():
        return length(terms(*segments(c))[0], c.shape[0])


def straight_line(x_from, x_to, num_segments):
    """[C x S+1 x Q]: the straight lines between x_from and x_to [C x Q]; their end rows are the bits of x_from and x_to."""
    t = torch.arange(num_segments + 1, dtype=x_from.dtype, device=x_from.device) / num_segments
    c = x_from[:, None, :] + t[None, :, None] * (x_to - x_from)[:, None, :]
    c[:, 0], c[:, -1] = x_from, x_to
    return c.contiguous()


def latent_geodesic(terms, x_from, x_to, q, device, num_segments=32, num_iterations=200, learning_rate=0.01, init=None):
    """(curve [C x S+1 x Q], length [C], energy [C]): E minimised over the interior points by Adam (torch.optim.Adam only applies
    the update) from the straight line, or from `init` [C x S+1 x Q] with its end rows replaced; each curve's lowest-energy
    iterate is kept, the start included, so the returned energy never exceeds the start's."""
    (a, b), _ = states_arg(q, device, x_from=x_from, x_to=x_to)
    num_segments, num_iterations = int(num_segments), int(num_iterations)
    assert num_segments >= 1 and num_iterations >= 0, 'num_segments >= 1 and num_iterations >= 0'
    n = a.shape[0]
    if init is None:
        c = straight_line(a, b, num_segments)
    else:
        c = curves_arg(init, q, device, 'init')[0].clone()
        assert tuple(c.shape) == (n, num_segments + 1, q), 'init must be [C x num_segments+1 x Q]'
        c[:, 0], c[:, -1] = a, b
    with torch.no_grad():
        best, best_e, best_energy = None, None, None

        def keep(e):
            nonlocal best, best_e, best_energy
            en = energy(e, n)
            if best is None:
                best, best_e, best_energy = c.clone(), e.reshape(n, -1).clone(), en
                return
            better = en < best_energy
            best = torch.where(better[:, None, None], c, best)
            best_e = torch.where(better[:, None], e.reshape(n, -1), best_e)
            best_energy = torch.where(better, en, best_energy)

        if num_segments > 1 and num_iterations > 0:
            inner = c[:, 1:-1].clone().requires_grad_(True)
            opt = torch.optim.Adam([inner], lr=learning_rate)
            for _ in range(num_iterations):
                e, dx, dv = terms(*segments(c))
                keep(e)
                inner.grad = gradient(dx, dv, n)[:, 1:-1].contiguous()
                opt.step()
                c[:, 1:-1] = inner.detach()
        keep(terms(*segments(c))[0])
        return best, length(best_e, n), best_energy


def geodesic_acceleration(accel, x, v, q, device):
    """a [N* x Q] (or [Q] for one point): x'' of the geodesics through x with the velocities v ([N* x Q] or [Q])."""
    (xs, vs), single = states_arg(q, device, x=x, v=v)
    with torch.no_grad():
        a = accel(xs, vs)[0]
    return a[0] if single else a


def _rk4(accel, xs, vs, num_steps):
    """(curve, vel [C x S+1 x Q], bad [C] int32): the classical RK4 steps of exp_map on the states xs, vs [C x Q]; bad counts the
    stages whose metric failed to factor.  Nothing is read on the host."""
    c, q, h = xs.shape[0], xs.shape[1], 1.0 / num_steps
    curve = torch.empty((c, num_steps + 1, q), dtype=xs.dtype, device=xs.device)
    vel = torch.empty_like(curve)
    bad = torch.zeros(c, dtype=torch.int32, device=xs.device)

    def f(xx, vv):
        nonlocal bad
        a, _, info = accel(xx, vv)
        bad = bad + (info != 0).to(torch.int32)
        return a

    curve[:, 0], vel[:, 0] = xs, vs
    for s in range(num_steps):
        k1x, k1v = vs, f(xs, vs)
        k2x = vs + (0.5 * h) * k1v
        k2v = f(xs + (0.5 * h) * k1x, k2x)
        k3x = vs + (0.5 * h) * k2v
        k3v = f(xs + (0.5 * h) * k2x, k3x)
        k4x = vs + h * k3v
        k4v = f(xs + h * k3x, k4x)
        xs = xs + (h / 6.0) * (k1x + 2.0 * k2x + 2.0 * k3x + k4x)
        vs = vs + (h / 6.0) * (k1v + 2.0 * k2v + 2.0 * k3v + k4v)
        curve[:, s + 1], vel[:, s + 1] = xs, vs
    return curve, vel, bad


def exp_map(accel, x, v, q, device, num_steps=64, return_velocity=False, shoot=None):
    """curve [C x S+1 x Q] (one curve [S+1 x Q] for x, v [Q]), S = num_steps: the exponential map of v at x, the classical RK4
    solution of (x', v') = (v, accel(x, v)) on t in [0, 1] at step 1 / S, all C curves in one batch; row 0 holds the bits of x.
    With return_velocity also the velocities in the same shape.  Four calls of accel per step plus element-wise work; nothing is
    read on the host until ONE read of the accumulated info at the end: FloatingPointError if the metric failed to factor at
    any stage of any curve.  shoot: None, or a callable (xs, vs [C x Q], num_steps) -> (curve, vel, bad) that takes the place of
    the loop on accel (marginals.Metric.shoot, the integrator on the device: the same bits)."""
    (xs, vs), single = states_arg(q, device, x=x, v=v)
    num_steps = int(num_steps)
    assert num_steps >= 1, 'num_steps >= 1'
    c = xs.shape[0]
    with torch.no_grad():
        curve, vel, bad = _rk4(accel, xs, vs, num_steps) if shoot is None else shoot(xs, vs, num_steps)
        failed = int(torch.count_nonzero(bad))
        if failed:
            raise FloatingPointError('latent_exp_map: the metric failed to factor (not positive definite in fp64) along %d of %d '
                                     'curves' % (failed, c))
    if single:
        curve, vel = curve[0], vel[0]
    return (curve, vel) if return_velocity else curve


# ---- the tangent of the initial-value side: Jacobi fields, and the logarithm map by Newton shooting ------------------------------
def geodesic_deviation(accel_tangent, x, v, dx, dv, q, device):
    """(a, da) [N* x Q] (or [Q] for one point): geodesic_acceleration's a with its bits, and its derivative along the direction
    (dx, dv) of the state (x, v), the right-hand side of the Jacobi equation.  accel_tangent: a callable
    (x, v, dx, dv [N,Q]) -> (a, da [N,Q], speed [N], info [N]) that a model builds ONCE per call (marginals.Metric.accel_tangent)."""
    (xs, vs, dxs, dvs), single = states_arg(q, device, x=x, v=v, dx=dx, dv=dv)
    with torch.no_grad():
        a, da = accel_tangent(xs, vs, dxs, dvs)[:2]
    return (a[0], da[0]) if single else (a, da)


def _rk4_tangent(accel_tangent, xs, vs, dxs, dvs, num_steps):
    """(curve, vel, dcurve, dvel [C x S+1 x Q], bad [C] int32, speed [C]): exp_map's steps on (x, v), with its bits, and their exact
    derivative on (dx, dv): every stage is differentiated by the chain rule, d k_x = dv_stage, d k_v = da.  bad counts the stages
    whose metric failed to factor; speed is v^T G(x) v at the start.  Nothing is read on the host."""
    c, q, h = xs.shape[0], xs.shape[1], 1.0 / num_steps
    curve = torch.empty((c, num_steps + 1, q), dtype=xs.dtype, device=xs.device)
    vel, dcurve, dvel = torch.empty_like(curve), torch.empty_like(curve), torch.empty_like(curve)
    bad = torch.zeros(c, dtype=torch.int32, device=xs.device)
    speed0 = None

    def f(xx, vv, dxx, dvv):
        nonlocal bad, speed0
        a, da, speed, info = accel_tangent(xx, vv, dxx, dvv)
        bad = bad + (info != 0).to(torch.int32)
        if speed0 is None:
            speed0 = speed
        return a, da

    curve[:, 0], vel[:, 0], dcurve[:, 0], dvel[:, 0] = xs, vs, dxs, dvs
    for s in range(num_steps):
        k1x, d1x = vs, dvs
        k1v, d1v = f(xs, vs, dxs, dvs)
        k2x, d2x = vs + (0.5 * h) * k1v, dvs + (0.5 * h) * d1v
        k2v, d2v = f(xs + (0.5 * h) * k1x, k2x, dxs + (0.5 * h) * d1x, d2x)
        k3x, d3x = vs + (0.5 * h) * k2v, dvs + (0.5 * h) * d2v
        k3v, d3v = f(xs + (0.5 * h) * k2x, k3x, dxs + (0.5 * h) * d2x, d3x)
        k4x, d4x = vs + h * k3v, dvs + h * d3v
        k4v, d4v = f(xs + h * k3x, k4x, dxs + h * d3x, d4x)
        xs = xs + (h / 6.0) * (k1x + 2.0 * k2x + 2.0 * k3x + k4x)
        vs = vs + (h / 6.0) * (k1v + 2.0 * k2v + 2.0 * k3v + k4v)
        dxs = dxs + (h / 6.0) * (d1x + 2.0 * d2x + 2.0 * d3x + d4x)
        dvs = dvs + (h / 6.0) * (d1v + 2.0 * d2v + 2.0 * d3v + d4v)
        curve[:, s + 1], vel[:, s + 1], dcurve[:, s + 1], dvel[:, s + 1] = xs, vs, dxs, dvs
    return curve, vel, dcurve, dvel, bad, speed0


def exp_map_tangent(accel_tangent, x, v, dx, dv, q, device, num_steps=64, return_velocity=False, shoot=None):
    """(curve, dcurve) [C x S+1 x Q] (single curves [S+1 x Q] for x, v, dx, dv [Q]): exp_map's curve, with its bits, and the
    tangent-linear classical RK4 solution started at (dx, dv): the EXACT derivative of exp_map's discrete map along that direction
    of (x, v), a discrete Jacobi field.  With return_velocity (curve, dcurve, velocity, dvelocity).  Four calls of accel_tangent
    per step plus element-wise work; the stages' info is accumulated on the device and read ONCE at the end:
    FloatingPointError if the metric failed to factor at any stage of any curve.  shoot: None, or a callable
    (xs, vs, dxs, dvs [C x Q], num_steps) -> _rk4_tangent's six results that takes its place (marginals.Metric.shoot_tangent,
    the integrator on the device: the same bits)."""
    (xs, vs, dxs, dvs), single = states_arg(q, device, x=x, v=v, dx=dx, dv=dv)
    num_steps = int(num_steps)
    assert num_steps >= 1, 'num_steps >= 1'
    with torch.no_grad():
        curve, vel, dcurve, dvel, bad, _ = _rk4_tangent(accel_tangent, xs, vs, dxs, dvs, num_steps) if shoot is None else \
            shoot(xs, vs, dxs, dvs, num_steps)
        failed = int(torch.count_nonzero(bad))
        if failed:
            raise FloatingPointError('latent_exp_map_tangent: the metric failed to factor (not positive definite in fp64) along '
                                     '%d of %d curves' % (failed, xs.shape[0]))
    out = (curve, dcurve, vel, dvel) if return_velocity else (curve, dcurve)
    return tuple(t[0] for t in out) if single else out


def _small_solve(a, b):
    """a^-1 b of the matrices a [C x Q x Q] and vectors b [C x Q] by Gauss-Jordan elimination with partial pivoting in
    element-wise device work: nothing is read on the host, and a system's bits do not depend on the batch it is in."""
    c, q = b.shape
    w = torch.cat([a, b[:, :, None]], dim=2).clone()
    rows = torch.arange(c, device=b.device)
    for j in range(q):
        piv = torch.argmax(torch.abs(w[:, j:, j]), dim=1) + j
        top, other = w[rows, piv], w[:, j].clone()
        w[rows, piv] = other
        w[:, j] = top / top[:, j:j + 1]
        fac = w[:, :, j:j + 1].clone()
        fac[:, j] = 0.0
        w = w - fac * w[:, j:j + 1, :]
    return w[:, :, q].contiguous()


def log_map(accel_tangent, x_from, x_to, q, device, num_steps=64, max_iterations=20, tol=1e-10, init=None, shoot=None):
    """(v [C x Q], distance [C], curve [C x S+1 x Q], residual [C]) (unbatched shapes for one pair): the logarithm map of x_to at
    x_from, the initial velocity whose exp_map at num_steps steps ends in x_to, by Newton shooting on the discrete map; distance =
    sqrt(v^T G(x_from) v), curve = exp_map(x_from, v), residual = |curve end - x_to|.

    From v = init [C x Q], or x_to - x_from.  An iteration is ONE batched shot of _rk4_tangent over C Q rows: row (c, r) carries
    dx = 0, dv = e_r, so that the rows' end tangents are the columns of J_c = d end / d v, and row (c, 0) supplies the end itself.
    With r_c = end_c - x_to_c the shot JUDGES the velocity it was fired with: the first one is taken as it is; a later one is
    accepted if its residual is smaller than the last accepted one's and every stage factored (lambda_c <- min(1, 2 lambda_c)),
    otherwise rejected (v_c goes back to the accepted velocity, lambda_c <- lambda_c / 2).  Then v_c - lambda_c J_c^-1 r_c of the
    accepted iterate is proposed.  A curve that has met the stop test is frozen while the others go on, so a pair's result does
    not depend on the batch it is in.  The accepted iterate is the best one met, so the result is never worse than the start.  At most
    max_iterations proposals are made and judged (1 + max_iterations shots); the loop ends early once every accepted residual is
    <= tol max(1, |x_to|).  ONE host read per iteration, of that test.  A curve whose residual stays above it is reported through
    `residual`, not raised; FloatingPointError only if the very first shot fails to factor.  The base features are recomputed for
    each of the Q directions.  shoot: as exp_map_tangent's; it fires every shot in the place of _rk4_tangent."""
    (a, b), single = states_arg(q, device, x_from=x_from, x_to=x_to)
    num_steps, max_iterations = int(num_steps), int(max_iterations)
    assert num_steps >= 1 and max_iterations >= 0, 'num_steps >= 1 and max_iterations >= 0'
    c = a.shape[0]
    with torch.no_grad():
        v = (b - a) if init is None else ends_arg(init, q, device, 'init').clone()
        assert v.shape == a.shape, 'init must have the shape of x_from'
        bound = tol * torch.clamp(torch.linalg.vector_norm(b, dim=1), min=1.0)
        rep = lambda t: t[:, None, :].expand(c, q, q).reshape(c * q, q).contiguous()
        xs, zero = rep(a), torch.zeros((c * q, q), dtype=a.dtype, device=a.device)
        unit = torch.eye(q, dtype=a.dtype, device=a.device).repeat(c, 1)
        lam = torch.ones(c, dtype=a.dtype, device=a.device)
        best = None                                           # (v, residual, step, curve, speed) of the accepted iterate
        fire = (lambda *state: _rk4_tangent(accel_tangent, *state)) if shoot is None else shoot
        for it in range(max_iterations + 1):
            curve, _, dcurve, _, bad, speed = fire(xs, rep(v), zero, unit, num_steps)
            base = curve.reshape(c, q, num_steps + 1, q)[:, 0]
            res = base[:, -1] - b
            norm = torch.linalg.vector_norm(res, dim=1)
            good = torch.sum(bad.reshape(c, q), dim=1) == 0
            jac = dcurve.reshape(c, q, num_steps + 1, q)[:, :, -1].transpose(1, 2)           # [C, end component, direction]
            step = _small_solve(jac, res)
            if best is None:
                ok = good
                best = [v, norm, step, base, speed.reshape(c, q)[:, 0]]
            else:
                ok = good & (norm < best[1]) & ~conv
                new = (v, norm, step, base, speed.reshape(c, q)[:, 0])
                best = [torch.where(ok.reshape((c,) + (1,) * (o.dim() - 1)), n, o) for n, o in zip(new, best)]
                lam = torch.where(ok, torch.clamp(2.0 * lam, max=1.0), 0.5 * lam)
            conv = best[1] <= bound
            done, failed = torch.stack([torch.all(conv), torch.any(~ok)]).tolist()
            if it == 0 and failed:
                raise FloatingPointError('latent_log_map: the metric failed to factor (not positive definite in fp64) along the '
                                         'first shot of %d of %d curves' % (int(torch.count_nonzero(~ok)), c))
            if done:
                break
            v = torch.where(conv[:, None], best[0], best[0] - lam[:, None] * best[2])
        v, norm, _, curve, speed = best
        dist = torch.sqrt(torch.clamp(speed, min=0.0))
    if single:
        return v[0], dist[0], curve[0], norm[0]
    return v, dist, curve.contiguous(), norm


# ---- parallel transport along geodesics ---------------------------------------------------------------------------------------------
def frames_arg(w, states, single, q, device):
    """w [C x F x Q], or one vector per point in the shape of the states ([C x Q], [Q] where they came as [Q]), as a contiguous
    fp64 tensor [C x F x Q] on the device, and whether it came as one vector."""
    w = w.detach() if torch.is_tensor(w) else torch.as_tensor(np.asarray(w, dtype=np.float64))
    w = w.to(device=device, dtype=TORCH_DTYPE)
    c = states.shape[0]
    one = w.dim() == (1 if single else 2)
    assert one or (w.dim() == 3 and not single), 'w must be [N* x F x Q], or one vector per point in the shape of x'
    w = (w.reshape(c, 1, q) if tuple(w.shape) == ((q,) if single else (c, q)) else None) if one else w
    assert w is not None and w.shape[0] == c and w.shape[1] >= 1 and w.shape[2] == q, \
        'w must be [N* x F x Q] with F >= 1, or one vector per point in the shape of x'
    return w.contiguous(), one


def parallel_transport_rate(transport, x, v, w, q, device):
    """(a, dw): geodesic_acceleration's a [N* x Q] (or [Q]) with its bits, and dw in the shape of w, the rates
    w_r' = -G(x)^-1 Gamma(x; v, w_r) of the vectors w ([N* x F x Q], or one vector per point [N* x Q] / [Q]) in parallel transport
    along the geodesics through x with the velocities v: the right-hand side of the transport equation.  transport: a callable
    (x, v [N,Q], w [N,F,Q]) -> (a [N,Q], dw [N,F,Q], speed [N], info [N]) that a model builds ONCE per call
    (marginals.Metric.transport)."""
    (xs, vs), single = states_arg(q, device, x=x, v=v)
    ws, one = frames_arg(w, xs, single, q, device)
    with torch.no_grad():
        a, dw = transport(xs, vs, ws)[:2]
    dw = dw[:, 0] if one else dw
    return (a[0], dw[0]) if single else (a, dw)


def _rk4_transport(transport, xs, vs, ws, num_steps):
    """(curve, vel [C x S+1 x Q], frames [C x S+1 x F x Q], bad [C] int32): the classical RK4 on the state (x, v, w_1 .. w_F) from
    xs, vs [C x Q] and ws [C x F x Q], with k_w = dw at each stage.  The x and v statements are _rk4's, and transport's a has
    accel's bits: curve and vel are exp_map's, bit for bit; frames[:, 0] holds the bits of ws.  bad counts the stages whose
    metric failed to factor.  Nothing is read on the host."""
    c, q, h = xs.shape[0], xs.shape[1], 1.0 / num_steps
    curve = torch.empty((c, num_steps + 1, q), dtype=xs.dtype, device=xs.device)
    vel = torch.empty_like(curve)
    frames = torch.empty((c, num_steps + 1) + tuple(ws.shape[1:]), dtype=xs.dtype, device=xs.device)
    bad = torch.zeros(c, dtype=torch.int32, device=xs.device)

    def f(xx, vv, ww):
        nonlocal bad
        a, dw, _, info = transport(xx, vv, ww)
        bad = bad + (info != 0).to(torch.int32)
        return a, dw

    curve[:, 0], vel[:, 0], frames[:, 0] = xs, vs, ws
    for s in range(num_steps):
        k1x = vs
        k1v, k1w = f(xs, vs, ws)
        k2x = vs + (0.5 * h) * k1v
        k2v, k2w = f(xs + (0.5 * h) * k1x, k2x, ws + (0.5 * h) * k1w)
        k3x = vs + (0.5 * h) * k2v
        k3v, k3w = f(xs + (0.5 * h) * k2x, k3x, ws + (0.5 * h) * k2w)
        k4x = vs + h * k3v
        k4v, k4w = f(xs + h * k3x, k4x, ws + h * k3w)
        xs = xs + (h / 6.0) * (k1x + 2.0 * k2x + 2.0 * k3x + k4x)
        vs = vs + (h / 6.0) * (k1v + 2.0 * k2v + 2.0 * k3v + k4v)
        ws = ws + (h / 6.0) * (k1w + 2.0 * k2w + 2.0 * k3w + k4w)
        curve[:, s + 1], vel[:, s + 1], frames[:, s + 1] = xs, vs, ws
    return curve, vel, frames, bad


def parallel_transport(transport, x, v, w, q, device, num_steps=64, return_curve=False):
    """The vectors w ([C x F x Q], or one per curve [C x Q] / [Q]) at the points x, moved by parallel transport along the
    geodesics exp_x(t v), t in [0, 1], to their ends: the frame at t = 1 in the shape of w, from the classical RK4 solution of
    (x', v', w_r') = (v, a, dw_r) at step 1 / S, S = num_steps (_rk4_transport; the loop runs on the host).  With return_curve
    (curve, velocity [C x S+1 x Q], frames [C x S+1 x F x Q]) (without the axes that x or w came without): curve and velocity are
    exp_map's, bit for bit; frames' row 0 holds the bits of w.  Transport keeps every <w_i, w_j>_G up to the integrator's error,
    and moves w = v as the velocity itself, bit for bit.  Four calls of transport per step; the stages' info is accumulated on
    the device and read ONCE at the end: FloatingPointError if the metric failed to factor at any stage of any curve."""
    (xs, vs), single = states_arg(q, device, x=x, v=v)
    ws, one = frames_arg(w, xs, single, q, device)
    num_steps = int(num_steps)
    assert num_steps >= 1, 'num_steps >= 1'
    with torch.no_grad():
        curve, vel, frames, bad = _rk4_transport(transport, xs, vs, ws, num_steps)
        failed = int(torch.count_nonzero(bad))
        if failed:
            raise FloatingPointError('latent_parallel_transport: the metric failed to factor (not positive definite in fp64) '
                                     'along %d of %d curves' % (failed, xs.shape[0]))
    if one:
        frames = frames[:, :, 0]
    if single:
        curve, vel, frames = curve[0], vel[0], frames[0]
    return (curve, vel, frames) if return_curve else frames[..., -1, :, :] if not one else frames[..., -1, :]


def transport_to(accel_tangent, transport, x_from, x_to, w, q, device, num_steps=64, max_iterations=20, tol=1e-10, shoot=None):
    """(w at x_to in the shape of w, v, distance, residual): the vectors w at x_from moved to x_to along the geodesic that joins
    them: log_map(x_from, x_to) finds its initial velocity v (with distance and residual as there; a pair that does not converge
    is reported through residual, and its vectors are moved along the geodesic that v does give), parallel_transport moves w
    along it at the same num_steps.  shoot: log_map's."""
    v, dist, _, res = log_map(accel_tangent, x_from, x_to, q, device, num_steps, max_iterations, tol, shoot=shoot)
    return parallel_transport(transport, x_from, v, w, q, device, num_steps), v, dist, res
