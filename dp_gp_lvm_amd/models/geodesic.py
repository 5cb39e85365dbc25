"""
Discrete curves in latent space under the expected metric G(x) of models/marginals.py (Tosi et al., UAI 2014): energy, length and
geodesics.  A curve is S + 1 points c_0 .. c_S [Q]; segment i has the midpoint x_i = (c_i + c_{i+1}) / 2 and the direction
v_i = c_{i+1} - c_i, and with e_i = v_i^T G(x_i) v_i

    energy  E = S sum_i e_i            (the Riemann sum of int_0^1 |c'(t)|_G^2 dt at step 1 / S)
    length  L = sum_i sqrt(e_i)        (L^2 <= E by Cauchy-Schwarz, with equality at constant speed)
    dE / dc_j = S [ (dx_{j-1} / 2 + dv_{j-1}) + (dx_j / 2 - dv_j) ],    dx_i = de_i / dx_i,  dv_i = de_i / dv_i

(a segment moves its midpoint by half of either end and its direction by -/+ the end).  A minimiser of E between fixed ends is a
discrete geodesic.  Everything here works on `terms`, a callable (x [N,Q], v [N,Q]) -> (e [N], dx [N,Q], dv [N,Q]) that a model
builds ONCE per call from its training side (marginals._Marginals.curve_terms on ops.ard_rbf_point_energy): C curves are one
call with N = C S, and an iteration of latent_geodesic is one call plus element-wise work.  fp64, no autograd.

The initial-value side: a geodesic obeys G x'' = -Gamma(x, x'), Gamma the Christoffel symbols of the first kind contracted twice
with the velocity.  exp_map integrates (x', v') = (v, -G^-1 Gamma) over t in [0, 1] by the classical Runge-Kutta scheme on `accel`,
a callable (x [N,Q], v [N,Q]) -> (a [N,Q], speed [N], info [N]) that a model builds ONCE per call
(marginals.geodesic_terms on ops.ard_rbf_point_christoffel and ops.geodesic_accel): C curves are one batch, a stage is one call.
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


def sum_terms(all_terms):
    """The terms of a sum of metrics."""
    def terms(x, v):
        out = [t(x, v) for t in all_terms]
        return tuple(torch.sum(torch.stack(parts), dim=0) if len(parts) > 1 else parts[0] for parts in zip(*out))
    return terms


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
    a, b = ends_arg(x_from, q, device, 'x_from'), ends_arg(x_to, q, device, 'x_to')
    assert a.shape == b.shape, 'x_from and x_to must have the same shape'
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


def prior_accel(v, weight):
    """accel's triple under a constant diagonal metric diag(weight [Q]): straight lines, (0, sum_q weight_q v_q^2, 0)."""
    return torch.zeros_like(v), torch.sum(v * v * weight, dim=1), torch.zeros(v.shape[0], dtype=torch.int32, device=v.device)


def geodesic_acceleration(accel, x, v, q, device):
    """a [N* x Q] (or [Q] for one point): x'' of the geodesics through x with the velocities v ([N* x Q] or [Q])."""
    single = (x.dim() if torch.is_tensor(x) else np.asarray(x).ndim) == 1
    xs, vs = ends_arg(x, q, device, 'x'), ends_arg(v, q, device, 'v')
    assert xs.shape == vs.shape, 'x and v must have the same shape'
    with torch.no_grad():
        a = accel(xs, vs)[0]
    return a[0] if single else a


def exp_map(accel, x, v, q, device, num_steps=64, return_velocity=False):
    """curve [C x S+1 x Q] (one curve [S+1 x Q] for x, v [Q]), S = num_steps: the exponential map of v at x, the classical RK4
    solution of (x', v') = (v, accel(x, v)) on t in [0, 1] at step 1 / S, all C curves in one batch; row 0 holds the bits of x.
    With return_velocity also the velocities in the same shape.  Four calls of accel per step plus element-wise work; nothing is
    read on the host until ONE read of the accumulated info at the end: FloatingPointError if the metric failed to factor at
    any stage of any curve."""
    single = (x.dim() if torch.is_tensor(x) else np.asarray(x).ndim) == 1
    xs, vs = ends_arg(x, q, device, 'x'), ends_arg(v, q, device, 'v')
    assert xs.shape == vs.shape, 'x and v must have the same shape'
    num_steps = int(num_steps)
    assert num_steps >= 1, 'num_steps >= 1'
    c, h = xs.shape[0], 1.0 / num_steps
    with torch.no_grad():
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
        failed = int(torch.count_nonzero(bad))
        if failed:
            raise FloatingPointError('latent_exp_map: the metric failed to factor (not positive definite in fp64) along %d of %d '
                                     'curves' % (failed, c))
    if single:
        curve, vel = curve[0], vel[0]
    return (curve, vel) if return_velocity else curve
