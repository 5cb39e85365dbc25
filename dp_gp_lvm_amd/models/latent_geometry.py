"""
The latent-geometry surface of the four latent-variable models, written once: magnification, curve energy and length, geodesics
between two points, the geodesic acceleration and exponential map, their tangents, the logarithm map and parallel transport
along geodesics.  Every model's metric is
one marginals.Metric (a sum over parts b_k(x)^T P_k b_k(x) plus constant diagonal terms), so the methods differ between the models
only in how that value is built: a model supplies ONE hook from its closure and its own latent_metric, and models/geodesic.py does
the work on the Metric's four callables.

    LatentGeometry        bayesian_gp_lvm, dp_gp_lvm, dp_gp_lvm_t (columns=): the hook _metric_of(columns, name) -> Metric
    ViewsLatentGeometry   manifold_relevance_determination (views=, total=): the hook _metrics_of(views, total) -> [Metric, ...]

Both need the class attributes _latent_dims (Q) and _device.  What is specific to a model (which kernels a call runs over, whether
a sharded model is refused) is said in that model's class docstring.
"""
import torch

from . import geodesic as _geodesic
from . import marginals as _marginals


def _shoot_of(metric, where, tangent=False):
    """The `shoot` of models/geodesic.py's integrating functions for a model's integrator `where`: 'host' (None: their own loop,
    a stage is a handful of launches from Python) or 'device' (the metric's shoot / shoot_tangent: ops.geodesic_shoot[_tangent],
    every stage of every step from one C call, the same bits)."""
    if where == 'host':
        return None
    return metric.shoot_tangent if tangent else metric.shoot


class _Integrator:
    """The attribute `integrator` of a model: where the Runge-Kutta loops of latent_exp_map, latent_exp_map_tangent and
    latent_log_map run.  'host' (the default: the Python loops of models/geodesic.py) or 'device' (the same steps, to the same
    bits, from one C call per shot); assigning anything else raises ValueError.  An attribute and not a keyword
    of the three methods: their signatures are pinned.  The loop of latent_parallel_transport (and of the transport half of
    latent_transport_to) runs on the host whatever the value: there is no transport shot on the device yet."""
    _integrator = 'host'

    @property
    def integrator(self):
        return self._integrator

    @integrator.setter
    def integrator(self, value):
        if value not in ('host', 'device'):
            raise ValueError("integrator must be 'host' or 'device', got %r" % (value,))
        self._integrator = value


class LatentGeometry(_Integrator):
    """The methods of a model whose geometry calls choose output dims by columns= (default: all D).  _metric_of(columns, name):
    the checks of `columns`, the training side and the Metric under latent_metric(., columns), formed once per call; `name` is
    the public method's, for a refusal's text.  _require_built(name) raises where a model in its current state builds none of
    this (here: never)."""

    def _require_built(self, name):
        pass

    def magnification(self, x, columns=None):
        """[N*]: the magnification factor sqrt(det G(x)) of latent_metric(x, columns), the volume element of the learnt map
        (what GPy draws as plot_magnification), as exp(1/2 logdet) from a Cholesky factorisation of G."""
        self._require_built('magnification')
        with torch.no_grad():
            return _marginals.magnification(self.latent_metric(x, columns))

    def curve_energy(self, curve, columns=None, return_gradient=False):
        """E [C] of the curves `curve` [C x S+1 x Q] (or one curve [S+1 x Q]; numpy or torch) under latent_metric(., columns):
        E = S sum_i v_i^T G(x_i) v_i over the segments' midpoints x_i and directions v_i (models/geodesic.py).  With
        return_gradient also dE / dcurve in the shape of `curve`.  One call of ops.ard_rbf_point_energy on the C S segments;
        the training side is built once per call.  fp64, torch.no_grad."""
        metric = self._metric_of(columns, 'curve_energy')
        return _geodesic.curve_energy(metric.curve_terms, curve, self._latent_dims, self._device, return_gradient)

    def curve_length(self, curve, columns=None):
        """L [C] = sum_i sqrt(v_i^T G(x_i) v_i) of the curves `curve`, as curve_energy (L^2 <= E)."""
        return _geodesic.curve_length(self._metric_of(columns, 'curve_length').curve_terms, curve, self._latent_dims, self._device)

    def latent_geodesic(self, x_from, x_to, num_segments=32, num_iterations=200, learning_rate=0.01, columns=None, init=None):
        """(curve [C x S+1 x Q], length [C], energy [C]): discrete geodesics under latent_metric(., columns) between the
        latent points x_from and x_to ([C x Q] or [Q]), S = num_segments: the curve energy minimised over the interior points
        by Adam from the straight line (or from `init` [C x S+1 x Q]), the end points fixed; each curve's lowest-energy
        iterate is returned, so its energy never exceeds the start's.  The training side is built once per call; an iteration
        is one call of ops.ard_rbf_point_energy plus element-wise work.  fp64."""
        metric = self._metric_of(columns, 'latent_geodesic')
        return _geodesic.latent_geodesic(metric.curve_terms, x_from, x_to, self._latent_dims, self._device, num_segments,
                                         num_iterations, learning_rate, init)

    def geodesic_acceleration(self, x, v, columns=None):
        """a [N* x Q] (or [Q]): the acceleration x'' = -G(x)^-1 Gamma(x, v) of the geodesic through the latent points x with
        the velocities v ([N* x Q] or [Q]; numpy or torch) under latent_metric(., columns), Gamma the Christoffel symbols of
        the first kind contracted twice with v (models/marginals.Metric.accel).  One call of
        ops.ard_rbf_point_christoffel and one of ops.geodesic_accel; the training side is built once per call.  fp64,
        torch.no_grad."""
        metric = self._metric_of(columns, 'geodesic_acceleration')
        return _geodesic.geodesic_acceleration(metric.accel, x, v, self._latent_dims, self._device)

    def latent_exp_map(self, x, v, num_steps=64, columns=None, return_velocity=False):
        """curve [C x num_steps+1 x Q] (or [num_steps+1 x Q] for x, v [Q]): the exponential map of the velocities v at the
        latent points x under latent_metric(., columns): the classical RK4 solution of (x', v') = (v, -G^-1 Gamma) on
        t in [0, 1], all C curves in one batch (models/geodesic.exp_map); row 0 holds the bits of x, and the curve is what
        curve_energy, curve_length, predictive_marginals and sample_functions take.  With return_velocity also the
        velocities, in the same shape.  A stage is one call of ops.ard_rbf_point_christoffel and one of ops.geodesic_accel
        plus element-wise work; the training side is built once per call; one host read at the end: FloatingPointError if the
        metric failed to factor at any stage.  With self.integrator = 'device' the same steps run, to the same bits, inside ONE
        call of ops.geodesic_shoot.  fp64, torch.no_grad."""
        metric = self._metric_of(columns, 'latent_exp_map')
        return _geodesic.exp_map(metric.accel, x, v, self._latent_dims, self._device, num_steps, return_velocity,
                                 shoot=_shoot_of(metric, self.integrator))

    def geodesic_deviation(self, x, v, dx, dv, columns=None):
        """(a, da) [N* x Q] (or [Q]): geodesic_acceleration(x, v, columns), with its bits, and its derivative along the
        direction (dx, dv) of the state (x, v): the right-hand side of the Jacobi equation of latent_metric(., columns), in
        closed form (no differencing).  One call of ops.ard_rbf_point_christoffel_tangent and one of
        ops.geodesic_accel_tangent; the training side is built once per call.  Q <= 31.  fp64, torch.no_grad."""
        metric = self._metric_of(columns, 'geodesic_deviation')
        return _geodesic.geodesic_deviation(metric.accel_tangent, x, v, dx, dv, self._latent_dims, self._device)

    def latent_exp_map_tangent(self, x, v, dx, dv, num_steps=64, columns=None, return_velocity=False):
        """(curve, dcurve) [C x num_steps+1 x Q] (or [num_steps+1 x Q]): latent_exp_map(x, v, num_steps, columns), with its
        bits, and the discrete Jacobi field started at (dx, dv): the tangent-linear RK4, the exact derivative of
        latent_exp_map's discrete map along that direction (models/geodesic.exp_map_tangent).  With return_velocity
        (curve, dcurve, velocity, dvelocity).  One host read at the end: FloatingPointError if the metric failed to factor at
        any stage.  self.integrator: as latent_exp_map ('device': ops.geodesic_shoot_tangent).  Q <= 31.  fp64, torch.no_grad."""
        metric = self._metric_of(columns, 'latent_exp_map_tangent')
        return _geodesic.exp_map_tangent(metric.accel_tangent, x, v, dx, dv, self._latent_dims, self._device, num_steps,
                                         return_velocity, shoot=_shoot_of(metric, self.integrator, True))

    def latent_log_map(self, x_from, x_to, num_steps=64, max_iterations=20, tol=1e-10, columns=None, init=None):
        """(v [C x Q], distance [C], curve [C x num_steps+1 x Q], residual [C]) (unbatched for x_from, x_to [Q]): the
        logarithm map of x_to at x_from under latent_metric(., columns), the inverse of latent_exp_map at the same num_steps:
        Newton shooting on the discrete map with latent_exp_map_tangent's exact Jacobian, step halving on a residual that
        does not fall, the best iterate kept (models/geodesic.log_map).  distance = sqrt(v^T G(x_from) v); residual =
        |curve end - x_to|, converged where it is <= tol max(1, |x_to|); a curve that is not is reported through residual,
        not raised.  An iteration is ONE batched shot over C Q rows and one host read; self.integrator = 'device' fires every shot
        through ops.geodesic_shoot_tangent, as latent_exp_map_tangent's.  Q <= 31.  fp64, torch.no_grad."""
        metric = self._metric_of(columns, 'latent_log_map')
        return _geodesic.log_map(metric.accel_tangent, x_from, x_to, self._latent_dims, self._device, num_steps, max_iterations,
                                 tol, init, shoot=_shoot_of(metric, self.integrator, True))

    def parallel_transport_rate(self, x, v, w, columns=None):
        """(a, dw): geodesic_acceleration(x, v, columns), with its bits, and the rates w_r' = -G(x)^-1 Gamma(x; v, w_r) of the
        vectors w in parallel transport along the geodesics through x with the velocities v under latent_metric(., columns):
        the right-hand side of the transport equation, Gamma the Christoffel symbols of the first kind contracted with v and
        w_r, in closed form.  w: a frame [N* x F x Q], or one vector per point [N* x Q] ([Q] with x, v [Q]); dw comes in the
        shape of w.  One call of ops.ard_rbf_point_transport and one of ops.geodesic_transport, whatever F; the training side
        is built once per call.  Q + 1 + F <= 64.  fp64, torch.no_grad."""
        metric = self._metric_of(columns, 'parallel_transport_rate')
        return _geodesic.parallel_transport_rate(metric.transport, x, v, w, self._latent_dims, self._device)

    def latent_parallel_transport(self, x, v, w, num_steps=64, columns=None, return_curve=False):
        """The vectors w at the latent points x after parallel transport along the geodesics exp_x(t v), t in [0, 1], under
        latent_metric(., columns): the frame at t = 1 in the shape of w ([C x F x Q], or one vector per curve [C x Q] / [Q]), the
        classical RK4 solution of (x', v', w_r') = (v, -G^-1 Gamma(v, v), -G^-1 Gamma(v, w_r)) at step 1 / num_steps
        (models/geodesic.parallel_transport).  With return_curve (curve, velocity, frames), every step's state: curve and
        velocity are latent_exp_map(x, v, num_steps, columns, return_velocity=True), bit for bit; frames' row 0 holds the bits
        of w.  Transport keeps the inner products <w_i, w_j>_G up to the integrator's error (fourth order) and moves w = v as
        the velocity itself.  A stage is one call of ops.ard_rbf_point_transport and one of ops.geodesic_transport for the
        whole frame; one host read at the end: FloatingPointError if the metric failed to factor at any stage.  The loop runs
        on the host whatever self.integrator says.  Q + 1 + F <= 64.  fp64, torch.no_grad."""
        metric = self._metric_of(columns, 'latent_parallel_transport')
        return _geodesic.parallel_transport(metric.transport, x, v, w, self._latent_dims, self._device, num_steps, return_curve)

    def latent_transport_to(self, x_from, x_to, w, num_steps=64, max_iterations=20, tol=1e-10, columns=None):
        """(w at x_to, v, distance, residual): the vectors w at x_from ([C x F x Q], [C x Q] or [Q]) moved to x_to along the
        geodesic that joins them under latent_metric(., columns): latent_log_map(x_from, x_to, num_steps, max_iterations, tol,
        columns) gives v, distance and residual, latent_parallel_transport moves w along exp_{x_from}(t v) at the same
        num_steps.  A pair that does not converge is reported through residual, as in the logarithm map.  self.integrator
        governs the logarithm map's shots; the transport loop runs on the host.  Q <= 31.  fp64, torch.no_grad."""
        metric = self._metric_of(columns, 'latent_transport_to')
        return _geodesic.transport_to(metric.accel_tangent, metric.transport, x_from, x_to, w, self._latent_dims, self._device,
                                      num_steps, max_iterations, tol, shoot=_shoot_of(metric, self.integrator, True))


class ViewsLatentGeometry(_Integrator):
    """The methods of manifold_relevance_determination: one result per view of `views` (default: all V, in order), each under the
    view's own latent_metric, or, with total=True, ONE result under the summed metric latent_metric(., views, total=True).
    _metrics_of(views, total): the check of `views`, the training side of all views and the Metrics, one per view or the one of
    their sum (the views' slabs then go to one factorisation), formed once per call."""

    def _per_metric(self, views, total, run):
        """run(metric) of every Metric of the call as a list, or its only entry with total."""
        out = [run(metric) for metric in self._metrics_of(views, total)]
        return out[0] if total else out

    def magnification(self, x, views=None):
        """One magnification factor sqrt(det G_v(x)) [N*] per view of `views` (default: all V, in order)."""
        with torch.no_grad():
            return [_marginals.magnification(g) for g in self.latent_metric(x, views)]

    def curve_energy(self, curve, views=None, total=False, return_gradient=False):
        """One curve energy E [C] per view of `views` (default: all V, in order) of the curves `curve` [C x S+1 x Q] (or one
        curve [S+1 x Q]), as bayesian_gp_lvm.curve_energy under the view's latent_metric; with return_gradient one pair
        (E, dE / dcurve) per view.  total=True: one result, under the summed metric latent_metric(., views, total=True)."""
        return self._per_metric(views, total, lambda m: _geodesic.curve_energy(
            m.curve_terms, curve, self._latent_dims, self._device, return_gradient))

    def curve_length(self, curve, views=None, total=False):
        """One curve length L [C] per view of `views`, as bayesian_gp_lvm.curve_length; total=True: under the summed metric."""
        return self._per_metric(views, total, lambda m: _geodesic.curve_length(
            m.curve_terms, curve, self._latent_dims, self._device))

    def latent_geodesic(self, x_from, x_to, num_segments=32, num_iterations=200, learning_rate=0.01, views=None, total=False,
                        init=None):
        """One triple (curve [C x S+1 x Q], length [C], energy [C]) per view of `views`: the view's own geodesics, as
        bayesian_gp_lvm.latent_geodesic under the view's latent_metric; total=True: one triple, the geodesics under the
        summed metric.  The training side of all views is built once per call."""
        return self._per_metric(views, total, lambda m: _geodesic.latent_geodesic(
            m.curve_terms, x_from, x_to, self._latent_dims, self._device, num_segments, num_iterations, learning_rate, init))

    def geodesic_acceleration(self, x, v, views=None, total=False):
        """One acceleration a [N* x Q] (or [Q]) per view of `views` (default: all V, in order), as
        bayesian_gp_lvm.geodesic_acceleration under the view's latent_metric; total=True: one result, under the summed
        metric latent_metric(., views, total=True).  The training side of all views is built once per call."""
        return self._per_metric(views, total, lambda m: _geodesic.geodesic_acceleration(
            m.accel, x, v, self._latent_dims, self._device))

    def latent_exp_map(self, x, v, num_steps=64, views=None, total=False, return_velocity=False):
        """One curve [C x num_steps+1 x Q] (or [num_steps+1 x Q]; with return_velocity one pair (curve, velocities)) per view
        of `views`: the view's own exponential map, as bayesian_gp_lvm.latent_exp_map under the view's latent_metric;
        total=True: one result, under the summed metric (a stage is then one ops.ard_rbf_point_christoffel call per view and
        one ops.geodesic_accel).  The training side of all views is built once per call.  self.integrator: 'host' or 'device', as
        bayesian_gp_lvm's (the summed metric's views are the parts of one ops.geodesic_shoot call)."""
        return self._per_metric(views, total, lambda m: _geodesic.exp_map(
            m.accel, x, v, self._latent_dims, self._device, num_steps, return_velocity, shoot=_shoot_of(m, self.integrator)))

    def geodesic_deviation(self, x, v, dx, dv, views=None, total=False):
        """One pair (a, da) per view of `views` (default: all V, in order), as bayesian_gp_lvm.geodesic_deviation under the
        view's latent_metric; total=True: one pair, under the summed metric.  The training side of all views is built once
        per call."""
        return self._per_metric(views, total, lambda m: _geodesic.geodesic_deviation(
            m.accel_tangent, x, v, dx, dv, self._latent_dims, self._device))

    def latent_exp_map_tangent(self, x, v, dx, dv, num_steps=64, views=None, total=False, return_velocity=False):
        """One result (curve, dcurve[, velocity, dvelocity]) per view of `views`, as bayesian_gp_lvm.latent_exp_map_tangent
        under the view's latent_metric; total=True: one result, under the summed metric (a stage is then one
        ops.ard_rbf_point_christoffel_tangent call per view and one ops.geodesic_accel_tangent).  self.integrator: as
        latent_exp_map."""
        return self._per_metric(views, total, lambda m: _geodesic.exp_map_tangent(
            m.accel_tangent, x, v, dx, dv, self._latent_dims, self._device, num_steps, return_velocity,
            shoot=_shoot_of(m, self.integrator, True)))

    def latent_log_map(self, x_from, x_to, num_steps=64, max_iterations=20, tol=1e-10, views=None, total=False, init=None):
        """One result (v, distance, curve, residual) per view of `views`: the view's own logarithm map, as
        bayesian_gp_lvm.latent_log_map under the view's latent_metric; total=True: one result, under the summed metric.
        The training side of all views is built once per call.  self.integrator: as latent_exp_map."""
        return self._per_metric(views, total, lambda m: _geodesic.log_map(
            m.accel_tangent, x_from, x_to, self._latent_dims, self._device, num_steps, max_iterations, tol, init,
            shoot=_shoot_of(m, self.integrator, True)))

    def parallel_transport_rate(self, x, v, w, views=None, total=False):
        """One pair (a, dw) per view of `views` (default: all V, in order), as bayesian_gp_lvm.parallel_transport_rate under the
        view's latent_metric; total=True: one pair, under the summed metric (one ops.ard_rbf_point_transport call per view and
        one ops.geodesic_transport).  The training side of all views is built once per call."""
        return self._per_metric(views, total, lambda m: _geodesic.parallel_transport_rate(
            m.transport, x, v, w, self._latent_dims, self._device))

    def latent_parallel_transport(self, x, v, w, num_steps=64, views=None, total=False, return_curve=False):
        """One transported frame (with return_curve one triple (curve, velocity, frames)) per view of `views`, as
        bayesian_gp_lvm.latent_parallel_transport under the view's latent_metric; total=True: one result, under the summed
        metric.  The loop runs on the host whatever self.integrator says."""
        return self._per_metric(views, total, lambda m: _geodesic.parallel_transport(
            m.transport, x, v, w, self._latent_dims, self._device, num_steps, return_curve))

    def latent_transport_to(self, x_from, x_to, w, num_steps=64, max_iterations=20, tol=1e-10, views=None, total=False):
        """One result (w at x_to, v, distance, residual) per view of `views`, as bayesian_gp_lvm.latent_transport_to under the
        view's latent_metric; total=True: one result, under the summed metric.  self.integrator governs the logarithm map's
        shots; the transport loop runs on the host."""
        return self._per_metric(views, total, lambda m: _geodesic.transport_to(
            m.accel_tangent, m.transport, x_from, x_to, w, self._latent_dims, self._device, num_steps, max_iterations, tol,
            shoot=_shoot_of(m, self.integrator, True)))
