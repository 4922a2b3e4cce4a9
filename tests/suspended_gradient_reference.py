"""What the tests hold the gradient entry points of excitation under ``suspended=`` against (tests/test_suspended_gradient_host.py,
tests/test_gpu_suspended_gradients.py): constraint_gradient_reference.Problem with a base state.  The torques come from
np_dynamics.inverse_dynamics_world at a given base state; the base state of a candidate from suspended_restatement.simulate_from_records.

* ``"held"``: the Richardson differences of the objective with the base arrays FROZEN at those of the unperturbed candidate
  (``richardson_held``: Problem.richardson, extrema pinned to their samples, on ``evaluate_held``).
* ``"identity"`` (the reference's rule, analyticalGradient.py:107-125): the position and velocity rows are those of ``"held"``; a torque row
  is sign(tau_swung) times the Richardson derivative of ``row_identity`` -- joint n's torque at the REST base (rpy, base twist, base
  acceleration zero) at the fixed sample where the SWUNG torque peaks; df1 and df3 are the reference's combinations of those rows, restated
  here from the swung utilisations (``identity_jacobian``).

Everything is NumPy on the host; nothing of the code under test is called but fourier_coefficients and objectives_from_extrema (through
Problem, as constraint_gradient_reference does)."""
import numpy as np

import constraint_gradient_reference as cgr
import suspended_restatement as sr
from np_dynamics import inverse_dynamics_world

BASE_KEYS = ("rpy", "base_vel", "base_acc")
# Largest relative error (constraint_gradient_reference.relative_error) of constraint_gradients_from_rows(..., suspended=) fed with NumPy
# rows against the yardsticks above, over both problems below, as tests/test_suspended_gradient_host.py measured it (it prints the figures
# and asserts that they stay within twice these); the device comparison (tests/test_gpu_suspended_gradients.py) allows ten times these.
MEASURED_CPU_ERROR_HELD = 3.372e-7
MEASURED_CPU_ERROR_IDENTITY = 2.069e-7


class SuspendedProblem(cgr.Problem):
    """``Problem`` on a floating base hanging from link ``att`` with ball-joint ``damping``"""

    def __init__(self, name, att, damping, bounded, T, freq, nf, amps, seed, config):
        super().__init__(name, True, bounded, T, freq, nf, amps, seed, dict(config, floatingBaseAttachment="suspended"))
        self.att_name, self.att, self.damping = att, list(self.topo.link_names).index(att), float(damping)
        self.spec = {"attachment_frame": att, "damping": self.damping, "x_std": self.x_std}
        self._base = None

    def base(self, x):
        """the simulated base motion of candidate x: rpy (T, 3), base_vel, base_acc (T, 6), base_position (T, 3), info (1, 2)"""
        q, dq, ddq = self.samples(self.candidate(x))
        return sr.simulate_from_records(sr.sample_records(self.topo, self.att, q, dq, ddq), 1, 1.0 / self.freq, self.damping)

    def rest(self, S):
        return {"rpy": np.zeros((S, 3)), "base_vel": np.zeros((S, 6)), "base_acc": np.zeros((S, 6))}

    def torques_at(self, q, dq, ddq, base):
        return inverse_dynamics_world(self.topo, q, dq, ddq, True, base["base_vel"], base["base_acc"], base["rpy"],
                                      x_inertial=self.x_std[:10 * self.topo.num_links])

    def torques(self, q, dq, ddq, sign):
        """at the base arrays ``evaluate_held`` froze (the rest base without)"""
        return self.torques_at(q, dq, ddq, self._base if self._base is not None else self.rest(q.shape[0]))

    def evaluate_held(self, x, base, sign=None):
        """restate_from_samples of candidate x with the base arrays of ``base`` (T rows), whatever x is"""
        self._base = base
        try:
            out = cgr.Problem.evaluate(self, x, sign)
            out["tau"] = self.torques(out["q"], out["dq"], out["ddq"], out["sign"])
        finally:
            self._base = None
        return out

    def richardson_held(self, x, base=None, h=1e-5):
        """``Problem.richardson`` of the frozen-base objective: (J, the evaluation at x, the base arrays)"""
        base = self.base(x) if base is None else base
        self._base = base
        try:
            J, ev = self.richardson(x, h)
            ev["tau"] = self.torques(ev["q"], ev["dq"], ev["ddq"], ev["sign"])
        finally:
            self._base = None
        return J, ev, base

    def rows_identity(self, x, samples):
        """(n,): joint n's torque at the rest base at the fixed sample samples[n] of candidate x (one torque call over the n samples)"""
        cand, t = self.candidate(x), self.times[np.asarray(samples)]
        cols = [cgr.fr.series(cand["wf"], cand["q_offset"][j], None if cand["q_range"] is None else cand["q_range"][j], cand["a"][j], cand["b"][j], t)
                for j in range(self.n)]
        q, dq, ddq = (np.stack([c[i] for c in cols], axis=1) for i in range(3))  # (Problem.samples at those times)
        return self.torques_at(q, dq, ddq, self.rest(len(t)))[np.arange(len(t)), self.fb + np.arange(self.n)]

    def row_identity(self, x, n, s):
        """joint n's torque at the rest base at the fixed sample s of candidate x"""
        return float(self.rows_identity(x, [s] * self.n)[n])

    def richardson_rows_identity(self, x, samples, h=1e-5):
        """d row_identity(., n, samples[n]) / d x for every joint: (n, n_vars), central differences at h and h / 2, extrapolated"""
        J = np.zeros((self.n, x.size))
        for v in range(x.size):
            d = []
            for step in (h, h / 2):
                xp, xm = x.copy(), x.copy()
                xp[v] += step
                xm[v] -= step
                d.append((self.rows_identity(xp, samples) - self.rows_identity(xm, samples)) / (2 * step))
            J[:, v] = (4.0 * d[1] - d[0]) / 3.0
        return J

    def identity_jacobian(self, x, J_held, ev):
        """The yardstick of the reference's rule in the layout of ``Problem.richardson`` ([f1, f2, f3, f4 | g]): ``J_held`` with the torque
        rows, the minimum-utilisation rows, df1 and df3 replaced.  ``ev``: the frozen-base evaluation at x (its ``tau`` are the swung
        torques: peak samples, signs, utilisations)."""
        n, fb = self.n, self.fb
        lay = self.exc.constraint_layout(n, bool(self.config.get("minVelocityConstraint", False)))
        s = ev["idx"]["torque_absmax_idx"]
        peak = ev["tau"][s, fb + np.arange(n)]
        dT = np.sign(peak)[:, None] * self.richardson_rows_identity(x, s)
        tlim = np.array([self.limits[j]["torque"] for j in self.names])
        util = np.abs(peak) / tlim
        mean, std = util.mean(), util.std()
        dutil = dT / tlim[:, None]
        J = J_held.copy()
        f1 = std / mean
        J[0] = ((((util - mean) / std - f1) / (n * mean))[:, None] * dutil).sum(0) if mean > 0 and std > 0 else 0.0
        J[2] = -dutil.mean(0) / self.config.get("trajectoryTargetTorqueUtil", 0.25) if ev["f3"] > 0 else 0.0
        J[4 + lay["torque"]:4 + lay["torque"] + n] = dT
        J[4 + lay["min_torque_util"]:4 + lay["min_torque_util"] + n] = -dT
        return J

    # ---- the inputs of constraint_gradients_from_rows in NumPy -------------------------------------------------------------------------
    def ag_cache(self, evs):
        """``Problem.ag_cache`` with the torque extrema of the evaluations' own (swung) torques"""
        ext = {"q_min": np.stack([e["q"].min(0) for e in evs]), "q_max": np.stack([e["q"].max(0) for e in evs]),
               "dq_absmax": np.stack([np.abs(e["dq"]).max(0) for e in evs]), "tau_absmax": np.stack([np.abs(e["tau"][:, self.fb:]).max(0) for e in evs])}
        for key, src in (("q_min_idx", "pos_min_idx"), ("q_max_idx", "pos_max_idx"), ("dq_absmax_idx", "vel_absmax_idx"), ("tau_absmax_idx", "torque_absmax_idx")):
            ext[key] = np.stack([e["idx"][src] for e in evs]).astype(np.int64)
        z = np.zeros(len(evs))
        return self.exc.objectives_from_extrema(z, z, ext, self.limits, self.names, self.config, 1.0, suspended=self.spec)["ag_cache"]

    def torque_jacobians_at(self, evs, bases, ag, eps, rest_base):
        """candidate_torque_jacobians(..., rest_base=) in NumPy: ``tau`` at the swung base of the peak sample, the forward differences at
        that base (``rest_base`` False) or at the rest base (True)"""
        n, C, R = self.n, len(evs), 1 + 3 * self.n
        sw, tau = np.zeros((C, n, R)), np.zeros((C, n))
        for c, (e, b) in enumerate(zip(evs, bases)):
            s = ag["torque_absmax_idx"][c]
            st = [np.repeat(e[k][s], R, axis=0) for k in ("q", "dq", "ddq")]
            for j in range(n):
                for kind in range(3):
                    for d in range(n):
                        st[kind][j * R + 1 + kind * n + d, d] += eps
            swung = {k: np.repeat(b[k][s], R, axis=0) for k in BASE_KEYS}
            t = self.torques_at(st[0], st[1], st[2], self.rest(n * R) if rest_base else swung)[:, self.fb:]
            sw[c] = t.reshape(n, R, n)[np.arange(n), :, np.arange(n)]
            tau[c] = e["tau"][s, self.fb + np.arange(n)]
        d = (sw[..., 1:] - sw[..., :1]) / eps
        return {"tau": tau, "dtau_dq": d[..., :n], "dtau_ddq_state": d[..., n:2 * n], "dtau_dddq": d[..., 2 * n:]}


CONFIG = {"minVelocityConstraint": True, "minVelocityPercentage": 0.1, "trajectoryTargetVelocity": 1.0, "trajectoryTargetTorqueUtil": 0.25}


def walkman_arm_suspended(seed=0, amps=(0.2, 0.2, 0.2), target_util=0.25):
    """the case of tests/test_gpu_suspended_objectives.py: the left arm floating, hung from LShy, damping 500, 3 candidates of 48 samples
    at 100 Hz (classic series)"""
    return SuspendedProblem("walkman_left_arm", "LShy", 500.0, False, 48, 100.0, 2, amps, seed, dict(CONFIG, trajectoryTargetTorqueUtil=target_util))


def three_links_suspended(seed=0, amps=(0.3, 0.6, 1.0), target_util=0.25, damping=50.0):
    """threeLinks floating (n = 2) hung from its last link; 65 samples: a candidate straddles a wave (bounded series)"""
    from common import load_topo

    last = list(load_topo("threeLinks").link_names)[-1]
    return SuspendedProblem("threeLinks", last, damping, True, 65, 100.0, 2, amps, seed,
                            dict(CONFIG, minVelocityConstraint=False, trajectoryTargetVelocity=1.3, trajectoryTargetTorqueUtil=target_util))
