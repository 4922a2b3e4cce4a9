"""What the tests hold Phase C of the analytical gradient (excitation.constraint_gradients_from_rows, candidate_gradients_from_coefficients)
against: the soft costs f1 .. f4 and the constraint vector g of ONE candidate as plain functions of the optimiser's variable vector
[wf | q0 (n) | a_0 .. | b_0 ..] -- samples from the series of fourier_gradient_restatement, torques from np_dynamics (plus a friction model
whose Coulomb sign series is HELD at the unperturbed candidate's, as the gradient holds it), objective from objective_restatement -- and
their Richardson-extrapolated central differences.  Everything here is NumPy on the host."""
import numpy as np

import fourier_gradient_restatement as fr
from np_dynamics import inverse_dynamics_world
from objective_restatement import restate_from_samples

IDX = ("torque_absmax_idx", "pos_min_idx", "pos_max_idx", "vel_absmax_idx")
# Largest relative error (relative_error below) of constraint_gradients_from_rows fed with NumPy rows against the Richardson differences,
# over both problems of tests/test_constraint_gradient_host.py, as that test measured it (it prints the figure); the device comparison
# (tests/test_gpu_candidate_gradients.py) allows ten times this.
MEASURED_CPU_ERROR = 1.005e-6


class Problem:
    """``name`` robot, ``nf`` harmonics per joint, C candidates drawn from ``seed`` with coefficient amplitudes ``amps`` (one per candidate)"""

    def __init__(self, name, floating, bounded, T, freq, nf, amps, seed, config, friction=False, sign_threshold=0.02):
        from common import load_topo
        from flobaroid_amd import excitation as exc

        self.exc = exc
        self.topo = t = load_topo(name)
        self.floating, self.bounded, self.T, self.freq, self.config = bool(floating), bool(bounded), int(T), float(freq), dict(config)
        self.n = n = t.num_dofs
        self.fb = 6 if floating else 0
        self.nf = [int(nf)] * n
        self.names = list(t.dof_names)
        self.limits = t.limits
        self.lim = [(t.limits[j]["lower"], t.limits[j]["upper"]) for j in self.names]
        rng = np.random.default_rng(seed)
        self.xs = [np.concatenate([[rng.uniform(0.8, 1.2)], rng.uniform(-0.2, 0.2, n), rng.standard_normal(2 * n * nf) * amp]) for amp in amps]
        self.friction = bool(friction)
        self.sign_threshold = float(sign_threshold)
        self.x_std = np.concatenate([t.x_std(), rng.uniform(0.1, 0.5, 4 * n)]) if friction else t.x_std()
        self.times = np.arange(self.T, dtype=np.float64) / self.freq

    def candidate(self, x):
        n, k = self.n, self.nf[0]
        a = [x[1 + n + k * j:1 + n + k * (j + 1)] for j in range(n)]
        b = [x[1 + n + k * n + k * j:1 + n + k * n + k * (j + 1)] for j in range(n)]
        return self.exc.fourier_coefficients(a, b, x[1:1 + n], self.nf, wf=float(x[0]), joint_limits=self.lim if self.bounded else None)

    def samples(self, cand):
        cols = [fr.series(cand["wf"], cand["q_offset"][j], None if cand["q_range"] is None else cand["q_range"][j], cand["a"][j], cand["b"][j], self.times)
                for j in range(self.n)]
        return tuple(np.stack([c[i] for c in cols], axis=1) for i in range(3))

    def torques(self, q, dq, ddq, sign):
        """(S, fb + n): np_dynamics plus, with friction, sign Fc + Fv dq + offset on the joint rows (model.py:299-326, symmetric, no Stribeck)"""
        S, n = q.shape
        z = lambda k: np.zeros((S, k))  # noqa: E731
        tau = inverse_dynamics_world(self.topo, q, dq, ddq, self.floating, z(6), z(6), z(3), x_inertial=self.x_std[:10 * self.topo.num_links])
        if self.friction:
            f0 = 10 * self.topo.num_links
            tau[:, self.fb:] += sign * self.x_std[f0:f0 + n] + self.x_std[f0 + n:f0 + 2 * n] * dq + self.x_std[f0 + 2 * n:f0 + 3 * n]
        return tau

    def sign_series(self, dq):
        return np.tanh(dq / self.sign_threshold)

    def evaluate(self, x, sign=None):
        """restate_from_samples of the candidate x (D-optimality term 0); ``sign``: the Coulomb series to hold (None: the candidate's own)"""
        q, dq, ddq = self.samples(self.candidate(x))
        sign = self.sign_series(dq) if sign is None else sign
        out = restate_from_samples(0.0, q, dq, self.torques(q, dq, ddq, sign), self.fb, self.limits, self.names, self.config, 1.0)
        out.update(q=q, dq=dq, ddq=ddq, sign=sign)
        return out

    def vector(self, ev):
        """[f1, f2, f3, f4 | g]: what is differentiated"""
        return np.concatenate([[ev["f1"], ev["f2"], ev["f3"], ev["f4"]], ev["g"]])

    def richardson(self, x, h=1e-5):
        """d vector / d x (4 + len(g), n_vars) by central differences at h and h / 2, extrapolated; asserts that every stencil point has the
        extrema at the samples of x itself (the derivative of an extremum is the derivative at its sample only while that holds)"""
        base = self.evaluate(x)

        def at(xv):
            ev = self.evaluate(xv, sign=base["sign"])
            for k in IDX:
                assert np.array_equal(ev["idx"][k], base["idx"][k]), f"{k} moves inside the difference stencil: change the seed"
            return self.vector(ev)

        J = np.zeros((self.vector(base).size, x.size))
        for v in range(x.size):
            d = []
            for step in (h, h / 2):
                xp, xm = x.copy(), x.copy()
                xp[v] += step
                xm[v] -= step
                d.append((at(xp) - at(xm)) / (2 * step))
            J[:, v] = (4.0 * d[1] - d[0]) / 3.0
        return J, base

    # ---- the inputs of constraint_gradients_from_rows in NumPy -------------------------------------------------------------------------
    def ag_cache(self, evs):
        """the ``ag_cache`` entries of objectives_from_extrema for the candidates' evaluations, from excitation.objectives_from_extrema itself
        fed with NumPy extrema"""
        n = self.n
        ext = {}
        for key, fun in (("q_min", lambda e: e["q"].min(0)), ("q_max", lambda e: e["q"].max(0)), ("dq_absmax", lambda e: np.abs(e["dq"]).max(0)),
                         ("tau_absmax", lambda e: np.abs(self.torques(e["q"], e["dq"], e["ddq"], e["sign"])[:, self.fb:]).max(0))):
            ext[key] = np.stack([fun(e) for e in evs])
        for key, src in (("q_min_idx", "pos_min_idx"), ("q_max_idx", "pos_max_idx"), ("dq_absmax_idx", "vel_absmax_idx"), ("tau_absmax_idx", "torque_absmax_idx")):
            ext[key] = np.stack([e["idx"][src] for e in evs]).astype(np.int64)
        assert ext["q_min"].shape == (len(evs), n)
        return self.exc.objectives_from_extrema(np.zeros(len(evs)), np.zeros(len(evs)), ext, self.limits, self.names, self.config, 1.0)["ag_cache"]

    def torque_jacobians(self, evs, ag, eps):
        """candidate_torque_jacobians in NumPy: forward differences of ``torques`` at the sample of every joint's torque peak"""
        n, C = self.n, len(evs)
        sw = np.zeros((C, n, 1 + 3 * n))
        for c, e in enumerate(evs):
            s = ag["torque_absmax_idx"][c]
            st = [np.repeat(e[k][s], 1 + 3 * n, axis=0) for k in ("q", "dq", "ddq")]
            for j in range(n):
                for kind in range(3):
                    for d in range(n):
                        st[kind][j * (1 + 3 * n) + 1 + kind * n + d, d] += eps
            tau = self.torques(st[0], st[1], st[2], np.repeat(e["sign"][s], 1 + 3 * n, axis=0))[:, self.fb:]
            sw[c] = tau.reshape(n, 1 + 3 * n, n)[np.arange(n), :, np.arange(n)]
        d = (sw[..., 1:] - sw[..., :1]) / eps
        return {"tau": sw[..., 0], "dtau_dq": d[..., :n], "dtau_ddq_state": d[..., n:2 * n], "dtau_dddq": d[..., 2 * n:]}

    def chain(self, cands):
        """Engine.fourier_state_chain in NumPy (fourier_gradient_restatement.chain over one sample per row)"""
        def run(sample, gq, gdq, gddq):
            C, R = sample.shape
            n, nh = cands[0]["a"].shape
            out = np.zeros((C, R, 1 + 2 * n + 2 * n * nh))
            for c in range(C):
                for r in range(R):
                    out[c, r] = fr.chain(cands[c]["wf"], cands[c]["q_range"], cands[c]["a"], cands[c]["b"], gq[c, r][None], gdq[c, r][None],
                                         gddq[c, r][None], self.times[[sample[c, r]]], dtype=np.float64)[0]
            return out
        return run

    def to_variables(self, rows, c):
        """rows (..., E) of candidate c on the optimiser's variables, the bounded form with the exact q0 dependence"""
        n, nh = self.n, self.nf[0]
        rows = np.asarray(rows).reshape(-1, rows.shape[-1])
        grad = {"wf": rows[:, 0], "q_offset": rows[:, 1:1 + n], "q_range": rows[:, 1 + n:1 + 2 * n],
                "a": rows[:, 1 + 2 * n:1 + 2 * n + n * nh].reshape(-1, n, nh), "b": rows[:, 1 + 2 * n + n * nh:].reshape(-1, n, nh)}
        return self.exc.constraint_gradient_to_optimizer_variables(grad, self.candidate(self.xs[c]), self.nf, exact=self.bounded,
                                                                   joint_limits=self.lim if self.bounded else None,
                                                                   q0=self.xs[c][1:1 + n] if self.bounded else None)


def relative_error(got, ref):
    """max over the rows of |got - ref|_inf / |ref|_inf (a row that is zero in ref must be zero in got: it counts as its absolute error)"""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    scale = np.abs(ref).max(axis=1)
    return float((np.abs(got - ref).max(axis=1) / np.where(scale > 0, scale, 1.0)).max())


def kuka_classic(friction=False):
    config = {"minVelocityConstraint": True, "minVelocityPercentage": 0.1, "trajectoryTargetVelocity": 1.0, "trajectoryTargetTorqueUtil": 0.08}
    return Problem("kuka_lwr4", False, False, 96, 20.0, 2, (0.15, 0.5, 1.0), 4, config, friction=friction)


def three_links_floating_bounded():
    config = {"minVelocityConstraint": False, "trajectoryTargetVelocity": 1.3, "trajectoryTargetTorqueUtil": 0.25}
    return Problem("threeLinks", True, True, 96, 20.0, 2, (0.15, 0.5, 1.0), 6, config)


def walkman_arm_floating_bounded():
    config = {"minVelocityConstraint": True, "minVelocityPercentage": 0.1, "trajectoryTargetVelocity": 1.0, "trajectoryTargetTorqueUtil": 0.25}
    return Problem("walkman_left_arm", True, True, 96, 20.0, 2, (0.15, 0.5, 1.0), 9, config)


def assembled(p, out, c):
    """[df1, df2, df3, df4 | con_grad] of candidate c of a constraint_gradients_from_rows result, on the optimiser's variables: the rows
    Problem.richardson differentiates"""
    return np.concatenate([p.to_variables(np.stack([np.asarray(out[k][c]) for k in ("df1", "df2", "df3", "df4")]), c),
                           p.to_variables(np.asarray(out["con_grad"][c]), c)])
