"""Shared by test_stage_function_xu_host.py, test_oracle_stage_function_xu.py and test_gpu_stage_function_xu.py (imported like conftest -- tests/ is on
the path): the state-control stage functions of csrc/stage_functions/ (slot 2 drive_power, slot 3 input_envelope) written out in numpy in the headers'
operation order, the descriptors and starts of the cases, and the reference of the iterate tests.

No fixture of the genuine reference pins this term (the reference driver under oracle/ does not know it).  The reference here is oracle.GenericProblem --
the same oracle_solve as the OCPs -- on a callback that stacks the unchanged OCP oracle's rows of the descriptor WITHOUT the term with the term's rows from
the host evaluator (corbo_hip_eval_stage_function_xu: the header the kernels compile), inserted where the reference creates the edge: behind the interval's
state and control terms, in front of its control-deviation rows (nlp_functions.cpp:109-115)."""
from __future__ import annotations

import numpy as np

from control_box_rst_amd import capi, problems

DRIVE_POWER, INPUT_ENVELOPE = 2, 3   # slots
HARD_X, HARD_CHI2 = 1e-5, 1e-5       # the hard gate on the derived tolerances (x, relative chi2)
DELTA = 1e-9                         # BaseEdge::computeJacobian's perturbation (edge_interface.cpp:55-96)


def np_drive_power(x, u, prm):
    pw = u[:, 0] * x[:, 2]
    return (pw * pw - prm[0] * prm[0])[:, None]


def np_input_envelope(x, u, prm):
    e0 = prm[0] + prm[1] * x[:, 2] * x[:, 2]
    e1 = prm[2] + prm[3] * x[:, 2] * x[:, 2]
    return np.stack([u[:, 0] - e0, -u[:, 0] - e0, u[:, 1] - e1, -u[:, 1] - e1], axis=1)


NP_FUNCTIONS = {DRIVE_POWER: np_drive_power, INPUT_ENVELOPE: np_input_envelope}
ENVELOPE = (0.2, 0.3, 0.15, 0.2)        # a_0, b_0, a_1, b_1 around the unicycle (|u| <= 1; the jittered starts have controls of 0.3)
ENVELOPE_QUAD = (9.7, 0.2, 0.01, 0.02)  # ... around the quadrotor: thrust (hover 9.81) and roll torque against the altitude
POWER = 0.05                            # drive-power limit of the cart-pole (force x cart speed)


def copy_desc(d):
    """a byte copy (the Python-side parameters of with_state_control_ineq do not travel)"""
    return type(d).from_buffer_copy(d)


def without_term(d):
    c = copy_desc(d)
    c.stage_ineq_state_control = 0
    return c


def make_desc(name, N):
    """name = base[+extra]*: cartpole (FD / Crank-Nicolson, slot 2), unicycle (FD / CN, slot 3), unicyclems (MS / RK4), unicyclet (FD_VARIABLE / CN, free dt),
    quad (MS / RK4, next to its keep-out ball); extras: rate (control-deviation term), unorm (control term, slot 1)."""
    base, *extras = name.split("+")
    if base == "cartpole":
        d = problems.with_state_control_ineq(problems.benchmark_desc("cartpole", N=N), DRIVE_POWER, (POWER,))
    elif base in ("unicycle", "unicyclems", "unicyclet"):
        d = problems.unicycle_desc(N=N)
        if base == "unicyclems":
            d.grid, d.defect = capi.GRID_MS, capi.DEFECT_RK4_SHOOTING
        if base == "unicyclet":
            d.grid, d.dt_lb, d.dt_ub = capi.GRID_FD_VARIABLE, 0.01, 10.0
        problems.with_state_control_ineq(d, INPUT_ENVELOPE, ENVELOPE)
    elif base == "quad":
        d = problems.with_state_control_ineq(problems.quad_desc(N=N, dt=0.05), INPUT_ENVELOPE, ENVELOPE_QUAD)
    else:
        raise KeyError(name)
    for e in extras:
        if e == "rate":
            d.ctrl_dev = capi.CTRL_DEV_RATE
            for i in range(d.nu):
                d.ctrl_dev_params[i] = (0.8, 0.5, 0.5, 0.5)[i]
        elif e == "unorm":
            d.stage_ineq_control = capi.STAGE_FN_USER + 1
            d.ineq_control_params[0] = 0.4
        else:
            raise KeyError(name)
    return d


def penalty_weights(name):
    base = name.split("+")[0]
    return {"cartpole": problems.BENCHMARK_WEIGHTS, "quad": problems.QUAD_WEIGHTS}.get(base, problems.UNICYCLE_WEIGHTS)


BATCH = 3


def make_start(O, name, N, jitter=None, dist=1.0, seed=0, dt=None):
    """-> (desc, X0 [B][nv], xref [B][nx]): the grid's straight line from x_0 to x_0 + dist (x_f - x_0) with jitter N(0, 1) on every parameter but a free dt
    (controls off zero: rows of the term are active at the start); a free dt starts at `dt` where that is given; deterministic in its arguments."""
    d = make_desc(name, N)
    base = name.split("+")[0]
    if jitter is None:
        jitter = 0.1 if base == "quad" else 0.3
    s = 4100 + 17 * N + sum(map(ord, name)) + seed
    rng = np.random.default_rng(s)
    B, nx = BATCH, d.nx
    if base == "cartpole":
        x0, xf = 0.3 * rng.uniform(-1, 1, (B, nx)), 0.3 * rng.uniform(-0.5, 0.5, (B, nx))
    elif base == "quad":
        x0, xf = problems.quad_instances(B, seed=s)
    else:
        x0, xf = problems.unicycle_instances(B, seed=s)
    xf = x0 + dist * (xf - x0)
    p = O.OracleProblem(without_term(d))
    X0 = np.stack([p.init_trajectory(x0[b], xf[b]) for b in range(B)])
    off = p.param_offsets().astype(np.int64)
    if d.grid in (capi.GRID_FD_VARIABLE, capi.GRID_MS_VARIABLE):
        off = off[:-1]
    X0[:, off] += jitter * rng.normal(size=(B, len(off)))
    if dt is not None:
        assert d.grid in (capi.GRID_FD_VARIABLE, capi.GRID_MS_VARIABLE) and d.dt_lb < dt < d.dt_ub
        X0[:, -1] = dt
    return d, X0, np.ascontiguousarray(xf)


def term_values(d, xv):
    """c(x_k, u_k) of every interval at the vertex vector xv, from the HOST evaluator: [N - 1][rows]"""
    N, S, nx = d.N, d.nx + d.nu, d.nx
    z = np.ascontiguousarray(xv[: (N - 1) * S]).reshape(N - 1, S)
    return capi.eval_stage_function_xu(d.stage_ineq_state_control, z[:, :nx], z[:, nx:], d.state_control_params)


def ineq_layout(d):
    """(rows of an interval in front of the term, rows of the term, rows behind it) in the interval's inequality list"""
    front = (1 if (d.stage_ineq and not d.stage_ineq_integral) else 0) + (1 if d.stage_ineq_control else 0)
    return front, capi.stage_function_rows(d.stage_ineq_state_control), (d.nu if d.ctrl_dev else 0)


def term_rows(d, dims):
    """residual rows of the term: [N - 1][rows]"""
    front, r, back = ineq_layout(d)
    first = dims.lsq + dims.eq
    return np.array([[first + k * (front + r + back) + front + j for j in range(r)] for k in range(d.N - 1)])


def box(d, nv):
    """The descriptor's boxes per vertex component (what set_instance_data fills in without lb / ub), the free dt's bounds behind them."""
    nx, nu, N, S = d.nx, d.nu, d.N, d.nx + d.nu
    lb, ub = np.full(nv, -capi.INF), np.full(nv, capi.INF)
    for k in range(N):
        for i in range(nx):
            lb[k * S + i], ub[k * S + i] = d.x_lb[i], d.x_ub[i]
        if k < N - 1:
            for i in range(nu):
                lb[k * S + nx + i], ub[k * S + nx + i] = d.u_lb[i], d.u_ub[i]
    if nv > (N - 1) * S + nx:
        lb[-1], ub[-1] = d.dt_lb, d.dt_ub
    return lb, ub


class Reference:
    """oracle.GenericProblem over (OCP oracle rows without the term) + (the term's rows from the host evaluator), one instance."""

    def __init__(self, O, d, x_start, xref):
        self.O, self.d = O, d
        self.ocp = O.OracleProblem(without_term(d))
        self.voff = self.ocp.param_offsets().astype(np.int64)
        self.base, self.xref = np.array(x_start, np.float64), np.array(xref, np.float64)
        dm = self.ocp.dims
        self.lsq, self.eq, self.ineq0, self.nv = dm.lsq, dm.eq, dm.ineq, dm.nv
        front, r, back = ineq_layout(d)
        self.front, self.r, self.back = front, r, back
        self.ineq = self.ineq0 + (d.N - 1) * r
        self.lb, self.ub = box(d, self.nv)
        # creation order per interval: state term, control term | the state-control term | control-deviation term; behind the intervals: the final-stage
        # inequality and the last control-deviation edge
        st = front + back
        term = np.array([k * (st + r) + front + j for k in range(d.N - 1) for j in range(r)], np.int64)
        self._term_idx, self._old_idx = term, np.setdiff1d(np.arange(self.ineq), term)
        self._key, self._val = None, None

    def rows(self, p):
        key = p.tobytes()
        if key != self._key:
            d, v = self.d, self.base.copy()
            v[self.voff] = p
            self.ocp.set_data(v, xref=self.xref)
            vals, _ = self.ocp.eval(1.0, 1.0, 1.0, jacobian=False)
            old = vals[self.lsq + self.eq: self.lsq + self.eq + self.ineq0]
            c = term_values(d, v)
            new = np.empty(self.ineq)
            new[self._old_idx], new[self._term_idx] = old, c.ravel()
            self._key, self._val = key, (vals[: self.lsq].copy(), vals[self.lsq: self.lsq + self.eq].copy(), new)
        return self._val

    def problem(self):
        return self.O.GenericProblem(len(self.voff), lsq=lambda p: self.rows(p)[0], dim_lsq=self.lsq, eq=lambda p: self.rows(p)[1], dim_eq=self.eq,
                                     ineq=lambda p: self.rows(p)[2], dim_ineq=self.ineq, lb=self.lb[self.voff], ub=self.ub[self.voff])

    def solve(self, start, k, weights):
        gp = self.problem()
        gp.set_data(start)
        opts = capi.default_lm_opts(k, *weights)
        _, chi2, tr = gp.solve(opts, new_run=True)
        return gp.x(), chi2, tr

    def iterate_with_spread(self, k, weights):
        """-> (x_k at the parameters, chi2, x tolerance, chi2 tolerance): max(the ledger's defaults, 4 x the oracle's own spread over starts one ulp away)"""
        from conftest import LEDGER
        p0 = self.base[self.voff]
        xo, co, _ = self.solve(p0, k, weights)
        sx, sc = 0.0, 0.0
        for direction in (np.inf, -np.inf):
            xu, cu, _ = self.solve(np.nextafter(p0, direction), k, weights)
            sx, sc = max(sx, float(np.abs(xu - xo).max())), max(sc, abs(cu - co) / abs(co))
        return xo, co, max(LEDGER["default_x_tol"], 4 * sx), max(LEDGER["default_chi2_rtol"], 4 * sc)

    def first_iteration(self, weights):
        """A record like lm_step_check.oracle_first_iteration's: the reference's J and r at the start (dense, its own central differences), its step and passes."""
        import lm_step_check as L
        p0 = self.base[self.voff]
        gp = self.problem()
        gp.set_data(p0)
        rows, cols = gp.structure()
        values, jac = gp.eval(*weights)
        x1, chi2, tr = self.solve(p0, 1, weights)
        n = len(p0)
        return dict(rows=rows, cols=cols, values=values, jac=jac, delta=x1 - p0, passes=tr[0]["inner_passes"], accepted=tr[0]["accepted"], x1=x1, off=self.voff,
                    fixed=np.setdiff1d(np.arange(self.nv), self.voff), chi2=chi2, mu0=L.initial_damping(cols, jac, n), n=n)


# ---- the tables --------------------------------------------------------------------------------------------------------------------------------------
# values / Jacobian and the LM step: (name, N).  3: the shortest horizon the gate admits; 129: the BIG instantiation of the block-tridiagonal route;
# 257: the LONG sweep (band route); quadrotor 6 / 7: an even and an odd number of grid points of the big-block family's band route
EVAL_CASES = (("cartpole", 3), ("cartpole", 12), ("unicyclems", 12), ("unicyclet", 12), ("unicycle", 129), ("unicycle", 257), ("quad", 6), ("quad", 7))
# rejecting starts of the LM-step test, one per case of EVAL_CASES: (jitter, dist, seed[, dt]) found with Reference on the CPU -- at least one instance that the step
# reference covers takes two or more passes in its first iteration (test_oracle_stage_function_xu.py asserts it).  The shooting grid's default start rejects as
# well (five passes per instance).  The free-dt grid: with dt at the descriptor's 0.1 no start tried rejects (jitter 0 .. 2, dist 2 .. 32: the dt column's entry of
# diag(J^T J) makes the initial damping large and the step short); from dt = 1 the three instances take 3, 3 and 5 passes and dt stays inside its bounds.
REJECTING = {("cartpole", 3): (1.0, 4.0, 1), ("cartpole", 12): (0.5, 8.0, 0), ("unicyclems", 12): (0.6, 2.0, 0), ("unicyclet", 12): (0.3, 4.0, 0, 1.0),
             ("unicycle", 129): (0.3, 8.0, 0), ("unicycle", 257): (0.3, 16.0, 0), ("quad", 6): (0.5, 8.0, 0), ("quad", 7): (0.3, 16.0, 0)}
assert set(REJECTING) == set(EVAL_CASES)
# the LM-step reference (a dense callback problem) is computed for every instance up to this many grid points and for instance 0 beyond
STEP_REFERENCE_ALL_UP_TO = 100
# ... and beyond this many not on the GPU box at all (its dense central differences take six seconds of host time per evaluation and per solve): the device's step is held to DEVICE_MARGIN x 2^-53
# there -- a reference eta of zero -- and the passes and accepted steps of instance 0's first iteration, which fix the expected damping, are the Reference's, recorded in
# STEP_PASSES_LONG: (name, N, rejecting) -> (passes, accepted).  test_oracle_stage_function_xu.py::test_recorded_pass_counts_are_the_references computes them again.
STEP_REFERENCE_NONE_ABOVE = 200
STEP_PASSES_LONG = {("unicycle", 257, False): (1, 1), ("unicycle", 257, True): (2, 1)}


def rejecting_start(O, name, N):
    return make_start(O, name, N, **dict(zip(("jitter", "dist", "seed", "dt"), REJECTING[(name, N)])))


def step_instances(N):
    """how many instances of the batch the LM-step test checks at this horizon"""
    return BATCH if N <= STEP_REFERENCE_ALL_UP_TO else 1


# iterates against Reference: (name, N, start options, iteration counts).  Seeds, start and parameters chosen on the CPU so that the derived tolerance stays at or
# below the hard gate (test_oracle_stage_function_xu.py).  The quadrotor: the oracle's own one-ulp spread on x is 6e-6 .. 9e-6 from the second iteration on
# (soft directions of its cost: thrust / torque weights 0.01 .. 0.1), 4 x that is 2.4e-5 .. 3.6e-5 for every start, parameter set and distance tried (seeds 0 .. 3,
# jitter 0.02 .. 0.1, goal distance 0.05 .. 1) -- beyond the gate; k = 1 is what can be compared there without a vacuous tolerance.
ITERATE_CASES = (("cartpole", 12, {}, (1, 2, 3, 4, 5)), ("unicycle", 12, {"seed": 2}, (1, 2, 3, 4, 5)), ("unicycle+unorm+rate", 12, {}, (1, 2, 3, 4, 5)),
                 ("unicyclet", 12, {}, (1, 2, 3, 4, 5)), ("quad", 6, {"jitter": 0.03, "dist": 0.1}, (1,)))
ITERATE_IDS = [f"{c[0]}-N{c[1]}" for c in ITERATE_CASES]
