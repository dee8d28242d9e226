"""Shared by test_stage_function_eq_host.py, test_oracle_stage_function_eq.py and test_gpu_stage_function_eq.py (imported like conftest -- tests/ is on
the path): the state-control stage EQUALITIES of csrc/stage_functions/ (slot 4 heading_tie, slot 6 input_circle) written out in numpy in the headers'
operation order, the descriptors and starts of the cases, and the reference of the iterate tests.

No fixture of the genuine reference pins this term (the reference driver under oracle/ does not know it).  The reference here is oracle.GenericProblem --
the same oracle_solve as the OCPs -- on a callback that stacks the unchanged OCP oracle's rows of the descriptor with stage_eq = 0 with the term's rows from
the host evaluator (corbo_hip_eval_stage_function_xu: the header the kernels compile), inserted where the reference creates the edge: in the equality
section each interval is [term rows | defect rows] (addEqualityEdge in front of the interval's dynamics edge, finite_differences_grid.cpp:58-61, 102-108;
multiple_shooting_grid.cpp:65-68, 78-85), the final-stage equality rows come behind the intervals.  A state-control INEQUALITY next to it (the extra
`envelope`) is stacked the way stage_function_xu_cases does it."""
from __future__ import annotations

import numpy as np

import stage_function_xu_cases as XU
from control_box_rst_amd import capi, problems

HEADING_TIE, INPUT_CIRCLE = 4, 6     # slots
HARD_X, HARD_CHI2 = XU.HARD_X, XU.HARD_CHI2   # the hard gate on the derived tolerances (x, relative chi2): 1e-5
DELTA = XU.DELTA                     # BaseEdge::computeJacobian's perturbation
BATCH = 3


def np_heading_tie(x, u, prm):
    return ((u[:, 1] - (prm[0] * u[:, 0]) * x[:, 2]) - prm[1])[:, None]


def np_input_circle(x, u, prm):
    e0 = ((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) - prm[0]) - (prm[1] * x[:, 2]) * x[:, 2]
    e1 = (u[:, 2] - (prm[2] * x[:, 0]) * u[:, 0]) - prm[3]
    return np.stack([e0, e1], axis=1)


NP_FUNCTIONS = {HEADING_TIE: np_heading_tie, INPUT_CIRCLE: np_input_circle}
TIE = (0.8, 0.05)                    # around the unicycle: u[1] = 0.8 u[0] x[2] + 0.05
CIRCLE_PAR3 = (0.2, 0.3, 0.5, 0.1)   # around the three parallel integrators
CIRCLE_QUAD = (0.5, 0.2, 0.02, 0.0)  # around the quadrotor: thrust / roll torque on a circle that grows with the altitude, pitch torque mixed with the thrust


def copy_desc(d):
    """a byte copy; the Python-side parameters of with_state_control_ineq travel as the attribute they are"""
    c = type(d).from_buffer_copy(d)
    if hasattr(d, "state_control_params"):
        c.state_control_params = d.state_control_params
    return c


def eq_params(d):
    return [d.stage_eq_params[i] for i in range(8)]


def without_term(d):
    """the descriptor without the equality term: stage_eq = 0 and its parameters cleared (what a descriptor that never had it holds)"""
    c = copy_desc(d)
    c.stage_eq = 0
    for i in range(len(c.stage_eq_params)):
        c.stage_eq_params[i] = 0.0
    return c


def _bare(d):
    """... and without a state-control inequality either: what the OCP oracle knows"""
    c = without_term(d)
    c.stage_ineq_state_control = 0
    return c


def make_desc(name, N):
    """name = base[+extra]*: unicycle (FD / Crank-Nicolson, slot 4), unicyclems (MS / RK4), unicyclet (FD_VARIABLE / CN, free dt), par3 (three parallel
    integrators, FD / CN, slot 6: two rows), quad (MS / RK4, slot 6, next to its keep-out ball); extras: envelope (state-control inequality, slot 3), unorm
    (control term, slot 1), rate (control-deviation term)."""
    base, *extras = name.split("+")
    if base in ("unicycle", "unicyclems", "unicyclet"):
        d = problems.unicycle_desc(N=N)
        if base == "unicyclems":
            d.grid, d.defect = capi.GRID_MS, capi.DEFECT_RK4_SHOOTING
        if base == "unicyclet":
            d.grid, d.dt_lb, d.dt_ub = capi.GRID_FD_VARIABLE, 0.01, 10.0
        problems.with_state_control_eq(d, HEADING_TIE, TIE)
    elif base == "par3":
        d = problems.with_state_control_eq(problems.parallel_integrator_desc(p=3, N=N), INPUT_CIRCLE, CIRCLE_PAR3)
    elif base == "quad":
        d = problems.with_state_control_eq(problems.quad_desc(N=N, dt=0.05), INPUT_CIRCLE, CIRCLE_QUAD)
    else:
        raise KeyError(name)
    for e in extras:
        if e == "envelope":
            problems.with_state_control_ineq(d, XU.INPUT_ENVELOPE, XU.ENVELOPE)
        elif e == "rate":
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
    return {"par3": problems.BENCHMARK_WEIGHTS, "quad": problems.QUAD_WEIGHTS}.get(base, problems.UNICYCLE_WEIGHTS)


def make_start(O, name, N, jitter=None, dist=1.0, seed=0, dt=None):
    """-> (desc, X0 [B][nv], xref [B][nx]): the grid's straight line from x_0 to x_0 + dist (x_f - x_0) with jitter N(0, 1) on every parameter but a free dt
    (controls off zero: the term's rows are non-zero at the start); a free dt starts at `dt` where that is given; deterministic in its arguments."""
    d = make_desc(name, N)
    base = name.split("+")[0]
    if jitter is None:
        jitter = 0.03 if base == "quad" else 0.3
    s = 5200 + 17 * N + sum(map(ord, name)) + seed
    rng = np.random.default_rng(s)
    B, nx = BATCH, d.nx
    if base == "par3":
        x0, xf = rng.uniform(-1, 1, (B, nx)), rng.uniform(-0.5, 0.5, (B, nx))
    elif base == "quad":
        x0, xf = problems.quad_instances(B, seed=s)
    else:
        x0, xf = problems.unicycle_instances(B, seed=s)
    xf = x0 + dist * (xf - x0)
    p = O.OracleProblem(_bare(d))
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
    """e(x_k, u_k) of every interval at the vertex vector xv, from the HOST evaluator: [N - 1][rows]"""
    N, S, nx = d.N, d.nx + d.nu, d.nx
    z = np.ascontiguousarray(xv[: (N - 1) * S]).reshape(N - 1, S)
    return capi.eval_stage_function_xu(d.stage_eq, z[:, :nx], z[:, nx:], eq_params(d))


def term_rows(d, dims):
    """residual rows of the term: [N - 1][rows]; an interval of the equality section is [term rows | nx defect rows]"""
    r = capi.stage_function_rows(d.stage_eq)
    return np.array([[dims.lsq + k * (d.nx + r) + j for j in range(r)] for k in range(d.N - 1)])


class Reference(XU.Reference):
    """oracle.GenericProblem over (OCP oracle rows without the term) + (the term's rows from the host evaluator), one instance; solve / iterate_with_spread /
    first_iteration are stage_function_xu_cases.Reference's."""

    def __init__(self, O, d, x_start, xref):
        self.O, self.d = O, d
        self.ocp = O.OracleProblem(_bare(d))
        self.voff = self.ocp.param_offsets().astype(np.int64)
        self.base, self.xref = np.array(x_start, np.float64), np.array(xref, np.float64)
        dm = self.ocp.dims
        self.lsq, self.eq0, self.ineq0, self.nv = dm.lsq, dm.eq, dm.ineq, dm.nv
        nx, n1 = d.nx, d.N - 1
        self.r = r = capi.stage_function_rows(d.stage_eq)
        self.eq = self.eq0 + n1 * r
        term = np.array([k * (nx + r) + j for k in range(n1) for j in range(r)], np.int64)
        self._eq_term, self._eq_old = term, np.setdiff1d(np.arange(self.eq), term)   # (the old rows keep their order: defects per interval, final-stage rows last)
        # a state-control inequality next to it: stage_function_xu_cases' layout of the inequality section
        self.has_xu = bool(d.stage_ineq_state_control)
        self.ineq = self.ineq0
        if self.has_xu:
            front, ri, back = XU.ineq_layout(d)
            self.ineq = self.ineq0 + n1 * ri
            it = np.array([k * (front + back + ri) + front + j for k in range(n1) for j in range(ri)], np.int64)
            self._in_term, self._in_old = it, np.setdiff1d(np.arange(self.ineq), it)
        self.lb, self.ub = XU.box(d, self.nv)
        self._key, self._val = None, None

    def rows(self, p):
        key = p.tobytes()
        if key != self._key:
            d, v = self.d, self.base.copy()
            v[self.voff] = p
            self.ocp.set_data(v, xref=self.xref)
            vals, _ = self.ocp.eval(1.0, 1.0, 1.0, jacobian=False)
            eq = np.empty(self.eq)
            eq[self._eq_old], eq[self._eq_term] = vals[self.lsq: self.lsq + self.eq0], term_values(d, v).ravel()
            ineq = vals[self.lsq + self.eq0: self.lsq + self.eq0 + self.ineq0].copy()
            if self.has_xu:
                old, ineq = ineq, np.empty(self.ineq)
                ineq[self._in_old], ineq[self._in_term] = old, XU.term_values(d, v).ravel()
            self._key, self._val = key, (vals[: self.lsq].copy(), eq, ineq)
        return self._val


# ---- the tables --------------------------------------------------------------------------------------------------------------------------------------
# values / Jacobian and the LM step: (name, N).  3: the shortest horizon the gate admits; 129: the BIG instantiation of the block-tridiagonal route;
# 257: the LONG sweep (band route); quadrotor 6 / 7: an even and an odd number of grid points of the big-block family's band route
EVAL_CASES = (("unicycle", 3), ("unicycle", 12), ("unicycle", 129), ("unicycle", 257), ("unicyclems", 12), ("unicyclet", 12), ("par3", 12), ("quad", 6), ("quad", 7))
# rejecting starts of the LM-step test, one per case of EVAL_CASES: (jitter, dist, seed[, dt]) found with Reference on the CPU -- at least one instance that the
# step reference covers takes two or more passes in its first iteration (test_oracle_stage_function_eq.py asserts it); one was found for every case.  The
# shooting grid's and the quadrotor's default starts reject as well (up to five passes per instance); the free-dt grid rejects from dt = 1, as the inequality's did.
REJECTING = {("unicycle", 3): (0.6, 4.0, 1), ("unicycle", 12): (0.3, 2.0, 0), ("unicycle", 129): (0.3, 4.0, 0), ("unicycle", 257): (0.3, 8.0, 1),
             ("unicyclems", 12): (0.3, 2.0, 0), ("unicyclet", 12): (0.3, 2.0, 0, 1.0), ("par3", 12): (0.3, 2.0, 1), ("quad", 6): (0.1, 2.0, 0), ("quad", 7): (0.1, 2.0, 0)}
assert set(REJECTING) == set(EVAL_CASES)
# the LM-step reference (a dense callback problem) is computed for every instance up to this many grid points and for instance 0 beyond
STEP_REFERENCE_ALL_UP_TO = 100
# ... and beyond this many not on the GPU box at all (its dense central differences take seconds of host time per evaluation and per solve): the device's step is
# held to DEVICE_MARGIN x 2^-53 there -- a reference eta of zero -- and the passes and accepted steps of instance 0's first iteration, which fix the expected
# damping, are the Reference's, recorded in STEP_PASSES_LONG: (name, N, rejecting) -> (passes, accepted).  test_oracle_stage_function_eq.py computes them again.
STEP_REFERENCE_NONE_ABOVE = 200
STEP_PASSES_LONG = {("unicycle", 257, False): (1, 1), ("unicycle", 257, True): (2, 1)}


def rejecting_start(O, name, N):
    return make_start(O, name, N, **dict(zip(("jitter", "dist", "seed", "dt"), REJECTING[(name, N)])))


def step_instances(N):
    """how many instances of the batch the LM-step test checks at this horizon"""
    return BATCH if N <= STEP_REFERENCE_ALL_UP_TO else 1


# iterates against Reference: (name, N, start options, iteration counts).  Seeds and starts chosen on the CPU so that the derived tolerance stays at or below the
# hard gate (test_oracle_stage_function_eq.py asserts it).  Seeds 0 .. 3 were tried per case; 4 x the oracle's own one-ulp spread over k = 1 .. 5 left the gate for
# unicycle seed 0 (1.3e-5), the shooting grid's seeds 1 and 2 (9.4e-5, 1.1e-5) and the quadrotor's seed 1 (3.9e-5 at k = 2); the seeds below stay at the ledger's
# defaults.  Their first iterations: unicycle seed 1 rejects at k = 3 (three passes), the envelope case at k = 1, 4 and 5, the shooting grid and the quadrotor
# take five passes in their first iteration, par3 four in its second.
ITERATE_CASES = (("unicycle", 12, {"seed": 1}, (1, 2, 3, 4, 5)), ("unicycle+envelope+unorm+rate", 12, {"seed": 3}, (1, 2, 3, 4, 5)),
                 ("unicyclet", 12, {}, (1, 2, 3, 4, 5)), ("unicyclems", 12, {}, (1, 2, 3, 4, 5)), ("par3", 12, {"seed": 1}, (1, 2, 3, 4, 5)),
                 ("quad", 6, {}, (1, 2)))
ITERATE_IDS = [f"{c[0]}-N{c[1]}" for c in ITERATE_CASES]
