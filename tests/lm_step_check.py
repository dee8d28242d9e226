"""The linear solve of one Levenberg-Marquardt iteration, checked against the normal equations (helper of test_oracle_linear_solve.py and
test_gpu_linear_solve.py; imported like conftest -- tests/ is on the path).

Every factor phase solves (J^T J + sum(mu) I) delta = -J^T r.  After ONE iteration from a known start x_0 the host has everything of that system
without a new entry point: delta = x_1 - x_0 at the parameter offsets, J and r at x_0 from the eval hook, mu_0 = 1e-5 max diag(J^T J), and the
damping the inner loop has added by its p-th pass, mu_0 (1 + 2 + 8 + 64 + ...): a rejected step multiplies mu by v = 2, 4, 8, ... and
H_ii += mu is never undone (levenberg_marquardt_sparse.cpp:135-138, 211-212).  The normwise backward error

    eta = |H delta - g|_inf / (|H|_inf |delta|_inf + |g|_inf),        H = J^T J + sum(mu) I,  g = -J^T r

of a backward-stable factorisation is a small multiple of 2^-53 whatever the elimination order; a factor phase that works on a Jacobian which
differs by finite-difference noise (1e-9 relative) lands at 1e-10 .. 1e-7, one that loses a Schur update, a Gram term or one mu of the sum far above.

CASES is the one table both files run: the smallest shapes at which each factorisation path of the device switches (not the workloads).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import scipy.sparse as sp

from control_box_rst_amd import capi, problems

TAU = 1e-5            # mu_0 = TAU max diag(J^T J)   (levenberg_marquardt_sparse.cpp:117)
U = 2.0 ** -53        # unit roundoff of float64
DEVICE_MARGIN = 16.0  # eta_device <= DEVICE_MARGIN max(eta_oracle, U): another elimination order, redundant lanes and tree reductions change the constant
                      # of Cholesky's backward-error bound, not its order
ORACLE_BOUND = 1e-14  # the oracle's envelope Cholesky (measured maximum over the table: see docs/measurements/r08.md)


def expected_damping(mu0: float, passes: int) -> float:
    """sum of the mu the reference's inner loop has added to the diagonal of H when its `passes`-th factorisation runs."""
    total, mu, v = 0.0, float(mu0), 2.0
    for _ in range(int(passes)):
        total += mu
        mu *= v
        v *= 2.0
    return total


def last_damping(mu0: float, passes: int) -> float:
    """the mu of the last pass alone (what a factor phase would use if the earlier passes' additions were lost)"""
    mu, v = float(mu0), 2.0
    for _ in range(int(passes) - 1):
        mu *= v
        v *= 2.0
    return mu


def initial_damping(cols, jac, n: int) -> float:
    d = np.zeros(n)
    np.add.at(d, cols, np.asarray(jac, np.float64) ** 2)
    return TAU * float(d.max())


def step_backward_error(rows, cols, jac, values, delta, sum_mu) -> float:
    """eta of the docstring above.  Sparse: the residual J^T (J delta + r) + sum(mu) delta and g in extended precision (np.longdouble accumulators over the
    COO triplets), |H|_inf from a float64 scipy.sparse product."""
    LD = np.longdouble
    rows, cols = np.asarray(rows), np.asarray(cols)
    m, n = len(values), len(delta)
    J, r, d = np.asarray(jac, LD), np.asarray(values, LD), np.asarray(delta, LD)
    Jd = np.zeros(m, LD)
    np.add.at(Jd, rows, J * d[cols])
    res = np.zeros(n, LD)
    np.add.at(res, cols, J * (Jd + r)[rows])
    res += LD(sum_mu) * d
    g = np.zeros(n, LD)
    np.add.at(g, cols, J * r[rows])
    Js = sp.coo_matrix((np.asarray(jac, np.float64), (rows, cols)), shape=(m, n)).tocsr()
    H = (Js.T @ Js).tocsr()
    h_inf = float(abs(H).sum(axis=1).max()) + float(sum_mu)
    return float(np.abs(res).max() / (LD(h_inf) * np.abs(d).max() + np.abs(g).max()))


def forward_error(rows, cols, jac, values, delta, sum_mu) -> float:
    """|delta - delta*|_inf / |delta*|_inf against a solve of the same system refined in extended precision (dense; small cases only)."""
    LD = np.longdouble
    m, n = len(values), len(delta)
    Js = sp.coo_matrix((np.asarray(jac, np.float64), (rows, cols)), shape=(m, n)).toarray()
    H = Js.T @ Js + sum_mu * np.eye(n)
    Hl, g = H.astype(LD), -(Js.T.astype(LD) @ np.asarray(values, LD))
    x = np.linalg.solve(H, g.astype(np.float64)).astype(LD)
    for _ in range(4):   # iterative refinement with an extended-precision residual
        x = x + np.linalg.solve(H, (g - Hl @ x).astype(np.float64)).astype(LD)
    return float(np.abs(np.asarray(delta, LD) - x).max() / np.abs(x).max())


# ---------------------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    route: str                # route class: "cr", "long", "bt", "band", "big"
    family: str               # descriptor family (make_desc)
    N: int
    start: tuple = ("line",)  # ("line",): the grid's straight-line initial guess; ("perturbed", scale, seed): + scale N(0, 1) on every parameter but a free dt
    options: tuple = ()       # corbo_hip_set_option pairs of the device handle
    create_route: int = 0     # corbo_hip_create_routed flags
    weights: tuple = ()       # penalty weights; () = the family's
    expect: int = -1          # capi.FACTOR_* the handle must report (-1: not asserted)

    @property
    def rejecting(self):
        return self.start[0] == "perturbed"

    @property
    def input_key(self):      # cases that differ in handle options only share their input (and the oracle's answer)
        return (self.family, self.N, self.start, self.weights)

    @property
    def id(self):
        s = f"{self.route}-{self.family}-N{self.N}"
        if self.rejecting:
            s += f"-rej{self.start[2]}"
        if self.create_route:
            s += f"-route{self.create_route}"
        return s + "".join(f"-{k}{v}" for k, v in self.options)


RATE = {"unicycle": (0.3, 0.3), "vdp": (0.7,), "cartpole": (0.5,), "quad": (4.0, 2.0, 2.0, 2.0), "int3t": (3.0,)}
EQ_LIN = {"vdp": (0.3, -0.2, 0.05, 0.1), "int3t": (0.01, 0.02, 0.0, 0.05, 0.0), "unicycle": (0.3, -0.2, 0.1, 0.05, 0.02, 0.1)}
_BASE_WEIGHTS = {"unicycle": problems.UNICYCLE_WEIGHTS, "vdp": problems.VDP_WEIGHTS, "cartpole": problems.BENCHMARK_WEIGHTS, "par3": problems.BENCHMARK_WEIGHTS,
                 "par2": problems.BENCHMARK_WEIGHTS, "int3": problems.INT3_WEIGHTS, "cartpolet": problems.DINT_WEIGHTS,
                 "int3t": problems.INT3_WEIGHTS, "dint": problems.DINT_WEIGHTS, "quad": problems.QUAD_WEIGHTS, "quadt": problems.QUAD_WEIGHTS, "pquad": problems.QUAD_WEIGHTS}


def _dense_weights(d, seed):
    """random symmetric positive definite Q / R / Qf as upper Cholesky factors in the descriptor (nx <= 4)"""
    rd = np.random.default_rng(seed)
    d.weights_dense = 1 | (2 if d.nu > 1 else 0) | (4 if d.final_cost else 0)
    for dst, n in ((d.q_sqrt, d.nx), (d.r_sqrt, d.nu), (d.qf_sqrt, d.nx)):
        a = rd.uniform(-1, 1, (n, n))
        for i, v in enumerate(np.linalg.cholesky(a.T @ a + 0.5 * np.eye(n)).T.ravel()):
            dst[i] = float(v)


def make_desc(family: str, N: int):
    """family = base[+extra]*: base one of unicycle, vdp, cartpole, cartpolet, par2, par3, unicyclems, int3, int3t, dint, quad, quadt, pquad; extras rate, eqlin (trapezoidal
    integral equality), dense (non-diagonal weights)."""
    base, *extras = family.split("+")
    if base == "unicycle":
        d = problems.unicycle_desc(N=N)
    elif base == "unicyclems":   # the shooting grid with RK4 defects
        d = problems.unicycle_desc(N=N)
        d.grid, d.defect = capi.GRID_MS, capi.DEFECT_RK4_SHOOTING
    elif base == "vdp":
        d = problems.vdp_desc(N=N)
    elif base == "cartpole":
        d = problems.benchmark_desc("cartpole", N=N)
    elif base == "cartpolet":    # the cart-pole, time-optimal like int3t: FiniteDifferencesVariableGrid, MinimumTime, x_f fixed -- shape (4, 1) with a free dt
        d = problems.benchmark_desc("cartpole", N=N)
        d.grid, d.stage_cost, d.final_cost, d.xf_fixed_mask = capi.GRID_FD_VARIABLE, capi.COST_MIN_TIME_LSQ, 0, 0b1111
        d.dt_lb, d.dt_ub = 0.01, 10.0
        for i in range(d.nx):
            d.q_diag[i] = d.qf_diag[i] = 0.0
        d.r_diag[0] = 0.0
    elif base == "par2":
        d = problems.parallel_integrator_desc(2, N=N)
    elif base == "par3":
        d = problems.parallel_integrator_desc(3, N=N)
    elif base == "int3":         # the fixed-dt serial integrator: shape (3, 1)
        d = problems.int3_desc(N=N, dt=0.1)
    elif base == "int3t":        # time-optimal: the free dt is the arrowhead of H
        d = problems.int3_desc(N=N, dt=0.1, time_optimal=True)
    elif base == "dint":
        d = problems.dint_desc(N=N)
    elif base == "quad":
        d = problems.quad_desc(N=N, dt=0.05)
    elif base == "quadt":
        d = problems.quad_desc(N=N, dt=0.05, time_optimal=True)
    elif base == "pquad":        # planar quadrotor on the finite-differences grid, Crank-Nicolson
        d = problems.planar_quadrotor_desc(N=N, dt=0.05)
        d.grid, d.defect = capi.GRID_FD, capi.DEFECT_CRANK_NICOLSON
    else:
        raise KeyError(family)
    key = {"unicyclems": "unicycle", "quadt": "quad"}.get(base, base)
    for e in extras:
        if e == "rate":
            d.ctrl_dev = capi.CTRL_DEV_RATE
            for i, v in enumerate(RATE[key]):
                d.ctrl_dev_params[i] = v
        elif e == "eqlin":
            d.stage_eq = capi.STAGE_EQ_LINEAR
            d.constraint_integration = capi.RULE_TRAPEZOIDAL
            for i, v in enumerate(EQ_LIN[key]):
                d.stage_eq_params[i] = v
        elif e == "dense":
            _dense_weights(d, 99000 + d.nx)
        else:
            raise KeyError(family)
    return d


def penalty_weights(case: Case):
    if case.weights:
        return case.weights
    base = case.family.split("+")[0]
    return _BASE_WEIGHTS[{"unicyclems": "unicycle"}.get(base, base)]


BATCH = 3
# Accepted-at-once starts, per base family: (dist, jitter).  The grid's straight-line guess between x_0 and x_0 + dist (x_f - x_0) with jitter N(0, 1) on
# every parameter but a free dt: close enough to a solution that the first pass is accepted at every
# horizon of the table, rough enough that the step is no smaller than a twentieth of the iterate (eta is computed from fl(x_0 + delta) - x_0) and that every
# block of H carries generic values.  test_oracle_linear_solve.py asserts both on every input.
START = {"unicycle": (1.0, 0.1), "vdp": (1.0, 0.1), "cartpole": (1.0, 0.1), "par3": (1.0, 0.1), "par2": (1.0, 0.1), "int3": (1.0, 0.1), "cartpolet": (0.3, 0.03), "unicyclems": (0.0, 0.3), "int3t": (0.3, 0.03), "dint": (0.3, 0.03),
         "unicycle+rate": (1.0, 0.3), "cartpole+rate": (1.0, 0.3), "unicycle+rate+eqlin+dense": (1.0, 0.3), "quad": (1.0, 0.3), "quad+rate": (0.3, 0.1), "pquad": (1.0, 0.1), "quadt": (1.0, 0.1)}


def make_start(case: Case, O):
    """-> (desc, X0 [B][nv], xref [B][nx]); deterministic in the case."""
    d = make_desc(case.family, case.N)
    base = case.family.split("+")[0]
    dist, jitter = START[case.family] if case.family in START else START[base]
    if case.rejecting:
        dist, jitter = (case.start[3] if len(case.start) > 3 else 1.0), case.start[1]
    seed = 7000 + 13 * case.N + sum(map(ord, case.family)) + (case.start[2] if case.rejecting else 0)
    rng = np.random.default_rng(seed)
    B, nx = BATCH, d.nx
    if base in ("unicycle", "unicyclems"):
        x0, xf = problems.unicycle_instances(B, seed=seed)
    elif base in ("quad", "quadt"):
        x0, xf = problems.quad_instances(B, seed=seed)
    elif base == "pquad":
        x0, xf = np.zeros((B, 6)), np.zeros((B, 6))
        x0[:, :2] = rng.uniform(-0.2, 0.2, (B, 2))
        xf[:, :2] = np.array([2.0, 1.0]) + rng.uniform(-0.3, 0.3, (B, 2))
    elif base in ("int3t", "dint", "cartpolet"):
        x0 = np.zeros((B, nx))
        x0[:, 0] = rng.uniform(-0.3, 0.3, B)
        xf = np.zeros((B, nx))
        xf[:, 0] = 1.0 + rng.uniform(-0.2, 0.2, B)
    elif base == "vdp" and case.rejecting:   # (a start away from the origin: the oscillator's nonlinearity is what makes the first steps fail)
        x0 = np.tile([2.0, -2.0], (B, 1)) + rng.uniform(-0.2, 0.2, (B, 2))
        xf = np.zeros((B, 2))
    else:
        x0 = rng.uniform(-1, 1, (B, nx)) * (0.3 if base == "cartpole" else 1.0)
        xf = rng.uniform(-0.5, 0.5, (B, nx)) * (0.3 if base == "cartpole" else 1.0) + (np.array([1.5, 0.5, 0.2, 0.0])[:nx] if base != "cartpole" else 0.0)
    xf = x0 + dist * (xf - x0)
    p = O.OracleProblem(d)
    X0 = np.stack([p.init_trajectory(x0[b], xf[b]) for b in range(B)])
    off = p.param_offsets().astype(np.int64)
    if d.grid in (capi.GRID_FD_VARIABLE, capi.GRID_MS_VARIABLE):
        off = off[:-1]   # (the free dt is the last parameter: left alone, a perturbed dt leaves its bounds)
    X0[:, off] += jitter * rng.normal(size=(B, len(off)))
    return d, X0, np.ascontiguousarray(xf)


def oracle_first_iteration(O, case: Case, d, X0, xref):
    """One LM iteration of the oracle per instance.  -> list of dicts: rows, cols, values, jac (at x_0), delta (at the parameter offsets), passes, accepted,
    x1, fixed (offsets of the vertex entries that are no parameters), chi2, mu0.  The oracle's eval perturbs x in place for its finite differences and
    restores it by a second addition (an ulp of drift): the start is uploaded again before the solve."""
    w = penalty_weights(case)
    opts = capi.default_lm_opts(1, *w)
    out = []
    for b in range(X0.shape[0]):
        p = O.OracleProblem(d)
        p.set_data(X0[b], xref=xref[b])
        rows, cols = p.structure()
        values, jac = p.eval(*w)
        p.set_data(X0[b], xref=xref[b])
        status, chi2, tr = p.solve(opts, new_run=True)
        x1 = p.x()
        off = p.param_offsets().astype(np.int64)
        fixed = np.setdiff1d(np.arange(p.dims.nv), off)
        out.append(dict(rows=rows, cols=cols, values=values, jac=jac, delta=x1[off] - X0[b][off], passes=tr[0]["inner_passes"], accepted=tr[0]["accepted"],
                        x1=x1, off=off, fixed=fixed, chi2=chi2, mu0=initial_damping(cols, jac, p.dims.n), n=p.dims.n))
    return out


def device_first_iteration(case: Case, d, X0, xref):
    """upload, eval(), restore_instance_data(), solve(), get_solution() on a device handle with the case's options.
    -> (solver, values [B][m], jac [B][nnz], x1 [B][nv], chi2 [B], stats)"""
    from control_box_rst_amd.solver import BatchedLevenbergMarquardt
    s = BatchedLevenbergMarquardt(d, X0.shape[0], route=case.create_route)
    for k, v in case.options:
        s.set_option(k, v)
    s.setIterations(1)
    s.setPenaltyWeights(*penalty_weights(case))
    s.set_instance_data(X0, xref=xref)
    values, jac = s.eval()
    s.restore_instance_data()
    s.solve()
    x1, chi2, status = s.get_solution()
    return s, values, jac, x1, chi2, s.get_stats()


def eta_of(o, delta=None, jac=None, values=None, sum_mu=None):
    """eta of an oracle_first_iteration record (optionally with another step / Jacobian / residual / damping in its place)"""
    return step_backward_error(o["rows"], o["cols"], o["jac"] if jac is None else jac, o["values"] if values is None else values,
                               o["delta"] if delta is None else delta, expected_damping(o["mu0"], o["passes"]) if sum_mu is None else sum_mu)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The table.  Horizons: the shortest the structure accepts, then both sides of every size at which a kernel changes shape (waves per instance, rounds
# of the cyclic reduction, the one-round first level, the 128- / 256-thread instantiations, the BIG instantiation of the block-tridiagonal route, ...).
CR_HORIZONS = (2, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 100, 101, 128, 129, 255, 256)
BT_HORIZONS = (3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 128, 129, 200, 256)
# factor_long_kernel keeps the state-block arrays in LDS where 27 (N | 1) + 130 doubles fit 160 KB (unicycle: N <= 751, launch_factor_a) and works in the
# HBM workspace beyond: 700 / 800 are one horizon on each side; 257 .. 512 run eight waves (two resp. one workgroup per CU), 513 sixteen.
LONG_HORIZONS = (257, 512, 513, 700, 800, 1024)
# ... and the same for every block shape (nx, nu, free dt) the build compiles factor_long_kernel for: the smallest horizons on each side of every switch of
# launch_factor_a that the shape can reach -- two workgroups' state blocks per CU | one (nx = 3: 373 | 374, with a free dt 335 | 336; nx = 2: 775 | 776, with a
# free dt 671 | 672 -- there the sixteen-wave instantiation is the same on both sides, what changes is how many workgroups a CU holds), eight | sixteen waves
# (512 | 513), LDS | HBM workspace (nx = 3: 751 | 752, free dt 677 | 678; nx = 4: 441 | 442, free dt 405 | 406).  corbo_hip_long_factor_plan reports the
# launcher's decision; test_oracle_linear_solve.py::test_table_covers_the_listed_paths asserts against it that every switch is straddled (docs/measurements/r10.md).
LONG_SHAPE_HORIZONS = {
    "vdp": (257, 512, 513, 775, 776, 1024),                          # (2, 1)
    "par2": (257, 512, 513, 775, 776, 1024),                         # (2, 2)
    "dint": (671, 672),                                              # (2, 1), free dt (the other horizons: LONG_HORIZONS)
    "int3": (257, 373, 374, 512, 513, 751, 752, 1024),               # (3, 1)
    "par3": (257, 373, 374, 512, 513, 751, 752, 1024),               # (3, 3)
    "unicyclems": (257, 373, 374, 513, 751, 752),                    # (3, 2), shooting grid, RK4 (512: the unicycle of LONG_HORIZONS)
    "int3t": (257, 335, 336, 512, 513, 677, 678, 1024),              # (3, 1), free dt
    "cartpole": (257, 441, 442, 512, 513, 1024),                     # (4, 1)
    "cartpolet": (257, 405, 406, 1024),                              # (4, 1), free dt
}
LONG_DENSE = (("cartpole+dense", 300), ("cartpole+dense", 500), ("par3+dense", 700), ("par3+dense", 800), ("vdp+dense", 1024))


def _cases():
    c = []
    for fam in ("unicycle", "vdp", "cartpole", "par3", "unicyclems", "int3t"):
        for N in CR_HORIZONS:
            c.append(Case("cr", fam, N, expect=capi.FACTOR_STAGE_CR))
    c.append(Case("cr", "unicycle", 100, options=(("run_to_completion", 0),), expect=capi.FACTOR_STAGE_CR))
    for N in (12, 100, 130):
        c.append(Case("cr", "unicycle+dense", N, expect=capi.FACTOR_STAGE_CR))
    for fam in ("unicycle", "dint"):
        for N in LONG_HORIZONS:
            c.append(Case("long", fam, N, expect=capi.FACTOR_STAGE_CR))
    c.append(Case("long", "unicycle+dense", 300, expect=capi.FACTOR_STAGE_CR))
    c.append(Case("long", "unicycle+dense", 800, expect=capi.FACTOR_STAGE_CR))
    for fam, horizons in LONG_SHAPE_HORIZONS.items():
        for N in horizons:
            c.append(Case("long", fam, N, expect=capi.FACTOR_STAGE_CR))
    for fam, N in LONG_DENSE:
        c.append(Case("long", fam, N, expect=capi.FACTOR_STAGE_CR))
    for fam in ("unicycle+rate", "vdp+eqlin", "cartpole+rate", "int3t+eqlin"):
        for N in BT_HORIZONS:
            for waves in (2, 3):
                c.append(Case("bt", fam, N, options=(("bt_waves", waves),), expect=capi.FACTOR_BLOCK_TRI))
        for N in (12, 40, 257, 300):
            for wide in (0, 1):
                c.append(Case("band", fam, N, options=(("band_wide", wide),), create_route=capi.ROUTE_XE_BAND, expect=capi.FACTOR_BAND))
    for N in (8, 20):
        c.append(Case("band", "quad+rate", N, expect=capi.FACTOR_BAND))
    c.append(Case("band", "unicycle+rate+eqlin+dense", 12, expect=capi.FACTOR_BAND))
    for fam in ("quad", "pquad"):
        for N in (8, 16, 37, 64, 65):
            for variant in (2, 6, 4, 3):
                c.append(Case("big", fam, N, options=(("chain_variant", variant),), expect=capi.FACTOR_STAGE_CHAIN))
    for N in (8, 37):
        for variant in (2, 4):
            c.append(Case("big", "quadt", N, options=(("chain_variant", variant),), expect=capi.FACTOR_STAGE_CHAIN))
    return c


# Rejecting starts: ("perturbed", jitter, seed[, dist]) -- the straight line from x_0 to x_0 + dist (x_f - x_0) with jitter N(0, 1) on the parameters.  Found with the
# oracle on the CPU (a Gauss-Newton step from these collocation starts is seldom rejected: it takes a shooting grid whose controls start at zero, goals several
# times further away than the controls' bounds allow, or a rate limit that the step activates): every instance of the batch takes three or more passes in its
# first iteration and still moves by a twentieth of the iterate; test_oracle_linear_solve.py asserts that.  They drive the cumulative damping, the snapshot
# reload of the block-tridiagonal route and the speculation of the big-block family.  unicycle+rate is the rate limit 0.3 with penalty weights 10.
def _rejecting():
    c = []
    CR, BT, BAND, CHAIN = capi.FACTOR_STAGE_CR, capi.FACTOR_BLOCK_TRI, capi.FACTOR_BAND, capi.FACTOR_STAGE_CHAIN
    for fam, N, start in (("unicyclems", 8, ("perturbed", 0.0, 0)), ("unicyclems", 33, ("perturbed", 0.0, 0)), ("unicyclems", 129, ("perturbed", 0.0, 0, 2.0)),
                          ("unicycle", 100, ("perturbed", 0.0, 0, 4.0)), ("vdp", 100, ("perturbed", 0.0, 0, 2.0)), ("cartpole", 16, ("perturbed", 0.3, 2, 8.0))):
        c.append(Case("cr", fam, N, start=start, expect=CR))
    for seed in (1, 2):
        c.append(Case("long", "unicycle", 257, start=("perturbed", 0.0, seed, 4.0), expect=CR))
    c.append(Case("long", "cartpole", 442, start=("perturbed", 0.3, 1, 16.0), expect=CR))   # nx = 4, HBM workspace below 512 grid points
    c.append(Case("long", "int3t", 336, start=("perturbed", 0.0, 0, 2.0), expect=CR))       # free dt, one workgroup per CU
    xe = (("unicycle+rate", 6, ("perturbed", 0.0, 0)), ("unicycle+rate", 12, ("perturbed", 0.0, 0)), ("unicycle+rate", 40, ("perturbed", 0.02, 0)),
          ("unicycle+rate", 200, ("perturbed", 0.02, 4)), ("cartpole+rate", 12, ("perturbed", 0.0, 1)), ("cartpole+rate", 40, ("perturbed", 0.0, 5)))
    for fam, N, start in xe:
        for waves in (2, 3):
            c.append(Case("bt", fam, N, start=start, options=(("bt_waves", waves),), expect=BT))
        for wide in (0, 1):
            c.append(Case("band", fam, N, start=start, options=(("band_wide", wide),), create_route=capi.ROUTE_XE_BAND, expect=BAND))
    c.append(Case("band", "cartpole+rate", 257, start=("perturbed", 0.02, 5), expect=BAND))
    for N in (8, 20):
        c.append(Case("band", "quad+rate", N, start=("perturbed", 0.0, 0), expect=BAND))
    for variant in (2, 4):
        for spec in (0, 1, 2):   # (2: speculation forced, whatever the batch size)
            c.append(Case("big", "quad", 37, start=("perturbed", 0.1, 0, 16.0), options=(("chain_variant", variant), ("reject_speculation", spec)), expect=CHAIN))
    return c


CASES = _cases() + _rejecting()
assert len({c.id for c in CASES}) == len(CASES)


def unique_inputs(cases=None):
    """one case per distinct input (cases that differ in handle options share theirs)"""
    seen, out = set(), []
    for c in (CASES if cases is None else cases):
        if c.input_key not in seen:
            seen.add(c.input_key)
            out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# A corbo_hip_create_weighted handle (non-diagonal Q, R, Qf around the big-block family).  The oracle takes non-diagonal weights through the descriptor only
# (nx <= 4); the reference of this case is assembled on the host instead: the oracle's residual and Jacobian of the SAME descriptor with unit weights, the
# cost blocks multiplied by the upper factors U (cost rows are U (x - ref), linear in the unit rows), one LM pass with LAPACK's dense Cholesky, the trial
# point evaluated the same way (accepted when chi2 falls: the gain ratio's denominator is positive for mu > 0).
WEIGHTED_N = 12


def _random_spd(n, seed):
    a = np.random.default_rng(seed).standard_normal((n, n))
    return a @ a.T / n + np.eye(n)


def weighted_case(O):
    """-> (desc, weights dict, X0 [B][nv], xref, records like oracle_first_iteration's)"""
    import scipy.linalg
    from control_box_rst_amd.solver import weight_factors
    d = problems.quad_desc(N=WEIGHTED_N, dt=0.05)
    nx, nu, N, S = d.nx, d.nu, d.N, d.nx + d.nu
    wts = {"Q": _random_spd(nx, 11), "R": 0.1 * _random_spd(nu, 12), "Qf": 10.0 * _random_spd(nx, 13)}
    wf = weight_factors(d, wts)
    Uf = {0: np.array(wf.q_sqrt[: nx * nx]).reshape(nx, nx), 1: np.array(wf.r_sqrt[: nu * nu]).reshape(nu, nu), 2: np.array(wf.qf_sqrt[: nx * nx]).reshape(nx, nx)}
    d1 = type(d).from_buffer_copy(d)
    for i in range(nx):
        d1.q_diag[i] = d1.qf_diag[i] = 1.0
    for i in range(nu):
        d1.r_diag[i] = 1.0
    case = Case("big", "quad", WEIGHTED_N)
    dd, X0, xref = make_start(case, O)
    w = penalty_weights(case)
    p = O.OracleProblem(d1)
    rows, cols = p.structure()
    off = p.param_offsets().astype(np.int64)
    m, n = p.dims.m, p.dims.n
    blocks = [(k * S + o, dim, cls) for k in range(N - 1) for o, dim, cls in ((0, nx, 0), (nx, nu, 1))] + [((N - 1) * S, nx, 2)]
    assert p.dims.lsq == (N - 1) * S + nx

    def evaluate(x, b, jacobian):
        p.set_data(x, xref=xref[b])
        v, j = p.eval(*w, jacobian=jacobian)
        J = sp.coo_matrix((j, (rows, cols)), shape=(m, n)).toarray() if jacobian else None
        for r0, dim, cls in blocks:
            v[r0: r0 + dim] = Uf[cls] @ v[r0: r0 + dim]
            if jacobian:
                J[r0: r0 + dim] = Uf[cls] @ J[r0: r0 + dim]
        return v, J

    out = []
    for b in range(X0.shape[0]):
        values, J = evaluate(X0[b], b, True)
        jac = J[rows, cols]
        assert np.count_nonzero(J) <= np.count_nonzero(jac), "the weighted cost blocks stay inside the descriptor's structure"
        mu0 = initial_damping(cols, jac, n)
        H = J.T @ J + mu0 * np.eye(n)
        delta = scipy.linalg.cho_solve(scipy.linalg.cho_factor(H), -(J.T @ values))
        x1 = X0[b].copy()
        x1[off] += delta
        v1, _ = evaluate(x1, b, False)
        out.append(dict(rows=rows, cols=cols, values=values, jac=jac, delta=x1[off] - X0[b][off], passes=1, accepted=int(float(v1 @ v1) < float(values @ values)),
                        x1=x1, off=off, fixed=np.setdiff1d(np.arange(p.dims.nv), off), chi2=float(v1 @ v1), mu0=mu0, n=n))
    return d, wts, X0, xref, out
