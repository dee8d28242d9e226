"""Inputs of the long-horizon tests (helper of test_gpu_long_horizon.py and test_oracle_long_horizon.py; imported like conftest -- tests/ is on the path).

Beyond 256 grid points the small-block families run kernels of their own: the sweep's LONG instantiation (Jacobian straight to HBM; one per model unit,
defect kind and DENSE) and factor_long_kernel.  Two sets of inputs, built here once so that the device file and its CPU twin see the same numbers:

  * MODEL_CASES: every small-block row of csrc/model_table.inc that problems.py can describe, at N = 257 (the smallest long horizon), on Crank-Nicolson and
    on the shooting grid with RK4; the unicycle and the cart-pole also with the other collocation formulas and shooting integrators;
  * fuzz_input(O, seed): the FUZZ_COUNT seeded random descriptors (test_gpu_fuzz.random_desc) at 257 .. 1024 grid points.
"""
from __future__ import annotations

import numpy as np

from control_box_rst_amd import capi, problems
from test_gpu_fuzz import random_desc

LONG_N = 257     # the smallest horizon of the long-horizon kernels
MODEL_BATCH = 2
MODEL_DT = 0.1   # the scenarios' own step
# The start: the grid's straight line from x_0 a part of the way to the seeded goal, noise on every free entry, every 16th control pushed past its upper bound.
# Close enough that three iterations of the oracle itself are reproducible to half the solve tolerances from starts one ulp apart (finite-difference noise
# amplified through the iterations; the CPU twin asserts it for every case) -- the full unicycle distance with |u| <= 1 is not (shooting grid: 1e-5).
NOISE, PUSH, PUSH_EVERY = 0.01, 0.25, 16
GOAL_FRACTION = {"unicycle": 0.1, "kcar": 0.05}

_LIN_SHAPES = ((2, 1), (2, 2), (3, 1), (3, 2), (3, 3), (4, 1))
COLLOCATION = {"forward": capi.DEFECT_FORWARD, "backward": capi.DEFECT_BACKWARD, "midpoint": capi.DEFECT_MIDPOINT, "cn": capi.DEFECT_CRANK_NICOLSON}
SHOOTING = {"euler": 1, "rk2": 2, "rk3": 3, "rk4": 0, "rk5": 5, "rk7": 7}   # corbo_hip_problem_desc::shooting_integrator (0: the default, RK4)


def _int2_desc(N, dt):
    """SerialIntegratorSystem of order 2 on the fixed grid with a quadratic cost (the int3 set-up, one state less)"""
    q = (1.0, 0.5)
    return problems.make_desc(grid=capi.GRID_FD, defect=capi.DEFECT_CRANK_NICOLSON, dynamics=capi.DYN_SERIAL_INTEGRATOR, nx=2, nu=1, N=N, dt=dt,
                              q=q, r=(0.1,), qf=tuple(10.0 * v for v in q), u_lb=(-1.0,), u_ub=(1.0,), dyn_params=(1.0,))


def _lin_desc(nx, nu, N, dt):
    r = np.random.default_rng(4100 + 10 * nx + nu)   # fixed seeded matrices per block shape
    return problems.linear_desc(r.uniform(-1, 1, (nx, nx)) - 1.0 * np.eye(nx), r.uniform(-1, 1, (nx, nu)), N=N, dt=dt)


MODELS = {"vdp": lambda N, dt: problems.vdp_desc(N=N, dt=dt), "int2": _int2_desc, "int3": lambda N, dt: problems.int3_desc(N=N, dt=dt),
          "unicycle": lambda N, dt: problems.unicycle_desc(N=N, dt=dt), "kcar": lambda N, dt: problems.kinematic_car_desc(N=N, dt=dt),
          "par2": lambda N, dt: problems.parallel_integrator_desc(2, N=N, dt=dt), "par3": lambda N, dt: problems.parallel_integrator_desc(3, N=N, dt=dt)}
for _name in problems.BENCHMARK_SYSTEMS:
    MODELS[_name] = (lambda n: (lambda N, dt: problems.benchmark_desc(n, N=N, dt=dt)))(_name)
for _nx, _nu in _LIN_SHAPES:
    MODELS[f"lin{_nx}{_nu}"] = (lambda a, b: (lambda N, dt: _lin_desc(a, b, N, dt)))(_nx, _nu)

# (model, formula): "cn" ... = collocation on the FiniteDifferencesGrid, "ms_*" = MultipleShootingGrid with that integrator
MODEL_CASES = [(m, f) for m in sorted(MODELS) for f in ("cn", "ms_rk4")]
MODEL_CASES += [(m, f) for m in ("unicycle", "cartpole") for f in ("forward", "backward", "midpoint", "ms_euler", "ms_rk2", "ms_rk3", "ms_rk5", "ms_rk7")]


def model_desc(model, formula, N=LONG_N):
    d = MODELS[model](N, MODEL_DT)
    if formula.startswith("ms_"):
        d.grid, d.defect, d.shooting_integrator = capi.GRID_MS, capi.DEFECT_RK4_SHOOTING, SHOOTING[formula[3:]]
    else:
        d.defect = COLLOCATION[formula]
    return d


def model_weights(model):
    return {"unicycle": problems.UNICYCLE_WEIGHTS, "kcar": problems.UNICYCLE_WEIGHTS, "vdp": problems.VDP_WEIGHTS, "int2": problems.INT3_WEIGHTS,
            "int3": problems.INT3_WEIGHTS}.get(model, problems.BENCHMARK_WEIGHTS)


def model_input(O, model, formula):
    """-> (desc, weights, X0 [B][nv], xf [B][nx]); bound rows are active at X0 (the Jacobian's bound entries are then -w / 0 / +w, not all zero)."""
    d = model_desc(model, formula)
    seed = 5200 + sum(map(ord, model + formula))
    rng = np.random.default_rng(seed)
    B, nx, s = MODEL_BATCH, d.nx, d.nx + d.nu
    if model in ("unicycle", "kcar"):
        x0, xf = problems.unicycle_instances(B, seed=seed)
    else:
        scale = 0.3 if model == "cartpole" else 1.0
        x0 = scale * rng.uniform(-1, 1, (B, nx))
        xf = scale * rng.uniform(-0.5, 0.5, (B, nx))
        if model == "rocket":   # third state = mass (a divisor): keep it away from zero
            x0[:, 2] = rng.uniform(0.9, 1.1, B)
            xf[:, 2] = rng.uniform(0.8, 1.0, B)
    xf = x0 + GOAL_FRACTION.get(model, 0.3) * (xf - x0)
    p = O.OracleProblem(d)
    X0 = np.stack([p.init_trajectory(x0[b], xf[b]) for b in range(B)])
    X0[:, nx:] += NOISE * rng.normal(size=X0[:, nx:].shape)
    for k in range(3, d.N - 1, PUSH_EVERY):
        X0[:, k * s + nx] = float(d.u_ub[0]) + PUSH
    return d, model_weights(model), X0, np.ascontiguousarray(xf)


# ---- the random campaign ----------------------------------------------------------------------------------------------------------------------
FUZZ_COUNT = 48
FUZZ_BATCH = 3
FUZZ_ITERATIONS = 3
FUZZ_BASE_SEED = 31000
# Seeds of the range whose inputs the oracle itself does not reproduce within the widening cap (8 x its one-ulp spread beyond WIDEN_CAP x the base tolerance),
# or on which it does not end with a finite chi2 and status converged / early terminated: replaced by the next integers (test_oracle_long_horizon.py asserts
# the condition on all FUZZ_COUNT seeds that remain).
FUZZ_REPLACED = ()
FUZZ_SEEDS = tuple([s for s in range(FUZZ_COUNT + len(FUZZ_REPLACED)) if s not in FUZZ_REPLACED][:FUZZ_COUNT])
assert len(FUZZ_SEEDS) == FUZZ_COUNT


def fuzz_input(O, seed):
    """-> (family, desc, weights, X0 [B][nv], xf [B][nx]).  random_desc's draw, then N uniform in 257 .. 1024 and a horizon of T = 3 .. 12 s (the short suite's
    steps of 0.05 .. 0.2 s would integrate unstable random systems over 200 s); every third seed with non-diagonal weights, drawn like
    test_gpu_fuzz.test_random_dense_weights_vs_oracle draws them.  The start is test_random_descriptor_vs_oracle's: off the straight line, so that bounds and
    inequalities get active."""
    rng = np.random.default_rng(FUZZ_BASE_SEED + seed)
    dense = seed % 3 == 0
    while True:
        fam, d = random_desc(rng, long_horizon=True)
        if not dense or (fam not in ("dint", "int3t") and d.grid in (capi.GRID_FD, capi.GRID_MS)):
            break
    d.N = int(rng.integers(257, 1025))
    d.dt_ref = float(rng.uniform(3.0, 12.0)) / (d.N - 1)
    nx, nu = d.nx, d.nu
    if dense:
        def factor(n):
            a = rng.uniform(-1, 1, (n, n))
            return np.linalg.cholesky(a.T @ a + 0.5 * np.eye(n)).T   # upper factor U, U^T U = the weight

        d.weights_dense = 1 | (2 if nu > 1 else 0) | (4 if d.final_cost else 0)
        for dst, U in ((d.q_sqrt, factor(nx)), (d.r_sqrt, factor(nu)), (d.qf_sqrt, factor(nx))):
            for i, v in enumerate(U.ravel()):
                dst[i] = float(v)
    B = FUZZ_BATCH
    w = tuple(float(v) for v in rng.uniform(1.0, 50.0, 3))
    x0 = rng.uniform(-1, 1, (B, nx))
    xf = rng.uniform(-1, 1, (B, nx)) + (np.array([1.5, 0.5, 0.2, 0.0])[:nx] if fam not in ("dint", "int3t") else np.array([1.0, 0.0, 0.0])[:nx])
    if fam == "rocket":   # third state = mass (a divisor): keep it away from zero
        x0[:, 2] = rng.uniform(0.9, 1.1, B)
        xf[:, 2] = rng.uniform(0.8, 1.0, B)
    p = O.OracleProblem(d)
    X0 = np.stack([p.init_trajectory(x0[b], xf[b]) for b in range(B)])
    X0 = X0 + 0.05 * rng.normal(size=X0.shape)
    X0[:, :nx] = x0
    if d.grid in (capi.GRID_FD_VARIABLE, capi.GRID_MS_VARIABLE):
        X0[:, -1] = d.dt_ref
    return str(fam), d, w, X0, np.ascontiguousarray(xf)


FUZZ_X_TOL = 3e-5     # relative to max(1, |x|): the base tolerances of test_gpu_fuzz.test_random_descriptor_vs_oracle


def fuzz_chi2_rtol(d):
    return 5e-4 if d.grid == capi.GRID_MS_VARIABLE else 5e-5
