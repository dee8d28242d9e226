"""GPU tests (-m gpu) of the stage equalities' non-integral state-control term e(x_k, u_k) = 0 (corbo_hip_problem_desc::stage_eq = CORBO_HIP_STAGE_FN_USER + slot;
user functions of csrc/stage_functions/, kind state_control_eq; EK_XU_EQ edges of the extra-edge sweep): values and central-difference Jacobian against the host
evaluator bit for bit, the LM step against the normal equations (tests/lm_step_check.py), LM iterates against oracle.GenericProblem, the two factorisation
routes against each other, batch / async / re-arm / per-pass modes, the closed loop, and the Hessian path's refusal.

No fixture of the genuine reference pins this term; tests/stage_function_eq_cases.py holds the reference construction, tests/test_oracle_stage_function_eq.py
asserts on the CPU that its tolerances stay inside the hard gate."""
import ctypes as C

import numpy as np
import pytest

import lm_step_check as L
import stage_function_eq_cases as E
from control_box_rst_amd import capi
from control_box_rst_amd.solver import BatchedLevenbergMarquardt, get_structure

pytestmark = pytest.mark.gpu

EVAL_IDS = [f"{n}-N{N}" for n, N in E.EVAL_CASES]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def starts(oracle_mod):
    """(name, N[, rejecting]) -> (desc, X0, xref); computed once per key, left unchanged"""
    cache = {}

    def get(name, N, rejecting=False):
        key = (name, N, rejecting)
        if key not in cache:
            cache[key] = E.rejecting_start(oracle_mod, name, N) if rejecting else E.make_start(oracle_mod, name, N)
        return cache[key]
    return get


def _handle(d, X0, xref, name, iters=1, route=0, B=None):
    B = X0.shape[0] if B is None else B
    s = BatchedLevenbergMarquardt(d, B, route=route)
    s.setIterations(iters)
    s.setPenaltyWeights(*E.penalty_weights(name))
    s.set_instance_data(X0[:B], xref=xref[:B])
    return s


def _small_block(name, N):
    return not name.startswith("quad") and N <= 256


def _expected_route(d, route=0):
    return capi.FACTOR_BAND if (route or d.nx > 4 or d.N > 256) else capi.FACTOR_BLOCK_TRI


# ---- 1. values and Jacobian ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, N", E.EVAL_CASES, ids=EVAL_IDS)
def test_values_and_jacobian_are_the_host_evaluators_bit_for_bit(starts, name, N):
    """corbo_hip_eval: the term's rows are w_eq e with e from the host evaluator (no max(0, .)); its Jacobian entries are the central differences of the host
    evaluator in the reference's order (x_i += delta -> v2; x_i += -2 delta -> v1; (1 / (2 delta)) (v2 - v1)) times w_eq; every other row and entry is what
    the same descriptor gives without the term."""
    d, X0, xref = starts(name, N)
    w = E.penalty_weights(name)
    s = _handle(d, X0, xref, name)
    if not name.startswith("par3"):
        assert s.factor_route() == _expected_route(d)
    values, jac = s.eval(*w)
    d0 = E.without_term(d)
    s0 = _handle(d0, X0, xref, name)
    values0, jac0 = s0.eval(*w)
    rows, cols = get_structure(d)
    trow = E.term_rows(d, s.dims)
    in_term = np.isin(rows, trow.ravel())
    row_in_term = np.zeros(s.dims.m, bool)
    row_in_term[trow.ravel()] = True
    assert row_in_term.sum() == s.dims.m - s0.dims.m and in_term.sum() == s.dims.nnz - s0.dims.nnz
    nx, S, r = d.nx, d.nx + d.nu, trow.shape[1]
    delta, scalar, w_eq = E.DELTA, 1.0 / (2 * E.DELTA), w[0]
    fn, prm = d.stage_eq, E.eq_params(d)
    for b in range(X0.shape[0]):
        # the rest of the problem: bit for bit the descriptor without the term
        assert np.array_equal(values[b][~row_in_term].view(np.int64), values0[b].view(np.int64)), (name, N, b)
        assert np.array_equal(jac[b][~in_term].view(np.int64), jac0[b].view(np.int64)), (name, N, b)
        e = E.term_values(d, X0[b])
        assert np.all(e != 0.0)
        want = e * w_eq
        assert np.array_equal(values[b][trow].view(np.int64), want.view(np.int64)), (name, N, b)
        # Jacobian: per interval, the unfixed components of x_k then u_k, one column each (value order: column by column, the edge's rows inside)
        z = X0[b][: (N - 1) * S].reshape(N - 1, S)
        got = jac[b][in_term]
        pos = 0
        for k in range(N - 1):
            comps = range(nx, S) if k == 0 else range(S)
            zk = np.repeat(z[k][None, :], 2 * len(comps), axis=0)
            for j, comp in enumerate(comps):
                a = z[k][comp] + delta
                zk[2 * j, comp] = a
                zk[2 * j + 1, comp] = a + -2 * delta
            v = capi.eval_stage_function_xu(fn, zk[:, :nx], zk[:, nx:], prm)
            wantj = (scalar * (v[0::2] - v[1::2])) * w_eq                       # [column][row]
            blk = got[pos: pos + len(comps) * r].reshape(len(comps), r)
            assert np.array_equal(blk.view(np.int64), wantj.view(np.int64)), (name, N, b, k)
            pos += len(comps) * r
        assert pos == len(got)


# ---- 2. the LM step -----------------------------------------------------------------------------------------------------------------------------------
def _step_cases():
    out = []
    for name, N in E.EVAL_CASES:
        for rejecting in (False, True):
            for route in ((0, capi.ROUTE_XE_BAND) if _small_block(name, N) else (0,)):
                out.append((name, N, rejecting, route))
    return out


@pytest.fixture(scope="module")
def step_reference(oracle_mod, starts):
    cache = {}

    def get(name, N, rejecting):
        key = (name, N, rejecting)
        if key not in cache:
            d, X0, xref = starts(name, N, rejecting)
            w = E.penalty_weights(name)
            if N > E.STEP_REFERENCE_NONE_ABOVE:
                # no dense callback reference beyond this horizon: instance 0 alone, the Reference's pass count as recorded in STEP_PASSES_LONG (the CPU twin
                # computes it again), and the strictest bound the helper gives -- DEVICE_MARGIN x 2^-53, i.e. a reference eta of zero
                voff = oracle_mod.OracleProblem(E._bare(d)).param_offsets().astype(np.int64)
                passes, accepted = E.STEP_PASSES_LONG[key]
                cache[key] = [dict(off=voff, n=len(voff), fixed=np.setdiff1d(np.arange(X0.shape[1]), voff), passes=passes, accepted=accepted)]
            else:
                cache[key] = [E.Reference(oracle_mod, d, X0[b], xref[b]).first_iteration(w) for b in range(E.step_instances(N))]
        return cache[key]
    return get


@pytest.mark.parametrize("name, N, rejecting, route", _step_cases(), ids=[f"{n}-N{N}{'-rej' if rj else ''}{'-band' if rt else ''}" for n, N, rj, rt in _step_cases()])
def test_lm_step_solves_the_normal_equations(starts, step_reference, name, N, rejecting, route):
    """One iteration from the jittered start (and from one whose first step is rejected): the step the device took solves
    (J^T J + sum(mu) I) delta = -J^T r of ITS Jacobian and residual at the start to the normwise backward error lm_step_check allows -- DEVICE_MARGIN (16) x
    max(the reference's own eta, 2^-53) -- with the damping the reference's pass count implies; through the default route and the forced band route.  The
    handle's counters must show the reference's passes and accepted steps (beyond 100 grid points: of instance 0, the only one checked there)."""
    d, X0, xref = starts(name, N, rejecting)
    rec = step_reference(name, N, rejecting)
    X0, xref = X0[: len(rec)], xref[: len(rec)]
    s = _handle(d, X0, xref, name, route=route)
    if route or not name.startswith("par3"):
        assert s.factor_route() == _expected_route(d, route)
    values, jac = s.eval()
    s.restore_instance_data()
    s.solve()
    x1, chi2, _ = s.get_solution()
    stats = s.get_stats()
    rows, cols = get_structure(d)
    failures = []
    for b, o in enumerate(rec):
        eta_ref = L.eta_of(o) if "jac" in o else 0.0
        delta = x1[b][o["off"]] - X0[b][o["off"]]
        sum_mu = L.expected_damping(L.initial_damping(cols, jac[b], o["n"]), o["passes"])
        eta = L.step_backward_error(rows, cols, jac[b], values[b], delta, sum_mu)
        bound = L.DEVICE_MARGIN * max(eta_ref, L.U)
        print(f"EQSTEP {name}-N{N} route={route} [{b}] passes={o['passes']} accepted={o['accepted']} eta_device={eta:.3e} eta_ref={eta_ref:.3e} bound={bound:.3e}")
        if not eta <= bound:
            failures.append((b, eta, bound))
        assert np.array_equal(x1[b][o["fixed"]].view(np.int64), X0[b][o["fixed"]].view(np.int64)), (name, b, "a vertex entry that is no parameter moved")
    assert not failures, (name, N, route, failures)
    passes, accepted = sum(o["passes"] for o in rec), sum(o["accepted"] for o in rec)
    assert stats["factorizations"] == passes and stats["accepted_steps"] == accepted and stats["rejected_steps"] == passes - accepted, (stats, passes, accepted)
    if rejecting:
        assert passes > len(rec)


# ---- 3. iterates --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, N, start, iterations", E.ITERATE_CASES, ids=E.ITERATE_IDS)
def test_lm_iterates_vs_generic_oracle(oracle_mod, name, N, start, iterations):
    """Iterates and chi2 after k iterations (1 .. 5; the quadrotor: 1, 2) against stage_function_eq_cases.Reference; tolerance max(5e-6 / 2e-6, 4 x the
    oracle's own one-ulp spread), which test_oracle_stage_function_eq.py holds at or below 1e-5."""
    d, X0, xref = E.make_start(oracle_mod, name, N, **start)
    w = E.penalty_weights(name)
    ref = E.Reference(oracle_mod, d, X0[0], xref[0])
    for k in iterations:
        xo, co, xtol, ctol = ref.iterate_with_spread(k, w)
        assert xtol <= E.HARD_X and ctol <= E.HARD_CHI2
        s = _handle(d, X0, xref, name, iters=k, B=1)
        s.solve(new_run=True)
        Xd, chi2, _ = s.get_solution()
        ex, ec = np.abs(Xd[0][ref.voff] - xo).max(), abs(chi2[0] - co) / abs(co)
        print(f"EQITER {name}-N{N} k={k} |dx|={ex:.3e} (tol {xtol:.1e}) dchi2={ec:.3e} (tol {ctol:.1e})")
        assert ex <= xtol, (name, k, ex, xtol)
        assert ec <= ctol, (name, k, chi2[0], co, ctol)


# ---- 4. routes and modes --------------------------------------------------------------------------------------------------------------------------------
ROUTE_CASES = (("unicycle", 3), ("unicycle", 12), ("unicycle+envelope+unorm+rate", 12), ("unicyclet", 12), ("unicyclems", 12), ("unicycle", 129))


@pytest.mark.parametrize("name, N", ROUTE_CASES, ids=[f"{n}-N{N}" for n, N in ROUTE_CASES])
def test_block_tridiagonal_route_vs_band_route(starts, name, N):
    """The same handles through both routes: same accept / reject decisions, within 2e-6 of each other (the cross-route figure of test_gpu_extra_edges.py)."""
    d, X0, xref = starts(name, N)
    out = []
    for route in (0, capi.ROUTE_XE_BAND):
        s = _handle(d, X0, xref, name, iters=5, route=route)
        assert s.factor_route() == (capi.FACTOR_BAND if route else capi.FACTOR_BLOCK_TRI), (name, route)
        s.solve()
        x, chi2, status = s.get_solution()
        out.append((x.copy(), chi2.copy(), status.copy(), s.get_stats()))
    (x0, c0, s0, t0), (x1, c1, s1, t1) = out
    assert np.array_equal(s0, s1)
    for k in ("factorizations", "accepted_steps", "rejected_steps", "jacobian_sweeps"):
        assert t0[k] == t1[k], (name, k, t0, t1)
    assert np.abs(x0 - x1).max() <= 2e-6 * max(1.0, np.abs(x1).max()), (name, np.abs(x0 - x1).max())
    assert np.allclose(c0, c1, rtol=2e-6, atol=0), (name, c0, c1)


def test_routes_reported():
    """BLOCK_TRI up to 256 grid points, BAND at 257 and around the quadrotor; the forced band route everywhere.  par3 (S = 6, two rows per edge): whichever
    route its product lists admit -- printed here and recorded in docs/measurements/r13.md (BLOCK_TRI: its lists stay inside the 32-round limit);
    test_par3_routes_agree holds the two routes against each other."""
    want = {("unicycle", 3): capi.FACTOR_BLOCK_TRI, ("unicycle", 12): capi.FACTOR_BLOCK_TRI, ("unicycle", 129): capi.FACTOR_BLOCK_TRI, ("unicycle", 256): capi.FACTOR_BLOCK_TRI,
            ("unicycle", 257): capi.FACTOR_BAND, ("unicyclems", 12): capi.FACTOR_BLOCK_TRI, ("unicyclet", 12): capi.FACTOR_BLOCK_TRI, ("quad", 6): capi.FACTOR_BAND,
            ("quad", 7): capi.FACTOR_BAND}
    for (name, N), route in want.items():
        d = E.make_desc(name, N)
        assert BatchedLevenbergMarquardt(d, 2).factor_route() == route, (name, N)
        assert BatchedLevenbergMarquardt(d, 2, route=capi.ROUTE_XE_BAND).factor_route() == capi.FACTOR_BAND, (name, N)
    got = BatchedLevenbergMarquardt(E.make_desc("par3", 12), 2).factor_route()
    print(f"EQROUTE par3-N12 factor_route={got} (BAND = {capi.FACTOR_BAND}, BLOCK_TRI = {capi.FACTOR_BLOCK_TRI})")
    assert got in (capi.FACTOR_BAND, capi.FACTOR_BLOCK_TRI)
    assert BatchedLevenbergMarquardt(E.make_desc("par3", 12), 2, route=capi.ROUTE_XE_BAND).factor_route() == capi.FACTOR_BAND


def test_par3_routes_agree(starts):
    d, X0, xref = starts("par3", 12)
    out = []
    for route in (0, capi.ROUTE_XE_BAND):
        s = _handle(d, X0, xref, "par3", iters=5, route=route)
        s.solve()
        x, chi2, status = s.get_solution()
        out.append((x.copy(), chi2.copy(), status.copy(), s.get_stats()))
    (x0, c0, s0, t0), (x1, c1, s1, t1) = out
    assert np.array_equal(s0, s1) and t0["factorizations"] == t1["factorizations"] and t0["accepted_steps"] == t1["accepted_steps"]
    assert np.abs(x0 - x1).max() <= 2e-6 * max(1.0, np.abs(x1).max()) and np.allclose(c0, c1, rtol=2e-6, atol=0)


def test_batch_of_600_is_per_instance_bitwise(starts):
    """600 instances (the three starts, 200 times) against three single handles, bit for bit."""
    name, N = "unicycle", 12
    d, X0, xref = starts(name, N)
    reps = 200
    Xb, xb = np.tile(X0, (reps, 1)), np.tile(xref, (reps, 1))
    s = _handle(d, Xb, xb, name, iters=5)
    s.solve()
    X, c, st = s.get_solution()
    assert np.all(np.isfinite(X))
    for b in range(X0.shape[0]):
        s1 = _handle(d, X0[b: b + 1], xref[b: b + 1], name, iters=5)
        s1.solve()
        x1, c1, t1 = s1.get_solution()
        same = X[b::3].view(np.int64) == x1[0].view(np.int64)[None, :]
        assert same.all() and np.all(c[b::3] == c1[0]) and np.all(st[b::3] == t1[0]), (b, np.nonzero(~same.all(axis=1))[0][:5])


@pytest.mark.parametrize("name, N", [("unicycle+envelope+unorm+rate", 12), ("par3", 12), ("quad", 6), ("unicycle", 257)], ids=["unicycle+envelope+unorm+rate-N12", "par3-N12", "quad-N6", "unicycle-N257"])
def test_modes_agree(starts, name, N):
    """solve, solve_async and the re-armed solve of one handle, bitwise.  The per-pass mode of the same handle runs the band kernels: it is bitwise equal to the
    others only where the handle's route is the band route.  On a block-tridiagonal handle it is another elimination order of the same H, held to the same
    decisions and to 2e-6 of the run-to-completion result."""
    d, X0, xref = starts(name, N)
    s = _handle(d, X0, xref, name, iters=5)
    s.solve()
    Xb, cb, sb = [a.copy() for a in s.get_solution()]
    st = s.get_stats()
    assert np.all(np.isfinite(Xb))
    s.restore_instance_data()
    s.solve_async()
    s.synchronize()
    Xa, ca, sa = s.get_solution()
    assert np.array_equal(Xa.view(np.int64), Xb.view(np.int64)) and np.array_equal(ca, cb) and np.array_equal(sa, sb)
    s.set_result_sink(True)
    for _ in range(2):
        s.solve_async(rearm=True)
    s.synchronize()
    Xr, cr, sr = s.fetch_solution()
    assert np.array_equal(np.asarray(Xr)[:, : Xb.shape[1]].view(np.int64), Xb.view(np.int64)) and np.array_equal(cr, cb) and np.array_equal(sr, sb)
    s.set_result_sink(False)
    s.set_option("run_to_completion", 0)
    s.restore_instance_data()
    s.solve()
    Xp, cp, sp_ = s.get_solution()
    stp = s.get_stats()
    assert np.array_equal(sp_, sb) and stp["factorizations"] == st["factorizations"] and stp["accepted_steps"] == st["accepted_steps"]
    if s.factor_route() == capi.FACTOR_BAND:   # the same kernels either way
        assert np.array_equal(Xp.view(np.int64), Xb.view(np.int64)) and np.array_equal(cp, cb)
    else:                                       # two elimination orders of the same H
        assert np.abs(Xp - Xb).max() <= 2e-6 * max(1.0, np.abs(Xb).max()) and np.allclose(cp, cb, rtol=2e-6, atol=0)


# ---- 5. closed loop -------------------------------------------------------------------------------------------------------------------------------------
def test_closed_loop_call_equals_stepwise_sequence():
    """Three steps of corbo_hip_closed_loop with the term on (unicycle, N = 12): bit-identical to the step-by-step entry points."""
    from control_box_rst_amd import problems
    d = E.make_desc("unicycle", 12)
    B, steps = E.BATCH, 3
    x0, xf = problems.unicycle_instances(B)
    rng = np.random.default_rng(12)
    dist = 1e-3 * rng.normal(size=(steps, B, d.nx))
    dt = d.dt_ref
    a, b = BatchedLevenbergMarquardt(d, B), BatchedLevenbergMarquardt(d, B)
    for s in (a, b):
        s.setIterations(4)
        s.setPenaltyWeights(*E.penalty_weights("unicycle"))
        s.set_instance_data(s.init_trajectory(x0, xf), xref=xf)
        s.solve(new_run=True)
        s.plant_set_state(x0)
    xs, us = a.closed_loop(steps, dt=dt, integrator=capi.INTEGRATOR_RK4, shift=True, disturbance=dist)
    for k in range(steps):
        u_applied = b.get_first_control()
        b.plant_step(dt=dt, integrator=capi.INTEGRATOR_RK4, disturbance=dist[k])
        assert np.array_equal(us[k], u_applied), k
        assert np.array_equal(xs[k], b.plant_get_state()), k
        b.warm_start_from_plant(shift=True)
        b.solve(new_run=True)
    Xa, ca, sa = a.get_solution()
    Xb, cb, sb = b.get_solution()
    assert np.array_equal(Xa, Xb) and np.array_equal(ca, cb) and np.array_equal(sa, sb)
    assert np.array_equal(a.plant_get_state(), b.plant_get_state())
    # the term is on: the first control obeys the tie to rounding of the penalty solve's residual, and differs from the plain problem's
    p = BatchedLevenbergMarquardt(E.without_term(d), B)
    p.setIterations(4)
    p.setPenaltyWeights(*E.penalty_weights("unicycle"))
    p.set_instance_data(p.init_trajectory(x0, xf), xref=xf)
    p.solve(new_run=True)
    assert not np.array_equal(p.get_first_control(), us[0])


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_hessian_path_operators_are_refused(starts):
    d, X0, xref = starts("unicycle", 12)
    s = _handle(d, X0, xref, "unicycle")
    B = X0.shape[0]
    grad, obj = np.zeros((B, s.dims.n)), np.zeros(B)
    dp = C.POINTER(C.c_double)
    assert s.lib.corbo_hip_eval_objective_gradient(s._h, grad.ctypes.data_as(dp), obj.ctypes.data_as(dp)) == -3
    assert "stage_eq" in s.lib.corbo_hip_last_error().decode()
    big = np.zeros(1 << 16)
    p = big.ctypes.data_as(dp)
    assert s.lib.corbo_hip_eval_hessians(s._h, 1, 1.0, None, None, p, p, p) == -3
    assert s.lib.corbo_hip_eval_linear_form(s._h, p, p, p) == -3
