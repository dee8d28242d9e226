"""The machinery of lm_step_check.py on the oracle (CPU): one LM iteration per input of the table test_gpu_linear_solve.py runs on the device -- the
reference computation of that file is under test wherever the suite runs.

  * the oracle's envelope Cholesky solves (J^T J + sum(mu) I) delta = -J^T r to a backward error eta <= 1e-14 on every input (measured maximum 1.5e-15:
    docs/measurements/r08.md), with the cumulative damping mu_0 (1 + 2 + 8 + 64 + ...) of the passes its trace reports;
  * the conditions the device file relies on: exactly one pass on the accepted-at-once starts, three or more on the rejecting ones, a step of at least a
    twentieth of the iterate (eta is computed from fl(x_0 + delta) - x_0);
  * the check can fail: the last mu alone in place of the sum, one entry of a mid-horizon defect block off by 1e-9 relative, one cost row's Gram term dropped
    -- each lands above the bound the device file applies.
Nothing is written."""
import numpy as np
import pytest

import lm_step_check as L

INPUTS = L.unique_inputs()


@pytest.fixture(scope="module")
def first_iterations(oracle_mod):
    """input key -> (X0, records of the oracle's first iteration); computed once, shared, left unchanged"""
    cache = {}

    def get(case):
        if case.input_key not in cache:
            d, X0, xref = L.make_start(case, oracle_mod)
            cache[case.input_key] = (X0, L.oracle_first_iteration(oracle_mod, case, d, X0, xref))
        return cache[case.input_key]
    return get


def test_table_covers_the_listed_paths():
    ids = {c.id for c in L.CASES}
    assert len(ids) == len(L.CASES) >= 413
    for route in ("cr", "long", "bt", "band", "big"):
        assert sum(L.BATCH for c in L.unique_inputs() if c.route == route and c.rejecting) >= 2, route   # at least two rejecting instances per route
    assert 2 <= L.BATCH <= 4


def _long_plan(lib, d):
    """(threads, workgroups per CU the LDS admits, non-diagonal weights) of corbo_hip_long_factor_plan: the instantiation class of factor_long_kernel"""
    import ctypes as C
    out = (C.c_int32 * 4)()
    assert lib.corbo_hip_long_factor_plan(C.byref(d), C.byref(out)) == 0, lib.corbo_hip_last_error()
    assert out[2] % 8 == 0 and (out[2] > 0) == (out[1] > 0) and out[2] + 128 + 64 <= 160 * 1024
    return (out[0], out[1], out[3])


def test_long_route_straddles_every_switch_of_the_launcher():
    """The long-horizon cases against the launcher's own decision (corbo_hip_long_factor_plan; host only).  Per block shape (nx, nu, free dt) of the long route:
    every instantiation class the plan returns for some N in 257 .. 1024 has a case, and wherever the class changes between N and N + 1 both horizons are
    cases of that shape.  A layout change that moves a switch fails here: the table cannot silently stop straddling it."""
    from control_box_rst_amd import capi
    lib = capi.load()
    shapes = {}   # (nx, nu, free dt, dense) -> {N: family}
    for c in L.CASES:
        if c.route == "long":
            d = L.make_desc(c.family, c.N)
            free = d.grid in (capi.GRID_FD_VARIABLE, capi.GRID_MS_VARIABLE)
            shapes.setdefault((d.nx, d.nu, free, bool(d.weights_dense)), {})[c.N] = c.family
    assert {k[:3] for k in shapes} == {(2, 1, False), (2, 1, True), (2, 2, False), (3, 1, False), (3, 1, True), (3, 2, False), (3, 3, False), (4, 1, False), (4, 1, True)}
    for (nx, nu, free, dense), have in sorted(shapes.items()):
        fam = next(iter(have.values()))
        plan = {N: _long_plan(lib, L.make_desc(fam, N)) for N in range(257, 1025)}
        reached = {plan[N] for N in have}
        if dense:   # the non-diagonal instantiations: with and without the LDS carve where the shape reaches both in the table's families
            assert reached <= set(plan.values()) and all(p[2] == 1 for p in reached), (nx, nu, free)
            continue
        assert reached == set(plan.values()), ((nx, nu, free), sorted(set(plan.values()) - reached))
        for N in range(257, 1024):
            if plan[N] != plan[N + 1]:
                assert N in have and N + 1 in have, ((nx, nu, free), N, plan[N], plan[N + 1])
    dense_classes = {_long_plan(lib, L.make_desc(c.family, c.N))[:2] for c in L.CASES if c.route == "long" and "+dense" in c.family}
    assert dense_classes == {(1024, 2), (1024, 1), (1024, 0)}   # E with two / one workgroup per CU, F


def test_long_factor_plan_switches():
    """the switches of docs/measurements/r10.md, from the library: c (N | 1) + 130 doubles (+ nx (N | 1) with a free dt) + the LM state + 64 bytes against 160 KB"""
    from control_box_rst_amd import capi
    lib = capi.load()
    two_one = ((1024, 2), (1024, 1))   # nx = 2: the same sixteen-wave instantiation, two | one workgroup per CU
    want = {"vdp": {775: two_one}, "dint": {671: two_one}, "par2": {775: two_one},
            "int3": {373: ((512, 2), (512, 1)), 751: ((1024, 1), (1024, 0))}, "par3": {373: ((512, 2), (512, 1)), 751: ((1024, 1), (1024, 0))},
            "unicycle": {373: ((512, 2), (512, 1)), 751: ((1024, 1), (1024, 0))},
            "int3t": {335: ((512, 2), (512, 1)), 677: ((1024, 1), (1024, 0))},
            "cartpole": {441: ((512, 1), (1024, 0))}, "cartpolet": {405: ((512, 1), (1024, 0))}}
    for fam, sw in want.items():
        plan = {N: _long_plan(lib, L.make_desc(fam, N))[:2] for N in range(257, 1025)}
        got = {N: (plan[N], plan[N + 1]) for N in range(257, 1024) if plan[N] != plan[N + 1] and N != 512}
        assert got == sw, (fam, got)
        assert plan[512][0] == 512 or plan[512][1] == 0, fam
        assert plan[513][0] == 1024, fam


def test_expected_damping_is_the_inner_loops_sum():
    mu0 = 0.3
    assert L.expected_damping(mu0, 1) == mu0 and L.last_damping(mu0, 1) == mu0
    assert L.expected_damping(mu0, 2) == mu0 * 3 and L.last_damping(mu0, 2) == mu0 * 2
    assert L.expected_damping(mu0, 4) == pytest.approx(mu0 * (1 + 2 + 8 + 64), rel=1e-15) and L.last_damping(mu0, 4) == pytest.approx(mu0 * 64, rel=1e-15)


def test_backward_error_of_an_exact_and_of_a_wrong_solve():
    """a dense 3 x 2 system by hand: eta of the exact step is at rounding level, eta of a step that is off by 1e-6 is about 1e-6"""
    rows, cols = np.array([0, 0, 1, 2, 2]), np.array([0, 1, 1, 0, 1])
    jac, r, mu = np.array([2.0, -1.0, 3.0, 0.5, 1.5]), np.array([1.0, -2.0, 0.25]), 0.125
    J = np.zeros((3, 2))
    J[rows, cols] = jac
    delta = np.linalg.solve(J.T @ J + mu * np.eye(2), -J.T @ r)
    assert L.step_backward_error(rows, cols, jac, r, delta, mu) <= 4 * L.U
    assert 1e-7 <= L.step_backward_error(rows, cols, jac, r, delta * (1 + 1e-6), mu) <= 1e-6
    assert L.forward_error(rows, cols, jac, r, delta, mu) <= 16 * L.U


@pytest.mark.parametrize("case", INPUTS, ids=[c.id for c in INPUTS])
def test_oracle_step_solves_the_normal_equations(first_iterations, case):
    X0, rec = first_iterations(case)
    assert len(rec) == L.BATCH
    for b, o in enumerate(rec):
        eta = L.eta_of(o)
        step = np.abs(o["delta"]).max() / np.abs(X0[b]).max()
        print(f"{case.id} [{b}] passes={o['passes']} eta={eta:.2e} step/iterate={step:.3f}")
        assert o["accepted"] == 1, (case.id, b)
        if case.rejecting:
            assert o["passes"] >= 3, (case.id, b, o["passes"])
        else:
            assert o["passes"] == 1, (case.id, b, o["passes"])
        assert step >= 0.05, (case.id, b, step)
        assert eta <= L.ORACLE_BOUND, (case.id, b, eta)
        assert np.array_equal(o["x1"][o["fixed"]].view(np.int64), X0[b][o["fixed"]].view(np.int64)), (case.id, b)
        assert len(o["off"]) == o["n"] and len(o["fixed"]) + o["n"] == len(X0[b])


def test_weighted_handle_reference_solves_its_normal_equations(oracle_mod):
    """the host-assembled reference of the corbo_hip_create_weighted case (lm_step_check.weighted_case): accepted at once, same conditions, same bound"""
    _, _, X0, _, rec = L.weighted_case(oracle_mod)
    for b, o in enumerate(rec):
        eta, step = L.eta_of(o), np.abs(o["delta"]).max() / np.abs(X0[b]).max()
        print(f"weighted [{b}] eta={eta:.2e} step/iterate={step:.3f}")
        assert o["accepted"] == 1 and o["passes"] == 1 and step >= 0.05 and eta <= L.ORACLE_BOUND, (b, o["accepted"], step, eta)


# ---- the check can fail (no kernel is touched): at least three inputs per route class; the rejecting ones carry the damping defect (only there the sum of the
#      mu differs from the last mu).  Left out on purpose: the quadrotor with a rate limit (band-quad+rate-*) -- its rate rows (1 / dt = 20, penalty weight 10) put
#      entries of 4e4 into |H|_inf next to defect entries of order one, and eta is a NORMWISE measure: one defect entry off by 1e-9 gives 8.7e-16 (N = 20, accepted
#      at once) resp. moves eta by less than 1e-17 (rejecting starts: sum(mu) = 1099 mu_0 after five passes) against a bound of 1.8e-15.  The damping and Gram-term
#      defects show there like everywhere else (5e-4, 1e-3).  docs/measurements/r08.md.
_SENSITIVITY_IDS = ("cr-unicyclems-N8-rej0", "cr-unicyclems-N33-rej0", "cr-unicycle-N100-rej0", "cr-int3t-N65",
                    "long-unicycle-N257-rej1", "long-unicycle-N257-rej2", "long-unicycle-N800", "long-dint-N513",
                    "long-cartpole-N442", "long-par3-N752", "long-int3t-N336",
                    "bt-unicycle+rate-N6-rej0-bt_waves2", "bt-unicycle+rate-N12-rej0-bt_waves2", "bt-unicycle+rate-N40-rej0-bt_waves2", "bt-int3t+eqlin-N129-bt_waves2",
                    "band-cartpole+rate-N257-rej5", "band-unicycle+rate+eqlin+dense-N12", "band-vdp+eqlin-N300-route2-band_wide0",
                    "big-quad-N37-rej0-chain_variant2-reject_speculation0", "big-pquad-N65-chain_variant2", "big-quadt-N37-chain_variant2", "big-quad-N64-chain_variant2")
SENSITIVITY = [c for c in INPUTS if c.id in _SENSITIVITY_IDS]
assert len(SENSITIVITY) == len(_SENSITIVITY_IDS)


def _mid_row(o, lo, hi):
    """the row of [lo, hi) nearest the middle that has Jacobian entries, and the index of its largest entry"""
    rows = np.asarray(o["rows"])
    for r in sorted(range(lo, hi), key=lambda v: abs(v - (lo + hi) // 2)):
        idx = np.nonzero((rows == r) & (o["jac"] != 0.0))[0]
        if len(idx):
            return r, idx[np.argmax(np.abs(o["jac"][idx]))]
    raise AssertionError("no row with entries")


@pytest.mark.parametrize("case", SENSITIVITY, ids=[c.id for c in SENSITIVITY])
def test_defects_land_above_the_device_bound(first_iterations, oracle_mod, case):
    X0, rec = first_iterations(case)
    d = L.make_desc(case.family, case.N)
    dims = oracle_mod.OracleProblem(d).dims
    for b, o in enumerate(rec):
        bound = L.DEVICE_MARGIN * max(L.eta_of(o), L.U)
        if o["passes"] > 1:   # the last mu alone in place of the cumulative damping
            eta = L.eta_of(o, sum_mu=L.last_damping(o["mu0"], o["passes"]))
            print(f"{case.id} [{b}] last mu alone: eta={eta:.2e} bound={bound:.2e}")
            assert eta > bound, (case.id, b, "last mu", eta, bound)
        else:
            assert not case.rejecting
        # one entry of a mid-horizon defect block (equality rows follow the cost rows) off by 1e-9 relative
        _, i = _mid_row(o, dims.lsq, dims.lsq + dims.eq)
        jac = o["jac"].copy()
        jac[i] *= 1.0 + 1e-9
        eta = L.eta_of(o, jac=jac)
        print(f"{case.id} [{b}] defect entry (1 + 1e-9): eta={eta:.2e} bound={bound:.2e}")
        assert eta > bound, (case.id, b, "defect entry", eta, bound)
        # one cost row's Gram term dropped
        r, _ = _mid_row(o, 0, dims.lsq)
        jac, values = o["jac"].copy(), o["values"].copy()
        jac[np.asarray(o["rows"]) == r] = 0.0
        values[r] = 0.0
        eta = L.eta_of(o, jac=jac, values=values)
        print(f"{case.id} [{b}] cost row dropped: eta={eta:.2e} bound={bound:.2e}")
        assert eta > bound, (case.id, b, "cost row", eta, bound)
