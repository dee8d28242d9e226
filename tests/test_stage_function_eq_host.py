"""CPU tests of the stage equalities' non-integral state-control term (corbo_hip_problem_desc::stage_eq = CORBO_HIP_STAGE_FN_USER + slot, csrc/stage_functions/
kind state_control_eq): registry, structure in the reference's creation order (the edge in front of the interval's dynamics edge, finite_differences_grid.cpp:58-61,
102-108 -- read there, asserted structurally: no fixture of the genuine reference has this term), the gate's refusals and the host evaluator against the
headers' formulas written out in numpy.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import stage_function_eq_cases as E
from control_box_rst_amd import capi, problems, solver


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return capi.load()


def test_kinds_and_rows_of_the_shipped_functions(lib):
    """(The shapes are {slot: (rows, nu_min)} like user_stage_function_shapes(): heading_tie reads u[1] -- nu_min 2 --, input_circle u[2] -- nu_min 3.)"""
    U = capi.STAGE_FN_USER
    assert lib.corbo_hip_stage_function_kind(U + 4) == 3 and lib.corbo_hip_stage_function_kind(U + 6) == 3
    assert lib.corbo_hip_stage_function_rows(U + 4) == 1 and lib.corbo_hip_stage_function_rows(U + 6) == 2
    for s in (5, 7, 9):
        assert lib.corbo_hip_stage_function_kind(U + s) == -1 and lib.corbo_hip_stage_function_rows(U + s) == -1
    import __graft_entry__ as g
    assert g.user_stage_function_shapes() == {2: (1, 1), 3: (4, 2)}
    assert g.user_stage_equality_shapes() == {4: (1, 2), 6: (2, 3)}
    fns = [f[:4] for f in g.user_stage_functions()]
    assert ("heading_tie", 4, 3, 3) in fns and ("input_circle", 6, 3, 3) in fns
    reg = open(g.os.path.join(g.CSRC, "stage_functions", "_registry.inc")).read()
    assert "CORBO_HIP_USER_STAGE_XU_EQ(heading_tie, 4, 1, 3, 2)" in reg and "CORBO_HIP_USER_STAGE_XU_EQ(input_circle, 6, 2, 3, 3)" in reg
    assert "CORBO_HIP_USER_STAGE_XU(heading_tie" not in reg and "CORBO_HIP_USER_STAGE_XU(input_circle" not in reg


def _structure(d):
    dims = solver.get_dims(d)
    rows, cols = solver.get_structure(d)
    return dims, rows, cols


@pytest.mark.parametrize("name", ["unicycle", "par3", "unicycle+envelope+unorm+rate", "unicyclems", "unicyclet"])
def test_structure_follows_the_creation_order(lib, oracle_mod, name):
    """N = 4: the term's rows of interval k sit in front of its defect rows, at lsq + k (nx + rows) + j; columns x_k then u_k; interval 0 (x_0 fixed) has no x
    columns; every other entry is the old structure, rows shifted past the inserted ones (with the inequality extras on: the inequality section is what it
    was, shifted by the equality section's growth)."""
    N = 4
    d = E.make_desc(name, N)
    d0 = E.without_term(d)
    dims, rows, cols = _structure(d)
    dims0, rows0, cols0 = _structure(d0)
    nx, nu, S = d.nx, d.nu, d.nx + d.nu
    r = {"unicycle": 1, "par3": 2}.get(name.split("+")[0], 1)
    assert capi.stage_function_rows(d.stage_eq) == r
    assert dims.eq == dims0.eq + r * (N - 1)
    assert dims.lsq == dims0.lsq and dims.ineq == dims0.ineq and dims.bounds == dims0.bounds and dims.n == dims0.n and dims.m == dims0.m + r * (N - 1)
    assert dims.nnz == dims0.nnz + r * (nu + (N - 2) * S)
    voff = oracle_mod.OracleProblem(E._bare(d)).param_offsets().astype(np.int64)
    col_of = {int(v): c for c, v in enumerate(voff)}
    trow = E.term_rows(d, dims)
    assert trow[0][0] == dims.lsq and trow[-1][-1] == dims.lsq + (N - 2) * (nx + r) + r - 1
    for k in range(N - 1):
        assert [int(t) for t in trow[k]] == [dims.lsq + k * (nx + r) + j for j in range(r)]
        want_cols = [col_of[k * S + c] for c in range(S) if k * S + c in col_of]   # x_k then u_k, unfixed components only
        assert len(want_cols) == (nu if k == 0 else S)
        idx = np.nonzero(np.isin(rows, trow[k]))[0]
        assert np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx))), "one contiguous block of values per edge"
        # value order of an edge's block: column by column, the edge's rows inside a column
        assert rows[idx].tolist() == [int(t) for _ in want_cols for t in trow[k]]
        assert cols[idx].tolist() == [c for c in want_cols for _ in trow[k]]
        # ... in front of the interval's dynamics edge
        first_defect = np.nonzero(rows == dims.lsq + k * (nx + r) + r)[0][0]
        assert idx[-1] + 1 == first_defect
    keep = ~np.isin(rows, trow.ravel())
    shift = np.searchsorted(np.sort(trow.ravel()), rows[keep])
    assert np.array_equal(rows[keep] - shift, rows0) and np.array_equal(cols[keep], cols0)
    # the inequality section: the old one, shifted by the equality section's growth
    in_ineq = rows >= dims.lsq + dims.eq
    in_ineq0 = rows0 >= dims0.lsq + dims0.eq
    assert np.array_equal(rows[in_ineq] - r * (N - 1), rows0[in_ineq0]) and np.array_equal(cols[in_ineq], cols0[in_ineq0])


def test_field_zero_and_the_linear_row_are_the_descriptors_of_before(lib):
    """stage_eq = 0 -- set and cleared again -- has the bytes, dims and structure of a copy taken before; a CORBO_HIP_STAGE_EQ_LINEAR descriptor keeps its
    structure (one integral row per interval, needs its integration rule); the descriptor's size and the field's offset are what they were."""
    for mk in (lambda: problems.unicycle_desc(N=12), lambda: problems.quad_desc(N=8), lambda: problems.parallel_integrator_desc(p=3, N=12)):
        d = mk()
        before = E.copy_desc(d)
        dims_b, rows_b, cols_b = _structure(before)
        problems.with_state_control_eq(d, E.INPUT_CIRCLE if d.nu >= 3 else E.HEADING_TIE, (0.3, 0.1, 0.2, 0.1))
        assert solver.get_dims(d).eq > dims_b.eq
        d = E.without_term(d)
        assert bytes(d) == bytes(before)
        dims_a, rows_a, cols_a = _structure(d)
        assert dims_a.as_dict() == dims_b.as_dict() and np.array_equal(rows_a, rows_b) and np.array_equal(cols_a, cols_b)
    assert C.sizeof(capi.ProblemDesc) == lib.corbo_hip_sizeof(0)
    assert len(capi.ProblemDesc().stage_eq_params) >= 8
    # the linear integral row: LeftSum = one row in front of the defect, Trapezoidal = appended; refused without a rule and on the shooting grids, as before
    base = solver.get_dims(problems.unicycle_desc(N=12))
    for rule in (1, 2):
        d = problems.unicycle_desc(N=12)
        d.stage_eq, d.constraint_integration = capi.STAGE_EQ_LINEAR, rule
        d.stage_eq_params[0], d.stage_eq_params[3], d.stage_eq_params[5] = 1.0, 0.5, 0.1
        dims = solver.get_dims(d)
        assert dims.eq == base.eq + 11 and dims.m == base.m + 11
        rows, _ = solver.get_structure(d)
        if rule == 2:   # LeftSum: the integral row of interval 0 in front of its three defect rows; columns u_0 alone (x_0 and dt are fixed)
            assert (rows == dims.lsq).sum() == 2
    d = problems.unicycle_desc(N=12); d.stage_eq = capi.STAGE_EQ_LINEAR
    rc, why = _refusal(lib, d)
    assert rc != 0 and "constraint_integration" in why
    d.constraint_integration = 1; d.grid, d.defect = capi.GRID_MS, capi.DEFECT_RK4_SHOOTING
    rc, why = _refusal(lib, d)
    assert rc != 0 and "integral-form constraint edges" in why


def _refusal(lib, d):
    dims = capi.Dims()
    rc = lib.corbo_hip_get_dims(C.byref(d), C.byref(dims))
    return rc, lib.corbo_hip_last_error().decode()


def test_the_gate_admits_every_grid_and_the_combinations(lib):
    for name in ("unicycle", "unicyclems", "unicyclet", "par3", "quad", "unicycle+envelope+unorm+rate", "unicyclems+rate"):
        assert _refusal(lib, E.make_desc(name, 12))[0] == 0, name
    d = E.make_desc("unicycle", 12)   # no constraint_integration needed; next to an integral-form inequality; non-diagonal weights for nx <= 4
    assert d.constraint_integration == 0
    d.stage_ineq, d.stage_ineq_integral, d.constraint_integration = capi.INEQ_BALL, 1, 1
    for i, v in enumerate((1.0, 0.5, 0.2, 0.3)):
        d.ineq_params[i] = v
    assert _refusal(lib, d)[0] == 0
    d = E.make_desc("unicycle", 12)
    d.weights_dense = 1
    for i in range(3):
        d.q_sqrt[i * 3 + i] = 1.0
    d.q_sqrt[1] = 0.1
    assert _refusal(lib, d)[0] == 0


def test_the_gate_refuses_with_a_named_reason(lib):
    U = capi.STAGE_FN_USER
    ok = E.make_desc("unicycle", 12)
    assert _refusal(lib, ok)[0] == 0
    # an unregistered id
    for bad in (U + 5, U + 7, U + 9, U + 15):
        d = E.make_desc("unicycle", 12); d.stage_eq = bad
        rc, why = _refusal(lib, d)
        assert rc != 0 and "stage_eq" in why and "unknown stage equality" in why, bad
    d = E.make_desc("unicycle", 12); d.stage_eq = 2
    rc, why = _refusal(lib, d)
    assert rc != 0 and "unknown stage equality" in why
    # an id of another kind
    for bad in (U + 0, U + 1, U + 2, U + 3):
        d = E.make_desc("unicycle", 12); d.stage_eq = bad
        rc, why = _refusal(lib, d)
        assert rc != 0 and "stage_eq" in why and "another kind" in why, bad
    # a state_control_eq id in the inequality fields
    for field in ("stage_ineq", "stage_ineq_control", "stage_ineq_state_control"):
        d = problems.unicycle_desc(N=12); setattr(d, field, U + 4)
        rc, why = _refusal(lib, d)
        assert rc != 0 and "stage_eq" in why and "state_control_eq" in why, field
    # dimensions below the minima: nu (the unicycle's two controls, input_circle needs three), nx (the Van der Pol oscillator)
    rc, why = _refusal(lib, problems.with_state_control_eq(problems.unicycle_desc(N=12), E.INPUT_CIRCLE, E.CIRCLE_PAR3))
    assert rc != 0 and "stage_eq" in why and "nu_min" in why
    rc, why = _refusal(lib, problems.with_state_control_eq(problems.vdp_desc(N=12), E.HEADING_TIE, E.TIE))
    assert rc != 0 and "stage_eq" in why and "nx_min" in why
    # the Hessian-path cost forms
    d = E.make_desc("unicycle", 12); d.cost_nonlsq = 1
    rc, why = _refusal(lib, d)
    assert rc != 0 and "stage_eq" in why and "Levenberg-Marquardt" in why
    d = E.make_desc("unicycle", 12); d.cost_nonlsq, d.cost_integral = 1, 1
    rc, why = _refusal(lib, d)
    assert rc != 0 and "stage_eq" in why and "Levenberg-Marquardt" in why
    # shooting integrators beyond Runge-Kutta 4
    for integ in (5, 6, 7):
        d = E.make_desc("unicyclems", 12); d.shooting_integrator = integ
        rc, why = _refusal(lib, d)
        assert rc != 0 and "stage_eq" in why and "Runge-Kutta 4" in why
    # N outside 3 .. 1024
    for N in (2, 1025):
        rc, why = _refusal(lib, E.make_desc("unicycle", N))
        assert rc != 0 and "stage_eq" in why and "3 <= N" in why
    assert _refusal(lib, E.make_desc("unicycle", 3))[0] == 0 and _refusal(lib, E.make_desc("unicycle", 1024))[0] == 0
    # the Hessian-path structure functions: unsupported, with the field's name
    nnz = (C.c_int32 * 3)()
    assert lib.corbo_hip_hessian_nnz(C.byref(ok), 1, nnz) == -3 and "stage_eq" in lib.corbo_hip_last_error().decode()
    # non-diagonal weights around a big-block model
    q = E.make_desc("quad", 8)
    w = solver.weight_factors(q, {"Q": np.eye(12) + 0.1})
    h = C.c_void_p()
    assert lib.corbo_hip_create_weighted(C.byref(q), C.byref(w), 1, 0, 0, C.byref(h)) == -1 and "extra edges" in lib.corbo_hip_last_error().decode()


@pytest.mark.parametrize("slot, nx, nu", [(4, 3, 2), (4, 3, 3), (6, 3, 3), (4, 12, 4), (6, 12, 4), (4, 6, 2)])
def test_host_evaluator_is_the_formula_bit_for_bit(lib, slot, nx, nu):
    rng = np.random.default_rng(100 * slot + 10 * nx + nu)
    n = 64
    x, u = rng.standard_normal((n, nx)), rng.standard_normal((n, nu))
    prm = rng.uniform(0.1, 1.0, 8)
    out = capi.eval_stage_function_xu(capi.STAGE_FN_USER + slot, x, u, prm)
    want = E.NP_FUNCTIONS[slot](x, u, prm)
    assert out.shape == want.shape == (n, capi.stage_function_rows(capi.STAGE_FN_USER + slot))
    assert np.array_equal(out.view(np.int64), want.view(np.int64))


def test_host_evaluator_refuses_what_it_cannot_evaluate(lib):
    """kinds 0 / 1, unregistered ids, dimensions below the minima (input_circle at (3, 2) and (6, 2): two controls; heading_tie at nx = 2 and nu = 1)"""
    U = capi.STAGE_FN_USER
    x, u, prm = np.zeros((2, 3)), np.zeros((2, 3)), np.zeros(8)
    for fn_id, xx, uu in ((U + 0, x, u), (U + 1, x, u), (U + 5, x, u), (U + 9, x, u), (U + 6, x, u[:, :2]), (U + 6, np.zeros((2, 6)), u[:, :2]),
                          (U + 4, x[:, :2], u), (U + 4, x, u[:, :1])):
        with pytest.raises(ValueError):
            capi.eval_stage_function_xu(fn_id, xx, uu, prm)
    # ... and the single-vertex evaluator refuses a state-control equality instead of returning zeros
    dp = C.POINTER(C.c_double)
    out = np.zeros(2)
    assert lib.corbo_hip_eval_stage_function(U + 4, 3, 2, x.ctypes.data_as(dp), prm.ctypes.data_as(dp), out.ctypes.data_as(dp)) != 0
