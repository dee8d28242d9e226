"""CPU tests of the stage inequalities' non-integral state-control term (corbo_hip_problem_desc::stage_ineq_state_control, csrc/stage_functions/ kind
state_control_ineq): registry, structure in the reference's creation order (nlp_functions.cpp:109-115 -- read there, asserted structurally: no fixture of the
genuine reference has this term), the gate's refusals and the host evaluator against the headers' formulas written out in numpy.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import stage_function_xu_cases as X
from control_box_rst_amd import capi, problems, solver


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return capi.load()


def test_kinds_and_rows_of_the_shipped_functions(lib):
    U = capi.STAGE_FN_USER
    assert [lib.corbo_hip_stage_function_kind(U + s) for s in range(4)] == [0, 1, 2, 2]
    assert [lib.corbo_hip_stage_function_rows(U + s) for s in range(4)] == [1, 1, 1, 4]
    assert lib.corbo_hip_stage_function_kind(U + 7) == -1 and lib.corbo_hip_stage_function_rows(U + 7) == -1
    import __graft_entry__ as g
    assert g.user_stage_function_shapes() == {2: (1, 1), 3: (4, 2)}
    assert ("drive_power", 2, 2, 3) in [f[:4] for f in g.user_stage_functions()] and ("input_envelope", 3, 2, 3) in [f[:4] for f in g.user_stage_functions()]


def _structure(d):
    dims = solver.get_dims(d)
    rows, cols = solver.get_structure(d)
    return dims, rows, cols


@pytest.mark.parametrize("extras", ["", "+unorm+rate"])
def test_structure_follows_the_creation_order(lib, oracle_mod, extras):
    """Unicycle, FD / Crank-Nicolson, N = 4, slot 3 (four rows): alone, and with the control term and the control-deviation term on -- the rows of interval k
    sit behind its control term's and in front of its control-deviation rows; columns x_k then u_k; interval 0 (x_0 fixed) has no x columns."""
    N = 4
    d = X.make_desc("unicycle" + extras, N)
    d0 = X.without_term(d)
    dims, rows, cols = _structure(d)
    dims0, rows0, cols0 = _structure(d0)
    nx, nu, S = d.nx, d.nu, d.nx + d.nu
    front, r, back = X.ineq_layout(d)
    assert (front, r, back) == ((1, 4, 2) if extras else (0, 4, 0))
    assert dims.ineq == dims0.ineq + 4 * (N - 1) and (dims.ineq == 4 * (N - 1) or extras)
    assert dims.n == dims0.n and dims.lsq == dims0.lsq and dims.eq == dims0.eq and dims.bounds == dims0.bounds and dims.m == dims0.m + 4 * (N - 1)
    assert dims.nnz == dims0.nnz + 4 * (nu + (N - 2) * S)
    voff = oracle_mod.OracleProblem(d0).param_offsets().astype(np.int64)
    col_of = {int(v): c for c, v in enumerate(voff)}
    trow = X.term_rows(d, dims)
    assert trow[0][0] == dims.lsq + dims.eq + front and trow[-1][-1] < dims.lsq + dims.eq + dims.ineq
    for k in range(N - 1):
        want_cols = [col_of[k * S + c] for c in range(S) if k * S + c in col_of]   # x_k then u_k, unfixed components only
        assert len(want_cols) == (nu if k == 0 else S)
        mask = np.isin(rows, trow[k])
        idx = np.nonzero(mask)[0]
        assert np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx))), "one contiguous block of values per edge"
        # value order of an edge's block: column by column, the edge's rows inside a column
        assert rows[idx].tolist() == [int(t) for _ in want_cols for t in trow[k]]
        assert cols[idx].tolist() == [c for c in want_cols for _ in trow[k]]
    # every other entry is the descriptor's without the term, rows shifted past the inserted ones
    keep = ~np.isin(rows, trow.ravel())
    shift = np.searchsorted(np.sort(trow.ravel()), rows[keep])
    assert np.array_equal(rows[keep] - shift, rows0) and np.array_equal(cols[keep], cols0)


def test_field_zero_is_the_descriptor_of_before(lib):
    """A descriptor whose field is 0 -- set and cleared again, parameters still attached -- has the dims and the structure of a copy taken before."""
    for mk in (lambda: problems.unicycle_desc(N=12), lambda: problems.quad_desc(N=8), lambda: X.without_term(X.make_desc("unicycle+unorm+rate", 12))):
        d = mk()
        before = X.copy_desc(d)
        dims_b, rows_b, cols_b = _structure(before)
        problems.with_state_control_ineq(d, X.DRIVE_POWER if d.nu == 1 else X.INPUT_ENVELOPE, (0.3, 0.1, 0.2, 0.1))
        assert solver.get_dims(d).ineq > dims_b.ineq
        d.stage_ineq_state_control = 0
        assert bytes(d) == bytes(before)
        dims_a, rows_a, cols_a = _structure(d)
        assert dims_a.as_dict() == dims_b.as_dict() and np.array_equal(rows_a, rows_b) and np.array_equal(cols_a, cols_b)
    assert C.sizeof(capi.ProblemDesc) == lib.corbo_hip_sizeof(0)
    assert capi.ProblemDesc.stage_ineq_state_control.offset == capi.ProblemDesc.stage_ineq_control.offset + 4


def _refusal(lib, d):
    dims = capi.Dims()
    rc = lib.corbo_hip_get_dims(C.byref(d), C.byref(dims))
    return rc, lib.corbo_hip_last_error().decode()


def test_the_gate_refuses_with_a_named_reason(lib):
    U = capi.STAGE_FN_USER
    ok = X.make_desc("unicycle", 12)
    assert _refusal(lib, ok)[0] == 0
    # nu below the function's nu_min: the cart-pole (nu = 1) with the input envelope (two controls)
    d = problems.with_state_control_ineq(problems.benchmark_desc("cartpole", N=12), X.INPUT_ENVELOPE, X.ENVELOPE)
    rc, why = _refusal(lib, d)
    assert rc != 0 and "stage_ineq_state_control" in why and "nu_min" in why
    # nx below nx_min: the Van der Pol oscillator (nx = 2)
    rc, why = _refusal(lib, problems.with_state_control_ineq(problems.vdp_desc(N=12), X.DRIVE_POWER, (0.1,)))
    assert rc != 0 and "stage_ineq_state_control" in why
    # the Hessian-path cost forms
    d = X.make_desc("unicycle", 12); d.cost_nonlsq = 1
    rc, why = _refusal(lib, d)
    assert rc != 0 and "stage_ineq_state_control" in why and "Levenberg-Marquardt" in why
    # shooting integrators beyond Runge-Kutta 4
    d = X.make_desc("unicyclems", 12); d.shooting_integrator = 6
    rc, why = _refusal(lib, d)
    assert rc != 0 and "Runge-Kutta 4" in why
    # two grid points
    rc, why = _refusal(lib, X.make_desc("unicycle", 2))
    assert rc != 0 and "3 <= N" in why
    rc, why = _refusal(lib, X.make_desc("unicycle", 1025))
    assert rc != 0 and "3 <= N" in why
    # an unregistered id, ids of the other kinds, a state-control id in the other fields
    for bad in (U + 9, U + 0, U + 1, 1, 999):
        d = X.make_desc("unicycle", 12); d.stage_ineq_state_control = bad
        rc, why = _refusal(lib, d)
        assert rc != 0 and "stage_ineq_state_control" in why, bad
    d = problems.unicycle_desc(N=12); d.stage_ineq_control = U + 3
    assert _refusal(lib, d)[0] != 0
    d = problems.unicycle_desc(N=12); d.stage_ineq = U + 3
    assert _refusal(lib, d)[0] != 0
    # the Hessian-path structure functions: unsupported, with the field's name
    nnz = (C.c_int32 * 3)()
    assert lib.corbo_hip_hessian_nnz(C.byref(ok), 1, nnz) == -3 and "stage_ineq_state_control" in lib.corbo_hip_last_error().decode()
    # non-diagonal weights around a big-block model
    q = X.make_desc("quad", 8)
    w = solver.weight_factors(q, {"Q": np.eye(12) + 0.1})
    h = C.c_void_p()
    assert lib.corbo_hip_create_weighted(C.byref(q), C.byref(w), 1, 0, 0, C.byref(h)) == -1 and "state-control" in lib.corbo_hip_last_error().decode()


@pytest.mark.parametrize("slot, nx, nu", [(2, 4, 1), (2, 3, 2), (3, 3, 2), (3, 12, 4), (3, 6, 2)])
def test_host_evaluator_is_the_formula_bit_for_bit(lib, slot, nx, nu):
    rng = np.random.default_rng(100 * slot + nx)
    n = 64
    x, u = rng.standard_normal((n, nx)), rng.standard_normal((n, nu))
    prm = rng.uniform(0.1, 1.0, 8)
    out = capi.eval_stage_function_xu(capi.STAGE_FN_USER + slot, x, u, prm)
    want = X.NP_FUNCTIONS[slot](x, u, prm)
    assert out.shape == want.shape == (n, capi.stage_function_rows(capi.STAGE_FN_USER + slot))
    assert np.array_equal(out.view(np.int64), want.view(np.int64))


def test_host_evaluator_refuses_what_it_cannot_evaluate(lib):
    x, u, prm = np.zeros((2, 3)), np.zeros((2, 2)), np.zeros(8)
    for fn_id, xx, uu in ((capi.STAGE_FN_USER + 1, x, u), (capi.STAGE_FN_USER + 9, x, u), (capi.STAGE_FN_USER + 3, x, u[:, :1]), (capi.STAGE_FN_USER + 2, x[:, :2], u)):
        with pytest.raises(ValueError):
            capi.eval_stage_function_xu(fn_id, xx, uu, prm)
    # ... and the single-vertex evaluator refuses a state-control function instead of returning zeros
    dp = C.POINTER(C.c_double)
    out = np.zeros(2)
    assert lib.corbo_hip_eval_stage_function(capi.STAGE_FN_USER + 2, 3, 2, x.ctypes.data_as(dp), prm.ctypes.data_as(dp), out.ctypes.data_as(dp)) != 0


def test_parameter_setter_without_a_handle(lib):
    prm = np.zeros(8)
    assert lib.corbo_hip_set_state_control_params(None, prm.ctypes.data_as(C.POINTER(C.c_double))) == -1
