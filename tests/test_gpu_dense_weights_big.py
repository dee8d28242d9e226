"""Non-diagonal Q / R / Qf through corbo_hip_create_weighted (-m gpu): the big-block family's dense cost blocks (big_stage_kernel WD, the DENSE
residual sweep) and the side structure's plumbing for the small-block families.

Tolerances: the ledger's defaults (5e-6 on iterates, 2e-6 relative on chi2); residual 1e-12 x max weight and Jacobian 1e-6 relative as in
tests/test_gpu_parity.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import LEDGER, desc_for, load_golden
from control_box_rst_amd import capi, problems
from control_box_rst_amd.solver import BatchedLevenbergMarquardt, get_structure

pytestmark = pytest.mark.gpu

X_TOL = LEDGER["default_x_tol"]
CHI2_RTOL = LEDGER["default_chi2_rtol"]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import __graft_entry__ as g
    g.build()


def _factors_of_desc(d):
    """The descriptor path's factors (weights_dense, q_sqrt / r_sqrt / qf_sqrt with stride nx / nu) as a side structure."""
    w = capi.WeightFactors()
    w.mask = d.weights_dense
    for i in range(d.nx * d.nx):
        w.q_sqrt[i], w.qf_sqrt[i] = d.q_sqrt[i], d.qf_sqrt[i]
    for i in range(d.nu * d.nu):
        w.r_sqrt[i] = d.r_sqrt[i]
    return w


def _copy(d):
    c = capi.ProblemDesc()
    C.memmove(C.byref(c), C.byref(d), C.sizeof(d))
    return c


def _solve(d, x, xref, k, weights=None, weights_pen=(2.0, 2.0, 2.0), spec=None, refv=None, xref_traj=None):
    s = BatchedLevenbergMarquardt(d, x.shape[0], weights=weights)
    if spec is not None:
        s.set_option("reject_speculation", spec)
    s.setIterations(k)
    s.setPenaltyWeights(*weights_pen)
    s.set_instance_data(x, xref=xref)
    if refv is not None:   # one reference per vertex component (the fixtures' ref_vertex)
        refv = np.ascontiguousarray(np.tile(refv, (x.shape[0], 1)))
        assert s.lib.corbo_hip_set_references(s._h, refv.ctypes.data_as(C.POINTER(C.c_double))) == 0
    if xref_traj is not None:
        s.set_references(xref_traj)
    s.solve(new_run=True)
    X, chi2, status = s.get_solution()
    return X.copy(), chi2.copy(), s


@pytest.mark.parametrize("name", ["unicycle_n12_fullq", "unicycle_n12_fullq_ms", "unicycle_n12_fullq_tvref", "cartpole_fullq", "par3_fullq", "lin33_fullq"])
def test_side_structure_is_the_descriptor_path_bitwise(name):
    g = load_golden(name)
    d = desc_for(g)
    assert d.weights_dense
    d0 = _copy(d)
    w = _factors_of_desc(d)
    d0.weights_dense = 0
    for i in range(16):
        d0.q_sqrt[i] = d0.r_sqrt[i] = d0.qf_sqrt[i] = 0.0
    k = g["after_iter"][-1]["k"]
    nv = BatchedLevenbergMarquardt(d, 1).dims.nv
    x = np.array(g["vertex_init"])[None, :nv] if g.get("start") else None
    xref = np.array(g["xf"])[None, :]
    if x is None:
        x = BatchedLevenbergMarquardt(d, 1).init_trajectory(g["x0"], g["xf"])
    refv = np.array(g["ref_vertex"])[:nv] if "ref_vertex" in g else None
    Xa, ca, _ = _solve(d, x, xref, k, weights_pen=g["weights"], refv=refv)
    Xb, cb, _ = _solve(d0, x, xref, k, weights=w, weights_pen=g["weights"], refv=refv)
    assert np.array_equal(Xa, Xb) and np.array_equal(ca, cb)


def _diag_factors(d):
    return {"Q_sqrt": np.diag(np.sqrt([d.q_diag[i] for i in range(d.nx)])), "R_sqrt": np.diag(np.sqrt([d.r_diag[i] for i in range(d.nu)])),
            "Qf_sqrt": np.diag(np.sqrt([d.qf_diag[i] for i in range(d.nx)]))}


def _pquad_fd(N):
    d = problems.planar_quadrotor_desc(N=N)
    d.grid, d.defect = capi.GRID_FD, capi.DEFECT_CRANK_NICOLSON
    return d


def _pquad_instances(B):
    x0, xf = np.zeros((B, 6)), np.zeros((B, 6))
    for b in range(B):
        rng = np.random.default_rng(100 + b)
        x0[b, :2] = rng.uniform(-0.2, 0.2, 2)
        xf[b, :2] = np.array([1.5, 1.0]) + rng.uniform(-0.2, 0.2, 2)
    return x0, xf


DIAG_CASES = ["quad_ms_rk4", "pquad_fd_cn", "quad_ms_tvref", "quad_ms_tilt", "quad_ms_teq", "quad_ms_pteq", "quad_ms_tball", "pquad_fd_midpoint_tvref"]


@pytest.mark.parametrize("case", DIAG_CASES)
def test_diagonal_factors_match_the_diagonal_handle_bitwise(case):
    """U = diag(sqrt(w)) passed as dense: every off-diagonal product is an exact zero, so the dense cost terms enter the sums where the single-entry rows do.
    Also around the time-varying references, the tilt cone (the USERINEQ instantiation) and the final-stage constraints."""
    if case.startswith("quad"):
        d, B = problems.quad_desc(N=30), 16
        x0, xf = problems.quad_instances(B)
    else:
        d, B = _pquad_fd(20), 4
        x0, xf = _pquad_instances(B)
        if "midpoint" in case:
            d.defect = capi.DEFECT_MIDPOINT
    if case.endswith("tilt"):   # user state function, slot 0 (csrc/stage_functions/tilt_cone.hpp), instead of the keep-out ball
        d.stage_ineq = capi.STAGE_FN_USER + 0
        for i in range(8):
            d.ineq_params[i] = 0.0
        d.ineq_params[0] = 0.3
    if case.endswith("teq") or case.endswith("pteq"):
        d.final_eq = 1
        d.final_eq_mask = 0b000000000111 if case.endswith("pteq") else 0
    if case.endswith("tball"):
        d.final_ineq = capi.FINAL_INEQ_TERMINAL_BALL
        for i in range(d.nx):
            d.final_ineq_params[i] = 1.0
        d.final_ineq_params[d.nx] = 0.05
    traj = None
    if case.endswith("tvref"):   # a reference trajectory: x0 -> xf along the horizon, one reference per grid point
        traj = x0[:, None, :] + (xf - x0)[:, None, :] * np.linspace(0.0, 1.0, d.N)[None, :, None]
    x = BatchedLevenbergMarquardt(d, B).init_trajectory(x0, xf)
    Xa, ca, _ = _solve(d, x, xf, 10, weights_pen=problems.QUAD_WEIGHTS, xref_traj=traj)
    Xb, cb, s = _solve(d, x, xf, 10, weights=_diag_factors(d), weights_pen=problems.QUAD_WEIGHTS, xref_traj=traj)
    assert s.factor_route() == capi.FACTOR_STAGE_CHAIN
    assert np.array_equal(Xa, Xb), np.abs(Xa - Xb).max()
    assert np.array_equal(ca, cb)


def _fullq_pattern(w):
    """The fullq pattern of oracle/ref_driver.cpp: off-diagonals 0.25 sqrt(w_i w_j)."""
    w = np.asarray(w, dtype=np.float64)
    W = 0.25 * np.sqrt(np.outer(w, w))
    np.fill_diagonal(W, w)
    return W


def _random_spd(n, seed):
    A = np.random.default_rng(seed).standard_normal((n, n))
    return A @ A.T / n + np.eye(n)


def _weights(d, kind):
    q = [d.q_diag[i] for i in range(d.nx)]
    r = [d.r_diag[i] for i in range(d.nu)]
    qf = [d.qf_diag[i] for i in range(d.nx)]
    if kind == "pattern":
        return {"Q": _fullq_pattern(q), "R": _fullq_pattern(r), "Qf": _fullq_pattern(qf)}
    return {"Q": _random_spd(d.nx, 11), "R": 0.1 * _random_spd(d.nu, 12), "Qf": 10 * _random_spd(d.nx, 13)}


def _row(U, r, dim, xd):
    """Row r of U xd in the oracle's order (dense_weight_times: pairwise for four columns, left to right otherwise)."""
    u = U[r]
    if dim == 4:
        return 0.0 + ((u[0] * xd[0] + u[1] * xd[1]) + (u[2] * xd[2] + u[3] * xd[3]))
    acc = 0.0
    for j in range(dim):
        acc += u[j] * xd[j]
    return acc


def _rows_vec(U, xd):
    """All rows of U xd at once in _row's order: numpy's cumsum adds left to right (four columns: the pairwise form)."""
    P = U * np.asarray(xd)[None, :]
    if U.shape[1] == 4:
        return 0.0 + ((P[:, 0] + P[:, 1]) + (P[:, 2] + P[:, 3]))
    return np.cumsum(P, axis=1)[:, -1]


@pytest.mark.parametrize("kind", ["pattern", "random"])
@pytest.mark.parametrize("case", ["quad_ms_rk4", "pquad_fd_cn"])
def test_residual_and_jacobian_vs_host(oracle_mod, case, kind):
    """corbo_hip_eval at the initial guess: non-cost rows and entries from the unchanged OCP oracle on the diagonal descriptor, cost rows U (x - ref)
    and the cost blocks' central differences (the reference's in-place order) on the host."""
    O = oracle_mod
    d = problems.quad_desc(N=12) if case == "quad_ms_rk4" else _pquad_fd(10)
    nx, nu, N, S = d.nx, d.nu, d.N, d.nx + d.nu
    x0, xf = problems.quad_instances(1) if nx == 12 else _pquad_instances(1)
    wts = _weights(d, kind)
    s = BatchedLevenbergMarquardt(d, 1, weights=wts)
    U = {0: np.array(s.weights.q_sqrt[: nx * nx]).reshape(nx, nx), 1: np.array(s.weights.r_sqrt[: nu * nu]).reshape(nu, nu),
         2: np.array(s.weights.qf_sqrt[: nx * nx]).reshape(nx, nx)}
    x = s.init_trajectory(x0, xf)
    x[0, S: (N - 1) * S] += 0.01 * np.sin(np.arange((N - 2) * S))   # (a non-trivial point: controls and states off the interpolation)
    s.set_instance_data(x, xref=xf)
    values, jac = s.eval(2.0, 2.0, 2.0)
    # the oracle on the diagonal descriptor with unit weights: cost rows = x - ref / u, everything else as the device computes it
    d1 = _copy(d)
    for i in range(nx):
        d1.q_diag[i] = d1.qf_diag[i] = 1.0
    for i in range(nu):
        d1.r_diag[i] = 1.0
    p = O.OracleProblem(d1)
    p.set_data(x[0], xref=xf[0])
    vo, jo = p.eval(2.0, 2.0, 2.0)
    lsq = s.dims.lsq
    assert lsq == (N - 1) * S + nx
    xv = x[0]
    blocks = []   # (first row, vertex offset, dim, class)
    for k in range(N - 1):
        blocks += [(k * S, k * S, nx, 0), (k * S + nx, k * S + nx, nu, 1)]
    blocks.append(((N - 1) * S, (N - 1) * S, nx, 2))
    exp = vo.copy()
    for r0, v0, dim, cls in blocks:
        ref = xf[0] if cls != 1 else np.zeros(nu)
        xd = [float(xv[v0 + j] - ref[j]) for j in range(dim)]
        assert np.array_equal(vo[r0: r0 + dim], np.array(xd))   # the row layout
        for r in range(dim):
            exp[r0 + r] = _row(U[cls], r, dim, xd)
    wmax = max(2.0, max(abs(U[c]).max() for c in U) ** 2)
    assert np.abs(values[0] - exp).max() <= 1e-12 * wmax
    # the cost rows bit for bit: the device sums them in the host helper's (the oracle's dense_weight_times) order
    assert np.array_equal(values[0][:lsq], exp[:lsq])
    # Jacobian: cost rows by central differences (x_c += delta -> v2, x_c += -2 delta -> v1, (v2 - v1) / (2 delta))
    rows, cols = get_structure(d)
    m, n = s.dims.m, s.dims.n
    voff = p.param_offsets()
    col_of = {int(v): c for c, v in enumerate(voff)}
    Jd = sp.coo_matrix((jac[0], (rows, cols)), shape=(m, n)).toarray()
    Je = sp.coo_matrix((jo, (rows, cols)), shape=(m, n)).toarray()
    delta, scalar = 1e-9, 1.0 / (2 * 1e-9)
    for r0, v0, dim, cls in blocks:
        ref = xf[0] if cls != 1 else np.zeros(nu)
        xd = [float(xv[v0 + j] - ref[j]) for j in range(dim)]
        for c in range(dim):
            if v0 + c not in col_of:
                continue   # (fixed x_0)
            a = float(xv[v0 + c]) + delta
            b = a + -2 * delta
            x2, x1 = list(xd), list(xd)
            x2[c], x1[c] = a - ref[c], b - ref[c]
            for r in range(dim):
                Je[r0 + r, col_of[v0 + c]] = scalar * (_row(U[cls], r, dim, x2) - _row(U[cls], r, dim, x1))
    scale = max(1.0, np.abs(Je).max())
    assert np.abs(Jd - Je).max() <= 1e-6 * scale
    # ... and the cost blocks' central differences bit for bit (same perturbation, same order of operations)
    assert np.array_equal(Jd[:lsq], Je[:lsq])


@pytest.mark.parametrize("case", ["quad_ms_rk4", "pquad_fd_cn"])
def test_dense_solve_chi2_is_its_residual(case):
    """The LM path on dense weights: chi2 falls, and the reported chi2 is the squared norm of the residual the sweep evaluates at the solution."""
    d = problems.quad_desc(N=20) if case == "quad_ms_rk4" else _pquad_fd(10)
    B = 4
    x0, xf = problems.quad_instances(B) if d.nx == 12 else _pquad_instances(B)
    s = BatchedLevenbergMarquardt(d, B, weights=_weights(d, "pattern"))
    x = s.init_trajectory(x0, xf)
    s.setPenaltyWeights(2.0, 2.0, 2.0)
    s.set_instance_data(x, xref=xf)
    v0, _ = s.eval(2.0, 2.0, 2.0, jacobian=False)
    s.setIterations(5)
    s.solve(new_run=True)
    X, chi2, status = s.get_solution()
    assert np.all(np.isfinite(X)) and np.all(chi2 < (v0 ** 2).sum(axis=1))
    s.set_instance_data(X, xref=xf)
    v1, _ = s.eval(2.0, 2.0, 2.0, jacobian=False)
    assert np.allclose((v1 ** 2).sum(axis=1), chi2, rtol=CHI2_RTOL, atol=0)


def test_speculation_bitwise():
    """Reject-streak speculation forced on (option 2: every rejecting instance may get candidates, whatever the batch) against off: the candidates run
    the WD stage kernel on the spare rows, the adopted states are the ones the instance would have reached itself."""
    d = problems.quad_desc(N=40)
    B = 256   # (46 rejected steps with these weights, candidates adopted nine times)
    x0, xf = problems.quad_instances(B)
    w = _weights(d, "random")
    x = BatchedLevenbergMarquardt(d, B).init_trajectory(x0, xf)
    Xa, ca, s = _solve(d, x, xf, 10, weights=w, weights_pen=problems.QUAD_WEIGHTS, spec=2)
    assert s.factor_route() == capi.FACTOR_STAGE_CHAIN
    st = s.get_stats()
    assert st["rejected_steps"] > 0 and st["speculative_takeovers"] > 0, st
    Xb, cb, _ = _solve(d, x, xf, 10, weights=w, weights_pen=problems.QUAD_WEIGHTS, spec=0)
    assert np.array_equal(Xa, Xb) and np.array_equal(ca, cb)


def test_large_batch_is_per_instance_bitwise():
    """A batch beyond what the chip holds at once (600 instances: two sub-batches on their own streams, speculation on by the automatic rule, the
    chain's workgroups in several rounds) against single-instance solves.  N = 40: the chain's formulation does not depend on the batch."""
    d = problems.quad_desc(N=40)
    B = 600
    x0, xf = problems.quad_instances(B)
    w = _weights(d, "pattern")
    x = BatchedLevenbergMarquardt(d, 1).init_trajectory(x0, xf)
    Xa, ca, s = _solve(d, x, xf, 10, weights=w, weights_pen=problems.QUAD_WEIGHTS)
    assert s.get_stats()["rejected_steps"] > 0
    for b in (0, 299, 599):
        Xs, cs, _ = _solve(d, x[b: b + 1], xf[b: b + 1], 10, weights=w, weights_pen=problems.QUAD_WEIGHTS)
        assert np.array_equal(Xs[0], Xa[b]) and cs[0] == ca[b], b


def test_unknown_weight_keys_are_refused():
    d = problems.quad_desc(N=10)
    with pytest.raises(ValueError):
        BatchedLevenbergMarquardt(d, 1, weights={"qf": np.eye(12)})


def test_sweep_timing_with_a_jacobian_is_refused():
    """The DENSE sweep of this family is residual-only: timing it with a Jacobian is refused, not reported as an empty launch."""
    d = problems.quad_desc(N=10)
    x0, xf = problems.quad_instances(1)
    s = BatchedLevenbergMarquardt(d, 1, weights=_weights(d, "pattern"))
    s.set_instance_data(s.init_trajectory(x0, xf), xref=xf)
    ms = C.c_float(0)
    assert s.lib.corbo_hip_time_sweep(s._h, 2.0, 2.0, 2.0, 1, 2, C.byref(ms)) == -3
    assert s.lib.corbo_hip_time_sweep(s._h, 2.0, 2.0, 2.0, 0, 2, C.byref(ms)) == 0


def test_hessian_path_operators_are_refused():
    d = problems.quad_desc(N=10)
    B = 2
    x0, xf = problems.quad_instances(B)
    s = BatchedLevenbergMarquardt(d, B, weights=_weights(d, "pattern"))
    s.set_instance_data(s.init_trajectory(x0, xf), xref=xf)
    grad = np.zeros((B, s.dims.n))
    obj = np.zeros(B)
    rc = s.lib.corbo_hip_eval_objective_gradient(s._h, grad.ctypes.data_as(C.POINTER(C.c_double)), obj.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == -3
    big = np.zeros(1 << 20)
    dp = big.ctypes.data_as(C.POINTER(C.c_double))
    assert s.lib.corbo_hip_eval_hessians(s._h, 1, 1.0, None, None, dp, dp, dp) == -3
    assert s.lib.corbo_hip_eval_linear_form(s._h, dp, dp, dp) == -3


def _box(d, nv):
    """The descriptor's boxes along the horizon, per vertex component (what set_instance_data fills in without lb / ub)."""
    nx, nu, N, S = d.nx, d.nu, d.N, d.nx + d.nu
    lb, ub = np.full(nv, -capi.INF), np.full(nv, capi.INF)
    for k in range(N):
        for i in range(nx):
            lb[k * S + i], ub[k * S + i] = d.x_lb[i], d.x_ub[i]
        if k < N - 1:
            for i in range(nu):
                lb[k * S + nx + i], ub[k * S + nx + i] = d.u_lb[i], d.u_ub[i]
    return lb, ub


@pytest.mark.parametrize("kind", ["pattern", "random"])
@pytest.mark.parametrize("case", ["quad_ms_rk4", "pquad_fd_cn"])
def test_lm_iterates_vs_generic_oracle(oracle_mod, case, kind):
    """LM iterates and chi2 after k = 1 .. 5 iterations against oracle.GenericProblem -- the same oracle_solve as the OCPs, on a callback that stacks the
    unchanged OCP oracle's rows (unit weights, diagonal descriptor) with its cost rows replaced by the dense ones U (x - ref) in the oracle's order, the
    bounds as lb / ub.  Its Jacobian is central differences of that callback: an independent assembly of the normal equations, dense Gram blocks included."""
    O = oracle_mod
    d = problems.quad_desc(N=10) if case == "quad_ms_rk4" else _pquad_fd(10)
    nx, nu, N, S = d.nx, d.nu, d.N, d.nx + d.nu
    x0, xf = problems.quad_instances(1) if nx == 12 else _pquad_instances(1)
    wts = _weights(d, kind)
    s = BatchedLevenbergMarquardt(d, 1, weights=wts)
    U = {0: np.array(s.weights.q_sqrt[: nx * nx]).reshape(nx, nx), 1: np.array(s.weights.r_sqrt[: nu * nu]).reshape(nu, nu),
         2: np.array(s.weights.qf_sqrt[: nx * nx]).reshape(nx, nx)}
    x = s.init_trajectory(x0, xf)
    nv, lsq, eq, ineq = s.dims.nv, s.dims.lsq, s.dims.eq, s.dims.ineq
    d1 = _copy(d)
    for i in range(nx):
        d1.q_diag[i] = d1.qf_diag[i] = 1.0
    for i in range(nu):
        d1.r_diag[i] = 1.0
    ocp = O.OracleProblem(d1)
    voff = ocp.param_offsets()
    blocks = [(k * S + o, dim, cls) for k in range(N - 1) for o, dim, cls in ((0, nx, 0), (nx, nu, 1))] + [((N - 1) * S, nx, 2)]
    base = x[0].copy()
    cache = {}

    def rows(p):
        key = p.tobytes()
        if key not in cache:
            v = base.copy()
            v[voff] = p
            ocp.set_data(v, xref=xf[0])
            vals, _ = ocp.eval(1.0, 1.0, 1.0, jacobian=False)   # cost rows x - ref / u (unit weights), raw constraint rows
            cost = vals[:lsq].copy()
            for r0, dim, cls in blocks:
                cost[r0: r0 + dim] = _rows_vec(U[cls], vals[r0: r0 + dim])
            cache.clear()
            cache[key] = (cost, vals[lsq: lsq + eq].copy(), vals[lsq + eq: lsq + eq + ineq].copy())
        return cache[key]

    lbv, ubv = _box(d, nv)
    opts = capi.default_lm_opts(1, *problems.QUAD_WEIGHTS)

    def generic(start, k):
        gp = O.GenericProblem(len(voff), lsq=lambda p: rows(p)[0], dim_lsq=lsq, eq=lambda p: rows(p)[1], dim_eq=eq,
                              ineq=(lambda p: rows(p)[2]) if ineq else None, dim_ineq=ineq, lb=lbv[voff], ub=ubv[voff])
        gp.set_data(start)
        opts.iterations = k
        _, c2, _ = gp.solve(opts, new_run=True)
        return gp.x(), c2

    p0 = base[voff]
    for k in range(1, 6):
        xo, chi2_o = generic(p0, k)
        # the oracle's own spread: the same solve from starts one ulp away (the ledger's rule for a tolerance beyond the default: <= 4 x this spread)
        spread_x, spread_c = 0.0, 0.0
        for direction in (np.inf, -np.inf):
            xu, cu = generic(np.nextafter(p0, direction), k)
            spread_x, spread_c = max(spread_x, np.abs(xu - xo).max()), max(spread_c, abs(cu - chi2_o) / abs(chi2_o))
        xtol, ctol = max(X_TOL, 4 * spread_x), max(CHI2_RTOL, 4 * spread_c)
        s.setIterations(k)
        s.setPenaltyWeights(*problems.QUAD_WEIGHTS)
        s.set_instance_data(x, xref=xf)
        s.solve(new_run=True)
        X, chi2, _ = s.get_solution()
        assert np.abs(X[0][voff] - xo).max() <= xtol, (k, np.abs(X[0][voff] - xo).max(), spread_x)
        assert abs(chi2[0] - chi2_o) <= ctol * abs(chi2_o), (k, chi2[0], chi2_o, spread_c)
