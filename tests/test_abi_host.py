"""CPU-side tests of the product: the C-ABI library loads, exports every symbol include/corbo_hip.h declares, and its
host-only entry points (dims, structure, trajectory initialisation) agree with the oracle / golden vectors.
No compute call touches a GPU here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, desc_for, load_golden
from control_box_rst_amd import capi, problems, solver


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return capi.load()


def test_exports_every_declared_symbol(lib):
    header = open(os.path.join(ROOT, "include", "corbo_hip.h")).read()
    declared = set(re.findall(r"\b(corbo_hip_[a-z_]+)\s*\(", header))
    assert declared == set(capi.EXPORTED_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name


def test_struct_sizes_match_header(lib):
    # sizes implied by include/corbo_hip.h (packing check of the ctypes mirrors)
    assert C.sizeof(capi.ProblemDesc) == 10 * 4 + 3 * 8 + (2 * 16 + 2 * 8 + 16 + 8 + 16 + 8 + 8) * 8 + 2 * 4 + 17 * 8 + 28 * 8 + 4 * 4 + 2 * 4 + 3 * 16 * 8 + 4 * 4 + (25 + 8) * 8 + 2 * 4 + 8 * 8   # (+ shooting_integrator, final_eq_mask, q_sqrt, r_sqrt, qf_sqrt; + the integral-constraint / control-deviation fields; + stage_ineq_control and its parameters)
    assert C.sizeof(capi.Dims) == 8 * 4
    assert C.sizeof(capi.LmOpts) == 8 + 9 * 8
    o = capi.LmOpts()
    lib.corbo_hip_default_lm_opts(C.byref(o))
    assert (o.iterations, o.weight_eq, o.adapt_factor_eq, o.adapt_max_bounds) == (10, 2.0, 1.0, 500.0)


@pytest.mark.parametrize("name", ["unicycle", "vdp", "dint", "vdp_forward", "unicycle_n12", "quad_n10", "unicycle_n12_tball", "vdp_tball", "vdp_ms_rk4", "unicycle_n12_ms_rk4", "unicycle_n24_ball", "unicycle_n12_teq", "vdp_teq", "unicycle_n12_patterns", "vdp_patterns", "int3", "int3_ms_rk4", "int3_time_optimal",
                                  "sf_quad_tilt", "xe_sf_unicycle_unorm", "xe_sf_unicycle_ball_unorm_rate", "xe_sf_int3_unorm_vargrid", "xe_sf_quad_tilt_unorm"])   # (user stage functions: the control term's edge between the state term's and the control-deviation edge)
def test_dims_and_structure_match_reference(lib, oracle_mod, name):
    g = load_golden(name)
    d = desc_for(g)
    dims = solver.get_dims(d)
    for k in ("n", "lsq", "eq", "ineq", "bounds", "m", "nnz"):
        assert getattr(dims, k) == g[k], k
    rows, cols = solver.get_structure(d)
    assert sorted(zip(rows.tolist(), cols.tolist())) == sorted(zip(g["jac_rows"], g["jac_cols"]))
    # same value order as the oracle (both follow the reference's sweep order)
    orows, ocols = oracle_mod.OracleProblem(d).structure()
    assert np.array_equal(rows, orows) and np.array_equal(cols, ocols)


def test_init_trajectory_matches_oracle_bitwise(lib, oracle_mod):
    d = problems.unicycle_desc()
    x0, xf = problems.unicycle_instances(5)
    X = solver.init_trajectory(d, x0, xf)
    p = oracle_mod.OracleProblem(d)
    for b in range(5):
        assert np.array_equal(X[b], p.init_trajectory(x0[b], xf[b]))
    d2 = problems.dint_desc()
    X2 = solver.init_trajectory(d2, [[0.0, 0.0]], [[1.0, 0.0]])
    assert np.array_equal(X2[0], oracle_mod.OracleProblem(d2).init_trajectory([0.0, 0.0], [1.0, 0.0]))
    assert X2[0][-1] == d2.dt_ref


def test_invalid_descriptors_are_rejected(lib):
    d = problems.unicycle_desc()
    d.nx = 5
    with pytest.raises(solver.CorboHipError):
        solver.get_dims(d)
    d = problems.unicycle_desc()
    d.grid = capi.GRID_MS  # MS grid needs the RK4 defect
    with pytest.raises(solver.CorboHipError):
        solver.get_dims(d)
    assert b"" != lib.corbo_hip_last_error()
    # the cost-form fields: an integral cost is a plain objective edge on the FiniteDifferencesGrid; only_last_n belongs to MinTimeQuadratic;
    # a minimum-time term needs a free dt
    for edit in (lambda d: setattr(d, "cost_integral", 1), lambda d: setattr(d, "cost_integral", 3), lambda d: setattr(d, "cost_nonlsq", 2),
                 lambda d: setattr(d, "quad_first_interval", 5), lambda d: setattr(d, "stage_cost", capi.COST_MIN_TIME_QUADRATIC_LSQ)):
        d = problems.unicycle_desc()
        edit(d)
        with pytest.raises(solver.CorboHipError):
            solver.get_dims(d)
    d = problems.unicycle_desc()
    d.cost_nonlsq, d.cost_integral = 1, 2
    assert solver.get_dims(d).lsq == 0   # plain objective edges are no rows of the LM residual


def _long_plan(lib, d):
    out = (C.c_int32 * 4)()
    rc = lib.corbo_hip_long_factor_plan(C.byref(d), C.byref(out))
    return rc, tuple(out)


def test_long_factor_plan_is_the_launchers_arithmetic(lib):
    """corbo_hip_long_factor_plan (host only) against the layout written out here: c (N | 1) + 130 doubles with c = nx (nx + 1) / 2 + 2 nx^2 + nx, nx (N | 1) more
    with a free dt; one workgroup fits when those bytes + the LM state (128) + 64 are within 160 KB, two when twice that is; eight waves up to 512 grid points;
    non-diagonal weights and the HBM workspace always run sixteen waves."""
    def expect(nx, N, free, dense):
        c = nx * (nx + 1) // 2 + 2 * nx * nx + nx + (nx if free else 0)
        lds = 8 * (c * (N | 1) + 130)
        fit = (lds + 128 + 64 <= 160 * 1024) + (2 * (lds + 128 + 64) <= 160 * 1024)
        return (512 if (N <= 512 and fit and not dense) else 1024, fit, lds if fit else 0, int(dense))

    makers = {(2, 1, False): lambda N: problems.vdp_desc(N=N), (2, 1, True): lambda N: problems.dint_desc(N=N), (2, 2, False): lambda N: problems.parallel_integrator_desc(2, N=N),
              (3, 1, False): lambda N: problems.int3_desc(N=N), (3, 1, True): lambda N: problems.int3_desc(N=N, time_optimal=True),
              (3, 2, False): lambda N: problems.unicycle_desc(N=N), (3, 3, False): lambda N: problems.parallel_integrator_desc(3, N=N),
              (4, 1, False): lambda N: problems.benchmark_desc("cartpole", N=N)}
    for (nx, nu, free), mk in makers.items():
        for N in (257, 335, 336, 373, 374, 405, 406, 441, 442, 512, 513, 671, 672, 677, 678, 751, 752, 775, 776, 1000, 1023, 1024):
            d = mk(N)
            assert (d.nx, d.nu) == (nx, nu)
            assert _long_plan(lib, d) == (0, expect(nx, N, free, False)), (nx, nu, free, N)
            if not free:
                d.weights_dense = 1
                for i in range(nx):
                    d.q_sqrt[i * nx + i] = 1.0
                assert _long_plan(lib, d) == (0, expect(nx, N, free, True)), (nx, nu, free, N, "dense")
    # the switches themselves: the last horizon with two workgroups per CU | the last with the state blocks in LDS
    assert [_long_plan(lib, problems.unicycle_desc(N=N))[1][:2] for N in (373, 374, 512, 513, 751, 752)] == [(512, 2), (512, 1), (512, 1), (1024, 1), (1024, 1), (1024, 0)]
    assert [_long_plan(lib, problems.int3_desc(N=N, time_optimal=True))[1][:2] for N in (335, 336, 677, 678)] == [(512, 2), (512, 1), (1024, 1), (1024, 0)]
    assert [_long_plan(lib, problems.benchmark_desc("cartpole", N=N))[1][:2] for N in (441, 442, 512)] == [(512, 1), (1024, 0), (1024, 0)]
    assert [_long_plan(lib, problems.vdp_desc(N=N))[1][:2] for N in (257, 512, 513, 775, 776, 1024)] == [(512, 2), (512, 2), (1024, 2), (1024, 2), (1024, 1), (1024, 1)]
    # no such kernel: short and too long horizons, the big-block family, extra edges (band / block-tridiagonal route), a null pointer
    for d in (problems.unicycle_desc(N=256), problems.unicycle_desc(N=1025), problems.quad_desc(N=300), problems.planar_quadrotor_desc(N=300)):
        assert _long_plan(lib, d)[0] != 0
    assert b"" != lib.corbo_hip_last_error()
    d = problems.unicycle_desc(N=300)
    d.ctrl_dev = capi.CTRL_DEV_RATE
    d.ctrl_dev_params[0] = d.ctrl_dev_params[1] = 0.3
    assert _long_plan(lib, d)[0] != 0
    assert lib.corbo_hip_long_factor_plan(None, None) != 0


def test_the_oracle_refuses_what_the_reference_solver_refuses(oracle_mod):
    """LevenbergMarquardtSparse::solve returns Error for a problem with plain objective edges (levenberg_marquardt_sparse.cpp:48-55)."""
    d = problems.vdp_desc(N=8)
    d.cost_nonlsq = 1
    p = oracle_mod.OracleProblem(d)
    p.set_data(p.init_trajectory([1.0, 0.0], [0.0, 0.0]), xref=np.zeros(2))
    assert p.dims.lsq == 0
    assert oracle_mod.load().oracle_solve(p.h, C.byref(capi.default_lm_opts(2, 2.0, 2.0, 2.0)), 1, None, None) == capi.SOLVER_ERROR


def test_create_without_gpu_fails_loudly(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(solver.CorboHipError):
        solver.BatchedLevenbergMarquardt(problems.unicycle_desc(N=12), 2)


def test_product_does_not_use_the_oracle():
    """The product path must never import / link / call anything under oracle/."""
    pkg = os.path.join(ROOT, "control_box_rst_amd")
    pat = re.compile(r"(import\s+oracle|from\s+oracle|liboracle|oracle_[a-z]+\s*\(|corbo_oracle\.h)")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert not pat.search(txt), (dirpath, f)


def test_create_refuses_descriptors_without_device_kernels_before_touching_the_device():
    """a descriptor that validates but has no sweep / pass kernel (serial integrator of order 4) is refused by corbo_hip_create itself (CORBO_HIP_ERR_UNSUPPORTED), not by the first solve.  The gate runs before any HIP call,
    so it is testable without a GPU."""
    import ctypes as C
    lib = capi.load()
    d = problems.int3_desc()
    d.nx = 4
    for i in range(4):
        d.q_diag[i], d.qf_diag[i] = 1.0, 1.0
    h = C.c_void_p()
    assert lib.corbo_hip_create(C.byref(d), 1, 0, C.byref(h)) == -3 and not h.value
    # (round 4: the big-block family on the grids with a FREE dt passes the gate -- band factorisation -- and fails only for want of a device here)
    import torch
    q = problems.quad_desc(N=10, time_optimal=True)
    rc = lib.corbo_hip_create(C.byref(q), 1, 0, C.byref(h))
    assert rc != -3
    if not torch.cuda.is_available():
        assert rc == -2 and not h.value
    elif rc == 0:
        lib.corbo_hip_destroy(h)


@pytest.mark.parametrize("name", ["hess_vdp", "hess_vdp_forward", "hess_vdp_teq", "hess_dint", "hess_int3_time_optimal", "hess_unicycle_n16",
                                  "hess_unicycle_xf_fixed", "hess_unicycle_n24_ball", "hess_pendulum_ms_rk4", "hess_cartpole", "hess_quad_n4", "hess_int3_ms_time_optimal",
                                  "hess_dint_mtq", "hess_int3_ms_mtq", "hess_dint_mtq_last5",
                                  "hess_vdp_nonlsq", "hess_unicycle_nonlsq", "hess_unicycle_nonlsq_tball", "hess_dint_nonlsq", "hess_dint_mtq_nonlsq", "hess_int3_ms_nonlsq",
                                  "hess_vdp_integral_trap", "hess_unicycle_integral_trap", "hess_unicycle_integral_left"])
def test_hessian_and_linear_form_structure_vs_reference(name):
    """corbo_hip_hessian_{nnz,structure} / corbo_hip_linear_form_structure are host-only functions of the descriptor: the three triplet
    lists of computeSparseHessiansStructure (full and lower part) and the linear form's, entry by entry as the genuine reference
    lists them (tests/golden/hess_*.json)."""
    import ctypes as C
    from conftest import desc_for, load_golden
    g = load_golden(name)
    d = desc_for(g)
    lib = capi.load()
    ipp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    for lower, tag in ((0, "full"), (1, "lower")):
        nnz = np.zeros(3, np.int32)
        assert lib.corbo_hip_hessian_nnz(C.byref(d), lower, ipp(nnz)) == 0
        rows = [np.zeros(max(1, n), np.int32) for n in nnz]
        cols = [np.zeros(max(1, n), np.int32) for n in nnz]
        assert lib.corbo_hip_hessian_structure(C.byref(d), lower, ipp(rows[0]), ipp(cols[0]), ipp(rows[1]), ipp(cols[1]), ipp(rows[2]), ipp(cols[2])) == 0
        for c, key in enumerate(("hobj", "heq", "hineq")):
            assert nnz[c] == len(g[f"{key}_rows_{tag}"]), (name, tag, key)
            assert np.array_equal(rows[c][:nnz[c]], np.array(g[f"{key}_rows_{tag}"], np.int32)), (name, tag, key)
            assert np.array_equal(cols[c][:nnz[c]], np.array(g[f"{key}_cols_{tag}"], np.int32)), (name, tag, key)
    n, m = C.c_int32(0), C.c_int32(0)
    assert lib.corbo_hip_linear_form_structure(C.byref(d), C.byref(n), C.byref(m), None, None) == 0
    assert n.value == len(g["lin_rows"]) and m.value == len(g["lin_lbA"])
    r, c = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
    assert lib.corbo_hip_linear_form_structure(C.byref(d), C.byref(n), C.byref(m), ipp(r), ipp(c)) == 0
    assert np.array_equal(r, np.array(g["lin_rows"], np.int32)) and np.array_equal(c, np.array(g["lin_cols"], np.int32))


def test_user_model_directory_is_registered(lib):
    """csrc/models/*.hpp (user dynamics models): the build registers every header under CORBO_HIP_DYN_USER + slot; the shipped example is the
    kinematic car in slot 0 -- accepted with its own shape, refused with another, and an empty slot is an unknown dynamics id."""
    import __graft_entry__ as g
    from control_box_rst_amd import problems
    models = g.user_models()
    assert ("kinematic_car", 0, 3, 2) in [(m[0], m[1], m[2], m[3]) for m in models]
    reg = open(os.path.join(ROOT, "control_box_rst_amd", "csrc", "models", "_registry.inc")).read()
    for name, slot, nx, nu, prm, _ in models:
        assert f"CORBO_HIP_USER_MODEL({name}, {slot}, {nx}, {nu}," in reg
    d = problems.kinematic_car_desc(N=12)
    dims = capi.Dims()
    assert lib.corbo_hip_get_dims(C.byref(d), C.byref(dims)) == 0 and dims.n == 55
    d.nu = 1
    assert lib.corbo_hip_get_dims(C.byref(d), C.byref(dims)) != 0
    d = problems.kinematic_car_desc(N=12)
    d.dynamics = capi.DYN_USER + 9
    assert lib.corbo_hip_get_dims(C.byref(d), C.byref(dims)) != 0
    # a model of the big-block family (5 <= nx <= 12): the planar quadrotor in slot 1
    assert ("planar_quadrotor", 1, 6, 2) in [(m[0], m[1], m[2], m[3]) for m in models]
    d = problems.planar_quadrotor_desc(N=10)
    assert lib.corbo_hip_get_dims(C.byref(d), C.byref(dims)) == 0 and (dims.n, dims.m) == (72, 159)   # = the reference's own count (tests/golden/pquad_n10.json)
    d.nx = 5
    assert lib.corbo_hip_get_dims(C.byref(d), C.byref(dims)) != 0


def test_user_stage_function_directory_is_registered(lib):
    """csrc/stage_functions/*.hpp (user stage inequalities): the build registers every header under CORBO_HIP_STAGE_FN_USER + slot with its kind; the shipped
    examples -- tilt cone (state term, slot 0), input-magnitude bound (control term, slot 1) -- evaluate on the host through the very templates the kernels compile."""
    import __graft_entry__ as g
    fns = g.user_stage_functions()
    assert ("tilt_cone", 0, 0, 8) in [f[:4] for f in fns] and ("control_norm", 1, 1, 1) in [f[:4] for f in fns]
    reg = open(os.path.join(ROOT, "control_box_rst_amd", "csrc", "stage_functions", "_registry.inc")).read()
    for name, slot, kind, nxmin, _ in fns:
        assert f"CORBO_HIP_USER_STAGE({name}, {slot}, {kind}, {nxmin})" in reg
    assert lib.corbo_hip_stage_function_kind(capi.STAGE_FN_USER + 0) == 0 and lib.corbo_hip_stage_function_kind(capi.STAGE_FN_USER + 1) == 1
    assert lib.corbo_hip_stage_function_kind(capi.STAGE_FN_USER + 7) == -1
    rng = np.random.default_rng(3)
    dp = C.POINTER(C.c_double)
    x = rng.standard_normal((5, 12)); u = rng.standard_normal((5, 4)); out = np.zeros(5)
    prm = np.zeros(8); prm[0] = 0.4
    assert lib.corbo_hip_eval_stage_function(capi.STAGE_FN_USER + 0, 12, 5, x.ctypes.data_as(dp), prm.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0
    assert np.array_equal(out, (x[:, 6] * x[:, 6] + x[:, 7] * x[:, 7]) - 0.4 * 0.4)
    assert lib.corbo_hip_eval_stage_function(capi.STAGE_FN_USER + 1, 4, 5, u.ctypes.data_as(dp), prm.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0
    ref = np.zeros(5)
    for i in range(4):
        ref = ref + u[:, i] * u[:, i]
    assert np.array_equal(out, ref - 0.4 * 0.4)
    ball = np.array([1.0, 0.5, 0.2, 0.3, 0, 0, 0, 0.0])
    assert lib.corbo_hip_eval_stage_function(capi.INEQ_BALL, 3, 5, np.ascontiguousarray(x[:, :3]).ctypes.data_as(dp), ball.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0
    d3 = x[:, :3] - ball[:3]
    assert np.allclose(out, 0.09 - (d3 * d3).sum(axis=1), rtol=1e-14)
    # descriptors: a state function below its nx_min, a control function named as the state term, an unregistered slot
    from control_box_rst_amd import problems
    dims = capi.Dims()
    d = problems.unicycle_desc(N=12); d.stage_ineq = capi.STAGE_FN_USER + 0
    assert lib.corbo_hip_get_dims(C.byref(d), C.byref(dims)) != 0
    d = problems.unicycle_desc(N=12); d.stage_ineq = capi.STAGE_FN_USER + 1
    assert lib.corbo_hip_get_dims(C.byref(d), C.byref(dims)) != 0
    d = problems.unicycle_desc(N=12); d.stage_ineq_control = capi.STAGE_FN_USER + 1
    assert lib.corbo_hip_get_dims(C.byref(d), C.byref(dims)) == 0 and dims.ineq == 11
    d.stage_ineq_control = capi.STAGE_FN_USER + 5
    assert lib.corbo_hip_get_dims(C.byref(d), C.byref(dims)) != 0
