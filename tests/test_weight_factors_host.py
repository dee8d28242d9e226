"""corbo_hip_create_weighted (non-diagonal Q / R / Qf beside the descriptor): layout mirror and the gate that runs before any HIP call.

Without a device a request that passes the gate fails with CORBO_HIP_ERR_DEVICE (-2); one the gate refuses fails with CORBO_HIP_ERR_INVALID (-1)
on any machine."""
import ctypes as C

import numpy as np
import pytest

from control_box_rst_amd import capi, problems
from control_box_rst_amd.solver import weight_factors


@pytest.fixture(scope="module")
def lib():
    return capi.load()


def _create(lib, d, w):
    h = C.c_void_p()
    rc = lib.corbo_hip_create_weighted(C.byref(d), None if w is None else C.byref(w), 1, 0, 0, C.byref(h))
    if rc == 0:
        lib.corbo_hip_destroy(h)
    else:
        assert not h.value
    return rc


def _quad_factors(d):
    rng = np.random.default_rng(7)
    A = rng.standard_normal((12, 12))
    Q = A @ A.T + 12 * np.eye(12)
    return weight_factors(d, {"Q": Q, "R": np.diag(problems.QUAD_R) + 0.001, "Qf": 10 * Q})


def test_sizeof_mirror(lib):
    assert lib.corbo_hip_sizeof(4) == C.sizeof(capi.WeightFactors) == 8 + (2 * 16 * 16 + 8 * 8) * 8


def test_upper_factor():
    W = np.array([[4.0, 2.0], [2.0, 3.0]])
    U = problems.upper_factor(W)
    assert U[1, 0] == 0.0 and np.allclose(U.T @ U, W, rtol=0, atol=1e-15)


@pytest.mark.parametrize("case", ["below_diagonal", "q_without_stage_cost", "qf_without_final_cost", "nonlsq", "ctrl_dev", "both_sources",
                                  "free_dt", "rk6"])
def test_gate_refuses_before_touching_the_device(lib, case):
    d = problems.quad_desc(N=10)
    w = _quad_factors(d)
    if case == "below_diagonal":
        w.q_sqrt[1 * 12 + 0] = 0.5
    elif case == "q_without_stage_cost":
        d.stage_cost = capi.COST_NONE
        w.mask = 1
    elif case == "qf_without_final_cost":
        d.final_cost = 0
        w.mask = 4
    elif case == "nonlsq":
        d.cost_nonlsq = 1
    elif case == "ctrl_dev":
        d.ctrl_dev = capi.CTRL_DEV_RATE
        for i in range(4):
            d.ctrl_dev_params[i] = 5.0
    elif case == "both_sources":
        d.weights_dense = 1
    elif case == "free_dt":
        d = problems.quad_desc(N=10, time_optimal=True)
        d.stage_cost = capi.COST_MIN_TIME_QUADRATIC_LSQ
        w.mask = 1
    elif case == "rk6":
        d.shooting_integrator = 6
    assert _create(lib, d, w) == -1
    why = lib.corbo_hip_last_error().decode()
    named = {"ctrl_dev": "extra edges", "free_dt": "free-dt grid", "rk6": "Runge-Kutta 5 - 7", "both_sources": "one source of truth",
             "below_diagonal": "upper triangular"}
    assert named.get(case, "") in why, why


def test_valid_quadrotor_request_passes_the_gate(lib):
    import torch
    d = problems.quad_desc(N=10)
    rc = _create(lib, d, _quad_factors(d))
    if not torch.cuda.is_available():
        assert rc == -2
    else:
        assert rc == 0


def test_null_weights_is_create_routed(lib):
    import torch
    d = problems.quad_desc(N=10)
    rc = _create(lib, d, None)
    assert rc == (0 if torch.cuda.is_available() else -2)
    d.nx = 5   # an invalid descriptor is refused the same way
    assert _create(lib, d, None) == -1


def test_small_family_factors_need_upper_triangular(lib):
    d = problems.unicycle_desc(N=12)
    w = weight_factors(d, {"Q_sqrt": np.triu(np.full((3, 3), 0.5)) + np.eye(3)})
    w.q_sqrt[2 * 3 + 1] = 0.1
    assert _create(lib, d, w) == -1
