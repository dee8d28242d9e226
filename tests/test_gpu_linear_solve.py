"""GPU tests (-m gpu): the linear solve inside one LM iteration of every factorisation route, against the normal equations (tests/lm_step_check.py).

A batch of three instances, setIterations(1): upload, eval() (J and r at x_0), restore_instance_data(), solve(), get_solution().  Per instance

  * eta_device = |H delta - g|_inf / (|H|_inf |delta|_inf + |g|_inf) <= 16 max(eta_oracle of the same instance, 2^-53), with H = J^T J + sum(mu) I from the
    device's own Jacobian, delta = x_1 - x_0 and the cumulative damping of the oracle's pass count (the counters below tie the device to that count);
  * x_1 is bit-equal to x_0 at every vertex entry that is no parameter (x_0 of the horizon, fixed components of x_f);
  * factorizations / accepted_steps / rejected_steps of corbo_hip_stats equal the sums over the oracle's traces;
  * the returned chi2 is |r(x_1)|^2 of a second eval at the uploaded x_1, to 1e-13 relative.

The table (lm_step_check.CASES) holds the smallest shapes at which each path switches: the stage-parallel cyclic reduction (lm_pass_kernel, per-pass mode, DENSE),
factor_long_kernel on both sides of its LDS / HBM workspace switch, lm_bt_kernel with two and three workgroups per CU up to its BIG instantiation,
band_narrow_kernel / band_factor_kernel, the chain kernels of the big-block family with one, two and four segments, a free dt, and reject-streak speculation;
rejecting starts drive the added mu and the snapshot reload.  test_oracle_linear_solve.py runs the same inputs on the oracle wherever the suite runs.

A corbo_hip_create_weighted handle (random symmetric positive definite Q, R, Qf around the quadrotor, N = 12) runs the same check against a reference
assembled on the host (lm_step_check.weighted_case: the oracle takes non-diagonal weights through the descriptor only, i.e. for nx <= 4).
"""
import math

import numpy as np
import pytest

import lm_step_check as L
from control_box_rst_amd.solver import get_structure

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def inputs(oracle_mod):
    """input key -> (desc, X0, xref, the oracle's first iteration, its eta per instance); computed once per input, shared by the cases that differ in handle
    options only, left unchanged"""
    cache = {}

    def get(case):
        if case.input_key not in cache:
            d, X0, xref = L.make_start(case, oracle_mod)
            rec = L.oracle_first_iteration(oracle_mod, case, d, X0, xref)
            cache[case.input_key] = (d, X0, xref, rec, [L.eta_of(o) for o in rec])
        return cache[case.input_key]
    return get


@pytest.mark.parametrize("case", L.CASES, ids=[c.id for c in L.CASES])
def test_lm_step_solves_the_normal_equations(inputs, case):
    d, X0, xref, rec, eta_oracle = inputs(case)
    s, values, jac, x1, chi2, stats = L.device_first_iteration(case, d, X0, xref)
    assert s.factor_route() == case.expect, (case.id, s.factor_route())
    rows, cols = get_structure(d)
    assert np.array_equal(rows, rec[0]["rows"]) and np.array_equal(cols, rec[0]["cols"])
    _check_instances(case.id, rows, cols, rec, eta_oracle, X0, values, jac, x1)
    _check_counters_and_chi2(case.id, s, rec, stats, x1, xref, chi2)


def _check_instances(name, rows, cols, rec, eta_ref, X0, values, jac, x1):
    failures = []
    for b, o in enumerate(rec):
        delta = x1[b][o["off"]] - X0[b][o["off"]]
        sum_mu = L.expected_damping(L.initial_damping(cols, jac[b], o["n"]), o["passes"])
        eta = L.step_backward_error(rows, cols, jac[b], values[b], delta, sum_mu)
        bound = L.DEVICE_MARGIN * max(eta_ref[b], L.U)
        print(f"LMSTEP {name} [{b}] n={o['n']} passes={o['passes']} eta_device={eta:.3e} eta_oracle={eta_ref[b]:.3e} bound={bound:.3e}")
        if not eta <= bound:
            failures.append((b, eta, bound))
        assert np.array_equal(x1[b][o["fixed"]].view(np.int64), X0[b][o["fixed"]].view(np.int64)), (name, b, "a vertex entry that is no parameter moved")
    assert not failures, (name, failures)


def _check_counters_and_chi2(name, s, rec, stats, x1, xref, chi2):
    passes, accepted = sum(o["passes"] for o in rec), sum(o["accepted"] for o in rec)
    assert stats["factorizations"] == passes, (name, stats, passes)
    assert stats["accepted_steps"] == accepted and stats["rejected_steps"] == passes - accepted, (name, stats, passes, accepted)
    s.set_instance_data(x1, xref=xref)   # chi2 of the solve = |r(x_1)|^2 of the hook at the uploaded x_1
    v1, _ = s.eval(jacobian=False)
    for b in range(len(rec)):
        want = math.fsum(float(v) * float(v) for v in v1[b])
        assert abs(chi2[b] - want) <= 1e-13 * want, (name, b, chi2[b], want)


def test_lm_step_of_a_weighted_handle(oracle_mod):
    from control_box_rst_amd import capi
    from control_box_rst_amd.solver import BatchedLevenbergMarquardt
    d, wts, X0, xref, rec = L.weighted_case(oracle_mod)
    s = BatchedLevenbergMarquardt(d, X0.shape[0], weights=wts)
    assert s.factor_route() == capi.FACTOR_STAGE_CHAIN
    s.setIterations(1)
    s.setPenaltyWeights(*L.penalty_weights(L.Case("big", "quad", L.WEIGHTED_N)))
    s.set_instance_data(X0, xref=xref)
    values, jac = s.eval()
    s.restore_instance_data()
    s.solve()
    x1, chi2, _ = s.get_solution()
    rows, cols = get_structure(d)
    assert np.array_equal(rows, rec[0]["rows"]) and np.array_equal(cols, rec[0]["cols"])
    _check_instances("big-quad+weighted-N12", rows, cols, rec, [L.eta_of(o) for o in rec], X0, values, jac, x1)
    _check_counters_and_chi2("big-quad+weighted-N12", s, rec, s.get_stats(), x1, xref, chi2)


PRECONDITION = [c for c in L.CASES if c.id in ("cr-unicycle-N100", "cr-int3t-N33", "long-unicycle-N800", "bt-unicycle+rate-N40-rej0-bt_waves2",
                                               "band-vdp+eqlin-N300-route2-band_wide0", "band-quad+rate-N20", "big-quad-N37-chain_variant4", "big-pquad-N16-chain_variant2")]


@pytest.mark.parametrize("case", PRECONDITION, ids=[c.id for c in PRECONDITION])
def test_two_evals_return_the_same_bits(inputs, case):
    """the hook leaves the resident iterate alone: a second eval() on the same handle returns bit-identical residuals and Jacobians"""
    from control_box_rst_amd.solver import BatchedLevenbergMarquardt
    assert len(PRECONDITION) == 8
    d, X0, xref, _, _ = inputs(case)
    s = BatchedLevenbergMarquardt(d, X0.shape[0], route=case.create_route)
    s.setPenaltyWeights(*L.penalty_weights(case))
    s.set_instance_data(X0, xref=xref)
    v0, j0 = s.eval()
    v1, j1 = s.eval()
    assert np.array_equal(v0.view(np.int64), v1.view(np.int64)) and np.array_equal(j0.view(np.int64), j1.view(np.int64))
    x, _, _ = s.get_solution()
    assert np.array_equal(x.view(np.int64), X0.view(np.int64))
