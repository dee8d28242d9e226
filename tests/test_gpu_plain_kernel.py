"""The plain instantiation of the fused pass kernel (-m gpu): lm_pass_kernel<.., PLAIN> exists for one shape -- N = 100, two waves, fixed dt, diagonal
weights, run to completion -- and one problem class: no stage / final inequality, no terminal equality, no per-vertex references, no instance queue, no
diagnostic option.  Its option code is compiled out, its arithmetic is the general instantiation's: with option "plain_kernel" 1 (default) and 0 a handle
gives the same bits -- iterates, chi2, status, every counter -- through the synchronous solve, the enqueued re-arming solves on both lanes, result sink on
and off.  A handle outside the class reports the general kernel (corbo_hip_stats::plain_kernel = 0) and agrees with the oracle as before.

N = 100 is the only horizon with the instantiation, hence the smallest shape at which it can be wrong; batches of three instances, 10 iterations."""
import numpy as np
import pytest

import lm_step_check as L
from control_box_rst_amd import capi, problems
from control_box_rst_amd.solver import BatchedLevenbergMarquardt

pytestmark = pytest.mark.gpu

N = 100
ITERATIONS = 10
X_TOL, CHI2_RTOL = 5e-6, 2e-6   # device against oracle: tests/tolerances.json default_x_tol / default_chi2_rtol (test_gpu_parity.py)

# every defect formula with a fused pass kernel: (id, lm_step_check family, defect or None = the family's)
DEFECTS = [("forward", "unicycle", capi.DEFECT_FORWARD), ("backward", "unicycle", capi.DEFECT_BACKWARD), ("midpoint", "unicycle", capi.DEFECT_MIDPOINT),
           ("crank_nicolson", "unicycle", capi.DEFECT_CRANK_NICOLSON), ("rk4_shooting", "unicyclems", None)]
# starts (lm_step_check.make_start): the accepted-at-once ones of its table, and its rejecting goals for N = 100 (the unicycle's: four times the distance; the
# shooting grid's: controls that start at zero, twice the distance)
STARTS = {"accepted": {"unicycle": ("line",), "unicyclems": ("line",)},
          "rejecting": {"unicycle": ("perturbed", 0.0, 0, 4.0), "unicyclems": ("perturbed", 0.0, 0, 2.0)}}


@pytest.fixture(scope="module", autouse=True)
def _built():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import __graft_entry__ as g
    g.build()


_inputs = {}


def _input(oracle_mod, family, start):
    """(descriptor, X0, xref) of an lm_step_check case at N = 100: computed once, shared, never written"""
    key = (family, start)
    if key not in _inputs:
        d, X0, xref = L.make_start(L.Case("cr", family, N, start=start), oracle_mod)
        X0.setflags(write=False)
        xref.setflags(write=False)
        _inputs[key] = (d, X0, xref)
    return _inputs[key]


def _handle(d, X0, xref, weights, iterations=ITERATIONS, options=()):
    s = BatchedLevenbergMarquardt(d, X0.shape[0])
    s.setIterations(iterations)
    s.setPenaltyWeights(*weights)
    s.set_instance_data(np.array(X0), xref=np.array(xref))
    for k, v in options:
        s.set_option(k, v)
    return s


def _counters(s):
    """(corbo_hip_stats without the times and the kernel flag, the kernel flag)"""
    st = s.get_stats()
    return {k: v for k, v in st.items() if not k.endswith("_ms") and k != "plain_kernel"}, st["plain_kernel"]


def _outcome(s):
    return [a.copy() for a in s.get_solution()], _counters(s)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["accepted", "rejecting"])
@pytest.mark.parametrize("name,family,defect", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_plain_kernel_gives_the_general_kernels_bits(oracle_mod, name, family, defect, kind):
    d, X0, xref = _input(oracle_mod, family, STARTS[kind][family])
    if defect is not None:
        d = type(d).from_buffer_copy(d)
        d.defect = defect
    ref = None
    for plain in (0, 1):
        for sink in (False, True):
            s = _handle(d, X0, xref, problems.UNICYCLE_WEIGHTS, options=(("plain_kernel", plain),))
            s.set_result_sink(sink)
            s.solve(rearm=True)                      # the synchronous solve
            got, (counters, flag) = _outcome(s)
            assert flag == plain, f"{name}: corbo_hip_stats.plain_kernel = {flag} with option plain_kernel = {plain}"
            if ref is None:
                ref = (got, counters)
                if kind == "rejecting":
                    assert counters["rejected_steps"] > 0, "the comparison misses the passes after a rejected step"
            assert _same(got, ref[0]) and counters == ref[1], f"{name} {kind}: synchronous solve, plain_kernel={plain} sink={sink}"
            for _ in range(3):                       # enqueued re-arming solves: both lanes
                s.solve_async(rearm=True)
            s.synchronize()
            fetched = [np.array(a, copy=True) for a in s.fetch_solution()]
            got, (counters, flag) = _outcome(s)
            assert flag == plain
            assert _same(got, ref[0]) and counters == ref[1], f"{name} {kind}: enqueued solves, plain_kernel={plain} sink={sink}"
            assert np.array_equal(fetched[0][:, : s.dims.nv], ref[0][0]) and np.array_equal(fetched[1], ref[0][1]) and np.array_equal(fetched[2], ref[0][2])
            s.close()


def _oracle(oracle_mod, d, X0, xref, weights, iterations, refs=None):
    X, chi2 = [], []
    for b in range(X0.shape[0]):
        p = oracle_mod.OracleProblem(d)
        p.set_data(np.array(X0[b]), xref=np.array(xref[b]))
        if refs is not None:
            p.set_references(refs[b])
        _, c, _ = p.solve(capi.default_lm_opts(iterations, *weights))
        X.append(p.x())
        chi2.append(c)
    return np.stack(X), np.array(chi2)


def _general_and_oracle(oracle_mod, what, s, d, X0, xref, weights, iterations, refs=None, x_tol=X_TOL):
    s.solve()
    (X, chi2, _), (_, flag) = _outcome(s)
    assert flag == 0, f"{what}: the handle ran the plain kernel"
    Xo, chi2o = _oracle(oracle_mod, d, X0, xref, weights, iterations, refs)
    err = float(np.abs(X - Xo).max())
    print(f"{what}: max|x_gpu - x_oracle| = {err:.3e}, chi2 rel {float(np.abs(chi2 - chi2o).max() / np.abs(chi2o).max()):.3e}")
    assert err <= x_tol, (what, err)
    assert np.allclose(chi2, chi2o, rtol=CHI2_RTOL), what


# handles outside the plain class: what puts them outside, descriptor family, descriptor change, handle options
def _ball(d):
    d.stage_ineq = capi.INEQ_BALL
    for i, v in enumerate((1.0, 0.5, 0.25, 0.35)):   # (the keep-out ball of the unicycle_n24_ball fixture)
        d.ineq_params[i] = v


def _terminal_ball(d):
    d.final_ineq = capi.FINAL_INEQ_TERMINAL_BALL
    for i, v in enumerate((1.0, 1.0, 0.1, 0.02)):
        d.final_ineq_params[i] = v


def _terminal_equality(d):
    d.final_eq = 1


OUTSIDE = [("stage_inequality", "unicycle", _ball, ()), ("terminal_ball", "unicycle", _terminal_ball, ()), ("terminal_equality", "unicycle", _terminal_equality, ()),
           ("phase_cycles", "unicycle", None, (("phase_cycles", 1),)), ("pass_timeline", "unicycle", None, (("pass_timeline", 0),)),
           ("free_dt", "int3t", None, ()), ("dense_weights", "unicycle+dense", None, ())]
ITER_OUTSIDE = 5   # (the comparison with the oracle: finite-difference noise grows with every iteration, the class of the handle does not change)


@pytest.mark.parametrize("what,family,change,options", OUTSIDE, ids=[o[0] for o in OUTSIDE])
def test_handles_outside_the_plain_class_run_the_general_kernel(oracle_mod, what, family, change, options):
    d, X0, xref = _input(oracle_mod, family, ("line",))
    if change is not None:
        d = type(d).from_buffer_copy(d)
        change(d)
    weights = L.penalty_weights(L.Case("cr", family, N))
    s = _handle(d, X0, xref, weights, ITER_OUTSIDE, options)
    # (the keep-out ball and the TerminalBall: twice the default, as in test_small_family_with_stage_inequality_vs_oracle)
    _general_and_oracle(oracle_mod, what, s, d, X0, xref, weights, ITER_OUTSIDE, x_tol=2 * X_TOL if what in ("stage_inequality", "terminal_ball") else X_TOL)
    if what == "phase_cycles":
        assert s.get_phase_cycles()[:, 2].min() > 0   # the diagnostic itself still works
    s.close()


def test_per_vertex_references_run_the_general_kernel(oracle_mod):
    d, X0, xref = _input(oracle_mod, "unicycle", ("line",))
    B, S = X0.shape[0], d.nx + d.nu
    traj = np.stack([X0[:, k * S:k * S + d.nx] for k in range(N)], axis=1) + 0.05   # [B][N][nx]: the start's states, shifted
    s = _handle(d, X0, xref, problems.UNICYCLE_WEIGHTS, ITER_OUTSIDE)
    s.set_references(traj)
    refs = np.zeros((B, s.dims.nv))
    for k in range(N):
        refs[:, k * S:k * S + d.nx] = traj[:, k]
    _general_and_oracle(oracle_mod, "per-vertex references", s, d, X0, xref, problems.UNICYCLE_WEIGHTS, ITER_OUTSIDE, refs=refs)
    s.set_references(None)   # ... and back inside the class
    s.restore_instance_data()
    s.solve()
    assert _counters(s)[1] == 1
    s.close()


def test_queue_mode_runs_the_general_kernel(oracle_mod):
    """More instances than resident workgroups (4 per compute unit): the instance queue.  Checked once: the first and the last rows against a small handle
    on the general kernel (bit for bit: the instances are independent) and against the oracle."""
    import torch
    B = 4 * torch.cuda.get_device_properties(0).multi_processor_count + 8
    d = problems.unicycle_desc(N=N)
    x0, xf = problems.unicycle_instances(B)
    s = BatchedLevenbergMarquardt(d, B)
    s.setIterations(ITER_OUTSIDE)
    s.setPenaltyWeights(*problems.UNICYCLE_WEIGHTS)
    X0 = s.init_trajectory(x0, xf)
    s.set_instance_data(X0, xref=xf)
    s.solve()
    (X, chi2, status), (_, flag) = _outcome(s)
    assert flag == 0, "queue mode: the handle ran the plain kernel"
    rows = np.r_[0:4, B - 4:B]
    small = _handle(d, X0[rows], xf[rows], problems.UNICYCLE_WEIGHTS, ITER_OUTSIDE, (("plain_kernel", 0),))
    small.solve()
    (Xs, chi2s, statuss), (_, flag) = _outcome(small)
    assert flag == 0
    assert np.array_equal(X[rows], Xs) and np.array_equal(chi2[rows], chi2s) and np.array_equal(status[rows], statuss)
    Xo, chi2o = _oracle(oracle_mod, d, X0[rows], xf[rows], problems.UNICYCLE_WEIGHTS, ITER_OUTSIDE)
    assert np.abs(Xs - Xo).max() <= X_TOL and np.allclose(chi2s, chi2o, rtol=CHI2_RTOL)
    s.close()
    small.close()
