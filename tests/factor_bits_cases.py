"""The cases of tests/test_gpu_factor_bits.py and tools/record_factor_bits.py (one table, so that the recorder and the test cannot drift apart).

Every case is a handle of four unicycle OCPs (problems.unicycle_instances(4), its default seed), 10 LM iterations, solved once; what is kept of it
is the iterates, chi2, status and the handle's counters (corbo_hip_get_stats without the times: the C-ABI counts per handle, i.e. the totals over the
four instances).  All of them run factor_body: the horizons are the smallest at which each lane mapping of its cyclic reduction can go wrong.

  headline class (Crank-Nicolson, plain problem class, two waves):
      N = 2 .. 5    root level only / no regular level          N = 64, 65   the COMPACT first level switches on above 64
      N = 8, 9      first regular level                         N = 100      the NPC = 101 instantiations: PLAIN and general (option plain_kernel 1 / 0)
      N = 16, 17    the twisted top appears                     N = 124      last two-wave horizon (N + nx + 1 = 128)
      N = 33
  rejecting start (the goal four times as far away, lm_step_check's ("perturbed", 0.0, 0, 4.0)): N = 12, N = 100 -- the reload path after a rejected step
  other instantiations of the same code: forward-Euler defect, a free dt (the arrowhead), non-diagonal weights, one pass per launch, all at N = 12;
      four waves at N = 130
"""
import numpy as np

from control_box_rst_amd import capi, problems

BATCH = 4
ITERATIONS = 10
COUNTERS = ("lm_iterations", "accepted_steps", "rejected_steps", "jacobian_sweeps", "residual_sweeps", "factorizations", "passes", "inner_loop_cuts",
            "plain_kernel", "counted_iterations", "speculative_takeovers")
REJECTING_DIST = 4.0


def _forward(d):
    d.defect = capi.DEFECT_FORWARD


def _free_dt(d):
    d.grid, d.dt_lb, d.dt_ub = capi.GRID_FD_VARIABLE, 0.01, 10.0


def _dense(d):
    """random symmetric positive definite Q / R / Qf as upper Cholesky factors (the construction of lm_step_check._dense_weights, its seed for nx = 3)"""
    rd = np.random.default_rng(99003)
    d.weights_dense = 1 | 2 | 4
    for dst, n in ((d.q_sqrt, d.nx), (d.r_sqrt, d.nu), (d.qf_sqrt, d.nx)):
        a = rd.uniform(-1, 1, (n, n))
        for i, v in enumerate(np.linalg.cholesky(a.T @ a + 0.5 * np.eye(n)).T.ravel()):
            dst[i] = float(v)


# id -> (N, rejecting start, descriptor change or None, handle options, expected corbo_hip_stats::plain_kernel or None)
CASES = {}
for _N in (2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 124):
    CASES[f"cn-N{_N}"] = (_N, False, None, (), 0)
for _plain in (1, 0):
    CASES[f"cn-N100-plain{_plain}"] = (100, False, None, (("plain_kernel", _plain),), _plain)
CASES["rej-N12"] = (12, True, None, (), 0)
for _plain in (1, 0):
    CASES[f"rej-N100-plain{_plain}"] = (100, True, None, (("plain_kernel", _plain),), _plain)
CASES["forward-N12"] = (12, False, _forward, (), 0)
CASES["free-dt-N12"] = (12, False, _free_dt, (), 0)
CASES["four-waves-N130"] = (130, False, None, (), 0)
CASES["dense-N12"] = (12, False, _dense, (), 0)
CASES["per-pass-N12"] = (12, False, None, (("run_to_completion", 0),), 0)


def run_case(case_id):
    """-> {"x": [4][nv], "chi2": [4], "status": [4] int32, "counters": [len(COUNTERS)] int64} of one solve on the device"""
    from control_box_rst_amd.solver import BatchedLevenbergMarquardt
    N, rejecting, change, options, plain = CASES[case_id]
    d = problems.unicycle_desc(N=N)
    if change is not None:
        change(d)
    x0, xf = problems.unicycle_instances(BATCH)
    if rejecting:
        xf = x0 + REJECTING_DIST * (xf - x0)
    s = BatchedLevenbergMarquardt(d, BATCH)
    try:
        s.setIterations(ITERATIONS)
        s.setPenaltyWeights(*problems.UNICYCLE_WEIGHTS)
        for k, v in options:
            s.set_option(k, v)
        s.set_instance_data(s.init_trajectory(x0, xf), xref=xf)
        s.solve()
        x, chi2, status = s.get_solution()
        st = s.get_stats()
    finally:
        s.close()
    assert st["plain_kernel"] == plain, f"{case_id}: corbo_hip_stats.plain_kernel = {st['plain_kernel']}, expected {plain}"
    if rejecting:
        assert st["rejected_steps"] > 0, f"{case_id}: the start is meant to reject"
    return {"x": x, "chi2": chi2, "status": status.astype(np.int32), "counters": np.array([st[k] for k in COUNTERS], np.int64)}
