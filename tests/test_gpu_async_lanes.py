"""The two lanes of a handle (-m gpu): enqueued re-arming solves (corbo_hip_solve_async, new_run = 2) alternate between two sets of stream + working
set + pinned result buffers and overlap on the chip; every other call is ordered behind both lanes and works on the lane of the newest solve.  Whatever
the routing, a caller sees what the synchronous calls give -- compared bit for bit, with option "async_lanes" 1 (one stream, as before) and 2 (default)."""
import time

import numpy as np
import pytest

from control_box_rst_amd import problems, sharding
from control_box_rst_amd.solver import BatchedLevenbergMarquardt, CorboHipError

pytestmark = pytest.mark.gpu

LANES = [1, 2]


@pytest.fixture(scope="module", autouse=True)
def _built():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import __graft_entry__ as g
    g.build()


def _solver(shape="small", lanes=2, B=48, N=40, seed=20260928):
    if shape == "headline":   # bench.py's flagship workload: 1024 unicycle OCPs, N = 100, 10 LM iterations
        import bench
        w = bench.workload(3, 1024)
        s = BatchedLevenbergMarquardt(w["desc"], 1024)
        s.setIterations(10)
        s.setPenaltyWeights(*w["weights"])
        s.set_instance_data(s.init_trajectory(w["x0"], w["xf"]), xref=w["xf"])
    else:
        d = problems.unicycle_desc(N=N)
        x0, xf = problems.unicycle_instances(B, seed=seed)
        s = BatchedLevenbergMarquardt(d, B)
        s.setPenaltyWeights(*problems.UNICYCLE_WEIGHTS)
        s.set_instance_data(s.init_trajectory(x0, xf), xref=xf)
    s.set_option("async_lanes", lanes)
    return s


def _stats(s):
    return {k: v for k, v in s.get_stats().items() if not k.endswith("_ms")}


def _results(s):
    """(fetch_solution views as copies, get_solution arrays, statistics, address of the pinned iterate view)."""
    Xv, cv, sv = s.fetch_solution()
    addr = Xv.__array_interface__["data"][0]
    fetched = [np.array(a, copy=True) for a in (Xv, cv, sv)]
    got = [a.copy() for a in s.get_solution()]
    return fetched, got, _stats(s), addr


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("sink", [True, False])
@pytest.mark.parametrize("count", [6, 5])
@pytest.mark.parametrize("shape", ["small", "headline"])
def test_back_to_back_rearming_solves_equal_one_synchronous_solve(shape, count, sink, lanes):
    s = _solver(shape, lanes)
    s.set_result_sink(sink)
    s.solve(rearm=True)
    ref_fetched, ref_got, ref_stats, addr0 = _results(s)
    for _ in range(count):
        s.solve_async(rearm=True)
    s.synchronize()
    fetched, got, stats, addr = _results(s)
    assert _same(fetched, ref_fetched), "fetch_solution"
    assert _same(got, ref_got), "get_solution"
    assert stats == ref_stats
    # the pinned views are the newest lane's: solve k of the chain runs on lane k mod 2 (the first one finds nothing in flight and stays)
    assert (addr != addr0) == (lanes == 2 and count % 2 == 0)
    s.solve(rearm=True)   # ... and a synchronous solve afterwards works on that lane
    assert _same(_results(s)[1], ref_got)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("lead", [0, 1])
def test_continuation_runs_from_the_newest_lanes_iterate(lead, lanes):
    """rearm, new_run = 0, new_run = 1: the second and third solve continue from the iterate of the solve before them -- on whichever lane that one ran
    (lead = 1: one more re-arming solve in front, so that it is the second lane)."""
    def run(async_):
        s = _solver("small", lanes)
        s.set_result_sink(True)
        go = s.solve_async if async_ else s.solve
        for _ in range(lead):
            go(rearm=True)
        go(rearm=True)
        go(new_run=False)
        go(new_run=True)
        s.synchronize()
        fetched, got, stats, _ = _results(s)
        return fetched + got, stats
    a, b = run(True), run(False)
    assert _same(a[0], b[0]) and a[1] == b[1]


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("mutator", ["warm_start", "set_instance_data", "restore_instance_data"])
def test_mutator_behind_enqueued_rearming_solves(mutator, lanes):
    def run(async_):
        s = _solver("small", lanes)
        s.set_result_sink(True)
        for _ in range(3):
            (s.solve_async if async_ else s.solve)(rearm=True)
        if mutator == "warm_start":
            x0, _ = problems.unicycle_instances(48, seed=7)
            s.warm_start(x0, shift=False)
        elif mutator == "set_instance_data":
            x0, xf = problems.unicycle_instances(48, seed=11)
            s.set_instance_data(s.init_trajectory(x0, xf), xref=xf)
        else:
            s.restore_instance_data()
        return [np.array(a, copy=True) for a in s.fetch_solution()]
    assert _same(run(True), run(False))


@pytest.mark.parametrize("lanes", LANES)
def test_pass_limit_on_both_lanes_is_reported_once(lanes):
    s = _solver("small", lanes)
    s.solve(rearm=True)
    ref = [a.copy() for a in s.get_solution()]
    s.set_option("pass_limit", 3)     # 10 outer iterations need at least 10 passes
    s.solve_async(rearm=True)
    s.solve_async(rearm=True)         # (two lanes: one failing solve on each)
    with pytest.raises(CorboHipError, match="pass limit"):
        s.synchronize()
    s.synchronize()                   # reported once
    s.set_option("pass_limit", 0)
    for _ in range(3):                # the handle is usable afterwards, enqueued solves included
        s.solve_async(rearm=True)
    s.synchronize()
    assert _same(s.get_solution(), ref)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("count", [3, 2])
def test_device_views_are_the_newest_lanes(count, lanes):
    import torch
    s = _solver("small", lanes)
    for _ in range(count):
        s.solve_async(rearm=True)
    dev = sharding.gather_trajectories_device(s, s.batch)   # world 1: a copy of the handle's resident iterates
    assert np.array_equal(dev.cpu().numpy(), s.get_solution()[0])
    # without a wait in between: the views' buffer is the newest lane's, and device-wide completion covers both lanes
    for _ in range(count):
        s.solve_async(rearm=True)
    view = s.device_tensor()
    torch.cuda.synchronize()
    got = view[:, : s.dims.nv].cpu().numpy()
    assert np.array_equal(got, s.get_solution()[0])


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("kind", ["queue", "host_driven"])
def test_queue_mode_and_host_driven_handles_stay_on_one_lane(kind, lanes):
    import torch
    if kind == "queue":   # more instances than resident workgroups (4 per compute unit): the instance queue, short horizon
        B = 4 * torch.cuda.get_device_properties(0).multi_processor_count + 64
        d = problems.unicycle_desc(N=10)
        x0, xf = problems.unicycle_instances(B)
        weights = problems.UNICYCLE_WEIGHTS
    else:                 # big-block family: passes launched from the host
        B = 4
        d = problems.quad_desc(N=24)
        x0, xf = problems.quad_instances(B)
        weights = problems.QUAD_WEIGHTS
    s = BatchedLevenbergMarquardt(d, B)
    s.setPenaltyWeights(*weights)
    s.set_instance_data(s.init_trajectory(x0, xf), xref=xf)
    s.set_option("async_lanes", lanes)
    s.set_result_sink(True)
    s.solve(rearm=True)
    ref_fetched, ref_got, ref_stats, addr0 = _results(s)
    for count in (2, 3):
        for _ in range(count):
            s.solve_async(rearm=True)
        s.synchronize()
        fetched, got, stats, addr = _results(s)
        assert _same(fetched, ref_fetched) and _same(got, ref_got) and stats == ref_stats
        assert addr == addr0, "the pinned result buffer changed: the solve left its lane"


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("shape,K", [("small", 7), ("headline", 8)])
def test_timing_counts_every_solve_and_is_bounded_by_the_wall_clock(shape, K, lanes):
    """corbo_hip_get_timing: the length of the union of the launch intervals -- overlapping launches are not counted twice, so the sum cannot exceed the
    host's wall clock from the first enqueue to the return of synchronize()."""
    s = _solver(shape, lanes)
    s.set_result_sink(True)
    s.solve(rearm=True)
    for _ in range(2):                # (both lanes exist before anything is timed)
        s.solve_async(rearm=True)
    s.synchronize()
    s.get_timing(reset=True)
    t0 = time.perf_counter()
    for _ in range(K):
        s.solve_async(rearm=True)
    s.synchronize()
    wall_ms = 1e3 * (time.perf_counter() - t0)
    ms, n = s.get_timing(reset=True)
    print(f"get_timing: n={n} sum={ms:.4f} ms, wall clock {wall_ms:.4f} ms (lanes={lanes}, {shape})")
    assert n == K
    assert ms > 0
    assert ms <= wall_ms
    assert s.get_stats()["solve_ms"] > 0   # the newest solve's own interval
