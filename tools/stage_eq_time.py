"""Headline workload (1024 unicycle OCPs, N = 100) with a user stage equality on (x_k, u_k) -- heading_tie, slot 4 of csrc/stage_functions/ -- per solve,
through the block-tridiagonal route and the band route, next to the same batch with the control-deviation term measured the same way (what bench.py reports
as secondary.band_path.headline_batch_with_rate_limit) and the plain problem (diagnostics; an informative figure, no gate).  python tools/stage_eq_time.py [kind ...]   (kinds: plain rate heading_tie; default all)"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from control_box_rst_amd import capi, problems
from control_box_rst_amd.solver import BatchedLevenbergMarquardt, get_dims
B = 1024
for kind in (sys.argv[1:] or ("plain", "rate", "heading_tie")):
    w = bench.workload(3, B)
    d = w["desc"]
    if kind == "rate":
        d.ctrl_dev = capi.CTRL_DEV_RATE
        d.ctrl_dev_params[0] = 1.0; d.ctrl_dev_params[1] = 1.0
    if kind == "heading_tie":
        problems.with_state_control_eq(d, 4, (0.8, 0.05))
    dims = get_dims(d)
    for route in ((0,) if kind == "plain" else (0, capi.ROUTE_XE_BAND)):
        s = BatchedLevenbergMarquardt(d, B, route=route); s.setIterations(10); s.setPenaltyWeights(*w["weights"])
        s.set_instance_data(s.init_trajectory(w["x0"], w["xf"]), xref=w["xf"]); s.solve(new_run=True); s.synchronize()
        reps = 5 if not route else 2
        t0 = time.perf_counter()
        for _ in range(reps): s.restore_instance_data(); s.solve(new_run=True)
        s.synchronize(); ms = (time.perf_counter() - t0) / reps * 1e3
        st = s.get_stats(); chi2 = s.get_solution()[1]
        tag = "" if kind == "plain" else (" band route " if route else " block route")
        print(f"batch {B:5d} {kind:12s}{tag}: {ms:8.2f} ms per solve, passes {st['passes']}, factorizations {st['factorizations']}, accepted {st['accepted_steps']}, chi2 sum {chi2.sum():.10g}, n {dims.n}, m {dims.m}", flush=True)
        del s
