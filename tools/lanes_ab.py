"""Option "async_lanes" 1 against 2 in ONE process, headline shape (1024 unicycle OCPs, N = 100, 10 LM iterations): wall clock per step of 100 enqueued
re-arming solves, alternating the option, next to corbo_hip_get_timing (union of the launch intervals) and the newest launch's own interval."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bench
from control_box_rst_amd.solver import BatchedLevenbergMarquardt
w = bench.workload(3, 1024)
s = BatchedLevenbergMarquardt(w["desc"], 1024)
s.setIterations(10); s.setPenaltyWeights(*w["weights"])
s.set_instance_data(s.init_trajectory(w["x0"], w["xf"]), xref=w["xf"])
s.set_result_sink(True)
t = time.perf_counter()
while time.perf_counter() - t < 0.5:
    s.solve(rearm=True)
out = {1: [], 2: []}
for rep in range(7):
    for lanes in (1, 2):
        s.set_option("async_lanes", lanes)
        for _ in range(4): s.solve_async(rearm=True)
        s.synchronize(); torch.cuda.synchronize(); s.get_timing(reset=True)
        t0 = time.perf_counter()
        for _ in range(100): s.solve_async(rearm=True)
        s.synchronize(); torch.cuda.synchronize()
        wall = 1e3 * (time.perf_counter() - t0) / 100
        ms, n = s.get_timing(reset=True)
        own = s.get_stats()["solve_ms"]
        out[lanes].append((wall, ms / n, own))
        print(f"rep {rep} lanes {lanes}: wall {wall:.4f} ms/step, get_timing union {ms / n:.4f} ms/launch (n={n}), newest launch's own interval {own:.4f} ms", flush=True)
for lanes in (1, 2):
    a = np.array(out[lanes])
    print(f"lanes {lanes}: wall median {np.median(a[:,0]):.4f} min {a[:,0].min():.4f} max {a[:,0].max():.4f}; union/launch median {np.median(a[:,1]):.4f}; own interval median {np.median(a[:,2]):.4f}")
