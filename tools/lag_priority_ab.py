"""Option "lag_priority" 2 (on for every launch) against 1 (the default: off for launches that overlap the other lane's) and 0 (off) in ONE process, headline shape (1024 unicycle OCPs, N = 100, 10 LM iterations, two lanes): wall clock per step of 100
enqueued re-arming solves, alternating the option (the per-pass progress-row bookkeeping of the fused pass kernel on / off), and a bit-compare of the results.
Then, general kernel only (PLAIN carries no diagnostics): the factor phase's mean cycles per pass from option "phase_cycles"."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bench
from control_box_rst_amd.solver import BatchedLevenbergMarquardt
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
w = bench.workload(3, 1024)


def handle(options=()):
    s = BatchedLevenbergMarquardt(w["desc"], 1024)
    s.setIterations(10); s.setPenaltyWeights(*w["weights"])
    for k, v in options: s.set_option(k, v)
    s.set_instance_data(s.init_trajectory(w["x0"], w["xf"]), xref=w["xf"])
    return s


s = handle()
s.set_result_sink(True)
t = time.perf_counter()
while time.perf_counter() - t < 0.5:
    s.solve(rearm=True)
out, res = {0: [], 1: [], 2: []}, {}
for rep in range(REPS):
    for lag in (2, 1, 0):
        s.set_option("lag_priority", lag)
        for _ in range(4): s.solve_async(rearm=True)
        s.synchronize(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(100): s.solve_async(rearm=True)
        s.synchronize(); torch.cuda.synchronize()
        wall = 1e3 * (time.perf_counter() - t0) / 100
        out[lag].append(wall)
        if lag not in res: res[lag] = [np.array(a, copy=True) for a in s.get_solution()]
        print(f"rep {rep} lag_priority {lag}: wall {wall:.4f} ms/step", flush=True)
for lag in (2, 1, 0):
    a = np.array(out[lag])
    print(f"lag_priority {lag}: median {np.median(a):.4f} min {a.min():.4f} max {a.max():.4f} ms/step")
print("results bit-identical on / default / off:", all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(res[0], res[1], res[2])))
s.close()
g = handle((("plain_kernel", 0), ("phase_cycles", 1)))
g.solve()
pc = g.get_phase_cycles()   # [batch][8]: cycles of the Jacobian sweep / residual sweep / factor phases [0..2], their counts [3..5]
print(f"general kernel, phase_cycles: factor phase {pc[:, 2].sum() / pc[:, 5].sum():.0f} cycles per pass over {int(pc[:, 5].sum())} passes; "
      f"Jacobian sweep {pc[:, 0].sum() / max(pc[:, 3].sum(), 1):.0f} x {int(pc[:, 3].sum())}, residual sweep {pc[:, 1].sum() / max(pc[:, 4].sum(), 1):.0f} x {int(pc[:, 4].sum())}")
g.close()
