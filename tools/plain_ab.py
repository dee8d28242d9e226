"""Option "plain_kernel" 0 against 1 in ONE process, headline shape (1024 unicycle OCPs, N = 100, 10 LM iterations): wall clock per step of 100 re-arming
solves, the option alternating, in three regimes -- enqueued on two lanes (bench.py's default), enqueued on one lane ("async_lanes" 1), synchronous
(bench.py --sync-steps).  The iterates of the two kernels are compared bit for bit first.   python tools/plain_ab.py [reps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bench
from control_box_rst_amd.solver import BatchedLevenbergMarquardt
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
w = bench.workload(3, 1024)
s = BatchedLevenbergMarquardt(w["desc"], 1024)
s.setIterations(10); s.setPenaltyWeights(*w["weights"])
s.set_instance_data(s.init_trajectory(w["x0"], w["xf"]), xref=w["xf"])
s.set_result_sink(True)
got = {}
for plain in (0, 1):
    s.set_option("plain_kernel", plain)
    s.solve(rearm=True)
    got[plain] = [a.copy() for a in s.get_solution()]
    assert s.get_stats()["plain_kernel"] == plain
print("bit-identical iterates, chi2, status:", all(np.array_equal(a, b) for a, b in zip(got[0], got[1])), flush=True)
t = time.perf_counter()
while time.perf_counter() - t < 0.5:
    s.solve(rearm=True)
REGIMES = (("two lanes", 2, True), ("one lane", 1, True), ("synchronous", 2, False))
out = {(r[0], p): [] for r in REGIMES for p in (0, 1)}
for rep in range(reps):
    for name, lanes, enq in REGIMES:
        s.set_option("async_lanes", lanes)
        for plain in (0, 1):
            s.set_option("plain_kernel", plain)
            for _ in range(4): s.solve_async(rearm=True)
            s.synchronize(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(100):
                if enq: s.solve_async(rearm=True)
                else: s.solve(rearm=True)
            s.synchronize(); torch.cuda.synchronize()
            out[(name, plain)].append(1e3 * (time.perf_counter() - t0) / 100)
for name, _, _ in REGIMES:
    a, b = np.array(out[(name, 0)]), np.array(out[(name, 1)])
    spread = max(a.max() - a.min(), b.max() - b.min())
    print(f"{name}: general median {np.median(a):.4f} [{a.min():.4f}, {a.max():.4f}]  plain median {np.median(b):.4f} [{b.min():.4f}, {b.max():.4f}] ms/step; "
          f"gain {np.median(a) - np.median(b):+.4f} ms = {100 * (1 - np.median(b) / np.median(a)):.2f} %, {((np.median(a) - np.median(b)) / spread if spread > 0 else float('inf')):.1f} x the larger spread; "
          f"ranges {'overlap' if b.max() >= a.min() else 'do not overlap'}")
