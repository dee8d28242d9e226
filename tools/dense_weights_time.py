"""Dense against diagonal weights on cfg 5's batch: 512 quadrotors, N = 200, multiple shooting with RK4, 10 LM iterations per solve.

One process, both handles built up front, warm-up solves first, then `--steps` timed solves of each (alternating, so that clock drift hits both);
per-solve time = the library's HIP-event time of corbo_hip_solve (corbo_hip_get_timing).  Dense weights: Q / R / Qf with the fullq pattern of
oracle/ref_driver.cpp (off-diagonals 0.25 sqrt(w_i w_j)) through corbo_hip_create_weighted.  Prints one JSON line.

    python tools/dense_weights_time.py [--batch 512] [--N 200] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fullq(w):
    w = np.asarray(w, dtype=np.float64)
    W = 0.25 * np.sqrt(np.outer(w, w))
    np.fill_diagonal(W, w)
    return W


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--N", type=int, default=200)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from control_box_rst_amd import problems
    from control_box_rst_amd.solver import BatchedLevenbergMarquardt

    d = problems.quad_desc(N=a.N)
    x0, xf = problems.quad_instances(a.batch)
    q = [d.q_diag[i] for i in range(12)]
    r = [d.r_diag[i] for i in range(4)]
    qf = [d.qf_diag[i] for i in range(12)]
    handles = {"diagonal": BatchedLevenbergMarquardt(d, a.batch),
               "dense": BatchedLevenbergMarquardt(d, a.batch, weights={"Q": fullq(q), "R": fullq(r), "Qf": fullq(qf)})}
    X0 = handles["diagonal"].init_trajectory(x0, xf)
    for s in handles.values():
        s.setIterations(a.iterations)
        s.setPenaltyWeights(*problems.QUAD_WEIGHTS)
        s.set_instance_data(X0, xref=xf)
    for _ in range(a.warmup):
        for s in handles.values():
            s.set_instance_data(X0, xref=xf)
            s.solve(new_run=True)
    for s in handles.values():
        s.get_timing(reset=True)
    for _ in range(a.steps):
        for s in handles.values():
            s.set_instance_data(X0, xref=xf)
            s.solve(new_run=True)
    out = {"batch": a.batch, "N": a.N, "iterations": a.iterations, "steps": a.steps}
    for name, s in handles.items():
        ms, n = s.get_timing()
        out[name + "_ms_per_solve"] = round(ms / max(n, 1), 4)
        X, chi2, status = s.get_solution()
        out[name + "_chi2_median"] = float(np.median(chi2))
        out[name + "_stats"] = {k: v for k, v in s.get_stats().items() if k in ("lm_iterations", "rejected_steps", "factorizations", "passes")}
    out["ratio"] = round(out["dense_ms_per_solve"] / out["diagonal_ms_per_solve"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
