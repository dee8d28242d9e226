"""GPU tests (-m gpu) of the kernels that rewrite the resident trajectories between solves -- warm_start_kernel (moving-horizon shift +
extrapolation), resample_kernel (time-optimal grid adaptation), reference_window_kernel (the resident tracking reference) -- on the table of
tests/grid_update_cases.py: every shift up to N - 2 and up to the look-ahead cap, a tie, a partially fixed goal together with a shift, fewer active
slots than the handle has, every block width (nx + nu = 3 .. 16), horizons beyond one trip of the 256-lane loops and rows above 64 KB of LDS.
Every comparison is bit for bit against the oracle (which test_oracle_grid_update.py holds against a plain restatement of the reference's lines on
the same table), but for the reference's own multi-sample shift fixtures, which go through a 0-iteration solve.  No test runs an LM iteration."""
import numpy as np
import pytest

import grid_update_cases as G
from conftest import desc_for, load_golden
from control_box_rst_amd import problems
from control_box_rst_amd.solver import BatchedLevenbergMarquardt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import __graft_entry__ as g
    g.build()


WS_GROUPS = G.ws_groups()


@pytest.mark.parametrize("key", list(WS_GROUPS), ids=lambda k: f"{k[0]}-N{k[1]}-{'shift' if k[2] else 'noshift'}")
def test_warm_start_equals_oracle_bitwise(oracle_mod, key):
    """set_instance_data -> warm_start -> get_solution: the cases of one (family, N) are the instances of one batch."""
    cases = WS_GROUPS[key]
    want, inputs = zip(*[G.oracle_warm_start(oracle_mod, c) for c in cases])
    d = inputs[0][0]
    s = BatchedLevenbergMarquardt(d, len(cases))
    assert s.dims.nv == len(want[0])
    s.set_instance_data(np.array([i[1] for i in inputs]), xref=np.array([i[3] for i in inputs]))
    s.warm_start(np.array([i[2] for i in inputs]), shift=key[2])
    Xd, _, _ = s.get_solution()
    for b, c in enumerate(cases):
        assert np.array_equal(Xd[b], want[b]), (G.ws_id(c), int((Xd[b] != want[b]).sum()), np.flatnonzero(Xd[b] != want[b])[:8])
    s.close()


def test_warm_start_leaves_the_slots_beyond_active_untouched(oracle_mod):
    a = G.WS_ACTIVE_CASE
    cases = [G.WsCase(a["family"], a["N"], "path", j, True, min(j, 20)) for j in a["targets"]]
    want, inputs = zip(*[G.oracle_warm_start(oracle_mod, c) for c in cases])
    X = np.array([i[1] for i in inputs])
    s = BatchedLevenbergMarquardt(inputs[0][0], a["batch"])
    s.set_instance_data(X, xref=np.array([i[3] for i in inputs]))
    s.prepare_slots(a["active"])
    s.warm_start(np.array([i[2] for i in inputs]), shift=True)
    s.prepare_slots(a["batch"])
    Xd, _, _ = s.get_solution()
    for b in range(a["batch"]):
        assert np.array_equal(Xd[b], want[b] if b < a["active"] else X[b]), b
    assert not np.array_equal(want[a["active"]], X[a["active"]])   # (the rows left alone would have moved)
    s.close()


@pytest.mark.parametrize("case", G.rs_cases(), ids=G.rs_id)
def test_resample_into_equals_oracle_bitwise(oracle_mod, case):
    """set_instance_data / prepare_slots -> resample_into -> get_solution; xref rows travel with the trajectories, untouched slots stay zero."""
    fam, grid, n_src, n_dst, exact = case
    nx, nu, mk = G.RS_FAMILIES[fam]
    B = G.RS_BATCH
    X, xref = G.rs_inputs(fam, n_src, n_dst, exact)
    src = BatchedLevenbergMarquardt(mk(n_src, grid), B)
    dst = BatchedLevenbergMarquardt(mk(n_dst, grid), B)
    src.set_instance_data(X, xref=xref)
    dst.prepare_slots(B)
    src.resample_into(dst, G.RS_SRC_INDEX, G.RS_DST_INDEX)
    Y, _, _ = dst.get_solution()
    for s_i, d_i in zip(G.RS_SRC_INDEX, G.RS_DST_INDEX):
        want = oracle_mod.resample_trajectory(nx, nu, X[s_i], n_dst)
        assert np.array_equal(Y[d_i], want), (G.rs_id(case), s_i, int((Y[d_i] != want).sum()), np.flatnonzero(Y[d_i] != want)[:8])
    for d_i in set(range(B)) - set(G.RS_DST_INDEX):
        assert np.array_equal(Y[d_i], np.zeros(dst.dims.nv)), d_i   # untouched slots
    # the xref rows were carried: with a fixed goal a warm start of the destination (no shift on a free dt) writes them into x_f
    mask = int(dst.desc.xf_fixed_mask)
    assert mask != 0
    dst.warm_start(Y[:, :nx], shift=False)
    Z, _, _ = dst.get_solution()
    for s_i, d_i in zip(G.RS_SRC_INDEX, G.RS_DST_INDEX):
        xf = Z[d_i, (n_dst - 1) * (nx + nu):(n_dst - 1) * (nx + nu) + nx]
        for c in range(nx):
            assert xf[c] == (xref[s_i, c] if (mask >> c) & 1 else Y[d_i, (n_dst - 1) * (nx + nu) + c]), (G.rs_id(case), d_i, c)
    if n_dst == n_src:   # same N: a move inside one handle (compaction), the source row staged before the destination is written
        src.resample_into(src, [4], [1])
        W, _, _ = src.get_solution()
        assert np.array_equal(W[1], X[4]) and np.array_equal(W[0], X[0]) and np.array_equal(W[4], X[4])
    src.close()
    dst.close()


WINDOW_FAMILIES = {2: lambda N: problems.vdp_desc(N=N), 3: lambda N: problems.unicycle_desc(N=N), 12: lambda N: problems.quad_desc(N=N)}
WINDOW_N = 9


@pytest.mark.parametrize("nx", sorted(WINDOW_FAMILIES))
def test_reference_window_equals_the_explicit_window_bitwise(nx):
    """Per-instance DIFFERENT reference trajectories of T samples, seen from control step `step`: set_reference_trajectory(traj, step) + eval() gives
    the residuals and the Jacobian of a second handle that was handed the window traj[b][min(step + k, T - 1)], k < N, through set_references."""
    N, B = WINDOW_N, 4
    d = WINDOW_FAMILIES[nx](N)
    rng = np.random.default_rng(nx)
    a, b = BatchedLevenbergMarquardt(d, B), BatchedLevenbergMarquardt(d, B)
    X = rng.normal(size=(B, a.dims.nv))
    xref = rng.normal(size=(B, nx))
    for h in (a, b):
        h.set_instance_data(X, xref=xref)
    v_static, _ = b.eval()
    for T in (1, N - 3, N, N + 5):
        traj = rng.normal(size=(B, T, nx))
        assert T == 1 or not np.array_equal(traj[0], traj[1])
        for step in (0, 3, T - 1, T + 2):
            a.set_reference_trajectory(traj, step=step)
            win = traj[:, [min(step + k, T - 1) for k in range(N)], :]
            b.set_references(win)
            va, ja = a.eval()
            vb, jb = b.eval()
            assert np.array_equal(va, vb) and np.array_equal(ja, jb), (nx, T, step, np.flatnonzero((va != vb).any(axis=0))[:8])
            assert not np.array_equal(vb, v_static)   # the window is what the cost terms see
            for i in range(1, B):
                assert not np.array_equal(vb[i], vb[0])
    a.close()
    b.close()


@pytest.mark.parametrize("name", list(G.SHIFT_FIXTURES))
def test_reference_multi_sample_shift_on_the_device(name):
    """The genuine reference shifting by 2 .. 20 samples (iters = 0: the dumps are the warm-started vertex vectors after the one Jacobian sweep of a
    0-iteration compute()): the previous dump -> warm_start -> the same 0-iteration solve, to the tolerance test_gpu_mpc.test_sequence_vs_reference
    uses for the family."""
    g = load_golden(name)
    d = desc_for(g)
    s = BatchedLevenbergMarquardt(d, 1)
    s.setPenaltyWeights(*g["weights"])
    s.setIterations(0)
    nv = s.dims.nv
    tol = 3e-4 if "quad" in name else 1e-5
    for k in range(1, len(g["steps"])):
        prev, cur = g["steps"][k - 1], g["steps"][k]
        assert G.fixture_num_shift(g, prev["vertex"], cur["x0"]) == G.SHIFT_FIXTURES[name][k - 1]
        s.set_instance_data(np.array(prev["vertex"])[None, :nv], xref=np.array(g["xf"])[None, :])
        s.warm_start(np.array(cur["x0"])[None, :], shift=True)
        s.solve(new_run=True)
        x, _, _ = s.get_solution()
        err = np.abs(x[0] - np.array(cur["vertex"])[:nv]).max()
        print(name, k, "num_shift", G.SHIFT_FIXTURES[name][k - 1], "max |x - ref|", err)
        assert err <= tol, (name, k, err)
    s.close()
