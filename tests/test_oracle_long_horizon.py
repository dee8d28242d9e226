"""CPU twin of test_gpu_long_horizon.py: the same inputs (long_horizon_inputs.py) through the oracle alone, wherever the suite runs.

What the device file relies on is asserted here:
  * the model cases cover every small-block row of csrc/model_table.inc and csrc/models/; their starts have active bound rows; three iterations of the oracle
    from starts one ulp apart agree to half the solve tolerances of the device file (the tolerance is never below the reference's own noise);
  * on every seed of the random campaign chi2 is finite, the status is converged or early terminated, and 8 x the oracle's own one-ulp spread stays within
    WIDEN_CAP x the base tolerance for the iterate and for chi2: the cap of the device file cannot hide the reference's own noise.
Nothing is written."""
import numpy as np
import pytest

import long_horizon_inputs as H
from conftest import LEDGER
from control_box_rst_amd import capi
from test_gpu_fuzz import WIDEN_CAP, oracle_own_spread

X_TOL = 2 * LEDGER["default_x_tol"]
CHI2_RTOL = LEDGER["default_chi2_rtol"]
_TABLE_NAME = {"int2": "integ2", "int3": "integ3", "kcar": "user_kinematic_car"}


def test_model_cases_cover_every_small_block_model_unit():
    import __graft_entry__ as g
    small = {n for n, _, nx, nu in g.builtin_models() if nx <= 4} | {"user_" + m[0] for m in g.user_models() if m[2] <= 4}
    for formula in ("cn", "ms_rk4"):
        have = {_TABLE_NAME.get(m, m) for m, f in H.MODEL_CASES if f == formula}
        assert have == small, (formula, sorted(small ^ have))
    for m in ("unicycle", "cartpole"):
        assert {f for mm, f in H.MODEL_CASES if mm == m} == {"cn", "forward", "backward", "midpoint", "ms_euler", "ms_rk2", "ms_rk3", "ms_rk4", "ms_rk5", "ms_rk7"}
    for m, f in H.MODEL_CASES:
        d = H.model_desc(m, f)
        assert (d.N, d.nx <= 4) == (257, True)
        assert (d.grid == capi.GRID_MS) == f.startswith("ms_")
    assert len(set(H.MODEL_CASES)) == len(H.MODEL_CASES) == 56 and H.MODEL_BATCH == 2


@pytest.mark.parametrize("model,formula", H.MODEL_CASES, ids=[f"{m}-{f}" for m, f in H.MODEL_CASES])
def test_model_case_is_well_posed_for_the_oracle(oracle_mod, model, formula):
    d, w, X0, xf = H.model_input(oracle_mod, model, formula)
    opts = capi.default_lm_opts(3, *w)
    for b in range(H.MODEL_BATCH):
        p = oracle_mod.OracleProblem(d)
        p.set_data(X0[b], xref=xf[b])
        rows, _ = p.structure()
        v, j = p.eval(*w)
        assert np.isfinite(v).all() and np.isfinite(j).all()
        assert np.count_nonzero(j[rows >= p.dims.m - p.dims.bounds]) >= 8, (model, formula, b)   # active bound rows
    Xo, chi2, status = oracle_mod.solve_batch(d, X0, xf, opts)
    sx, sc = oracle_own_spread(oracle_mod, d, X0, xf, opts, d.nx)
    sx_abs = sx * max(1.0, np.abs(Xo).max())
    print(f"{model}-{formula} chi2={chi2} status={status.tolist()} own spread: x {sx_abs:.2e} chi2 {sc:.2e}")
    assert np.isfinite(chi2).all() and set(status.tolist()) <= {0, 1}
    assert sx_abs <= 0.5 * X_TOL and sc <= 0.5 * CHI2_RTOL, (model, formula, sx_abs, sc)


def test_fuzz_seeds_are_48_and_reach_every_block_shape(oracle_mod):
    assert len(H.FUZZ_SEEDS) == len(set(H.FUZZ_SEEDS)) == 48 and not set(H.FUZZ_SEEDS) & set(H.FUZZ_REPLACED)
    assert (H.FUZZ_BATCH, H.FUZZ_ITERATIONS) == (3, 3)
    descs = [H.fuzz_input(oracle_mod, s)[1] for s in H.FUZZ_SEEDS]
    assert all(257 <= d.N <= 1024 for d in descs)
    assert {(d.nx, d.nu) for d in descs} == {(2, 1), (2, 2), (3, 1), (3, 2), (3, 3), (4, 1)}
    assert {d.grid for d in descs} == {capi.GRID_FD, capi.GRID_FD_VARIABLE, capi.GRID_MS, capi.GRID_MS_VARIABLE}
    assert all(bool(d.weights_dense) == (s % 3 == 0) for s, d in zip(H.FUZZ_SEEDS, descs))


@pytest.mark.parametrize("seed", H.FUZZ_SEEDS)
def test_fuzz_seed_is_reproducible_by_the_oracle(oracle_mod, seed):
    fam, d, w, X0, xf = H.fuzz_input(oracle_mod, seed)
    opts = capi.default_lm_opts(H.FUZZ_ITERATIONS, *w)
    _, chi2, status = oracle_mod.solve_batch(d, X0, xf, opts)
    sx, sc = oracle_own_spread(oracle_mod, d, X0, xf, opts, d.nx)
    print(f"seed={seed} {fam} N={d.N} nx={d.nx} nu={d.nu} grid={d.grid} dense={d.weights_dense} status={status.tolist()} own spread: x {sx:.2e} chi2 {sc:.2e}")
    assert np.isfinite(chi2).all(), (seed, fam, chi2)
    assert set(status.tolist()) <= {0, 1}, (seed, fam, status)   # converged / early terminated
    assert 8.0 * sx <= WIDEN_CAP * H.FUZZ_X_TOL, (seed, fam, sx)
    assert 8.0 * sc <= WIDEN_CAP * H.fuzz_chi2_rtol(d), (seed, fam, sc)
