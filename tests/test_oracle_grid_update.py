"""CPU tests of the grid-update table (tests/grid_update_cases.py): the oracle's warm start and resampling against plain numpy restatements written
from the reference's lines, bit for bit, on every case the device runs in test_gpu_grid_update.py; every warm-start case shifts by what it was built
for; every mutant of the restatements -- one plausible slip each -- differs from the oracle somewhere on the table, so the table can see that slip;
every descriptor of the table passes corbo_hip_create's device-kernel gate (host only), so no device test can come back `unsupported`.  The reference
fixtures of the same shapes are replayed by test_oracle_mpc.py (mpc_*_jump*) and test_oracle_adapt.py (the nx = 3 / 6 / 12 chains)."""
import numpy as np
import pytest

import grid_update_cases as G


@pytest.fixture(scope="module")
def ws_oracle(oracle_mod):
    """{case: (oracle result, inputs)}: computed once, shared, never written."""
    return {c: G.oracle_warm_start(oracle_mod, c) for c in G.WS_CASES}


@pytest.fixture(scope="module")
def rs_oracle(oracle_mod):
    """{(family, n_src, n_dst, exact): (X, [oracle result per instance])} -- the two grid variants share inputs and expectation."""
    out = {}
    for fam, _, n_src, n_dst, exact in G.rs_cases():
        key = (fam, n_src, n_dst, exact)
        if key not in out:
            nx, nu, _ = G.RS_FAMILIES[fam]
            X, _ = G.rs_inputs(fam, n_src, n_dst, exact)
            out[key] = (X, [oracle_mod.resample_trajectory(nx, nu, X[b], n_dst) for b in range(G.RS_BATCH)])
    return out


def _np_ws(c, inputs, mutant=None):
    d, X, x0, xref = inputs
    return G.np_warm_start(X, x0, xref, d.nx, d.nu, c.N, c.shift, int(d.xf_fixed_mask), mutant=mutant)


@pytest.mark.parametrize("case", G.WS_CASES, ids=G.ws_id)
def test_warm_start_restatement_equals_oracle_and_shifts_as_intended(ws_oracle, case):
    want, inputs = ws_oracle[case]
    got, num_shift = _np_ws(case, inputs)
    assert num_shift == case.expect, (G.ws_id(case), num_shift, case.expect)   # a condition on the INPUTS: the case reaches the path it names
    assert np.array_equal(got, want), G.ws_id(case)
    d, X = inputs[0], inputs[1]
    s = d.nx + d.nu
    if case.expect > 0:
        assert not np.array_equal(want[s:2 * s], X[s:2 * s])   # something did move
    if case.kind == "tie":
        assert np.array_equal(X[s:s + d.nx], X[2 * s:2 * s + d.nx])


def test_warm_start_table_reaches_every_path():
    """The paths the issue names, by what the cases realise."""
    shifts = {(c.N, c.expect) for c in G.WS_CASES}
    assert {(3, 1), (4, 2), (7, 5), (22, 20)} <= shifts                              # num_shift == N - 2 (extrapolation from idx = 2)
    assert any(c.expect == 20 and c.target > 20 for c in G.WS_CASES)                  # the look-ahead cap cuts the search
    assert any(c.kind == "tie" for c in G.WS_CASES) and any(c.kind == "same_start" for c in G.WS_CASES)
    for fam, mk in G.WS_FAMILIES.items():
        assert any(c.family == fam and not c.shift for c in G.WS_CASES), fam
    assert any(int(G.WS_FAMILIES[c.family](c.N).xf_fixed_mask) == 0b101 and c.expect > 0 for c in G.WS_CASES)
    lds = lambda fam, N: 8 * ((((N - 1) * (G.WS_FAMILIES[fam](N).nx + G.WS_FAMILIES[fam](N).nu) + G.WS_FAMILIES[fam](N).nx + 2) & ~1) + 24)
    assert lds("quad", 510) <= 65536 < lds("quad", 511) and lds("pquad", 1024) == 65728   # the rows above 64 KB of LDS are in the table
    assert {("quad", 511), ("quad", 520), ("pquad", 1024), ("unicycle", 257)} <= {(c.family, c.N) for c in G.WS_CASES}


@pytest.mark.parametrize("mutant", G.WS_MUTANTS)
def test_every_warm_start_mutant_differs_from_the_oracle_somewhere(ws_oracle, mutant):
    seen = [G.ws_id(c) for c in G.WS_CASES if not np.array_equal(_np_ws(c, ws_oracle[c][1], mutant)[0], ws_oracle[c][0])]
    assert seen, mutant


@pytest.mark.parametrize("mutant", G.WS_EQUIVALENT_MUTANTS)
def test_equivalent_warm_start_mutants_change_nothing(ws_oracle, mutant):
    """See grid_update_cases.WS_EQUIVALENT_MUTANTS: a slip no input can show (here the stray control is NaN, and no NaN survives)."""
    for c in G.WS_CASES:
        assert np.array_equal(_np_ws(c, ws_oracle[c][1], mutant)[0], ws_oracle[c][0]), G.ws_id(c)


@pytest.mark.parametrize("case", [c for c in G.rs_cases() if c[1] == "fd"], ids=G.rs_id)
def test_resampling_restatement_equals_oracle(rs_oracle, case):
    fam, _, n_src, n_dst, exact = case
    nx, nu, _ = G.RS_FAMILIES[fam]
    X, want = rs_oracle[(fam, n_src, n_dst, exact)]
    for b in range(G.RS_BATCH):
        assert np.array_equal(G.np_resample(nx, nu, X[b], n_dst), want[b]), (G.rs_id(case), b)
    if exact:   # the comparisons of the running while-loop ARE exact: every new time is a multiple of the old dt in binary
        dt_new = X[0, -1] * float(n_src - 1) / float(n_dst - 1)
        hits = [k for k in range(1, n_dst - 1) if any(dt_new * float(k) == float(j) * 0.125 for j in range(1, n_src))]
        assert X[0, -1] == 0.125 and len(hits) >= (n_dst - 2) // 2, (hits, n_dst)


@pytest.mark.parametrize("mutant", G.RS_MUTANTS)
def test_every_resampling_mutant_differs_from_the_oracle_somewhere(rs_oracle, mutant):
    seen = []
    for (fam, n_src, n_dst, exact), (X, want) in rs_oracle.items():
        nx, nu, _ = G.RS_FAMILIES[fam]
        if not np.array_equal(G.np_resample(nx, nu, X[0], n_dst, mutant), want[0]):
            seen.append((fam, n_src, n_dst))
    assert seen, mutant
    if mutant == "ge_for_gt":   # an exact hit tells `>=` from `>`: every exact case does
        assert {(f, a, b) for (f, a, b, e) in rs_oracle if e} <= set(seen)


def test_every_descriptor_of_the_table_passes_the_device_kernel_gate():
    """corbo_hip_create accepts every (family, N) the device tests create -- none had to be replaced by a smaller N."""
    refused = [(fam, N) for fam, N in sorted({(c.family, c.N) for c in G.WS_CASES}) if not G.gate_accepts(G.WS_FAMILIES[fam](N))]
    for fam, (_, _, mk) in G.RS_FAMILIES.items():
        for grid in ("fd", "ms"):
            for N in sorted({n for c in G.rs_cases() if c[0] == fam for n in c[2:4]}):
                if not G.gate_accepts(mk(N, grid)):
                    refused.append((fam, grid, N))
    assert not refused, refused


def test_index_lists_permute_and_leave_slots_untouched():
    assert len(set(G.RS_SRC_INDEX)) == len(G.RS_SRC_INDEX) == len(set(G.RS_DST_INDEX)) and G.RS_SRC_INDEX != G.RS_DST_INDEX
    assert set(range(G.RS_BATCH)) - set(G.RS_DST_INDEX)
