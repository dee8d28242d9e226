"""CPU twin of test_gpu_stage_function_xu.py's iterate and LM-step tests: the reference they compare against (stage_function_xu_cases.Reference --
oracle.GenericProblem over the OCP oracle's rows plus the state-control term's rows from the host evaluator) is built and solved here without a device, and
what makes the GPU tests meaningful is asserted: rows of the term are active at every start, the rejecting starts reject, and the derived tolerances of
every case -- max(the ledger's defaults, 4 x the oracle's own spread over starts one ulp away) -- stay at or below the hard gate 1e-5 on x and on relative
chi2 for k = 1 .. 5, so that the GPU comparison cannot go vacuous."""
import numpy as np
import pytest

import lm_step_check as L
import stage_function_xu_cases as X


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


@pytest.mark.parametrize("name, N, start, iterations", X.ITERATE_CASES, ids=X.ITERATE_IDS)
def test_iterate_reference_has_active_rows_and_tolerances_inside_the_hard_gate(oracle_mod, name, N, start, iterations):
    """(The quadrotor is compared at k = 1 only: see the note at stage_function_xu_cases.ITERATE_CASES.)"""
    d, X0, xref = X.make_start(oracle_mod, name, N, **start)
    w = X.penalty_weights(name)
    ref = X.Reference(oracle_mod, d, X0[0], xref[0])
    c0 = X.term_values(d, X0[0])
    assert (c0 > 0).any() and (c0 < 0).any(), "active and inactive rows of the term at the start"
    chi2_prev = None
    for k in iterations:
        xo, co, xtol, ctol = ref.iterate_with_spread(k, w)
        print(f"XUREF {name}-N{N} k={k} chi2={co:.9e} xtol={xtol:.3e} ctol={ctol:.3e}")
        assert np.all(np.isfinite(xo)) and np.isfinite(co)
        assert xtol <= X.HARD_X and ctol <= X.HARD_CHI2, (name, k, xtol, ctol)
        assert chi2_prev is None or co <= chi2_prev
        chi2_prev = co
    # the term matters: the same solve without its rows ends elsewhere
    p = oracle_mod.OracleProblem(X.without_term(d))
    p.set_data(X0[0], xref=xref[0])
    from control_box_rst_amd import capi
    p.solve(capi.default_lm_opts(iterations[-1], *w), new_run=True)
    assert np.abs(p.x()[ref.voff] - xo).max() > 2 * xtol   # (further apart than the comparison's tolerance)


@pytest.mark.parametrize("name, N", [c for c in X.EVAL_CASES if c[1] <= X.STEP_REFERENCE_ALL_UP_TO], ids=[f"{n}-N{N}" for n, N in X.EVAL_CASES if N <= X.STEP_REFERENCE_ALL_UP_TO])
def test_lm_step_reference_of_the_default_starts(oracle_mod, name, N):
    """The first iteration of the reference from the jittered start: rows of the term active in every instance, a step taken, and the reference's own backward
    error at rounding level (what the device's bound is a multiple of)."""
    d, X0, xref = X.make_start(oracle_mod, name, N)
    w = X.penalty_weights(name)
    for b in range(X0.shape[0]):
        assert (X.term_values(d, X0[b]) > 0).any()
        o = X.Reference(oracle_mod, d, X0[b], xref[b]).first_iteration(w)
        eta = L.eta_of(o)
        print(f"XUSTEP {name}-N{N} [{b}] passes={o['passes']} accepted={o['accepted']} eta_ref={eta:.3e}")
        assert eta <= L.ORACLE_BOUND, eta
        assert np.abs(o["delta"]).max() > 0


@pytest.mark.parametrize("key", sorted(X.REJECTING), ids=[f"{n}-N{N}" for n, N in sorted(X.REJECTING)])
def test_rejecting_starts_reject(oracle_mod, key):
    """Among the instances that the GPU's LM-step test checks (all three up to 100 grid points, instance 0 beyond) at least one takes two or more passes."""
    name, N = key
    d, X0, xref = X.rejecting_start(oracle_mod, name, N)
    w = X.penalty_weights(name)
    passes, accepted = [], []
    for b in range(X.step_instances(N)):
        ref = X.Reference(oracle_mod, d, X0[b], xref[b])
        _, _, tr = ref.solve(ref.base[ref.voff], 1, w)
        passes.append(tr[0]["inner_passes"])
        accepted.append(tr[0]["accepted"])
        assert (X.term_values(d, X0[b]) > 0).any()
    print(f"XUREJ {name}-N{N} passes={passes} accepted={accepted}")
    assert max(passes) >= 2
    if N > X.STEP_REFERENCE_NONE_ABOVE:
        assert X.STEP_PASSES_LONG[(name, N, True)] == (passes[0], accepted[0])


@pytest.mark.parametrize("key", sorted(k for k in X.STEP_PASSES_LONG if not k[2]), ids=lambda k: f"{k[0]}-N{k[1]}")
def test_recorded_pass_counts_are_the_references(oracle_mod, key):
    """The pass counts that the GPU test takes from STEP_PASSES_LONG at the default start (those of the rejecting starts: test_rejecting_starts_reject)."""
    name, N, _ = key
    d, X0, xref = X.make_start(oracle_mod, name, N)
    ref = X.Reference(oracle_mod, d, X0[0], xref[0])
    _, _, tr = ref.solve(ref.base[ref.voff], 1, X.penalty_weights(name))
    assert X.STEP_PASSES_LONG[key] == (tr[0]["inner_passes"], tr[0]["accepted"])
    assert (X.term_values(d, X0[0]) > 0).any()
