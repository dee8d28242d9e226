"""CPU twin of test_gpu_stage_function_eq.py's iterate and LM-step tests: the reference they compare against (stage_function_eq_cases.Reference --
oracle.GenericProblem over the OCP oracle's rows plus the state-control equality's rows from the host evaluator) is built and solved here without a device, and
what makes the GPU tests meaningful is asserted: the term's rows are non-zero at every start, the rejecting starts reject, and the derived tolerances of
every case -- max(the ledger's defaults, 4 x the oracle's own spread over starts one ulp away) -- stay at or below the hard gate 1e-5 on x and on relative
chi2 for every iteration count listed, so that the GPU comparison cannot go vacuous."""
import numpy as np
import pytest

import lm_step_check as L
import stage_function_eq_cases as E
from control_box_rst_amd import capi


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


@pytest.mark.parametrize("name, N, start, iterations", E.ITERATE_CASES, ids=E.ITERATE_IDS)
def test_iterate_reference_has_nonzero_rows_and_tolerances_inside_the_hard_gate(oracle_mod, name, N, start, iterations):
    d, X0, xref = E.make_start(oracle_mod, name, N, **start)
    w = E.penalty_weights(name)
    ref = E.Reference(oracle_mod, d, X0[0], xref[0])
    e0 = E.term_values(d, X0[0])
    assert np.all(e0 != 0.0), "the term's rows are non-zero at the start"
    xtol = None
    for k in iterations:
        xo, co, xtol, ctol = ref.iterate_with_spread(k, w)
        print(f"EQREF {name}-N{N} k={k} chi2={co:.9e} xtol={xtol:.3e} ctol={ctol:.3e}")
        assert np.all(np.isfinite(xo)) and np.isfinite(co)
        assert xtol <= E.HARD_X and ctol <= E.HARD_CHI2, (name, k, xtol, ctol)
    # the term matters: the same solve without its rows ends elsewhere (further apart than twice the comparison's tolerance)
    x_without, _, _ = _solve_without_term(oracle_mod, d, X0[0], xref[0], iterations[-1], w)
    assert np.abs(x_without - xo).max() > 2 * xtol


def _solve_without_term(O, d, x_start, xref, k, w):
    """the same reference construction on the descriptor without the equality term (a state-control inequality next to it stays)"""
    d0 = E.without_term(d)
    if not d0.stage_ineq_state_control:
        p = O.OracleProblem(d0)
        p.set_data(x_start, xref=xref)
        _, chi2, tr = p.solve(capi.default_lm_opts(k, *w), new_run=True)
        return p.x()[p.param_offsets().astype(np.int64)], chi2, tr
    import stage_function_xu_cases as XU
    ref = XU.Reference(O, d0, x_start, xref)
    return ref.solve(ref.base[ref.voff], k, w)


STEP_SHORT = [c for c in E.EVAL_CASES if c[1] <= E.STEP_REFERENCE_ALL_UP_TO]


@pytest.mark.parametrize("name, N", STEP_SHORT, ids=[f"{n}-N{N}" for n, N in STEP_SHORT])
def test_lm_step_reference_of_the_default_starts(oracle_mod, name, N):
    """The first iteration of the reference from the jittered start: the term's rows non-zero in every instance, a step taken, and the reference's own backward
    error at rounding level (what the device's bound is a multiple of)."""
    d, X0, xref = E.make_start(oracle_mod, name, N)
    w = E.penalty_weights(name)
    for b in range(X0.shape[0]):
        assert np.all(E.term_values(d, X0[b]) != 0.0)
        o = E.Reference(oracle_mod, d, X0[b], xref[b]).first_iteration(w)
        eta = L.eta_of(o)
        print(f"EQSTEP {name}-N{N} [{b}] passes={o['passes']} accepted={o['accepted']} eta_ref={eta:.3e}")
        assert eta <= L.ORACLE_BOUND, eta
        assert np.abs(o["delta"]).max() > 0


@pytest.mark.parametrize("key", sorted(E.REJECTING), ids=[f"{n}-N{N}" for n, N in sorted(E.REJECTING)])
def test_rejecting_starts_reject(oracle_mod, key):
    """Among the instances that the GPU's LM-step test checks (all three up to 100 grid points, instance 0 beyond) at least one takes two or more passes."""
    name, N = key
    d, X0, xref = E.rejecting_start(oracle_mod, name, N)
    w = E.penalty_weights(name)
    passes, accepted = [], []
    for b in range(E.step_instances(N)):
        ref = E.Reference(oracle_mod, d, X0[b], xref[b])
        _, _, tr = ref.solve(ref.base[ref.voff], 1, w)
        passes.append(tr[0]["inner_passes"])
        accepted.append(tr[0]["accepted"])
        assert np.all(E.term_values(d, X0[b]) != 0.0)
    print(f"EQREJ {name}-N{N} passes={passes} accepted={accepted}")
    assert max(passes) >= 2
    if N > E.STEP_REFERENCE_NONE_ABOVE:
        assert E.STEP_PASSES_LONG[(name, N, True)] == (passes[0], accepted[0])


@pytest.mark.parametrize("key", sorted(k for k in E.STEP_PASSES_LONG if not k[2]), ids=lambda k: f"{k[0]}-N{k[1]}")
def test_recorded_pass_counts_are_the_references(oracle_mod, key):
    """The pass counts that the GPU test takes from STEP_PASSES_LONG at the default start (those of the rejecting starts: test_rejecting_starts_reject)."""
    name, N, _ = key
    d, X0, xref = E.make_start(oracle_mod, name, N)
    ref = E.Reference(oracle_mod, d, X0[0], xref[0])
    _, _, tr = ref.solve(ref.base[ref.voff], 1, E.penalty_weights(name))
    assert E.STEP_PASSES_LONG[key] == (tr[0]["inner_passes"], tr[0]["accepted"])
    assert np.all(E.term_values(d, X0[0]) != 0.0)
