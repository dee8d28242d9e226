"""The factor phase of the fused pass kernel keeps the parent's bits (-m gpu).  Work on factor_body's addressing, selects and option tests may not change a
single floating-point result: every case of tests/factor_bits_cases.py -- the horizons at which each lane mapping of the cyclic reduction can go wrong, a
rejecting start, and the other instantiations of the same code -- is solved once and compared BIT FOR BIT with tests/golden/factor_bits_parent.npz, which
tools/record_factor_bits.py wrote from the build of the commit named inside the file ("parent_commit"): iterates, chi2, status and the handle's counters."""
import os

import numpy as np
import pytest

import factor_bits_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def parent():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "factor_bits_parent.npz")) as z:
        rec = {k: z[k] for k in z.files}
    assert list(rec["case_ids"]) == list(F.CASES) and tuple(rec["counter_names"]) == F.COUNTERS, "the recording does not match the case table: record it again from the parent's build"
    assert len(str(rec["parent_commit"])) >= 7
    return rec


@pytest.mark.parametrize("case_id", list(F.CASES))
def test_factor_phase_keeps_the_parents_bits(parent, case_id):
    got = F.run_case(case_id)
    for k in ("status", "counters", "chi2", "x"):
        want = parent[f"{case_id}/{k}"]
        if k == "counters" and not np.array_equal(got[k], want):
            pytest.fail(f"{case_id}: counters {dict(zip(F.COUNTERS, got[k].tolist()))}, parent {dict(zip(F.COUNTERS, want.tolist()))}")
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (case_id, k)
        same = got[k].view(np.uint8) == want.view(np.uint8)   # bytes: -0.0 against 0.0 and NaN payloads count
        assert same.all(), f"{case_id}: {k} differs from the parent's bits in {int((~same.reshape(got[k].size, -1).all(axis=1)).sum())} of {got[k].size} entries" + \
            (f", max |difference| {float(np.abs(got[k] - want).max()):.3e}" if k in ("x", "chi2") else "")
