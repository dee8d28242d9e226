"""Record tests/golden/factor_bits_parent.npz: the bits -- iterates, chi2, status, counters -- that the library of a PARENT commit gives on the cases of
tests/factor_bits_cases.py.  tests/test_gpu_factor_bits.py compares the tree's own build against this file bit for bit, so the file is produced by the parent's
build, never by the code under test:

    python tools/record_factor_bits.py --commit <hash of the commit the loaded library was built from> [--out tests/golden/factor_bits_parent.npz]

with that library in place (or named by CORBO_HIP_LIB).  Needs the GPU.  The hash is stored inside the file ("parent_commit")."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

import factor_bits_cases as F
from control_box_rst_amd import capi


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", required=True, help="hash of the commit whose build is loaded")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "factor_bits_parent.npz"))
    a = ap.parse_args()
    out = {"parent_commit": np.array(a.commit), "counter_names": np.array(F.COUNTERS), "case_ids": np.array(list(F.CASES))}
    for cid in F.CASES:
        first, again = F.run_case(cid), F.run_case(cid)
        for k, v in first.items():   # (a case that does not repeat its own bits cannot be a yardstick)
            assert np.array_equal(v, again[k]), f"{cid}: {k} differs between two solves of the same library"
            out[f"{cid}/{k}"] = v
        c = dict(zip(F.COUNTERS, first["counters"].tolist()))
        print(f"{cid}: chi2[0] = {first['chi2'][0]!r}, accepted {c['accepted_steps']}, rejected {c['rejected_steps']}, factorisations {c['factorizations']}, plain_kernel {c['plain_kernel']}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(f"{a.out}: {len(F.CASES)} cases from {capi.lib_path()} (commit {a.commit}), {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
