#!/usr/bin/env python
"""Where the gates of tests/test_gpu_eval.py come from (CPU only): for every Jacobian row of tests/eval_cases.py, the error of the
REFERENCE's own formula (voxelmorph/py/utils.py:491-516: np.gradient of disp + grid, cofactor expansion) evaluated on float32 against
the same formula in float64, on the inputs the GPU tests use.

A class is (field regime, dimensionality).  The gate of vxm_jacdet3d / vxm_jacdet2d's determinant is 4 x the worst such error over the
rows of its class, in rel-L2 and in max-abs.  The number of non-positive determinants cannot be exact where |det| is below the rounding
error: with m = 8 x the reference's fp32 max-abs error of the row, the kernel's count has to lie in [#(det64 < -m), #(det64 <= m)], and
the inputs are chosen so that at most 0.1 % of a row's voxels have |det64| <= m (printed as `undecided`).

    python tools/eval_gates.py > profiles/pr06_eval_gates_cpu.txt

Lines that start with `GATE` carry the constants of the test file (tests/test_cpu_eval.py compares them)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import eval_cases as ec                            # noqa: E402


def main():
    gates = []
    for cls in ec.JAC_CLASSES:
        rel, mabs, rows = ec.jac_class_gates(cls)
        for row, (er, ea) in rows:
            d64 = ec.jacdet64(ec.jac_arrays(row))
            m = ec.BAND * ea
            lo, hi = ec.count_band(d64, m)
            print("jac %-14s class %-12s fp32 reference vs fp64: rel-L2 %.3e  max-abs %.3e | min |det64| %.3e  det64 <= 0: %s of %d  "
                  "band m %.3e: count in [%s, %s], undecided %.5f %%" % (
                      row[0], cls, er, ea, np.abs(d64).min(), (d64 <= 0).reshape(d64.shape[0], -1).sum(1).tolist(), d64[0].size, m,
                      lo.tolist(), hi.tolist(), 100.0 * (np.abs(d64) <= m).mean()))
            gates.append(("jac %s band" % row[0], m))
        gates += [("jac %s rel_l2" % cls, rel), ("jac %s max_abs" % cls, mabs)]
    for key, value in gates:
        print("GATE %-40s %.3e" % (key, value))


if __name__ == "__main__":
    main()
