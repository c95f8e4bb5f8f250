#!/usr/bin/env python
"""Where the gates of tests/test_gpu_mi.py come from (CPU only): for every row of tests/mi_cases.py, the error of the fp32 reference
formulation of the mutual information loss (the definition in plain ATen ops with autograd, float32, one thread) against the float64
arbiter (the same ops in float64), on the inputs the GPU tests use, with the row's upstream gradient.

A class is a value regime.  Its gate is 4 x the worst such error over its rows: the loss by absolute error (the tests never gate it below
4 x 2^-24 x max(1, |loss|)), the gradients by rel-L2 -- in the classes const_true, const_pred and single (true gradient ~0) by absolute L2.

    python tools/mi_gates.py > profiles/pr08_mi_gates_cpu.txt

Lines that start with `GATE` carry the constants the tests read (tests/test_cpu_mi.py recomputes them)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import mi_cases as mc                              # noqa: E402


def main():
    torch.set_num_threads(1)                       # one summation order
    gates = []
    for cls in mc.CLASSES:
        gl, gg, rows = mc.class_gates(cls)
        for name, el, rel, ab in rows:
            l64, _, _ = mc.arbiter(mc.BY_NAME[name])
            norm = mc.errors(mc.BY_NAME[name], *mc.arbiter(mc.BY_NAME[name]))[3]
            print("mi %-26s class %-11s arbiter: loss %+.6e  gradient norm %.3e | fp32 reference formulation vs arbiter: loss %.3e  "
                  "gradients rel-L2 %.3e  abs-L2 %.3e" % (name, cls, l64, norm, el, rel, ab))
        kl, kg = mc.gate_keys(cls)
        gates += [(kl, gl), (kg, gg)]
    for key, value in gates:
        print("GATE %-28s %.3e" % (key, value))


if __name__ == "__main__":
    main()
