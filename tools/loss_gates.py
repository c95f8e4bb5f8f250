#!/usr/bin/env python
"""Where the gates of tests/test_gpu_losses.py come from (CPU only): for every finite-valued row of tests/loss_cases.py, the error of the
REFERENCE's own fp32 evaluation (oracle.ncc_loss / oracle.grad_loss on fp32 CPU tensors with autograd: ATen, one thread) against the
float64 arbiter (oracle.ncc_explicit_win; oracle.grad_loss in float64), on the inputs the GPU tests use, with upstream gradient 1.

A class is (value regime x window) for NCC and (penalty x value regime) for Grad.  Its gate is 4 x the worst such error over its rows; a
scalar loss is never gated below 4 x 2^-24 (absolute for NCC, |loss| <= 1; relative for Grad); gradients are gated by rel-L2, in the
`same` (I == J), `single` / `single1d` (one voxel) and window-1 classes (true gradient ~0 or ill-conditioned) by max-abs error; the
well-conditioned classes are capped by the fixed gates of tests/test_gpu_parity.py.

    python tools/loss_gates.py > profiles/pr05_loss_gates_cpu.txt

Lines that start with `GATE` carry the constants of the test file (tests/test_cpu_losses.py compares them)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import loss_cases as lc                            # noqa: E402


def emit(key, value):
    print("GATE %-40s %.3e" % (key, value))


def main():
    torch.set_num_threads(1)                       # one summation order
    gates = []
    for cls in lc.NCC_CLASSES:
        loss, grad, rows = lc.ncc_class_gates(cls, lc.TODAY_NCC)
        for row, (el, eg, ea) in rows:
            print("ncc  %-34s class %-16s fp32 reference vs fp64 arbiter: loss %.3e  gradients rel-L2 %.3e  max-abs %.3e" % (row[0], cls, el, eg, ea))
        gates += [("ncc %s loss_abs" % cls, loss), ("ncc %s %s" % (cls, "grad_maxabs" if lc.by_maxabs(rows[0][0]) else "grad"), grad)]
    for cls in lc.GRAD_CLASSES:
        loss, grad, rows = lc.grad_class_gates(cls, lc.TODAY_GRAD)
        for row, (el, eg) in rows:
            print("grad %-34s class %-16s fp32 reference vs fp64: loss (relative) %.3e  gradient rel-L2 %.3e" % (row[0], cls, el, eg))
        gates += [("grad %s loss_rel" % cls, loss), ("grad %s grad" % cls, grad)]
    for key, value in gates:
        emit(key, value)


if __name__ == "__main__":
    main()
