#!/usr/bin/env python
"""Where the gates of tests/test_gpu_synth.py come from (CPU only).  For every row of tests/synth_cases.py the error against the float64
arbiters (synth_cases.blur_arbiter / finish_arbiter) of the PLAIN fp32 evaluation of the same definition: torch float32 on the CPU, one
thread (synth_cases.blur_torch: three conv3d calls; finish_torch: exp, mul, clamp, amin, amax, sub, div, pow).  The blur runs at every
tap count of the table with Gaussian taps that differ per sample and per axis, the finish in every variant of the table (a bias field,
gamma 0.5 and 1.7, inputs that clip at both ends).  Each gate is 4 x the largest rel-L2 error of its class over the rows.  The draw and the
one-hot have no gate: a multiply and an add, and 0.0 / 1.0, reproduce bit for bit.

    python tools/synth_gates.py            # one line per row and case, then the gates
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import synth_cases as sc                           # noqa: E402


def gates():
    torch.set_num_threads(1)                       # one summation order
    worst = dict.fromkeys(sc.GATE_CLASSES, 0.0)
    lines = []
    for row in sc.ROWS:
        a = sc.row_arrays(row)
        for T in sc.BLUR_T:
            taps = sc.taps_for(a["sigma"], T)
            with torch.no_grad():
                got = sc.blur_torch(torch.from_numpy(a["x"]), torch.from_numpy(taps)).numpy()
            e = sc.rel_l2(got, sc.blur_arbiter(a["x"], taps))
            lines.append("%-18s blur   T %2d          fp32 vs fp64 arbiter: %.3e" % (row[0], T, e))
            worst["blur"] = max(worst["blur"], e)
        for variant in sc.FINISH_VARIANTS:
            x, lb, gamma = sc.finish_inputs(a, variant)
            with torch.no_grad():
                got = sc.finish_torch(torch.from_numpy(x), torch.from_numpy(lb), torch.from_numpy(gamma)).numpy()
            e = sc.rel_l2(got, sc.finish_arbiter(x, lb, gamma))
            lines.append("%-18s finish %-13s fp32 vs fp64 arbiter: %.3e" % (row[0], variant, e))
            worst["finish"] = max(worst["finish"], e)
    return worst, {k: 4.0 * v for k, v in worst.items()}, lines


def main():
    worst, out, lines = gates()
    print("\n".join(lines))
    for k in sc.GATE_CLASSES:
        print("largest %-8s %.3e  -> gate (x4): %.3e" % (k, worst[k], out[k]))


if __name__ == "__main__":
    main()
