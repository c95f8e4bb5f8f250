#!/usr/bin/env python
"""Where the gates of tests/test_gpu_step_tail.py come from (CPU only): for every case of tests/step_tail_cases.py, the error of the
REFERENCE's own fp32 evaluation of the operation on the CPU (torch.optim.Adam, oracle.mse_loss / dice_loss and their autograd, the
oracle's training loop) against the float64 arbiter, on the inputs the GPU tests use.  A gate is 4 x the largest such error over the
cases it covers; a scalar fp32 result is never gated below 4 x 2^-24 relative (half an ulp).

    python tools/step_tail_gates.py > profiles/pr03_step_tail_gates_cpu.txt

Lines that start with `GATE` carry the constants of the test file (tests/test_cpu_step_tail.py compares them)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import step_tail_cases as sc                       # noqa: E402

HALF_ULP = 2.0 ** -24
MARGIN = 4.0


def emit(key, value):
    print("GATE %-64s %.3e" % (key, value))


def adam():
    worst = {}
    for h, hyper in enumerate(sc.ADAM_HYPER):
        for n in sc.ADAM_N:
            p0, g, _, _ = sc.adam_arrays(n)
            for gs in sc.ADAM_GSCALE:
                r32 = sc.adam_torch(p0, g, hyper, gs, torch.float32, check=sc.ADAM_CHECK)
                r64 = sc.adam_torch(p0, g, hyper, gs, torch.float64, check=sc.ADAM_CHECK)
                for s in sc.ADAM_CHECK:
                    e = sc.adam_errors(r32[s], r64[s], hyper[0])
                    print("adam hyper%d n=%-6d gscale=%.4f step %2d  fp32 reference vs fp64: max|dp|/lr %.3e  exp_avg %.3e  exp_avg_sq %.3e"
                          % ((h, n, gs, s) + e))
                    worst[(h, s)] = [max(a, b) for a, b in zip(worst.get((h, s), (0.0, 0.0, 0.0)), e)]
    L = sc.ADAM_LATE
    p0, g, m0, v0 = sc.adam_arrays(L["n"], L["steps"], late=True)
    hyper, steps = sc.ADAM_HYPER[L["hyper"]], tuple(range(1, L["steps"] + 1))
    r32 = sc.adam_torch(p0, g, hyper, L["gscale"], torch.float32, m0, v0, L["start"], steps)
    r64 = sc.adam_torch(p0, g, hyper, L["gscale"], torch.float64, m0, v0, L["start"], steps)
    for s in steps:
        e = sc.adam_errors(r32[s], r64[s], hyper[0])
        print("adam late start (counter %d) n=%d step %d  fp32 reference vs fp64: max|dp|/lr %.3e  exp_avg %.3e  exp_avg_sq %.3e"
              % ((L["start"], L["n"], s) + e))
        worst[("late", s)] = list(e)
    for (h, s), e in worst.items():
        for what, v in zip(("p_over_lr", "exp_avg", "exp_avg_sq"), e):
            emit("adam %s step%d %s" % (h if h == "late" else "hyper%d" % h, s, what), MARGIN * v)


def trajectory():
    l32, t32 = sc.traj_oracle(torch.float32)
    l64, t64 = sc.traj_oracle(torch.float64)
    dl = max(abs(a - b) for a, b in zip(l32, l64))
    floor = MARGIN * HALF_ULP * max(abs(v) for v in l64)
    print("trajectory losses fp32 %s" % " ".join("%.8f" % v for v in l32))
    print("trajectory losses fp64 %s" % " ".join("%.8f" % v for v in l64))
    print("trajectory loss: fp32 oracle vs fp64 oracle, largest |difference| over %d steps %.3e (floor 4 x 2^-24 x |loss| = %.3e)" % (sc.TRAJ_K, dl, floor))
    emit("trajectory loss_abs", max(MARGIN * dl, floor))
    assert len(t64) == 24
    for name in t64:
        e = tuple(sc.rel_l2(a, b) for a, b in zip(t32[name], t64[name]))
        print("trajectory %-40s fp32 oracle vs fp64 oracle after %d steps: p_K - p_0 %.3e  exp_avg %.3e  exp_avg_sq %.3e" % ((name, sc.TRAJ_K) + e))
        assert max(e) < 1e-2, "the reference itself is no yardstick for %s: %s" % (name, e)
        for what, v in zip(("dp", "exp_avg", "exp_avg_sq"), e):
            emit("trajectory %s %s" % (name, what), MARGIN * v)


def mse():
    wl = wg = 0.0
    for n in sc.MSE_N:
        a, b = sc.mse_arrays(n)
        l32, ga32, gb32 = sc.mse_reference(a, b, torch.float32)
        l64, ga64, gb64 = sc.mse_reference(a, b, torch.float64)
        el, eg = abs(l32 - l64) / abs(l64), max(sc.rel_l2(ga32, ga64), sc.rel_l2(gb32, gb64))
        print("mse n=%-8d fp32 reference vs fp64: loss (relative) %.3e  gradients %.3e" % (n, el, eg))
        wl, wg = max(wl, el), max(wg, eg)
    emit("mse loss_rel", max(MARGIN * wl, MARGIN * HALF_ULP))
    emit("mse grad", MARGIN * wg)


def dice():
    wl = wg = lmax = 0.0
    for case in sc.DICE_CASES:
        yt, yp = sc.dice_arrays(case)
        if case[1] > 2:
            sub = (yt[:, 2].astype(np.float64) + yp[:, 2].astype(np.float64)).sum(axis=1)
            assert 0.0 < sub.min() and sub.max() < sc.DICE_CLAMP, sub
            assert float(np.minimum(yt[:, 2], yp[:, 2]).min()) > 0.0
            print("dice B=%d C=%d V=%d channel 2 sums %s (clamp %.0e)" % (case + (" ".join("%.6e" % v for v in sub), sc.DICE_CLAMP)))
        l32, gt32, gp32 = sc.dice_reference(yt, yp, torch.float32)
        l64, gt64, gp64 = sc.dice_reference(yt, yp, torch.float64)
        el, eg = abs(l32 - l64), max(sc.rel_l2(gt32, gt64), sc.rel_l2(gp32, gp64))
        print("dice B=%d C=%d V=%-8d fp32 reference vs fp64: loss (absolute) %.3e  gradients %.3e" % (case + (el, eg)))
        wl, wg, lmax = max(wl, el), max(wg, eg), max(lmax, abs(l64))
    emit("dice loss_abs", max(MARGIN * wl, MARGIN * HALF_ULP * lmax))
    emit("dice grad", MARGIN * wg)


def main():
    torch.set_num_threads(1)                       # one summation order
    adam()
    mse()
    dice()
    trajectory()


if __name__ == "__main__":
    main()
