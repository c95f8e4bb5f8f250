#!/usr/bin/env python
"""Where the gates of tests/test_gpu_prob.py come from (CPU only).  For every row of tests/prob_cases.py, both prior weights and both upstream
gradients, and the lattice row, the error against the float64 arbiters (prob_cases.kl_arbiter / sample_arbiter) of the PLAIN fp32
evaluation of the same definition: torch float32 on the CPU, one thread (prob_cases.kl_torch / sample_torch and autograd's fp32 backward).
Each gate is 4 x the largest error of its class over the table -- the KL loss (relative error of one number), the KL gradient of the mean
and of log sigma^2, the sample and the sample's gradient of log sigma^2 (rel-L2) -- and the loss gate is never below 2^-23: the loss is one
fp32 number.

    python tools/prob_gates.py            # one line per row and variant, then the gates
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import prob_cases as pc                            # noqa: E402


def kl_errors(params, lam, g):
    p = torch.from_numpy(params).requires_grad_()
    loss = pc.kl_torch(p, lam, torch.float32)
    loss.backward(torch.tensor(g, dtype=torch.float32))
    l64, gp64 = pc.kl_arbiter(params, lam, g)
    gp = p.grad.numpy()
    return abs(float(loss.detach()) - l64) / abs(l64), pc.rel_l2(gp[:, :3], gp64[:, :3]), pc.rel_l2(gp[:, 3:], gp64[:, 3:])


def sample_errors(arr):
    p = torch.from_numpy(arr["params"]).requires_grad_()
    z = pc.sample_torch(p, torch.from_numpy(arr["eps"]))
    z.backward(torch.from_numpy(arr["gz"]))
    z64, gp64 = pc.sample_arbiter(arr["params"], arr["eps"], arr["gz"])
    return pc.rel_l2(z.detach().numpy(), z64), pc.rel_l2(p.grad.numpy()[:, 3:], gp64[:, 3:])


def gates():
    """{class: gate} over the table (what the GPU tests import when the recorded file is absent is NOT this: they carry the numbers)"""
    torch.set_num_threads(1)                       # one summation order
    worst = dict.fromkeys(pc.GATE_CLASSES, 0.0)
    lines = []
    for row in pc.ROWS:
        arr = pc.row_arrays(row)
        for lam in pc.LAMBDAS:
            for g in pc.UPSTREAM:
                e = kl_errors(arr["params"], lam, g)
                lines.append("%-16s lambda %4g g %5g  fp32 vs fp64 arbiter: loss %.3e  gmu %.3e  gls %.3e" % ((row[0], lam, g) + e))
                for k, v in zip(pc.GATE_CLASSES[:3], e):
                    worst[k] = max(worst[k], v)
        e = sample_errors(arr)
        lines.append("%-16s sample               fp32 vs fp64 arbiter: z %.3e  gls %.3e" % ((row[0],) + e))
        for k, v in zip(pc.GATE_CLASSES[3:], e):
            worst[k] = max(worst[k], v)
    out = {k: 4.0 * v for k, v in worst.items()}
    out["kl_loss"] = max(out["kl_loss"], pc.LOSS_GATE_FLOOR)
    return worst, out, lines


def main():
    worst, out, lines = gates()
    print("\n".join(lines))
    lat = pc.lattice_arrays()
    p = torch.from_numpy(lat["params"])
    l32 = float(pc.kl_torch(p, lat["lam"], torch.float32))
    l64, _ = pc.kl_arbiter(lat["params"], lat["lam"])
    print("%-16s lambda %4g  arbiter %.17g, rounded to fp32 %.9g; plain fp32 torch gives %.9g" % (pc.LATTICE[0], lat["lam"], l64, np.float32(l64), l32))
    for k in pc.GATE_CLASSES:
        print("largest %-10s %.3e  -> gate (x4%s): %.3e" % (k, worst[k], ", floor 2^-23" if k == "kl_loss" else "", out[k]))


if __name__ == "__main__":
    main()
