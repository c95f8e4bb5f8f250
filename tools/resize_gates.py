#!/usr/bin/env python
"""Where the resize gates of tests/test_gpu_parity.py come from (CPU only): for every case of tests/resize_cases.py, the error of the
REFERENCE's own fp32 evaluation (oracle.resize_transform in float32: ATen's forward and autograd) against the float64 arbiter, on the
inputs the GPU tests use.  The gates are 4 x the largest value over the table: forward rel-L2, backward rel-L2, adjoint gap.

    python tools/resize_gates.py            # prints one line per case and the three gates
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import resize_cases as rc                          # noqa: E402
from oracle import vxm_oracle as orc               # noqa: E402


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def evaluate(x, g, vel, dtype):
    xt = torch.from_numpy(x).to(dtype).requires_grad_()
    y = orc.resize_transform(xt, vel)
    y.backward(torch.from_numpy(g).to(dtype))
    return y.detach().numpy(), xt.grad.numpy()


def errors(x, g, vel):
    y32, gx32 = evaluate(x, g, vel, torch.float32)
    y64, gx64 = evaluate(x, g, vel, torch.float64)
    return rel_l2(y32, y64), rel_l2(gx32, gx64), rc.adjoint_gap(y32, g, x, gx32)


def main():
    torch.set_num_threads(1)                       # one summation order
    worst = {}
    for what, rows in (("3-D", [(c[0], c[2], rc.arrays(c)) for c in rc.CASES]),
                       ("2-D", [("%dx%d_vel%.3g" % (s + (v,)), v, rc.planar_arrays(s, v)) for s in rc.PLANAR_SHAPES for v in rc.PLANAR_VELS])):
        w = [0.0, 0.0, 0.0]
        for name, vel, (x, g) in rows:
            if g is None:
                print("%-24s no output (the reference raises)" % name)
                continue
            e = errors(x, g, vel)
            print("%-24s fp32 reference vs fp64: forward %.3e  backward %.3e  adjoint gap %.3e" % ((name,) + e))
            w = [max(a, b) for a, b in zip(w, e)]
        worst[what] = w
        print("%s largest: forward %.3e backward %.3e adjoint %.3e  -> gates (x4): %.2e %.2e %.2e" % ((what,) + tuple(w) + tuple(4 * v for v in w)))


if __name__ == "__main__":
    main()
