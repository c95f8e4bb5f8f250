#!/usr/bin/env python
"""Where the gates of tests/test_gpu_affine.py come from (CPU only).  For every noise row and variant of tests/affine_cases.py, and the
lattice row, the error against the float64 arbiter (affine_cases.shift_arbiter) of the PLAIN fp32 evaluation of the same definition: torch
float32 on the CPU, one thread -- the pinned chain q = (i - c) + w, x = (((M0 q0) + (M1 q1)) + (M2 q2)) + t, shift = x - (i - c), and
autograd's fp32 backward for the gradient of the right-composed field.  Each gate is 4 x the largest rel-L2 error of its class over the
table: shift, shift-gw.  Also printed: the round-trip bound of the inversion test, 1.5 x the round-trip interpolation error of the float64
arbiters on the same inputs (oracle.warp_arbiter on the float32 field of shift_arbiter).

    python tools/affine_gates.py            # one line per row and variant, then the gates
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import affine_cases as ac                          # noqa: E402
from oracle import vxm_oracle as orc               # noqa: E402


def fp32_shift(mat, flow, B, size, shift_center=True):
    m = mat.expand(B, 3, 4)
    mesh, q = [], []
    for k, S in enumerate(size):
        shp = [1, 1, 1, 1]
        shp[k + 1] = S
        g = (torch.arange(S, dtype=torch.float32) - (0.5 * (S - 1) if shift_center else 0.0)).reshape(shp)
        mesh.append(g)
        qk = g.expand((B,) + tuple(size))
        q.append(qk + flow[:, k] if flow is not None else qk)
    out = []
    for a in range(3):
        e = [m[:, a, k].reshape(B, 1, 1, 1) for k in range(4)]
        out.append(((((e[0] * q[0]) + (e[1] * q[1])) + (e[2] * q[2])) + e[3]) - mesh[a])
    return torch.stack(out, dim=1)


def shift_errors(arr, vname):
    mat, flow = ac.variant(arr, vname)
    B = arr["gshift"].shape[0] if flow is not None else mat.shape[0]
    f = torch.from_numpy(flow).requires_grad_() if flow is not None else None
    sh = fp32_shift(torch.from_numpy(mat), f, B, arr["size"])
    g = arr["gshift"][:B]
    if f is not None:
        sh.backward(torch.from_numpy(g))
    s64, gf64 = ac.shift_arbiter(mat, arr["size"], True, flow, g)
    return ac.rel_l2(sh.detach().numpy(), s64), ac.rel_l2(f.grad.numpy(), gf64) if f is not None else 0.0


def roundtrip_error():
    vol, m, mi = ac.roundtrip_arrays()
    size, margin = ac.ROUNDTRIP[1], ac.ROUNDTRIP[3]
    once, _, _ = orc.warp_arbiter(vol, ac.shift_arbiter(m, size)[0].astype(np.float32))
    back, _, _ = orc.warp_arbiter(once.astype(np.float32), ac.shift_arbiter(mi, size)[0].astype(np.float32))
    return ac.rel_l2(ac.interior(back, margin), ac.interior(vol, margin))


def main():
    torch.set_num_threads(1)                       # one summation order
    rows = [(r[0], ac.noise_arrays(r)) for r in ac.NOISE] + [(ac.LATTICE[0], ac.lattice_arrays())]
    worst = [0.0, 0.0]
    for name, arr in rows:
        for v in ac.VARIANTS:
            e = shift_errors(arr, v)
            print("%-18s %-13s fp32 vs fp64 arbiter: shift %.3e  gw %.3e" % ((name, v) + e))
            worst = [max(a, b) for a, b in zip(worst, e)]
    print("affine shift largest: shift %.3e gw %.3e  -> gates (x4): %.2e %.2e" % (tuple(worst) + tuple(4 * v for v in worst)))
    e = roundtrip_error()
    print("round trip %s, %g degrees, interior margin %d: the arbiters' own interpolation error %.4e -> bound (x1.5): %.3e"
          % (ac.ROUNDTRIP[0], ac.ROUNDTRIP[2], ac.ROUNDTRIP[3], e, 1.5 * e))


if __name__ == "__main__":
    main()
