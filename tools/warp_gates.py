#!/usr/bin/env python
"""Where the warp gates of tests/test_gpu_warp.py come from (CPU only): for every finite-valued row of tests/warp_cases.py, the error of the
REFERENCE's own fp32 evaluation (oracle.spatial_transformer / oracle.vecint in float32: ATen's forward and autograd, one thread) against the
float64 arbiter (oracle.warp_arbiter / vecint_arbiter), on the inputs the GPU tests use.  Each gate is 4 x the largest value over the
table, separately for 3-D and 2-D: forward rel-L2, gsrc rel-L2, gflow rel-L2, the adjoint gap |<out, g> - <src, gsrc>| / (|out| |g|).

    python tools/warp_gates.py            # prints one line per row and the gates
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import resize_cases as rc                          # noqa: E402
import warp_cases as wc                            # noqa: E402
from oracle import vxm_oracle as orc               # noqa: E402


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def warp_errors(src, flow, gout):
    s, f = torch.from_numpy(src).requires_grad_(), torch.from_numpy(flow).requires_grad_()
    out = orc.spatial_transformer(s, f)
    out.backward(torch.from_numpy(gout))
    o64, gs64, gf64 = orc.warp_arbiter(src, flow, gout)
    return (rel_l2(out.detach().numpy(), o64), rel_l2(s.grad.numpy(), gs64), rel_l2(f.grad.numpy(), gf64),
            rc.adjoint_gap(out.detach().numpy(), gout, src, s.grad.numpy()))


def vecint_errors(vec, gout, nsteps):
    """forward: the largest error of any one step (the reference's field k + 1 against the arbiter's evaluation of the step on its field k)"""
    v = torch.from_numpy(vec).requires_grad_()
    out = orc.vecint(v, nsteps)
    out.backward(torch.from_numpy(gout))
    _, g64, outs = orc.vecint_arbiter(vec, nsteps, gout)
    f = v.detach() * (1.0 / 2 ** nsteps)
    fwd = 0.0
    for k in range(nsteps):
        f = f + orc.spatial_transformer(f, f)
        fwd = max(fwd, rel_l2(f.numpy(), outs[k]))
    assert torch.equal(f, out.detach())
    return fwd, rel_l2(v.grad.numpy(), g64)


def fullsize(fl, full):
    """ResizeTransform(1 / 2) of the reference (layers.py:91-94: x2, then the align_corners interpolation) onto the image's extents"""
    mode = "trilinear" if len(full) == 3 else "bilinear"
    return torch.nn.functional.interpolate(2.0 * torch.from_numpy(fl), size=full, mode=mode, align_corners=True).numpy()


def main():
    torch.set_num_threads(1)                       # one summation order
    rows = {"3-D": [], "2-D": []}
    for case in wc.CASES:
        if case[4] == "far":                       # non-finite displacements: judged by its non-finite SET and on the finite voxels, under these gates
            continue
        rows["%d-D" % len(case[1])].append((case[0], wc.arrays(case)))
    for row in wc.FUSED:
        img, fl, gout = wc.fused_arrays(row)
        rows["3-D"].append((row[0], (img, fullsize(fl, row[2]), gout)))
    for what in ("3-D", "2-D"):
        w = [0.0] * 4
        for name, (src, flow, gout) in rows[what]:
            e = warp_errors(src, flow, gout)
            print("%-22s fp32 reference vs fp64 arbiter: forward %.3e  gsrc %.3e  gflow %.3e  adjoint gap %.3e" % ((name,) + e))
            w = [max(a, b) for a, b in zip(w, e)]
        print("%s warp largest: forward %.3e gsrc %.3e gflow %.3e adjoint %.3e  -> gates (x4): %.2e %.2e %.2e %.2e"
              % ((what,) + tuple(w) + tuple(4 * v for v in w)))
    for dims, _ in wc.VECINT:
        w = [0.0] * 2
        for nsteps in wc.VECINT_STEPS:
            vec, gout = wc.vecint_arrays(dims, nsteps)
            e = vecint_errors(vec, gout, nsteps)
            print("vecint %-10s nsteps %d fp32 reference vs fp64 arbiter: forward %.3e  backward %.3e" % (("x".join(map(str, dims)), nsteps) + e))
            w = [max(a, b) for a, b in zip(w, e)]
        print("%d-D vecint largest: forward %.3e backward %.3e  -> gates (x4): %.2e %.2e" % ((len(dims),) + tuple(w) + tuple(4 * v for v in w)))


if __name__ == "__main__":
    main()
