#!/usr/bin/env python
"""Time the affine path (voxelmorph_amd/csrc/affine.hip) at 160 x 192 x 224, C = 1, B = 1, with HIP events: a rotation by 10 degrees plus
a 3-voxel translation, alone and right-composed with a smooth 5-voxel field (the regime of bench.py's trained-flow extra: a 5 / 3 / 4-voxel
translation plus a slowly varying part).  Timed:

  * the matrix as a dense field:        the shift kernel against the ATen formulation (the dense shift by torch.matmul on a resident mesh),
                                        forward, and forward + backward for the gradient of the right-composed field
  * the matrix applied to a volume:     shift kernel + the dense warp kernel (one interpolation) against the ATen formulation on the same
                                        device: torch.matmul shift, then the reference's SpatialTransformer op chain (add, normalise, permute,
                                        grid_sample; the grid is a resident buffer, as in the reference)
  * the dense warp kernel alone on the same field: the yardstick of what the second launch costs

Each candidate is warmed up, then timed in windows of `--reps` back-to-back calls between two events; candidates are ALTERNATED over
`--windows` windows and the median, minimum and maximum window are printed (per call), with the algorithmic bytes (every tensor read or
written once) over the median against the 6.29 TB/s measured for HBM.  Before anything is timed the kernel path is compared with the
ATen formulation on the timed inputs.

    python tools/affine_time.py > profiles/pr10_affine_time.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM = 6.29e12                 # B/s, measured


def window(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps            # us per call


def race(title, cands, args):
    """cands: [(name, fn, algorithmic bytes or None)]"""
    for _, fn, _ in cands:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in cands]
    for _ in range(args.windows):                            # alternate: every candidate sees the same neighbours on the machine
        for t, (_, fn, _) in zip(times, cands):
            t.append(window(fn, args.reps))
    print(title)
    base = float(np.median(times[0]))
    for t, (name, _, nbytes) in zip(times, cands):
        m = float(np.median(t))
        bw = "" if nbytes is None else " | %6.0f GB/s of the algorithmic bytes = %4.1f %% of HBM" % (nbytes / m * 1e-3, 100 * nbytes / (m * 1e-6) / HBM)
        print("    %-58s %9.1f us (min %9.1f max %9.1f) | %5.2fx the first line%s" % (name, m, min(t), max(t), m / base, bw))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shape", type=int, nargs=3, default=(160, 192, 224))
    p.add_argument("--reps", type=int, default=10, help="calls per timed window")
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("affine_time.py measures on an MI355X; no HIP device found (there is no CPU fallback and no CPU timing)")

    import voxelmorph_amd as vxm
    from voxelmorph_amd.torch import functional as VF
    import torch.nn.functional as F

    vol = tuple(args.shape)
    V = int(np.prod(vol))
    scan = np.load(os.path.join(ROOT, "tests", "golden", "real_scan_u8.npz"), allow_pickle=False)["vol_u8"].astype(np.float32) / 255.0
    assert all(v <= s for v, s in zip(vol, scan.shape)), "the scan is %s" % (scan.shape,)
    src = torch.from_numpy(np.ascontiguousarray(scan[:vol[0], :vol[1], :vol[2]])).cuda()[None, None]
    t = np.deg2rad(10.0)
    m = np.eye(4)[:3]
    m[1, 1], m[1, 2], m[2, 1], m[2, 2] = np.cos(t), -np.sin(t), np.sin(t), np.cos(t)
    m[:, 3] = (3.0, -3.0, 3.0)
    mat = torch.from_numpy(m[None].astype(np.float32)).cuda()
    z, y, x = np.meshgrid(*[np.linspace(0, 2 * np.pi, s) for s in vol], indexing="ij")
    field = np.stack([5.0 + 0.5 * np.sin(y + 0.5 * x), 3.0 + 0.5 * np.cos(z - x), 4.0 + 0.5 * np.sin(z + y)]).astype(np.float32)
    flow = torch.from_numpy(field[None]).cuda()
    del z, y, x, field
    mesh = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float32, device="cuda") - 0.5 * (s - 1) for s in vol], indexing="ij")).reshape(3, -1)
    print("device %s | volume %s, C = 1, B = 1 | windows of %d calls, %d alternated windows, median (min max) per call"
          % (torch.cuda.get_device_name(0), "x".join(map(str, vol)), args.reps, args.windows))

    grid = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float32, device="cuda") for s in vol], indexing="ij")).unsqueeze(0)

    def aten_transformer(img, fl):
        """the op chain of the reference's SpatialTransformer.forward (torch/layers.py:30-48) on the resident grid buffer"""
        locs = grid + fl
        locs = torch.stack([2 * (locs[:, i] / (s - 1) - 0.5) for i, s in enumerate(vol)], dim=-1).flip(-1)
        return F.grid_sample(img, locs, align_corners=True, mode="bilinear")

    def aten_shift(mt, w):
        q = mesh if w is None else mesh + w.reshape(3, -1)
        return ((torch.matmul(mt[0, :, :3], q) + mt[0, :, 3:]) - mesh).reshape((1, 3) + vol)

    with torch.no_grad():
        sh_k, sh_a = vxm.utils.affine_to_dense_shift(mat, vol, warp_right=flow), aten_shift(mat, flow)
        two = VF.WarpFn.apply(src, sh_k, "bilinear")
        aten = aten_transformer(src, sh_a)
        print("on the timed inputs: shift kernel vs ATen shift rel-L2 %.2e, moved image rel-L2 %.2e"
              % (float((sh_k - sh_a).norm() / sh_a.norm()), float((two - aten).norm() / aten.norm())))
        assert float((sh_k - sh_a).norm() / sh_a.norm()) < 1e-5 and float((two - aten).norm() / aten.norm()) < 1e-4
        del sh_k, sh_a, two, aten

    gout, gsh = torch.rand_like(src), torch.rand_like(flow)
    fg = flow.clone().requires_grad_()

    for tag, w in (("matrix + field", flow), ("matrix alone", None)):
        nf = 3 if w is not None else 0

        def s_kernel():
            with torch.no_grad():
                return vxm.utils.affine_to_dense_shift(mat, vol, warp_right=w)

        def s_aten():
            with torch.no_grad():
                return aten_shift(mat, w)

        def f_two():
            with torch.no_grad():
                return VF.WarpFn.apply(src, vxm.utils.affine_to_dense_shift(mat, vol, warp_right=w), "bilinear")

        def f_aten():
            with torch.no_grad():
                return aten_transformer(src, aten_shift(mat, w))
        race("the matrix as a dense field, forward, %s" % tag, [("shift kernel", s_kernel, 4.0 * V * (3 + nf)),
                                                                ("ATen: torch.matmul on a resident mesh", s_aten, None)], args)
        race("the matrix applied to a volume, forward, %s" % tag,
             [("shift kernel + dense warp kernel (one interpolation)", f_two, 4.0 * V * (3 + nf) + 4.0 * V * 5),
              ("ATen: torch.matmul shift + SpatialTransformer op chain", f_aten, None)], args)

    def sb_kernel():
        fg.grad = None
        vxm.utils.affine_to_dense_shift(mat, vol, warp_right=fg).backward(gsh)

    def sb_aten():
        fg.grad = None
        aten_shift(mat, fg).backward(gsh)

    def b_two():
        fg.grad = None
        VF.WarpFn.apply(src, vxm.utils.affine_to_dense_shift(mat, vol, warp_right=fg), "bilinear").backward(gout)

    def b_aten():
        fg.grad = None
        aten_transformer(src, aten_shift(mat, fg)).backward(gout)
    race("the matrix as a dense field, forward + backward (gw)", [("shift kernels", sb_kernel, 4.0 * V * 6 + 4.0 * V * 6),
                                                                  ("ATen: torch.matmul on a resident mesh", sb_aten, None)], args)
    race("the matrix applied to a volume, forward + backward (gw)",
         [("shift + dense warp kernels", b_two, 4.0 * V * 6 + 4.0 * V * 5 + 4.0 * V * 8 + 4.0 * V * 6),
          ("ATen: torch.matmul shift + SpatialTransformer op chain", b_aten, None)], args)

    # the yardstick: the existing dense warp kernel alone on the same field
    def f_dense():
        with torch.no_grad():
            return VF.WarpFn.apply(src, flow, "bilinear")

    def b_dense():
        fg.grad = None
        VF.WarpFn.apply(src, fg, "bilinear").backward(gout)
    race("yardstick: the dense warp kernel alone on the field", [("k_warp3d_fwd", f_dense, 4.0 * V * 5), ("k_warp3d_fwd + k_warp3d_bwd (gflow)", b_dense, 4.0 * V * 5 + 4.0 * V * 8)], args)


if __name__ == "__main__":
    main()
