#!/usr/bin/env python
"""Time the evaluation kernels (voxelmorph_amd/csrc/metrics.hip) at 160 x 192 x 224 with HIP events, on seeded inputs, next to the ways the
same numbers were computed before they existed:

  label_overlap (30 labels)       vs  the per-label `==` / sum formulation (py/utils.py:283-284) in torch on the device
  warped_dice                     vs  SpatialTransformer(mode='nearest') followed by that formulation
  vxm_jacdet3d (det + stats)      vs  scripts/register.py's jacobian_determinant on the device (torch.gradient, stack, eye, cofactors)

Each candidate is warmed up, then timed in windows of `--reps` back-to-back calls between two events; the pairs are ALTERNATED over
`--windows` windows and the median, minimum and maximum window are printed (per call).  The results of the two ways are compared on the
timed inputs before anything is timed.  Bytes are what the algorithm has to move (each input once, each output once) over the median.

    python tools/eval_time.py > profiles/pr06_eval_time.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]


def label_maps(vol, labels, seed):
    """piecewise-constant maps: a coarse lattice of labels (8-voxel cells, two thirds background) upsampled to the volume; b = a moved by 3 voxels"""
    rng = np.random.default_rng(seed)
    vals = np.concatenate([np.zeros(2 * len(labels)), labels]).astype(np.float32)
    coarse = vals[rng.integers(0, len(vals), tuple(-(-n // 8) for n in vol))]
    a = np.kron(coarse, np.ones((8, 8, 8), np.float32))[:vol[0], :vol[1], :vol[2]]
    return np.ascontiguousarray(a), np.ascontiguousarray(np.roll(a, (3, 3, 3), (0, 1, 2)))


def torch_counts(a, b, labels):
    """the reference's formulation on the device: three reductions per label"""
    out = []
    for lab in labels:
        ea, eb = a == lab, b == lab
        out.append(torch.stack([(ea & eb).sum(), ea.sum(), eb.sum()]))
    return torch.stack(out)[None]


def window(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps            # us per call


def compare(name, new, old, nbytes, args):
    for fn in (new, old):
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    t_new, t_old = [], []
    for _ in range(args.windows):                            # alternate: both see the same neighbours on the machine
        t_new.append(window(new, args.reps))
        t_old.append(window(old, args.reps))
    m_new, m_old = float(np.median(t_new)), float(np.median(t_old))
    print("%-28s kernel path %9.1f us (min %9.1f max %9.1f)  %7.1f GB/s of required bytes | before %9.1f us (min %9.1f max %9.1f) | ratio %.2fx"
          % (name, m_new, min(t_new), max(t_new), nbytes / m_new * 1e-3, m_old, min(t_old), max(t_old), m_old / m_new))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shape", type=int, nargs=3, default=(160, 192, 224))
    p.add_argument("--reps", type=int, default=20, help="calls per timed window")
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("eval_time.py measures on an MI355X; no HIP device found (there is no CPU fallback and no CPU timing)")

    import voxelmorph_amd as vxm
    from voxelmorph_amd import metrics
    from voxelmorph_amd._lib import call, ptr, stream
    import register                                        # scripts/register.py: the Jacobian helper as it stands
    import eval_cases as ec

    vol = tuple(args.shape)
    V = int(np.prod(vol))
    labels = ec.LABELS30
    a_np, b_np = label_maps(vol, labels, 0)
    a, b = (torch.from_numpy(x).cuda()[None, None] for x in (a_np, b_np))
    rng = np.random.default_rng(1)
    flow = torch.from_numpy(ec._smooth(rng, 3, vol, 5.0).astype(np.float32)).cuda()[None]
    lab_list = [float(x) for x in labels]
    st = vxm.layers.SpatialTransformer(vol, mode="nearest").cuda()
    print("device %s | volume %s | %d labels | windows of %d calls, %d alternated windows, median (min max) per call"
          % (torch.cuda.get_device_name(0), "x".join(map(str, vol)), len(labels), args.reps, args.windows))

    with torch.no_grad():
        # the two ways agree on the timed inputs
        c_new = metrics.label_overlap(a.reshape(1, -1), b.reshape(1, -1), labels)
        assert torch.equal(c_new, torch_counts(a, b, lab_list)), "label_overlap differs from the per-label formulation"
        lab_dev, L = metrics._device_labels(labels, a.device)
        counts = torch.empty((1, L, 3), dtype=torch.int64, device="cuda")

        def fused():
            call("vxm_warp3d_label_overlap", ptr(a), ptr(flow), ptr(b), None, ptr(lab_dev), L, ptr(counts), 1, *vol, stream())
        fused()
        assert torch.equal(counts, torch_counts(st(a, flow), b, lab_list)), "fused warp + overlap differs from warp, then per-label sums"
        det = torch.empty((1,) + vol, dtype=torch.float32, device="cuda")
        stats = torch.empty((1, 2), dtype=torch.int64, device="cuda")

        def jac():
            call("vxm_jacdet3d", ptr(flow), ptr(det), ptr(stats), 1, *vol, stream())

        def jac_before():
            return (register.jacobian_determinant(flow[0]) <= 0).float().mean()
        jac()
        d_old = register.jacobian_determinant(flow[0])
        err = float((det[0] - d_old).abs().max())
        n_old = int((d_old <= 0).sum())
        print("jacobian: max |kernel - register.py helper| %.2e, det <= 0: kernel %d, helper %d of %d" % (err, int(stats[0, 0]), n_old, V))
        assert err < 1e-4 and abs(int(stats[0, 0]) - n_old) <= 1e-4 * V
        del d_old

        compare("label_overlap", lambda: metrics.label_overlap(a.reshape(1, -1), b.reshape(1, -1), lab_dev),
                lambda: torch_counts(a, b, lab_list), 8.0 * V, args)
        compare("warped_dice (counts)", fused, lambda: torch_counts(st(a, flow), b, lab_list), 20.0 * V, args)
        compare("jacdet3d (det + stats)", jac, jac_before, 16.0 * V, args)
        compare("jacdet3d (stats only)", lambda: call("vxm_jacdet3d", ptr(flow), None, ptr(stats), 1, *vol, stream()), jac_before, 12.0 * V, args)
        # a field that folds at half of its voxels: every block has counts to add (the smooth field above folds nowhere)
        noise = torch.from_numpy(ec.jac_field(vol, "noise5", 3)).cuda()

        def jac_noise():
            call("vxm_jacdet3d", ptr(noise), ptr(det), ptr(stats), 1, *vol, stream())
        jac_noise()
        print("5-voxel noise: det <= 0 at %d of %d voxels" % (int(stats[0, 0]), V))
        compare("jacdet3d, folding field", jac_noise, lambda: (register.jacobian_determinant(noise[0]) <= 0).float().mean(), 16.0 * V, args)


if __name__ == "__main__":
    main()
