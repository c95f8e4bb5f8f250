#!/usr/bin/env python
"""Time the mutual information loss (voxelmorph_amd/csrc/mi.hip) at 160 x 192 x 224, B = 1, K = 32 and K = 16, with HIP events, next to
the ATen formulation of the same definition (tests/mi_cases.py `formulation` at float32: two [1, N, K] weight tensors and a bmm) on the
same device in the same process; then a training step with the loss next to the same step with NCC.

Inputs: the real scan scaled to [0, 1] and its smoothly remapped (contrast-inverted) copy displaced by one voxel.  Each candidate is warmed
up, then timed in windows of `--reps` back-to-back calls between two events; the pairs are ALTERNATED over `--windows` windows and the
median, minimum and maximum window are printed (per call).  Both ways are compared with the float64 arbiter on the timed inputs before anything is timed.

The bound per direction is modelled as 4 K^2 N FLOP at the 155 TFLOP/s measured for the fp32 matrix pipe plus 2 K exp per voxel at a
quarter of the fp32 vector lane rate; the required traffic is the two images (55 MB), each read once, against 6.29 TB/s measured.

    python tools/mi_time.py > profiles/pr08_mi_time.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

MATRIX_FP32 = 155e12          # FLOP/s, measured (v_mfma_f32_32x32x2_f32)
EXP_RATE = 256 * 4 * 16 * 2.4e9 / 4        # exp/s: 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz, quarter rate
HBM = 6.29e12                 # B/s, measured


def window(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps            # us per call


def compare(name, new, old, args, bound_us=None, nbytes=None, old_name="ATen formulation"):
    for fn in (new, old):
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    t_new, t_old = [], []
    for _ in range(args.windows):                            # alternate: both see the same neighbours on the machine
        t_new.append(window(new, args.reps))
        t_old.append(window(old, args.reps))
    m_new, m_old = float(np.median(t_new)), float(np.median(t_old))
    extra = ""
    if bound_us is not None:
        extra = " | modelled bound %.1f us = %.0f %% of the time; %.0f GB/s of the required bytes = %.1f %% of HBM" % (
            bound_us, 100 * bound_us / m_new, nbytes / m_new * 1e-3, 100 * nbytes / (m_new * 1e-6) / HBM)
    print("%-34s kernel path %10.1f us (min %10.1f max %10.1f) | %s %10.1f us (min %10.1f max %10.1f) | ratio %.2fx%s"
          % (name, m_new, min(t_new), max(t_new), old_name, m_old, min(t_old), max(t_old), m_old / m_new, extra))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shape", type=int, nargs=3, default=(160, 192, 224))
    p.add_argument("--reps", type=int, default=5, help="calls per timed window")
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--no-step", action="store_true", help="skip the training steps")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("mi_time.py measures on an MI355X; no HIP device found (there is no CPU fallback and no CPU timing)")

    import voxelmorph_amd as vxm
    from voxelmorph_amd import _lib
    from voxelmorph_amd.graph import GraphedStep
    from voxelmorph_amd.optim import FlatAdam
    import mi_cases as mc

    vol = tuple(args.shape)
    N = int(np.prod(vol))
    scan = np.load(os.path.join(ROOT, "tests", "golden", "real_scan_u8.npz"), allow_pickle=False)["vol_u8"].astype(np.float32) / 255.0
    assert all(v <= s for v, s in zip(vol, scan.shape)), "the scan is %s" % (scan.shape,)
    scan = scan[:vol[0], :vol[1], :vol[2]]
    fixed = torch.from_numpy(np.ascontiguousarray(scan)).cuda()[None, None]
    moving = torch.from_numpy(np.ascontiguousarray(mc.remap(np.roll(scan, 1, axis=2)))).cuda()[None, None]
    print("device %s | volume %s, B = 1 | windows of %d calls, %d alternated windows, median (min max) per call"
          % (torch.cuda.get_device_name(0), "x".join(map(str, vol)), args.reps, args.windows))

    for K in (32, 16):
        mi = vxm.losses.MutualInformation(nb_bins=K)
        bound = (4.0 * K * K * N / MATRIX_FP32 + 2.0 * K * N / EXP_RATE) * 1e6
        pred = moving.clone().requires_grad_()

        def aten():
            return mc.formulation(fixed, pred, mi.bin_centers, dtype=torch.float32)
        def once(fn):
            loss = fn()
            loss.backward()
            g, pred.grad = pred.grad.double(), None
            return float(loss.detach()), g
        l_new, g_new = once(lambda: mi.loss(fixed, pred))
        torch.cuda.reset_peak_memory_stats()
        l_old, g_old = once(aten)
        peak = torch.cuda.max_memory_allocated() / 1e9
        l_64, g_64 = once(lambda: mc.formulation(fixed, pred, mi.bin_centers, dtype=torch.float64))         # the arbiter, on the device
        rel_new, rel_old = (float((g - g_64).norm() / g_64.norm()) for g in (g_new, g_old))
        print("K = %d against the float64 arbiter (loss %.9f): kernel loss error %.2e, gradient rel-L2 %.2e | ATen fp32 formulation loss error "
              "%.2e, gradient rel-L2 %.2e | workspace %.2f MB, peak memory of one ATen fp32 forward + backward %.2f GB"
              % (K, l_64, abs(l_new - l_64), rel_new, abs(l_old - l_64), rel_old, _lib.lib().vxm_mi_workspace_bytes(1, N, K) / 1e6, peak))
        assert abs(l_new - l_64) < 1e-5 and rel_new < 1e-4, "the kernel path is off the arbiter on the timed inputs"
        del g_new, g_old, g_64
        torch.cuda.empty_cache()

        def fwd_new():
            with torch.no_grad():
                return mi.loss(fixed, moving)

        def fwd_old():
            with torch.no_grad():
                return mc.formulation(fixed, moving, mi.bin_centers, dtype=torch.float32)

        def fb_new():
            pred.grad = None
            mi.loss(fixed, pred).backward()

        def fb_old():
            pred.grad = None
            aten().backward()
        compare("K = %d forward" % K, fwd_new, fwd_old, args, bound, 8.0 * N)
        compare("K = %d forward + backward" % K, fb_new, fb_old, args, 2 * bound, 20.0 * N)
        del pred
        torch.cuda.empty_cache()

    if args.no_step:
        return

    def make_step(image_loss):
        torch.manual_seed(0)
        model = vxm.networks.VxmDense(vol, int_steps=7, int_downsize=2).cuda()
        opt = FlatAdam(model, lr=1e-4)
        reg = vxm.losses.Grad("l2", loss_mult=2).loss

        def fwd():
            y, pre = model(moving, fixed)
            return vxm.losses.weighted_sum([image_loss(fixed, y), reg(None, pre)], [1.0, 0.01])
        return GraphedStep(fwd, opt, eager_steps=2)
    step_mi, step_ncc = make_step(vxm.losses.MutualInformation().loss), make_step(vxm.losses.NCC().loss)
    compare("training step (fp32, graph replay)", step_mi, step_ncc, args, old_name="the same step with NCC")
    print("replays: MI %d, NCC %d" % (step_mi.replays, step_ncc.replays))


if __name__ == "__main__":
    main()
