#!/usr/bin/env python
"""Time the SynthMorph image synthesis (voxelmorph_amd/csrc/synth.hip, voxelmorph_amd/synth.py) at 160 x 192 x 224, B = 1, 26 labels, with
HIP events:

  * each kernel -- draw, blur (T = 7), finish, one-hot -- against its ATen formulation on the same device (tests/synth_cases.py draw_torch /
    blur_torch / finish_torch / onehot_torch: a gather by label and `randn * std + mean`, three conv3d calls, exp / mul / clamp / amin /
    amax / pow, L compares), with the algorithmic bytes per voxel (draw 12, blur 8, finish 20, one-hot 4 + 4 Lout) over the median
    against the 6.29 TB/s measured for HBM;
  * the whole `labels_to_image` call, and the same call with the four kernels replaced by their ATen formulations (the deformation
    and the smooth fields are this library's kernels in both);
  * two syntheses beside one training step of VxmDense (MSE + Grad, launch by launch) -- the step of the parent commit, whose code
    this change leaves as it was.

Each candidate is warmed up, then timed in windows of `--reps` back-to-back calls between two events; candidates are ALTERNATED over
`--windows` windows and the median, minimum and maximum window are printed (per call).

    python tools/synth_time.py > profiles/pr12_synth_time.txt
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


def race(title, cands, args, reps=None):
    """cands: [(name, fn, algorithmic bytes or None)]"""
    reps = reps or args.reps
    for _, fn, _ in cands:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in cands]
    for _ in range(args.windows):                            # alternate: every candidate sees the same neighbours on the machine
        for t, (_, fn, _) in zip(times, cands):
            t.append(window(fn, reps))
    print(title)
    base = float(np.median(times[0]))
    for t, (name, _, nbytes) in zip(times, cands):
        m = float(np.median(t))
        bw = "" if nbytes is None else " | %6.0f GB/s of the algorithmic bytes = %4.1f %% of HBM" % (nbytes / m * 1e-3, 100 * nbytes / (m * 1e-6) / HBM)
        print("    %-58s %9.1f us (min %9.1f max %9.1f) | %5.2fx the first line%s" % (name, m, min(t), max(t), m / base, bw))
    sys.stdout.flush()
    return [float(np.median(t)) for t in times]


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shape", type=int, nargs=3, default=(160, 192, 224))
    p.add_argument("--labels", type=int, default=26)
    p.add_argument("--reps", type=int, default=10, help="calls per timed window")
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--no-step", action="store_true", help="time the synthesis only, not the training step")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("synth_time.py measures on an MI355X; no HIP device found (there is no CPU fallback and no CPU timing)")

    import synth_cases as sc
    import voxelmorph_amd as vxm
    from voxelmorph_amd.optim import FlatAdam
    S = vxm.synth

    vol = tuple(args.shape)
    V = int(np.prod(vol))
    L = args.labels
    print("device %s | volume %s, B = 1, %d labels | windows of %d calls, %d alternated windows, median (min max) per call"
          % (torch.cuda.get_device_name(0), "x".join(map(str, vol)), L, args.reps, args.windows))
    g = torch.Generator(device="cuda").manual_seed(12)
    label_list = [0] + sorted(np.random.default_rng(1).choice(np.arange(1, 2036), size=L - 1, replace=False).tolist())
    table = S.LabelTable(label_list)
    lab_t = torch.tensor(label_list, dtype=torch.float32, device="cuda")
    # a piecewise constant label map: a coarse random map of list indices, nearest-upsampled x8
    coarse = torch.randint(0, L, (1, 1) + tuple(-(-s // 8) for s in vol), device="cuda", generator=g)
    idx = coarse.repeat_interleave(8, 2).repeat_interleave(8, 3).repeat_interleave(8, 4)[:, :, :vol[0], :vol[1], :vol[2]]
    labels = lab_t[idx].contiguous()
    draws = S.draw_params(g, table, vol, batch_size=1)
    taps = draws.taps
    with torch.no_grad():
        raw = S.draw(labels, table, draws.means, draws.stds, draws.noise)
        blurred = S.blur(raw, taps)
        bias = S.draw_perlin(vol, (40,), draws.bias_std, draws.bias_noise)
        # the kernels against the ATen formulation on the timed inputs
        e_draw = float((raw - sc.draw_torch(labels, lab_t, draws.means, draws.stds, draws.noise)).abs().max())
        e_blur = float((blurred - sc.blur_torch(raw, taps)).norm() / blurred.norm())
        fin = S.finish(blurred, bias, draws.gamma)
        e_fin = float((fin - sc.finish_torch(blurred, bias, draws.gamma)).norm() / fin.norm())
        same_hot = torch.equal(S.onehot(labels, table), sc.onehot_torch(labels, lab_t))
    print("on the timed inputs: draw max |diff| %.2e, blur rel-L2 %.2e, finish rel-L2 %.2e, one-hot equal: %s"
          % (e_draw, e_blur, e_fin, same_hot))
    assert e_draw < 1e-4 and e_blur < 1e-6 and e_fin < 1e-5 and same_hot

    def nograd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run
    race("draw (12 B / voxel)", [("synth_draw_kernel", nograd(lambda: S.draw(labels, table, draws.means, draws.stds, draws.noise)), 12.0 * V),
                                 ("ATen: bucketize, 2 gathers, mul, add, where", nograd(lambda: sc.draw_torch(labels, lab_t, draws.means, draws.stds, draws.noise)), None)], args)
    race("blur, T = %d (8 B / voxel at least)" % draws.T,
         [("blur_strided_kernel x 2 + blur_row_kernel", nograd(lambda: S.blur(raw, taps)), 8.0 * V),
          ("ATen: three conv3d calls", nograd(lambda: sc.blur_torch(raw, taps)), None)], args)
    race("finish with a bias field (20 B / voxel)",
         [("finish_minmax_kernel + finish_apply_kernel", nograd(lambda: S.finish(blurred, bias, draws.gamma)), 20.0 * V),
          ("ATen: exp, mul, clamp, amin, amax, sub, div, pow, where", nograd(lambda: sc.finish_torch(blurred, bias, draws.gamma)), None)], args)
    race("one-hot, Lout = %d (4 + 4 Lout B / voxel)" % L,
         [("onehot_kernel", nograd(lambda: S.onehot(labels, table)), (4.0 + 4.0 * L) * V),
          ("ATen: L compares in one broadcast `==`, cast to fp32", nograd(lambda: sc.onehot_torch(labels, lab_t)), None)], args)

    def synth_kernels():
        return S.labels_to_image(labels, table, draws=draws)

    def synth_aten():
        with torch.no_grad():
            warped = S.deform(labels, draws)
            image = sc.blur_torch(sc.draw_torch(warped, lab_t, draws.means, draws.stds, draws.noise), draws.taps)
            image = sc.finish_torch(image, S.draw_perlin(vol, (40,), draws.bias_std, draws.bias_noise), draws.gamma)
            return image, sc.onehot_torch(warped, lab_t)

    def deform_only():
        with torch.no_grad():
            return S.deform(labels, draws), S.draw_perlin(vol, (40,), draws.bias_std, draws.bias_noise)
    t_k, t_a, t_d = race("labels_to_image, the whole call (draws given)",
                         [("the four kernels", synth_kernels, None), ("the ATen formulation of the four", synth_aten, None),
                          ("of which: velocity, integration, warp, bias field (both)", deform_only, None)], args, reps=5)
    t_p = race("draw_params: the random inputs of one image (torch.rand / randn on the device)",
               [("draw_params", lambda: S.draw_params(g, table, vol, batch_size=1), None)], args, reps=5)[0]
    if args.no_step:
        return
    del raw, blurred, bias, fin
    torch.cuda.empty_cache()
    src, trg = torch.rand((1, 1) + vol, device="cuda", generator=g), torch.rand((1, 1) + vol, device="cuda", generator=g)
    torch.manual_seed(3)
    det = vxm.networks.VxmDense(vol, int_steps=7, int_downsize=2).cuda()
    opt = FlatAdam(det, lr=1e-4)
    mse, grad = vxm.losses.MSE().loss, vxm.losses.Grad("l2", loss_mult=2).loss

    def step():
        y, pre = det(src, trg)
        loss = vxm.losses.weighted_sum([mse(trg, y), grad(None, pre)], [1.0, 0.01])
        opt.zero_grad()
        loss.backward()
        opt.step()
    t_s = race("training step of VxmDense, MSE + Grad, launch by launch (unchanged code)", [("one step", step, None)], args, reps=5)[0]
    print("two syntheses (draws included) beside one training step: 2 x (%.0f + %.0f) us = %.0f us = %.1f %% of the step's %.0f us; "
          "with the ATen formulation 2 x (%.0f + %.0f) us = %.1f %%"
          % (t_k, t_p, 2 * (t_k + t_p), 100 * 2 * (t_k + t_p) / t_s, t_s, t_a, t_p, 100 * 2 * (t_a + t_p) / t_s))


if __name__ == "__main__":
    main()
