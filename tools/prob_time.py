#!/usr/bin/env python
"""Time the probabilistic velocity field (voxelmorph_amd/csrc/prob.hip) at 160 x 192 x 224, B = 1, with HIP events:

  * the KL loss, forward and forward + backward, and the sampler, forward and forward + backward, each against its ATen formulation on the
    same device (tests/prob_cases.py kl_torch / sample_torch in fp32 with autograd), with the algorithmic bytes (every tensor read or
    written once) over the median against the 6.29 TB/s measured for HBM;
  * a full training step of VxmDenseProbabilistic (MSE / sigma^2 + KL, fresh noise per step), launch by launch and replayed as one hipGraph,
    against the same step of VxmDense with MSE + Grad -- whose code this change leaves as it was.  The difference is the price of the two
    unfused heads, the vxm_add2 launches, the sampler and the KL loss.

Each candidate is warmed up, then timed in windows of `--reps` back-to-back calls between two events; candidates are ALTERNATED over
`--windows` windows and the median, minimum and maximum window are printed (per call).

    python tools/prob_time.py > profiles/pr11_prob_time.txt
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


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shape", type=int, nargs=3, default=(160, 192, 224))
    p.add_argument("--reps", type=int, default=10, help="calls per timed window")
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--no-steps", action="store_true", help="time the kernels only, not the training steps")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("prob_time.py measures on an MI355X; no HIP device found (there is no CPU fallback and no CPU timing)")

    import prob_cases as pc
    import voxelmorph_amd as vxm
    from voxelmorph_amd.graph import GraphedStep
    from voxelmorph_amd.optim import FlatAdam
    from voxelmorph_amd.torch import functional as VF

    vol = tuple(args.shape)
    V = int(np.prod(vol))
    print("device %s | volume %s, B = 1 | windows of %d calls, %d alternated windows, median (min max) per call"
          % (torch.cuda.get_device_name(0), "x".join(map(str, vol)), args.reps, args.windows))
    g = torch.Generator(device="cuda").manual_seed(11)
    params = torch.cat([0.5 * torch.randn((1, 3) + vol, device="cuda", generator=g),
                        -12.0 + 14.0 * torch.rand((1, 3) + vol, device="cuda", generator=g)], 1).requires_grad_()
    eps, gz = torch.randn((1, 3) + vol, device="cuda", generator=g), torch.randn((1, 3) + vol, device="cuda", generator=g)
    lam = 10.0
    kl = vxm.losses.KL(lam, vol).loss
    one = torch.ones((), device="cuda")

    with torch.no_grad():
        a, b = kl(None, params), pc.kl_torch(params, lam, torch.float32)
        za, zb = VF.SampleLogVarFn.apply(params, eps), pc.sample_torch(params, eps)
        print("on the timed inputs: KL kernel %.7g, ATen fp32 %.7g; sample rel-L2 %.2e" % (float(a), float(b), float((za - zb).norm() / zb.norm())))
        assert abs(float(a) - float(b)) < 1e-4 * abs(float(b)) and float((za - zb).norm() / zb.norm()) < 1e-6
        del za, zb

    def k_fwd():
        with torch.no_grad():
            return kl(None, params)

    def a_fwd():
        with torch.no_grad():
            return pc.kl_torch(params, lam, torch.float32)

    def k_fb():
        params.grad = None
        kl(None, params).backward(one)

    def a_fb():
        params.grad = None
        pc.kl_torch(params, lam, torch.float32).backward(one)

    def s_fwd():
        with torch.no_grad():
            return VF.SampleLogVarFn.apply(params, eps)

    def sa_fwd():
        with torch.no_grad():
            return pc.sample_torch(params, eps)

    def s_fb():
        params.grad = None
        VF.SampleLogVarFn.apply(params, eps).backward(gz)

    def sa_fb():
        params.grad = None
        pc.sample_torch(params, eps).backward(gz)
    race("KL loss, forward", [("kl_fwd_kernel + kl_finish_kernel", k_fwd, 4.0 * V * 6), ("ATen fp32 formulation", a_fwd, None)], args)
    race("KL loss, forward + backward", [("vxm_kl_fwd + vxm_kl_bwd", k_fb, 4.0 * V * (6 + 6 + 6)), ("ATen fp32 formulation, autograd", a_fb, None)], args)
    race("sample, forward", [("sample_fwd_kernel", s_fwd, 4.0 * V * (6 + 3 + 3)), ("ATen fp32 formulation", sa_fwd, None)], args)
    race("sample, forward + backward", [("vxm_sample_logvar_fwd + _bwd", s_fb, 4.0 * V * (12 + 3 + 3 + 3 + 6)),
                                        ("ATen fp32 formulation, autograd", sa_fb, None)], args)
    if args.no_steps:
        return
    del params, eps, gz
    torch.cuda.empty_cache()

    src, trg = torch.rand((1, 1) + vol, device="cuda", generator=g), torch.rand((1, 1) + vol, device="cuda", generator=g)
    mse = vxm.losses.MSE().loss
    steps = []
    for graphed in (False, True):
        torch.manual_seed(3)
        det = vxm.networks.VxmDense(vol, int_steps=7, int_downsize=2).cuda()
        opt_d = FlatAdam(det, lr=1e-4)
        grad = vxm.losses.Grad("l2", loss_mult=2).loss

        def fwd_det(det=det, grad=grad):
            y, pre = det(src, trg)
            return vxm.losses.weighted_sum([mse(trg, y), grad(None, pre)], [1.0, 0.01])
        prob = vxm.networks.VxmDenseProbabilistic(vol, int_steps=7, int_downsize=2).cuda()
        opt_p = FlatAdam(prob, lr=1e-4)
        prob.draw_noise(batch=1)

        def fwd_prob(prob=prob):
            y, fp = prob(src, trg, noise=prob.noise)
            return vxm.losses.weighted_sum([mse(trg, y), kl(None, fp)], [1.0 / 0.02 ** 2, 0.01])
        sd, sp = GraphedStep(fwd_det, opt_d, eager_steps=2, enabled=graphed), GraphedStep(fwd_prob, opt_p, eager_steps=2, enabled=graphed)

        def step_prob(prob=prob, sp=sp):
            prob.draw_noise()
            sp()
        tag = "one hipGraph replay" if graphed else "launch by launch"
        steps.append((sd, sp))
        race("training step, %s" % tag, [("VxmDense, MSE + Grad (unchanged code)", sd, None),
                                          ("VxmDenseProbabilistic, MSE / sigma^2 + KL, noise drawn per step", step_prob, None)], args, reps=5)
        if graphed:
            print("    (replays: %d / %d; capture errors: %r / %r)" % (sd.replays, sp.replays, sd.capture_error, sp.capture_error))


if __name__ == "__main__":
    main()
