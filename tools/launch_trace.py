#!/usr/bin/env python
"""Record every launch `voxelmorph_amd.torch.functional` makes through the C ABI in one training step, as text that two versions of the host
code can be diffed by.

`Recorder` replaces `functional.call` (a module attribute, looked up at call time by every wrapper in that module) by a recorder that
forwards.  The script runs two seeded training steps of VxmDense at a given shape -- forward, NCC + Grad, backward, FlatAdam -- and prints one
line per call of the SECOND step (packed operators stale after the first optimiser step, caches warm): the entry point, every integer and
float argument, `P` / `NULL` for a pointer, and the stream it went to as an ordinal in order of first use by the process (the second stream,
which builds the packed operators beside the first layer, is used first: stream0; the main stream is stream1).

    python tools/launch_trace.py --shape 160 192 224 > trace.txt
    VXM_S3_MIN_TILES=1 VXM_S3U=0 python tools/launch_trace.py --shape 32 32 32
"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Recorder:
    """with Recorder(functional) as rec: ...; rec.calls == [(entry point, args, stream handle), ...]"""

    def __init__(self, module):
        self.module, self.calls, self.streams = module, [], {}

    def __enter__(self):
        self.forward = self.module.call
        self.module.call = self
        return self

    def __exit__(self, *exc):
        self.module.call = self.forward

    def __call__(self, name, *args):
        self.calls.append((name, args))
        return self.forward(name, *args)

    def lines(self, calls=None):
        from voxelmorph_amd import _lib
        out = []
        for name, args in (self.calls if calls is None else calls):
            types = _lib.SIGNATURES[name]
            words = []
            assert len(args) == len(types) and types[-1] is ctypes.c_void_p, name      # every entry point takes the stream last
            for a, t in zip(args[:-1], types[:-1]):
                if t is ctypes.c_void_p:
                    words.append("NULL" if a is None else "P")
                else:
                    words.append(repr(float(a)) if t is ctypes.c_float else str(int(a)))
            handle = args[-1] or 0
            words.append("stream%d" % self.streams.setdefault(handle, len(self.streams)))
            out.append("%s %s" % (name, " ".join(words)))
        return out


def train_steps(shape, steps, rec, batch=1):
    """`steps` seeded training steps of VxmDense under `rec`; returns the index into rec.calls at which each step began"""
    import voxelmorph_amd as vxm
    from voxelmorph_amd.optim import FlatAdam
    torch.manual_seed(0)
    model = vxm.networks.VxmDense(shape, int_steps=7, int_downsize=2).cuda()
    opt = FlatAdam(model, lr=1e-4)
    src, trg = torch.rand((batch, 1) + tuple(shape), device="cuda"), torch.rand((batch, 1) + tuple(shape), device="cuda")
    ncc, grad = vxm.losses.NCC().loss, vxm.losses.Grad("l2", loss_mult=2).loss
    begins = []
    for _ in range(steps):
        begins.append(len(rec.calls))
        opt.zero_grad()
        y, pre = model(src, trg)
        loss = ncc(trg, y) + 0.01 * grad(None, pre)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    return begins


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", type=int, nargs=3, default=(160, 192, 224))
    ap.add_argument("--batch", type=int, default=1)
    args = ap.parse_args()
    from voxelmorph_amd.torch import functional as VF
    with Recorder(VF) as rec:
        begins = train_steps(tuple(args.shape), 2, rec, args.batch)
    print("# launch trace of training step 2: VxmDense %s, B = %d, engine %s" % ("x".join(map(str, args.shape)), args.batch, VF.FP32_ENGINE))
    rec.lines(rec.calls[:begins[1]])         # (stream ordinals in order of first use by the process, step 1 included)
    for line in rec.lines(rec.calls[begins[1]:]):
        print(line)


if __name__ == "__main__":
    main()
