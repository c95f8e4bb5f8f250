#!/usr/bin/env python
"""SynthMorph training on MI355X: a contrast-agnostic registration learned from label maps alone.

Every step draws two label maps, synthesises an image of random contrast and geometry from each on the device
(`voxelmorph_amd.synth.labels_to_image`: a random smooth deformation, intensities per label, blur, bias field, gamma) and trains the
registration of the two images with the Dice of the warped one-hot maps plus a smoothness term -- no acquired image is ever read.

The reference has this entry point for its TensorFlow backend (`scripts/tf/train_synthmorph.py`); this script takes that command line
(same flag names and defaults; `--steps-per-epoch` is an addition, the reference fixes 100) and runs its loop: the model is
`VxmDenseSemiSupervisedSeg(seg_resolution=1, unet_half_res=True, int_downsize=2)` -- the reference's `VxmDense(int_resolution=2,
svf_resolution=2)` plus a linear warp of the full-resolution one-hot map by `pos_flow` -- the loss `Dice(map_2, pred) + 1 +
Grad('l2', loss_mult=reg_param)(flow)`, Adam, a checkpoint of the starting weights and one every `--save-freq` epochs (`%05d.pt`).
Generation runs eagerly, outside any captured region.

    M Hoffmann, B Billot, DN Greve, JE Iglesias, B Fischl, AV Dalca.  SynthMorph: learning contrast-invariant registration without
    acquired images.  IEEE Transactions on Medical Imaging 41 (3), 543-558, 2022.  https://doi.org/10.1109/TMI.2021.3116879
"""
import argparse
import os
import pickle
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

_FLAGS = [
    # data organization parameters
    ('--label-dir', dict(nargs='+', required=True, help='path or glob pattern pointing to input label maps')),
    ('--model-dir', dict(default='models', help='model output directory [models]')),
    # generation parameters
    ('--same-subj', dict(action='store_true', help='generate image pairs from same label map')),
    ('--blur-std', dict(type=float, default=1, help='maximum blurring std. dev. [1]')),
    ('--gamma', dict(type=float, default=0.25, help='std. dev. of gamma [0.25]')),
    ('--vel-std', dict(type=float, default=0.5, help='std. dev. of SVF [0.5]')),
    ('--vel-res', dict(type=float, nargs='+', default=[16], help='SVF scale [16]')),
    ('--bias-std', dict(type=float, default=0.3, help='std. dev. of bias field [0.3]')),
    ('--bias-res', dict(type=float, nargs='+', default=[40], help='bias scale [40]')),
    ('--out-labels', dict(default=None, help='labels to optimize: .npy list or .pickle dict {input: output} [all input labels]')),
    # training parameters
    ('--gpu', dict(default='0', help='ID of GPU to use [0]')),
    ('--epochs', dict(type=int, default=1500, help='training epochs [1500]')),
    ('--steps-per-epoch', dict(type=int, default=100, help='optimiser steps per epoch [100]')),
    ('--batch-size', dict(type=int, default=1, help='batch size [1]')),
    ('--init-weights', dict(help='optional checkpoint (.pt of this script) to initialize with')),
    ('--save-freq', dict(type=int, default=20, help='epochs between model saves [20]')),
    ('--reg-param', dict(type=float, default=1., help='regularization weight [1]')),
    ('--lr', dict(type=float, default=1e-4, help='learning rate [1e-4]')),
    ('--init-epoch', dict(type=int, default=0, help='initial epoch number [0]')),
    ('--seed', dict(type=int, default=0, help='seed of the label-map draws and of the synthesis [0]')),
    # network architecture parameters
    ('--int-steps', dict(type=int, default=5, help='number of integration steps [5]')),
    ('--enc', dict(type=int, nargs='+', default=[64] * 4, help='U-Net encoder filters [64 64 64 64]')),
    ('--dec', dict(type=int, nargs='+', default=[64] * 6, help='U-Net decoder filters [64 x 6]')),
]


def parse(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for flag, kw in _FLAGS:
        parser.add_argument(flag, **kw)
    return parser.parse_args(argv)


def output_labels(path, labels_in):
    """the reference's `--out-labels` handling (train_synthmorph.py:117-123): a .npy list or a .pickle dict, restricted to the input labels"""
    present = set(np.asarray(labels_in).tolist())
    if path is None:
        return None
    if path.endswith('.npy'):
        return sorted(x for x in np.load(path).tolist() if x in present)
    if path.endswith('.pickle'):
        with open(path, 'rb') as f:
            return {k: v for k, v in pickle.load(f).items() if k in present}
    return None


def build_model(vxm, in_shape, nb_labels, enc, dec, int_steps):
    return vxm.networks.VxmDenseSemiSupervisedSeg(inshape=in_shape, nb_labels=nb_labels, nb_unet_features=[list(enc), list(dec)],
                                                  seg_resolution=1, int_steps=int_steps, int_downsize=2, unet_half_res=True)


def register(model, ima_1, ima_2, map_1):
    """(pos_flow, pred): the full-resolution displacement the reference regularises (`model.references.pos_flow`, train_synthmorph.py:163)
    and the one-hot map of image 1 warped linearly by it (:164)"""
    _, _, _, pos_flow, _ = model.vxm_model._forward_all(ima_1, ima_2)
    return pos_flow, model.seg_transformer(map_1, model.seg_resize(pos_flow))


def make_step(vxm, model, opt, reg_param, running=None):
    """one eager optimiser step on a synthesised pair: loss = Dice(map_2, pred) + 1 + Grad('l2', reg_param)(pos_flow)"""
    dice, grad = vxm.losses.Dice().loss, vxm.losses.Grad('l2', loss_mult=reg_param).loss

    def step(ima_1, map_1, ima_2, map_2):
        flow, pred = register(model, ima_1, ima_2, map_1)
        loss = vxm.losses.weighted_sum([dice(map_2, pred), grad(None, flow)], [1.0, 1.0], running=running) + 1.0
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss
    return step


def main(argv=None):
    args = parse(argv)
    import voxelmorph_amd as vxm
    from voxelmorph_amd.optim import FlatAdam
    from voxelmorph_amd.pacing import InFlight

    dev = torch.device('cuda', int(args.gpu.split(',')[0]))
    torch.cuda.set_device(dev)
    labels_in, label_maps = vxm.py.utils.load_labels(args.label_dir)
    gen = vxm.data.synthmorph(label_maps, batch_size=args.batch_size, same_subj=args.same_subj, flip=True, device=dev, seed=args.seed)
    in_shape = label_maps[0].shape
    table = vxm.synth.LabelTable(labels_in, output_labels(args.out_labels, labels_in))
    gen_args = dict(shape=in_shape, batch_size=args.batch_size, warp_std=args.vel_std, warp_res=args.vel_res, blur_std=args.blur_std,
                    bias_std=args.bias_std, bias_res=args.bias_res, gamma_std=args.gamma)
    rng = torch.Generator(device=dev).manual_seed(args.seed)

    def synthesise(labels):
        draws = vxm.synth.draw_params(rng, table, **gen_args)
        return vxm.synth.labels_to_image(labels, table, draws=draws, warp_res=args.vel_res, bias_res=args.bias_res, int_steps=args.int_steps)

    if args.init_weights:
        model = vxm.networks.VxmDenseSemiSupervisedSeg.load(args.init_weights, dev)
    else:
        model = build_model(vxm, in_shape, table.out_labels.size, args.enc, args.dec, args.int_steps)
    model.to(dev)
    model.train()
    opt = FlatAdam(model, lr=args.lr)
    terms = torch.zeros(3, device=dev)
    step = make_step(vxm, model, opt, args.reg_param, running=terms)

    os.makedirs(args.model_dir, exist_ok=True)
    model.save(os.path.join(args.model_dir, '%05d.pt' % args.init_epoch))
    pace = InFlight(2)
    for epoch in range(args.init_epoch, args.epochs):
        terms.zero_()
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(args.steps_per_epoch):
            pace.wait()                      # at most two steps in flight (voxelmorph_amd/pacing.py)
            src, trg = next(gen)
            ima_1, map_1 = synthesise(src)
            ima_2, map_2 = synthesise(trg)
            step(ima_1, map_1, ima_2, map_2)
            pace.mark()
        torch.cuda.synchronize()
        dt = (time.time() - t0) / args.steps_per_epoch
        t = (terms / args.steps_per_epoch).tolist()
        print('Epoch %d/%d - %.4f sec/step - loss: %.4e  (dice %.4e, grad %.4e)' % (epoch + 1, args.epochs, dt, t[-1] + 1.0, t[0], t[1]), flush=True)
        if (epoch + 1) % args.save_freq == 0 or epoch + 1 == args.epochs:
            model.save(os.path.join(args.model_dir, '%05d.pt' % (epoch + 1)))


if __name__ == '__main__':
    main()
