#!/usr/bin/env python
"""Score a trained VxmDense on MI355X -- the command line of the reference's `scripts/tf/test.py` (:46-55: --gpu --model --pairs
--img-suffix --seg-suffix --img-prefix --seg-prefix --labels --multichannel).  For every pair of the list: register moving to fixed,
propagate the moving segmentation through the warp with the bit-exact nearest-neighbour transformer, and report the Dice overlap with the
fixed segmentation over the label list (:86-116); then the two summary lines (:118-121).  Warp and Dice are ONE kernel launch per pair
(voxelmorph_amd.metrics.warped_dice); the warped segmentation is never written.  `--jacobian` (this package's addition) also prints the
share of voxels with a non-positive Jacobian determinant of each warp.

    test.py --model model.pt --pairs pairs.txt --img-suffix /img.npz --seg-suffix /seg.npz --labels labels.npy

pairs.txt holds one whitespace-separated moving / fixed pair per line; images are read from the npz variable 'vol', segmentations from
'seg' (nii / nii.gz / mgz / npy work too)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--gpu', default='0', help='GPU number (this path has no CPU fallback; default 0)')
    p.add_argument('--model', required=True, help='VxmDense model file')
    p.add_argument('--pairs', required=True, help='path to list of image pairs to register')
    p.add_argument('--img-suffix', help='input image file suffix')
    p.add_argument('--seg-suffix', help='input seg file suffix')
    p.add_argument('--img-prefix', help='input image file prefix')
    p.add_argument('--seg-prefix', help='input seg file prefix')
    p.add_argument('--labels', help='optional label list to compute dice for (in npy format)')
    p.add_argument('--multichannel', action='store_true', help='specify that data has multiple channels')
    p.add_argument('--jacobian', action='store_true', help='also print the share of non-positive Jacobian determinants per pair')
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    if args.img_prefix == args.seg_prefix and args.img_suffix == args.seg_suffix:          # test.py:59-61
        print('Error: Must provide a differing file suffix and/or prefix for images and segs.')
        return 1

    import torch
    import voxelmorph_amd as vxm
    from voxelmorph_amd import metrics

    img_pairs = vxm.py.utils.read_pair_list(args.pairs, prefix=args.img_prefix, suffix=args.img_suffix)
    seg_pairs = vxm.py.utils.read_pair_list(args.pairs, prefix=args.seg_prefix, suffix=args.seg_suffix)
    labels = np.load(args.labels) if args.labels else None
    dev = torch.device('cuda', int(args.gpu))
    torch.cuda.set_device(dev)

    def load(path, np_var, multichannel=False):
        """[*vol] (or [*vol, C] with --multichannel) -> [1, C, *vol] fp32 on the device"""
        vol = np.asarray(vxm.py.utils.load_volfile(path, np_var=np_var))
        vol = np.moveaxis(vol, -1, 0) if multichannel else vol[None]
        return torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32))[None].to(dev)

    model = vxm.networks.VxmDense.load(args.model, dev)
    model.to(dev)
    model.eval()

    reg_times, dice_means = [], []
    with torch.no_grad():
        for i in range(len(img_pairs)):
            moving_vol, fixed_vol = load(img_pairs[i][0], 'vol', args.multichannel), load(img_pairs[i][1], 'vol', args.multichannel)
            moving_seg, fixed_seg = load(seg_pairs[i][0], 'seg'), load(seg_pairs[i][1], 'seg')

            torch.cuda.synchronize(dev)
            start = time.time()
            _, warp = model(moving_vol, fixed_vol, registration=True)
            torch.cuda.synchronize(dev)
            reg_time = time.time() - start
            if i != 0:                                     # the first prediction carries the one-off set-up (test.py:104-106)
                reg_times.append(reg_time)

            if labels is None:       # the reference takes the union of the WARPED and the fixed map (py/utils.py:275-277): two launches
                warped_seg = vxm.layers.SpatialTransformer(moving_seg.shape[2:], mode='nearest').to(dev)(moving_seg, warp)
                overlap = metrics.dice(warped_seg, fixed_seg)
            else:
                overlap = metrics.warped_dice(moving_seg, warp, fixed_seg, labels)
            dice_means.append(np.mean(overlap))
            print('Pair %d    Reg Time: %.4f    Dice: %.4f +/- %.4f' % (i + 1, reg_time, np.mean(overlap), np.std(overlap)))
            if args.jacobian:
                print('Pair %d    non-positive Jacobian fraction: %.6f' % (i + 1, metrics.nonpositive_jacobian_fraction(warp)))

    print()
    print('Avg Reg Time: %.4f +/- %.4f  (skipping first prediction)' % (np.mean(reg_times), np.std(reg_times)))
    print('Avg Dice: %.4f +/- %.4f' % (np.mean(dice_means), np.std(dice_means)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
