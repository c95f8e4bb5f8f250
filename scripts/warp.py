#!/usr/bin/env python
"""Apply a saved transform to an image on MI355X -- the command line of the reference's `scripts/tf/warp.py` (:36-45: --moving --warp --moved
--interp --gpu --multichannel), plus `--affine FILE`: a 3 x 4 or 4 x 4 voxel-space matrix (identity = no motion, applied about the volume's
centre) in `.npy` or whitespace text.  `--warp` is a dense displacement field [3, D, H, W] in voxels, as `register.py --warp` writes it; it
is optional here.  With both options the image is resampled ONCE, at matrix (p + warp(p)) -- what applying the matrix to the image first and
the warp to the result would give with two interpolations (the matrix and the warp are composed into one dense transform first).  nii / nii.gz / mgz / npz / npy in,
nii / nii.gz / npz / npy out; the moved image is saved with the warp's affine, else the moving image's."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def load_affine(path):
    """a 3 x 4 or 4 x 4 matrix from .npy or whitespace text -> [1, 3, 4] float32"""
    m = np.load(path) if path.endswith('.npy') else np.loadtxt(path)
    m = np.asarray(m, dtype=np.float64)
    if m.shape not in ((3, 4), (4, 4)):
        raise ValueError("%s: expected a 3 x 4 or 4 x 4 matrix, got %s" % (path, m.shape))
    return np.ascontiguousarray(m[None, :3], dtype=np.float32)


def save_vol(arr, path, affine=None):
    from voxelmorph_amd import data as vdata
    if path.endswith('.npy'):
        np.save(path, arr)
    else:
        vdata.save_volfile(arr, path, affine)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--moving', required=True, help='moving image filename')
    p.add_argument('--warp', help='warp image filename: a dense displacement field [3, D, H, W] in voxels (optional with --affine)')
    p.add_argument('--affine', help='3 x 4 or 4 x 4 voxel-space matrix (.npy or whitespace text), applied to the image before the warp')
    p.add_argument('--moved', required=True, help='warped image output filename')
    p.add_argument('--interp', default='linear', help='interpolation method linear/nearest (default: linear)')
    p.add_argument('-g', '--gpu', default='0', help='GPU number (this path has no CPU fallback)')
    p.add_argument('--multichannel', action='store_true', help='specify that data has multiple channels (trailing feature axis)')
    args = p.parse_args(argv)
    if not args.warp and not args.affine:
        p.error('give --warp, --affine or both')

    import voxelmorph_amd as vxm
    from voxelmorph_amd import data as vdata
    dev = torch.device('cuda', int(args.gpu))
    torch.cuda.set_device(dev)

    vol, vol_affine = vdata.load_volfile(args.moving, ret_affine=True)
    vol = np.asarray(vol)
    vol = np.moveaxis(vol, -1, 0) if args.multichannel else vol[None]
    moving = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32))[None].to(dev)
    warp, out_affine = None, vol_affine
    if args.warp:
        w, out_affine = vdata.load_volfile(args.warp, ret_affine=True)
        warp = torch.from_numpy(np.ascontiguousarray(np.asarray(w), dtype=np.float32))[None].to(dev)
    with torch.no_grad():
        if args.affine:
            mat = torch.from_numpy(load_affine(args.affine)).to(dev)
            moved = vxm.utils.affine_warp(moving, mat, warp, interp_method=args.interp)          # one interpolation, with or without the warp
        else:
            moved = vxm.utils.transform(moving, warp, interp_method=args.interp)
    out = (moved[0].permute(1, 2, 3, 0) if args.multichannel else moved[0, 0]).cpu().numpy()
    save_vol(out, args.moved, out_affine)


if __name__ == '__main__':
    main()
