"""The part of `voxelmorph/py/utils.py` that an evaluation needs, under the reference's path (`vxm.py.utils.*`): the file-list readers
(:32-66), the volume readers / writers (:69-158, from voxelmorph_amd/data.py), the label-map reader of SynthMorph (:161-199) and the two metrics (:265-287, :473-516), which run on the
device (voxelmorph_amd/metrics.py)."""
import glob
import os

import numpy as np

from ..data import load_volfile, save_volfile  # noqa: F401
from ..metrics import dice, jacobian_determinant  # noqa: F401


def read_file_list(filename, prefix=None, suffix=None):
    """Reads a list of files from a line-separated text file (py/utils.py:32-48): blank lines dropped, names stripped."""
    with open(filename, 'r') as file:
        filelist = [line.strip() for line in file if line.strip()]
    if prefix is not None:
        filelist = [prefix + f for f in filelist]
    if suffix is not None:
        filelist = [f + suffix for f in filelist]
    return filelist


def read_pair_list(filename, delim=None, prefix=None, suffix=None):
    """Reads a list of registration file pairs from a line-separated text file (py/utils.py:51-66); `delim` separates the names of a
    line (default: any whitespace); prefix / suffix are added to every name."""
    pairlist = [f.split(delim) for f in read_file_list(filename)]
    if prefix is not None:
        pairlist = [[prefix + f for f in pair] for pair in pairlist]
    if suffix is not None:
        pairlist = [[f + suffix for f in pair] for pair in pairlist]
    return pairlist


def load_labels(arg, ext=('.nii.gz', '.nii', '.mgz', '.npy', '.npz')):
    """Load label maps, return the sorted unique labels and the list of label maps (py/utils.py:161-199).  `arg`: a folder, a glob pattern
    or a list of these; files are kept by extension; the maps must be of an integer type and of one shape."""
    if not isinstance(arg, (tuple, list)):
        arg = [arg]
    files = [os.path.join(f, '*') if os.path.isdir(f) else f for f in map(str, arg)]
    files = sum((sorted(glob.glob(f)) for f in files), [])
    files = [f for f in files if f.endswith(tuple(ext))]
    if len(files) == 0:
        raise ValueError('no labels found for argument "%s"' % (arg,))
    label_maps = []
    shape = None
    for f in files:
        x = np.squeeze(load_volfile(f))
        if shape is None:
            shape = np.shape(x)
        if not np.issubdtype(x.dtype, np.integer):
            raise ValueError('file "%s" has non-integral data type' % f)
        if x.shape != shape:
            raise ValueError('shape %s of file "%s" is not %s' % (x.shape, f, shape))
        label_maps.append(x)
    return np.unique(label_maps), label_maps
