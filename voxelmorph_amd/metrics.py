"""Evaluation metrics on the device: the two numbers a registration is judged by.

`dice` is the reference's per-label hard Dice (`voxelmorph/py/utils.py:265-287`), `jacobian_determinant` its Jacobian determinant of a
displacement field (`py/utils.py:473-516`); `warped_dice` is the evaluation protocol of `scripts/tf/test.py:109-112` (nearest-neighbour
warp of the moving segmentation, Dice against the fixed one) in one kernel launch.  All of them run the kernels of csrc/metrics.hip through
include/vxm_hip.h: the label maps are read once for all labels together, the determinant is one pass over the field.  There is no CPU or
ATen fallback; a tensor that is not on a HIP device raises.

The kernels return INTEGER counts; Dice is formed from them in float64 on the host exactly as the reference forms it (`2 * inter /
max(|a| + |b|, eps)`), so the values equal the reference's bit for bit.
"""
import numpy as np
import torch

from ._lib import VxmHipError, call, ptr, require_device, stream

LABELS_MAX = 1024                      # VXM_LABELS_MAX of include/vxm_hip.h
_EXACT_INT = 1 << 24                   # integers up to here are exact in fp32
_label_cache = {}


def _device():
    if not torch.cuda.is_available():
        raise VxmHipError("voxelmorph_amd runs on an MI355X (HIP) device only; there is no CPU fallback.")
    return torch.device("cuda", torch.cuda.current_device())


def _as_f32_device(x, what, device=None):
    """numpy array or device tensor -> contiguous fp32 device tensor holding the same VALUES (integers are checked against 2^24, float64
    against its fp32 round trip), so that `==` on the device decides what `==` decides on the caller's array."""
    if isinstance(x, np.ndarray) or not torch.is_tensor(x):
        x = np.asarray(x)
        if x.dtype == np.bool_:
            x = x.astype(np.float32)
        elif x.dtype.kind in "iu":
            if x.size and int(np.abs(x.astype(np.int64, copy=False)).max()) >= _EXACT_INT:
                raise ValueError("%s: integer values of magnitude >= 2^24 are not exact in fp32" % what)
            x = x.astype(np.float32)
        elif x.dtype.kind == "f":
            y = x.astype(np.float32)
            if x.dtype.itemsize > 4 and not np.array_equal(y.astype(x.dtype), x, equal_nan=True):
                raise ValueError("%s: values that fp32 cannot hold exactly" % what)
            x = y
        else:
            raise TypeError("%s: dtype %s" % (what, x.dtype))
        return torch.from_numpy(np.ascontiguousarray(x)).to(device or _device())
    if not x.is_cuda:
        raise VxmHipError("voxelmorph_amd runs on an MI355X (HIP) device only; got a %s tensor. "
                          "Move the inputs with .to('cuda'); there is no CPU fallback." % x.device)
    if x.dtype != torch.float32:
        if x.dtype.is_floating_point:
            y = x.float()
            if x.dtype == torch.float64 and not bool(((y.double() == x) | (x != x)).all()):
                raise ValueError("%s: values that fp32 cannot hold exactly" % what)
            x = y
        else:
            if x.numel() and x.dtype != torch.bool and int(x.long().abs().max()) >= _EXACT_INT:
                raise ValueError("%s: integer values of magnitude >= 2^24 are not exact in fp32" % what)
            x = x.float()
    return x.contiguous()


def _device_labels(labels, device):
    """strictly increasing fp32 label list on `device` (uploaded once per list and device) and its length"""
    if torch.is_tensor(labels):
        if labels.is_cuda:                     # the caller vouches for a strictly increasing fp32 list: checking it would synchronise
            require_device(labels)
            if labels.dim() != 1:
                raise ValueError("labels: a 1-D list, got shape %s" % (tuple(labels.shape),))
            return labels.contiguous(), labels.numel()
        labels = labels.numpy()
    lab = np.asarray(labels, dtype=np.float64).reshape(-1)
    if not (1 <= lab.size <= LABELS_MAX):
        raise VxmHipError("label_overlap: %d labels (1 .. %d)" % (lab.size, LABELS_MAX))
    if not np.all(lab[1:] > lab[:-1]) or np.isnan(lab).any():
        raise ValueError("label_overlap: labels must be strictly increasing (dice() takes them in any order)")
    l32 = lab.astype(np.float32)
    if not np.array_equal(l32.astype(np.float64), lab):
        raise ValueError("label_overlap: labels that fp32 cannot hold exactly")
    key = (l32.tobytes(), device.index)
    t = _label_cache.get(key)
    if t is None:
        if len(_label_cache) >= 64:
            _label_cache.clear()
        t = _label_cache[key] = torch.from_numpy(l32).to(device)
    return t, lab.size


def label_overlap(a, b, labels):
    """counts [B, L, 3] (int64, on the device, no synchronisation) = {|a == l and b == l|, |a == l|, |b == l|} for every label l of `labels`
    (strictly increasing: a sequence, or an fp32 device tensor the caller vouches for) over the fp32 device label maps a, b [B, ...].
    One pass over the maps for all labels together (vxm_label_overlap)."""
    require_device(a, b)
    if a.shape != b.shape or a.dim() < 1 or a.numel() == 0:
        raise ValueError("label_overlap: maps of shapes %s and %s" % (tuple(a.shape), tuple(b.shape)))
    a, b = a.contiguous(), b.contiguous()
    lab, L = _device_labels(labels, a.device)
    B = a.shape[0]
    counts = torch.empty((B, L, 3), dtype=torch.int64, device=a.device)
    call("vxm_label_overlap", ptr(a), ptr(b), ptr(lab), L, ptr(counts), B, a.numel() // B, stream())
    return counts


def _label_plan(labels, include_zero):
    """the reference's label handling (py/utils.py:278-279) -> (labels in the caller's order, the sorted distinct ones the device can
    search, index of each of the caller's labels in that list or -1)"""
    labels = np.asarray(labels).reshape(-1)
    if not include_zero:
        labels = np.delete(labels, np.argwhere(labels == 0))
    lab64 = labels.astype(np.float64)
    ok = ~np.isnan(lab64) & (lab64.astype(np.float32).astype(np.float64) == lab64)     # any other label equals no fp32 voxel
    uniq = np.unique(lab64[ok])                                                        # sorted; -0.0 and 0.0 are one label
    where = np.full(lab64.shape, -1, dtype=np.int64)
    if uniq.size:
        pos = np.clip(np.searchsorted(uniq, lab64), 0, uniq.size - 1)
        where = np.where(ok & (uniq[pos] == lab64), pos, -1)
    return labels, uniq, where


def _dice_from_counts(counts, where):
    """[B, L, 3] int64 host counts -> [B, len(where)] float64, the arithmetic of py/utils.py:283-286"""
    out = np.zeros((counts.shape[0], where.size))
    eps = np.finfo(float).eps
    for k, j in enumerate(where):
        if j >= 0:
            out[:, k] = (2 * counts[:, j, 0]) / np.maximum(counts[:, j, 1] + counts[:, j, 2], eps)
    return out


def dice(array1, array2, labels=None, include_zero=False):
    """`voxelmorph.py.utils.dice` (py/utils.py:265-287): the Dice overlap of two label maps per label, as a float64 numpy vector in the
    caller's label order (duplicates included; label 0 dropped unless include_zero).  The maps may be device tensors or numpy arrays
    (integer dtypes are converted to fp32 after checking that magnitudes are below 2^24); they are read once for all labels, and the
    quotient is formed in float64 on the host from the integer counts, so it equals the reference's bit for bit (an absent label gives
    0 / eps = 0.0 as there).  labels=None takes the sorted union of the values of both maps as the reference does -- through
    torch.unique, an ATen pass that is off the measured path; pass the label list where time matters."""
    dev = array1.device if torch.is_tensor(array1) and array1.is_cuda else (array2.device if torch.is_tensor(array2) and array2.is_cuda else None)
    a, b = _as_f32_device(array1, "dice: array1", dev), _as_f32_device(array2, "dice: array2", dev)
    if a.shape != b.shape:
        raise ValueError("dice: arrays of shapes %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if labels is None:
        labels = np.unique(torch.cat([torch.unique(a), torch.unique(b)]).cpu().numpy().astype(np.float64))      # :276-277
    labels, uniq, where = _label_plan(labels, include_zero)
    if a.numel() == 0 or uniq.size == 0:
        return np.zeros(labels.size)
    counts = label_overlap(a.reshape(1, -1), b.reshape(1, -1), uniq)          # more than LABELS_MAX distinct labels: raises
    return _dice_from_counts(counts.cpu().numpy(), where)[0]


def warped_dice(moving_seg, flow, fixed_seg, labels, return_warped=False, include_zero=False):
    """The evaluation step of scripts/tf/test.py:109-112 in one launch (vxm_warp3d_label_overlap): nearest-neighbour warp of moving_seg
    [B, 1, D, H, W] (or [D, H, W]) by flow [B, 3, D, H, W] with the bit-exact transformer arithmetic, and `dice` of the result against
    fixed_seg for `labels` (required: a union over a map that is never written cannot be taken).  Returns the float64 Dice vector ([B, n]
    for B > 1), and the warped map too with return_warped -- the same values as SpatialTransformer(mode='nearest') followed by `dice`."""
    require_device(flow)
    seg = _as_f32_device(moving_seg, "warped_dice: moving_seg", flow.device)
    fix = _as_f32_device(fixed_seg, "warped_dice: fixed_seg", flow.device)
    flow = flow.contiguous()
    if flow.dim() != 5 or flow.shape[1] != 3:
        raise ValueError("warped_dice: flow of shape %s (expected [B, 3, D, H, W])" % (tuple(flow.shape),))
    B, _, D, H, W = flow.shape
    if seg.numel() != B * D * H * W or fix.numel() != B * D * H * W:
        raise ValueError("warped_dice: segmentations of shapes %s / %s do not match flow %s" % (tuple(seg.shape), tuple(fix.shape), tuple(flow.shape)))
    if labels is None:
        raise ValueError("warped_dice: a label list is required")
    labels, uniq, where = _label_plan(labels, include_zero)
    if uniq.size > LABELS_MAX:
        raise VxmHipError("warped_dice: %d labels (1 .. %d)" % (uniq.size, LABELS_MAX))
    warped = torch.empty((B, 1, D, H, W), dtype=torch.float32, device=flow.device) if return_warped else None
    if uniq.size == 0 and not return_warped:
        out = np.zeros((B, labels.size))
    else:
        lab, L = _device_labels(uniq if uniq.size else np.zeros(1), flow.device)
        counts = torch.empty((B, L, 3), dtype=torch.int64, device=flow.device)
        call("vxm_warp3d_label_overlap", ptr(seg), ptr(flow), ptr(fix), ptr(warped), ptr(lab), L, ptr(counts), B, D, H, W, stream())
        out = _dice_from_counts(counts.cpu().numpy(), where) if uniq.size else np.zeros((B, labels.size))
    out = out[0] if B == 1 else out
    return (out, warped) if return_warped else out


def _field(disp):
    """device tensor [B, nd, *vol] or [nd, *vol] -> ([B, nd, *vol] contiguous, nd, had a batch axis)"""
    require_device(disp)
    s = tuple(disp.shape)
    if disp.dim() == 5 and s[1] == 3:
        return disp.contiguous(), 3, True
    if disp.dim() == 3 and s[0] == 2:
        return disp.contiguous()[None], 2, False
    if disp.dim() == 4:
        vol3, img2 = s[0] == 3, s[1] == 2
        if vol3 and img2:
            raise ValueError("jacobian_determinant: shape %s is both an unbatched volume field [3, D, H, W] and a batch of planar fields "
                             "[B, 2, H, W]; add the batch axis" % (s,))
        if vol3:
            return disp.contiguous()[None], 3, False
        if img2:
            return disp.contiguous(), 2, True
    raise ValueError("jacobian_determinant: displacement of shape %s (expected [B, nd, *vol] or [nd, *vol] with nd = len(vol) in (2, 3))" % (s,))


def _jacdet(f, nd, det, stats):
    B, vol = f.shape[0], f.shape[2:]
    call("vxm_jacdet3d" if nd == 3 else "vxm_jacdet2d", ptr(f), ptr(det), ptr(stats), B, *vol, stream())


def jacobian_determinant(disp):
    """`voxelmorph.py.utils.jacobian_determinant` (py/utils.py:473-516): det(I + grad disp) with np.gradient's differences, one kernel pass.
    A device tensor in the model's layout, [B, nd, *vol] or [nd, *vol], returns a device tensor [B, *vol] / [*vol]; a numpy array in the
    reference's layout [*vol, nd] returns numpy."""
    if not torch.is_tensor(disp):
        d = np.asarray(disp)
        if d.ndim not in (3, 4) or d.shape[-1] != d.ndim - 1:
            raise ValueError("jacobian_determinant: flow has to be 2D or 3D, [*vol_shape, nb_dims]; got %s" % (d.shape,))
        t = torch.from_numpy(np.ascontiguousarray(np.moveaxis(d, -1, 0), dtype=np.float32)).to(_device())
        return jacobian_determinant(t).cpu().numpy()
    f, nd, batched = _field(disp)
    det = torch.empty((f.shape[0],) + tuple(f.shape[2:]), dtype=torch.float32, device=f.device)
    _jacdet(f, nd, det, None)
    return det if batched else det[0]


def nonpositive_jacobian(disp):
    """int64 device tensor [B, 2] ([2] without a batch axis) = (number of voxels with det <= 0, number with a non-finite det) of
    `jacobian_determinant(disp)`, without writing the determinant and without synchronising."""
    f, nd, batched = _field(disp)
    stats = torch.empty((f.shape[0], 2), dtype=torch.int64, device=f.device)
    _jacdet(f, nd, None, stats)
    return stats if batched else stats[0]


def nonpositive_jacobian_fraction(disp):
    """share of voxels at which the deformation folds (det <= 0), over the whole batch, as a float"""
    f, nd, _ = _field(disp)
    stats = torch.empty((f.shape[0], 2), dtype=torch.int64, device=f.device)
    _jacdet(f, nd, None, stats)
    return int(stats.cpu().numpy()[:, 0].sum()) / float(f.numel() // nd)
