"""SynthMorph image synthesis from label maps on the device (`vxm.synth`; include/vxm_hip.h, "image synthesis from label maps").

SynthMorph (Hoffmann et al., IEEE TMI 41(3), 2022) trains a contrast-agnostic registration without acquired images: every step synthesises
two images of random contrast from label maps and scores the registration by the Dice of the warped one-hot maps.  The reference ships the
training script (`scripts/tf/train_synthmorph.py`) and the label-map generator (`generators.py:421-454`); the synthesis is a model of another
package.  This module is this project's restatement of it on the kernels of csrc/synth.hip:

    labels --warp by a smooth random diffeomorphism (nearest)--> warped labels
           --mean[label] + std[label] * noise--> raw image --separable Gaussian blur--> --* exp(smooth bias), clip to [0, 255],
           min-max normalise, ^ gamma--> image in [0, 1];      warped labels --recode, one-hot--> map

Everything runs under `no_grad`: generation is data.  Every random number is an input (`SynthDraws`), so a call is a deterministic function
of its arguments; `draw_params` makes the draws on the device with the ranges of `train_synthmorph.py` and the generator's defaults.
"""
import math

import numpy as np
import torch

from ._lib import call, lib, ptr, require_device, stream
from .torch import functional as VF

LABELS_MAX, PLANES_MAX, TAPS_MAX = 4096, 256, 25


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# --------------------------------------------------------------------------- label tables
class LabelTable:
    """The sorted input labels and where each goes: `labels` (sorted unique input labels), `out_labels` (sorted unique output labels: the
    planes of the one-hot map), `out_index[k]` = plane of input label k or -1 (dropped), `out_value[k]` = the output label of input label k
    (0 for a dropped one).  `out_label_list`: None (keep all), a list (keep these) or a dict {input label: output label}."""

    def __init__(self, in_label_list, out_label_list=None):
        labels = np.unique(np.asarray(in_label_list).reshape(-1))
        if labels.size < 1 or labels.size > LABELS_MAX:
            raise ValueError("1 .. %d input labels are implemented, got %d" % (LABELS_MAX, labels.size))
        if out_label_list is None:
            mapping = {v: v for v in labels.tolist()}
        elif isinstance(out_label_list, dict):
            mapping = {k: v for k, v in out_label_list.items()}
        else:
            mapping = {v: v for v in np.asarray(out_label_list).reshape(-1).tolist()}
        mapping = {k: v for k, v in mapping.items() if k in set(labels.tolist())}
        out_labels = np.unique(np.asarray(list(mapping.values()))) if mapping else np.zeros(0)
        if out_labels.size < 1:
            raise ValueError("no output label is among the input labels")
        pos = {v: i for i, v in enumerate(out_labels.tolist())}
        self.labels = labels.astype(np.float32)
        if not np.array_equal(self.labels.astype(np.float64), labels.astype(np.float64)) or np.any(np.diff(self.labels) <= 0):
            raise ValueError("label values must be exactly representable in fp32")
        self.out_labels = out_labels
        self.out_index = np.asarray([pos[mapping[v]] if v in mapping else -1 for v in labels.tolist()], dtype=np.int32)
        self.out_value = np.asarray([mapping.get(v, 0) for v in labels.tolist()], dtype=np.float32)
        self._dev = {}

    def device(self, dev):
        """(labels fp32 [L], out_index int32 [L], out_value fp32 [1,L], zeros fp32 [1,L]) on `dev`, uploaded once"""
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.labels).to(dev), torch.from_numpy(self.out_index).to(dev),
                              torch.from_numpy(self.out_value)[None].to(dev), torch.zeros((1, self.labels.size), device=dev))
        return self._dev[key]


def _table(in_label_list, out_label_list=None):
    return in_label_list if isinstance(in_label_list, LabelTable) else LabelTable(in_label_list, out_label_list)


def _label_map(labels, what):
    if labels.dim() != 5 or labels.shape[1] != 1:
        raise ValueError("%s: a label map [B,1,D,H,W] is expected, got %s" % (what, tuple(labels.shape)))


# --------------------------------------------------------------------------- the four kernels
def draw(labels, label_list, means, stds, noise):
    """image [B,1,*shape] = means[b, k] + stds[b, k] * noise with k the index of the voxel's label in the sorted `label_list`; 0 for a label
    that is not in the list (vxm_synth_draw_fwd).  means, stds: [B,L]; noise: [B,1,*shape]."""
    _label_map(labels, "draw")
    table = _table(label_list)
    B, L = labels.shape[0], table.labels.size
    if tuple(means.shape) != (B, L) or tuple(stds.shape) != (B, L):
        raise ValueError("means and stds must be [B,L] = %s, got %s and %s" % ((B, L), tuple(means.shape), tuple(stds.shape)))
    if tuple(noise.shape) != tuple(labels.shape):
        raise ValueError("noise %s does not match the label map %s" % (tuple(noise.shape), tuple(labels.shape)))
    require_device(labels, means, stds, noise)
    labels, means, stds, noise = _c(labels), _c(means), _c(stds), _c(noise)
    out = torch.empty_like(labels)
    call("vxm_synth_draw_fwd", ptr(labels), ptr(table.device(labels.device)[0]), ptr(means), ptr(stds), ptr(noise), ptr(out), L, B,
         labels[0].numel(), stream())
    return out


def onehot(labels, in_label_list, out_label_list=None):
    """[B,Lout,*shape] one-hot fp32 of a label map [B,1,*shape], recoded: the planes are the sorted output labels; a dropped or unknown
    label gives zeros in every plane (vxm_onehot_fwd)."""
    _label_map(labels, "onehot")
    table = _table(in_label_list, out_label_list)
    Lout = table.out_labels.size
    if Lout > PLANES_MAX:
        raise ValueError("1 .. %d output labels are implemented, got %d" % (PLANES_MAX, Lout))
    require_device(labels)
    labels = _c(labels)
    sorted_, index, _, _ = table.device(labels.device)
    out = torch.empty((labels.shape[0], Lout) + tuple(labels.shape[2:]), dtype=torch.float32, device=labels.device)
    call("vxm_onehot_fwd", ptr(labels), ptr(sorted_), ptr(index), table.labels.size, Lout, ptr(out), labels.shape[0], labels[0].numel(), stream())
    return out


def recode(labels, in_label_list, out_label_list=None):
    """the label map with every label replaced by its output label and dropped or unknown labels set to 0 (the draw kernel with the output
    labels as means and a zero std)"""
    _label_map(labels, "recode")
    table = _table(in_label_list, out_label_list)
    require_device(labels)
    labels = _c(labels)
    B = labels.shape[0]
    sorted_, _, value, zero = table.device(labels.device)
    out = torch.empty_like(labels)
    means, stds = _c(value.expand(B, -1)), _c(zero.expand(B, -1))     # named: both stay allocated until the launch is enqueued
    call("vxm_synth_draw_fwd", ptr(labels), ptr(sorted_), ptr(means), ptr(stds), ptr(labels), ptr(out), table.labels.size, B,
         labels[0].numel(), stream())
    return out


def gaussian_taps(sigma, T):
    """[B,3,T] fp32 taps of a Gaussian per sample and axis from sigma [B,3]: exp(-0.5 ((j - R) / sigma)^2) in float64, normalised to sum 1,
    then rounded to fp32; sigma <= 1e-6 gives a delta (no blur along that axis)."""
    T = int(T)
    if T < 1 or T > TAPS_MAX or T % 2 == 0:
        raise ValueError("T must be odd and in 1 .. %d, got %d" % (TAPS_MAX, T))
    sigma = torch.as_tensor(sigma)
    if sigma.dim() != 2 or sigma.shape[1] != 3:
        raise ValueError("sigma must be [B,3], got %s" % (tuple(sigma.shape),))
    s = sigma.to(torch.float64)[..., None]
    j = torch.arange(T, dtype=torch.float64, device=sigma.device) - (T - 1) // 2
    small = s <= 1e-6
    g = torch.exp(-0.5 * (j / torch.where(small, torch.ones_like(s), s)) ** 2)
    g = g / g.sum(-1, keepdim=True)
    delta = (j == 0).to(torch.float64).expand_as(g)
    return torch.where(small, delta, g).to(torch.float32).contiguous()


def blur(x, taps):
    """separable "same" convolution of x [B,C,D,H,W] with per-sample, per-axis taps [B,3,T], zero padding (vxm_blur3d_fwd)"""
    VF._vol3(x, "blur")
    B, C, D, H, W = (int(v) for v in x.shape)
    if taps.dim() != 3 or taps.shape[0] != B or taps.shape[1] != 3:
        raise ValueError("taps must be [B,3,T] with B = %d, got %s" % (B, tuple(taps.shape)))
    T = int(taps.shape[2])
    if T < 1 or T > TAPS_MAX or T % 2 == 0:
        raise ValueError("T must be odd and in 1 .. %d, got %d" % (TAPS_MAX, T))
    require_device(x, taps)
    x, taps = _c(x), _c(taps)
    out, work = torch.empty_like(x), torch.empty_like(x)
    need = int(lib().vxm_blur3d_workspace_bytes(T, B, C, D, H, W))
    assert need <= work.numel() * 4
    call("vxm_blur3d_fwd", ptr(x), ptr(taps), T, ptr(out), ptr(work), work.numel() * 4, B, C, D, H, W, stream())
    return out


def finish(x, log_bias, gamma):
    """out = ((y - min y) / (max y - min y)) ^ gamma[b] per sample, y = clamp(x * exp(log_bias), 0, 255) (no multiply for log_bias None);
    zeros for a constant y (vxm_synth_finish_fwd).  x, log_bias: [B,...]; gamma: [B]."""
    B = int(x.shape[0])
    if log_bias is not None and tuple(log_bias.shape) != tuple(x.shape):
        raise ValueError("log_bias %s does not match x %s" % (tuple(log_bias.shape), tuple(x.shape)))
    if tuple(gamma.shape) != (B,):
        raise ValueError("gamma must be [B] = (%d,), got %s" % (B, tuple(gamma.shape)))
    require_device(x, log_bias, gamma)
    x, gamma = _c(x), _c(gamma)
    log_bias = None if log_bias is None else _c(log_bias)
    V = x[0].numel()
    out = torch.empty_like(x)
    work = torch.empty(max(1, int(lib().vxm_synth_finish_workspace_bytes(B, V)) // 4), dtype=torch.float32, device=x.device)
    call("vxm_synth_finish_fwd", ptr(x), ptr(log_bias), ptr(gamma), ptr(out), ptr(work), work.numel() * 4, B, V, stream())
    return out


# --------------------------------------------------------------------------- smooth random fields
def perlin_extents(shape, scale):
    """extents of the noise that `draw_perlin` upsamples to `shape` for one scale: ceil(shape / scale)"""
    return tuple(int(math.ceil(s / float(scale))) for s in shape)


def draw_perlin(shape, scales, stds, noises):
    """A smooth random field [B,C,*shape]: for each scale s the noise `noises[k]` [B,C,*ceil(shape / s)] times its std `stds[k]` ([B] or a
    number), upsampled to `shape` (vxm_resize3d_fwd: linear, align_corners, values not rescaled), summed over the scales in order."""
    shape = tuple(int(s) for s in shape)
    if not (len(scales) == len(stds) == len(noises)) or len(scales) < 1:
        raise ValueError("one std and one noise tensor per scale are expected")
    total = None
    for scale, std, noise in zip(scales, stds, noises):
        VF._vol3(noise, "draw_perlin")
        if tuple(noise.shape[2:]) != perlin_extents(shape, scale):
            raise ValueError("the noise of scale %g must have extents %s, got %s" % (scale, perlin_extents(shape, scale), tuple(noise.shape[2:])))
        require_device(noise)
        B, C, D, H, W = (int(v) for v in noise.shape)
        std = std.to(noise.dtype).view(B, 1, 1, 1, 1) if torch.is_tensor(std) else float(std)
        low = _c(noise * std)
        up = torch.empty((B, C) + shape, dtype=noise.dtype, device=noise.device)
        call("vxm_resize3d_fwd", ptr(low), ptr(up), B, C, D, H, W, shape[0], shape[1], shape[2], 1.0, stream())
        total = up if total is None else total.add_(up)
    return total


# --------------------------------------------------------------------------- the random inputs of one image
class SynthDraws:
    """Every random input of one synthesised image (batch B, L input labels):
        means, stds   [B,L]            intensity statistics per label
        noise         [B,1,*shape]     N(0,1) per voxel
        vel_noise     list per warp scale of [B,3,*ceil(shape/2 / (s/2))], vel_std list of [B]   (None: no deformation)
        blur_sigma    [B,3], taps = gaussian_taps(blur_sigma, T)
        bias_noise    list per bias scale of [B,1,*ceil(shape / s)], bias_std list of [B]         (None: no bias field)
        gamma         [B]"""
    FIELDS = ("means", "stds", "noise", "vel_noise", "vel_std", "blur_sigma", "T", "bias_noise", "bias_std", "gamma")

    def __init__(self, means, stds, noise, vel_noise, vel_std, blur_sigma, T, bias_noise, bias_std, gamma):
        self.means, self.stds, self.noise, self.vel_noise, self.vel_std = means, stds, noise, vel_noise, vel_std
        self.blur_sigma, self.T, self.bias_noise, self.bias_std, self.gamma = blur_sigma, int(T), bias_noise, bias_std, gamma

    @property
    def taps(self):
        return gaussian_taps(self.blur_sigma, self.T)


def blur_taps_count(blur_std):
    """T = 2 round(3 blur_std) + 1: three standard deviations of the widest kernel on either side"""
    T = 2 * int(round(3 * float(blur_std))) + 1
    if T > TAPS_MAX:
        raise ValueError("blur_std = %g needs %d taps, at most %d are implemented" % (blur_std, T, TAPS_MAX))
    return T


def draw_params(generator, in_label_list, shape, batch_size=1, warp_std=0.5, warp_res=(16,), blur_std=1.0, bias_std=0.3, bias_res=(40,),
                gamma_std=0.25, mean_range=(25.0, 225.0), std_range=(5.0, 25.0), zero_background=0.2, device=None):
    """`SynthDraws` for one image of `batch_size` label maps of extents `shape`, drawn on the device from `generator` (a torch.Generator of
    that device) with the ranges that train_synthmorph.py passes and the generator's own defaults:
        means U(25, 225), the background label 0 U(0, 225); stds U(5, 25), background U(0, 25); background mean and std zeroed with
        probability 0.2; velocity noise N(0,1) times a std from U(0, warp_std) per scale; blur sigma per axis U(0, blur_std),
        T = 2 round(3 blur_std) + 1; bias noise N(0,1) times a std from U(0, bias_std) per scale; gamma = exp(N(0, gamma_std))."""
    table = _table(in_label_list)
    dev = torch.device(device) if device is not None else generator.device
    shape = tuple(int(s) for s in shape)
    B, L = int(batch_size), table.labels.size
    kw = dict(device=dev, generator=generator, dtype=torch.float32)

    def rand(*size):
        return torch.rand(size, **kw)

    def randn(*size):
        return torch.randn(size, **kw)
    bg = torch.from_numpy(table.labels == 0).to(dev)[None]
    lo_m = torch.where(bg, torch.zeros((), device=dev), torch.full((), float(mean_range[0]), device=dev))
    lo_s = torch.where(bg, torch.zeros((), device=dev), torch.full((), float(std_range[0]), device=dev))
    means = lo_m + (mean_range[1] - lo_m) * rand(B, L)
    stds = lo_s + (std_range[1] - lo_s) * rand(B, L)
    keep = ~(bg & (rand(B, 1) < zero_background))
    means, stds = means * keep, stds * keep
    vel_noise = vel_std = bias_noise = bias_s = None
    if warp_std > 0:
        half = tuple(s // 2 for s in shape)
        vel_noise = [randn(B, 3, *perlin_extents(half, r / 2.0)) for r in warp_res]
        vel_std = [warp_std * rand(B) for _ in warp_res]
    if bias_std > 0:
        bias_noise = [randn(B, 1, *perlin_extents(shape, r)) for r in bias_res]
        bias_s = [bias_std * rand(B) for _ in bias_res]
    return SynthDraws(means, stds, randn(B, 1, *shape), vel_noise, vel_std, blur_std * rand(B, 3), blur_taps_count(blur_std), bias_noise, bias_s,
                      torch.exp(gamma_std * randn(B)))


# --------------------------------------------------------------------------- the generator
def deform(labels, draws, warp_res=(16,), int_steps=5):
    """the label map [B,1,*shape] warped (nearest) by the diffeomorphism of `draws`: a smooth velocity field at half resolution
    (`draw_perlin`), integrated (vxm_vecint_fwd), upsampled x2 and applied -- one fused kernel where it takes the shapes"""
    if draws.vel_noise is None:
        return labels
    shape = tuple(int(s) for s in labels.shape[2:])
    if any(s % 2 for s in shape):
        raise ValueError("the deformation is drawn at half resolution: every extent must be even, got %s" % (shape,))
    half = tuple(s // 2 for s in shape)
    vel = draw_perlin(half, [r / 2.0 for r in warp_res], draws.vel_std, draws.vel_noise)
    disp = VF.VecIntFn.apply(vel, int_steps) if int_steps > 0 else vel
    if VF.warp_up_ok(labels, disp):
        return VF.WarpUpFn.apply(labels, disp, 2.0, "nearest", False)
    return VF.WarpFn.apply(labels, VF.ResizeFn.apply(disp, 2.0), "nearest")


def labels_to_image(labels, in_label_list, out_label_list=None, draws=None, warp_res=(16,), bias_res=(40,), int_steps=5, one_hot=True):
    """One synthesised image and its label map from label maps [B,1,*shape] (fp32 label values) and the random inputs `draws`:
    returns (image [B,1,*shape] in [0,1], map): map = the one-hot [B,Lout,*shape] of the WARPED labels recoded to `out_label_list` (None:
    all input labels; a list: these; a dict {input label: output label}; planes in sorted order of the output labels), or with
    one_hot=False the warped label map itself, recoded, with dropped labels set to 0."""
    if draws is None:
        raise ValueError("labels_to_image is deterministic: pass draws=draw_params(generator, ...)")
    _label_map(labels, "labels_to_image")
    table = _table(in_label_list, out_label_list)
    with torch.no_grad():
        warped = deform(labels, draws, warp_res, int_steps)
        image = draw(warped, table, draws.means, draws.stds, draws.noise)
        image = blur(image, draws.taps)
        log_bias = None if draws.bias_noise is None else draw_perlin(labels.shape[2:], bias_res, draws.bias_std, draws.bias_noise)
        image = finish(image, log_bias, draws.gamma)
        return image, (onehot(warped, table) if one_hot else recode(warped, table))
