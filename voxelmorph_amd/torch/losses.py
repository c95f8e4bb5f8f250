"""Drop-in mirror of `voxelmorph/torch/losses.py` (reference) on the MI355X HIP kernels.

Every class keeps the reference's `loss(y_true, y_pred) -> 0-dim tensor` contract.
"""
import math

from . import functional as VF
from . import planar as VP


class NCC:
    """Local (over window) normalized cross correlation loss (reference: losses.py:7-67)."""

    def __init__(self, win=None):
        self.win = win

    def loss(self, y_true, y_pred):
        ndims = len(list(y_true.size())) - 2
        assert ndims in [1, 2, 3], "volumes should be 1 to 3 dimensions. found: %d" % ndims
        win = [9] * ndims if self.win is None else list(self.win)
        if len(win) != ndims or len(set(win)) != 1 or int(win[0]) % 2 == 0 or int(win[0]) != win[0]:
            # the reference pads every axis by win[0] // 2 whatever the other window sizes are (losses.py:31-36): windows that are not
            # odd and of one size change the SHAPE of the box sums -- the general separable passes follow that rule
            if len(win) != ndims:
                # (torch.ones([1, 1, *win]) of another rank makes the reference's conv raise)
                raise ValueError("NCC: %d window sizes for a %d-D volume" % (len(win), ndims))
            return VF.NCCWinFn.apply(y_true, y_pred, [int(w) for w in win])
        if ndims == 1:
            return VP.NCC1dFn.apply(y_true, y_pred, int(win[0]))
        if ndims == 2:
            return VP.NCC2dFn.apply(y_true, y_pred, int(win[0]))
        return VF.NCCFn.apply(y_true, y_pred, int(win[0]))


class MSE:
    """Mean squared error loss (reference: losses.py:70-76)."""

    def loss(self, y_true, y_pred):
        return VF.MSEFn.apply(y_true, y_pred)


class MutualInformation:
    """Global soft (Parzen-window) mutual information for pairs of different contrast (T1 / T2, MR / CT).

    The reference has this loss on its TensorFlow side only (voxelmorph/tf/losses.py:352-367), and that file shows the wrapper alone:
    `loss = -volumes(y_true, y_pred)` of a class of another package.  The algorithm is therefore this project's restatement of the
    formulation cited there (Guo's thesis; Hoffmann et al.), written out in include/vxm_hip.h and DESIGN.md; the float64 evaluation in the
    test table is its arbiter.  No bit parity with that other package is claimed.

    bin_centers: strictly increasing sequence of K floats, default linspace(min_clip, max_clip, nb_bins) with nb_bins = 32; 2 <= K <= 32.
    sigma = sigma_ratio * mean(diff(bin_centers)).  Inputs: two fp32 device tensors [B, ...] of one shape, at least 2 dimensions; every
    sample is flattened (channels included) and clamped to [min_clip, max_clip]; the loss is -mean over the batch of MI.  A NaN voxel
    makes the loss NaN.  Local (patch-wise) mutual information and more than 32 bins are out of scope."""

    MAX_BINS = 32

    def __init__(self, bin_centers=None, nb_bins=None, sigma_ratio=0.5, min_clip=0.0, max_clip=1.0):
        self.min_clip, self.max_clip = float(min_clip), float(max_clip)
        if not self.min_clip <= self.max_clip:
            raise ValueError("MutualInformation: min_clip %r above max_clip %r" % (min_clip, max_clip))
        if bin_centers is None:
            k = 32 if nb_bins is None else int(nb_bins)
            if k != (32 if nb_bins is None else nb_bins) or not 2 <= k <= self.MAX_BINS:
                raise ValueError("MutualInformation: nb_bins must be an integer in 2 .. %d, got %r" % (self.MAX_BINS, nb_bins))
            step = (self.max_clip - self.min_clip) / (k - 1)
            centres = [self.min_clip + step * i for i in range(k - 1)] + [self.max_clip]
        else:
            centres = [float(c) for c in bin_centers]
            if nb_bins is not None and int(nb_bins) != len(centres):
                raise ValueError("MutualInformation: nb_bins=%r but %d bin_centers" % (nb_bins, len(centres)))
        if not 2 <= len(centres) <= self.MAX_BINS:
            raise ValueError("MutualInformation: %d bins; 2 .. %d are implemented" % (len(centres), self.MAX_BINS))
        if any(not math.isfinite(c) for c in centres) or any(b <= a for a, b in zip(centres, centres[1:])):
            raise ValueError("MutualInformation: bin_centers must be finite and strictly increasing")
        self.sigma_ratio = float(sigma_ratio)
        sigma = self.sigma_ratio * (centres[-1] - centres[0]) / (len(centres) - 1)        # mean(diff(bin_centers))
        if not (sigma > 0 and math.isfinite(sigma)):
            raise ValueError("MutualInformation: sigma_ratio must be positive, got %r" % (sigma_ratio,))
        self.bin_centers = tuple(centres)
        self.sigma = sigma
        self.alpha = 1.0 / (2.0 * sigma * sigma)

    def loss(self, y_true, y_pred):
        return VF.MIFn.apply(y_true, y_pred, self.bin_centers, self.alpha, self.min_clip, self.max_clip)


class KL:
    """Kullback-Leibler divergence for probabilistic flows (the reference has it on its TensorFlow side only: voxelmorph/tf/losses.py:247-349).

    `y_pred` is the 6-channel tensor [B,6,D,H,W] of VxmDenseProbabilistic: channels 0..2 the mean of the velocity field, channels 3..5
    log sigma^2; `y_true` is not read (the reference takes only the shape from it).  The prior is the Gaussian Markov random field with precision
    prior_lambda * (degree - adjacency) on the 6-neighbour grid; the definition is written out in include/vxm_hip.h and DESIGN.md 4.13.
    3-D only in this version."""

    def __init__(self, prior_lambda, flow_vol_shape):
        self.prior_lambda = float(prior_lambda)
        self.flow_vol_shape = tuple(int(s) for s in flow_vol_shape)
        if len(self.flow_vol_shape) != 3:
            raise ValueError("KL: 3-D volumes only in this version, got flow_vol_shape %r" % (tuple(flow_vol_shape),))

    def loss(self, _, y_pred):
        if y_pred.dim() != 5:
            raise ValueError("KL: 3-D volumes only in this version: expected [B,6,D,H,W], got %s" % (tuple(y_pred.shape),))
        if tuple(y_pred.shape[2:]) != self.flow_vol_shape:
            raise ValueError("KL: y_pred lives on the grid %s, the loss was built for flow_vol_shape %s"
                             % (tuple(y_pred.shape[2:]), self.flow_vol_shape))
        return VF.KLFn.apply(y_pred, self.prior_lambda)


class Dice:
    """N-D dice for segmentation (reference: losses.py:79-90)."""

    def loss(self, y_true, y_pred):
        return VF.DiceFn.apply(y_true, y_pred)


class Grad:
    """N-D gradient loss (reference: losses.py:93-135)."""

    def __init__(self, penalty='l1', loss_mult=None):
        self.penalty = penalty
        self.loss_mult = loss_mult

    def loss(self, _, y_pred):
        if self.penalty != 'l1':
            assert self.penalty == 'l2', 'penalty can only be l1 or l2. Got: %s' % self.penalty
        mult = 1.0 if self.loss_mult is None else float(self.loss_mult)
        if y_pred.dim() == 4:
            return VP.GradLoss2dFn.apply(y_pred, self.penalty, mult)
        return VF.GradLossFn.apply(y_pred, self.penalty, mult)


def weighted_sum(terms, weights, running=None):
    """The reference loop's `loss += loss_function(y_true[n], y_pred[n]) * weights[n]` (scripts/torch/train.py:205-212) for terms already
    evaluated: one HIP launch forward, one backward, no ATen kernel (`a + w * b` on 0-dim tensors costs a mul and an add launch each way).
    `running`: optional device tensor of len(terms) + 1 floats that accumulates the weighted terms and the total (per-epoch logging)."""
    return VF.WeightedSumFn.apply(tuple(float(w) for w in weights), running, *terms)
