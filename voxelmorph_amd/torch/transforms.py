"""Affine transforms on the device (`vxm.utils`): apply a matrix to a volume, compose it with a dense warp, convert it to a dense
displacement field, invert it.

This project's restatement of the reference's TensorFlow-side toolkit (`voxelmorph/tf/utils/utils.py:96-174` transform, `:253-318` compose,
`:525-635` the affine helpers, `:638-699` affine_to_dense_shift); no bit parity with that package is claimed.  The definition the kernels
follow is pinned in include/vxm_hip.h (csrc/affine.hip).

Conventions: volumes and fields are `[B,C,D,H,W]` / `[B,3,D,H,W]` fp32 (channel a = the displacement along axis a in voxels, 'ij' indexing);
a matrix is `[Bm,3,4]` or `[Bm,4,4]` with Bm in {1, B} (Bm = 1: one matrix for the whole batch), a FULL matrix (identity = no motion).  The
last row of a 4 x 4 is ignored and gets a zero gradient.  The resampling and conversion functions run on the HIP device only; the
matrix-only helpers (`invert_affine`, `make_square_affine`, matrix x matrix `compose`, ...) are elementwise torch ops that run where the
tensor lives.

What is NOT here yet: a kernel that resamples a volume by the matrix itself (other output extents, the gradient of the matrix);
a matrix is applied through its dense field.
"""
import torch

from .. import profiler as _prof
from .._lib import call, ptr, require_device, stream
from .. import _lib
from . import functional as VF

_MODES = {"linear": 0, "bilinear": 0, "trilinear": 0, "nearest": 1}
_WARP_MODE = {0: "bilinear", 1: "nearest"}


def _mode(interp_method):
    if interp_method not in _MODES:
        raise ValueError("interp_method should be 'linear' or 'nearest', got %r" % (interp_method,))
    return _MODES[interp_method]


# --------------------------------------------------------------------------- matrix helpers (utils.py:525-635)
def validate_affine_shape(shape):
    """`shape` = (..., M, N + 1) with N in (2, 3) and M in (N, N + 1) (utils.py:539-553)"""
    ndim, rows = shape[-1] - 1, shape[-2]
    if ndim not in (2, 3):
        raise ValueError("Affine matrix must be 2D or 3D, got %dD" % ndim)
    if rows not in (ndim, ndim + 1):
        raise ValueError("%dD affine matrix must have %d or %d rows, got %d." % (ndim, ndim, ndim + 1, rows))


def is_affine_shape(shape):
    """does `shape` (WITHOUT the batch axis) describe an affine matrix (utils.py:525-536)?  (3, 4) and (4, 4) do; a field's (3, D, H, W) does not"""
    if len(shape) == 2 and shape[-1] != 1:
        validate_affine_shape(shape)
        return True
    return False


def _is_matrix(t):
    return t.dim() == 3 and is_affine_shape(tuple(t.shape[1:]))


def _mat3(mat, what):
    """[Bm,3,4] contiguous view of a 3-D matrix argument; 2-D matrices are refused (out of scope)"""
    if mat.dim() != 3:
        raise ValueError("%s: a matrix is [Bm,3,4] or [Bm,4,4], got %s" % (what, tuple(mat.shape)))
    validate_affine_shape(tuple(mat.shape))
    if mat.shape[-1] != 4:
        raise NotImplementedError("%s: 2-D affine matrices %s are not implemented on the MI355X path (3-D volumes only; DESIGN.md 4.12)"
                                  % (what, tuple(mat.shape)))
    return mat if mat.shape[1] == 3 else mat[:, :3, :]          # a 3 x 4 goes to the kernels as it is: no slice node, no ATen fill / copy in its backward


def make_square_affine(mat):
    """(..., N, N + 1) -> (..., N + 1, N + 1) by appending the row (0, ..., 0, 1) (utils.py:556-580)"""
    validate_affine_shape(tuple(mat.shape))
    if mat.shape[-2] == mat.shape[-1]:
        return mat
    row = torch.zeros(tuple(mat.shape[:-2]) + (1, mat.shape[-1]), dtype=mat.dtype, device=mat.device)
    row[..., -1] = 1
    return torch.cat((mat, row), dim=-2)


def _eye_rows(mat):
    rows, n = mat.shape[-2:]
    return torch.eye(n, dtype=mat.dtype, device=mat.device)[:rows]


def affine_add_identity(mat):
    """a 'shift' affine -> a full one (utils.py:583-594)"""
    return mat + _eye_rows(mat)


def affine_remove_identity(mat):
    """a full affine -> a 'shift' one (utils.py:597-608)"""
    return mat - _eye_rows(mat)


def rescale_affine(mat, factor):
    """scale the translation column by `factor` (utils.py:625-635)"""
    return torch.cat((mat[..., :-1], mat[..., -1:] * factor), dim=-1)


def invert_affine(mat):
    """inverse of a 3-D affine (..., M, 4), M in (3, 4), in closed form: the 3 x 3 adjugate over the determinant, elementwise torch ops
    where the tensor lives (differentiable; no solver library is loaded for a 3 x 3).  utils.py:611-622"""
    validate_affine_shape(tuple(mat.shape))
    if mat.shape[-1] != 4:
        raise NotImplementedError("invert_affine: 2-D affine matrices are not implemented (DESIGN.md 4.12)")
    rows = mat.shape[-2]
    a = [[mat[..., i, j] for j in range(3)] for i in range(3)]
    t = [mat[..., i, 3] for i in range(3)]
    c = [[a[(j + 1) % 3][(i + 1) % 3] * a[(j + 2) % 3][(i + 2) % 3] - a[(j + 1) % 3][(i + 2) % 3] * a[(j + 2) % 3][(i + 1) % 3]
          for j in range(3)] for i in range(3)]                       # c[i][j] = cofactor(j, i): the adjugate
    det = a[0][0] * c[0][0] + a[0][1] * c[1][0] + a[0][2] * c[2][0]
    inv = [[c[i][j] / det for j in range(3)] for i in range(3)]
    out_rows = []
    for i in range(3):
        ti = -(inv[i][0] * t[0] + inv[i][1] * t[1] + inv[i][2] * t[2])
        out_rows.append(torch.stack((inv[i][0], inv[i][1], inv[i][2], ti), dim=-1))
    if rows == 4:
        last = torch.zeros_like(out_rows[0])
        last[..., 3] = 1
        out_rows.append(last)
    return torch.stack(out_rows, dim=-2)


def _matmul_small(a, b):
    """batched product of two small square matrices by elementwise ops (no BLAS handle for a 4 x 4)"""
    return (a.unsqueeze(-1) * b.unsqueeze(-3)).sum(dim=-2)


# --------------------------------------------------------------------------- device ops
def _check_flow(flow, B, size, what):
    if flow is not None and tuple(flow.shape) != (B, 3) + tuple(size):
        raise ValueError("%s: the right-composed field %s does not match the output grid %s" % (what, tuple(flow.shape), (B, 3) + tuple(size)))


class AffineShiftFn(torch.autograd.Function):
    """shift[b,a,i] = (M (i - c + w(i)))[a] - (i[a] - c[a]): a matrix as a dense displacement field on the grid `size`, optionally
    right-composed with the field `flow` (vxm_affine_shift3d_fwd / _bwd; utils.py:638-699).  The batch is flow's, or mat's without one.
    Differentiable with respect to `flow`.  There is no kernel for the gradient of the matrix yet: a matrix that requires a gradient is
    refused, not differentiated some other way."""

    @staticmethod
    def forward(ctx, mat, flow, size, shift_center):
        require_device(mat, flow)
        mat = VF._c(mat)
        flow = None if flow is None else VF._c(flow)
        D, H, W = (int(v) for v in size)
        Bm = int(mat.shape[0])
        B = Bm if flow is None else int(flow.shape[0])
        if Bm not in (1, B):
            raise ValueError("%d matrices for a batch of %d (one per sample, or one for all)" % (Bm, B))
        _check_flow(flow, B, (D, H, W), "affine_to_dense_shift")
        shift = torch.empty((B, 3, D, H, W), dtype=mat.dtype, device=mat.device)
        with _prof.region("affine_shift3d_fwd", nbytes=4.0 * B * D * H * W * (3 + (3 if flow is not None else 0))):
            call("vxm_affine_shift3d_fwd", ptr(mat), Bm, ptr(flow), ptr(shift), B, D, H, W, int(bool(shift_center)), stream())
        ctx.save_for_backward(mat)
        ctx.args = (B, D, H, W, flow is not None)
        return shift

    @staticmethod
    def backward(ctx, gout):
        mat, = ctx.saved_tensors
        B, D, H, W, has_flow = ctx.args
        gflow = None
        if has_flow and ctx.needs_input_grad[1]:
            gout = VF._c(gout)
            gflow = torch.empty_like(gout)
            with _prof.region("affine_shift3d_bwd", nbytes=4.0 * B * D * H * W * 6):
                call("vxm_affine_shift3d_bwd", ptr(mat), int(mat.shape[0]), ptr(gout), ptr(gflow), B, D, H, W, stream())
        return None, gflow, None, None


def _vol3(t, what):
    if t.dim() != 5:
        raise NotImplementedError("%s: affine transforms are implemented for 3-D volumes [B,C,D,H,W]; got a %d-dimensional tensor "
                                  "(2-D images are out of scope, DESIGN.md 4.12)" % (what, t.dim()))


def affine_to_dense_shift(matrix, shape, shift_center=True, warp_right=None):
    """A matrix [Bm,3,4] / [Bm,4,4] as the dense displacement field [B,3,*shape] (utils.py:638-699): M (p - c) - (p - c), or, right-composed
    with the field `warp_right` [B,3,*shape], M (p - c + w(p)) - (p - c)."""
    m = _mat3(matrix, "affine_to_dense_shift")
    if len(tuple(shape)) != 3:
        raise NotImplementedError("affine_to_dense_shift: 3-D shapes only, got %s (DESIGN.md 4.12)" % (tuple(shape),))
    if warp_right is not None:
        _vol3(warp_right, "affine_to_dense_shift")
    if m.requires_grad and torch.is_grad_enabled():
        raise _lib.VxmHipError("affine_to_dense_shift: the gradient with respect to the matrix has no HIP kernel yet (DESIGN.md 4.12); "
                               "detach the matrix or run under torch.no_grad()")
    return AffineShiftFn.apply(m, warp_right, tuple(int(s) for s in shape), shift_center)


def affine_warp(vol, mat, warp_right=None, interp_method='linear', shift_center=True):
    """`vol` resampled at `mat (p + warp_right(p))` with ONE interpolation: what applying `mat` to the volume first and the dense field
    `warp_right` to the result would give with two.  Two launches: the matrix (and the field) become one dense transform in the shift kernel,
    which the SpatialTransformer kernel applies.  The output is on vol's own grid."""
    _vol3(vol, "affine_warp")
    mode = _WARP_MODE[_mode(interp_method)]
    m = _mat3(mat, "affine_warp")
    if warp_right is not None:
        _vol3(warp_right, "affine_warp")
    dense = affine_to_dense_shift(m, tuple(vol.shape[2:]), shift_center=shift_center, warp_right=warp_right)
    if dense.shape[0] != vol.shape[0]:
        dense = dense.expand((vol.shape[0],) + tuple(dense.shape[1:]))
    return VF.WarpFn.apply(vol, dense, mode)


def transform(vol, trf, interp_method='linear', shift_center=True, shape=None):
    """Apply the transform `trf` to `vol` [B,C,D,H,W] (utils.py:96-174): a dense field [B,3,D,H,W] on vol's grid, or a matrix [Bm,3,4] /
    [Bm,4,4], which is converted to a dense field on vol's grid first, as the reference does.  An output `shape` other than vol's own is not
    implemented (it needs the resampling kernel that takes the matrix itself)."""
    _vol3(vol, "transform")
    _mode(interp_method)
    if shape is not None and tuple(int(s) for s in shape) != tuple(vol.shape[2:]):
        raise NotImplementedError("transform: an output shape %s other than the volume's %s is not implemented (DESIGN.md 4.12)"
                                  % (tuple(shape), tuple(vol.shape[2:])))
    if trf.dim() == 3:
        return affine_warp(vol, trf, None, interp_method, shift_center)
    _vol3(trf, "transform")
    if tuple(trf.shape[2:]) != tuple(vol.shape[2:]):
        raise ValueError("transform: the dense field %s is not on the volume's grid %s" % (tuple(trf.shape), tuple(vol.shape)))
    return VF.WarpFn.apply(vol, trf, _WARP_MODE[_mode(interp_method)])


def compose(transforms, interp_method='linear', shift_center=True, shape=None):
    """One transform from a list of matrices and / or dense fields, in the order in which they would be applied to an image one after the
    other (utils.py:253-318): compose([A, B]) resamples like transform(transform(vol, A), B).  Dense unless every entry is a matrix.
      dense left of dense:   curr + warp(next, curr)            (the SpatialTransformer kernel plus an add)
      matrix left of dense:  the shift kernel with warp_right = curr
      dense left of matrix:  the matrix as a shift on next's grid (or `shape`), then the dense case
      matrix left of matrix: the 4 x 4 product"""
    if len(transforms) == 0:
        raise ValueError("Compose transform list cannot be empty")
    mode = _mode(interp_method)
    curr = None
    for nxt in reversed(list(transforms)):
        if curr is None:
            curr = nxt
            continue
        if not _is_matrix(nxt):
            _vol3(nxt, "compose")
            if _is_matrix(curr):
                curr = affine_to_dense_shift(curr, tuple(nxt.shape[2:]) if shape is None else shape, shift_center=shift_center)
            curr = curr + VF.WarpFn.apply(nxt, curr, _WARP_MODE[mode])
        elif not _is_matrix(curr):
            curr = affine_to_dense_shift(nxt, tuple(curr.shape[2:]), shift_center=shift_center, warp_right=curr)
        else:
            curr = _matmul_small(make_square_affine(nxt), make_square_affine(curr))[..., :-1, :]
    return curr
