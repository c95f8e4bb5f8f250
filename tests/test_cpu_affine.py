"""CPU side of the affine transforms (csrc/affine.hip, voxelmorph_amd/torch/transforms.py): the float64 arbiter of tests/affine_cases.py agrees
with an independent restatement of the reference's formula, the matrix helpers are right, and the host refuses what it must."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import affine_cases as ac                         # noqa: E402
import voxelmorph_amd as vxm                      # noqa: E402
from voxelmorph_amd import _lib                   # noqa: E402

NEW_SYMBOLS = ("vxm_affine_shift3d_fwd", "vxm_affine_shift3d_bwd")


@pytest.fixture(scope="module")
def noise():
    return {r[0]: ac.noise_arrays(r) for r in ac.NOISE}


def test_lattice_row_is_exact_in_fp32():
    a = ac.lattice_arrays()
    sh, _ = ac.shift_arbiter(a["mat"], a["size"], True, a["flow"])
    assert np.array_equal(2 * sh, np.round(2 * sh)) and np.array_equal(sh.astype(np.float32).astype(np.float64), sh)


def _shift_restated(mat, shape, shift_center, warp_right):
    """float64 numpy restatement of voxelmorph/tf/utils/utils.py:677-695 (mesh, optional warp_right, matrix product, minus mesh), channels first"""
    mat = np.asarray(mat, np.float64)
    mesh = [np.arange(s, dtype=np.float64) for s in shape]
    if shift_center:
        mesh = [m - 0.5 * (s - 1) for m, s in zip(mesh, shape)]
    mesh = np.stack([m.reshape(-1) for m in np.meshgrid(*mesh, indexing="ij")])          # N x nb_voxels
    B = warp_right.shape[0] if warp_right is not None else mat.shape[0]
    outs = []
    for b in range(B):
        m = mat[b if mat.shape[0] > 1 else 0]
        out = mesh
        if warp_right is not None:
            out = out + np.asarray(warp_right[b], np.float64).reshape(3, -1)
        out = m[:3, :-1] @ out + m[:3, -1:]
        outs.append((out - mesh).reshape((3,) + tuple(shape)))
    return np.stack(outs)


@pytest.mark.parametrize("name", ac.NOISE_IDS)
def test_shift_arbiter_equals_the_restated_reference_formula(noise, name):
    a = noise[name]
    for v in ac.VARIANTS:
        mat, flow = ac.variant(a, v)
        for sc in (True, False):
            got, _ = ac.shift_arbiter(mat, a["size"], sc, flow)
            assert np.abs(got - _shift_restated(mat, a["size"], sc, flow)).max() < 1e-12, (name, v, sc)


def test_compose_of_matrices_is_the_matrix_product_and_inversion_is_right():
    rng = np.random.default_rng(7)
    a = np.eye(4)[None, :3] + 0.2 * rng.standard_normal((3, 3, 4))
    b = np.eye(4)[None] + 0.2 * rng.standard_normal((3, 4, 4))
    b[:, 3] = (0, 0, 0, 1)
    sq = lambda m: np.concatenate([m, np.broadcast_to([[[0, 0, 0, 1.0]]], (m.shape[0], 1, 4))], 1) if m.shape[1] == 3 else m
    got = vxm.utils.compose([torch.from_numpy(a), torch.from_numpy(b)])
    assert tuple(got.shape) == (3, 3, 4) and np.abs(got.numpy() - (sq(a) @ sq(b))[:, :3]).max() < 1e-14      # applied first = leftmost factor
    three = vxm.utils.compose([torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(a[:1])])
    assert np.abs(three.numpy() - (sq(a) @ sq(b) @ sq(a[:1]))[:, :3]).max() < 1e-13
    for m in (a, b):
        inv = vxm.utils.invert_affine(torch.from_numpy(m))
        assert inv.shape == m.shape and inv.dtype == torch.float64
        assert np.abs(inv.numpy() - np.linalg.inv(sq(m))[:, :m.shape[1]]).max() < 1e-12
        assert np.abs(vxm.layers.InvertAffine()(torch.from_numpy(m)).numpy() - inv.numpy()).max() == 0
    m = torch.from_numpy(a).requires_grad_()
    vxm.utils.invert_affine(m).sum().backward()                                  # differentiable, closed form
    assert torch.isfinite(m.grad).all() and float(m.grad.abs().max()) > 0
    assert torch.equal(vxm.utils.make_square_affine(torch.from_numpy(a))[:, 3], torch.tensor([[0, 0, 0, 1.0]] * 3, dtype=torch.float64))
    sh = vxm.utils.affine_remove_identity(torch.from_numpy(a))
    assert np.abs(sh.numpy() - (a - np.eye(4)[:3])).max() == 0 and np.abs(vxm.utils.affine_add_identity(sh).numpy() - a).max() < 1e-15
    assert np.abs(vxm.utils.rescale_affine(torch.from_numpy(a), 2.0).numpy() - np.concatenate([a[..., :3], 2 * a[..., 3:]], -1)).max() == 0
    assert vxm.utils.is_affine_shape((3, 4)) and vxm.utils.is_affine_shape((4, 4)) and not vxm.utils.is_affine_shape((3, 8, 8, 8))
    with pytest.raises(ValueError):
        vxm.utils.is_affine_shape((5, 6))


def test_new_symbols_layers_and_utils_exist():
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES, s
    h = _lib.lib()
    assert h.vxm_version() >= 505
    p = 16                                                   # never dereferenced: the argument checks come first
    assert h.vxm_affine_shift3d_fwd(p, 2, None, p, 3, 4, 4, 4, 1, None) == 1          # Bm neither 1 nor B
    assert h.vxm_affine_shift3d_fwd(p, 1, None, p, 1, 4, 4, 4, 2, None) == 2          # shift_center neither 0 nor 1
    assert h.vxm_affine_shift3d_fwd(None, 1, None, p, 1, 4, 4, 4, 1, None) == 3
    assert h.vxm_affine_shift3d_bwd(p, 1, p, None, 1, 4, 4, 4, None) == 3
    assert h.vxm_affine_shift3d_bwd(p, 1, p, p, 1, 0, 4, 4, None) == 1
    for name in ("AffineToDenseShift", "ComposeTransform", "InvertAffine"):
        assert hasattr(vxm.layers, name), name
    for name in ("transform", "affine_to_dense_shift", "compose", "invert_affine", "make_square_affine", "affine_add_identity",
                 "affine_remove_identity", "rescale_affine", "is_affine_shape", "affine_warp", "AffineShiftFn"):
        assert hasattr(vxm.utils, name), name
    lay = vxm.layers.AffineToDenseShift((4, 5, 6))
    assert lay.shape == (4, 5, 6) and lay.shift_center is True
    c = vxm.layers.ComposeTransform()
    assert (c.interp_method, c.shift_center, c.shape) == ("linear", True, None)


def test_affine_ops_refuse_cpu_tensors_planar_inputs_and_other_dtypes():
    eye = torch.eye(4)[None, :3]
    vol, field = torch.zeros(1, 1, 4, 5, 6), torch.zeros(1, 3, 4, 5, 6)
    calls = [lambda: vxm.layers.SpatialTransformer((4, 5, 6))(vol, eye),
             lambda: vxm.utils.transform(vol, eye),
             lambda: vxm.utils.transform(vol, torch.eye(4)[None]),
             lambda: vxm.utils.affine_to_dense_shift(eye, (4, 5, 6)),
             lambda: vxm.layers.AffineToDenseShift((4, 5, 6))(eye),
             lambda: vxm.utils.compose([eye, field]),
             lambda: vxm.layers.ComposeTransform()([field, eye]),
             lambda: vxm.utils.compose([field, field])]
    for f in calls:
        with pytest.raises(_lib.VxmHipError, match="no CPU fallback"):
            f()
    with pytest.raises(_lib.VxmHipError):
        vxm.utils.transform(vol.double(), eye.double())
    eye2 = torch.eye(3)[None, :2]
    with pytest.raises(NotImplementedError, match="2-D"):
        vxm.layers.SpatialTransformer((5, 6))(torch.zeros(1, 1, 5, 6), eye2)
    with pytest.raises(NotImplementedError):
        vxm.utils.transform(torch.zeros(1, 1, 5, 6), eye2)
    with pytest.raises(NotImplementedError):
        vxm.utils.affine_to_dense_shift(eye2, (5, 6))
    with pytest.raises(NotImplementedError):
        vxm.utils.transform(vol, eye2)
    with pytest.raises(ValueError):
        vxm.utils.transform(vol, eye, interp_method="cubic")
    with pytest.raises(ValueError):
        vxm.utils.compose([])
    with pytest.raises(NotImplementedError, match="output shape"):
        vxm.utils.transform(vol, eye, shape=(6, 5, 4))


def test_scripts_list_the_new_flags():
    for script, flags in (("warp.py", ("--moving", "--warp", "--moved", "--interp", "--gpu", "--multichannel", "--affine")),
                          ("register.py", ("--affine",))):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--help"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        for f in flags:
            assert f in out.stdout, (script, f)
