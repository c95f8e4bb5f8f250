"""The affine kernels (csrc/affine.hip) through the layers and `vxm.utils`, i.e. the C ABI, against the float64 arbiter of
tests/affine_cases.py.  Gates: tools/affine_gates.py (profiles/pr10_affine_gates_cpu.txt) -- 4 x the error of the plain fp32 evaluation of the
same definition against the arbiter on exactly these inputs, the worst over the table, per class.  `pytest -s` prints every margin
(profiles/pr10_affine_gpu_tests.log)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import affine_cases as ac                         # noqa: E402

# tools/affine_gates.py, 4 x the largest fp32-vs-arbiter rel-L2 error of the class
GATE_SHIFT, GATE_SHIFT_GW = 2.93e-06, 1.68e-07
ROUNDTRIP_BOUND = 3.402e-02                       # 1.5 x the float64 arbiters' own round-trip interpolation error (same tool, same inputs)

ROWS = ac.NOISE_IDS + [ac.LATTICE[0]]
ROW_VARIANTS = [(r, v) for r in ROWS for v in ac.VARIANTS]


@pytest.fixture(scope="module")
def vxm():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    import voxelmorph_amd
    from voxelmorph_amd import _lib
    _lib.lib()
    return voxelmorph_amd


@pytest.fixture(scope="module")
def table():
    t = {r[0]: ac.noise_arrays(r) for r in ac.NOISE}
    t[ac.LATTICE[0]] = ac.lattice_arrays()
    return t


def G(x, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return t.requires_grad_() if grad else t


def N(t):
    return None if t is None else t.detach().cpu().numpy()


def run_shift(vxm, a, mat, flow):
    f = G(flow, True) if flow is not None else None
    sh = vxm.utils.affine_to_dense_shift(G(mat), a["size"], warp_right=f)
    if f is not None:
        sh.backward(G(a["gshift"][:sh.shape[0]]))
    return N(sh), N(f.grad) if f is not None else None


def check(name, what, got, want, gate):
    err = ac.rel_l2(got, want)
    print("%-32s %-9s rel-L2 %.3e  gate %.2e  margin %s" % (name, what, err, gate, "%.1fx" % (gate / err) if err else "exact"))
    assert np.isfinite(got).all() and err <= gate, (name, what, err, gate)


@pytest.mark.parametrize("row,v", ROW_VARIANTS, ids=["%s-%s" % rv for rv in ROW_VARIANTS])
def test_affine_shift_against_the_arbiter(vxm, table, row, v):
    a = table[row]
    mat, flow = ac.variant(a, v)
    B = a["gshift"].shape[0] if flow is not None else mat.shape[0]
    s64, gw64 = ac.shift_arbiter(mat, a["size"], True, flow, a["gshift"][:B])
    sh, gw = run_shift(vxm, a, mat, flow)
    name = "%s %s" % (row, v)
    check(name, "shift", sh, s64, GATE_SHIFT)
    if flow is not None:
        check(name, "shift-gw", gw, gw64, GATE_SHIFT_GW)
    if row == ac.LATTICE[0]:
        assert np.array_equal(sh, s64)                                 # every value exact in fp32
    sh2, gw2 = run_shift(vxm, a, mat, flow)                            # run to run: the same bits
    assert np.array_equal(sh, sh2) and (flow is None or np.array_equal(gw, gw2))
    if flow is None:
        assert np.array_equal(N(vxm.layers.AffineToDenseShift(a["size"])(G(mat))), sh)
        s0, _ = ac.shift_arbiter(mat, a["size"], False)
        check(name, "no centre", N(vxm.utils.affine_to_dense_shift(G(mat), a["size"], shift_center=False)), s0, GATE_SHIFT)


def test_square_matrix_gives_the_3x4_result_and_a_matrix_gradient_is_refused(vxm, table):
    from voxelmorph_amd._lib import VxmHipError
    a = table["noise_7x9x70"]
    sh3, gw3 = run_shift(vxm, a, a["mat"], a["flow"])
    last = np.tile(np.array([[[0.3, -2.0, 5.0, 7.0]]], dtype=np.float32), (a["mat"].shape[0], 1, 1))           # ignored, whatever it holds
    sh4, gw4 = run_shift(vxm, a, np.concatenate([a["mat"], last], axis=1), a["flow"])
    assert np.array_equal(sh4, sh3) and np.array_equal(gw4, gw3)
    with pytest.raises(VxmHipError, match="gradient with respect to the matrix"):       # no kernel for it: an error, not another route
        vxm.utils.affine_to_dense_shift(G(a["mat"], True), a["size"])
    with torch.no_grad():
        assert np.array_equal(N(vxm.utils.affine_to_dense_shift(G(a["mat"], True), a["size"], warp_right=G(a["flow"]))), sh3)


def test_compose(vxm, table):
    a = table["noise_7x9x70"]
    rng = np.random.default_rng(11)
    w1, w2 = G((0.6 * rng.standard_normal(a["flow"].shape)).astype(np.float32)), G(a["flow"])
    st = vxm.layers.SpatialTransformer(a["size"]).cuda()
    # dense left of dense: compose([w1, w2]) = w2 + warp(w1, w2), bit for bit
    assert torch.equal(vxm.utils.compose([w1, w2]), w2 + st(w1, w2))
    assert torch.equal(vxm.layers.ComposeTransform()([w1, w2]), w2 + st(w1, w2))
    m = G(a["mat"])
    # matrix left of dense: the shift kernel with warp_right; dense left of matrix: the matrix as a shift, then the dense case
    assert torch.equal(vxm.utils.compose([m, w2]), vxm.utils.affine_to_dense_shift(m, a["size"], warp_right=w2))
    sm = vxm.utils.affine_to_dense_shift(m, a["size"])
    assert torch.equal(vxm.utils.compose([w1, m]), sm + st(w1, sm))
    # three transforms: the list is folded from the right
    assert torch.equal(vxm.utils.compose([w1, m, w2]), vxm.utils.compose([w1, vxm.utils.compose([m, w2])]))
    # matrices only: stays a matrix
    mm = vxm.utils.compose([m, m])
    sq = np.concatenate([a["mat"].astype(np.float64), np.tile([[[0, 0, 0, 1.0]]], (a["mat"].shape[0], 1, 1))], axis=1)
    assert tuple(mm.shape) == tuple(m.shape) and np.abs(N(mm) - (sq @ sq)[:, :3]).max() < 1e-5
    # the gradient reaches the right-composed field through the composition
    w = G(a["flow"], True)
    vxm.utils.compose([m, w]).backward(G(a["gshift"]))
    _, gw64 = ac.shift_arbiter(a["mat"], a["size"], True, a["flow"], a["gshift"])
    check("compose([M, w])", "gw", N(w.grad), gw64, GATE_SHIFT_GW)


@pytest.mark.parametrize("row", ["channels_5x6x40", "noise_7x9x70"])
def test_a_matrix_is_applied_through_its_dense_field(vxm, table, row):
    """transform(vol, M), SpatialTransformer(src, M) and affine_warp(vol, M, w) are the dense transformer on the field of the shift kernel,
    bit for bit, in both modes; the composed call resamples ONCE (it equals transform by compose([M, w]))"""
    from voxelmorph_amd.torch import functional as VF
    a = table[row]
    s, w = G(a["src"]), G(a["flow"])
    for Bm in (a["mat"].shape[0], 1):
        m = G(a["mat"][:Bm])
        dense = vxm.utils.affine_to_dense_shift(m, a["size"])
        dense = dense.expand(s.shape[0], -1, -1, -1, -1).contiguous()
        for mode, interp in (("bilinear", "linear"), ("nearest", "nearest")):
            want = VF.WarpFn.apply(s, dense, mode)
            assert torch.equal(vxm.utils.transform(s, m, interp_method=interp), want)
            assert torch.equal(vxm.layers.SpatialTransformer(a["size"], mode).cuda()(s, m), want)
            both = vxm.utils.affine_warp(s, m, w, interp_method=interp)
            assert torch.equal(both, vxm.utils.transform(s, vxm.utils.compose([m, w]), interp_method=interp))
            assert torch.equal(both, VF.WarpFn.apply(s, vxm.utils.affine_to_dense_shift(m, a["size"], warp_right=w), mode))
    assert torch.equal(vxm.layers.SpatialTransformer(a["size"]).cuda()(s, w), VF.WarpFn.apply(s, w, "bilinear"))      # a dense field: as before


def test_inverse_round_trip_returns_the_volume_on_the_interior(vxm):
    vol, m, _ = ac.roundtrip_arrays()
    v, mat = G(vol), G(m)
    back = vxm.utils.transform(vxm.utils.transform(v, mat), vxm.utils.invert_affine(mat))
    margin = ac.ROUNDTRIP[3]
    err = ac.rel_l2(ac.interior(N(back), margin), ac.interior(vol, margin))
    print("round trip: rel-L2 on the interior %.4e, bound %.3e" % (err, ROUNDTRIP_BOUND))
    assert err <= ROUNDTRIP_BOUND
    assert err > 1e-4                                              # two interpolations: not the identity either
    assert torch.equal(vxm.layers.InvertAffine()(mat), vxm.utils.invert_affine(mat))


def test_no_element_of_an_output_is_left_unwritten(vxm, table):
    """straight through the C ABI with caller-filled buffers: every element of shift / gflow is written (no NaN sentinel survives), nothing
    beyond them is, and the result equals the layers'"""
    from voxelmorph_amd._lib import call, ptr, stream
    a = table["noise_6x11x37"]
    B, size = a["flow"].shape[0], a["size"]
    V = int(np.prod(size))
    mat, flow, gshift = G(a["mat"]), G(a["flow"]), G(a["gshift"])
    nan = float("nan")
    for Bm in (B, 1):
        m = mat[:Bm].contiguous()
        for fl in (flow, None):
            buf = torch.full((B * 3 * V + 64,), nan, device="cuda")
            call("vxm_affine_shift3d_fwd", ptr(m), Bm, ptr(fl), ptr(buf), B, *size, 1, stream())
            torch.cuda.synchronize()
            assert torch.isfinite(buf[:B * 3 * V]).all() and torch.isnan(buf[B * 3 * V:]).all()
            want = vxm.utils.affine_to_dense_shift(m.expand(B, 3, 4).contiguous() if fl is None else m, size, warp_right=fl)
            assert torch.equal(buf[:B * 3 * V].view(B, 3, *size), want)
        buf = torch.full((B * 3 * V + 64,), nan, device="cuda")
        call("vxm_affine_shift3d_bwd", ptr(m), Bm, ptr(gshift), ptr(buf), B, *size, stream())
        torch.cuda.synchronize()
        assert torch.isfinite(buf[:B * 3 * V]).all() and torch.isnan(buf[B * 3 * V:]).all()
        _, gw = run_shift(vxm, a, N(m), a["flow"])
        assert np.array_equal(N(buf[:B * 3 * V]).reshape(gw.shape), gw)
