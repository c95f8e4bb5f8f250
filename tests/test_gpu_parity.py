"""Parity tests proper: the HIP path (through the C ABI, via voxelmorph_amd) against the oracle and the
golden fixtures produced by the unmodified reference.  Run on the MI355X box: `pytest -m gpu`.

Tolerances (SURVEY.md §8c / BASELINE.md §4): nearest warp + index grid bit-exact; trilinear warp
<= 1e-5 abs; integrated flows <= 1e-4 abs; conv activations rel-L2 <= 1e-5; NCC kernels: loss <= 2.5e-7 vs the fp64
arbiter, gradients <= 2.5e-6 vs fp64 (the NCC_* gates below); parameter gradients rel-L2 <= 1e-4.
The absolute warp / VecInt tolerances here are smoke-level (100 - 500 x the reference's own fp32 error): the warp kernels are pinned in
tests/test_gpu_warp.py, against the float64 arbiter that resolves `floor` where the reference does, under 4 x the reference's own error
(2.8e-7 forward, 3.3e-7 gsrc, 4.9e-7 gflow in 3-D), with samples placed where the kernels branch and the non-finite footprint checked.
"""
import os

import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import vxm_oracle as orc

import resize_cases as rc           # tests/resize_cases.py: the resize table, shared with test_cpu_host.py and tools/resize_gates.py

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vxm():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    import voxelmorph_amd
    from voxelmorph_amd import _lib
    _lib.lib()                     # fails loudly if libvxm_hip.so is missing
    return voxelmorph_amd


def G(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return t.requires_grad_() if grad else t


def N(t):
    return t.detach().cpu().numpy()


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def gate(what, measured, bound):
    """Assert measured < bound and print the margin (`pytest -s` / the committed GPU log shows how tight the gate is)."""
    print("[gate] %-58s measured %.3e  bound %.1e" % (what, measured, bound))
    assert measured < bound, "%s: %.3e >= %.1e" % (what, measured, bound)


# ------------------------------------------------------------------ SpatialTransformer
def test_warp_trilinear_golden(vxm, g_layers):
    st = vxm.layers.SpatialTransformer(g_layers["warp_src"].shape[2:]).cuda()
    s, f = G(g_layers["warp_src"], True), G(g_layers["warp_flow"], True)
    out = st(s, f)
    np.testing.assert_allclose(N(out), g_layers["warp_out"], atol=1e-5, rtol=0)
    out.backward(G(g_layers["warp_gout"]))
    np.testing.assert_allclose(N(s.grad), g_layers["warp_gsrc"], atol=1e-5, rtol=0)
    np.testing.assert_allclose(N(f.grad), g_layers["warp_gflow"], atol=2e-5, rtol=0)


def test_warp_nearest_bit_exact_golden(vxm, g_layers):
    vol = g_layers["near_seg"].shape[2:]
    st = vxm.layers.SpatialTransformer(vol, mode="nearest").cuda()
    out = st(G(g_layers["near_seg"]), G(g_layers["near_flow"]))
    assert np.array_equal(N(out), g_layers["near_out"])
    ident = st(G(g_layers["near_seg"]), torch.zeros(1, 3, *vol, device="cuda"))
    assert np.array_equal(N(ident), g_layers["near_seg"])


@pytest.mark.parametrize("vol", [(20, 24, 28), (17, 33, 65), (40, 48, 56)])
def test_warp_nearest_bit_exact_vs_oracle(vxm, vol):
    rng = np.random.default_rng(sum(vol))
    seg = rng.integers(0, 40, size=(2, 3) + vol).astype(np.float32)
    flow = np.concatenate([rng.integers(-9, 10, size=(1, 3) + vol) * 0.5,           # ties
                           rng.standard_normal((1, 3) + vol) * 4.0]).astype(np.float32)  # generic + out of range
    out = vxm.layers.SpatialTransformer(vol, mode="nearest").cuda()(G(seg), G(flow))
    ref = c_oracle.warp3d(seg, flow, mode="nearest")
    assert np.array_equal(N(out), ref), "mismatches: %d" % int((N(out) != ref).sum())
    ref_t = orc.spatial_transformer(torch.from_numpy(seg), torch.from_numpy(flow), mode="nearest").numpy()
    assert np.array_equal(N(out), ref_t)


@pytest.mark.parametrize("vol,C", [((12, 20, 70), 1), ((33, 18, 21), 4)])
def test_warp_trilinear_vs_oracle(vxm, vol, C):
    rng = np.random.default_rng(5)
    src = rng.random((2, C) + vol).astype(np.float32)
    flow = (rng.standard_normal((2, 3) + vol) * 3).astype(np.float32)
    gout = rng.standard_normal((2, C) + vol).astype(np.float32)
    s, f = G(src, True), G(flow, True)
    out = vxm.layers.SpatialTransformer(vol).cuda()(s, f)
    out.backward(G(gout))
    so, fo = torch.from_numpy(src).requires_grad_(), torch.from_numpy(flow).requires_grad_()
    ref = orc.spatial_transformer(so, fo)
    ref.backward(torch.from_numpy(gout))
    np.testing.assert_allclose(N(out), ref.detach().numpy(), atol=1e-5, rtol=0)
    np.testing.assert_allclose(N(s.grad), so.grad.numpy(), atol=2e-5, rtol=0)
    np.testing.assert_allclose(N(f.grad), fo.grad.numpy(), atol=5e-5, rtol=0)
    np.testing.assert_allclose(N(out), c_oracle.warp3d(src, flow), atol=1e-5, rtol=0)


def test_warp_errors(vxm):
    st = vxm.layers.SpatialTransformer((8, 8, 8)).cuda()
    with pytest.raises(RuntimeError):
        st(torch.zeros(1, 1, 8, 8, 8), torch.zeros(1, 3, 8, 8, 8))        # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        st(torch.zeros(1, 1, 8, 8, 8).cuda(), torch.zeros(1, 3, 4, 8, 8).cuda())
    with pytest.raises(ValueError):
        vxm.layers.SpatialTransformer((8, 8, 8), mode="bicubic")


# ------------------------------------------------------------------ VecInt / Resize
def test_vecint_golden(vxm, g_layers):
    vol = g_layers["vecint_in"].shape[2:]
    vi = vxm.layers.VecInt(vol, 7).cuda()
    v = G(g_layers["vecint_in"], True)
    out = vi(v)
    np.testing.assert_allclose(N(out), g_layers["vecint_out"], atol=1e-4, rtol=0)
    out.backward(G(g_layers["vecint_gout"]))
    np.testing.assert_allclose(N(v.grad), g_layers["vecint_gin"], atol=2e-4, rtol=1e-4)
    with pytest.raises(AssertionError):
        vxm.layers.VecInt(vol, -1)
    z = vxm.layers.VecInt(vol, 7).cuda()(torch.zeros(1, 3, *vol, device="cuda"))
    assert float(z.abs().max()) == 0.0


@pytest.mark.parametrize("nsteps", [1, 4])
def test_vecint_vs_oracle(vxm, nsteps):
    vol = (16, 20, 36)
    rng = np.random.default_rng(nsteps)
    vec = (rng.standard_normal((2, 3) + vol) * 2).astype(np.float32)
    gout = rng.standard_normal((2, 3) + vol).astype(np.float32)
    v = G(vec, True)
    out = vxm.layers.VecInt(vol, nsteps).cuda()(v)
    out.backward(G(gout))
    vo = torch.from_numpy(vec).requires_grad_()
    ref = orc.vecint(vo, nsteps)
    ref.backward(torch.from_numpy(gout))
    np.testing.assert_allclose(N(out), ref.detach().numpy(), atol=1e-4, rtol=0)
    np.testing.assert_allclose(N(v.grad), vo.grad.numpy(), atol=2e-4, rtol=1e-4)


@pytest.mark.parametrize("std,nsteps", [(2.0, 4), (6.0, 3), (40.0, 2)])
def test_vecint_large_displacements_deterministic_vs_oracle(vxm, std, nsteps):
    """Steps that move voxels by one voxel or more (a trained network's field): the far senders are scattered by the deterministic
    tile pass (64-bit fixed-point LDS accumulators) -- against the reference's autograd, and bit-identical from run to run.  std 40:
    displacements beyond the tile pass's radius (24 voxels per step) take the atomic fallback (correct, not bit-reproducible)."""
    vol = (16, 20, 36)
    rng = np.random.default_rng(int(std) + nsteps)
    vec = (rng.standard_normal((2, 3) + vol) * std).astype(np.float32)
    gout = rng.standard_normal((2, 3) + vol).astype(np.float32)
    grads = []
    for _ in range(3):
        v = G(vec, True)
        out = vxm.layers.VecInt(vol, nsteps).cuda()(v)
        out.backward(G(gout))
        grads.append(v.grad.clone())
    vo = torch.from_numpy(vec).requires_grad_()
    ref = orc.vecint(vo, nsteps)
    ref.backward(torch.from_numpy(gout))
    np.testing.assert_allclose(N(out), ref.detach().numpy(), atol=1e-4 * max(1.0, std), rtol=0)
    gate("vecint std %.0f: dL/dvec vs reference autograd" % std, rel_l2(N(grads[0]), vo.grad.numpy()), 2e-5)
    if std < 30:
        assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])


def test_vecint_outlier_senders_per_tile_radius_and_poison_locality(vxm):
    """A smooth 3-voxel field with a handful of ~20-voxel outliers (verdict round 5, item 5): the deterministic far pass grows an output
    tile by what the sender tiles around it need (per-tile records left by the gather) instead of by the batch maximum -- the same bits as
    the global-radius pass (the ABI-0.4 scratch size selects it), the reference's gradient, and a NaN in ONE far sender's upstream
    gradient makes NaN only what that sender targets (grid_sample's backward: the 8 corners), not the 1024 voxels of a tile."""
    from voxelmorph_amd.torch import functional as VF
    vol, nsteps, B = (24, 32, 64), 5, 1
    rng = np.random.default_rng(77)
    low = torch.from_numpy(rng.standard_normal((B, 3, 3, 4, 5)).astype(np.float32))
    vec = torch.nn.functional.interpolate(low, size=vol, mode="trilinear", align_corners=True)
    vec = (vec * (3.0 / float(vec.abs().max()))).contiguous()
    # two smooth bumps of ~20 voxels (sigma 4: wide enough that scaling and squaring really moves their voxels that far) in a 3-voxel field
    zz, yy, xx = torch.meshgrid(*[torch.arange(n, dtype=torch.float32) for n in vol], indexing="ij")
    for (z, y, x, c, a) in ((5, 8, 12, 2, 20.0), (18, 24, 50, 1, -19.0)):
        vec[0, c] += a * torch.exp(-((zz - z) ** 2 + (yy - y) ** 2 + (xx - x) ** 2) / (2 * 4.0 ** 2))
    gout = torch.from_numpy(rng.standard_normal((B, 3) + vol).astype(np.float32))
    v = vec.cuda().requires_grad_()
    out = vxm.layers.VecInt(vol, nsteps).cuda()(v)
    out.backward(gout.cuda())
    vo = vec.clone().requires_grad_()
    ref = orc.vecint(vo, nsteps)
    ref.backward(gout)
    gate("vecint with 20-voxel outliers: dL/dvec vs reference autograd", rel_l2(N(v.grad), vo.grad.numpy()), 2e-5)
    # the C ABI with the ABI-0.4 scratch size: the step's global maximum as every tile's radius -- same bits
    D, H, W = vol
    n = vec.numel()
    steps = torch.empty((nsteps,) + tuple(vec.shape), device="cuda")
    VF.call("vxm_vecint_fwd", VF.ptr(v.detach()), VF.ptr(steps), B, D, H, W, nsteps, VF.stream())
    res = []
    for elems in (2 * n + 128, VF.vecint_work_elems(vec.shape)):
        work, gvec = torch.empty(elems, device="cuda"), torch.empty_like(v)
        VF.call("vxm_vecint_bwd_ws", VF.ptr(v.detach()), VF.ptr(steps), VF.ptr(gout.cuda()), VF.ptr(gvec), VF.ptr(work), elems * 4, B, D, H, W, nsteps, VF.stream())
        res.append(gvec)
    assert torch.equal(res[0], res[1]) and torch.equal(res[1], v.grad)
    with pytest.raises(VF._lib.VxmHipError, match="work holds"):
        VF.call("vxm_vecint_bwd_ws", VF.ptr(v.detach()), VF.ptr(steps), VF.ptr(gout.cuda()), VF.ptr(gvec), VF.ptr(work), (2 * n + 32) * 4, B, D, H, W, nsteps, VF.stream())
    # poison locality: one step, one far sender (displacement 6.5 voxels along W) with a NaN upstream gradient
    one = torch.zeros((1, 3) + vol)
    one[0, 2, 10, 12, 20] = 13.0                      # / 2^1 = 6.5 voxels in the single step
    g1 = torch.randn((1, 3) + vol, generator=torch.Generator().manual_seed(1))
    g1[0, 1, 10, 12, 20] = float("nan")
    v1 = one.cuda().requires_grad_()
    vxm.layers.VecInt(vol, 1).cuda()(v1).backward(g1.cuda())
    where = set(map(tuple, torch.nonzero(torch.isnan(v1.grad[0]).cpu()).tolist()))
    o1 = one.clone().requires_grad_()
    orc.vecint(o1, 1).backward(g1)
    expect = set(map(tuple, torch.nonzero(torch.isnan(o1.grad[0])).tolist()))
    # the reference: the sender itself and, in channel 1, the 8 corners of x' (NaN x weight 0 is NaN too) -- 9 entries, not a tile's 1024 x 3
    assert where == expect and len(expect) <= 3 + 8, (sorted(where), sorted(expect))


def test_full_size_vecint_trained_flow_regime(vxm):
    """The regime a trained network is in (smooth field, |v| ~ 5 voxels) at the size the metric is quoted on: the
    half-resolution 80 x 96 x 112 field, 7 steps.  Forward and gradient against the reference's op sequence on the host, and the
    gradient bit-identical between runs (most voxels of the last steps are far senders)."""
    vol, nsteps = (80, 96, 112), 7
    rng = np.random.default_rng(5)
    low = torch.from_numpy(rng.standard_normal((1, 3, 5, 6, 7)).astype(np.float32))
    vec = torch.nn.functional.interpolate(low, size=vol, mode="trilinear", align_corners=True)
    vec = (vec * (5.0 / float(vec.abs().max()))).contiguous()
    gout = torch.from_numpy(rng.standard_normal((1, 3) + vol).astype(np.float32))
    grads = []
    for _ in range(2):
        v = vec.cuda().requires_grad_()
        out = vxm.layers.VecInt(vol, nsteps).cuda()(v)
        out.backward(gout.cuda())
        grads.append(v.grad.clone())
    assert torch.equal(grads[0], grads[1])
    vo = vec.clone().requires_grad_()
    ref = orc.vecint(vo, nsteps)
    ref.backward(gout)
    print("integrated field: max |v| %.2f voxels" % float(ref.abs().max()))
    gate("full-size vecint, 5-voxel field: forward max abs", float((out.detach().cpu() - ref.detach()).abs().max()), 1e-4)
    gate("full-size vecint, 5-voxel field: dL/dvec vs reference autograd", rel_l2(N(grads[0]), vo.grad.numpy()), 2e-5)


def test_resize_golden(vxm, g_layers):
    x = G(g_layers["resize_in"], True)
    down = vxm.layers.ResizeTransform(2, 3)(x)
    np.testing.assert_allclose(N(down), g_layers["resize_down"], atol=2e-6, rtol=0)
    down.backward(G(g_layers["resize_gdown"]))
    np.testing.assert_allclose(N(x.grad), g_layers["resize_down_gin"], atol=1e-5, rtol=0)
    x2 = G(g_layers["resize_in"], True)
    up = vxm.layers.ResizeTransform(0.5, 3)(x2)
    np.testing.assert_allclose(N(up), g_layers["resize_up"], atol=5e-6, rtol=0)     # fp32 rounding of O(10) values (x2 rescale), different association than ATen
    up.backward(G(g_layers["resize_gup"]))
    np.testing.assert_allclose(N(x2.grad), g_layers["resize_up_gin"], atol=2e-5, rtol=0)
    assert vxm.layers.ResizeTransform(1, 3)(x) is x


# ------------------------------------------------------------------ losses
# NCC gates, all <= 5x what was measured on the MI355X (round 4, profiles/r04*_gpu_tests.log prints the measured values):
#   gradients against the fp64 evaluation      2-D / 3-D  measured <= 4.98e-7  -> 2.5e-6;  1-D (4..9-tap windows: the formula's conditioning)  2.05e-5 -> 1e-4
#   gradients against the reference's own fp32 gradients (which carry their own fp32 error)   measured <= 5.9e-6 -> 1.5e-5 ... 3e-5 (1-D)
#   loss against the fp64 arbiter  measured <= 4.5e-8 -> 2.5e-7;  against the reference's fp32 value  measured <= 4.8e-7 -> 2.5e-6
# (tests/test_gpu_losses.py pins the NCC and Grad kernels at their edges -- halo-only volumes, tile / segment edges, the column remap, the value
#  regimes in which the variance cancels, NaN / Inf voxels -- under gates taken from the reference's own fp32 error; these fixed gates cap them)
NCC_GRAD_GATE = 2.5e-6
NCC_GRAD_GATE_REF = 1.5e-5
NCC_GRAD_GATE_1D = 1e-4
NCC_LOSS_GATE, NCC_LOSS_GATE_REF = 2.5e-7, 2.5e-6
# Resize gates (test_resize_every_backward_kernel_vs_fp64, test_resize_planar_vs_fp64): NOT from what the kernels give -- 4 x the largest error
# of the REFERENCE's own fp32 evaluation (ATen forward and autograd on the CPU) against the float64 arbiter over the cases of
# tests/resize_cases.py, on the tests' inputs (`python tools/resize_gates.py` prints them; profiles/pr02_resize_gates_cpu.txt).  ATen forms
# `ratio * dst` in fp32, so its weights sit ~1e-6 from the fp64 ones: the kernels reproduce that arithmetic and may reorder the sums, no more.
#   3-D  forward rel-L2 2.948e-6 -> 1.179e-5;  backward rel-L2 2.884e-6 -> 1.153e-5;  adjoint gap |<y,g> - <x,gx>| / (|y| |g|) 2.179e-9 -> 8.71e-9
#   2-D  forward        1.868e-6 -> 7.47e-6;   backward        1.846e-6 -> 7.38e-6;   adjoint gap                              1.179e-8 -> 4.71e-8
RESIZE_FWD_GATE, RESIZE_BWD_GATE, RESIZE_ADJ_GATE = 1.179e-5, 1.153e-5, 8.71e-9
RESIZE2D_FWD_GATE, RESIZE2D_BWD_GATE, RESIZE2D_ADJ_GATE = 7.47e-6, 7.38e-6, 4.71e-8


def test_ncc_golden(vxm, g_losses):
    I, J = G(g_losses["I"]), G(g_losses["J"], True)
    l = vxm.losses.NCC().loss(I, J)
    gate("ncc golden: loss vs fp32 reference", abs(float(l) - float(g_losses["ncc"])), NCC_LOSS_GATE_REF)
    gate("ncc golden: loss vs fp64 arbiter", abs(float(l) - orc.ncc_explicit(g_losses["I"], g_losses["J"])), NCC_LOSS_GATE)
    l.backward()
    gate("ncc golden: dJ vs reference (fp32)", rel_l2(N(J.grad), g_losses["ncc_gJ"]), NCC_GRAD_GATE_REF)
    J5 = G(g_losses["J"], True)
    l5 = vxm.losses.NCC(win=[5, 5, 5]).loss(I, J5)
    gate("ncc5 golden: loss vs fp32 reference", abs(float(l5) - float(g_losses["ncc5"])), NCC_LOSS_GATE_REF)
    l5.backward()
    gate("ncc5 golden: dJ vs reference (fp32)", rel_l2(N(J5.grad), g_losses["ncc5_gJ"]), NCC_GRAD_GATE_REF)


def test_ncc_any_window_golden(vxm, g_nccwin):
    """Windows that are not odd and of one size per axis (losses.py:26-36: every axis padded by win[0] // 2, box sums of extent
    S + 2 pad - win + 1): value and both gradients against the fixtures of the unmodified reference and against the fp64 arbiter."""
    for tag in g_nccwin["cases"]:
        tag = str(tag)
        win = [int(w) for w in g_nccwin[tag + "_win"]]
        nd = len(win)
        Ia, Ja = g_nccwin["I%d" % nd], g_nccwin["J%d" % nd]
        I, J = G(Ia, True), G(Ja, True)
        l = vxm.losses.NCC(win=win).loss(I, J)
        l.backward()
        le, gJ, gI = orc.ncc_explicit_win(Ia, Ja, win, grad=True)
        g64, gref = (NCC_GRAD_GATE_1D, 2 * NCC_GRAD_GATE_REF) if nd == 1 else (NCC_GRAD_GATE, NCC_GRAD_GATE_REF)
        gate("ncc win=%s: loss vs fp32 reference" % win, abs(float(l) - float(g_nccwin[tag])), NCC_LOSS_GATE_REF)
        gate("ncc win=%s: loss vs fp64 arbiter" % win, abs(float(l) - le), NCC_LOSS_GATE)
        gate("ncc win=%s: dJ vs reference" % win, rel_l2(N(J.grad), g_nccwin[tag + "_gJ"]), gref)
        gate("ncc win=%s: dI vs reference" % win, rel_l2(N(I.grad), g_nccwin[tag + "_gI"]), gref)
        gate("ncc win=%s: dJ vs fp64" % win, rel_l2(N(J.grad), gJ), g64)
        gate("ncc win=%s: dI vs fp64" % win, rel_l2(N(I.grad), gI), g64)
    # a window that leaves no box sums raises, as the reference's conv does
    with pytest.raises(ValueError):
        vxm.losses.NCC(win=[3, 9]).loss(G(g_nccwin["I2"][..., :4]), G(g_nccwin["J2"][..., :4]))
    with pytest.raises(ValueError):
        vxm.losses.NCC(win=[9, 9]).loss(G(g_nccwin["I3"]), G(g_nccwin["J3"]))


@pytest.mark.parametrize("win", [[9, 9, 5], [4, 6, 8], [11, 3, 3]])
def test_ncc_any_window_larger_volume_vs_fp64(vxm, win):
    rng = np.random.default_rng(sum(win))
    vol = (21, 34, 45)
    I = rng.random((2, 1) + vol).astype(np.float32)
    J = (0.6 * I + 0.4 * rng.random((2, 1) + vol)).astype(np.float32)
    Ig, Jg = G(I, True), G(J, True)
    l = vxm.losses.NCC(win=win).loss(Ig, Jg)
    l.backward()
    le, gJ, gI = orc.ncc_explicit_win(I, J, win, grad=True)
    gate("ncc win=%s %s: loss vs fp64" % (win, vol), abs(float(l) - le), NCC_LOSS_GATE)
    gate("ncc win=%s %s: dJ vs fp64" % (win, vol), rel_l2(N(Jg.grad), gJ), NCC_GRAD_GATE)
    gate("ncc win=%s %s: dI vs fp64" % (win, vol), rel_l2(N(Ig.grad), gI), NCC_GRAD_GATE)


def test_ncc_grad_vs_fp64(vxm):
    rng = np.random.default_rng(2)
    vol = (24, 20, 40)
    I = rng.random((1, 1) + vol).astype(np.float32)
    J = (0.5 * I + 0.5 * rng.random((1, 1) + vol)).astype(np.float32)
    Jg = G(J, True)
    Ig = G(I, True)
    l = vxm.losses.NCC().loss(Ig, Jg)
    l.backward()
    Jd = torch.from_numpy(J).double().requires_grad_()
    Id = torch.from_numpy(I).double().requires_grad_()
    ld = orc.ncc_loss(Id, Jd)
    ld.backward()
    gate("ncc 9^3: loss vs fp64", abs(float(l) - float(ld)), NCC_LOSS_GATE)
    gate("ncc 9^3: dJ vs fp64", rel_l2(N(Jg.grad), Jd.grad.numpy()), NCC_GRAD_GATE)
    gate("ncc 9^3: dI vs fp64", rel_l2(N(Ig.grad), Id.grad.numpy()), NCC_GRAD_GATE)


@pytest.mark.parametrize("win", [3, 7, 9, 11])
def test_ncc_windows_batches_segments_vs_fp64(vxm, win):
    """Fused march (win <= 9: several depth segments, ragged tiles, batch 2) and the separable passes (win 11)."""
    rng = np.random.default_rng(win)
    vol = (45, 19, 37)
    I = rng.random((2, 1) + vol).astype(np.float32)
    J = (0.6 * I + 0.4 * rng.random((2, 1) + vol)).astype(np.float32)
    Jg = G(J, True)
    l = vxm.losses.NCC(win=[win] * 3).loss(G(I), Jg)
    l.backward()
    Jd = torch.from_numpy(J).double().requires_grad_()
    ld = orc.ncc_loss(torch.from_numpy(I).double(), Jd, win=[win] * 3)
    ld.backward()
    gate("ncc %d^3 B=2: loss vs fp64" % win, abs(float(l) - float(ld)), NCC_LOSS_GATE)
    gate("ncc %d^3 B=2: dJ vs fp64" % win, rel_l2(N(Jg.grad), Jd.grad.numpy()), NCC_GRAD_GATE)


@pytest.mark.parametrize("win", [None, 5, 4])
def test_ncc_one_dimensional_vs_reference_formula(vxm, win):
    """NCC on [B,1,L] signals (losses.py:15-67 with ndims = 1: conv1d box filter): the oracle IS the reference's formula (same ATen
    calls, filter on the input's device); loss against its fp32 and fp64 evaluations, both gradients against fp64.  win = 4: an even
    window (L + 1 box sums, losses.py:31)."""
    rng = np.random.default_rng(11)
    L = 777
    I = rng.random((3, 1, L)).astype(np.float32)
    J = (0.5 * I + 0.5 * rng.random((3, 1, L))).astype(np.float32)
    w = None if win is None else [win]
    Ig, Jg = G(I, True), G(J, True)
    l = vxm.losses.NCC(win=w).loss(Ig, Jg)
    l.backward()
    l32 = orc.ncc_loss(torch.from_numpy(I), torch.from_numpy(J), win=w)
    Id, Jd = torch.from_numpy(I).double().requires_grad_(), torch.from_numpy(J).double().requires_grad_()
    ld = orc.ncc_loss(Id, Jd, win=w)
    ld.backward()
    gate("ncc 1-D win=%s: loss vs fp32 formula" % w, abs(float(l.detach()) - float(l32)), NCC_LOSS_GATE_REF)
    gate("ncc 1-D win=%s: loss vs fp64" % w, abs(float(l.detach()) - float(ld.detach())), NCC_LOSS_GATE)
    gate("ncc 1-D win=%s: dJ vs fp64" % w, rel_l2(N(Jg.grad), Jd.grad.numpy()), NCC_GRAD_GATE_1D)
    gate("ncc 1-D win=%s: dI vs fp64" % w, rel_l2(N(Ig.grad), Id.grad.numpy()), NCC_GRAD_GATE_1D)


def test_grad_mse_dice_golden(vxm, g_losses):
    for pen, mult in (("l1", None), ("l2", 2)):
        fl = G(g_losses["flow"], True)
        l = vxm.losses.Grad(pen, loss_mult=mult).loss(None, fl)
        np.testing.assert_allclose(float(l), g_losses["grad_%s" % pen], rtol=1e-5)
        l.backward()
        np.testing.assert_allclose(N(fl.grad), g_losses["grad_%s_g" % pen], atol=1e-8, rtol=1e-4)
    with pytest.raises(AssertionError):
        vxm.losses.Grad("l3").loss(None, G(g_losses["flow"]))
    J = G(g_losses["J"], True)
    m = vxm.losses.MSE().loss(G(g_losses["I"]), J)
    np.testing.assert_allclose(float(m), g_losses["mse"], rtol=1e-5)
    m.backward()
    np.testing.assert_allclose(N(J.grad), g_losses["mse_gJ"], atol=1e-9, rtol=1e-4)
    yp = G(g_losses["dice_pred"], True)
    d = vxm.losses.Dice().loss(G(g_losses["dice_true"]), yp)
    np.testing.assert_allclose(float(d), g_losses["dice"], rtol=1e-5)
    d.backward()
    np.testing.assert_allclose(N(yp.grad), g_losses["dice_g"], atol=1e-9, rtol=1e-4)


@pytest.mark.parametrize("shape", [(2, 3, 40, 48, 56), (1, 3, 7, 9, 12), (2, 3, 5, 6, 260), (1, 3, 6, 5, 11), (1, 2, 1, 9, 16)])
@pytest.mark.parametrize("pen", ["l1", "l2"])
def test_grad_loss_kernel_variants_vs_oracle(vxm, shape, pen):
    """Both Grad kernels (16-byte loads when W % 4 == 0 — incl. W > 256, where a wave walks a row in two pieces — and the
    scalar one otherwise), volumes and a planar field (D = 1), value and gradient against the fp64 oracle."""
    rng = np.random.default_rng(sum(shape))
    planar = shape[2] == 1
    f = rng.standard_normal(shape).astype(np.float32)
    fg = G(f[:, :, 0] if planar else f, True)
    l = vxm.losses.Grad(pen, loss_mult=2).loss(None, fg)
    l.backward()
    fo = torch.from_numpy(f[:, :, 0] if planar else f).double().requires_grad_()
    lo = orc.grad_loss(fo, pen, 2)
    lo.backward()
    assert abs(float(l.detach()) - float(lo.detach())) <= 1e-6 * abs(float(lo.detach()))
    assert rel_l2(N(fg.grad), fo.grad.numpy()) < 1e-6


# ------------------------------------------------------------------ conv / pool / U-Net
@pytest.mark.parametrize("cin,cout,vol,slope", [
    (2, 16, (8, 8, 16), 0.2), (16, 32, (8, 12, 16), 0.2), (32, 32, (5, 6, 7), 0.2), (48, 32, (4, 8, 32), 0.2),
    (64, 32, (8, 4, 16), 0.2), (16, 3, (9, 10, 33), 1.0), (5, 7, (6, 7, 19), 0.2), (20, 40, (4, 4, 16), 0.2),
    (17, 16, (5, 7, 28), 0.2), (32, 48, (6, 9, 36), 1.0), (3, 3, (3, 3, 4), 0.2),
    (16, 3, (6, 8, 20), 1.0), (24, 2, (5, 6, 16), 0.2),        # few output channels: role-swapped backward-weight
    (1, 16, (8, 8, 16), 0.2), (4, 20, (8, 8, 16), 0.2),        # few input channels: dense-K MFMA kernel (with VXM_CONV_WIDE_MIN_TILES=1)
    (2, 16, (8, 8, 32), 0.2), (3, 5, (8, 4, 64), 1.0), (16, 32, (8, 4, 64), 0.2),      # W % 32 == 0: the 8 x 2 x 32 tile instances
])
def test_conv_block_vs_oracle(vxm, cin, cout, vol, slope):
    from voxelmorph_amd.torch import functional as VF
    rng = np.random.default_rng(cin * 100 + cout)
    x = rng.standard_normal((2, cin) + vol).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3, 3)) / np.sqrt(27 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    gy = rng.standard_normal((2, cout) + vol).astype(np.float32)
    xg, wg, bg = G(x, True), G(w, True), G(b, True)
    y = VF.ConvFn.apply(xg, wg, bg, slope)
    y.backward(G(gy))
    xo, wo, bo = (torch.from_numpy(a).double().requires_grad_() for a in (x, w, b))
    yo = orc.conv_block(xo, wo, bo, slope)
    yo.backward(torch.from_numpy(gy).double())
    assert rel_l2(N(y), yo.detach().numpy()) < 1e-5
    assert rel_l2(N(xg.grad), xo.grad.numpy()) < 1e-5
    assert rel_l2(N(wg.grad), wo.grad.numpy()) < 1e-5
    assert rel_l2(N(bg.grad), bo.grad.numpy()) < 1e-5


@pytest.mark.parametrize("ndims,stride", [(3, 2), (3, 3), (2, 2)])
def test_conv_block_with_a_stride_vs_fp64(vxm, ndims, stride):
    """`ConvBlock(ndims, cin, cout, stride)` (networks.py:295-299): the reference accepts any stride; here it is the stride-1 block sampled at
    every stride-th voxel.  Output and all three gradients against fp64 torch of the reference's op sequence."""
    torch.manual_seed(40 + ndims + stride)
    vol = (9, 12, 14)[3 - ndims:]
    blk = vxm.networks.ConvBlock(ndims, 5, 7, stride).cuda()
    x = torch.randn((2, 5) + vol, device="cuda", requires_grad=True)
    y = blk(x)
    gy = torch.randn_like(y)
    y.backward(gy)
    conv = torch.nn.functional.conv3d if ndims == 3 else torch.nn.functional.conv2d
    xd = x.detach().cpu().double().requires_grad_()
    wd, bd = blk.main.weight.detach().cpu().double().requires_grad_(), blk.main.bias.detach().cpu().double().requires_grad_()
    yd = torch.nn.functional.leaky_relu(conv(xd, wd, bd, stride=stride, padding=1), 0.2)
    assert tuple(y.shape) == tuple(yd.shape)
    yd.backward(gy.cpu().double())
    assert rel_l2(N(y), yd.detach().numpy()) < 1e-5
    assert rel_l2(N(x.grad), xd.grad.numpy()) < 1e-5 and rel_l2(N(blk.main.weight.grad), wd.grad.numpy()) < 1e-5
    assert rel_l2(N(blk.main.bias.grad), bd.grad.numpy()) < 1e-5


@pytest.mark.parametrize("cin,cout,vol", [(8, 2, (8, 8, 16)), (16, 3, (8, 8, 16)), (5, 7, (6, 7, 20)), (24, 20, (8, 8, 32)), (3, 16, (8, 12, 16))])
def test_conv_block_output_guard(vxm, cin, cout, vol):
    """The epilogues store through buffer descriptors and let the hardware drop lanes that are out of range: channel counts that do
    not fill the 16-channel MFMA tiles must not touch anything beyond their own channels (neighbouring channels of a larger
    buffer, the next sample, the tail), forward and backward-data."""
    from voxelmorph_amd.torch import functional as VF
    D, H, W = vol
    V = D * H * W
    B, pad = 2, 5
    torch.manual_seed(cin * 31 + cout)
    x = torch.randn(B, cin, D, H, W, device="cuda")
    w = torch.randn(cout, cin, 3, 3, 3, device="cuda") / (27 * cin) ** 0.5
    b = torch.randn(cout, device="cuda")
    big = torch.full((B + 1, cout + pad, D, H, W), 7.25, device="cuda")          # sentinel everywhere
    y = big[:B, :cout]
    VF.conv_forward(x, cin, cin * V, False, None, 0, 0, w, b, y, (cout + pad) * V, cout, 0.2, B, D, H, W)
    assert bool((big[:B, cout:] == 7.25).all()) and bool((big[B] == 7.25).all())
    ref = orc.conv_block(x.cpu().double(), w.cpu().double(), b.cpu().double(), 0.2)
    assert rel_l2(N(y), ref.numpy()) < 1e-5
    dz = torch.randn(B, cout, D, H, W, device="cuda")
    mask = torch.randn(B, cin, D, H, W, device="cuda")
    gfull = torch.full((B + 1, cin, D, H, W), 7.25, device="cuda")
    VF.conv_bwd_data(dz, cout, w, gfull[:B], cin, mask, 0.2, B, D, H, W)
    assert bool((gfull[B] == 7.25).all())
    xr = x.cpu().double().requires_grad_()
    torch.nn.functional.conv3d(xr, w.cpu().double(), None, padding=1).backward(dz.cpu().double())
    want = xr.grad * torch.where(mask.cpu().double() > 0, 1.0, 0.2)
    assert rel_l2(N(gfull[:B]), want.numpy()) < 1e-5


@pytest.mark.parametrize("c0,c1,cout,vol", [(32, 16, 32, (16, 8, 32)), (8, 0, 16, (8, 12, 16)), (6, 5, 20, (12, 8, 32)), (32, 32, 32, (8, 8, 16))])
def test_conv_upsampled_segment_collapsed_weights(vxm, c0, c1, cout, vol):
    """cat([upsample2(x0), x1]) conv with the upsampled segment evaluated at low resolution through per-parity collapsed
    2x2x2 weights (k_conv3d_k3_t8u) against the plain fp64 conv over the materialised concat; borders included."""
    import subprocess  # noqa: F401
    from voxelmorph_amd import _lib
    from voxelmorph_amd.torch import functional as VF
    rng = np.random.default_rng(c0 + c1)
    B = 2
    x0 = rng.standard_normal((B, c0) + tuple(s // 2 for s in vol)).astype(np.float32)
    x1 = rng.standard_normal((B, c1) + vol).astype(np.float32) if c1 else None
    w = (rng.standard_normal((cout, c0 + c1, 3, 3, 3)) / np.sqrt(27 * (c0 + c1))).astype(np.float32)
    bias = rng.standard_normal(cout).astype(np.float32)
    gx0, gx1, gw, gb = G(x0), (G(x1) if c1 else None), G(w), G(bias)
    y = torch.empty((B, cout) + vol, device="cuda")
    D, H, W = vol
    V = D * H * W
    os.environ.setdefault("VXM_CONV_WIDE_MIN_TILES", "1")          # read once per process: harmless if already loaded
    ok = _lib.lib().vxm_conv3d_k3_up_ok(gx0.data_ptr(), c0, gx0[0].numel(), gx1.data_ptr() if c1 else None, c1, c1 * V, y.data_ptr(), cout, B, D, H, W)
    VF.conv_forward(gx0, c0, gx0[0].numel(), True, gx1, c1, c1 * V, gw, gb, y, cout * V, cout, 0.2, B, D, H, W)
    xin = torch.nn.functional.interpolate(torch.from_numpy(x0).double(), scale_factor=2, mode="nearest")
    if c1:
        xin = torch.cat([xin, torch.from_numpy(x1).double()], 1)
    ref = torch.nn.functional.leaky_relu(torch.nn.functional.conv3d(xin, torch.from_numpy(w).double(), torch.from_numpy(bias).double(), padding=1), 0.2)
    assert rel_l2(N(y), ref.numpy()) < 1e-5, "collapsed path used: %s" % bool(ok)


@pytest.mark.parametrize("c0,c1,cout,vol", [(1, 1, 16, (3, 9, 68)), (2, 0, 16, (5, 7, 20)), (2, 1, 16, (4, 8, 64)), (16, 0, 3, (3, 9, 68)), (16, 0, 2, (5, 17, 132)),
                                            (16, 0, 1, (4, 8, 64))])
@pytest.mark.parametrize("pieces", ["f16x2", "fp32"])
def test_few_channel_backward_weight_kernel(vxm, c0, c1, cout, vol, pieces):
    """`k_fewch_bwd_weight_h` (round 6: fp16 pieces on the 16-bit matrix pipe, the default engine's kernel) and `k_fewch_bwd_weight` (fp32
    MFMA) -- first block: 1-3 input channels as a virtual concat of two tensors; flow conv: 1-3 output channels: weight and bias gradient
    against fp64 autograd with two samples, rows that do not fill the tiles, more than one tile along W with a partial last one
    (VXM_FEWCH is read once per process, so the comparison partner here is fp64 only).  Gates: 1e-6 on the pieces (as every split kernel), 1e-5 fp32."""
    from voxelmorph_amd import _lib
    from voxelmorph_amd.torch import functional as VF
    if pieces == "f16x2" and VF.FP32_ENGINE != "f16x2":
        pytest.skip("the fp16-piece few-channel kernel belongs to the f16x2 engine")
    keep = VF.FEWCH_H
    VF.FEWCH_H = pieces == "f16x2"
    try:
        _few_channel_backward_weight(vxm, c0, c1, cout, vol, 1e-6 if pieces == "f16x2" else 1e-5)
    finally:
        VF.FEWCH_H = keep


def _few_channel_backward_weight(vxm, c0, c1, cout, vol, bound):
    from voxelmorph_amd import _lib
    from voxelmorph_amd.torch import functional as VF
    D, H, W = vol
    V, B, cin = D * H * W, 2, c0 + c1
    torch.manual_seed(17 * cin + cout)
    x0 = torch.randn(B, c0, D, H, W, device="cuda")
    x1 = torch.randn(B, c1, D, H, W, device="cuda") if c1 else None
    dz = torch.randn(B, cout, D, H, W, device="cuda")
    v = _lib.lib().vxm_conv3d_k3_bwd_weight_variant(x0.data_ptr(), c0, c0 * V, 0, x1.data_ptr() if c1 else None, c1, c1 * V, dz.data_ptr(), cout * V, cout, D, H, W)
    assert v // 10 == 3, "the dedicated kernel should take this shape (variant %d)" % v
    gw, gb = torch.full((cout, cin, 3, 3, 3), 7.25, device="cuda"), torch.full((cout,), 7.25, device="cuda")
    VF.conv_bwd_weight(VF._Workspace(x0.device), x0, c0, c0 * V, False, x1, c1, c1 * V, dz, cout, gw, gb, B, D, H, W)
    xin = torch.cat([x0, x1], 1) if c1 else x0
    wr = torch.zeros(cout, cin, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    br = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv3d(xin.cpu().double(), wr, br, padding=1).backward(dz.cpu().double())
    gate("few-channel weight gradient %d+%d -> %d" % (c0, c1, cout), rel_l2(N(gw), wr.grad.numpy()), bound)
    gate("few-channel bias gradient %d+%d -> %d" % (c0, c1, cout), rel_l2(N(gb), br.grad.numpy()), bound)
    # inputs spread over 20 orders of magnitude per sample: the per-tile scales keep the relative accuracy (exact powers of two)
    gw2, gb2 = torch.empty_like(gw), torch.empty_like(gb)
    VF.conv_bwd_weight(VF._Workspace(x0.device), x0, c0, c0 * V, False, x1, c1, c1 * V, dz, cout, gw2, gb2, B, D, H, W)
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)           # fixed summation order


def test_conv_bwd_data_and_workspace_umbrella_names(vxm):
    """SURVEY.md section 8b lists `vxm_conv3d_k3_bwd_data` and `vxm_workspace_bytes(op, dims)`: the first packs the adjoint operator into the
    caller's scratch and runs the forward kernel on it (fp64 conv-transpose as the arbiter, with and without the fused LeakyReLU' mask and
    on a channel sub-range), the second dispatches to the per-op queries."""
    from voxelmorph_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(5)
    B, cin, cout, vol = 2, 8, 5, (6, 7, 20)
    V = vol[0] * vol[1] * vol[2]
    w = rng.standard_normal((cout, cin, 3, 3, 3)).astype(np.float32) * 0.2
    dz = rng.standard_normal((B, cout) + vol).astype(np.float32)
    mask = rng.standard_normal((B, cin) + vol).astype(np.float32)
    ref = torch.nn.grad.conv3d_input((B, cin) + vol, torch.from_numpy(w).double(), torch.from_numpy(dz).double(), padding=1).numpy()
    for lo, n, use_mask in ((0, cin, False), (0, cin, True), (2, 4, True)):
        nbytes = L.vxm_workspace_bytes(5, n, cout, B, *vol)
        assert nbytes == 4 * L.vxm_conv3d_k3_packed_elems(cout, n) and nbytes > 0
        scratch = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
        gx = torch.full((B, n) + vol, float("nan"), dtype=torch.float32, device="cuda")
        mk = G(np.ascontiguousarray(mask[:, lo:lo + n])) if use_mask else None
        dz_d, w_d = G(dz), G(w)                 # (named: a temporary would be freed, and its memory reused, before the launch reads it)
        _lib.call("vxm_conv3d_k3_bwd_data", _lib.ptr(dz_d), cout, cout * V, _lib.ptr(w_d), cin, lo, n, _lib.ptr(scratch), _lib.ptr(gx), n * V,
                  _lib.ptr(mk), n * V, 0.2, B, *vol, _lib.stream())
        torch.cuda.synchronize()
        want = ref[:, lo:lo + n]
        if use_mask:
            want = want * np.where(mask[:, lo:lo + n] > 0, 1.0, 0.2)
        gate("vxm_conv3d_k3_bwd_data channels [%d, %d) mask %s" % (lo, lo + n, use_mask), rel_l2(N(gx), want), 1e-5)
    assert L.vxm_workspace_bytes(1, 16, 32, 1, 40, 48, 56) == L.vxm_conv3d_k3_bwd_weight_workspace_bytes(16, 32, 1, 40, 48, 56)
    assert L.vxm_workspace_bytes(2, 16, 32, 1, 40, 48, 56) == L.vxm_conv3d_k3_s3_bwd_weight_workspace_bytes(16, 32, 1, 40, 48, 56)
    assert L.vxm_workspace_bytes(3, 32, 32, 1, 160, 192, 224) == L.vxm_conv3d_k3_s3u_bwd_weight_workspace_bytes(32, 32, 1, 160, 192, 224)
    assert L.vxm_workspace_bytes(4, 16, 32, 1, 40, 48, 56) == L.vxm_bf16_conv_bwd_weight_workspace_bytes(16, 32, 1, 40, 48, 56)
    # VecInt backward: two gradient buffers + the per-step statistics + (round 6) the per-tile displacement records of up to 30 steps (2 x 1 x 1 tiles x 2 samples)
    assert L.vxm_workspace_bytes(6, 0, 0, 2, 8, 8, 8) == 4 * (2 * 2 * 3 * 512 + 128 + 30 * 2 * 2) and L.vxm_workspace_bytes(99, 1, 1, 1, 1, 1, 1) == 0


def test_conv_bwd_weight_bitwise_deterministic(vxm):
    """The backward-weight path has a fixed summation order: repeated launches on the same inputs must agree
    bit for bit (a race in the tile hand-over or the partial reduction would show here)."""
    from voxelmorph_amd.torch import functional as VF
    rng = np.random.default_rng(11)
    B, cin, cout, vol = 2, 48, 32, (12, 20, 48)
    V = vol[0] * vol[1] * vol[2]
    x0 = G(rng.standard_normal((B, 32, vol[0] // 2, vol[1] // 2, vol[2] // 2)))
    x1 = G(rng.standard_normal((B, 16) + vol))
    dz = G(rng.standard_normal((B, cout) + vol))
    ws = VF._Workspace(x0.device)
    outs = []
    for _ in range(25):
        gw = torch.full((cout, cin, 3, 3, 3), float("nan"), device="cuda")
        gb = torch.full((cout,), float("nan"), device="cuda")
        VF.conv_bwd_weight(ws, x0, 32, x0[0].numel(), True, x1, 16, x1[0].numel(), dz, cout, gw, gb, B, *vol)
        outs.append((gw, gb))
    torch.cuda.synchronize()
    for gw, gb in outs[1:]:
        assert torch.equal(gw, outs[0][0]) and torch.equal(gb, outs[0][1])
    xin = torch.cat([torch.nn.functional.interpolate(x0, scale_factor=2, mode="nearest"), x1], 1).cpu().double().requires_grad_()
    w = torch.zeros(cout, cin, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv3d(xin, w, None, padding=1).backward(dz.cpu().double())
    assert rel_l2(N(outs[0][0]), w.grad.numpy()) < 1e-5


def test_conv_wide_forward_kernel_on_small_volumes_in_subprocess():
    """VXM_CONV_WIDE_MIN_TILES=1 sends every eligible forward / backward-data launch through the 8-wave wide-load
    kernel (normally reserved for the large layers), so that the oracle parity tests cover it at small sizes."""
    import subprocess
    import sys
    env = dict(os.environ, VXM_CONV_WIDE_MIN_TILES="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.join(root, "tests", "test_gpu_parity.py"),
                        "-k", "conv_block_vs_oracle or unet_vs_oracle or vxm_dense_golden or collapsed_weights"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_conv_generic_kernel_in_subprocess():
    """VXM_CONV_GENERIC=1 routes backward-weight through the LDS-DMA kernel (the path taken when W % 4 != 0 or the
    tensors are not 16-byte aligned); the switch is read once per process, hence the subprocess."""
    import subprocess
    import sys
    env = dict(os.environ, VXM_CONV_GENERIC="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.join(root, "tests", "test_gpu_parity.py"),
                        "-k", "conv_block_vs_oracle or unet_vs_oracle or bitwise_deterministic"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_conv_block_module_matches_c_arbiter(vxm):
    blk = vxm.networks.ConvBlock(3, 3, 4).cuda()
    rng = np.random.default_rng(9)
    x = rng.standard_normal((1, 3, 5, 6, 7)).astype(np.float32)
    y = blk(G(x))
    ref = c_oracle.conv3d_k3(x, N(blk.main.weight), N(blk.main.bias))
    np.testing.assert_allclose(N(y), ref, atol=2e-5)


def test_maxpool_ties_first_index(vxm):
    """All-equal input: ATen routes the gradient to the first element of each 2x2x2 block."""
    from voxelmorph_amd._lib import call, ptr, stream
    x = torch.ones(1, 2, 4, 4, 4, device="cuda")
    gp = torch.arange(16, dtype=torch.float32, device="cuda").reshape(1, 2, 2, 2, 2) + 1
    dz = torch.empty_like(x)
    call("vxm_maxpool2_bwd", ptr(x), x[0].numel(), ptr(gp), None, 0, ptr(dz), 1.0, 1, 2, 4, 4, 4, stream())
    xo = torch.ones(1, 2, 4, 4, 4, requires_grad=True)
    torch.nn.functional.max_pool3d(xo, 2).backward(gp.cpu())
    assert torch.equal(dz.cpu(), xo.grad)


def test_maxpool_forward_codes_hold_what_the_backward_reads(vxm):
    """vxm_maxpool2_fwd_code (round 6): the pooled tensor is max_pool3d's, and the 16-bit word of a pooled voxel holds the sign bits of its
    2x2x2 block (bit k = 4 dz + 2 dy + dx: x > 0) and the arg-max ATen routes the gradient to (first maximum in scan order; a NaN wins) --
    on noise, on exact ties, with negatives, zeros and NaNs in the blocks, two samples."""
    from voxelmorph_amd._lib import call, ptr, stream
    torch.manual_seed(12)
    B, C, D, H, W = 2, 3, 6, 8, 10
    x = torch.randn(B, C, D, H, W, device="cuda")
    x[0, 0, :2] = 0.5                      # ties: the first element wins
    x[0, 1, 2:4] = -1.0                    # ties among negatives
    x[1, 2, 4:, :4] = 0.0                  # zeros are not > 0
    x[1, 0, 1, 3, 5] = float("nan")        # a NaN is the maximum of its block ...
    x[1, 0, 1, 3, 4] = float("nan")        # ... and a later NaN replaces an earlier one (ATen: val > max || isnan(val))
    y = torch.empty(B, C, D // 2, H // 2, W // 2, device="cuda")
    code = torch.empty(B, C, D // 2, H // 2, W // 2, dtype=torch.int16, device="cuda")
    call("vxm_maxpool2_fwd_code", ptr(x), x[0].numel(), ptr(y), ptr(code), B, C, D, H, W, stream())
    y0 = torch.empty_like(y)
    call("vxm_maxpool2_fwd", ptr(x), x[0].numel(), ptr(y0), B, C, D, H, W, stream())
    assert torch.equal(y.nan_to_num(nan=7.0), y0.nan_to_num(nan=7.0))
    blocks = x.cpu().reshape(B, C, D // 2, 2, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(B, C, D // 2, H // 2, W // 2, 8)
    cd = code.cpu().to(torch.int32) & 0xffff
    bits = sum(((blocks[..., k] > 0).to(torch.int32) << k) for k in range(8))
    assert torch.equal(cd & 0xff, bits)
    arg = torch.zeros(blocks.shape[:-1], dtype=torch.int32)
    m = blocks[..., 0].clone()
    for k in range(1, 8):
        v = blocks[..., k]
        take = (v > m) | torch.isnan(v)
        m = torch.where(take, v, m)
        arg = torch.where(take, torch.full_like(arg, k), arg)
    assert torch.equal((cd >> 8) & 7, arg) and int((cd >> 11).max()) == 0
    # and the routed gradient of the reference agrees with that arg-max where the block has no NaN
    xo = x.cpu().nan_to_num(nan=9.0).requires_grad_()
    gp = torch.rand(B, C, D // 2, H // 2, W // 2) + 1.0
    torch.nn.functional.max_pool3d(xo, 2).backward(gp)
    routed = xo.grad.reshape(B, C, D // 2, 2, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(B, C, D // 2, H // 2, W // 2, 8)
    clean = ~torch.isnan(blocks).any(-1)
    assert torch.equal(routed.argmax(-1).to(torch.int32)[clean], arg[clean])
    with pytest.raises(Exception, match="even"):
        call("vxm_maxpool2_fwd_code", ptr(x), x[0].numel(), ptr(y), ptr(code), B, C, D - 1, H, W, stream())


@pytest.mark.parametrize("c0,up0,c1,cout,vol,B,with_mask", [(32, False, 0, 32, (20, 24, 28), 1, False), (32, False, 0, 32, (10, 12, 14), 2, True),
                                                           (32, True, 32, 32, (20, 24, 28), 1, False), (32, False, 0, 64, (20, 24, 28), 1, True),
                                                           (40, False, 0, 24, (9, 11, 13), 1, True), (24, True, 16, 40, (6, 10, 18), 2, False),
                                                           (20, False, 12, 32, (7, 12, 20), 1, True)])           # (a chunk that straddles the two segments)
def test_small_volume_conv_kernel_vs_fp64(vxm, c0, up0, c1, cout, vol, B, with_mask):
    """k_conv3d_k3_sm (round 6): the conv launches of the U-Net levels at 1/8 and 1/16 resolution -- input channels split over the waves of a
    block, partial tiles added in wave order -- forward (bias, LeakyReLU, virtual concat with an x2-upsampled segment) and backward-data (fused
    LeakyReLU' mask) against an fp64 evaluation on the host: the shapes of the default network, two output-channel groups, channel counts that
    are not multiples of 8 / 16, odd extents, two samples; the dispatcher must actually have chosen it (variant code 300 + waves)."""
    from voxelmorph_amd import _lib
    from voxelmorph_amd.torch import functional as VF
    if os.environ.get("VXM_CONV_SMALL_MAX_BLOCKS") == "0" or os.environ.get("VXM_CONV_GENERIC") == "1":
        pytest.skip("the small-volume kernel is switched off in this process")
    import torch.nn.functional as F
    D, H, W = vol
    V, cin = D * H * W, c0 + c1
    torch.manual_seed(40 + cout)
    x0 = torch.randn(B, c0, *((D // 2, H // 2, W // 2) if up0 else vol), device="cuda")
    x1 = torch.randn(B, c1, D, H, W, device="cuda") if c1 else None
    w = torch.randn(cout, cin, 3, 3, 3, device="cuda") / (27 * cin) ** 0.5
    b = torch.randn(cout, device="cuda")
    y = torch.full((B, cout, D, H, W), float("nan"), device="cuda")
    dz = torch.randn(B, cout, D, H, W, device="cuda")
    gx = torch.full((B, cin, D, H, W), float("nan"), device="cuda")
    mask = torch.randn(B, cin, D, H, W, device="cuda") if with_mask else None
    wpk = VF.pack_weights_cached(w, False, 0, cin)
    assert not VF.s3_route(c0, up0, c1, cout, B, D, H, W) and not (up0 and VF.s3u_route(c0, c1, cout, B, D, H, W))      # (levels below the split engine)
    code = _lib.lib().vxm_conv3d_k3_fwd_variant(VF.ptr(x0), c0, x0[0].numel(), VF.ptr(x1), c1, x1[0].numel() if c1 else 0, VF.ptr(wpk), cout, B, D, H, W)
    assert code == (308 if cin >= 64 else 304), code
    VF.conv_forward(x0, c0, x0[0].numel(), up0, x1, c1, x1[0].numel() if c1 else 0, w, b, y, cout * V, cout, 0.2, B, D, H, W)
    VF.conv_bwd_data(dz, cout, w, gx, cin, mask, 0.2, B, D, H, W)
    xin = x0.cpu().double()
    if up0:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    if c1:
        xin = torch.cat([xin, x1.cpu().double()], 1)
    ref = F.leaky_relu(F.conv3d(xin, w.cpu().double(), b.cpu().double(), padding=1), 0.2)
    gref = F.conv_transpose3d(dz.cpu().double(), w.cpu().double(), padding=1)
    if mask is not None:
        gref = gref * torch.where(mask.cpu() > 0, 1.0, 0.2).double()
    ey, eg = rel_l2(N(y).astype(np.float64), ref.numpy()), rel_l2(N(gx).astype(np.float64), gref.numpy())
    print("small-volume conv %d%s+%d -> %d at %s, B=%d: rel-L2 vs fp64 forward %.2e, backward-data %.2e" % (c0, "^" if up0 else "", c1, cout, vol, B, ey, eg))
    assert ey <= 1e-6 and eg <= 1e-6, (ey, eg)


@pytest.mark.parametrize("kw", [dict(), dict(nb_features=[[4, 8], [8, 8, 4]]), dict(nb_features=8, nb_levels=3, nb_conv_per_level=2),
                                dict(half_res=True), dict(nb_features=[[8, 8], [8, 8]])])
def test_unet_vs_oracle(vxm, kw):
    inshape = (16, 16, 32)
    # Seeded weights, and a conditioning check: the network is piecewise linear, so when a pre-activation lands within fp32 rounding
    # of 0 (or two entries of a pooling window within rounding of each other) LeakyReLU' / the arg-max differ between ANY two
    # evaluations with different summation orders -- the fp32 path and the fp64 oracle, or the fp32-MFMA and the split kernels -- and
    # at the deepest levels (a few hundred activations) one such flip moves a gradient by more than the tolerance.  A seed whose
    # smallest margin (oracle.conditioning) is inside that rounding is not a parity sample; the next seed is taken instead, and at
    # least one well-conditioned seed must exist and pass.
    checked = 0
    for seed in (20240607, 20240608, 20240609, 20240610):
        torch.manual_seed(seed)
        net = vxm.networks.Unet(inshape, infeats=2, **kw).cuda()
        sd = {("unet_model." + k): v for k, v in net.state_dict().items()}
        rng = np.random.default_rng(4)
        x = rng.standard_normal((2, 2) + inshape).astype(np.float32)
        sdo = {k: v.detach().cpu().double().requires_grad_() for k, v in sd.items()}
        xo = torch.from_numpy(x).double().requires_grad_()
        okw = {k: v for k, v in kw.items()}
        with orc.conditioning() as margins:
            yo = orc.unet_forward(xo, sdo, **okw)
        if min(margins.values()) < 1e-6:          # fp32 conv outputs differ from fp64 by 1e-7 .. 3e-7 of their rms (measured, both engines)
            print("seed %d: smallest margins %s -- inside fp32 rounding, not a parity sample" % (seed, margins))
            continue
        checked += 1
        xg = G(x, True)
        y = net(xg)
        assert y.shape == yo.shape and y.shape[1] == net.final_nf
        assert rel_l2(N(y), yo.detach().numpy()) < 1e-5
        gy = rng.standard_normal(tuple(y.shape)).astype(np.float32)
        y.backward(G(gy))
        yo.backward(torch.from_numpy(gy).double())
        for name, p in net.named_parameters():
            assert rel_l2(N(p.grad), sdo["unet_model." + name].grad.numpy()) < 1e-4, (seed, name)
        assert rel_l2(N(xg.grad), xo.grad.numpy()) < 1e-4, seed
        break
    assert checked >= 1, "no well-conditioned seed among the four"


@pytest.mark.parametrize("tag", ["p3_vol", "aniso_vol", "p3_img", "p42_img"])
def test_unet_with_other_pooling_factors_vs_reference_golden(vxm, g_unetpools, tag):
    """Unet(max_pool = 3, per-axis tuples, per-level lists; networks.py:79-85,122-144) on the general-factor pooling kernels against the
    fixtures of the unmodified reference: output, gradient onto the input and onto every parameter.  (The fixtures hold single samples,
    not conditioned seeds: gates at the fp32-vs-fp32 level of two summation orders.)"""
    from conftest import UNET_POOL_CASES
    g = g_unetpools
    inshape, infeats, feats, pool = UNET_POOL_CASES[tag]
    net = vxm.networks.Unet(inshape=inshape, infeats=infeats, nb_features=feats, max_pool=pool).cuda()
    names = [str(n) for n in g[tag + "_grad_names"]]
    assert names == [k for k, _ in net.named_parameters()]
    net.load_state_dict({n: torch.from_numpy(g[tag + "_param_" + n]) for n in names})
    x = G(g[tag + "_x"], True)
    y = net(x)
    gate("unet %s output" % tag, rel_l2(N(y), g[tag + "_y"]), 2e-6)
    (y * G(g[tag + "_r"])).sum().backward()
    gate("unet %s grad x" % tag, rel_l2(N(x.grad), g[tag + "_gx"]), 4e-6)
    gate("unet %s grad enc0" % tag, rel_l2(N(net.encoder[0][0].main.weight.grad), g[tag + "_gw_enc0"]), 4e-6)
    for (n, p), ref in zip(net.named_parameters(), g[tag + "_grad_norms"]):
        assert abs(float(p.grad.double().norm()) - ref) <= 1e-4 * ref + 1e-6, (tag, n)


def test_unet_pooling_kernels_bit_exact_and_error_behaviour(vxm):
    """MaxPoolNd(k) / Upsample(k)+cat of the general-factor kernels against ATen on the same values (bit-exact: pure selection / copies;
    the gradient of the upsampling is a sum in a fixed order); a volume the pools do not divide is refused at the concat, as torch.cat
    refuses it in the reference."""
    from voxelmorph_amd.torch import functional as VF
    rng = np.random.default_rng(8)
    x = rng.standard_normal((2, 3, 7, 9, 11)).astype(np.float32)
    x[0, 0, :3, :3, :3] = 1.0                                     # ties: the first maximum of the scan takes the gradient
    for k in (3, (2, 3, 1), (1, 2, 4)):
        xg, xo = G(x, True), torch.from_numpy(x).requires_grad_()
        y, yo = VF.MaxPoolKFn.apply(xg, k), torch.nn.functional.max_pool3d(xo, k)
        assert torch.equal(y.cpu(), yo.detach()), k
        gy = rng.standard_normal(tuple(yo.shape)).astype(np.float32)
        y.backward(G(gy)); yo.backward(torch.from_numpy(gy))
        assert torch.equal(xg.grad.cpu(), xo.grad), k
    lo, sk = rng.standard_normal((2, 3, 2, 3, 2)).astype(np.float32), rng.standard_normal((2, 2, 6, 6, 2)).astype(np.float32)
    lg, sg = G(lo, True), G(sk, True)
    lt, st = torch.from_numpy(lo).requires_grad_(), torch.from_numpy(sk).requires_grad_()
    out = VF.UpsampleCatKFn.apply(lg, sg, (3, 2, 1))
    ref = torch.cat([torch.nn.functional.interpolate(lt, scale_factor=(3.0, 2.0, 1.0), mode="nearest"), st], dim=1)
    assert torch.equal(out.cpu(), ref.detach())
    go = rng.standard_normal(tuple(ref.shape)).astype(np.float32)
    out.backward(G(go)); ref.backward(torch.from_numpy(go))
    assert torch.equal(sg.grad.cpu(), st.grad)
    np.testing.assert_allclose(N(lg.grad), lt.grad.numpy(), rtol=1e-6, atol=1e-6)
    net = vxm.networks.Unet(inshape=(10, 9, 9), infeats=1, nb_features=[[4], [4, 4]], max_pool=3).cuda()
    with pytest.raises(RuntimeError, match="must match"):
        net(torch.zeros(1, 1, 10, 9, 9, device="cuda"))


@pytest.mark.parametrize("src_feats,trg_feats", [(2, 1), (1, 3)])
def test_vxm_dense_multi_feature_inputs_vs_oracle(vxm, src_feats, trg_feats):
    """networks.py:161-162 `src_feats` / `trg_feats`: the first block reads the virtual concat of a multi-channel source and target
    (3 / 4 input channels: the dense-K kernel with two segments), the warp moves every source channel; forward, loss and
    parameter gradients against the oracle."""
    inshape = (16, 32, 32)
    torch.manual_seed(11)
    model = vxm.networks.VxmDense(inshape, int_steps=3, int_downsize=2, src_feats=src_feats, trg_feats=trg_feats).cuda()
    with torch.no_grad():
        model.flow.weight.normal_(0, 0.05)
    sd = {k: v.detach().cpu().double().requires_grad_() for k, v in model.state_dict().items() if not k.endswith(".grid")}
    rng = np.random.default_rng(src_feats * 10 + trg_feats)
    src = rng.random((2, src_feats) + inshape).astype(np.float32)
    trg = rng.random((2, trg_feats) + inshape).astype(np.float32)
    y, pre = model(G(src), G(trg))
    yo, preo = orc.vxm_dense_forward(torch.from_numpy(src).double(), torch.from_numpy(trg).double(), sd, int_steps=3, int_downsize=2)
    assert y.shape == (2, src_feats) + inshape
    np.testing.assert_allclose(N(y), yo.detach().numpy(), atol=2e-5, rtol=0)
    np.testing.assert_allclose(N(pre), preo.detach().numpy(), atol=2e-5, rtol=0)
    loss = (y * y).mean() + vxm.losses.Grad("l2", loss_mult=2).loss(None, pre)
    losso = (yo * yo).mean() + orc.grad_loss(preo, "l2", 2)
    assert abs(float(loss) - float(losso)) < 1e-5
    loss.backward()
    losso.backward()
    for name, p in model.named_parameters():
        assert rel_l2(N(p.grad), sd[name].grad.numpy()) < 2e-4, name


@pytest.mark.parametrize("feats,image_loss", [(1, "ncc"), (2, "mse")])
def test_step_on_inputs_built_as_the_reference_training_loop_builds_them(vxm, feats, image_loss):
    """Drop-in proof for the caller: scripts/torch/train.py:199-201 hands the model `torch.from_numpy(d).to(device).float().permute(0, 4, 1, 2, 3)`
    of the generators' float64 [B, *vol, C] arrays -- a channels-last VIEW (non-contiguous for C > 1) -- and the same for y_true, including
    the zero "true flow" that Grad ignores (generators.py:98-105, losses.py:122).  Model + losses + backward on exactly those tensors,
    combined with the loop's weighted sum (train.py:205-212), against the oracle on the contiguous copies."""
    inshape, B, lam = (16, 32, 32), 2, 0.02
    torch.manual_seed(21)
    model = vxm.networks.VxmDense(inshape, int_steps=3, int_downsize=2, src_feats=feats, trg_feats=feats).cuda()
    with torch.no_grad():
        model.flow.weight.normal_(0, 0.05)
    sd = {k: v.detach().cpu().double().requires_grad_() for k, v in model.state_dict().items() if not k.endswith(".grid")}
    rng = np.random.default_rng(40 + feats)
    invols = [rng.random((B,) + inshape + (feats,)) for _ in range(2)]                       # float64, feature axis last (generators.py:89-95)
    outvols = [invols[1], np.zeros((B,) + inshape + (3,))]
    inputs = [torch.from_numpy(d).to("cuda").float().permute(0, 4, 1, 2, 3) for d in invols]      # train.py:200
    y_true = [torch.from_numpy(d).to("cuda").float().permute(0, 4, 1, 2, 3) for d in outvols]     # train.py:201
    assert feats == 1 or not inputs[0].is_contiguous()
    img = vxm.losses.NCC().loss if image_loss == "ncc" else vxm.losses.MSE().loss
    losses, weights = [img, vxm.losses.Grad("l2", loss_mult=2).loss], [1.0, lam]
    y_pred = model(*inputs)
    loss = vxm.losses.weighted_sum([fn(y_true[n], y_pred[n]) for n, fn in enumerate(losses)], weights)
    ref_list = 0
    for n, fn in enumerate(losses):                                                                # the loop of train.py:205-212 itself
        ref_list = ref_list + fn(y_true[n], y_pred[n]) * weights[n]
    assert abs(float(loss) - float(ref_list)) <= 1e-7 * max(1.0, abs(float(ref_list)))
    loss.backward()
    src, trg = (torch.from_numpy(np.ascontiguousarray(np.moveaxis(d, -1, 1))).float().double() for d in invols)
    losso, (_, _, yo, preo) = orc.train_step_loss(src, trg, sd, image_loss, lam, int_steps=3, int_downsize=2)
    losso.backward()
    np.testing.assert_allclose(N(y_pred[0]), yo.detach().numpy(), atol=2e-5, rtol=0)
    np.testing.assert_allclose(N(y_pred[1]), preo.detach().numpy(), atol=2e-5, rtol=0)
    assert abs(float(loss) - float(losso)) < 2e-5, (float(loss), float(losso))
    # (NCC in fp32 on a 16 x 32 x 32 noise pair against the fp64 oracle: the variance terms cancel to ~1e-4 relative on the coarsest
    # level's weight gradients, measured 2.3e-4; the fp32 evaluations of the reference itself differ by more -- DESIGN.md section 2)
    # (the first layer of the four-channel MSE case: 2.3e-4 -- a small volume, two samples, the fp16-piece engine against fp64)
    bound = 1e-3
    for name, p in model.named_parameters():
        assert rel_l2(N(p.grad), sd[name].grad.numpy()) < bound, name


@pytest.mark.parametrize("int_downsize,int_steps,half_res", [(1, 2, False), (4, 3, False), (2, 3, True)])
def test_vxm_dense_integration_variants_vs_oracle(vxm, int_downsize, int_steps, half_res):
    """networks.py:223-242: integration at full resolution (no resize), at quarter resolution (ResizeTransform 4 and 1/4), and with
    `unet_half_res` (the U-Net already ends at half resolution: no down-resize, networks.py:223); forward and gradients."""
    inshape = (32, 32, 32)
    torch.manual_seed(5)
    model = vxm.networks.VxmDense(inshape, int_steps=int_steps, int_downsize=int_downsize, unet_half_res=half_res).cuda()
    with torch.no_grad():
        model.flow.weight.normal_(0, 0.05)
    sd = {k: v.detach().cpu().double().requires_grad_() for k, v in model.state_dict().items() if not k.endswith(".grid")}
    rng = np.random.default_rng(int_downsize)
    src, trg = (rng.random((1, 1) + inshape).astype(np.float32) for _ in range(2))
    y, pre = model(G(src), G(trg))
    yo, preo = orc.vxm_dense_forward(torch.from_numpy(src).double(), torch.from_numpy(trg).double(), sd, int_steps=int_steps,
                                     int_downsize=int_downsize, unet_half_res=half_res)
    assert pre.shape == preo.shape
    np.testing.assert_allclose(N(y), yo.detach().numpy(), atol=2e-5, rtol=0)
    np.testing.assert_allclose(N(pre), preo.detach().numpy(), atol=2e-5, rtol=0)
    loss = (y * y).mean() + (pre * pre).mean()
    losso = (yo * yo).mean() + (preo * preo).mean()
    loss.backward()
    losso.backward()
    for name, p in model.named_parameters():
        assert rel_l2(N(p.grad), sd[name].grad.numpy()) < 5e-4, name      # fp32 path vs fp64 oracle through 9 blocks and the integration


# ------------------------------------------------------------------ VxmDense (golden, produced by the reference)
CASES = {
    "diffeo": dict(int_steps=7, int_downsize=2, bidir=False, loss="ncc", lam=1.0),
    "dense": dict(int_steps=0, int_downsize=2, bidir=False, loss="mse", lam=0.01),
    "bidir": dict(int_steps=3, int_downsize=2, bidir=True, loss="mse", lam=0.01),
}


def _build(vxm, g_network, cfg):
    inshape = tuple(int(v) for v in g_network["inshape"])
    model = vxm.networks.VxmDense(inshape, int_steps=cfg["int_steps"], int_downsize=cfg["int_downsize"], bidir=cfg["bidir"])
    sd = orc.seeded_state_dict(inshape, seed=5, flow_std=0.2)
    res = model.load_state_dict(sd, strict=False)
    assert all(k.endswith(".grid") for k in res.missing_keys) and not res.unexpected_keys
    return model.cuda()


@pytest.mark.parametrize("tag", list(CASES))
def test_vxm_dense_golden(vxm, g_network, tag):
    cfg = CASES[tag]
    model = _build(vxm, g_network, cfg)
    src, trg = G(g_network["source"]), G(g_network["target"])
    pred = model(src, trg)
    img_fn = vxm.losses.NCC().loss if cfg["loss"] == "ncc" else vxm.losses.MSE().loss
    if cfg["bidir"]:
        img = 0.5 * img_fn(trg, pred[0]) + 0.5 * img_fn(src, pred[1])
        np.testing.assert_allclose(N(pred[1]), g_network[tag + "_y_target"], atol=2e-5, rtol=0)
    else:
        img = img_fn(trg, pred[0])
    reg = vxm.losses.Grad("l2", loss_mult=cfg["int_downsize"]).loss(None, pred[-1])
    loss = img + cfg["lam"] * reg
    np.testing.assert_allclose(N(pred[0]), g_network[tag + "_y_source"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(N(pred[-1]), g_network[tag + "_preint"], atol=2e-5, rtol=0)
    ref = g_network[tag + "_loss"]
    assert abs(float(loss) - ref[0]) < 1e-3 * max(1.0, abs(ref[0]))
    assert abs(float(reg) - ref[2]) < 1e-4 * max(1.0, abs(ref[2]))
    loss.backward()
    names = [str(n) for n in g_network[tag + "_grad_names"]]
    norms = g_network[tag + "_grad_norms"]
    params = dict(model.named_parameters())
    tol = 2e-3 if cfg["loss"] == "ncc" else 1e-4      # NCC's fp32 formula is ill-conditioned
    worst_n = worst_g = 0.0
    for n, r in zip(names, norms):
        got = float(params[n].grad.double().norm())
        worst_n = max(worst_n, abs(got - r) / max(r, 1e-12))
        assert abs(got - r) <= tol * max(r, 1e-12), (n, got, r)
    for key in g_network.files:
        if key.startswith(tag + "_grad_") and key not in (tag + "_grad_names", tag + "_grad_norms"):
            pname = key[len(tag + "_grad_"):]
            e = rel_l2(N(params[pname].grad), g_network[key])
            worst_g = max(worst_g, e)
            assert e < tol, (pname, e)
    print("golden %s: worst gradient-norm error %.2e, worst gradient rel-L2 %.2e (tol %.0e)" % (tag, worst_n, worst_g, tol))
    with torch.no_grad():
        _, pos = model(src, trg, registration=True)
    np.testing.assert_allclose(N(pos), g_network[tag + "_pos_flow"], atol=1e-4, rtol=0)
    # one Adam step through the fused flat-buffer optimiser (train.py:161,218-220)
    from voxelmorph_amd.optim import FlatAdam
    opt = FlatAdam(model, lr=1e-4)
    opt.load_grads_from_params()
    opt.step()
    assert rel_l2(N(model.flow.weight), g_network[tag + "_flow_weight_after_adam"]) < 1e-4
    assert rel_l2(N(model.unet_model.encoder[0][0].main.weight), g_network[tag + "_enc0_weight_after_adam"]) < 1e-5


def test_semisupervised_seg_vs_oracle(vxm):
    """BASELINE.json configs[4] wiring (VxmDense + warped half-resolution one-hot segmentation + Dice) against the
    oracle composition, forward and parameter gradients; label evaluation by the bit-exact nearest warp."""
    inshape, nb_labels = (32, 32, 32), 5
    rng = np.random.default_rng(21)
    src = rng.random((2, 1) + inshape).astype(np.float32)
    trg = rng.random((2, 1) + inshape).astype(np.float32)
    lab = rng.integers(0, nb_labels, size=(2,) + tuple(s // 2 for s in inshape))
    seg_src = np.stack([(lab == k) for k in range(nb_labels)], 1).astype(np.float32)
    lab_t = rng.integers(0, nb_labels, size=lab.shape)
    seg_trg = np.stack([(lab_t == k) for k in range(nb_labels)], 1).astype(np.float32)
    sd = orc.seeded_state_dict(inshape, seed=3, flow_std=0.2)
    model = vxm.networks.VxmDenseSemiSupervisedSeg(inshape, nb_labels, int_steps=5, int_downsize=2)
    res = model.vxm_model.load_state_dict(sd, strict=False)
    assert all(k.endswith(".grid") for k in res.missing_keys) and not res.unexpected_keys
    model = model.cuda()
    y, pre, yseg = model(G(src), G(trg), G(seg_src))
    loss = vxm.losses.MSE().loss(G(trg), y) + 0.02 * vxm.losses.Grad("l2", loss_mult=2).loss(None, pre) \
        + 0.01 * vxm.losses.Dice().loss(G(seg_trg), yseg)
    loss.backward()
    sdo = {k: v.clone().double().requires_grad_() for k, v in sd.items()}
    to = lambda a: torch.from_numpy(a).double()
    yo, preo, ysego, poso = orc.vxm_semisupervised_forward(to(src), to(trg), to(seg_src), sdo, int_steps=5)
    losso = orc.mse_loss(to(trg), yo) + 0.02 * orc.grad_loss(preo, "l2", 2) + 0.01 * orc.dice_loss(to(seg_trg), ysego)
    losso.backward()
    np.testing.assert_allclose(N(yseg), ysego.detach().numpy(), atol=2e-5)
    assert abs(float(loss) - float(losso)) < 1e-5
    for name, p in model.vxm_model.named_parameters():
        assert rel_l2(N(p.grad), sdo[name].grad.numpy()) < 2e-4, name
    # evaluation protocol (scripts/tf/test.py:80-112): nearest warp of the full-resolution label map, then Dice
    full = rng.integers(0, nb_labels, size=(2, 1) + inshape).astype(np.float32)
    moved = model.apply_transform(G(src), G(trg), G(full), interp_method="nearest")
    ref = c_oracle.warp3d(full, poso.detach().float().numpy(), mode="nearest")
    agree = float((N(moved) == ref).mean())
    assert agree > 0.999          # the flow itself differs by fp32 rounding between the two paths: ties may flip
    d_hip = orc.dice_metric(N(moved)[0, 0], full[0, 0], labels=list(range(1, nb_labels)))
    d_ref = orc.dice_metric(ref[0, 0], full[0, 0], labels=list(range(1, nb_labels)))
    assert np.abs(np.asarray(d_hip) - np.asarray(d_ref)).max() < 1e-3


def test_pair_loader_resident_and_streaming(vxm):
    """Data path: batches are [B,1,D,H,W] fp32 on the device, every sample is one of the source
    volumes bit for bit, ranks draw different pairs, the zero flow target has the reference's role (generators.py:98-105)."""
    from voxelmorph_amd import data as vdata
    rng = np.random.default_rng(1)
    vols = [rng.random((8, 12, 16)) for _ in range(5)]              # float64 like the reference's npz volumes
    ref = np.stack(vols).astype(np.float32)
    for resident_bytes in (1 << 30, 0):                              # resident in HBM / streamed through pinned staging
        ld = vdata.scan_to_scan(vols, batch_size=3, bidir=True, device="cuda", rank=0, seed=7, resident_bytes=resident_bytes)
        assert ld.resident == (resident_bytes > 0)
        for _ in range(4):
            (s1, s2), (t1, t2, z) = next(ld)
            assert s1.shape == (3, 1, 8, 12, 16) and s1.dtype == torch.float32 and s1.is_cuda and s1.is_contiguous()
            assert t1 is s2 and t2 is s1 and z.shape == (3, 3, 8, 12, 16) and float(z.abs().max()) == 0.0
            for t in (s1, s2):
                for b in range(3):
                    assert any(np.array_equal(N(t)[b, 0], ref[i]) for i in range(5))
    a = vdata.PairLoader(vols, batch_size=4, device="cuda", rank=0, seed=7)
    b = vdata.PairLoader(vols, batch_size=4, device="cuda", rank=1, seed=7)
    assert not all(torch.equal(next(a)[0][0], next(b)[0][0]) for _ in range(4))


def test_train_and_register_cli_end_to_end(vxm, tmp_path):
    """scripts/train.py (flags of scripts/torch/train.py) for a few steps on synthetic volumes, then scripts/register.py
    (flags of scripts/torch/register.py) on its checkpoint: moved / warp / nearest-warped labels come out."""
    import subprocess
    import sys
    rng = np.random.default_rng(3)
    base = rng.random((32, 32, 32)).astype(np.float32)
    names = []
    for i in range(4):
        v = np.roll(base, shift=i, axis=2) + 0.05 * rng.random(base.shape).astype(np.float32)
        np.savez(tmp_path / ("v%d.npz" % i), vol=v, seg=(v > 0.5).astype(np.float32))
        names.append(str(tmp_path / ("v%d.npz" % i)))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "train.py"), "--img-list", str(tmp_path / "list.txt"),
                        "--model-dir", str(tmp_path / "models"), "--epochs", "3", "--steps-per-epoch", "6", "--image-loss", "ncc",
                        "--lambda", "1", "--lr", "1e-3"], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(ln.split("loss:")[1].split()[0]) for ln in r.stdout.splitlines() if "loss:" in ln]
    assert len(losses) == 3 and all(np.isfinite(losses)) and all(v < 0 for v in losses)     # NCC + small smoothness term
    ckpt = tmp_path / "models" / "0003.pt"
    assert ckpt.exists() and (tmp_path / "models" / "0000.pt").exists()
    np.savez(tmp_path / "seg.npz", vol=(base > 0.5).astype(np.float32))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "register.py"), "--moving", names[0], "--fixed", names[1],
                        "--moved", str(tmp_path / "moved.npz"), "--warp", str(tmp_path / "warp.npz"), "--model", str(ckpt),
                        "--seg", str(tmp_path / "seg.npz"), "--moved-seg", str(tmp_path / "mseg.npz"), "--jacobian"],
                       capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert np.load(tmp_path / "moved.npz")["vol"].shape == (32, 32, 32)
    assert np.load(tmp_path / "warp.npz")["vol"].shape == (3, 32, 32, 32)
    assert set(np.unique(np.load(tmp_path / "mseg.npz")["vol"])) <= {0.0, 1.0}
    assert "non-positive Jacobian fraction" in r.stdout
    # the reference's default file type: NIfTI in and out (voxelmorph_amd/nifti.py, no nibabel); the outputs carry the FIXED image's affine
    from voxelmorph_amd import data as vdata
    aff = np.array([[-1.0, 0, 0, 16.0], [0, 0, 1.0, -16.0], [0, -1.0, 0, 16.0], [0, 0, 0, 1.0]])
    aff_fixed = aff.copy()
    aff_fixed[:3, 3] += 2.0
    vdata.save_volfile(np.load(names[0])["vol"], str(tmp_path / "mov.nii.gz"), aff)
    vdata.save_volfile(np.load(names[1])["vol"], str(tmp_path / "fix.nii.gz"), aff_fixed)
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "register.py"), "--moving", str(tmp_path / "mov.nii.gz"), "--fixed",
                        str(tmp_path / "fix.nii.gz"), "--moved", str(tmp_path / "moved.nii.gz"), "--warp", str(tmp_path / "warp.nii.gz"),
                        "--model", str(ckpt)], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    mv, am = vdata.load_volfile(str(tmp_path / "moved.nii.gz"), ret_affine=True)
    np.testing.assert_allclose(am, aff_fixed, atol=1e-5)
    np.testing.assert_allclose(mv, np.load(tmp_path / "moved.npz")["vol"], atol=1e-6)          # same registration as the npz run
    assert vdata.load_volfile(str(tmp_path / "warp.nii.gz")).shape == (3, 32, 32, 32)


def test_checkpoint_roundtrip_reference_format(vxm, g_network, tmp_path):
    model = _build(vxm, g_network, CASES["diffeo"])
    path = os.path.join(tmp_path, "m.pt")
    model.save(path)
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"config", "model_state"}
    keys = [str(k) for k in g_network["state_keys"] if not str(k).endswith(".grid")]
    assert list(ck["model_state"].keys()) == keys
    assert ck["config"]["int_steps"] == 7 and ck["config"]["inshape"] == tuple(int(v) for v in g_network["inshape"])
    again = vxm.networks.VxmDense.load(path, "cuda")
    for (k, a), (_, b) in zip(model.state_dict().items(), again.state_dict().items()):
        assert torch.equal(a.cpu(), b.cpu()), k


# ------------------------------------------------------------------ fullsize + final warp as one kernel (networks.py:275-280)
@pytest.mark.parametrize("low,C,B", [((16, 24, 40), 1, 1), ((10, 12, 18), 2, 2), ((21, 13, 35), 1, 1), ((6, 8, 8), 1, 1)])
def test_fused_fullsize_warp_equals_resize_then_warp(vxm, low, C, B):
    """functional.WarpUpFn (vxm_warp3d_up_fwd / _bwd) against ResizeTransform(1/2) followed by SpatialTransformer: moved image and returned
    displacement bit for bit in both modes (the fused kernel evaluates the resize kernel's expression and the warp kernel's coordinate
    arithmetic), the gradient onto the low-resolution field against the two-kernel path and against the fp64 oracle; tiles that are ragged
    in every axis, two channels, two samples, a ratio below the marching resize-backward kernel's range (6 -> 12: 5/11)."""
    from voxelmorph_amd.torch import functional as VF
    full = tuple(2 * s for s in low)
    rng = np.random.default_rng(sum(low) + C)
    fl = (rng.standard_normal((B, 3) + low) * 1.2).astype(np.float32)
    img = rng.random((B, C) + full).astype(np.float32)
    gout = rng.standard_normal((B, C) + full).astype(np.float32)
    src = G(img)
    assert VF.warp_up_ok(src, G(fl))
    for mode in ("bilinear", "nearest"):
        a, b = G(fl, True), G(fl, True)
        out, pos = VF.WarpUpFn.apply(src, a, 2.0, mode, True)
        pos2 = VF.ResizeFn.apply(b, 2.0)
        out2 = VF.WarpFn.apply(src, pos2, mode)
        assert torch.equal(pos, pos2) and torch.equal(out, out2), (mode, float((out - out2).abs().max()))
        only = VF.WarpUpFn.apply(src, a, 2.0, mode, False)             # without the displacement output: same image
        assert torch.equal(only, out)
        out.backward(G(gout))
        out2.backward(G(gout))
        if mode == "nearest":
            assert float(a.grad.abs().max()) == 0.0 and float(b.grad.abs().max()) == 0.0
            continue
        gate("fused fullsize+warp: gradient vs the two-kernel path %s" % (low,), rel_l2(N(a.grad), N(b.grad)), 1e-6)
        # the oracle in the reference's own dtype: d(trilinear sample)/d(flow) jumps where a coordinate crosses an integer, and an fp64
        # evaluation puts ~1 voxel per 10^5 in the neighbouring cell (measured: 3e-3 rel-L2 from ONE such voxel)
        fd = torch.from_numpy(fl).requires_grad_()
        ref = orc.spatial_transformer(torch.from_numpy(img), orc.resize_transform(fd, 0.5))
        ref.backward(torch.from_numpy(gout))
        np.testing.assert_allclose(N(out), ref.detach().numpy(), atol=2e-5, rtol=0)
        gate("fused fullsize+warp: gradient vs the fp32 oracle %s" % (low,), rel_l2(N(a.grad), fd.grad.numpy()), 2e-5)


@pytest.mark.parametrize("low,BC", [((10, 12, 18), (2, 3)), ((24, 17, 33), (1, 3)), ((40, 48, 56), (1, 1)), ((9, 40, 70), (1, 2))])
def test_resize_upsampling_backward_marching_kernel_vs_oracle(vxm, low, BC):
    """k_resize3d_bwd_march (round 6: one thread per input voxel marching through the output planes; ratios in [0.47, 0.75)) against the
    autograd of the oracle's ResizeTransform (layers.py:85-97): ragged tiles in H and W, several depth segments, the x2 rescale."""
    B, C = BC
    rng = np.random.default_rng(sum(low))
    x = (rng.standard_normal((B, C) + low)).astype(np.float32)
    g = rng.standard_normal((B, C) + tuple(2 * s for s in low)).astype(np.float32)
    xg = G(x, True)
    up = vxm.layers.ResizeTransform(0.5, 3)(xg)
    up.backward(G(g))
    # the oracle in the reference's dtype: ATen evaluates `ratio * dst` in fp32, so at index ~100 its interpolation weights sit ~1e-6 from
    # the fp64 ones -- and the kernels reproduce the fp32 arithmetic (against fp64 the gap grows with the volume: 2.6e-7 / 7.5e-7 / 1.4e-6)
    xd = torch.from_numpy(x).requires_grad_()
    upd = orc.resize_transform(xd, 0.5)
    upd.backward(torch.from_numpy(g))
    np.testing.assert_allclose(N(up), upd.detach().numpy(), atol=1e-5, rtol=0)
    gate("resize x2 backward (marching) %s" % (low,), rel_l2(N(xg.grad), xd.grad.numpy()), 1e-6)
    up2 = vxm.layers.ResizeTransform(0.5, 3)(xg)                      # deterministic: no atomics
    xg.grad = None
    up2.backward(G(g))
    first = N(xg.grad).copy()
    xg.grad = None
    vxm.layers.ResizeTransform(0.5, 3)(xg).backward(G(g))
    assert np.array_equal(first, N(xg.grad))


_RESIZE_REF = {}


def _resize_reference(key, x, g, vel):
    """float64 arbiter of one case (oracle.resize_transform and its autograd), computed once per process and left unchanged"""
    if key not in _RESIZE_REF:
        xd = torch.from_numpy(x).double().requires_grad_()
        y = orc.resize_transform(xd, vel)
        y.backward(torch.from_numpy(g).double())
        _RESIZE_REF[key] = (y.detach().numpy(), xd.grad.numpy())
    return _RESIZE_REF[key]


def _resize_switch_is_sep():
    return os.environ.get("VXM_RESIZE_BWD", "")[:1] == "s"


@pytest.mark.parametrize("case", rc.CASES, ids=rc.IDS)
def test_resize_every_backward_kernel_vs_fp64(vxm, case):
    """Each of the five kernels vxm_resize3d_bwd chooses between (and the one forward kernel) at the edges of its range -- ratios away from
    1/2, several tiles and depth blocks, ragged tiles, odd extents, an LDS block that does not fit, output axes of extent 1, input voxels
    no output names -- against the float64 evaluation of the reference's ResizeTransform; gates from the reference's own fp32 error
    (RESIZE_* above).  The kernel the dispatcher picks is asserted first: a threshold that moves fails here, it does not move a shape to
    another kernel unseen.  Under VXM_RESIZE_BWD=sep (test_resize_backward_sep_switch_in_subprocess) march shapes run sep, down shapes
    gather_tiled."""
    from voxelmorph_amd import _lib
    name, inp, vel, out, code = case
    if _resize_switch_is_sep():
        code = {rc.MARCH: rc.SEP, rc.DOWN: rc.GATHER_TILED}.get(code, code)
    assert _lib.lib().vxm_resize3d_bwd_kernel(*inp, *out) == code
    tag = "resize %s [%s]" % (name, rc.KERNELS[code])
    x, g = rc.arrays(case)
    assert g.shape[2:] == out
    y64, gx64 = _resize_reference(name, x, g, vel)
    layer = vxm.layers.ResizeTransform(vel, 3)
    xg = G(x, True)
    y = layer(xg)
    assert tuple(y.shape) == g.shape
    factor = 1.0 / vel
    np.testing.assert_allclose(N(y), c_oracle.resize3d(x, vel), atol=5e-6 * max(1.0, factor), rtol=0)
    gate(tag + " forward vs fp64", rel_l2(N(y), y64), RESIZE_FWD_GATE)
    y.backward(G(g))
    gx = N(xg.grad).copy()
    gate(tag + " backward vs fp64", rel_l2(gx, gx64), RESIZE_BWD_GATE)
    gate(tag + " adjoint <y,g> - <x,gx>", rc.adjoint_gap(N(y), g, x, gx), RESIZE_ADJ_GATE)
    if code != rc.SCATTER:                                        # documented as deterministic: no atomics
        xg.grad = None
        layer(xg).backward(G(g))
        assert torch.equal(xg.grad.cpu(), torch.from_numpy(gx)), tag + ": two backward runs differ"
    if name in rc.SKIPPING:
        # voxels no output names: exactly 0 (written, not left uninitialised), and a NaN in one gradient voxel reaches the voxels the
        # reference's fp32 autograd carries it to (the up to 8 that output names, one with weight 0 where the source coordinate is an
        # integer) and no other -- a kernel that multiplies a clamped load by a zero weight spreads it
        ones = torch.from_numpy(x).requires_grad_()
        orc.resize_transform(ones, vel).backward(torch.ones(g.shape))
        unnamed = ones.grad.numpy() == 0
        assert unnamed.sum() > x.size // 2 and np.all(gx[unnamed] == 0)
        gn = g.copy()
        gn[0, 1, out[0] // 2, out[1] // 2, out[2] // 2] = np.nan
        xr = torch.from_numpy(x).requires_grad_()
        orc.resize_transform(xr, vel).backward(torch.from_numpy(gn))
        want = np.isnan(xr.grad.numpy())
        xg.grad = None
        layer(xg).backward(G(gn))
        got = N(xg.grad)
        assert 1 <= want.sum() <= 8
        assert np.array_equal(np.isnan(got), want), "%s: NaN voxels %s, the reference's %s" % (tag, np.argwhere(np.isnan(got)).tolist(), np.argwhere(want).tolist())
        assert np.all(got[unnamed & ~want] == 0)


def test_resize_backward_sep_switch_in_subprocess():
    """VXM_RESIZE_BWD=sep (read once per process, hence the fresh child) takes the marching kernel out of the choice: the three march rows
    of the table run k_resize3d_bwd_sep -- (9,17,33) on tiles that all fit its LDS block -- against the same fp64 gradient and gates."""
    import subprocess
    import sys
    env = dict(os.environ, VXM_RESIZE_BWD="sep")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", os.path.join(root, "tests", "test_gpu_parity.py"),
                        "-k", "test_resize_every_backward_kernel_vs_fp64 and march"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=120)
    print("\n".join(line for line in r.stdout.splitlines() if line.startswith("[gate]")))
    assert r.returncode == 0 and "3 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("vel", rc.PLANAR_VELS, ids=["vel0.8", "vel1/3", "vel3", "vel1.5"])
@pytest.mark.parametrize("shape", rc.PLANAR_SHAPES, ids=["13x37", "2x9"])
def test_resize_planar_vs_fp64(vxm, shape, vel):
    """ResizeTransform(vel, 2) (k_resize2d_fwd / k_resize2d_bwd, a scatter: no repeatability to assert) against the float64 oracle: forward,
    backward and the adjoint identity at odd extents, two rows, an output of one row (2 rows x 1/1.5), and the case with NO output row
    (2 rows x 1/3), which the reference refuses and the product must refuse too."""
    from voxelmorph_amd import _lib
    x, g = rc.planar_arrays(shape, vel)
    layer = vxm.layers.ResizeTransform(vel, 2)
    if g is None:
        with pytest.raises(RuntimeError):
            orc.resize_transform(torch.from_numpy(x), vel)
        with pytest.raises(_lib.VxmHipError, match="bad output shape"):
            layer(G(x))
        return
    tag = "resize 2-D %s vel_resize %.3g" % (shape, vel)
    y64, gx64 = _resize_reference(("2d", shape, vel), x, g, vel)
    xg = G(x, True)
    y = layer(xg)
    assert tuple(y.shape) == g.shape
    gate(tag + " forward vs fp64", rel_l2(N(y), y64), RESIZE2D_FWD_GATE)
    y.backward(G(g))
    gate(tag + " backward vs fp64", rel_l2(N(xg.grad), gx64), RESIZE2D_BWD_GATE)
    gate(tag + " adjoint <y,g> - <x,gx>", rc.adjoint_gap(N(y), g, x, N(xg.grad)), RESIZE2D_ADJ_GATE)


# ------------------------------------------------------------------ full benchmark size (160x192x224): properties
FULL = (160, 192, 224)


def test_full_size_identity_and_nearest(vxm):
    rng = np.random.default_rng(0)
    seg = torch.from_numpy(rng.integers(0, 46, size=(1, 1) + FULL).astype(np.float32)).cuda()
    zero = torch.zeros(1, 3, *FULL, device="cuda")
    assert torch.equal(vxm.layers.SpatialTransformer(FULL, mode="nearest").cuda()(seg, zero), seg)      # index grid exact
    img = torch.rand(1, 1, *FULL, device="cuda")
    out = vxm.layers.SpatialTransformer(FULL).cuda()(img, zero)
    # not exact in the reference either: its normalise/un-normalise round trip perturbs integer coordinates
    # by up to 7.6e-6 per axis, i.e. up to ~2.3e-5 on U[0,1) noise
    assert float((out - img).abs().max()) <= 3e-5
    ref = orc.spatial_transformer(img.cpu(), zero.cpu())            # the oracle carries the same perturbation
    assert float((out.cpu() - ref).abs().max()) <= 1e-5
    # integer shift by +1 voxel along W == slicing (away from the border), for both modes
    shift = zero.clone()
    shift[:, 2] = 1.0
    for mode in ("nearest", "bilinear"):
        o = vxm.layers.SpatialTransformer(FULL, mode=mode).cuda()(img, shift)
        assert float((o[..., :-1] - img[..., 1:]).abs().max()) <= (0.0 if mode == "nearest" else 3e-5)
        assert float(o[..., -1].abs().max()) == 0.0                                                   # zeros padding


def test_full_size_dice_of_warped_labels_matches_oracle(vxm):
    rng = np.random.default_rng(1)
    lab = rng.integers(0, 30, size=(1, 1, 40, 48, 56)).astype(np.float32)
    seg = np.kron(lab, np.ones((1, 1, 4, 4, 4), np.float32))                 # blocky label map at 160x192x224
    flow = orc.resize_explicit((rng.standard_normal((1, 3, 20, 24, 28)) * 0.6).astype(np.float32), 1 / 8)   # smooth, |v| ~ 5
    warped = N(vxm.layers.SpatialTransformer(FULL, mode="nearest").cuda()(G(seg), G(flow)))
    ref = c_oracle.warp3d(seg, flow, mode="nearest")
    assert np.array_equal(warped, ref)
    labels = np.arange(1, 30)
    d_gpu = orc.dice_metric(warped[0, 0], seg[0, 0], labels).mean()
    d_ref = orc.dice_metric(ref[0, 0], seg[0, 0], labels).mean()
    assert abs(d_gpu - d_ref) <= 1e-3


def _full_size_step_vs_oracle(vxm, src, trg, seed, flow_std, fp64_ncc_arbiter=False):
    """One headline-config training step (VxmDense 160x192x224, int_steps=7, int_downsize=2, NCC(9^3) + Grad('l2', x2),
    lambda 1; scripts/torch/train.py:194-223) on the HIP path against `oracle.vxm_oracle.train_step_loss` on the host cores:
    forward tensors, loss and every parameter gradient.  Returns the GPU model and the positive full-resolution flow.

    fp64_ncc_arbiter: the reference's fp32 NCC formula cancels catastrophically where the image is locally flat (SURVEY.md §7;
    a real scan is, noise is not), so two fp32 evaluations of it in different summation orders differ by more than either differs
    from the exact value.  The gradients are then judged against the oracle with the NCC term evaluated in fp64 (same fp32
    network), and the HIP path must be at least as close to it as the reference-order fp32 evaluation is (factor 2 of slack)."""
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    sd = orc.seeded_state_dict(FULL, seed=seed, flow_std=flow_std)
    model = vxm.networks.VxmDense(FULL, int_steps=7, int_downsize=2)
    res = model.load_state_dict(sd, strict=False)
    assert all(k.endswith(".grid") for k in res.missing_keys) and not res.unexpected_keys
    model = model.cuda()
    s, t = G(src), G(trg)
    y, pre = model(s, t)                                       # the training outputs: fullsize + transformer as one kernel, no pos_flow in HBM
    loss = vxm.losses.NCC().loss(t, y) + vxm.losses.Grad("l2", loss_mult=2).loss(None, pre)
    loss.backward()
    with torch.no_grad():
        y_reg, pos = model(s, t, registration=True)            # the same kernel with the displacement written out (register.py:87)
    assert torch.equal(y_reg, y)
    torch.cuda.synchronize()
    assert tuple(y.shape) == tuple(src.shape) and tuple(pre.shape) == (src.shape[0], 3) + tuple(d // 2 for d in FULL)
    sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
    names, params = list(sdo), list(sdo.values())
    ts = torch.from_numpy(trg)
    ref, (_, reg, ys, pres) = orc.train_step_loss(torch.from_numpy(src), ts, sdo, "ncc", 1.0)
    g32 = dict(zip(names, torch.autograd.grad(ref, params, retain_graph=fp64_ncc_arbiter)))
    err_y = float((y.detach().cpu() - ys.detach()).abs().max())
    err_p = float((pre.detach().cpu() - pres.detach()).abs().max())
    gerr = {name: rel_l2(N(p.grad), g32[name].numpy()) for name, p in model.named_parameters()}
    worst = max(gerr, key=gerr.get)
    print("full-size step: loss hip=%.7f oracle=%.7f | max|dy|=%.2e max|dpreint|=%.2e | worst grad rel-L2 vs fp32 oracle %.2e (%s)"
          % (float(loss), float(ref), err_y, err_p, gerr[worst], worst))
    # preint_flow is a conv output (<= 2e-5 abs).  y_source is an image sampled at (voxel + integrated flow): the stated
    # tolerance of the integrated flows is 1e-4 abs (fp32 scaling and squaring drifts 3.9e-5 against fp64 after 7
    # steps) and a U[0,1) noise image changes by O(1) per voxel, so the moved image inherits that bound, not the 1e-5 of a
    # single warp on identical flows.
    # measured (round 2, native fp32 engine): err_y 6e-6 .. 3e-5, err_p <= 1e-7, worst gradient 1.8e-5 on the noise pair
    assert err_p <= 2e-5 and err_y <= 5e-5, (err_y, err_p)
    assert abs(float(loss) - float(ref)) <= 1e-3
    assert len(gerr) == 24
    if not fp64_ncc_arbiter:
        for name, e in gerr.items():
            assert e <= 1e-4, (name, e)                  # the stated parameter-gradient tolerance (module docstring)
    else:
        ref64 = orc.ncc_loss(ts, ys, dtype=torch.float64).float() + reg
        g64 = dict(zip(names, torch.autograd.grad(ref64, params)))
        assert abs(float(loss) - float(ref64)) <= 1e-3
        for name, p in model.named_parameters():
            e_hip, e_ref = rel_l2(N(p.grad), g64[name].numpy()), rel_l2(g32[name].numpy(), g64[name].numpy())
            print("  %-40s vs fp64-NCC arbiter: hip %.2e, fp32 oracle %.2e" % (name, e_hip, e_ref))
            assert e_hip <= max(3e-4, 2.0 * e_ref), (name, e_hip, e_ref)       # measured 1.0e-5 .. 1.4e-4
    return model, pos.detach()


def test_full_size_train_step_vs_oracle_noise_pair(vxm):
    """BASELINE.json configs[2] at the size the metric is quoted on, noise pairs U[0,1), flow weights
    N(0, 0.05) so that the integrated field is a real deformation (|v| up to ~1 voxel at half resolution) rather than the
    near-identity of the N(0, 1e-5) start."""
    rng = np.random.default_rng(1234)
    src = rng.random((1, 1) + FULL).astype(np.float32)
    trg = rng.random((1, 1) + FULL).astype(np.float32)
    _full_size_step_vs_oracle(vxm, src, trg, seed=11, flow_std=0.05)


def test_channel_blocked_interior_tensors_change_no_bit_of_the_step(vxm):
    """The fused U-Net keeps the activations that only split kernels touch channel-blocked (functional._blocked_tensors; VXM_BLOCKED=0
    turns it off).  Layout is not arithmetic: the full headline step -- moved image, field, loss and every parameter gradient -- must be
    BIT-IDENTICAL with and without it, at the size the metric is quoted on and at a size where only part of the chain qualifies."""
    from voxelmorph_amd.torch import functional as VF
    if VF.FP32_ENGINE != "f16x2":
        pytest.skip("channel-blocked tensors exist on the fp16 piece scheme only")
    keep, keep_signs = VF.BLOCKED, VF.SIGNS
    try:
        for shape, B, expect in ((FULL, 1, 3), ((64, 96, 128), 2, 1)):          # (3: rem0, rem1 and -- round 6, late -- the last activation, read by the flow conv)
            rng = np.random.default_rng(77)
            src, trg = G(rng.random((B, 1) + shape)), G(rng.random((B, 1) + shape))
            torch.manual_seed(3)
            model = vxm.networks.VxmDense(shape, int_steps=7, int_downsize=2).cuda()
            with torch.no_grad():
                model.flow.weight.normal_(0, 0.02)
            plan = model.unet_model.plan(model._feats, extra=((model.flow.out_channels, 1.0),))
            VF.BLOCKED = True
            assert len(VF._blocked_tensors(plan, B, shape)) >= expect, (shape, VF._blocked_tensors(plan, B, shape))
            results = []
            for flag, signs in ((False, True), (True, True), (True, False)):
                # (round 6: the blocked activations' LeakyReLU' is read from their SIGN tensors, functional.SIGNS -- one bit is all the product
                # takes from the activation, so that changes no bit either)
                VF.BLOCKED, VF.SIGNS = flag, signs
                for p in model.parameters():
                    p.grad = None
                moved, field = model(src, trg)
                loss = vxm.losses.NCC().loss(trg, moved) + vxm.losses.Grad("l2", loss_mult=2).loss(None, field)
                loss.backward()
                results.append([moved.detach().clone(), field.detach().clone(), loss.detach().clone()] + [p.grad.clone() for p in model.parameters()])
            for a, b, c in zip(*results):
                assert torch.equal(a, b) and torch.equal(b, c)
            del model, results, src, trg
            torch.cuda.empty_cache()
    finally:
        VF.BLOCKED, VF.SIGNS = keep, keep_signs


def test_pooling_backward_fused_into_the_first_weight_gradient_changes_no_bit(vxm):
    """Round 6: the gradient at the first ConvBlock's pre-activation -- max_pool3d backward + the skip branch + leaky_relu_backward, 0.44 GB at
    160x192x224 with ONE reader -- is formed inside that reader (vxm_conv3d_k3_fewch_bwd_weight_pool, from the 16-bit codes of
    vxm_maxpool2_fwd_code) instead of by vxm_maxpool2_bwd.  Same operations in the same order: every parameter gradient of the headline step must
    be BIT-IDENTICAL with and without the fusion (functional.POOL_FUSE), with one and two pairs, on noise and with ties / negatives / a NaN in play
    (an image of zeros makes every first-block activation of a channel equal: the arg-max is then decided by scan order alone)."""
    from voxelmorph_amd.torch import functional as VF
    if VF.FP32_ENGINE != "f16x2":
        pytest.skip("the few-channel fp16-piece weight gradient exists on the fp16 piece scheme only")
    keep = VF.POOL_FUSE
    try:
        for shape, B, kind in ((FULL, 1, "noise"), ((32, 48, 64), 2, "noise"), ((32, 48, 64), 1, "flat"), ((32, 48, 64), 1, "nan")):
            rng = np.random.default_rng(5)
            src, trg = G(rng.random((B, 1) + shape)), G(rng.random((B, 1) + shape))
            if kind == "flat":
                src[:, :, :16] = 0.0
                trg[:, :, :16] = 0.0
            if kind == "nan":
                src[0, 0, 9, 13, 21] = float("nan")
            torch.manual_seed(3)
            model = vxm.networks.VxmDense(shape, int_steps=7, int_downsize=2).cuda()
            with torch.no_grad():
                model.flow.weight.normal_(0, 0.02)
            plan = model.unet_model.plan(model._feats, extra=((model.flow.out_channels, 1.0),))
            VF.POOL_FUSE = True
            fus = [t for t in range(plan.n_tensors) if VF._pool_fusable(plan, t, shape, False, VF._blocked_tensors(plan, B, shape))]
            assert len(fus) == 1 and plan.lvl[fus[0]] == 0 and plan.ch[fus[0]] == 16, fus
            results = []
            for flag in (False, True):
                VF.POOL_FUSE = flag
                for p in model.parameters():
                    p.grad = None
                moved, field = model(src, trg)
                loss = vxm.losses.NCC().loss(trg, moved) + vxm.losses.Grad("l2", loss_mult=2).loss(None, field)
                loss.backward()
                results.append([loss.detach().clone()] + [p.grad.clone() for p in model.parameters()])
            for a, b in zip(*results):
                assert torch.equal(a, b) or (kind == "nan" and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(), b.nan_to_num()))
            if kind == "noise":
                assert all(bool(torch.isfinite(g).all()) for g in results[1])
            del model, results, src, trg
            torch.cuda.empty_cache()
    finally:
        VF.POOL_FUSE = keep


def test_full_size_train_step_batch_of_two_vs_oracle(vxm):
    """The same step with TWO pairs in the batch (scripts/torch/train.py:128-129,200-220: the per-GPU batch of BASELINE
    configs[3] is > 1): batch strides, 32-bit buffer offsets of the second sample and the batch mean of both losses at the
    size the metric is quoted on -- forward tensors, loss and all 24 parameter gradients against the oracle."""
    rng = np.random.default_rng(4321)
    src = rng.random((2, 1) + FULL).astype(np.float32)
    trg = rng.random((2, 1) + FULL).astype(np.float32)
    _full_size_step_vs_oracle(vxm, src, trg, seed=13, flow_std=0.05)


def _real_scan():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_scan_u8.npz"))
    vol = (d["vol_u8"].astype(np.float64) / 255.0).astype(np.float32)       # == test_scan.npz['vol'].astype(float32), bit for bit
    return vol, d["seg_u8"].astype(np.float32), d["labels"]


def _smooth_svf(shape, sigma=8.0, max_disp=5.0, seed=0):
    """BASELINE.md §4 structured pair: Gaussian-filtered N(0,1) noise (sigma = 8 voxels) scaled to max |v| = 5 voxels.  (The raw
    maximum of the filtered field is a boundary artefact at one corner, 18x its mean; the scale is set by the 99.9th percentile
    of |v| and the few longer vectors are shortened to 5 voxels, which leaves a field with |v| ~ 1.5 voxels on average.)"""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    f = np.stack([gaussian_filter(rng.standard_normal(shape), sigma, mode="nearest") for _ in range(3)])
    mag = np.sqrt((f ** 2).sum(0))
    f *= max_disp / np.percentile(mag, 99.9)
    mag = np.sqrt((f ** 2).sum(0))
    f *= np.minimum(1.0, max_disp / np.maximum(mag, 1e-12))
    return f[None].astype(np.float32)


def test_full_size_real_scan_step_and_label_dice_gate(vxm):
    """The structured pair of SURVEY.md §8d / BASELINE.md §4 on the reference's real scan (data/test_scan.npz, shipped as
    tests/golden/real_scan_u8.npz): target = the scan, source = the scan warped by a fixed smooth 5-voxel field.
    (1) the training step against the oracle as above; (2) the accuracy gate of the north star: the label map restricted to
    the 30 evaluated labels (data/labels.npz), nearest-warped by the network's full-resolution flow plus the fixed 5-voxel field, is BIT-EXACT
    against the C oracle on that flow, and its Dice (py/utils.py:265-287) differs by <= 1e-3 from the Dice of the label map
    warped by the ORACLE's flow (the two flows differ by fp32 rounding, so a handful of ties may flip)."""
    vol, seg, labels = _real_scan()
    assert vol.shape == FULL and len(labels) == 30
    svf = _smooth_svf(FULL)
    trg = vol[None, None]
    src = c_oracle.warp3d(trg, svf, mode="bilinear")
    model, pos = _full_size_step_vs_oracle(vxm, src, trg, seed=12, flow_std=0.05, fp64_ncc_arbiter=True)
    seg30 = np.where(np.isin(seg, labels), seg, 0.0).astype(np.float32)[None, None]
    # the freshly seeded network moves voxels by a fraction of a voxel only; the gate is run on a deformation of realistic
    # size: the network's flow on top of the fixed smooth 5-voxel field
    gate = pos + G(svf)
    moved = N(vxm.layers.SpatialTransformer(FULL, mode="nearest").cuda()(G(seg30), gate))
    ref_same_flow = c_oracle.warp3d(seg30, N(gate), mode="nearest")
    assert np.array_equal(moved, ref_same_flow), "nearest label warp differs in %d voxels" % int((moved != ref_same_flow).sum())
    assert set(np.unique(moved)) <= set(np.unique(seg30))
    with torch.no_grad():
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items() if not k.endswith(".grid")}
        _, pos_o = orc.vxm_dense_forward(torch.from_numpy(src), torch.from_numpy(trg), sd, registration=True)
    ref = c_oracle.warp3d(seg30, pos_o.numpy() + svf, mode="nearest")
    d_hip = np.asarray(orc.dice_metric(moved[0, 0], seg30[0, 0], labels=labels))
    d_ref = np.asarray(orc.dice_metric(ref[0, 0], seg30[0, 0], labels=labels))
    print("real-scan label gate: mean Dice hip=%.6f oracle=%.6f, max per-label diff %.2e, flow max|d|=%.2e, label agreement %.6f"
          % (d_hip.mean(), d_ref.mean(), np.abs(d_hip - d_ref).max(), float((pos.cpu() - pos_o).abs().max()), (moved == ref).mean()))
    assert 0.2 < d_hip.mean() < 0.99            # a real deformation: the structures moved, and still overlap
    assert d_hip.shape == (30,) and np.abs(d_hip - d_ref).max() <= 1e-3


def test_full_size_step_with_heavy_tailed_activations_on_all_three_engines(vxm):
    """The fp16-piece engine scales every staged tile by ONE power of two: inside a tile a value far below the tile's largest
    magnitude keeps an absolute, not a relative, error bound.  A synthetic conv test documents that on one tile (test_gpu_s3.py); this is the
    whole headline step on a realistic tensor with heavy tails: the real scan pair with 0.1 % of the voxels of both images multiplied by
    2^12 .. 2^20 (log-uniform) -- about one outlier per staged 8 x 8 x 16 tile, i.e. nearly every tile carries one (range_report: 48 % of
    the first layer's activations lie below 2^-18 of their tile's maximum).  Every engine (f16x2 = default, split = bf16x3, native = fp32
    MFMA) is compared with the oracle whose NCC term is evaluated in fp64.
    Measured (round 6): worst parameter gradient (flow.bias, a sum
    that cancels to 1e-4 of its terms; the reference-order fp32 oracle itself is 8.1e-3 from the arbiter) 1.3e-2 on split, 9.7e-3 on native,
    8.9e-2 on f16x2; medians over the 24 parameters 3.4e-5 / 2.4e-5 / 1.9e-4.  (Round 5 read 1.0e-1 / 1.8e-1 / 9.0e-2: rounding
    elsewhere in the step, removed since, hid the difference.)  So on THIS input the fp16 pieces cost about one digit, which is exactly what the engine guard is for.
    Gates: forward field <= 1e-4 relative on every engine; the two engines that carry fp32's exponent range inside 1.5 x the gate of every
    parameter; the fp16-piece engine within 40 x (its documented absolute-error regime, not a broken kernel) AND refused for this batch by
    the guard every GraphedStep runs on its first step (diagnostics.guard_engine moves the process to `split`)."""
    import warnings
    from voxelmorph_amd.torch import functional as VF
    from voxelmorph_amd import invalidate_packs, diagnostics
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    guard = None
    vol, _, _ = _real_scan()
    trg = vol[None, None].copy()
    src = c_oracle.warp3d(trg, _smooth_svf(FULL), mode="bilinear")
    rng = np.random.default_rng(99)
    for img in (src, trg):
        idx = rng.choice(img.size, size=img.size // 1000, replace=False)
        img.reshape(-1)[idx] *= np.exp2(rng.uniform(12.0, 20.0, size=idx.size)).astype(np.float32)
    sd = orc.seeded_state_dict(FULL, seed=21, flow_std=0.05)
    sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
    names, params = list(sdo), list(sdo.values())
    ts = torch.from_numpy(trg)
    ref, (_, reg, ys, pres) = orc.train_step_loss(torch.from_numpy(src), ts, sdo, "ncc", 1.0)
    g32 = dict(zip(names, torch.autograd.grad(ref, params, retain_graph=True)))
    ref64 = orc.ncc_loss(ts, ys, dtype=torch.float64).float() + reg
    g64 = dict(zip(names, torch.autograd.grad(ref64, params)))
    e_ref = {n: rel_l2(g32[n].numpy(), g64[n].numpy()) for n in names}
    keep = VF.FP32_ENGINE
    s, t = G(src), G(trg)
    ratio = {}                     # engine -> worst (error against the fp64-NCC arbiter) / (gate of that parameter)
    try:
        for engine in ("f16x2", "split", "native"):
            VF.FP32_ENGINE = engine
            model = vxm.networks.VxmDense(FULL, int_steps=7, int_downsize=2)
            model.load_state_dict(sd, strict=False)
            model = model.cuda()
            invalidate_packs(model)
            box = []

            def step():
                y, pre = model(s, t)
                loss = vxm.losses.NCC().loss(t, y) + vxm.losses.Grad("l2", loss_mult=2).loss(None, pre)
                loss.backward()
                box.append((y, pre, loss))
            if engine == "f16x2":                  # under the probe of the guard: same launches, plus one probe per tensor
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    guard = diagnostics.guard_engine(step)
                assert VF.FP32_ENGINE == "split"   # the guard moved the process off the fp16 pieces ...
                VF.FP32_ENGINE = engine            # ... (this leg measures them anyway; the step above ran on them)
            else:
                step()
            y, pre, loss = box[0]
            torch.cuda.synchronize()
            err_p = float((pre.detach().cpu() - pres.detach()).abs().max()) / max(float(pres.detach().abs().max()), 1e-30)
            errs = {n: rel_l2(N(p.grad), g64[n].numpy()) for n, p in model.named_parameters()}
            worst = max(errs, key=lambda n: errs[n] / max(3e-4, 2.0 * e_ref[n]))
            ratio[engine] = errs[worst] / max(3e-4, 2.0 * e_ref[worst])
            print("heavy tails, engine %-6s: loss hip=%.7f fp64-NCC oracle=%.7f | preint rel-max err %.2e | worst gradient %s: %.2e (fp32 oracle %.2e) "
                  "= %.2f x its gate | median over the 24 parameters %.2e"
                  % (engine, float(loss), float(ref64), err_p, worst, errs[worst], e_ref[worst], ratio[engine], float(np.median(list(errs.values())))))
            assert abs(float(loss) - float(ref64)) <= 1e-3 * max(1.0, abs(float(ref64)))
            assert err_p <= 1e-4
            del model, y, pre, loss
            torch.cuda.empty_cache()
    finally:
        VF.FP32_ENGINE = keep
    assert max(ratio["split"], ratio["native"]) <= 1.5, ratio
    assert ratio["f16x2"] <= 40.0, ratio                  # (a broken kernel is orders of magnitude out, not a factor)
    assert guard is not None and guard["recommended_engine"] == "split" and guard["worst"]["share_below_2^-18_of_tile_max"] > 0.1, guard["worst"]


@pytest.mark.parametrize("c0,up0,c1,cout", [(32, False, 0, 16), (16, False, 0, 32), (32, True, 16, 32), (2, False, 0, 16), (16, False, 0, 3)])
def test_full_size_conv_adjoint_identity(vxm, c0, up0, c1, cout):
    """Size-independent property at 160x192x224 (where the oracle is too slow): a bias-free, activation-free convolution
    is linear, so  <conv(x), dz> = <x, conv_bwd_data(dz)> = <w, conv_bwd_weight(x, dz)>.  One identity ties the forward,
    backward-data and backward-weight kernels of the full-resolution layers together (the 8-wave MFMA kernels, and for
    cat([upsample(x0), x1]) the collapsed-weight forward / backward-weight kernels)."""
    from voxelmorph_amd.torch import functional as VF
    D, H, W = FULL
    V = D * H * W
    torch.manual_seed(c0 + cout)
    x0 = torch.randn(1, c0, D // 2, H // 2, W // 2, device="cuda") if up0 else torch.randn(1, c0, D, H, W, device="cuda")
    x1 = torch.randn(1, c1, D, H, W, device="cuda") if c1 else None
    cin = c0 + c1
    w = torch.randn(cout, cin, 3, 3, 3, device="cuda") / (27 * cin) ** 0.5
    y = torch.empty(1, cout, D, H, W, device="cuda")
    VF.conv_forward(x0, c0, x0[0].numel(), up0, x1, c1, x1[0].numel() if c1 else 0, w, None, y, cout * V, cout, 1.0, 1, D, H, W)
    dz = y + 0.5 * torch.randn_like(y)          # correlated with y: the inner products are O(|y|^2), not a random-sign sum
    lhs = float((y.double() * dz.double()).sum())
    gw, gb = torch.empty_like(w), torch.empty(cout, device="cuda")
    VF.conv_bwd_weight(VF._Workspace(y.device), x0, c0, x0[0].numel(), up0, x1, c1, x1[0].numel() if c1 else 0, dz, cout, gw, gb, 1, D, H, W)
    via_w = float((gw.double() * w.double()).sum())
    scale = float(y.double().norm() * dz.double().norm())
    assert abs(lhs - via_w) <= 1e-5 * scale, (lhs, via_w, scale)
    np.testing.assert_allclose(N(gb), N(dz.double().sum(dim=(0, 2, 3, 4)).float()), rtol=1e-4, atol=1e-2)
    gx = torch.empty(1, cin, D, H, W, device="cuda")
    VF.conv_bwd_data(dz, cout, w, gx, cin, None, 1.0, 1, D, H, W)
    if up0:      # the gradient of the upsampled segment folds back onto the half-resolution tensor (sum over the 2x2x2 children)
        g0 = gx[:, :c0].reshape(1, c0, D // 2, 2, H // 2, 2, W // 2, 2).double().sum(dim=(3, 5, 7))
        via_x = float((g0 * x0.double()).sum()) + float((gx[:, c0:].double() * x1.double()).sum())
    else:
        via_x = float((gx.double() * x0.double()).sum())
    assert abs(lhs - via_x) <= 1e-5 * scale, (lhs, via_x, scale)


@pytest.mark.parametrize("c0,up0,c1,cout", [(32, False, 0, 16), (16, False, 0, 16), (16, False, 0, 32), (32, True, 16, 32), (2, False, 0, 16),
                                            (16, False, 0, 3)])
def test_full_size_conv_adjoint_identity_four_pairs(vxm, c0, up0, c1, cout):
    """The adjoint identity of every full-resolution conv product at the per-GPU load of BASELINE configs[3] (4 pairs per GPU,
    scripts/torch/train.py:128-129): B = 4 at 160x192x224.  Checked PER SAMPLE -- a kernel that mixed up batch strides would
    still satisfy the identity summed over the batch -- plus bit-equality of sample 0 with the B = 1 launch (forward), so the
    later samples are tied to an already-verified one through linearity."""
    from voxelmorph_amd.torch import functional as VF
    D, H, W = FULL
    V, B = D * H * W, 4
    torch.manual_seed(100 + c0 + cout)
    lo = (D // 2, H // 2, W // 2)
    x0 = torch.randn(B, c0, *(lo if up0 else FULL), device="cuda")
    x1 = torch.randn(B, c1, D, H, W, device="cuda") if c1 else None
    cin = c0 + c1
    w = torch.randn(cout, cin, 3, 3, 3, device="cuda") / (27 * cin) ** 0.5
    y = torch.empty(B, cout, D, H, W, device="cuda")
    VF.conv_forward(x0, c0, x0[0].numel(), up0, x1, c1, x1[0].numel() if c1 else 0, w, None, y, cout * V, cout, 1.0, B, D, H, W)
    y1 = torch.empty(1, cout, D, H, W, device="cuda")
    VF.conv_forward(x0[:1], c0, x0[0].numel(), up0, x1[:1] if c1 else None, c1, x1[0].numel() if c1 else 0, w, None, y1, cout * V, cout, 1.0, 1, D, H, W)
    assert torch.equal(y[:1], y1)
    del y1
    dz = y + 0.5 * torch.randn_like(y)
    lhs = (y.double() * dz.double()).sum(dim=(1, 2, 3, 4))
    scale = y.double().flatten(1).norm(dim=1) * dz.double().flatten(1).norm(dim=1)
    gx = torch.empty(B, cin, D, H, W, device="cuda")
    VF.conv_bwd_data(dz, cout, w, gx, cin, None, 1.0, B, D, H, W)
    if up0:
        g0 = gx[:, :c0].reshape(B, c0, D // 2, 2, H // 2, 2, W // 2, 2).double().sum(dim=(3, 5, 7))
        via_x = (g0 * x0.double()).sum(dim=(1, 2, 3, 4)) + (gx[:, c0:].double() * x1.double()).sum(dim=(1, 2, 3, 4))
        del g0
    else:
        via_x = (gx.double() * x0.double()).sum(dim=(1, 2, 3, 4))
    del gx
    assert bool(((lhs - via_x).abs() <= 1e-5 * scale).all()), (lhs, via_x, scale)
    # the weight gradient sums over the batch: per-sample identity through one-sample launches on views of the batch
    ws = VF._Workspace(y.device)
    gsum = torch.zeros_like(w, dtype=torch.float64)
    for b in range(B):
        gw, gb = torch.empty_like(w), torch.empty(cout, device="cuda")
        VF.conv_bwd_weight(ws, x0[b:b + 1], c0, x0[0].numel(), up0, x1[b:b + 1] if c1 else None, c1, x1[0].numel() if c1 else 0, dz[b:b + 1], cout,
                           gw, gb, 1, D, H, W)
        via_w = float((gw.double() * w.double()).sum())
        assert abs(float(lhs[b]) - via_w) <= 1e-5 * float(scale[b]), (b, float(lhs[b]), via_w)
        gsum += gw.double()
    gw, gb = torch.empty_like(w), torch.empty(cout, device="cuda")
    VF.conv_bwd_weight(ws, x0, c0, x0[0].numel(), up0, x1, c1, x1[0].numel() if c1 else 0, dz, cout, gw, gb, B, D, H, W)
    assert rel_l2(N(gw), gsum.cpu().numpy()) <= 1e-5
    np.testing.assert_allclose(N(gb), N(dz.double().sum(dim=(0, 2, 3, 4)).float()), rtol=1e-4, atol=4e-2)


def test_semisupervised_config5_shape_vs_oracle(vxm):
    """BASELINE.json configs[4] AT ITS SHAPE: VxmDenseSemiSupervisedSeg 160x192x224 with the 30 evaluated
    labels one-hot at half resolution [1, 30, 80, 96, 112], losses [NCC, Grad('l2', x2), Dice] weighted [1, 1, 0.01]
    (voxelmorph/tf/networks.py:287-388, scripts/tf/train_semisupervised_seg.py:117-140) on the structured pair built from the
    reference's real scan: forward tensors, loss and every parameter gradient against the oracle composition; then the
    evaluation protocol of scripts/tf/test.py:80-112 -- nearest warp of the full-resolution label map (bit-exact against the C
    oracle on the same flow) and py/utils.py:265-287 Dice against the oracle's."""
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    vol, seg, labels = _real_scan()
    nb = len(labels)
    assert nb == 30
    svf = _smooth_svf(FULL)
    trg = vol[None, None]
    src = c_oracle.warp3d(trg, svf, mode="bilinear")
    seg30 = np.where(np.isin(seg, labels), seg, 0.0).astype(np.float32)
    seg_moving = c_oracle.warp3d(seg30[None, None], svf, mode="nearest")[0, 0]
    half = tuple(slice(None, None, 2) for _ in range(3))                       # generators.py:161-165: seg[::2, ::2, ::2] split into one-hot labels
    onehot = lambda lab: np.stack([(lab[half] == l) for l in labels], 0).astype(np.float32)[None]
    seg_src, seg_trg = onehot(seg_moving), onehot(seg30)
    assert seg_src.shape == (1, 30, 80, 96, 112)
    sd = orc.seeded_state_dict(FULL, seed=14, flow_std=0.05)
    model = vxm.networks.VxmDenseSemiSupervisedSeg(FULL, nb, int_steps=7, int_downsize=2)
    res = model.vxm_model.load_state_dict(sd, strict=False)
    assert all(k.endswith(".grid") for k in res.missing_keys) and not res.unexpected_keys
    model = model.cuda()
    y, pre, yseg = model(G(src), G(trg), G(seg_src))
    l_dice = vxm.losses.Dice().loss(G(seg_trg), yseg)
    loss = vxm.losses.NCC().loss(G(trg), y) + vxm.losses.Grad("l2", loss_mult=2).loss(None, pre) + 0.01 * l_dice
    loss.backward()
    torch.cuda.synchronize()
    sdo = {k: v.clone().requires_grad_() for k, v in sd.items()}
    names, params = list(sdo), list(sdo.values())
    ts, tt = torch.from_numpy(src), torch.from_numpy(trg)
    yo, preo, ysego, poso = orc.vxm_semisupervised_forward(ts, tt, torch.from_numpy(seg_src), sdo)
    reg_o, dice_o = orc.grad_loss(preo, "l2", 2), orc.dice_loss(torch.from_numpy(seg_trg), ysego)
    # the image term against the fp64-NCC arbiter: the reference's fp32 NCC formula loses its digits on a real scan (see above)
    ref64 = orc.ncc_loss(tt, yo, dtype=torch.float64).float() + reg_o + 0.01 * dice_o
    g64 = dict(zip(names, torch.autograd.grad(ref64, params)))
    err_seg = float((yseg.detach().cpu() - ysego.detach()).abs().max())
    print("config-5 step: loss hip=%.7f oracle=%.7f | dice term hip=%.6f oracle=%.6f | max|d warped seg|=%.2e"
          % (float(loss), float(ref64), float(l_dice), float(dice_o), err_seg))
    assert tuple(yseg.shape) == (1, 30, 80, 96, 112)
    assert err_seg <= 1e-4 and abs(float(l_dice) - float(dice_o)) <= 1e-5 and abs(float(loss) - float(ref64)) <= 1e-3
    for name, p in model.vxm_model.named_parameters():
        e = rel_l2(N(p.grad), g64[name].numpy())
        print("  %-40s vs fp64-NCC arbiter: hip %.2e" % (name, e))
        assert e <= 3e-4, (name, e)
    # evaluation: nearest warp of the full-resolution moving label map with the predicted flow
    moved = N(model.apply_transform(G(src), G(trg), G(seg_moving[None, None]), interp_method="nearest"))
    with torch.no_grad():
        flow_hip = model.register(G(src), G(trg))
    ref_same_flow = c_oracle.warp3d(seg_moving[None, None], N(flow_hip), mode="nearest")
    assert np.array_equal(moved, ref_same_flow), "nearest label warp differs in %d voxels" % int((moved != ref_same_flow).sum())
    ref = c_oracle.warp3d(seg_moving[None, None], poso.detach().numpy(), mode="nearest")
    d_hip = np.asarray(orc.dice_metric(moved[0, 0], seg30, labels=labels))
    d_ref = np.asarray(orc.dice_metric(ref[0, 0], seg30, labels=labels))
    print("config-5 evaluation: mean Dice hip=%.6f oracle=%.6f, max per-label diff %.2e" % (d_hip.mean(), d_ref.mean(), np.abs(d_hip - d_ref).max()))
    assert d_hip.shape == (30,) and np.abs(d_hip - d_ref).max() <= 1e-3


# ------------------------------------------------------------------ 2-D (planar) variants: golden fixtures from the reference
def test_planar_layers_golden(vxm, g_planar):
    g = g_planar
    img = g["warp_src"].shape[2:]
    s, f = G(g["warp_src"], True), G(g["warp_flow"], True)
    out = vxm.layers.SpatialTransformer(img).cuda()(s, f)
    np.testing.assert_allclose(N(out), g["warp_out"], atol=1e-5, rtol=0)
    out.backward(G(g["warp_gout"]))
    np.testing.assert_allclose(N(s.grad), g["warp_gsrc"], atol=1e-5, rtol=0)
    np.testing.assert_allclose(N(f.grad), g["warp_gflow"], atol=2e-5, rtol=0)
    near = vxm.layers.SpatialTransformer(img, mode="nearest").cuda()(G(g["near_seg"]), G(g["near_flow"]))
    assert np.array_equal(N(near), g["near_out"])                     # label warp: bit-exact
    v = G(g["vecint_in"], True)
    iv = vxm.layers.VecInt(img, 5).cuda()(v)
    np.testing.assert_allclose(N(iv), g["vecint_out"], atol=1e-4, rtol=0)
    iv.backward(G(g["vecint_gout"]))
    np.testing.assert_allclose(N(v.grad), g["vecint_gin"], atol=2e-4, rtol=1e-4)
    x = G(g["resize_in"], True)
    down = vxm.layers.ResizeTransform(2, 2)(x)
    np.testing.assert_allclose(N(down), g["resize_down"], atol=2e-6, rtol=0)
    down.backward(G(g["resize_gdown"]))
    np.testing.assert_allclose(N(x.grad), g["resize_down_gin"], atol=1e-5, rtol=0)
    x2 = G(g["resize_in"], True)
    up = vxm.layers.ResizeTransform(0.5, 2)(x2)
    np.testing.assert_allclose(N(up), g["resize_up"], atol=1e-5, rtol=0)        # O(10) values after the x2 rescale: a few fp32 ulps (FMA contraction)
    up.backward(G(g["resize_gup"]))
    np.testing.assert_allclose(N(x2.grad), g["resize_up_gin"], atol=2e-5, rtol=0)


def test_planar_losses_golden(vxm, g_planar):
    g = g_planar
    for tag, win in (("ncc", None), ("ncc5", [5, 5])):
        J = G(g["J"], True)
        l = vxm.losses.NCC(win=win).loss(G(g["I"]), J)
        gate("planar %s: loss vs fp32 reference" % tag, abs(float(l) - float(g[tag])), NCC_LOSS_GATE_REF)
        ref64 = orc.ncc_loss(torch.from_numpy(g["I"]), torch.from_numpy(g["J"]), win=win, dtype=torch.float64).item()
        gate("planar %s: loss vs fp64" % tag, abs(float(l) - ref64), NCC_LOSS_GATE)
        l.backward()
        gate("planar %s: dJ vs reference (fp32)" % tag, rel_l2(N(J.grad), g[tag + "_gJ"]), NCC_GRAD_GATE_REF)
    for pen, mult in (("l1", None), ("l2", 2)):
        fl = G(g["warp_flow"], True)
        l = vxm.losses.Grad(pen, loss_mult=mult).loss(None, fl)
        np.testing.assert_allclose(float(l), float(g["grad_%s" % pen]), rtol=1e-5)
        l.backward()
        np.testing.assert_allclose(N(fl.grad), g["grad_%s_g" % pen], atol=1e-8, rtol=1e-5)


def test_planar_unet_blocks_vs_oracle(vxm):
    """MaxPool2d / Upsample+cat / depth-one MFMA conv against the oracle's ATen composition, forward and gradients."""
    torch.manual_seed(7)
    net = vxm.networks.Unet((32, 48), infeats=2).cuda()
    sd = {"unet_model." + k: v.detach().cpu().double().requires_grad_() for k, v in net.state_dict().items()}
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 2, 32, 48)).astype(np.float32)
    xg = G(x, True)
    y = net(xg)
    xo = torch.from_numpy(x).double().requires_grad_()
    yo = orc.unet_forward(xo, sd)
    assert rel_l2(N(y), yo.detach().numpy()) < 1e-5
    gy = rng.standard_normal(tuple(y.shape)).astype(np.float32)
    y.backward(G(gy))
    yo.backward(torch.from_numpy(gy).double())
    for name, p in net.named_parameters():
        assert rel_l2(N(p.grad), sd["unet_model." + name].grad.numpy()) < 1e-4, name
    assert rel_l2(N(xg.grad), xo.grad.numpy()) < 1e-4


PLANAR_CASES = {
    "diffeo": dict(int_steps=5, int_downsize=2, bidir=False, loss="ncc", lam=1.0),
    "dense": dict(int_steps=0, int_downsize=2, bidir=False, loss="mse", lam=0.01),
    "bidir": dict(int_steps=3, int_downsize=2, bidir=True, loss="mse", lam=0.01),
}


@pytest.mark.parametrize("tag", list(PLANAR_CASES))
def test_planar_vxm_dense_golden(vxm, g_planar, tag):
    g, cfg = g_planar, PLANAR_CASES[tag]
    inshape = tuple(int(v) for v in g["inshape"])
    model = vxm.networks.VxmDense(inshape, int_steps=cfg["int_steps"], int_downsize=cfg["int_downsize"], bidir=cfg["bidir"])
    res = model.load_state_dict(orc.seeded_state_dict(inshape, seed=7, flow_std=0.2), strict=False)
    assert all(k.endswith(".grid") for k in res.missing_keys) and not res.unexpected_keys
    if cfg["int_steps"] > 0:
        assert [k for k in model.state_dict().keys()] == [str(k) for k in g["state_keys"]]
    model = model.cuda()
    src, trg = G(g["source"]), G(g["target"])
    pred = model(src, trg)
    img_fn = vxm.losses.NCC().loss if cfg["loss"] == "ncc" else vxm.losses.MSE().loss
    if cfg["bidir"]:
        img = 0.5 * img_fn(trg, pred[0]) + 0.5 * img_fn(src, pred[1])
        np.testing.assert_allclose(N(pred[1]), g[tag + "_y_target"], atol=2e-5, rtol=0)
    else:
        img = img_fn(trg, pred[0])
    reg = vxm.losses.Grad("l2", loss_mult=cfg["int_downsize"]).loss(None, pred[-1])
    loss = img + cfg["lam"] * reg
    np.testing.assert_allclose(N(pred[0]), g[tag + "_y_source"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(N(pred[-1]), g[tag + "_preint"], atol=2e-5, rtol=0)
    ref = g[tag + "_loss"]
    assert abs(float(loss) - ref[0]) < 1e-3 * max(1.0, abs(ref[0]))
    loss.backward()
    params = dict(model.named_parameters())
    tol = 2e-3 if cfg["loss"] == "ncc" else 1e-4
    for n, r in zip([str(n) for n in g[tag + "_grad_names"]], g[tag + "_grad_norms"]):
        got = float(params[n].grad.double().norm())
        assert abs(got - r) <= tol * max(r, 1e-12), (n, got, r)
    for key in g.files:
        if key.startswith(tag + "_grad_") and key not in (tag + "_grad_names", tag + "_grad_norms"):
            assert rel_l2(N(params[key[len(tag + "_grad_"):]].grad), g[key]) < tol, key
    with torch.no_grad():
        _, pos = model(src, trg, registration=True)
    np.testing.assert_allclose(N(pos), g[tag + "_pos_flow"], atol=1e-4, rtol=0)


def test_planar_train_step_updates_weights_through_flat_adam(vxm, g_planar):
    """The training loop as scripts/train.py runs it (FlatAdam built first; zero_grad, backward, step) on a 2-D model: the
    per-op 2-D network hands its parameter gradients to autograd (p.grad), not to the flat bucket; FlatAdam.step must fold
    them in.  Weights after one step == Adam (train.py:161) applied to the reference's golden gradients."""
    from voxelmorph_amd.optim import FlatAdam
    g, cfg, tag = g_planar, PLANAR_CASES["dense"], "dense"
    inshape = tuple(int(v) for v in g["inshape"])
    model = vxm.networks.VxmDense(inshape, int_steps=cfg["int_steps"], int_downsize=cfg["int_downsize"])
    model.load_state_dict(orc.seeded_state_dict(inshape, seed=7, flow_std=0.2), strict=False)
    model = model.cuda()
    opt = FlatAdam(model, lr=1e-3)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    src, trg = G(g["source"]), G(g["target"])
    opt.zero_grad()
    y, pre = model(src, trg)
    loss = vxm.losses.MSE().loss(trg, y) + cfg["lam"] * vxm.losses.Grad("l2", loss_mult=2).loss(None, pre)
    loss.backward()
    opt.step()
    assert float(opt.flat_grad.abs().sum()) > 0
    for key in g.files:
        if key.startswith(tag + "_grad_") and key not in (tag + "_grad_names", tag + "_grad_norms"):
            name = key[len(tag + "_grad_"):]
            gref = torch.from_numpy(g[key])
            want, _, _ = orc.adam_step_explicit(before[name].cpu(), gref, torch.zeros_like(gref), torch.zeros_like(gref), 1, lr=1e-3)
            got = dict(model.named_parameters())[name].detach().cpu()
            assert not torch.equal(got, before[name].cpu()), name + " did not move"
            # first Adam step = -lr * sign(g) where |g| >> eps: compare the update itself
            assert rel_l2((got - before[name].cpu()).numpy(), (want - before[name].cpu()).numpy()) < 2e-3, name


def test_flat_adam_accumulates_across_backward_calls(vxm):
    """Two forward/backward passes before one step (gradient accumulation) on the fused 3-D engine: the first pass writes the
    bucket directly, the second goes through autograd's p.grad; step() sees their sum."""
    from voxelmorph_amd.optim import FlatAdam
    inshape = (16, 32, 16)
    rng = np.random.default_rng(5)
    pairs = [(G(rng.random((1, 1) + inshape)), G(rng.random((1, 1) + inshape))) for _ in range(2)]
    model = vxm.networks.VxmDense(inshape, int_steps=2)
    model.load_state_dict(orc.seeded_state_dict(inshape, seed=2, flow_std=0.1), strict=False)
    model = model.cuda()

    def grads(batch, opt=None):
        for a, b in batch:
            y, pre = model(a, b)
            (vxm.losses.MSE().loss(b, y) + 0.01 * vxm.losses.Grad("l2", loss_mult=2).loss(None, pre)).backward()

    grads(pairs[:1])
    g0 = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).clone()
    model.zero_grad(set_to_none=True)
    grads(pairs[1:])
    g1 = torch.cat([p.grad.reshape(-1) for p in model.parameters()]).clone()
    model.zero_grad(set_to_none=True)
    opt = FlatAdam(model, lr=1e-4)
    opt.zero_grad()
    grads(pairs)
    opt.load_grads_from_params()
    assert rel_l2(N(opt.flat_grad), N(g0 + g1)) < 1e-6
    # an optimiser step between a forward and its backward is an error, not silently wrong gradients
    opt.zero_grad()
    y, pre = model(*pairs[0])
    opt.step()
    with pytest.raises(RuntimeError, match="modified in place"):
        vxm.losses.MSE().loss(pairs[0][1], y).backward()


def test_atlas_and_semisupervised_loaders(vxm, tmp_path):
    """generators.py:110-143 / :146-194 tuple contracts on the device loaders (resident and streaming)."""
    from voxelmorph_amd import data as vdata
    rng = np.random.default_rng(2)
    shape = (8, 12, 16)
    vols = [rng.random(shape) for _ in range(4)]
    segs = [rng.integers(0, 6, size=shape).astype(np.float64) for _ in range(4)]
    atlas = rng.random(shape)
    refv = np.stack(vols).astype(np.float32)
    for resident_bytes in (1 << 30, 0):
        ld = vdata.scan_to_atlas(vols, atlas[None, ..., None], batch_size=2, bidir=True, device="cuda", resident_bytes=resident_bytes)
        (scan, atl), (o0, o1, z) = next(ld)
        assert scan.shape == (2, 1) + shape and atl.shape == scan.shape and o0 is atl and o1 is scan
        assert np.array_equal(N(atl)[1, 0], atlas.astype(np.float32)) and z.shape == (2, 3) + shape and float(z.abs().max()) == 0
        assert all(any(np.array_equal(N(scan)[b, 0], refv[i]) for i in range(4)) for b in range(2))
        ld = vdata.scan_to_atlas(vols, atlas, batch_size=2, segs=segs, no_warp=True, device="cuda", resident_bytes=resident_bytes)
        (scan, atl), (seg,) = next(ld)
        for b in range(2):          # the segmentation handed out belongs to the scan drawn
            i = [k for k in range(4) if np.array_equal(N(scan)[b, 0], refv[k])][0]
            assert np.array_equal(N(seg)[b, 0], segs[i].astype(np.float32))
        labels = np.array([1, 3, 5])
        ld = vdata.semisupervised(vols, segs, labels, device="cuda", resident_bytes=resident_bytes)
        (sv, tv, ss), (tv2, z, ts) = next(ld)
        assert sv.shape == (1, 1) + shape and ss.shape == (1, 3, 4, 6, 8) and ts.shape == ss.shape and tv2 is tv
        i = [k for k in range(4) if np.array_equal(N(sv)[0, 0], refv[k])][0]
        want = np.stack([(segs[i] == lab) for lab in labels])[:, ::2, ::2, ::2].astype(np.float32)      # split_seg, :161-165
        assert np.array_equal(N(ss)[0], want)
    np.savez(tmp_path / "atlas.npz", vol=atlas, seg=segs[0])
    ld = vdata.semisupervised(vols, segs, labels, atlas_file=str(tmp_path / "atlas.npz"), device="cuda")
    (sv, tv, ss), (tv2, z, ts) = next(ld)
    assert np.array_equal(N(tv)[0, 0], atlas.astype(np.float32))
    assert np.array_equal(N(ts)[0], np.stack([(segs[0] == lab) for lab in labels])[:, ::2, ::2, ::2].astype(np.float32))
    mc = [rng.random(shape + (2,)) for _ in range(3)]                       # multichannel volumes [*vol, C] (train.py:101)
    (a, b), _ = next(vdata.scan_to_scan(mc, batch_size=2, add_feat_axis=False, device="cuda"))
    assert a.shape == (2, 2) + shape and any(np.array_equal(N(a)[0], np.moveaxis(m, -1, 0).astype(np.float32)) for m in mc)


def test_device_loaders_against_reference_generator_fixture(vxm, tmp_path):
    """The device loaders against what the UNMODIFIED reference generators yield on the same inputs
    (tests/golden/generators.npz, written by tests/golden/make_generators_golden.py from voxelmorph/generators.py:71-194; pinned to
    the live reference by tests/test_cpu_contracts.py): same tuple structure, and every tensor equals the reference array after the
    one documented transform -- `[B, *vol, C]` float64 -> `[B, C, *vol]` float32 (scripts/torch/train.py:199-201 does the same
    cast + permute on the device every step)."""
    from voxelmorph_amd import data as vdata
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generators.npz"))
    vol, seg, atlas_vol, atlas_seg, labels = g["vol"], g["seg"], g["atlas_vol"], g["atlas_seg"], g["labels"]
    np.savez(tmp_path / "atlas.npz", vol=atlas_vol, seg=atlas_seg)
    atlas = atlas_vol[np.newaxis, ..., np.newaxis]
    runs = {
        "s2s": vdata.scan_to_scan([vol], batch_size=2, device="cuda"),
        "s2s_bidir": vdata.scan_to_scan([vol], bidir=True, batch_size=1, device="cuda"),
        "s2s_nowarp": vdata.scan_to_scan([vol], no_warp=True, batch_size=1, device="cuda"),
        "s2a": vdata.scan_to_atlas([vol], atlas, batch_size=2, device="cuda"),
        "s2a_bidir": vdata.scan_to_atlas([vol], atlas, bidir=True, batch_size=1, device="cuda"),
        "s2a_segs": vdata.scan_to_atlas([vol], atlas, batch_size=1, segs=[seg], device="cuda"),
        "semi": vdata.semisupervised([vol], [seg], list(labels), device="cuda"),
        "semi_atlas": vdata.semisupervised([vol], [seg], list(labels), atlas_file=str(tmp_path / "atlas.npz"), device="cuda"),
    }
    for tag, loader in runs.items():
        invols, outvols = next(loader)
        assert [len(invols), len(outvols)] == list(g[tag + "_n"]), tag
        for kind, got in (("in", invols), ("out", outvols)):
            for i, t in enumerate(got):
                want = np.moveaxis(g["%s_%s%d" % (tag, kind, i)], -1, 1).astype(np.float32)
                assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous(), (tag, kind, i)
                assert tuple(t.shape) == want.shape and np.array_equal(N(t), want), (tag, kind, i)


def test_train_cli_atlas_multichannel_and_semisupervised(vxm, tmp_path):
    """scripts/train.py --atlas / --multichannel / --gpu / --cudnn-nondet (scripts/torch/train.py:56,59,63,72) and
    scripts/train_semisupervised_seg.py (flags of scripts/tf/train_semisupervised_seg.py:41-79): a 2-epoch run each."""
    import subprocess
    import sys
    rng = np.random.default_rng(4)
    base = rng.random((32, 32, 32)).astype(np.float32)
    names, stems = [], []
    for i in range(3):
        v = np.roll(base, shift=i, axis=1)
        lab = (np.roll(base, shift=i, axis=1) * 4).astype(np.int32).astype(np.float32)
        np.savez(tmp_path / ("s%d_img.npz" % i), vol=v)
        np.savez(tmp_path / ("s%d_seg.npz" % i), vol=lab)
        np.savez(tmp_path / ("m%d.npz" % i), vol=np.stack([v, 1 - v], -1))
        names.append(str(tmp_path / ("s%d_img.npz" % i)))
        stems.append(str(tmp_path / ("s%d" % i)))
    np.savez(tmp_path / "atlas.npz", vol=base, seg=(base * 4).astype(np.int32).astype(np.float32))
    np.save(tmp_path / "labels.npy", np.array([1, 2, 3]))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    (tmp_path / "mlist.txt").write_text("\n".join(str(tmp_path / ("m%d.npz" % i)) for i in range(3)) + "\n")
    (tmp_path / "stems.txt").write_text("\n".join(stems) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(script, *argv):
        r = subprocess.run([sys.executable, os.path.join(root, "scripts", script)] + list(argv) + ["--epochs", "2", "--steps-per-epoch", "3"],
                           capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        losses = [float(ln.split("loss:")[1].split()[0]) for ln in r.stdout.splitlines() if "loss:" in ln]
        assert len(losses) == 2 and all(np.isfinite(losses))
        return r

    run("train.py", "--img-list", str(tmp_path / "list.txt"), "--atlas", str(tmp_path / "atlas.npz"), "--model-dir", str(tmp_path / "ma"),
        "--gpu", "0", "--cudnn-nondet", "--bidir", "--image-loss", "ncc", "--lambda", "1")
    ck = torch.load(tmp_path / "ma" / "0002.pt", map_location="cpu")
    assert ck["config"]["bidir"] is True
    run("train.py", "--img-list", str(tmp_path / "mlist.txt"), "--multichannel", "--model-dir", str(tmp_path / "mm"))
    ck = torch.load(tmp_path / "mm" / "0002.pt", map_location="cpu")
    assert ck["config"]["src_feats"] == 2 and ck["model_state"]["unet_model.encoder.0.0.main.weight"].shape[1] == 4
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "register.py"), "--moving", str(tmp_path / "m0.npz"), "--fixed",
                        str(tmp_path / "m1.npz"), "--moved", str(tmp_path / "mmoved.npz"), "--model", str(tmp_path / "mm" / "0002.pt"),
                        "--multichannel", "-g", "0"], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert np.load(tmp_path / "mmoved.npz")["vol"].shape == (32, 32, 32, 2)            # register.py:69-72: [*vol, C] in and out
    for extra in ([], ["--atlas", str(tmp_path / "atlas.npz")]):
        run("train_semisupervised_seg.py", "--img-list", str(tmp_path / "stems.txt"), "--img-suffix", "_img.npz", "--seg-suffix", "_seg.npz",
            "--labels", str(tmp_path / "labels.npy"), "--model-dir", str(tmp_path / "ms"), "--image-loss", "ncc", *extra)
    ck = torch.load(tmp_path / "ms" / "0002.pt", map_location="cpu")
    assert ck["config"]["nb_labels"] == 3 and (tmp_path / "ms" / "0000.pt").exists()


def test_inference_mode_and_flat_adam_zero_grad_contract(vxm):
    """(1) torch.inference_mode(): inference tensors carry no version counter -- the fused engines must not read one (fp32 and
    bf16 engine, parameters created inside inference_mode included).  (2) FlatAdam.step() without FlatAdam.zero_grad() since the
    previous step raises instead of adding new gradients onto the old, already reduced ones."""
    from voxelmorph_amd.optim import FlatAdam
    inshape = (16, 16, 16)
    src, trg = torch.rand(1, 1, *inshape, device="cuda"), torch.rand(1, 1, *inshape, device="cuda")
    model = vxm.networks.VxmDense(inshape, int_steps=2).cuda()
    with torch.no_grad():
        want, _ = model(src, trg, registration=True)
    with torch.inference_mode():
        got, _ = model(src, trg, registration=True)
        m2 = vxm.networks.VxmDense(inshape, int_steps=2).cuda()            # parameters that are inference tensors themselves
        m2(src, trg, registration=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            m2(src, trg, registration=True)
    assert torch.equal(got, want)
    opt = FlatAdam(model, lr=1e-4)
    for it in range(2):
        opt.zero_grad()
        y, pre = model(src, trg)
        (vxm.losses.MSE().loss(trg, y) + 0.01 * vxm.losses.Grad("l2", loss_mult=2).loss(None, pre)).backward()
        opt.step()
    y, pre = model(src, trg)
    vxm.losses.MSE().loss(trg, y).backward()
    with pytest.raises(RuntimeError, match="zero_grad"):
        opt.step()


def test_native_comm_world_one(vxm):
    """libvxm_comm.so on the device: a one-rank RCCL communicator (all a 1-GPU box can host) runs the all-reduce and the
    broadcast in place on the current stream and leaves the bucket unchanged; FlatAdam takes it as its exchange."""
    from voxelmorph_amd.comm import NativeComm
    from voxelmorph_amd.optim import FlatAdam
    c = NativeComm(0, 1, NativeComm.new_unique_id())
    try:
        t = torch.arange(327331, dtype=torch.float32, device="cuda")
        ref = t.clone()
        c.all_reduce_sum(t)
        c.broadcast(t, 0)
        torch.cuda.synchronize()
        assert torch.equal(t, ref)
        model = vxm.networks.VxmDense((16, 16, 16), int_steps=1).cuda()
        opt = FlatAdam(model, lr=1e-4, comm=c)
        assert opt.world == 1
        opt.broadcast_params(0)
        opt.flat_grad.fill_(1.0)
        before = opt.flat_param.clone()
        opt.step()
        torch.cuda.synchronize()
        assert float((before - opt.flat_param).abs().max()) > 0
        with pytest.raises(Exception):
            c.all_reduce_sum(torch.zeros(4))
    finally:
        c.destroy()


_COMM_WORKER = r"""
import os, sys
sys.path.insert(0, %(root)r)
import torch, torch.distributed as dist
from voxelmorph_amd.comm import NativeComm
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)                                   # both ranks on the one GPU of this box
dist.init_process_group("gloo", rank=rank, world_size=world)   # rendezvous only: carries the 128-byte unique id
comm = NativeComm.try_from_torch_dist()
if comm is None:
    print("rank", rank, "native communicator refused (two ranks on one device): fell back together")
else:
    t = torch.full((327331,), float(rank + 1), device="cuda")
    comm.all_reduce_sum(t)
    torch.cuda.synchronize()
    assert float(t.min()) == float(t.max()) == 3.0
    b = torch.full((16,), float(rank), device="cuda")
    comm.broadcast(b, 1)
    torch.cuda.synchronize()
    assert float(b.max()) == 1.0
    comm.destroy()
    print("rank", rank, "native all-reduce over", world, "ranks ok")
dist.barrier()
"""


def test_native_comm_two_ranks_agree(vxm, tmp_path):
    """libvxm_comm.so beyond one rank, as far as a 1-GPU box allows: two processes create the communicator through
    `NativeComm.try_from_torch_dist` (what `dist.native_comm()` uses for every multi-rank job).  Either RCCL accepts two ranks
    on one device and the SUM all-reduce / broadcast of the 1.31 MB bucket are checked, or it refuses and BOTH ranks drop the
    communicator together (the job would continue on torch.distributed) -- never a hang, never a split decision."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(tmp_path, "comm_worker.py")
    with open(script, "w") as f:
        f.write(_COMM_WORKER % dict(root=root))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29553", script], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    ok, refused = out.stdout.count("ranks ok"), out.stdout.count("fell back together")
    print(out.stdout.strip().splitlines()[-2:])
    assert (ok, refused) in ((2, 0), (0, 2)), out.stdout[-2000:]


# ------------------------------------------------------------------ the route table against the launches of a step
# entry point -> kernel family, as functional.conv_fwd_route / conv_bwd_low_route / conv_bwd_weight_route name them
_FWD_FAMILY = {"vxm_conv3d_k3_fewout_fwd": "fewout", "vxm_conv3d_k3_fewout_fwd_layout": "fewout", "vxm_conv3d_k3_s3u_fwd": "s3u",
               "vxm_conv3d_k3_s3u_fwd_signs": "s3u", "vxm_conv3d_k3_s3_fwd": "s3", "vxm_conv3d_k3_up_fwd": "up", "vxm_conv3d_k3_fwd": "fp32",
               "vxm_conv3d_k3_fwd_layout": "fp32"}
_BWD_FAMILY = dict(_FWD_FAMILY, **{"vxm_conv3d_k3_s3u_bwd_data": "s3u_pc", "vxm_conv3d_k3_s3u_bwd_low": "s3u_dlow", "vxm_conv3d_k3_up_bwd_low": "dlow",
                                   "vxm_conv3d_k3_s3_bwd_weight": "w:s3", "vxm_conv3d_k3_s3u_bwd_weight": "w:s3u", "vxm_conv3d_k3_fewch_bwd_weight": "w:fewch",
                                   "vxm_conv3d_k3_fewch_bwd_weight_pool": "w:fewch", "vxm_conv3d_k3_bwd_weight_up_segment": "w:up",
                                   "vxm_conv3d_k3_bwd_weight": "w:fp32"})
_BWW_LAUNCHES = {"s3": ["w:s3"], "s3u+s3": ["w:s3u", "w:s3"], "fewch": ["w:fewch"], "up+s3": ["w:up", "w:s3"], "fp32": ["w:fp32"]}
# `*pack_weights*` calls of one step outside _prepack_plan at 32x32x32, B = 1, on the code before the route table existed (its launch trace,
# profiles/pr07_launch_trace.txt: the pack launches of step 2 on the main stream), by (thresholds forced to one tile, VXM_S3U)
_ON_DEMAND_PACKS_BEFORE = {(True, True): 1, (True, False): 2, (False, True): 9}


def test_route_table_names_the_launches_of_a_step(vxm):
    """functional._route_plan against what a training step of VxmDense (32x32x32, B = 1) really launches, in the environment the test runs in.
    (a) For every conv op the entry points called in the forward, the backward-data (onto the low-resolution producer, and per channel range)
    and the weight gradient are the ones the table names, in launch order.  (b) With every parameter's version bumped, the packed operators
    built OUTSIDE _prepack_plan -- on demand, on the main stream, in the middle of the chain -- are exactly the ones the table marks so, and
    no more than before the table existed.  (Round 5 found such a pack with a profiler: 0.23 ms per step.)"""
    import importlib.util
    from voxelmorph_amd.torch import functional as VF
    spec = importlib.util.spec_from_file_location("launch_trace", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "launch_trace.py"))
    lt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lt)
    shape = (32, 32, 32)
    torch.manual_seed(0)
    model = vxm.networks.VxmDense(shape, int_steps=7, int_downsize=2).cuda()
    src, trg = torch.rand((1, 1) + shape, device="cuda"), torch.rand((1, 1) + shape, device="cuda")
    inside, prepack = [], VF._prepack_plan

    def marked_prepack(*a, **k):
        begin = len(rec.calls)
        try:
            return prepack(*a, **k)
        finally:
            inside.extend(range(begin, len(rec.calls)))

    def step():
        y, pre = model(src, trg)
        mid = len(rec.calls)
        (vxm.losses.NCC().loss(trg, y) + 0.01 * vxm.losses.Grad("l2", loss_mult=2).loss(None, pre)).backward()
        torch.cuda.synchronize()
        return mid

    VF._prepack_plan = marked_prepack
    try:
        with lt.Recorder(VF) as rec:
            step()
            with torch.no_grad():
                for p in model.parameters():
                    p.add_(0)
            model.zero_grad()
            begin = len(rec.calls)
            mid = step()
    finally:
        VF._prepack_plan = prepack
    plan = model.unet_model.plan(model._feats, extra=((model.flow.out_channels, 1.0),))
    table = VF._route_plan(plan, 1, shape)
    convs = list(table.convs.values())
    names = [name for name, _ in rec.calls]
    # (a) forward: one launch per conv op, in op order
    got = [_FWD_FAMILY[n] for n in names[begin:mid] if n in _FWD_FAMILY]
    print("[route] forward  ", got)
    assert got == [rt.fwd for rt in convs]
    # ... backward: per conv op from the last to the first, the weight gradient's launches, then (unless it feeds the network inputs, which ask
    # for no gradient) the low-resolution product and one launch per channel range
    want = []
    for rt in reversed(convs):
        want += _BWW_LAUNCHES[rt.bww]
        if not rt.feeds_inputs:
            want += ([rt.low] if rt.low is not None else []) + ["s3" if split else "fp32" for _, _, split in rt.bwd]
    got = [_BWD_FAMILY[n] for n in names[mid:] if n in _BWD_FAMILY]
    print("[route] backward ", got)
    assert got == want
    # (b) packs on demand
    got = sorted((n, a[2:7] if n.endswith("_range") else a[2:5]) for i, (n, a) in enumerate(rec.calls) if i >= begin and "pack_weights" in n and i not in inside)
    want = sorted(("vxm_conv3d_k3_pack_weights_range", (rt.cin, rt.cout, args[1], args[2] - args[1], int(args[0]))) if kind == "fp32" else
                  ("vxm_conv3d_k3_up_pack_weights", (rt.c0, rt.c1, rt.cout))
                  for rt in convs for grp, kind, args, _ in rt.packs(True, False) if grp is None)
    print("[route] on demand", got)
    assert got == want
    assert len(got) <= _ON_DEMAND_PACKS_BEFORE[(bool(os.environ.get("VXM_S3_MIN_TILES")), VF.S3U)]


def test_route_table_on_every_split_family_in_subprocess():
    """the check above with the tile thresholds of the split kernels forced to one, where a 32x32x32 volume reaches every split family (the
    [32, 16] adjoint pair of the 48-channel layer included), and with VXM_S3U=0: the gather-through-upsampling forward and the adjoint of the
    whole concat"""
    if os.environ.get("VXM_S3_MIN_TILES"):
        pytest.skip("already inside the forced run")
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for env in ({"VXM_S3_MIN_TILES": "1", "VXM_S3U_MIN_TILES": "1", "VXM_S3U_BWW_MIN_TILES": "1"}, {"VXM_S3_MIN_TILES": "1", "VXM_S3U": "0"}):
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.join(root, "tests", "test_gpu_parity.py"), "-k",
                            "route_table_names_the_launches"], env=dict(os.environ, **env), cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
