"""The spatial-transformer kernels (k_warp3d_fwd / bwd, the fused k_warp3d_up_fwd / bwd, k_warp2d_fwd / bwd and the VecInt forward steps) against
the float64 arbiter that resolves `floor` where the reference does (oracle.warp_arbiter / vecint_arbiter), on the table of tests/warp_cases.py:
samples on lattice points, on the last plane, in the half-covered rim, far outside, at NaN / Inf displacements.  Run on the MI355X box:
`pytest -m gpu tests/test_gpu_warp.py -s` prints the margin of every gate.

The gates are 4 x the REFERENCE's own fp32 error against the same arbiter on the same inputs (tools/warp_gates.py, output committed as
profiles/pr04_warp_gates_cpu.txt): the kernels form (wz wy) wx and sum 8 products in fp32, the same class of arithmetic as ATen."""
import numpy as np
import pytest
import torch

from oracle import vxm_oracle as orc

import resize_cases as rc
import warp_cases as wc

pytestmark = pytest.mark.gpu

# tools/warp_gates.py: forward, gsrc, gflow rel-L2 and the adjoint gap |<out, g> - <src, gsrc>| / (|out| |g|)
WARP_GATES = {3: (2.76e-7, 3.29e-7, 4.91e-7, 3.33e-9), 2: (2.12e-7, 2.31e-7, 2.42e-7, 2.18e-8)}
VECINT_GATES = {3: (1.52e-7, 6.15e-7), 2: (1.43e-7, 3.46e-7)}          # forward (the worst single step), backward
RESIZE_FWD_GATE, RESIZE_BWD_GATE = 1.179e-5, 1.153e-5                  # tools/resize_gates.py (as in test_gpu_parity.py)
SENTINEL = 12345.678


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


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def gate(what, measured, bound):
    """Assert measured < bound and print the margin (`pytest -s` / the committed GPU log shows how tight the gate is)."""
    print("[gate] %-66s measured %.3e  bound %.1e" % (what, measured, bound))
    assert measured < bound, "%s: %.3e >= %.1e" % (what, measured, bound)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def bad(a):
    return ~np.isfinite(a)


def same_set(what, got, want):
    assert np.array_equal(bad(got), bad(want)), "%s: non-finite voxels %s, the reference's %s" % (
        what, np.argwhere(bad(got))[:12].tolist(), np.argwhere(bad(want))[:12].tolist())


_ARBITER = {}


def _arbiter(key, src, flow, gout):
    """float64 arbiter of one row, computed once per process and left unchanged"""
    if key not in _ARBITER:
        _ARBITER[key] = orc.warp_arbiter(src, flow, gout)
    return _ARBITER[key]


def _reference(src, flow, gout):
    """the reference in its own dtype: ATen's forward and autograd"""
    s, f = T(src).requires_grad_(), T(flow).requires_grad_()
    out = orc.spatial_transformer(s, f)
    out.backward(T(gout))
    return out.detach().numpy(), s.grad.numpy(), f.grad.numpy()


def _layer_run(vxm, dims, src, flow, gout):
    s, f = G(src, True), G(flow, True)
    out = vxm.layers.SpatialTransformer(dims).cuda()(s, f)
    out.backward(G(gout))
    torch.cuda.synchronize()
    return N(out), N(s.grad), N(f.grad)


@pytest.mark.parametrize("case", wc.CASES, ids=wc.IDS)
def test_warp_every_case_vs_fp64(vxm, case):
    """layers.SpatialTransformer (3-D: k_warp3d_fwd / k_warp3d_bwd, 2-D: k_warp2d_fwd / k_warp2d_bwd) on every row of the table: out, src.grad
    and flow.grad against the arbiter under the reference's gates, the adjoint identity of the pair (the warp is linear in src), and out /
    flow.grad bit-identical between two runs (neither has atomics).  The `far` row (|flow| of 1e4 .. 3e38, +-Inf, NaN): the run completes,
    huge and infinite displacements sample 0, the non-finite SETS of out, gsrc and gflow are the fp32 reference's, the finite values are
    under the same gates."""
    name, dims, B, C, recipe, _ = case
    nd = len(dims)
    src, flow, gout = wc.arrays(case)
    o64, gs64, gf64 = _arbiter(name, src, flow, gout)
    out, gs, gf = _layer_run(vxm, dims, src, flow, gout)
    out2, _, gf2 = _layer_run(vxm, dims, src, flow, gout)
    assert same_bits(out, out2), name + ": two forward runs differ"
    assert same_bits(gf, gf2), name + ": two flow-gradient runs differ"
    mo = mgs = mgf = slice(None)
    if recipe == "far":
        ro, rgs, rgf = _reference(src, flow, gout)
        same_set(name + " out", out, ro)
        same_set(name + " gsrc", gs, rgs)
        same_set(name + " gflow", gf, rgf)
        with np.errstate(invalid="ignore"):
            wild = np.any(np.abs(flow) >= 1e4, axis=1, keepdims=True)               # finite huge and +-Inf (NaN compares false)
        assert wild.sum() >= 6 * nd and np.all(out[np.broadcast_to(wild, out.shape)] == 0)
        mo, mgs, mgf = ~bad(ro), ~bad(rgs), ~bad(rgf)
    else:
        assert not (bad(out).any() or bad(gs).any() or bad(gf).any())
    fwd, bsrc, bflow, adj = WARP_GATES[nd]
    gate("warp %s forward vs fp64" % name, rel_l2(out[mo], o64[mo]), fwd)
    gate("warp %s gsrc vs fp64" % name, rel_l2(gs[mgs], gs64[mgs]), bsrc)
    gate("warp %s gflow vs fp64" % name, rel_l2(gf[mgf], gf64[mgf]), bflow)
    if recipe != "far" or not (bad(out).any() or bad(gs).any()):
        gate("warp %s adjoint <out,g> - <src,gsrc>" % name, rc.adjoint_gap(out, gout, src, gs), adj)


def _guarded(shape, values=None, pad=512):
    """a device tensor of `shape` inside a buffer with `pad` sentinel floats on either side; the tensor itself starts as sentinels too"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.float32, device="cuda")
    view = buf[pad:pad + n].view(*shape)
    if values is not None:
        view.copy_(G(values))
    return buf, view


def _guards_untouched(buf, pad=512):
    return bool((buf[:pad] == SENTINEL).all()) and bool((buf[-pad:] == SENTINEL).all())


@pytest.mark.parametrize("name", ["rim_5x6x40", "rim_13x37"])
def test_warp_gradient_subsets_through_the_abi(vxm, name):
    """vxm_warp3d_bwd / vxm_warp2d_bwd with only gsrc, only gflow, and both: gflow bit-equal to the both-case, gsrc (atomics) under its gate, a
    missing output leaves its buffer untouched, the inputs keep their bits (the gflow == NULL path of the 3-D kernel stores through a
    zero-length descriptor over `flow`) and the sentinel bands around all five buffers are intact."""
    from voxelmorph_amd._lib import call, ptr, stream
    case = wc.CASES[wc.IDS.index(name)]
    _, dims, B, C, _, _ = case
    nd = len(dims)
    src, flow, gout = wc.arrays(case)
    _, gs64, gf64 = _arbiter(name, src, flow, gout)
    fn = "vxm_warp3d_bwd" if nd == 3 else "vxm_warp2d_bwd"
    bs, s = _guarded(src.shape, src)
    bf, f = _guarded(flow.shape, flow)
    bg, g = _guarded(gout.shape, gout)
    results = {}
    for want_src, want_flow in ((True, True), (True, False), (False, True)):
        bgs, gs = _guarded(src.shape)
        bgf, gf = _guarded(flow.shape)
        call(fn, ptr(s), ptr(f), ptr(g), ptr(gs) if want_src else None, ptr(gf) if want_flow else None, B, C, *dims, 0, stream())
        torch.cuda.synchronize()
        tag = "%s gsrc=%d gflow=%d" % (fn, want_src, want_flow)
        for b in (bs, bf, bg, bgs, bgf):
            assert _guards_untouched(b), tag + ": a sentinel band was written"
        assert same_bits(N(s), src) and same_bits(N(f), flow) and same_bits(N(g), gout), tag + ": an input changed"
        if not want_src:
            assert bool((gs == SENTINEL).all()), tag + ": gsrc written"
        if not want_flow:
            assert bool((gf == SENTINEL).all()), tag + ": gflow written"
        results[(want_src, want_flow)] = (N(gs), N(gf))
    both = results[(True, True)]
    assert same_bits(results[(False, True)][1], both[1]), fn + ": gflow alone differs from gflow with gsrc"
    gate("%s %s gflow (both) vs fp64" % (fn, name), rel_l2(both[1], gf64), WARP_GATES[nd][2])
    gate("%s %s gsrc (both) vs fp64" % (fn, name), rel_l2(both[0], gs64), WARP_GATES[nd][1])
    gate("%s %s gsrc (alone) vs fp64" % (fn, name), rel_l2(results[(True, False)][0], gs64), WARP_GATES[nd][1])


def _fullsize(fl, full, dtype=torch.float32):
    """ResizeTransform(1 / 2) of the reference (layers.py:91-94: x2, then F.interpolate(align_corners=True)) onto the image's extents; for
    extents that are twice the field's this IS oracle.resize_transform(x, 0.5) (asserted in test_cpu_host.py)"""
    x = fl if torch.is_tensor(fl) else T(fl)
    return torch.nn.functional.interpolate(2.0 * x.to(dtype), size=full, mode="trilinear", align_corners=True)


def _fused_forward(src, flo, full, low, mode):
    from voxelmorph_amd._lib import call, ptr, stream
    B, C = src.shape[:2]
    out = torch.empty_like(src)
    pos = torch.empty((B, 3) + tuple(full), dtype=torch.float32, device="cuda")
    call("vxm_warp3d_up_fwd", ptr(src), ptr(flo), ptr(out), ptr(pos), B, C, *full, *low, 2.0, mode, stream())
    torch.cuda.synchronize()
    return N(out), N(pos)


@pytest.mark.parametrize("row", wc.FUSED, ids=wc.FUSED_IDS)
def test_fused_warp_vs_fp64(vxm, row):
    """vxm_warp3d_up_fwd / vxm_warp3d_up_bwd (k_warp3d_up_fwd / bwd) on the fused rows.  The full-resolution field the kernel reports (pos_flow)
    is checked once against the reference's fp32 resize, and is the arbiter's input, so the warp part is judged on its own: the moved image
    and the full-resolution gradient gpos (left in `work`) under the warp gates; gflow_lo against the float64 adjoint of the reference's
    resize applied to the arbiter's gflow, at the resize-backward gate; mode 'nearest' bit-exact against the reference on the kernel's field."""
    from voxelmorph_amd._lib import call, ptr, stream
    name, low, full, _ = row
    img, fl, gout = wc.fused_arrays(row)
    B, C = img.shape[:2]
    src, flo = G(img), G(fl)
    out, pos = _fused_forward(src, flo, full, low, 0)
    gate("fused %s pos_flow vs the reference's fp32 resize" % name, rel_l2(pos, _fullsize(fl, full).numpy()), RESIZE_FWD_GATE)
    o64, _, gf64 = _arbiter(name, img, pos, gout)
    fwd, _, bflow, _ = WARP_GATES[3]
    gate("fused %s forward vs fp64" % name, rel_l2(out, o64), fwd)
    work = torch.full((B, 3) + tuple(full), SENTINEL, dtype=torch.float32, device="cuda")
    gflow_lo = torch.full_like(flo, SENTINEL)
    call("vxm_warp3d_up_bwd", ptr(src), ptr(flo), ptr(G(gout)), ptr(gflow_lo), ptr(work), work.numel() * 4, B, C, *full, *low, 2.0, 0, stream())
    torch.cuda.synchronize()
    gate("fused %s gpos (work) vs fp64" % name, rel_l2(N(work), gf64), bflow)
    x = torch.zeros((B, 3) + tuple(low), dtype=torch.float64, requires_grad=True)
    _fullsize(x, full, torch.float64).backward(T(gf64))
    gate("fused %s gflow_lo vs the fp64 adjoint of the resize" % name, rel_l2(N(gflow_lo), x.grad.numpy()), RESIZE_BWD_GATE)
    out_n, pos_n = _fused_forward(src, flo, full, low, 1)
    assert same_bits(pos_n, pos)
    assert np.array_equal(out_n, orc.spatial_transformer(T(img), T(pos_n), mode="nearest").numpy()), name + ": nearest is not bit-exact"


@pytest.mark.parametrize("nsteps", wc.VECINT_STEPS)
@pytest.mark.parametrize("dims", [d for d, _ in wc.VECINT], ids=["x".join(map(str, d)) for d, _ in wc.VECINT])
def test_vecint_forward_and_backward_vs_fp64(vxm, dims, nsteps):
    """VecInt, 3-D and 2-D, nsteps 1 and 3, on a field whose first step has 10 - 40 % of its samples at the rim, under 4 x the reference's own
    fp32 error against oracle.vecint_arbiter (tools/warp_gates.py).  The arbiter evaluates every step in float64 ON THE fp32 FIELD THE STEP
    SAMPLED: for the reference that is the reference's field, for the kernels the field they report themselves (vxm_vecint_fwd returns every
    step), exactly as the fused warp is judged on the pos_flow it reports.  So: every step's output against the arbiter's evaluation of that
    step at the forward gate; layers.VecInt returns the last step bit for bit; its gradient against the arbiter's float64 chain rule over the
    same fields at the backward gate.  The whole chain against the arbiter on the REFERENCE's fields is printed, not gated: on these white-noise
    fields the last bits of v_k move the samples of step k + 1 by more than that step's rounding -- 3.8e-7 for (6,9,40) at nsteps 3, where an
    independent plain-C fp32 evaluation of the same chain (c_oracle.vecint3d) is 3.9e-7 off and the reference, whose fields the
    arbiter shares, 3.7e-8; at nsteps 1 the two arbiters are the same."""
    from voxelmorph_amd._lib import call, ptr, stream
    vec, gout = wc.vecint_arrays(dims, nsteps)
    nd = len(dims)
    v = G(vec, True)
    steps = torch.full((nsteps,) + vec.shape, SENTINEL, dtype=torch.float32, device="cuda")
    call("vxm_vecint_fwd" if nd == 3 else "vxm_vecint2d_fwd", ptr(v), ptr(steps), vec.shape[0], *dims, nsteps, stream())
    torch.cuda.synchronize()
    steps = N(steps)
    out = vxm.layers.VecInt(dims, nsteps).cuda()(v)
    out.backward(G(gout))
    torch.cuda.synchronize()
    assert same_bits(N(out), steps[-1])
    fields = [vec * np.float32(2.0 ** -nsteps)] + [steps[k] for k in range(nsteps - 1)]        # the power-of-two scale is exact
    _, g64, outs = orc.vecint_arbiter(vec, nsteps, gout, fields=fields)
    fwd, bwd = VECINT_GATES[nd]
    tag = "vecint %s nsteps %d" % ("x".join(map(str, dims)), nsteps)
    for k in range(nsteps):
        gate(tag + " step %d forward vs fp64" % (k + 1), rel_l2(steps[k], outs[k]), fwd)
    gate(tag + " backward vs fp64", rel_l2(N(v.grad), g64), bwd)
    whole = rel_l2(steps[-1], orc.vecint_arbiter(vec, nsteps)[0])
    print("[info] %-66s measured %.3e  (not gated)" % (tag + " whole chain vs the arbiter on the reference's fields", whole))
    if nsteps == 1:
        assert whole < fwd


def _footprint_forward(vxm, kind, x, fl):
    """(kernel output, the flow it sampled at) of one of the five forward kernels on the sampled tensor x"""
    dims = wc.FOOTPRINT_DIMS[kind]
    if kind.startswith("vecint"):
        return N(vxm.layers.VecInt(dims, 1).cuda()(G(x))), None
    if kind == "fused":
        return _fused_forward(G(x), G(fl), dims, tuple(d // 2 for d in dims), 0)
    return N(vxm.layers.SpatialTransformer(dims).cuda()(G(x), G(fl))), fl


@pytest.mark.parametrize("kind", wc.FOOTPRINT)
def test_warp_non_finite_footprint(vxm, kind):
    """One NaN and one +Inf in border voxels of the sampled tensor (for VecInt the field itself), samples placed outside the volume along the
    lines through them.  The set of non-finite outputs of each of the five forward kernels must EQUAL the fp32 reference's on the same inputs --
    ATen's zero padding never reads an outside corner; a kernel that loads the clamped voxel and multiplies it by a zero weight makes Inf * 0 =
    NaN of every such sample -- and every other voxel keeps the bits of the run on the clean input (VecInt: except at the two poisoned voxels,
    which also MOVE: their own coordinates are non-finite).  Not vacuous: the reference's set is non-empty and below 5 % of the voxels, and at
    least 5 samples have an outside corner whose clamped index names a poisoned voxel while the reference is finite there.
    Backward (warp3d, warp2d): a NaN in gout against the footprint of the reference's autograd, gsrc and gflow."""
    dims = wc.FOOTPRINT_DIMS[kind]
    x, fl, gout, where = wc.footprint_arrays(kind)
    xp = wc.poisoned(x, where)
    clean, _ = _footprint_forward(vxm, kind, x, fl)
    got, flow = _footprint_forward(vxm, kind, xp, fl)
    if kind.startswith("vecint"):
        ref = orc.vecint(T(xp), 1).numpy()
        flow = xp * np.float32(0.5)
    else:
        ref = orc.spatial_transformer(T(xp), T(flow)).numpy()
    coords = orc._src_coords_explicit(flow)
    mask = bad(xp).any(axis=1)
    hits = wc.clamped_poison_hits(coords, dims, mask) & ~bad(ref).any(axis=1)
    print("[footprint] %-9s reference non-finite %d of %d, kernel %d; samples whose clamped outside corner names a poisoned voxel (reference finite): %d"
          % (kind, bad(ref).sum(), ref.size, bad(got).sum(), hits.sum()))
    assert 0 < bad(ref).sum() < 0.05 * ref.size and hits.sum() >= 5
    same_set(kind + " forward", got, ref)
    keep = ~bad(ref)
    if kind.startswith("vecint"):
        keep &= ~np.broadcast_to(mask[:, None], keep.shape)
    assert same_bits(got[keep], clean[keep]), kind + ": a finite output changed with the poison"
    if kind not in ("warp3d", "warp2d"):
        return
    gn = gout.copy()
    gn[(0, 0) + tuple(d // 2 for d in dims)] = np.nan
    _, rgs, rgf = _reference(x, flow, gn)
    _, gs, gf = _layer_run(vxm, dims, x, flow, gn)
    _, cgs, cgf = _layer_run(vxm, dims, x, flow, gout)
    print("[footprint] %-9s NaN in gout: reference gsrc %d gflow %d non-finite, kernel %d %d" % (kind, bad(rgs).sum(), bad(rgf).sum(), bad(gs).sum(), bad(gf).sum()))
    assert 0 < bad(rgs).sum() <= 2 ** len(dims) and 0 < bad(rgf).sum() <= len(dims)
    same_set(kind + " gsrc", gs, rgs)
    same_set(kind + " gflow", gf, rgf)
    assert same_bits(gf[~bad(rgf)], cgf[~bad(rgf)]), kind + ": a finite flow gradient changed with the poison"
    gate("%s gsrc beside the NaN footprint vs the clean run" % kind, rel_l2(gs[~bad(rgs)], cgs[~bad(rgs)]), WARP_GATES[len(dims)][1])
