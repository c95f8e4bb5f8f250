"""The bf16-activation engine (voxelmorph_amd/csrc/conv_bf16.hip) through the C ABI, bit for bit.  Run on the MI355X box: `pytest -m gpu`.

Every input of tests/bf16_cases.py is exactly summable (small integers times a power of two, every partial sum below 2^24), so the fp32
accumulation of the kernels is exact in any order and on any tile shape: what a kernel stores is the round-to-nearest-even bf16 of a
known integer, and every comparison here is an equality of bits against the plain tap-by-tap arbiter of that module (whose agreement with
F.conv3d / autograd in float64 is tests/test_cpu_bf16.py).  The one inexact assertion is the pinned NaN-for-Inf set of
`test_non_finite_activations`.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bf16_cases as bc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64               # NaN-prefilled elements in front of and behind every output tensor
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    import voxelmorph_amd  # noqa: F401
    from voxelmorph_amd import _lib
    _lib.lib()
    return _lib


def guarded(shape, dtype):
    """a NaN-prefilled output tensor inside a NaN-prefilled allocation: (tensor, allocation)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device="cuda")
    return whole[GUARD:GUARD + n].view(shape), whole


def untouched(whole):
    return bool(torch.isnan(torch.cat([whole[:GUARD], whole[-GUARD:]])).all())


def dev_blocked(x, cblk=None):
    return None if x is None else bc.blocked(x, cblk).cuda()


def pack(lib, wg, ci_lo, ci_n, flip, batch=False):
    """the packed operator of fp32 cuda weights `wg`, through vxm_bf16_conv_pack_weights or one job of vxm_bf16_conv_pack_weights_batch"""
    cout, cin = wg.shape[:2]
    inc, outc = (cout, ci_n) if flip else (ci_n, cout)
    wp = torch.full((lib.lib().vxm_bf16_conv_packed_bytes(inc, outc),), 0xAB, dtype=torch.uint8, device="cuda")
    if batch:
        table = (lib.Bf16PackJob * 1)()
        table[0] = lib.Bf16PackJob(wg.data_ptr(), wp.data_ptr(), cin, cout, ci_lo, ci_n, 1 if flip else 0)
        lib.call("vxm_bf16_conv_pack_weights_batch", ctypes.cast(table, ctypes.c_void_p), 1, lib.stream())
    else:
        lib.call("vxm_bf16_conv_pack_weights", wg.data_ptr(), cin, cout, ci_lo, ci_n, 1 if flip else 0, wp.data_ptr(), lib.stream())
    return wp


class Launch:
    """the device operands of one run of bf16_cases.build_run, uploaded once"""

    def __init__(self, lib, run, batch_pack=False):
        self.lib, self.run = lib, run
        self.wg = run["w"].to(torch.float32).cuda()
        self.wp = pack(lib, self.wg, *run["pack"], batch=batch_pack)
        self.x0, self.x1 = dev_blocked(run["x0"], run["C0"]), dev_blocked(run["x1"])
        self.mask = dev_blocked(run["mask"])
        self.bias = run["bias"].to(torch.float32).cuda() if run["bias"] is not None else None

    def __call__(self, rev=0, x0=None):
        lib, run = self.lib, self.run
        B, (D, H, W), cout = run["B"], run["vol"], run["cout"]
        y, whole = guarded((B, cout, D, H, W), torch.float32) if run["planar"] else guarded((B, cout // 8, D, H, W, 8), bc.BF)
        lib.call("vxm_bf16_conv_fwd", lib.ptr(self.x0 if x0 is None else x0), run["C0"], 1 if run["up0"] else 0, lib.ptr(self.x1), run["C1"],
                 lib.ptr(self.wp), lib.ptr(self.bias), lib.ptr(y), cout, (1 if run["planar"] else 0) | rev, float(run["slope"]),
                 lib.ptr(self.mask), float(run["mask_slope"]), B, D, H, W, lib.stream())
        torch.cuda.synchronize()
        assert untouched(whole), "the launch wrote outside its output tensor"
        return y.cpu()


def expected(run, v):
    """what the kernel stores for the arbiter's fp32 values: planar fp32 as they are, blocked outputs rounded once (RNE), as bits"""
    return v.contiguous().view(torch.int32) if run["planar"] else bc.bits(bc.blocked(v, run["cout"]))


def as_bits(run, y):
    return y.contiguous().view(torch.int32) if run["planar"] else bc.bits(y)


def check_conv(lib, op, direction, masked, revs=(0,)):
    run = bc.build_run(op, direction, masked)
    _, v = bc.run_reference(run, torch.float32 if op["multi"] else torch.float64)
    want = expected(run, v)
    launch = Launch(lib, run)
    for rev in revs:
        assert torch.equal(as_bits(run, launch(rev)), want), (op["name"], direction, masked, rev)
    return run


@pytest.mark.parametrize("case", bc.CONV_IDS, ids=bc.run_id)
def test_conv_exact(lib, case):
    """forward, and the flipped operator onto every segment (backward-data), with and without the fused LeakyReLU' mask: one tile per block"""
    name, direction, masked = case
    run = check_conv(lib, bc.OP_BY_NAME[name], direction, masked)
    assert bc.conv_geometry(run["C0"] + run["C1"], run["cout"], run["vol"], run["B"], run["planar"])["ntiles"] < 64


@pytest.mark.parametrize("case", bc.MULTI_IDS, ids=bc.run_id)
def test_multi_tile_conv_exact_in_both_walk_directions(lib, case):
    """>= 64 tiles: the XCD range split; with VXM_BF16_PERSIST < 0 (the variant runs below) every block walks several tiles.  The `| 2`
    walk-back flag is scheduling: the same bits as the arbiter in both directions"""
    name, direction, masked = case
    op = bc.OP_BY_NAME[name]
    run = check_conv(lib, op, direction, masked, revs=(0, 2))
    if direction == "fwd":
        assert bc.conv_geometry(run["C0"] + run["C1"], run["cout"], run["vol"], run["B"], run["planar"])["ntiles"] >= 64


@pytest.mark.parametrize("direction,masked", [("fwd", False), ("fwd", True), ("flip0", True)])
def test_multi_tile_default_grid_gives_blocks_a_second_tile(lib, direction, masked):
    """16 -> 16 on 64 x 64 x W with W from the device's CU count: more tiles than the 2 x CUs persistent blocks of the default grid"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    op = bc.default_grid_op(cus)
    run = check_conv(lib, op, direction, masked, revs=(0, 2))
    assert bc.conv_geometry(run["C0"], run["cout"], run["vol"], run["B"])["ntiles"] >= 2 * cus + 64


@pytest.mark.parametrize("case", bc.FUSED_IDS, ids=lambda t: "%s%s" % (t[0], "-mask" if t[1] else ""))
def test_fused_bwd_data_up_exact(lib, case):
    """vxm_bf16_conv_bwd_data_up: adjoint conv, bf16 rounding of every full-resolution value, exact 2 x 2 x 2 sum, low-resolution mask, rounding"""
    name, masked = case
    fu = bc.FUSED_BY_NAME[name]
    fr = bc.build_fused(fu, masked)
    _, s = bc.fused_reference(fr, torch.float32 if fu["multi"] else torch.float64)
    B, (D, H, W), cdz, cup = fr["B"], fr["vol"], fr["cdz"], fr["cup"]
    wg = fr["w"].to(torch.float32).cuda()
    wp = pack(lib, wg, 0, cup, True)
    dzb, maskb = dev_blocked(fr["dz"]), dev_blocked(fr["mask"])
    got, whole = guarded((B, cup // 8) + fr["low"] + (8,), bc.BF)
    lib.call("vxm_bf16_conv_bwd_data_up", lib.ptr(dzb), cdz, lib.ptr(wp), lib.ptr(got), cup, lib.ptr(maskb), float(fr["mask_slope"]), B, D, H, W,
             lib.stream())
    torch.cuda.synchronize()
    assert untouched(whole)
    assert torch.equal(bc.bits(got.cpu()), bc.bits(bc.blocked(s)))
    if fu["multi"]:
        assert bc.conv_geometry(cdz, cup, fr["vol"], B)["ntiles"] >= 64


@pytest.mark.parametrize("cout_w,cin_w", bc.IMPULSE_OPS)
@pytest.mark.parametrize("flip", [False, True])
def test_impulse_response_is_the_rounded_weight_of_the_matching_tap(lib, cout_w, cin_w, flip):
    """one 1.0 per input channel (interior, tile face, volume corner), non-integer fp32 weights with bf16 ties: every displaced voxel holds
    the RNE-rounded weight of its tap, everything else is zero -- the rounding and the tap order of bf_pack_word, through both packers"""
    x, want, w = bc.impulse_case(cout_w, cin_w, flip)
    n_in, n_out = (cout_w, cin_w) if flip else (cin_w, cout_w)
    run = dict(x0=x, x1=None, C0=n_in, up0=False, C1=0, pack=(0, cin_w, flip), w=w, bias=None, cout=n_out, planar=False, slope=1.0, mask=None,
               mask_slope=1.0, B=bc.IMPULSE_B, vol=bc.IMPULSE_VOL)
    single, batch = Launch(lib, run), Launch(lib, run, batch_pack=True)
    assert torch.equal(single.wp, batch.wp)
    for launch in (single, batch):
        assert torch.equal(bc.bits(launch()), bc.bits(bc.blocked(want)))


# ---------------------------------------------------------------------------------------------------------------------------------
# non-finite activations
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ["fwd", "flip0"])
@pytest.mark.parametrize("name", ["past_tile", "mt_16_32_odd"])
def test_non_finite_activations(lib, name, direction):
    """One +Inf, then one NaN, at a voxel p (interior, on a tile face, the volume's corner) in a channel of the first and of the second 8 of a
    chunk.  The non-finite outputs are exactly the reference's (the clipped 3 x 3 x 3 box around p), NaN wherever the reference has NaN, the
    same sign wherever both are Inf, every finite output unchanged.  Pinned, from the code: the two padded K slots of the fifth K-step
    (units 18, 19: zero weights) read the voxel of unit 0 -- tap kd = 0, kw = 0, channel block 0 -- so an Inf in the FIRST 8 channels of a
    chunk turns the outputs p + (1, {-1, 0, 1}, 1) into NaN (0 x Inf) where the reference has +-Inf; nowhere else."""
    op = bc.OP_BY_NAME[name]
    run = bc.build_run(op, direction, False)
    B, (D, H, W), cin = run["B"], run["vol"], run["C0"]
    rows = bc.conv_geometry(cin, run["cout"], run["vol"], B)["ROWS"]
    zbase = bc.conv_taps(run["x0"], run["wop"])
    launch = Launch(lib, run)
    b = B - 1
    seen_nan_for_inf = 0
    for p in ((3, 3, 5), (7, min(rows, H) - 1, 15), (D - 1, H - 1, W - 1)):
        for c, first8 in ((cin - 16 + 3, True), (cin - 16 + 11, False)):
            for val in (float("inf"), NAN):
                x = run["x0"].clone()
                z = zbase.clone()
                box = torch.zeros(z.shape, dtype=torch.bool)
                for t in range(27):
                    d, h, w = p[0] - (t // 9 - 1), p[1] - ((t // 3) % 3 - 1), p[2] - (t % 3 - 1)       # the output whose tap t reads p
                    if 0 <= d < D and 0 <= h < H and 0 <= w < W:
                        z[b, :, d, h, w] += -run["wop"][:, c, t] * x[b, c][p] + run["wop"][:, c, t] * val      # (0 x Inf = NaN, elementwise)
                        box[b, :, d, h, w] = True
                x[b, c][p] = val
                want = bc.rne(bc.epilogue(z, run["bias"], run["slope"], None, 1.0))
                xb = bc.blocked(x.to(torch.float32), cin)
                assert torch.isinf(xb).sum() + torch.isnan(xb).sum() == 1
                got = bc.planar(launch(x0=xb.cuda()))
                gf, wf = got.float(), want.float()
                bad_g, bad_w = ~torch.isfinite(gf), ~torch.isfinite(wf)
                assert torch.equal(bad_w, box) and torch.equal(bad_g, bad_w), (p, c, val)
                assert torch.equal(bc.bits(got)[~bad_w], bc.bits(want)[~bad_w])                        # every finite output, bit for bit
                assert bool(torch.isnan(gf)[torch.isnan(wf)].all())
                both_inf = torch.isinf(gf) & torch.isinf(wf)
                assert torch.equal(gf[both_inf], wf[both_inf])
                predicted = torch.zeros_like(box)
                if first8 and val == float("inf"):
                    for dh in (-1, 0, 1):
                        d, h, w = p[0] + 1, p[1] + dh, p[2] + 1
                        if d < D and 0 <= h < H and w < W:
                            predicted[b, :, d, h, w] = True
                nan_for_inf = torch.isnan(gf) & torch.isinf(wf)
                assert not bool((nan_for_inf & ~predicted).any()), (p, c, val)
                seen_nan_for_inf += int(nan_for_inf.sum())
    print("%s %s: NaN where the reference has +-Inf at %d outputs (all inside the predicted set)" % (name, direction, seen_nan_for_inf))


# ---------------------------------------------------------------------------------------------------------------------------------
# weight gradients
# ---------------------------------------------------------------------------------------------------------------------------------
def run_wgrad(lib, c):
    """gw, gb of two calls (the workspace scribbled over in between), checked against the arbiter and against each other; returns NBLK"""
    x0, x1, dz = bc.wgrad_tensors(c)
    gw_ref, gb_ref = bc.wgrad_reference(c)
    B, (D, H, W) = c["B"], c["vol"]
    cin, cdz, cin_w, cout_w = c["c0"] + c["c1"], c["cdz"], c["cin_w"], c["cout_w"]
    x0b, x1b, dzb = dev_blocked(x0), dev_blocked(x1), dev_blocked(dz)
    need = lib.lib().vxm_bf16_conv_bwd_weight_workspace_bytes(cin, cdz, B, D, H, W)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        work.fill_(0xFF)
        (gw, gww), (gb, gbw) = guarded((cout_w, cin_w, 3, 3, 3), torch.float32), guarded((cout_w,), torch.float32)
        lib.call("vxm_bf16_conv_bwd_weight", lib.ptr(x0b), c["c0"], 1 if c["up0"] else 0, lib.ptr(x1b), c["c1"], lib.ptr(dzb), cdz, lib.ptr(gw), cin_w,
                 cout_w, lib.ptr(gb), lib.ptr(work), need, B, D, H, W, lib.stream())
        torch.cuda.synchronize()
        assert untouched(gww) and untouched(gbw), "gw / gb rows outside [Cout_w][Cin_w] were written"
        outs.append((gw.cpu(), gb.cpu()))
    assert np.array_equal(outs[0][0].numpy(), gw_ref.to(torch.float32).numpy()), c["name"]
    assert np.array_equal(outs[0][1].numpy(), gb_ref.to(torch.float32).numpy()), c["name"]
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    return bc.workspace_nblk(need, cin // 16, cdz // 16)


@pytest.mark.parametrize("c", [c for c in bc.WGRAD if not c["big"]], ids=lambda c: c["name"])
def test_weight_gradient_exact(lib, c):
    run_wgrad(lib, c)


def test_weight_gradient_ring_wraps_exact(lib):
    """x0 32 + x1 16, dz 32, 47 x 60 x 120, B = 2: depth segments of >= 3 tiles, so the 6-slot plane ring wraps, the loads of tile t + 1 are
    in flight under tile t, the second dZ buffer is used, and the last tile's second slice lies beyond D.  If another CU count makes the
    case lose the path this FAILS: raise D in the table."""
    c = bc.WGRAD_BY_NAME["wg_ring"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    D, H, W = c["vol"]
    nblk, nseg, seg_len = bc.bwb_tasks(3, c["B"], D, H, W, cus)
    assert seg_len >= 3 and D % 2 == 1, (cus, nblk, nseg, seg_len)
    assert run_wgrad(lib, c) == nblk
    if cus == bc.CUS_REF:
        assert (nblk, nseg, seg_len) == bc.WGRAD_TASKS_256["wg_ring"] and nblk % 8 != 0


def test_weight_gradient_task_rr_exact(lib):
    """16, 16, 128^3, values in {-1, 0, 1}: D H W >= 2^21 and NBLK % 8 == 0, the round-robin task order inside an XCD's range"""
    c = bc.WGRAD_BY_NAME["wg_task_rr"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    D, H, W = c["vol"]
    nblk, nseg, seg_len = bc.bwb_tasks(1, c["B"], D, H, W, cus)
    assert nblk % 8 == 0 and D * H * W >= 1 << 21 and seg_len >= 3, (cus, nblk, nseg, seg_len)
    assert run_wgrad(lib, c) == nblk


# ---------------------------------------------------------------------------------------------------------------------------------
# other grids, in fresh processes
# ---------------------------------------------------------------------------------------------------------------------------------
def _rerun(env_extra, select, timeout=600):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.join(ROOT, "tests", "test_gpu_bf16_exact.py"), "-k", select],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.parametrize("persist", ["-8", "-24", "0"])
def test_multi_tile_and_fused_cases_on_other_grids_in_subprocess(persist):
    """VXM_BF16_PERSIST=-8: one block per XCD range, 8 to 19 tiles each (the chunk stream across tile changes, the prefetch under the MFMAs,
    weights kept in LDS across tiles, the uneven range split, the walk-back flag under a multi-tile walk); -24: three blocks round-robin
    inside uneven ranges; 0: one tile per block"""
    if os.environ.get("VXM_BF16_PERSIST") is not None:
        pytest.skip("already inside a variant run")
    _rerun({"VXM_BF16_PERSIST": persist}, "multi_tile_conv or multi_tile_default_grid or fused_bwd_data_up")


# ---------------------------------------------------------------------------------------------------------------------------------
# elementwise kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def test_to_blocked_special_values_two_sources_and_strides(lib):
    """ties to even both ways, overflow to +-Inf, denormals, +-0, +-Inf, NaN, against torch's CPU RNE conversion; two sources with batch strides
    that are not the dense ones and V no multiple of 256"""
    s = bc.special_f32()
    B, C0, C1, V, cblk = 2, 5, 3, 285, 16
    rng = np.random.default_rng(5)
    big0 = torch.from_numpy(rng.standard_normal((B, C0 + 2, V)).astype(np.float32))
    big1 = torch.from_numpy(rng.standard_normal((B, C1 + 1, V)).astype(np.float32))
    d0, d1 = big0[:, :C0].clone(), big1[:, :C1].clone()
    d0.view(-1)[:2 * s.numel()] = torch.cat([s, s.flip(0)])
    d0[1].view(-1)[7:7 + s.numel()] = s
    d1[1].view(-1)[3:3 + s.numel()] = s
    big0[:, :C0], big1[:, :C1] = d0, d1
    g0, g1 = big0.cuda(), big1.cuda()
    out, whole = guarded((B, cblk // 8, V, 8), bc.BF)
    lib.call("vxm_bf16_to_blocked", g0.data_ptr(), C0, (C0 + 2) * V, g1.data_ptr(), C1, (C1 + 1) * V, lib.ptr(out), cblk, B, V, lib.stream())
    torch.cuda.synchronize()
    assert untouched(whole)
    want = torch.zeros((B, cblk, V), dtype=bc.BF)
    want[:, :C0], want[:, C0:C0 + C1] = big0[:, :C0].to(bc.BF), big1[:, :C1].to(bc.BF)
    got = out.cpu().permute(0, 1, 3, 2).reshape(B, cblk, V)
    assert bc.same_or_both_nan(got, want)
    assert torch.isnan(want.float()).sum() >= 18 and torch.isinf(want.float()).sum() >= 18
    # and back: from_blocked hands every bf16 pattern over as the fp32 with the same upper half; channels beyond C stay untouched
    patt = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).reshape(B, 2, 2048, 8).contiguous()       # every bf16 there is
    xb = patt.view(bc.BF).cuda()
    f, fwhole = guarded((B, 11, 2048), torch.float32)
    lib.call("vxm_bf16_from_blocked", lib.ptr(xb), 16, lib.ptr(f), 11, B, 2048, lib.stream())
    torch.cuda.synchronize()
    assert untouched(fwhole)
    ref = patt.view(bc.BF).permute(0, 1, 3, 2).reshape(B, 16, 2048)[:, :11].to(torch.float32)
    assert bc.same_or_both_nan(f.cpu(), ref)


def _pool_call(lib, fn, *args):
    lib.call(fn, *args, lib.stream())
    torch.cuda.synchronize()


def test_maxpool2_fwd_odd_extents_ties_and_nan(lib):
    B, C = 2, 16
    for vol in ((5, 7, 9), (4, 6, 8), (2, 3, 2)):
        x = bc.pool_inputs(vol)
        want, _ = bc.maxpool_reference(x)
        lo = tuple(s // 2 for s in vol)
        y, whole = guarded((B, C // 8) + lo + (8,), bc.BF)
        xb = dev_blocked(x)
        _pool_call(lib, "vxm_bf16_maxpool2_fwd", lib.ptr(xb), lib.ptr(y), B, C, *vol)
        assert untouched(whole)
        assert torch.isnan(want).any() and bc.same_or_both_nan(bc.planar(y.cpu()), want.to(bc.BF))


@pytest.mark.parametrize("slope", [1.0, 0.25, 0.2])
@pytest.mark.parametrize("skip", [False, True])
def test_maxpool2_bwd_ties_nan_skip_and_slopes(lib, slope, skip):
    """first arg-max under ATen's `(v > m) || isnan(v)` rule, + the skip gradient, x LeakyReLU'(x) (NaN and 0 take the slope), one rounding"""
    B, C, vol = 2, 16, (4, 6, 10)
    lo = tuple(s // 2 for s in vol)
    x = bc.pool_inputs(vol)
    rng = np.random.default_rng(11)
    gp = bc.ints(rng, (B, C) + lo, 100, -3).to(torch.float32)
    gs = bc.ints(rng, (B, C) + vol, 100, -3).to(torch.float32) if skip else None
    want = bc.maxpool_bwd_reference(x, gp, gs, slope).to(bc.BF)
    dz, whole = guarded((B, C // 8) + vol + (8,), bc.BF)
    xb, gpb, gsb = dev_blocked(x), dev_blocked(gp), dev_blocked(gs)
    _pool_call(lib, "vxm_bf16_maxpool2_bwd", lib.ptr(xb), lib.ptr(gpb), lib.ptr(gsb), lib.ptr(dz), slope, B, C, *vol)
    assert untouched(whole)
    assert bc.same_or_both_nan(bc.planar(dz.cpu()), want)


@pytest.mark.parametrize("masked", [False, True])
def test_upsample2_bwd_exact_sums_and_mask_values(lib, masked):
    B, C, low = 2, 16, (3, 5, 7)
    vol = tuple(2 * s for s in low)
    g = bc.ints(np.random.default_rng(2), (B, C) + vol, 200, -4).to(torch.float32)
    y = bc.mask_values((B, C) + low, "upsample") if masked else None
    gb, yb = dev_blocked(g), dev_blocked(y)
    for slope in (0.2, 0.25):
        want = bc.upsample2_bwd_reference(g, y, slope).to(bc.BF)
        dz, whole = guarded((B, C // 8) + low + (8,), bc.BF)
        _pool_call(lib, "vxm_bf16_upsample2_bwd", lib.ptr(gb), lib.ptr(yb), lib.ptr(dz), slope, B, C, *low)
        assert untouched(whole)
        assert torch.equal(bc.bits(bc.planar(dz.cpu())), bc.bits(want))
    assert bc.rounding_shares(bc.upsample2_bwd_reference(g, None, 1.0))[0] >= bc.MIN_ROUNDED       # (of the inputs: the sums need a rounding)


@pytest.mark.parametrize("words", [8192 * 256 + 257, 1])
def test_lrelu_bwd_second_grid_stride_pass_and_mask_values(lib, words):
    """dz = g x LeakyReLU'(y) on n 16-byte words; above 8192 x 256 words the grid takes a second pass.  Mask values +-0 and NaN take the slope."""
    n = words * 8
    gen = torch.Generator().manual_seed(words)
    g = torch.randn(n, generator=gen).to(bc.BF)
    y = torch.randint(-2, 3, (n,), generator=gen).to(torch.float32)
    y[3::11], y[7::13] = -0.0, NAN
    y[-8:] = torch.tensor([1.0, -1.0, 0.0, -0.0, NAN, 2.0, -2.0, 1.0])
    want = (g.to(torch.float32) * bc.lrelu_grad(y, 0.2)).to(bc.BF)
    dz, whole = guarded((n,), bc.BF)
    gg, yg = g.cuda(), y.to(bc.BF).cuda()
    lib.call("vxm_bf16_lrelu_bwd", lib.ptr(gg), lib.ptr(yg), lib.ptr(dz), 0.2, n, lib.stream())
    torch.cuda.synchronize()
    assert untouched(whole)
    assert torch.equal(bc.bits(dz.cpu()), bc.bits(want))
    assert words == 1 or words > 8192 * 256
