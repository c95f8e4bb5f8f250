"""The arbiters, the table and the gates of tests/test_gpu_losses.py, checked without a GPU: the float64 arbiters agree with float64 autograd of
the reference's formula, every row of tests/loss_cases.py reaches the branch of voxelmorph_amd/csrc/losses.hip it is named for (by arithmetic
on the constants restated from the source), the reference's non-finite footprints are what the GPU tests expect, and every gate literal of the
GPU test file is a `GATE` line of profiles/pr05_loss_gates_cpu.txt (the output of tools/loss_gates.py), recomputed here for a few classes."""
import os
import re

import numpy as np
import torch

import loss_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = {r[0]: r for r in lc.NCC_ROWS}
GROWS = {r[0]: r for r in lc.GRAD_ROWS}


def _grad_explicit(y, pen):
    """losses.py:102-135 spelled out in float64 numpy: (loss, dy)"""
    y = np.asarray(y, np.float64)
    nd, B = y.ndim - 2, y.shape[0]
    loss, g = 0.0, np.zeros_like(y)
    for a in range(2, y.ndim):
        d = np.diff(y, axis=a)
        n = d[0].size
        loss += (np.abs(d) if pen == "l1" else d * d).reshape(B, -1).mean(axis=1).mean() / nd
        dd = (np.sign(d) if pen == "l1" else 2 * d) / (n * nd * B)
        hi, lo = [slice(None)] * y.ndim, [slice(None)] * y.ndim
        hi[a], lo[a] = slice(1, None), slice(0, -1)
        g[tuple(hi)] += dd
        g[tuple(lo)] -= dd
    return loss, g


def test_arbiters_agree_with_float64_autograd_of_the_reference_formula():
    """oracle.ncc_explicit_win (separable sums, transposed box filters) against float64 autograd of oracle.ncc_loss (ATen's dense conv) on the
    small rows, to 1e-12 -- relative to the largest gradient entry, so that the rows whose true gradient vanishes are judged too.  The four
    regimes in which the variance cancels (offset, plateau, I == J, ramp) and the one-voxel volume (var = I^2 (1 - 1/n): nothing but the 1e-5
    keeps the quotient finite) lose up to 8 digits of float64 itself: two float64 summation orders agree to 1e-8 there (measured: 1.5e-9), far
    below the fp32 errors the GPU gates of those classes come from; I == J, whose gradient is ~1e-12 itself, is held to 1e-14 absolute.
    Grad: float64 autograd of oracle.grad_loss against the formula spelled out in numpy."""
    worst = {}
    for row in lc.NCC_ROWS:
        name, B, vol, win, regime = row
        if B * int(np.prod(vol)) > 25000 or (int(np.prod(vol)) > 5000 and max(win) > 9):      # (a dense 11^3 float64 conv takes seconds)
            continue
        if vol == lc.REG_VOL and win == [9] * 3 and regime != "offset":                       # (9^3 on the regime volume: the worst-conditioned one only)
            continue
        I, J = lc.ncc_arrays(row)
        l, gJ, gI = lc.ncc_arbiter(I, J, win)
        lr, rJ, rI = lc.ncc_reference(I, J, win, torch.float64)
        scale = 1.0 if regime == "same" else max(np.abs(rJ).max(), np.abs(rI).max(), 1e-30)      # I == J: the gradient itself is ~1e-12, absolute
        e = max(abs(l - lr), lc.max_abs(gJ, rJ) / scale, lc.max_abs(gI, rI) / scale)
        hard = regime in ("offset", "plateau", "same", "ramp", "single", "single1d")
        worst[hard] = max(worst.get(hard, 0.0), e)
        assert e <= (1e-14 if regime == "same" else 1e-8 if hard else 1e-12), (name, e)
    assert len(worst) == 2
    for row in lc.GRAD_ROWS:
        if int(np.prod(row[1])) > 25000:
            continue
        y = lc.grad_arrays(row)
        for pen in ("l1", "l2"):
            l, g = lc.grad_reference(y, pen, torch.float64)
            le, ge = _grad_explicit(y, pen)
            assert abs(l - le) <= 1e-12 * max(abs(le), 1.0) and lc.max_abs(g, ge) <= 1e-12 * max(np.abs(ge).max(), 1.0), (row[0], pen)


def test_the_constants_restated_from_losses_hip():
    src = open(os.path.join(ROOT, "voxelmorph_amd", "csrc", "losses.hip")).read()
    assert "constexpr int NF_TH = %d, NF_TW = %d, NF_SEG = %d;" % (lc.NF_TH, lc.NF_TW, lc.NF_SEG) in src
    assert "while (seg > 20 && cols * ((D + seg - 1) / seg) < 1024) seg = (seg + 1) / 2;" in src
    assert "(win >= %d && win <= %d && B > 0 && B <= %d)" % (lc.NCC_FUSED_WIN + (lc.NCC_MAX_GRID_B,)) in src
    assert "(gridDim.x & 7) == 0" in src and "#define VXM_GRAD_RU 4" in src
    caps = lc.GRAD_CAPS
    assert "rows4 > %d ? %d : rows4), B);          // 4 rows per block and pass; atomics" % ((caps["fwd"][0],) * 2) in src
    assert "rowsb > %d ? %d : rowsb" % ((caps["fwd_v4"][0],) * 2) in src and caps["fwd_v4"][1] == 4 * 4
    assert "rows4 > %d ? %d : rows4), B);        // 4 rows per block and pass" % ((caps["bwd"][0],) * 2) in src
    assert "rows8 > %d ? %d : rows8" % ((caps["bwd_v4"][0],) * 2) in src and caps["bwd_v4"][1] == 8
    assert len(re.findall(r"B <= 65535 && C > 0", src)) == 1          # the Grad refusal: a batch beyond gridDim.y
    import test_gpu_parity as P
    assert lc.TODAY_NCC == (P.NCC_LOSS_GATE, P.NCC_GRAD_GATE, P.NCC_GRAD_GATE_1D)


def test_every_ncc_row_reaches_the_branch_it_is_named_for():
    assert len(lc.NCC_IDS) == len(set(lc.NCC_IDS))
    for row in lc.NCC_ROWS:
        name, B, vol, win, regime = row
        tag = name.split("_")[0]
        path = lc.ncc_path(B, vol, win)
        I, J = lc.ncc_arrays(row)
        assert I.shape == J.shape == (B, 1) + vol and I.dtype == J.dtype == np.float32
        if len(vol) == 3:
            cols, seg, segs, remap = lc.ncc_grid(B, vol)
        if tag == "halo":           # one block per sample, thinner than the tile on every axis; the four rows are the four instances R = 1 .. 4
            assert path == "fused" and cols == segs == 1 and vol[1] < lc.NF_TH and vol[2] < lc.NF_TW and vol[0] <= win[0] // 2 + 1
        elif tag == "single":
            assert path == "fused" and vol == (1, 1, 1)
        elif tag == "tile":
            assert path == "fused" and cols == (1 if vol[1:] == (lc.NF_TH, lc.NF_TW) else 4) and vol[1] - lc.NF_TH in (0, 1) and vol[2] - lc.NF_TW in (0, 1)
        elif tag == "remap":
            assert path == "fused" and remap and cols in (8, 16)
        elif tag == "noremap":
            assert path == "fused" and not remap and cols == 6
        elif tag == "seg20":
            assert path == "fused" and seg == 20 and segs == {20: 1, 21: 2, 41: 3}[vol[0]] and (vol[0] - 1) % 20 + 1 == (20 if vol[0] == 20 else 1)
        elif tag == "seg40":        # 512 columns x 2 segments = 1024 blocks: the rule keeps 40; segments of 40 and 1; 64 tiles along W
            assert path == "fused" and seg == lc.NF_SEG and segs == 2 and cols * B * segs == 1024 and vol[0] - seg == 1 and vol[2] // lc.NF_TW == 64
        elif tag == "generic":
            assert path == "generic" and win[0] in (1, 11, 13)
        elif tag == "batch":
            assert path == "generic" and B > lc.NCC_MAX_GRID_B and win[0] == 3
        elif tag == "anywin":
            pad = win[0] // 2
            assert path == "win" and all(s + 2 * pad - w + 1 >= 1 for s, w in zip(vol, win))
        elif tag in ("planar", "signal"):
            assert len(vol) == (2 if tag == "planar" else 1) and regime == ("single1d" if vol == (1,) else "lowdim") and len(set(win)) == 1 and win[0] % 2 == 1
        else:
            assert tag == regime and vol == lc.REG_VOL and path == {"9": "fused", "3": "fused", "11": "generic", "9x9x5": "win"}[lc._wt(win)]
    fused = set(r[3][0] for r in lc.NCC_ROWS if r[0].startswith("halo"))
    assert fused == {3, 5, 7, 9}
    # the regimes are what they say
    I, J = lc.ncc_arrays(ROWS["same_1x20x27x40_w9"])
    assert np.array_equal(I, J)
    I, J = lc.ncc_arrays(ROWS["zerobg_1x20x27x40_w9"])
    keep = lc.clipped_box(lc.REG_VOL, (0, 0, 0), 0)
    keep[:] = False
    keep[lc.REG_BOX] = True
    assert not I[0, 0][~keep].any() and not J[0, 0][~keep].any() and I[0, 0][keep].all()
    I, J = lc.ncc_arrays(ROWS["plateau_1x20x27x40_w9"])
    assert np.all(I[..., 20:] == np.float32(0.3)) and np.all(J[..., 20:] == np.float32(0.7)) and I[..., :20].std() > 0.2
    I, J = lc.ncc_arrays(ROWS["offset_1x20x27x40_w9"])
    assert I.min() >= 100 and J.min() >= 100
    I, J = lc.ncc_arrays(ROWS["ramp_1x20x27x40_w9"])
    assert np.array_equal(J, I * I) and I[0, 0, 0, 0, 0] == 0 and I[0, 0, -1, -1, -1] == 1
    I, J = lc.ncc_arrays(ROWS["anti_1x20x27x40_w9"])
    assert np.array_equal(J, np.float32(1) - I)
    assert lc.ncc_arrays(ROWS["signed_1x20x27x40_w9"])[0].min() < -0.4 and lc.ncc_arrays(ROWS["x255_1x20x27x40_w9"])[0].max() > 200
    # the non-finite volume: four ragged tiles, segments of 20 and 4, the positions on either side of the edges
    cols, seg, segs, _ = lc.ncc_grid(1, lc.NF_VOL)
    assert (cols, seg, segs) == (4, 20, 2)
    P = lc.NF_POS
    assert P["tile_lo"][1:] == (lc.NF_TH - 1, lc.NF_TW - 1) and P["tile_hi"][1:] == (lc.NF_TH, lc.NF_TW)
    assert P["seg_lo"][0] == seg - 1 and P["seg_hi"][0] == seg and P["last"] == tuple(s - 1 for s in lc.NF_VOL)
    assert len(lc.NF_CASES) == 7 * 2 * 3


def test_every_grad_row_reaches_the_branch_it_is_named_for():
    assert len(lc.GRAD_IDS) == len(set(lc.GRAD_IDS))
    for name, shape, regime in lc.GRAD_ROWS:
        v4 = shape[-1] % 4 == 0
        fwd, bwd = ("fwd_v4", "bwd_v4") if v4 else ("fwd", "bwd")
        passes = (lc.grad_passes(shape, fwd), lc.grad_passes(shape, bwd))
        if name.startswith("stride_v4"):
            assert v4 and passes == (9, 2) and lc.grad_rows(shape) == 131670 and lc.grad_rows(shape) % 4 == 2
        elif name.startswith("stride_scalar"):
            assert not v4 and passes == (3, 2) and lc.grad_rows(shape) == 65712
        elif name.startswith("stride_fwd_v4"):
            assert v4 and passes == (2, 1) and shape[0] == 2
        else:
            assert passes == (1, 1)
        if name.startswith("w_v4"):
            assert v4 and shape[2:4] == (2, 2)
        if name.startswith("w_scalar"):
            assert not v4 and shape[2:4] == (2, 2)
    lanes = [-(-(GROWS["w_v4_2x3x2x2x%d" % W][1][-1] // 4) // 64) for W in (4, 8, 256, 260, 516)]       # passes of 64 lanes of 16 bytes over a row
    assert lanes == [1, 1, 1, 2, 3] and 256 // 4 == 64
    assert lc.GRAD_UNALIGNED[-1] % 4 == 0 and [s[-1] % 4 for s in lc.GRAD_NF_SHAPES] == [0, 3, 0] and len(lc.GRAD_NF_SHAPES[2]) == 4
    y = lc.grad_arrays(GROWS["ties_2x3x5x6x8"])
    assert np.array_equal(y * 2, np.round(y * 2)) and (np.diff(y, axis=-1) == 0).mean() > 0.1
    assert len(np.unique(lc.grad_arrays(GROWS["const_2x3x5x6x7"]))) == 1 and np.abs(lc.grad_arrays(GROWS["big_2x3x5x6x8"])).max() > 2e4
    pos = lc.grad_nf_positions(lc.GRAD_NF_SHAPES[0])
    assert len(pos) == 7 and pos["last2"][2] == 7 and pos["first0"][0] == 0 and pos["last0"][0] == 3


def test_reference_non_finite_footprint_of_ncc():
    """One NaN / Inf voxel in either image: the fp32 reference (ATen) gives a NaN loss and non-finite gradients on exactly the set the float64
    arbiter gives -- for a cubic window the (4R+1)^3 box around the voxel, clipped to the volume: 125 voxels at win 3 for an interior voxel."""
    for win in lc.NF_WINS:
        R2 = 2 * (win[0] // 2)
        dense = win[0] > 3 and len(set(win)) == 1      # 9^3, 11^3: the reference on every position, both images and all three values once
        for k, case in enumerate(lc.NF_CASES):
            I, J = lc.ncc_nf_arrays(win, case)
            l64, gJ, gI = lc.ncc_arbiter(I, J, win)
            assert np.isnan(l64)
            if k % 2 == 0 or not dense:
                with np.errstate(invalid="ignore"):
                    l32, rJ, rI = lc.ncc_reference(I, J, win, torch.float32)
                assert np.isnan(l32)
                assert np.array_equal(~np.isfinite(gJ), ~np.isfinite(rJ)) and np.array_equal(~np.isfinite(gI), ~np.isfinite(rI)), (win, case)
            if len(set(win)) == 1:
                box = lc.clipped_box(lc.NF_VOL, lc.NF_POS[case[0]], R2)
                assert np.array_equal(~np.isfinite(gJ[0, 0]), box) and np.array_equal(~np.isfinite(gI[0, 0]), box), (win, case)
                if case[0] == "interior" and win[0] == 3:
                    assert box.sum() == 125
    assert lc.clipped_box((40, 40, 40), (20, 20, 20), 8).sum() == 4913               # win 9, were the volume large enough


def test_reference_non_finite_footprint_of_grad():
    """+-Inf in the field: the reference's loss is +Inf for l1 and l2; its l2 gradient is +-Inf at the voxel and at its existing neighbours and has no
    NaN; its l1 gradient is finite everywhere.  NaN: a NaN loss; the l1 gradient stays finite (sign(NaN) = 0 in ATen), the l2 gradient is NaN there."""
    for shape in lc.GRAD_NF_SHAPES:
        for where, pos in lc.grad_nf_positions(shape).items():
            nbrs = sum(1 for a in range(len(pos)) for s in (-1, 1) if 0 <= pos[a] + s < shape[2 + a])
            for val in lc.GRAD_NF_VALUES:
                y = lc.grad_nf_array(shape, pos, val)
                for pen in ("l1", "l2"):
                    l, g = lc.grad_reference(y, pen, torch.float32, 2)
                    if np.isnan(val):
                        assert np.isnan(l) and np.isnan(g).sum() == (0 if pen == "l1" else nbrs + 1) and not np.isinf(g).any()
                    else:
                        assert l == np.inf and not np.isnan(g).any() and np.isinf(g).sum() == (0 if pen == "l1" else nbrs + 1)
                        if pen == "l2":
                            assert g[(0, 1) + pos] == val
    # the refusals are the reference's NaN: the mean of no differences
    assert np.isnan(lc.grad_reference(np.zeros((1, 2, 1, 5, 8), np.float32), "l2", torch.float32)[0])


def _recorded():
    out = {}
    with open(os.path.join(ROOT, "profiles", "pr05_loss_gates_cpu.txt")) as f:
        for line in f:
            if line.startswith("GATE "):
                parts = line.split()
                out[" ".join(parts[1:-1])] = float(parts[-1])
    return out


def test_gpu_gates_are_four_times_the_measured_reference_error():
    """Every literal of test_gpu_losses.py is a GATE line of the committed output of tools/loss_gates.py, and the other way round.  A few classes
    that take seconds are recomputed: ATen's summation order depends on the CPU's vector width, so the recomputed gate has to agree with the
    literal within a factor 1.5 (a loss at its floor: exactly), not to the last digit."""
    import test_gpu_losses as T
    recorded = _recorded()
    used = {}
    for cls, (gl, gg) in T.NCC_GATES.items():
        used["ncc %s loss_abs" % cls] = gl
        maxabs = cls.split("/")[0] in lc.MAXABS or cls.endswith("/1")
        used["ncc %s %s" % (cls, "grad_maxabs" if maxabs else "grad")] = gg
    for cls, (gl, gg) in T.GRAD_GATES.items():
        used["grad %s loss_rel" % cls] = gl
        used["grad %s grad" % cls] = gg
    assert used == recorded
    assert set(T.NCC_GATES) == set(lc.NCC_CLASSES) and set(T.GRAD_GATES) == set(lc.GRAD_CLASSES)
    floor = float("%.3e" % (lc.MARGIN * lc.HALF_ULP))
    assert T.FLOOR == lc.MARGIN * 2.0 ** -24 and min(min(v[0] for v in T.NCC_GATES.values()), min(v[0] for v in T.GRAD_GATES.values())) == floor
    # no new gate of a well-conditioned class is looser than the fixed gates of test_gpu_parity.py
    for cls, (gl, gg) in T.NCC_GATES.items():
        if cls.split("/")[0] in lc.WELL:
            assert gl <= lc.TODAY_NCC[0] and gg <= (lc.TODAY_NCC[2] if cls.startswith("lowdim") else lc.TODAY_NCC[1])
    assert all(max(T.GRAD_GATES[c]) <= lc.TODAY_GRAD for c in ("l1/normal", "l2/normal"))
    torch.set_num_threads(1)

    def close(new, lit):
        return new == lit == floor or float("%.3e" % new) == lit or (lit / 1.5 <= new <= lit * 1.5)
    for cls in ("plateau/9x9x5", "offset/3", "ramp/9", "same/3", "single/9", "signed/11", "uniform/1", "lowdim/11"):
        gl, gg, _ = lc.ncc_class_gates(cls, lc.TODAY_NCC)
        assert close(gl, T.NCC_GATES[cls][0]) and close(gg, T.NCC_GATES[cls][1]), (cls, gl, gg, T.NCC_GATES[cls])
    for cls in ("l1/ties", "l2/ties", "l2/big"):
        gl, gg, _ = lc.grad_class_gates(cls, lc.TODAY_GRAD)
        assert close(gl, T.GRAD_GATES[cls][0]) and close(gg, T.GRAD_GATES[cls][1]), (cls, gl, gg, T.GRAD_GATES[cls])
