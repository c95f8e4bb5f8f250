"""CPU-side conditions of the bit-exact bf16 conv-engine tests: every case of tests/bf16_cases.py is exactly summable (worst-case bound
below 2^24, every generated value a bf16), its blocked outputs exercise the final rounding (>= 10 % rounded, >= 5 % exact ties), the
tap-by-tap arbiter gives the same integers in float32 and float64 and agrees with F.conv3d / autograd, and the launch-geometry claims
of the table hold.  No GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 50000            # voxels (x batch) up to which a case is also compared with F.conv3d / autograd in float64
ALL_OPS = bc.OPS + [bc.default_grid_op(bc.CUS_REF)]


def _voxels(vol, B):
    return B * vol[0] * vol[1] * vol[2]


@pytest.mark.parametrize("op", ALL_OPS, ids=lambda o: o["name"])
def test_conv_cases_are_exact_and_round(op):
    for d, masked in bc.conv_runs(op):
        run = bc.build_run(op, d, masked)
        assert run["bound"] < bc.TWO24
        tensors = [run["x0"], run["w"]] + [t for t in (run["x1"], run["mask"]) if t is not None]
        assert all(bc.is_bf16(t) for t in tensors), (op["name"], d)
        assert -9 <= op["ex"] <= 6 and -9 <= op["ew"] <= 6
        if run["bias"] is not None:
            assert torch.equal(run["bias"].float().double(), run["bias"])
        z32, v32 = bc.run_reference(run, torch.float32)
        z64, v64 = bc.run_reference(run, torch.float64)
        assert torch.equal(z32.double(), z64) and torch.equal(v32, v64)
        unit = 2.0 ** (op["ex"] + op["ew"])
        assert float(z64.abs().max()) <= run["bound"] * unit and torch.equal(z64 / unit, (z64 / unit).round())
        if not run["planar"] and not masked:
            rounded, ties = bc.rounding_shares(v64[:, :run["n_real"]])
            assert rounded >= bc.MIN_ROUNDED and ties >= bc.MIN_TIES, (op["name"], d, rounded, ties)
        if _voxels(run["vol"], run["B"]) <= SMALL:
            wop = run["wop"]
            ref = F.conv3d(bc.virtual_input(run["x0"], run["up0"], run["x1"]), wop.reshape(wop.shape[0], wop.shape[1], 3, 3, 3), padding=1)
            assert torch.equal(ref, z64)
            assert torch.equal(F.conv3d(bc.virtual_input(run["x0"], run["up0"], run["x1"]).float(), wop.reshape(wop.shape[0], wop.shape[1], 3, 3, 3).float(),
                                        padding=1).double(), z64)


@pytest.mark.parametrize("op", [o for o in bc.OPS if _voxels(o["vol"], o["B"]) <= SMALL], ids=lambda o: o["name"])
def test_flipped_operators_are_the_adjoint_by_autograd(op):
    """backward-data of the float64 conv (autograd) against the arbiter on the flipped operator of every segment"""
    x0, x1, w, _ = bc.op_tensors(op)
    X0 = x0.clone().requires_grad_()
    X1 = x1.clone().requires_grad_() if x1 is not None else None
    x = bc.virtual_input(X0, op["up0"], X1)[:, :op["cw_in"]]
    for d in ("flip0", "flip1")[:2 if op["c1"] else 1]:
        run = bc.build_run(op, d, False)
        for t in (X0, X1):
            if t is not None:
                t.grad = None
        dz = run["x0"][:, :op["cout"]]
        F.conv3d(x, w, padding=1).backward(dz, retain_graph=True)
        z, _ = bc.run_reference(run)
        ci_lo, ci_n, _ = run["pack"]
        if d == "flip0" and op["up0"]:
            B, _, D, H, W = z.shape
            got = z[:, :ci_n].reshape(B, ci_n, D // 2, 2, H // 2, 2, W // 2, 2).sum(dim=(3, 5, 7))
            assert torch.equal(got, X0.grad)
        else:
            want = (X0 if d == "flip0" else X1).grad
            assert torch.equal(z[:, :ci_n], want[:, :ci_n]) and float(z[:, ci_n:].abs().max() if z.shape[1] > ci_n else 0.0) == 0.0


@pytest.mark.parametrize("fu", bc.FUSED, ids=lambda f: f["name"])
def test_fused_cases_are_exact_and_round_twice(fu):
    for masked in (False, True):
        fr = bc.build_fused(fu, masked)
        assert fr["bound"] < bc.TWO24 and 8 * fr["bound"] < bc.TWO24 and bc.is_bf16(fr["dz"]) and bc.is_bf16(fr["w"])
        z32, s32 = bc.fused_reference(fr, torch.float32)
        z64, s64 = bc.fused_reference(fr, torch.float64)
        assert torch.equal(z32.double(), z64) and torch.equal(s32, s64)
        if not masked:
            rounded, ties = bc.rounding_shares(z64)
            assert rounded >= bc.MIN_ROUNDED and ties >= bc.MIN_TIES
            assert bc.rounding_shares(s64)[0] >= 0.40                         # the 2 x 2 x 2 sums need a rounding again
        if _voxels(fu["vol"], fu["B"]) <= SMALL:
            # the flipped operator on segment 0 is backward-data of Conv3d(cup + 16 -> cdz) onto its first cup input channels
            X = torch.zeros((fu["B"], fu["cup"] + 16) + fu["vol"], dtype=torch.float64, requires_grad=True)
            F.conv3d(X, fr["w"], padding=1).backward(fr["dz"])
            assert torch.equal(X.grad[:, :fu["cup"]], z64)


def test_impulse_expectation_is_the_rounded_weight_of_the_matching_tap():
    pos = bc.impulse_positions(32)
    assert len(set(pos)) == 32
    for a in range(32):
        for b in range(a):
            assert max(abs(pos[a][k] - pos[b][k]) for k in range(3)) >= 3          # the 3 x 3 x 3 boxes do not meet
    D, H, W = bc.IMPULSE_VOL
    assert (0, 0, 0) in pos[:16] and (D - 1, H - 1, W - 1) in pos[:16] and any(0 < d < D - 1 and 0 < h < H - 1 and 0 < w < W - 1 for d, h, w in pos[:16])
    for cout, cin in bc.IMPULSE_OPS:
        w = bc.impulse_weights(cout, cin)
        wr = bc.rne(w).float()
        assert not bc.is_bf16(w) and float((wr != w).float().mean()) > 0.9
        assert (w == 1 + 2.0 ** -8).any() and (w == 1 + 3 * 2.0 ** -8).any() and (w == 2 - 2.0 ** -10).any()
        assert float(bc.rne(torch.tensor(1 + 2.0 ** -8))) == 1.0 and float(bc.rne(torch.tensor(1 + 3 * 2.0 ** -8))) == 1 + 2.0 ** -6
        assert float(bc.rne(torch.tensor(2 - 2.0 ** -10))) == 2.0
        w27 = wr.reshape(cout, cin, 27)
        assert float((w27 != w27.flip(2))[:, :, :13].float().mean()) > 0.95                 # asymmetric taps, after the rounding too
        for flip in (False, True):
            x, want, _ = bc.impulse_case(cout, cin, flip)
            wop = bc.wop_flipped(wr.double(), 0, cin) if flip else bc.wop_forward(wr.double(), 0, cin)
            assert torch.equal(bc.conv_taps(x, wop), want)
            boxes = sum(len([1 for t in range(27) if 0 <= p[0] + t // 9 - 1 < D and 0 <= p[1] + (t // 3) % 3 - 1 < H and 0 <= p[2] + t % 3 - 1 < W])
                        for p in pos[:cout if flip else cin])
            assert int((want[0].abs().sum(0) != 0).sum()) == boxes                 # the clipped 3 x 3 x 3 boxes and zero elsewhere


@pytest.mark.parametrize("c", bc.WGRAD, ids=lambda c: c["name"])
def test_weight_gradient_cases_are_exact(c):
    assert bc.wgrad_bound(c) < bc.TWO24
    x0, x1, dz = bc.wgrad_tensors(c)
    assert all(bc.is_bf16(t) for t in (x0, dz)) and (x1 is None or bc.is_bf16(x1))
    gw32, gb32 = bc.wgrad_reference(c, torch.float32)
    gw64, gb64 = bc.wgrad_reference(c, torch.float64)
    assert torch.equal(gw32.double(), gw64) and torch.equal(gb32.double(), gb64)
    unit = 2.0 ** (c["ex"] + c["edz"])
    assert float(gw64.abs().max()) <= bc.wgrad_bound(c) * unit and float(gw64.abs().max()) > 0
    if _voxels(c["vol"], c["B"]) <= SMALL:
        X0 = x0.clone().requires_grad_()
        x = bc.virtual_input(X0, c["up0"], x1)
        Wt = torch.zeros((c["cdz"], c["c0"] + c["c1"], 3, 3, 3), dtype=torch.float64, requires_grad=True)
        b = torch.zeros(c["cdz"], dtype=torch.float64, requires_grad=True)
        F.conv3d(x, Wt, b, padding=1).backward(dz)
        assert torch.equal(Wt.grad[:c["cout_w"], :c["cin_w"]], gw64) and torch.equal(b.grad[:c["cout_w"]], gb64)


def test_geometry_claims_of_the_table():
    geo = {}
    for op in ALL_OPS:
        for d, m in bc.conv_runs(op):
            run = bc.build_run(op, d, m)
            geo[(op["name"], d)] = bc.conv_geometry(run["C0"] + run["C1"], run["cout"], run["vol"], run["B"], run["planar"])
    for op in ALL_OPS:
        if op["multi"]:
            assert geo[(op["name"], "fwd")]["ntiles"] >= 64, op["name"]
    assert [geo[(n, "fwd")]["ntiles"] for n in ("mt_16_16", "mt_16_32_odd", "mt_q3", "mt_q1", "mt_head_3")] == [64, 150, 64, 64, 64]
    assert geo[("mt_16_32_odd", "fwd")]["ntiles"] % 8 != 0 and geo[("mt_16_32_odd", "flip0")]["ntiles"] == 120
    assert geo[("mt_q3", "fwd")]["Q"] == 3 and geo[("mt_q3", "fwd")]["NCT"] == 2 and geo[("mt_q1", "fwd")]["Q"] == 1 and geo[("mt_q1", "fwd")]["NCT"] == 2
    # the walk-back flag under a multi-tile walk of a FLIPPED operator: these flips keep >= 64 tiles
    assert all(geo[(n, "flip0")]["ntiles"] >= 64 for n in ("mt_16_16", "mt_16_32_odd", "mt_q3", "mt_head_3", "mt_default_grid"))
    assert bc.default_grid_w(256) == 160 and geo[("mt_default_grid", "fwd")]["ntiles"] == 640 >= 2 * 256 + 64
    assert geo[("two_groups", "fwd")] == dict(NCT=2, ROWS=6, ntiles=4, Q=1, G=2) and geo[("two_groups", "flip0")]["Q"] == 3
    assert geo[("two_chunks", "fwd")]["Q"] == 2 and geo[("two_chunks", "fwd")]["ntiles"] == 1
    assert geo[("three_chunks", "fwd")]["Q"] == 3 and geo[("six_rows", "fwd")] == dict(NCT=2, ROWS=6, ntiles=3, Q=1, G=1)
    assert all(geo[(o["name"], d)]["ntiles"] < 64 for o in bc.OPS if not o["multi"] for d, _ in bc.conv_runs(o))
    fg = bc.FUSED_BY_NAME["fu_mt_32_32"]
    assert bc.conv_geometry(fg["cdz"], fg["cup"], fg["vol"], fg["B"])["ntiles"] == 64
    # weight gradient: every small case has one tile per depth segment; the two big ones reach the ring and the round-robin task order
    for c in bc.WGRAD:
        D, H, W = c["vol"]
        nblk, nseg, seg_len = bc.bwb_tasks((c["c0"] + c["c1"]) // 16, c["B"], D, H, W, 256)
        if c["big"]:
            assert (nblk, nseg, seg_len) == bc.WGRAD_TASKS_256[c["name"]]
        else:
            assert seg_len == 1
    assert bc.WGRAD_TASKS_256 == {"wg_ring": (85, 6, 4), "wg_task_rr": (256, 16, 4)}
    ring = bc.WGRAD_BY_NAME["wg_ring"]
    assert 85 % 8 != 0 and ring["vol"][0] % 2 == 1 and 128 ** 3 >= 1 << 21 and 256 % 8 == 0
    assert bc.workspace_nblk(85 * 3 * 2 * 28 * 32 * 16 * 4, 3, 2) == 85


def test_elementwise_references():
    """the plain references of the pool / upsample kernels against ATen where ATen defines the operation"""
    for vol in ((5, 7, 9), (4, 6, 8)):
        x = bc.pool_inputs(vol)
        assert torch.isnan(x).any()
        m, arg = bc.maxpool_reference(x)
        ref, idx = F.max_pool3d(x, 2, return_indices=True)
        assert bc.same_or_both_nan(m, ref)
        D, H, W = vol
        k = arg
        d2, h2, w2 = torch.meshgrid(torch.arange(D // 2), torch.arange(H // 2), torch.arange(W // 2), indexing="ij")
        flat = ((2 * d2 + ((k >> 2) & 1)) * H + 2 * h2 + ((k >> 1) & 1)) * W + 2 * w2 + (k & 1)
        assert torch.equal(flat, idx)                                              # the same arg-max, ties and NaN included
    x = bc.pool_inputs((4, 6, 8), nan_every=0)                               # no NaN: autograd routes the gradient
    assert not torch.isnan(x).any()
    X = x.double().requires_grad_()
    gp = bc.ints(np.random.default_rng(0), (2, 16, 2, 3, 4), 5, 0)
    F.max_pool3d(X, 2).backward(gp)
    assert torch.equal(bc.maxpool_bwd_reference(x, gp, None, 1.0).double(), X.grad)
    s = bc.special_f32()
    assert torch.isnan(s).sum() == 6 and torch.isinf(s).sum() == 2 and torch.isinf(s.to(bc.BF).float()).sum() == 6
    m = bc.mask_values((2, 16, 3, 3, 3), "t")
    assert torch.isnan(m).any() and ((m == 0) & torch.signbit(m)).any() and ((m == 0) & ~torch.signbit(m)).any()
    assert float(bc.lrelu_grad(torch.tensor([float("nan"), -0.0, 0.0, 1.0]), 0.2).sum()) == np.float32(0.2) * 3 + 1


def test_cases_file_is_what_the_table_computes():
    with open(os.path.join(ROOT, "profiles", "pr09_bf16_cases_cpu.txt")) as f:
        recorded = f.read().splitlines()
    assert recorded == bc.report_lines()
    for line in recorded:
        if line.startswith(("conv", "fused", "wgrad")):
            assert int(line.split("bound")[1].split()[0]) < bc.TWO24
