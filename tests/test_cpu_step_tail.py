"""The arbiters and the gates of tests/test_gpu_step_tail.py, checked without a GPU: the float64 Adam recurrence the kernel is judged by IS
torch.optim.Adam, the oracle's explicit update agrees with it, the case table holds what it promises, and every gate constant of the GPU
test file is a `4 x measured` line of profiles/pr03_step_tail_gates_cpu.txt (the output of tools/step_tail_gates.py)."""
import os

import numpy as np
import torch

from oracle import vxm_oracle as orc

import step_tail_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adam_arbiter_is_torch_adam_in_float64_and_the_explicit_oracle_agrees():
    n = 4099
    p0, g, _, _ = sc.adam_arrays(n)
    for hyper in sc.ADAM_HYPER:
        for gscale in sc.ADAM_GSCALE:
            # unrounded doubles on both sides (gscale is applied to the gradients beforehand: adam_torch would round it)
            gs = (g.astype(np.float64) * gscale)
            mine = sc.adam_arbiter(p0, gs, hyper, 1.0, check=sc.ADAM_CHECK, rounded=False)
            ref = sc.adam_torch(p0, gs, hyper, 1.0, torch.float64, check=sc.ADAM_CHECK)
            p, m, v = (torch.from_numpy(np.asarray(a, np.float64)) for a in (p0, np.zeros(n), np.zeros(n)))
            for k in range(sc.ADAM_K):
                p, m, v = orc.adam_step_explicit(p, torch.from_numpy(gs[k]), m, v, k + 1, *hyper)
                if k + 1 in sc.ADAM_CHECK:
                    for a, b, c in zip(mine[k + 1], ref[k + 1], (p, m, v)):
                        assert sc.rel_l2(a, b) < 1e-12 and sc.rel_l2(c.numpy(), a) < 1e-12
                    assert float(np.abs(mine[k + 1][0] - ref[k + 1][0]).max()) / hyper[0] < 1e-10
    # the late start: moments and counter taken over
    L = sc.ADAM_LATE
    p0, g, m0, v0 = sc.adam_arrays(L["n"], L["steps"], late=True)
    hyper, steps = sc.ADAM_HYPER[L["hyper"]], tuple(range(1, L["steps"] + 1))
    mine = sc.adam_arbiter(p0, g, hyper, 1.0, m0, v0, L["start"], steps, rounded=False)
    ref = sc.adam_torch(p0, g.astype(np.float64), hyper, 1.0, torch.float64, m0, v0, L["start"], steps)
    for s in steps:
        for a, b in zip(mine[s], ref[s]):
            assert sc.rel_l2(a, b) < 1e-12
    # rounding the hyper-parameters as the ABI does moves exp_avg_sq by ~1e-5: the arbiter of the kernel is not torch's fp64 Adam
    rounded = sc.adam_arbiter(p0, g, hyper, 1.0, m0, v0, L["start"], steps)
    assert 1e-7 < sc.rel_l2(rounded[1][2] - v0, mine[1][2] - v0) < 1e-4


def test_step_tail_case_table():
    for n in sc.ADAM_N:
        p0, g, _, _ = sc.adam_arrays(n)
        zero = sc.adam_zero_mask(n)
        assert g.shape == (sc.ADAM_K, n) and p0.dtype == g.dtype == np.float32
        assert not g[:, zero].any() and int(zero.sum()) == n // sc.ADAM_ZERO_EVERY
        mag = np.abs(g[:, ~zero])
        assert mag.size == 0 or (1e-12 <= float(mag.min()) and float(mag.max()) <= 10.0)
    assert sc.ADAM_N[-1] == 327331 and sc.ADAM_K == 25 and set((1, 2, 3, sc.ADAM_K)) == set(sc.ADAM_CHECK)
    p0, g, m0, v0 = sc.adam_arrays(sc.ADAM_LATE["n"], sc.ADAM_LATE["steps"], late=True)
    assert m0.any() and v0.min() >= 0 and v0.any() and len(g) == 3
    # Dice: channel 1 absent, channel 2 positive in both tensors and below the clamp at every V
    for case in sc.DICE_CASES:
        yt, yp = sc.dice_arrays(case)
        assert yt.shape == yp.shape == case and 0 <= yp.min() and yp.max() < 1
        if case[1] > 1:
            assert not yt[:, 1].any() and not yp[:, 1].any()
        if case[1] > 2:
            s = (yt[:, 2].astype(np.float64) + yp[:, 2]).sum(axis=1)
            assert np.all(np.abs(s - sc.DICE_SUBCLAMP_SUM) < 1e-3 * sc.DICE_SUBCLAMP_SUM) and s.max() < sc.DICE_CLAMP
            assert yt[:, 2].min() > 0 and yp[:, 2].min() > 0
        binary = np.delete(yt, 2, axis=1) if case[1] > 2 else yt
        assert set(np.unique(binary)) <= {0.0, 1.0}
    assert sc.MSE_N[-1] > 1024 * 2048 and sc.MSE_N[-1] > 8192 * 256 and sc.DICE_CASES[3][2] > 256 * 256
    img = sc.smooth_image(1)
    assert img.shape == (1, 1) + sc.TRAJ_SHAPE and img.dtype == np.float32 and 0 <= img.min() and img.max() < 1
    assert len(sc.traj_pairs()) == sc.TRAJ_K >= 3
    total, run = sc.combine_reference(np.float32([1, 2]), np.float32([0.5, 0.25]), np.float32([1, 1, 1]))
    assert total == 1.0 and list(run) == [1.5, 1.5, 2.0]
    assert sc.LOSS_TERMS_MAX == int([l.split()[2] for l in open(os.path.join(ROOT, "include", "vxm_hip.h")) if l.startswith("#define VXM_LOSS_TERMS_MAX")][0])


def test_gpu_gates_are_four_times_the_measured_reference_error():
    import test_gpu_step_tail as T
    recorded = {}
    with open(os.path.join(ROOT, "profiles", "pr03_step_tail_gates_cpu.txt")) as f:
        for line in f:
            if line.startswith("GATE "):
                parts = line.split()
                recorded[" ".join(parts[1:-1])] = float(parts[-1])
    used = {"mse loss_rel": T.MSE_LOSS_GATE, "mse grad": T.MSE_GRAD_GATE, "dice loss_abs": T.DICE_LOSS_GATE, "dice grad": T.DICE_GRAD_GATE,
            "trajectory loss_abs": T.TRAJ_LOSS_GATE}
    for (h, s), vals in T.ADAM_GATES.items():
        for what, v in zip(("p_over_lr", "exp_avg", "exp_avg_sq"), vals):
            used["adam %s step%d %s" % (h if h == "late" else "hyper%d" % h, s, what)] = v
    for name, vals in T.TRAJ_GATES.items():
        for what, v in zip(("dp", "exp_avg", "exp_avg_sq"), vals):
            used["trajectory %s %s" % (name, what)] = v
    assert used == recorded
    assert len(T.TRAJ_GATES) == 24 and max(max(v) for v in T.TRAJ_GATES.values()) < 4e-2
    assert set(T.ADAM_GATES) == {(h, s) for h in range(len(sc.ADAM_HYPER)) for s in sc.ADAM_CHECK} | {("late", s) for s in (1, 2, 3)}
    # the floor of a scalar fp32 result
    assert T.MSE_LOSS_GATE >= 4 * 2.0 ** -24 * (1 - 1e-3) and T.TRAJ_LOSS_GATE >= 4 * 2.0 ** -24 * 0.39
