"""The end of the training step against float64: the flat Adam kernel over many steps (both entry points), several optimiser steps of the
whole model against the oracle's loop, and MSE / Dice / the loss combiner / vxm_add2 / vxm_fill_zero / vxm_lrelu_bwd at the edges of
their grids.  Run on the MI355X box: `pytest -m gpu`.

Every gate is 4 x the error of the REFERENCE's own fp32 evaluation of the same operation on the CPU against the float64 arbiter, on the
inputs of tests/step_tail_cases.py (a scalar fp32 result never below 4 x 2^-24 relative); tools/step_tail_gates.py measures them and
profiles/pr03_step_tail_gates_cpu.txt is its output.  The margin of 4 allows another summation order and FMA contraction, no more.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import vxm_oracle as orc

import step_tail_cases as sc        # tests/step_tail_cases.py: the table, shared with test_cpu_step_tail.py and tools/step_tail_gates.py

pytestmark = pytest.mark.gpu

# 4 x the fp32 reference's own error against float64 (the `GATE` lines of profiles/pr03_step_tail_gates_cpu.txt; tests/test_cpu_step_tail.py
# holds the two together).  Measured values, largest over the cases a gate covers (n, gscale):
#   Adam, torch.optim.Adam in fp32 against fp64: after 25 steps max |dp| / lr 8.2e-4 (lr 1e-4) and 8.3e-6 (lr 1e-2), exp_avg 2.7e-7 / 7.3e-8,
#   exp_avg_sq 3.4e-7 / 3.6e-7 (its decay fl32(beta2) against the double's); after one step 7.5e-5 / 9.1e-7, 4.6e-8, 8.6e-8 / 6.2e-8
#   MSE: loss 5.4e-8 relative (the gate is the floor 4 x 2^-24 = 2.4e-7), gradients 7.9e-8
#   Dice: loss 2.1e-8 absolute, gradients 2.7e-7 (the single-voxel case; 1.3e-7 on the others)
#   four steps of the whole model, fp32 oracle against fp64 oracle: loss 4.9e-7, per tensor p_K - p_0 1.0e-5 .. 5.6e-4,
#   exp_avg 2.7e-5 .. 1.2e-3, exp_avg_sq 5.9e-5 .. 1.2e-3 -- every one below 1e-2, so every gate is below 4e-2
ADAM_GATES = {                                  # (hyper set | 'late', step): max |p - p64| / lr, rel-L2 exp_avg, rel-L2 exp_avg_sq
    (0, 1): (2.982e-04, 1.821e-07, 3.452e-07),
    (0, 2): (5.886e-04, 2.380e-07, 4.083e-07),
    (0, 3): (8.542e-04, 2.005e-07, 3.980e-07),
    (0, 25): (3.269e-03, 1.075e-06, 1.347e-06),
    (1, 1): (3.621e-06, 1.821e-07, 2.483e-07),
    (1, 2): (6.499e-06, 2.199e-07, 2.618e-07),
    (1, 3): (9.016e-06, 1.976e-07, 3.127e-07),
    (1, 25): (3.328e-05, 2.906e-07, 1.421e-06),
    ("late", 1): (2.935e-04, 1.201e-07, 1.200e-07),
    ("late", 2): (4.688e-04, 1.613e-07, 2.026e-07),
    ("late", 3): (6.342e-04, 1.707e-07, 2.332e-07),
}
MSE_LOSS_GATE, MSE_GRAD_GATE = 2.384e-07, 3.171e-07
DICE_LOSS_GATE, DICE_GRAD_GATE = 8.595e-08, 1.061e-06
TRAJ_LOSS_GATE = 1.978e-06
TRAJ_GATES = {                                  # tensor: rel-L2 of p_K - p_0, of its slice of exp_avg, of its slice of exp_avg_sq
    "unet_model.encoder.0.0.main.weight": (9.965e-04, 9.783e-04, 1.542e-03),
    "unet_model.encoder.0.0.main.bias": (6.014e-04, 9.023e-04, 1.616e-03),
    "unet_model.encoder.1.0.main.weight": (1.540e-03, 2.280e-03, 2.002e-03),
    "unet_model.encoder.1.0.main.bias": (1.020e-03, 2.068e-03, 1.972e-03),
    "unet_model.encoder.2.0.main.weight": (1.066e-03, 2.291e-03, 2.825e-03),
    "unet_model.encoder.2.0.main.bias": (1.462e-03, 1.477e-03, 1.848e-03),
    "unet_model.encoder.3.0.main.weight": (1.057e-03, 2.751e-03, 4.493e-03),
    "unet_model.encoder.3.0.main.bias": (7.824e-04, 2.932e-03, 4.818e-03),
    "unet_model.decoder.0.0.main.weight": (1.541e-03, 2.988e-03, 4.364e-03),
    "unet_model.decoder.0.0.main.bias": (1.561e-03, 2.673e-03, 4.604e-03),
    "unet_model.decoder.1.0.main.weight": (1.590e-03, 2.917e-03, 3.698e-03),
    "unet_model.decoder.1.0.main.bias": (9.455e-04, 2.618e-03, 4.327e-03),
    "unet_model.decoder.2.0.main.weight": (1.516e-03, 3.342e-03, 3.778e-03),
    "unet_model.decoder.2.0.main.bias": (9.821e-04, 3.018e-03, 3.784e-03),
    "unet_model.decoder.3.0.main.weight": (2.228e-03, 4.079e-03, 2.570e-03),
    "unet_model.decoder.3.0.main.bias": (5.927e-04, 4.854e-03, 3.723e-03),
    "unet_model.remaining.0.main.weight": (1.040e-03, 1.663e-03, 1.152e-03),
    "unet_model.remaining.0.main.bias": (6.368e-04, 1.517e-03, 6.986e-04),
    "unet_model.remaining.1.main.weight": (9.195e-04, 8.612e-04, 8.464e-04),
    "unet_model.remaining.1.main.bias": (4.693e-04, 8.080e-04, 3.370e-04),
    "unet_model.remaining.2.main.weight": (6.024e-04, 1.098e-03, 1.388e-03),
    "unet_model.remaining.2.main.bias": (2.028e-04, 1.027e-03, 6.807e-04),
    "flow.weight": (1.323e-04, 2.835e-04, 4.919e-04),
    "flow.bias": (4.085e-05, 1.079e-04, 2.342e-04),
}


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


rel_l2 = sc.rel_l2


def gate(what, measured, bound):
    """Assert measured < bound and print the margin (`pytest -s` / the committed GPU log shows how tight the gate is)."""
    print("[gate] %-58s measured %.3e  bound %.1e" % (what, measured, bound))
    assert measured < bound, "%s: %.3e >= %.1e" % (what, measured, bound)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def call(name, *args):
    from voxelmorph_amd import _lib
    _lib.call(name, *(args + (_lib.stream(),)))


class Buf:
    """`data` on the device with `off` floats of sentinel in front of it (off = 1: a pointer that is 4-byte aligned only) and 64 behind"""

    def __init__(self, data, off=0):
        data = np.asarray(data, np.float32).ravel()
        host = np.full(off + data.size + sc.SENTINELS, sc.SENTINEL, np.float32)
        host[off:off + data.size] = data
        self.t, self.off, self.n = torch.from_numpy(host).cuda(), off, data.size

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.off

    @property
    def data(self):
        return self.t[self.off:self.off + self.n]

    def get(self):
        return N(self.data)

    def intact(self):
        return bool((self.t[:self.off] == float(sc.SENTINEL)).all()) and bool((self.t[self.off + self.n:] == float(sc.SENTINEL)).all())


def empty(n, off=0):
    return Buf(np.full(n, sc.SENTINEL, np.float32), off)


# ------------------------------------------------------------------ 1. the Adam kernel, both entry points, many steps
_ADAM_IN = {}


def _adam_inputs(n, late):
    """host arrays and the gradients on the device, once per size"""
    if (n, late) not in _ADAM_IN:
        p0, g, m0, v0 = sc.adam_arrays(n, sc.ADAM_LATE["steps"] if late else sc.ADAM_K, late=late)
        _ADAM_IN[(n, late)] = (p0, g, m0, v0, torch.from_numpy(g).cuda())
    return _ADAM_IN[(n, late)]


def _adam_run(entry, n, h, gscale, off=0, late=False):
    p0, g, m0, v0, g_dev = _adam_inputs(n, late)
    hyper = sc.ADAM_HYPER[h]
    start = sc.ADAM_LATE["start"] if late else 0
    steps = len(g)
    check = tuple(range(1, steps + 1)) if late else sc.ADAM_CHECK
    want = sc.adam_arbiter(p0, g, hyper, gscale, m0, v0, start, check)
    zero = sc.adam_zero_mask(n)
    p, gb = Buf(p0, off), empty(n, off)
    m, v = Buf(np.zeros(n) if m0 is None else m0, off), Buf(np.zeros(n) if v0 is None else v0, off)
    state = torch.zeros(2, dtype=torch.int64, device="cuda")             # VXM_ADAM_STATE_BYTES, the counter at offset 0
    state[0] = start
    tag = "%s n=%d hyper%d gscale=%.3g%s%s" % (entry[4:], n, h, gscale, " +1 float" if off else "", " from %d" % start if late else "")
    for k in range(steps):
        gb.data.copy_(g_dev[k])
        if entry == "vxm_adam_step":
            call(entry, p.ptr, gb.ptr, m.ptr, v.ptr, n, hyper[0], hyper[1], hyper[2], hyper[3], start + k + 1, float(gscale))
        else:
            call(entry, p.ptr, gb.ptr, m.ptr, v.ptr, n, hyper[0], hyper[1], hyper[2], hyper[3], state.data_ptr(), float(gscale))
        assert p.intact() and gb.intact() and m.intact() and v.intact(), "%s: step %d wrote outside its %d elements" % (tag, k + 1, n)
        if k + 1 in check:
            got = (p.get(), m.get(), v.get())
            ep, em, ev = sc.adam_errors(got, want[k + 1], hyper[0])
            bp, bm, bv = ADAM_GATES[("late" if late else h, k + 1)]
            gate("%s step %d max|dp|/lr" % (tag, k + 1), ep, bp)
            gate("%s step %d exp_avg" % (tag, k + 1), em, bm)
            gate("%s step %d exp_avg_sq" % (tag, k + 1), ev, bv)
            # a gradient that is 0 on every step leaves the parameter alone, bit for bit
            assert same_bits(got[0][zero], p0[zero])
            if not late:
                assert not got[1][zero].any() and not got[2][zero].any()
    if entry == "vxm_adam_step_dev":
        assert int(state[0].item()) == start + steps


@pytest.mark.parametrize("n", sc.ADAM_N)
@pytest.mark.parametrize("entry", ["vxm_adam_step", "vxm_adam_step_dev"])
def test_adam_kernel_vs_fp64_recurrence(vxm, entry, n):
    """25 steps from zero state, both hyper-parameter sets, gscale 1, 1/2, 1/3: p, exp_avg and exp_avg_sq after steps 1, 2, 3 and 25
    against the float64 recurrence with the hyper-parameters as the ABI rounds them"""
    for h in range(len(sc.ADAM_HYPER)):
        for gscale in sc.ADAM_GSCALE:
            _adam_run(entry, n, h, gscale)


@pytest.mark.parametrize("entry", ["vxm_adam_step", "vxm_adam_step_dev"])
def test_adam_kernel_late_start_and_unaligned_pointers(vxm, entry):
    """non-zero moments with the counter at 1000 (bias corrections near 1 and far from the first steps'), and one case with every
    pointer advanced by one float (the ABI asks for 4-byte alignment only)"""
    L = sc.ADAM_LATE
    _adam_run(entry, L["n"], L["hyper"], L["gscale"], late=True)
    c = sc.ADAM_OFFSET_CASE
    _adam_run(entry, c["n"], c["hyper"], c["gscale"], off=1)


# ------------------------------------------------------------------ 2. several optimiser steps of the whole model
_TRAJ_REF = []


def _traj_reference():
    """the float64 oracle's four steps: computed once, shared by the three variants, never modified"""
    if not _TRAJ_REF:
        import os
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        _TRAJ_REF.append(sc.traj_oracle(torch.float64))
    return _TRAJ_REF[0]


@pytest.mark.parametrize("mode", ["capturable", "host_counter", "graph"])
def test_four_optimiser_steps_vs_fp64_oracle(vxm, mode):
    """VxmDense 32^3 (int_steps 3), NCC + Grad('l2', x2) through the loss combiner, FlatAdam(lr 1e-3), a new smooth pair per step: the
    loss of every step, and after step 4 the movement of each of the 24 parameter tensors and its slices of exp_avg and exp_avg_sq,
    against the float64 oracle with torch.optim.Adam.  The moments are non-zero when steps 2 .. 4 use them.  graph: one eager step,
    the capture, three replays."""
    from voxelmorph_amd.graph import GraphedStep
    from voxelmorph_amd.optim import FlatAdam
    losses64, ref = _traj_reference()
    sd = orc.seeded_state_dict(sc.TRAJ_SHAPE, seed=sc.TRAJ_SEED, flow_std=sc.TRAJ_FLOW_STD)
    model = vxm.networks.VxmDense(sc.TRAJ_SHAPE, int_steps=sc.TRAJ_INT_STEPS, int_downsize=sc.TRAJ_INT_DOWNSIZE)
    res = model.load_state_dict(sd, strict=False)
    assert all(k.endswith(".grid") for k in res.missing_keys) and not res.unexpected_keys
    model = model.cuda()
    opt = FlatAdam(model, lr=sc.TRAJ_LR, capturable=mode != "host_counter")
    p0 = opt.flat_param.clone()
    src, trg = (torch.empty((1, 1) + sc.TRAJ_SHAPE, device="cuda") for _ in range(2))
    ncc, reg = vxm.losses.NCC().loss, vxm.losses.Grad("l2", loss_mult=2).loss

    def fwd():
        y, pre = model(src, trg)
        return vxm.losses.weighted_sum([ncc(trg, y), reg(None, pre)], [1.0, 1.0])
    step = GraphedStep(fwd, opt, eager_steps=1, enabled=mode == "graph")
    losses = []
    for s, t in sc.traj_pairs():
        src.copy_(G(s))
        trg.copy_(G(t))
        losses.append(float(step().detach()))
    torch.cuda.synchronize()
    assert opt.step_count == sc.TRAJ_K
    if mode == "graph":
        assert step.graph is not None and step.replays == sc.TRAJ_K - 1, step.capture_error
    for k in range(sc.TRAJ_K):
        gate("%s step %d loss (absolute)" % (mode, k + 1), abs(losses[k] - losses64[k]), TRAJ_LOSS_GATE)
    named = [(name, p) for name, p in model.named_parameters() if p.requires_grad]
    assert len(named) == 24 and [id(p) for _, p in named] == [id(p) for p in opt.params] and set(n for n, _ in named) == set(ref) == set(TRAJ_GATES)
    dp, m, v = N(opt.flat_param.double() - p0.double()), N(opt.exp_avg), N(opt.exp_avg_sq)
    off, failed = 0, []
    for name, p in named:
        sl = slice(off, off + p.numel())
        off += p.numel()
        for what, got, want, bound in zip(("p_K - p_0", "exp_avg", "exp_avg_sq"), (dp[sl], m[sl], v[sl]), ref[name], TRAJ_GATES[name]):
            e = rel_l2(got, want.ravel())
            print("[gate] %-58s measured %.3e  bound %.1e" % ("%s %s %s" % (mode, name, what), e, bound))
            if not e < bound:
                failed.append((name, what, e, bound))
    assert off == opt.n
    assert not failed, failed


# ------------------------------------------------------------------ 3. MSE
_MSE_REF = {}


def _mse_case(n):
    if n not in _MSE_REF:
        a, b = sc.mse_arrays(n)
        _MSE_REF[n] = (a, b) + sc.mse_reference(a, b, torch.float64)
    return _MSE_REF[n]


@pytest.mark.parametrize("n", sc.MSE_N)
def test_mse_class_api_vs_fp64(vxm, n):
    a, b, l64, ga64, gb64 = _mse_case(n)
    for need_a, need_b in ((True, False), (False, True), (True, True)):
        ta, tb = G(a, need_a), G(b, need_b)
        loss = vxm.losses.MSE().loss(ta, tb)
        loss.backward()
        tag = "MSE n=%d grad to %s" % (n, "+".join(x for x, y in (("a", need_a), ("b", need_b)) if y))
        gate(tag + " loss (relative)", abs(float(loss.detach()) - l64) / abs(l64), MSE_LOSS_GATE)
        if need_a:
            gate(tag + " ga", rel_l2(N(ta.grad), ga64), MSE_GRAD_GATE)
        if need_b:
            gate(tag + " gb", rel_l2(N(tb.grad), gb64), MSE_GRAD_GATE)
        assert (ta.grad is None) == (not need_a) and (tb.grad is None) == (not need_b)


@pytest.mark.parametrize("n", sc.MSE_N)
def test_mse_abi_nullable_gradients(vxm, n):
    a, b, l64, ga64, gb64 = _mse_case(n)
    A, B = Buf(a), Buf(b)
    loss, acc, gloss = torch.empty((), device="cuda"), torch.empty(1, dtype=torch.float64, device="cuda"), G(np.ones(1))
    call("vxm_mse_fwd", A.ptr, B.ptr, loss.data_ptr(), acc.data_ptr(), n)
    gate("vxm_mse_fwd n=%d loss (relative)" % n, abs(float(loss.detach()) - l64) / abs(l64), MSE_LOSS_GATE)
    for need_a, need_b in ((False, True), (True, False), (True, True)):
        ga, gb = (empty(n) if need_a else None), (empty(n) if need_b else None)
        call("vxm_mse_bwd", A.ptr, B.ptr, gloss.data_ptr(), ga.ptr if ga else None, gb.ptr if gb else None, n)
        tag = "vxm_mse_bwd n=%d%s" % (n, "" if need_a and need_b else (" gb null" if need_a else " ga null"))
        if ga:
            gate(tag + " ga", rel_l2(ga.get(), ga64), MSE_GRAD_GATE)
            assert ga.intact()
        if gb:
            gate(tag + " gb", rel_l2(gb.get(), gb64), MSE_GRAD_GATE)
            assert gb.intact()
    call("vxm_mse_bwd", A.ptr, B.ptr, gloss.data_ptr(), None, None, n)          # nothing to write: OK, no launch
    torch.cuda.synchronize()
    assert same_bits(A.get(), a) and same_bits(B.get(), b) and A.intact() and B.intact()


# ------------------------------------------------------------------ Dice
_DICE_REF = {}


def _dice_case(case):
    if case not in _DICE_REF:
        yt, yp = sc.dice_arrays(case)
        _DICE_REF[case] = (yt, yp) + sc.dice_reference(yt, yp, torch.float64)
    return _DICE_REF[case]


def _dice_checks(tag, case, yt, yp, gt, gp, gt64, gp64):
    B, C, V = case
    if gt is not None:
        gate(tag + " g_true", rel_l2(gt, gt64), DICE_GRAD_GATE)
    if gp is not None:
        gate(tag + " g_pred", rel_l2(gp, gp64), DICE_GRAD_GATE)
    for g, other in ((gt, yp), (gp, yt)):
        if g is None:
            continue
        if C > 1:               # a label absent from both volumes: the clamp holds the denominator, the numerator is 0 -- no gradient at all
            assert not g[:, 1].any()
        if C > 2:               # below the clamp with a non-zero numerator: 2 y / 1e-5 alone, the clamp passes nothing to the denominator
            want = (-1.0 / (B * C)) * 2.0 * other[:, 2].astype(np.float64) / sc.DICE_CLAMP
            gate(tag + " sub-clamp channel", rel_l2(g[:, 2], want), DICE_GRAD_GATE)


@pytest.mark.parametrize("case", sc.DICE_CASES, ids=lambda c: "B%d-C%d-V%d" % c)
def test_dice_class_api_vs_fp64(vxm, case):
    yt, yp, l64, gt64, gp64 = _dice_case(case)
    tt, tp = G(yt, True), G(yp, True)
    loss = vxm.losses.Dice().loss(tt, tp)
    loss.backward()
    tag = "Dice B=%d C=%d V=%d" % case
    gate(tag + " loss (absolute)", abs(float(loss.detach()) - l64), DICE_LOSS_GATE)
    _dice_checks(tag, case, yt, yp, N(tt.grad), N(tp.grad), gt64, gp64)


@pytest.mark.parametrize("case", sc.DICE_CASES, ids=lambda c: "B%d-C%d-V%d" % c)
def test_dice_abi_nullable_gradients(vxm, case):
    yt, yp, l64, gt64, gp64 = _dice_case(case)
    B, C, V = case
    T, P = Buf(yt), Buf(yp)
    loss, acc, gloss = torch.empty((), device="cuda"), torch.empty(2 * B * C, dtype=torch.float64, device="cuda"), G(np.ones(1))
    call("vxm_dice_fwd", T.ptr, P.ptr, loss.data_ptr(), acc.data_ptr(), B, C, V)
    tag = "vxm_dice B=%d C=%d V=%d" % case
    gate(tag + " loss (absolute)", abs(float(loss.detach()) - l64), DICE_LOSS_GATE)
    for need_t, need_p in ((False, True), (True, False), (True, True)):
        gt, gp = (empty(B * C * V) if need_t else None), (empty(B * C * V) if need_p else None)
        call("vxm_dice_bwd", T.ptr, P.ptr, acc.data_ptr(), gloss.data_ptr(), gt.ptr if gt else None, gp.ptr if gp else None, B, C, V)
        sub = tag + ("" if need_t and need_p else (" g_pred null" if need_t else " g_true null"))
        _dice_checks(sub, case, yt, yp, gt.get().reshape(case) if gt else None, gp.get().reshape(case) if gp else None, gt64, gp64)
        assert (gt is None or gt.intact()) and (gp is None or gp.intact())
    call("vxm_dice_bwd", T.ptr, P.ptr, acc.data_ptr(), gloss.data_ptr(), None, None, B, C, V)
    torch.cuda.synchronize()
    assert T.intact() and P.intact()


def test_dice_refuses_more_rows_than_the_grid_has(vxm):
    """B * C is the grid's y extent: 65535 at the most"""
    from voxelmorph_amd._lib import VxmHipError
    t = torch.zeros((256, 256, 1), device="cuda")
    with pytest.raises(VxmHipError, match="vxm_dice_fwd"):
        vxm.losses.Dice().loss(t, t)


# ------------------------------------------------------------------ loss combiner
def _combine(terms_dev, weights, n, total, running):
    tp = (ctypes.c_void_p * max(n, 1))(*[terms_dev.data_ptr() + 4 * i for i in range(max(n, 1))])
    wv = (ctypes.c_float * max(n, 1))(*[float(w) for w in weights[:max(n, 1)]])
    call("vxm_loss_combine_fwd", ctypes.cast(tp, ctypes.c_void_p), ctypes.cast(wv, ctypes.c_void_p), n, total.data_ptr(),
         running.ptr if running is not None else None)


@pytest.mark.parametrize("with_running", [False, True])
@pytest.mark.parametrize("n", range(1, sc.LOSS_TERMS_MAX + 1))
def test_loss_combiner_exact(vxm, n, with_running):
    """the kernel multiplies and adds in the reference's order without contraction: equal to the float32 loop bit for bit, the running
    sums after two calls included; backward g * w_n"""
    terms, weights = sc.combine_arrays(n)
    T = G(terms)
    total = torch.empty((), device="cuda")
    run0 = np.arange(1, n + 2, dtype=np.float32) * np.float32(0.37)
    running, want_run = (Buf(run0) if with_running else None), (run0 if with_running else None)
    for _ in range(2):
        _combine(T, weights, n, total, running)
        want, want_run = sc.combine_reference(terms, weights, want_run)
        assert same_bits(N(total).reshape(1), np.array([want]))
        if with_running:
            assert same_bits(running.get(), want_run) and running.intact()
    gtotal, gterms = G(np.array([0.7])), empty(n)
    wv = (ctypes.c_float * n)(*[float(w) for w in weights])
    call("vxm_loss_combine_bwd", gtotal.data_ptr(), ctypes.cast(wv, ctypes.c_void_p), n, gterms.ptr)
    assert same_bits(gterms.get(), np.float32(0.7) * weights) and gterms.intact()


@pytest.mark.parametrize("n", [0, sc.LOSS_TERMS_MAX + 1])
def test_loss_combiner_refuses_term_counts_out_of_range(vxm, n):
    from voxelmorph_amd._lib import VxmHipError
    terms, weights = sc.combine_arrays(sc.LOSS_TERMS_MAX + 1)
    T, total, gterms = G(terms), torch.empty((), device="cuda"), empty(sc.LOSS_TERMS_MAX + 1)
    with pytest.raises(VxmHipError, match="vxm_loss_combine_fwd"):
        _combine(T, weights, n, total, None)
    wv = (ctypes.c_float * len(weights))(*[float(w) for w in weights])
    with pytest.raises(VxmHipError, match="vxm_loss_combine_bwd"):
        call("vxm_loss_combine_bwd", G(np.ones(1)).data_ptr(), ctypes.cast(wv, ctypes.c_void_p), n, gterms.ptr)
    torch.cuda.synchronize()
    assert gterms.intact() and not (gterms.get() != sc.SENTINEL).any()


# ------------------------------------------------------------------ vxm_add2, vxm_fill_zero, vxm_lrelu_bwd
@pytest.mark.parametrize("offs", [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], ids=lambda o: "a+%d_b+%d_out+%d" % o)
@pytest.mark.parametrize("n", sc.ADD2_N)
def test_add2_bit_exact_with_tail_and_unaligned_pointers(vxm, n, offs):
    """16-byte lanes where all three pointers allow them, scalars otherwise and for the n % 4 tail: a + b, nothing past n"""
    rng = np.random.default_rng(3600 + n % 1000)
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    A, B, O = Buf(a, offs[0]), Buf(b, offs[1]), empty(n, offs[2])
    call("vxm_add2", A.ptr, B.ptr, O.ptr, n)
    assert same_bits(O.get(), a + b)
    assert O.intact() and A.intact() and B.intact()


@pytest.mark.parametrize("nbytes", sc.FILL_BYTES)
def test_fill_zero_touches_its_bytes_only(vxm, nbytes):
    n = nbytes // 4
    buf = Buf(np.arange(1, n + 1, dtype=np.float32), off=sc.SENTINELS)
    call("vxm_fill_zero", buf.ptr, nbytes)
    torch.cuda.synchronize()
    assert buf.intact() and same_bits(buf.get(), np.zeros(n, np.float32))


def test_lrelu_bwd_batch_strides_that_differ(vxm):
    """the views the fused backward hands it: g, y and dz each with its own batch stride, all larger than C * V.  At y == 0 the derivative
    is the slope (vxm_lrelu_grad: y > 0 ? 1 : slope) -- ATen's choice as well, checked here against F.leaky_relu's backward on the CPU."""
    c = sc.LRELU_CASE
    B, CV, slope = c["B"], c["C"] * c["V"], c["slope"]
    rng = np.random.default_rng(3700)
    x = rng.standard_normal((B, CV)).astype(np.float32)
    x[:, ::5] = 0.0
    x[0, 5] = -0.0
    g = rng.standard_normal((B, CV)).astype(np.float32)
    want = g * np.where(x > 0, np.float32(1.0), np.float32(slope))
    xt = torch.from_numpy(x).requires_grad_()
    yt = torch.nn.functional.leaky_relu(xt, slope)
    yt.backward(torch.from_numpy(g))
    assert same_bits(xt.grad.numpy(), want)                      # the reference's derivative at 0 is the slope
    y = yt.detach().numpy()                                      # what the kernel sees: the activation's OUTPUT (same sign, same zeros)

    def strided(data, pad):
        host = np.full((B, CV + pad), sc.SENTINEL, np.float32)
        host[:, :CV] = data
        return Buf(host), CV + pad
    (Gb, gs), (Yb, ys), (Db, ds) = strided(g, c["pad"][0]), strided(y, c["pad"][1]), strided(np.full((B, CV), sc.SENTINEL), c["pad"][2])
    assert len({gs, ys, ds}) == 3 and min(gs, ys, ds) > CV
    from voxelmorph_amd import _lib
    _lib.call("vxm_lrelu_bwd", Gb.ptr, gs, Yb.ptr, ys, Db.ptr, ds, float(slope), B, c["C"], c["V"], _lib.stream())
    dz = Db.get().reshape(B, ds)
    assert same_bits(dz[:, :CV], want)
    assert not (dz[:, CV:] != sc.SENTINEL).any() and Db.intact() and Gb.intact() and Yb.intact()
