"""The loss kernels of voxelmorph_amd/csrc/losses.hip that produce the headline loss -- the NCC family (k_ncc_fused_fwd / bwd<1..4>, the generic
separable passes, the any-window passes) and the four Grad kernels (k_gradloss_fwd / fwd_v4 / bwd / bwd_v4) -- through losses.NCC / losses.Grad
against float64 arbiters (oracle.ncc_explicit_win; oracle.grad_loss in float64 with autograd) on the table of tests/loss_cases.py: volumes that
are all halo, tile and segment edges, the XCD column remap, the value regimes in which the variance cancels, the second grid-stride pass, NaN /
Inf voxels.  Run on the MI355X box: `pytest -m gpu tests/test_gpu_losses.py -s` prints the margin of every gate.

A class is (value regime x window) for NCC, (penalty x value regime) for Grad.  Its gate is 4 x the worst error of the REFERENCE's own fp32
evaluation against the same arbiter on the same inputs (tools/loss_gates.py, output committed as profiles/pr05_loss_gates_cpu.txt;
tests/test_cpu_losses.py compares the literals below with it); a scalar loss is never gated below 4 x 2^-24; the well-conditioned classes are
capped by the fixed gates of test_gpu_parity.py.  A bound of 0 (window 1: the reference is exact) is met by an error of 0: gates are `<=`."""
import numpy as np
import pytest
import torch

import loss_cases as lc

pytestmark = pytest.mark.gpu

# tools/loss_gates.py: class -> (|loss - arbiter|, gradients: rel-L2, or max-abs in the same/*, single/*, single1d/* and */1 classes)
NCC_GATES = {
    "anti/11": (2.394e-07, 9.555e-05), "anti/3": (2.384e-07, 7.168e-05), "anti/9": (2.384e-07, 9.447e-05), "anti/9x9x5": (2.390e-07, 3.070e-05),
    "lowdim/11": (2.500e-07, 5.735e-06), "lowdim/9": (2.500e-07, 5.585e-06),
    "offset/11": (5.772e-02, 1.299e+00), "offset/3": (2.999e-03, 7.267e-02), "offset/9": (5.432e-02, 9.356e-01),
    "offset/9x9x5": (9.498e-03, 3.507e-01),
    "plateau/11": (2.805e-01, 1.114e+01), "plateau/3": (2.384e-07, 3.631e-06), "plateau/9": (1.094e-01, 4.661e-01),
    "plateau/9x9x5": (1.740e-02, 4.513e-02),
    "ramp/11": (6.176e-06, 1.145e-03), "ramp/3": (4.975e-06, 4.590e-03), "ramp/9": (2.381e-05, 2.580e-03), "ramp/9x9x5": (3.448e-05, 1.256e-03),
    "same/11": (2.384e-07, 9.306e-10), "same/3": (2.384e-07, 1.850e-09), "same/9": (2.384e-07, 9.334e-10), "same/9x9x5": (2.384e-07, 9.489e-10),
    "signed/11": (3.987e-07, 5.135e-06), "signed/3": (2.942e-07, 8.503e-07), "signed/9": (2.959e-07, 3.652e-06),
    "signed/9x9x5": (2.384e-07, 2.801e-06),
    "single/3": (2.666e-07, 1.343e-06), "single/9": (2.384e-07, 6.484e-07), "single1d/9": (2.384e-07, 6.558e-07),
    "uniform/1": (2.384e-07, 0.000e+00), "uniform/11": (2.500e-07, 2.500e-06), "uniform/13": (2.500e-07, 2.500e-06),
    "uniform/3": (2.500e-07, 2.500e-06), "uniform/3x11x11": (2.500e-07, 2.500e-06), "uniform/4x6x8": (2.500e-07, 2.500e-06),
    "uniform/5": (2.500e-07, 2.500e-06), "uniform/7": (2.500e-07, 2.500e-06), "uniform/9": (2.500e-07, 2.500e-06),
    "uniform/9x9x5": (2.384e-07, 2.500e-06),
    "x255/11": (2.500e-07, 2.500e-06), "x255/3": (2.384e-07, 2.500e-06), "x255/9": (2.500e-07, 2.500e-06), "x255/9x9x5": (2.384e-07, 2.500e-06),
    "zerobg/11": (2.500e-07, 2.500e-06), "zerobg/3": (2.384e-07, 2.472e-06), "zerobg/9": (2.384e-07, 2.500e-06),
    "zerobg/9x9x5": (2.384e-07, 2.500e-06),
}
# tools/loss_gates.py: class -> (|loss - arbiter| / |arbiter|, gradient rel-L2)
GRAD_GATES = {
    "l1/normal": (4.341e-07, 3.394e-07), "l1/ties": (2.384e-07, 2.300e-07),
    "l2/normal": (3.366e-07, 2.838e-07), "l2/ties": (2.384e-07, 2.625e-07), "l2/big": (3.895e-07, 2.840e-07),
}
FLOOR = lc.MARGIN * lc.HALF_ULP


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


def gate(what, measured, bound):
    """Assert measured <= bound and print the margin (`pytest -s` / the committed GPU log shows how tight the gate is)."""
    print("[gate] %-78s measured %.3e  bound %.3e" % (what, measured, bound))
    assert measured <= bound, "%s: %.3e > %.3e" % (what, measured, bound)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def bad(a):
    return ~np.isfinite(a)


def same_set(what, got, want):
    assert np.array_equal(bad(got), bad(want)), "%s: %d non-finite voxels %s, the reference's %d %s" % (
        what, bad(got).sum(), np.argwhere(bad(got))[:8].tolist(), bad(want).sum(), np.argwhere(bad(want))[:8].tolist())


def up_tensor(up):
    return torch.tensor(up, dtype=torch.float32, device="cuda")


def ncc_run(vxm, I, J, win, up=1.0):
    """(loss, dJ, dI) of losses.NCC with upstream gradient `up`"""
    Ig, Jg = G(I, True), G(J, True)
    l = vxm.losses.NCC(win=list(win)).loss(Ig, Jg)
    l.backward(up_tensor(up))
    torch.cuda.synchronize()
    return float(l.detach()), N(Jg.grad), N(Ig.grad)


def grad_run(vxm, y, pen, mult=None, up=1.0):
    """(loss, dy) of losses.Grad; `y` a numpy array or a device tensor (used as it is: the unaligned view)"""
    yg = G(y, True) if isinstance(y, np.ndarray) else y.detach().requires_grad_()
    l = vxm.losses.Grad(pen, loss_mult=mult).loss(None, yg)
    l.backward(up_tensor(up))
    torch.cuda.synchronize()
    return float(l.detach()), N(yg.grad)


# ------------------------------------------------------------------ NCC
@pytest.mark.parametrize("row", lc.NCC_ROWS, ids=lc.NCC_IDS)
def test_ncc_every_row_vs_fp64(vxm, row):
    """losses.NCC on every row of the table, with upstream gradient 1 and -0.37: the loss, dJ AND dI against oracle.ncc_explicit_win under the
    gates of the row's class; two calls give bit-identical gradients (no atomics there) and a loss within the floor of its final rounding (the
    fp64 block sums meet in atomics).  What a row is named for -- which kernels it takes, the remap, the segments -- is proved by arithmetic in
    tests/test_cpu_losses.py."""
    name, B, vol, win, regime = row
    I, J = lc.ncc_arrays(row)
    l64, gJ, gI = lc.ncc_arbiter(I, J, win)
    gl, gg = NCC_GATES[lc.ncc_class(row)]
    err = lc.max_abs if lc.by_maxabs(row) else lc.rel_l2
    for up in lc.UPSTREAM:
        l, dJ, dI = ncc_run(vxm, I, J, win, up)
        tag = "ncc %s up %+.2f" % (name, up)
        gate(tag + " loss vs fp64", abs(l - l64), gl)
        gate(tag + " dJ vs fp64", err(dJ, up * gJ), gg * (abs(up) if lc.by_maxabs(row) else 1.0))
        gate(tag + " dI vs fp64", err(dI, up * gI), gg * (abs(up) if lc.by_maxabs(row) else 1.0))
    l2, dJ2, dI2 = ncc_run(vxm, I, J, win, up)
    assert same_bits(dJ, dJ2) and same_bits(dI, dI2), name + ": two calls give different gradient bits"
    gate("ncc %s loss of a second call" % name, abs(l - l2), FLOOR)


@pytest.mark.parametrize("win", lc.NF_WINS, ids=["w" + lc._wt(w) for w in lc.NF_WINS])
def test_ncc_non_finite_footprint(vxm, win):
    """One voxel of I or of J set to NaN / +Inf / -Inf: in the interior, at (0,0,0), at the last voxel, on either side of a tile edge (h = 7 | 8,
    w = 31 | 32) and of a segment edge (d = 19 | 20).  The loss is NaN; the non-finite SETS of dJ and dI equal the arbiter's on the same poisoned
    input -- which tests/test_cpu_losses.py shows to be the fp32 reference's, the clipped (4R+1)^3 box for a cubic window --; every other voxel is
    under the gate of the uniform class."""
    clean = lc.ncc_nf_arrays(win, ("interior", "I", 0.5))
    _, gJc, _ = ncc_run(vxm, clean[0], clean[1], win)
    assert not bad(gJc).any()
    _, gg = NCC_GATES["uniform/" + lc._wt(win)]
    worst = 0.0
    for case in lc.NF_CASES:
        I, J = lc.ncc_nf_arrays(win, case)
        l64, gJ, gI = lc.ncc_arbiter(I, J, win)
        l, dJ, dI = ncc_run(vxm, I, J, win)
        tag = "ncc w%s %s %s=%s" % (lc._wt(win), case[0], case[1], case[2])
        assert np.isnan(l64) and np.isnan(l), tag + ": loss %r, arbiter %r" % (l, l64)
        assert 0 < bad(gJ).sum() < gJ.size
        same_set(tag + " dJ", dJ, gJ)
        same_set(tag + " dI", dI, gI)
        e = max(lc.rel_l2(dJ[~bad(gJ)], gJ[~bad(gJ)]), lc.rel_l2(dI[~bad(gI)], gI[~bad(gI)]))
        assert e <= gg, "%s: finite remainder %.3e > %.3e" % (tag, e, gg)
        worst = max(worst, e)
    gate("ncc w%s non-finite: finite remainder of dJ, dI, worst of %d cases" % (lc._wt(win), len(lc.NF_CASES)), worst, gg)


# ------------------------------------------------------------------ Grad
@pytest.mark.parametrize("row", lc.GRAD_ROWS, ids=lc.GRAD_IDS)
def test_grad_every_row_vs_fp64(vxm, row):
    """losses.Grad on every row: l1 and l2, loss_mult None / 2 / 0.01, upstream gradient 1 and -0.37, against oracle.grad_loss in float64 (the
    loss scaled by loss_mult, the gradient by loss_mult and the upstream gradient).  A constant field gives a loss and gradients of exactly 0;
    the `ties` rows hold many exact zeros of the differences (sign(0) = 0 in the reference's l1 gradient).  dy is bit-identical between two calls."""
    name, shape, regime = row
    y = lc.grad_arrays(row)
    for pen in (("l2",) if regime == "big" else ("l1", "l2")):
        l64, g64 = lc.grad_reference(y, pen, torch.float64)
        for mult in lc.GRAD_MULTS:
            m = 1.0 if mult is None else mult
            for up in lc.UPSTREAM:
                l, dy = grad_run(vxm, y, pen, mult, up)
                tag = "grad %s %s mult %s up %+.2f" % (name, pen, mult, up)
                if regime == "const":
                    assert l == 0.0 and l64 == 0.0 and not dy.any() and not g64.any(), tag + ": a constant field has loss and gradient 0"
                    continue
                gl, gg = GRAD_GATES[lc.grad_class(pen, regime)]
                gate(tag + " loss vs fp64", abs(l - m * l64) / abs(m * l64), gl)
                gate(tag + " dy vs fp64", lc.rel_l2(dy, (m * up) * g64), gg)
        l2, dy2 = grad_run(vxm, y, pen, mult, up)
        assert same_bits(dy, dy2), name + ": two calls give different gradient bits"
        gate("grad %s %s loss of a second call" % (name, pen), abs(l - l2) / max(abs(l), 1e-30), FLOOR)


@pytest.mark.parametrize("pen", ["l1", "l2"])
def test_grad_unaligned_pointer_takes_the_scalar_kernels(vxm, pen):
    """W % 4 == 0 but the field starts one float into a larger buffer: the 16-byte loads are not allowed, the scalar kernels run.  They agree
    with the arbiter, and with the `_v4` kernels on the aligned copy, within the gate."""
    shape = lc.GRAD_UNALIGNED
    y = np.random.default_rng(6400).standard_normal(shape).astype(np.float32)
    n = y.size
    buf = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    view = buf[1:1 + n].view(*shape)
    view.copy_(G(y))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and shape[-1] % 4 == 0
    l64, g64 = lc.grad_reference(y, pen, torch.float64, 2)
    gl, gg = GRAD_GATES[lc.grad_class(pen, "normal")]
    lu, du = grad_run(vxm, view, pen, 2)
    la, da = grad_run(vxm, y, pen, 2)
    assert bool((buf[0] == 0).all()) and bool((buf[1 + n:] == 0).all())
    gate("grad unaligned %s loss vs fp64" % pen, abs(lu - l64) / abs(l64), gl)
    gate("grad unaligned %s dy vs fp64" % pen, lc.rel_l2(du, g64), gg)
    gate("grad unaligned %s loss vs the aligned run" % pen, abs(lu - la) / abs(la), gl)
    gate("grad unaligned %s dy vs the aligned run" % pen, lc.rel_l2(du, da), gg)


@pytest.mark.parametrize("pen", ["l1", "l2"])
@pytest.mark.parametrize("shape", lc.GRAD_NF_SHAPES, ids=["v4_W8", "scalar_W7", "planar_v4_W8"])
def test_grad_non_finite_footprint(vxm, shape, pen):
    """One voxel set to +Inf / -Inf / NaN: in the interior and on the first and the last plane of every axis, on a `_v4` shape, a scalar one and a planar
    `_v4` one (no D axis at all: its clamped loads name the voxel itself everywhere).
    The fp32 reference on the same input decides: the loss keeps its class (Inf of the same sign, or NaN), dy has the reference's non-finite
    set and the reference's Inf signs (l1: finite everywhere, sign(NaN) = 0), every other voxel is under the gate against float64.  A missing
    neighbour must be dropped, not replaced by the voxel: Inf - Inf is NaN."""
    gl, gg = GRAD_GATES[lc.grad_class(pen, "normal")]
    worst = 0.0
    for where, pos in lc.grad_nf_positions(shape).items():
        for val in lc.GRAD_NF_VALUES:
            for up in lc.UPSTREAM:
                y = lc.grad_nf_array(shape, pos, val)
                with np.errstate(invalid="ignore"):
                    lr, gr = lc.grad_reference(y, pen, torch.float32, 2, up)
                    _, g64 = lc.grad_reference(y, pen, torch.float64, 2, up)
                l, dy = grad_run(vxm, y, pen, 2, up)
                tag = "grad %s %s %s=%s up %+.2f" % ("x".join(map(str, shape)), pen, where, val, up)
                assert not np.isfinite(lr)
                assert (np.isnan(l) and np.isnan(lr)) or l == lr, tag + ": loss %r, the reference's %r" % (l, lr)
                same_set(tag + " dy", dy, gr)
                inf = np.isinf(gr)
                assert np.array_equal(dy[inf], gr[inf]), tag + ": signs of the infinite gradients"
                assert np.array_equal(np.isnan(dy), np.isnan(gr)), tag + ": NaN set"
                keep = ~bad(gr) & ~bad(g64)
                e = lc.rel_l2(dy[keep], g64[keep])
                assert e <= gg, "%s: finite remainder %.3e > %.3e" % (tag, e, gg)
                worst = max(worst, e)
    gate("grad %s %s non-finite: finite remainder of dy, worst case" % ("x".join(map(str, shape)), pen), worst, gg)


def test_grad_refusals(vxm):
    """Where the reference returns NaN (the mean of no differences) the kernels refuse: an axis of one voxel raises with the shape in the
    message; so does a batch beyond gridDim.y."""
    from voxelmorph_amd._lib import VxmHipError
    for shape in ((1, 2, 1, 5, 8), (1, 2, 4, 1, 8), (2, 3, 4, 5, 1), (1, 2, 1, 8), (1, 2, 9, 1)):
        with pytest.raises(VxmHipError, match=",".join(map(str, shape))):
            vxm.losses.Grad("l2").loss(None, torch.zeros(shape, device="cuda"))
    with pytest.raises(VxmHipError, match="65536"):
        vxm.losses.Grad("l1").loss(None, torch.zeros((65536, 1, 2, 2, 2), device="cuda"))
