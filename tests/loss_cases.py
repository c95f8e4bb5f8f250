"""The NCC / Grad loss table shared by tests/test_cpu_losses.py (the arbiters, the structural claim of every row, the reference's non-finite
footprints, the gate literals), tests/test_gpu_losses.py (the kernels of voxelmorph_amd/csrc/losses.hip through losses.NCC / losses.Grad
against the float64 arbiters) and tools/loss_gates.py (the gates, from the reference's own fp32 error on exactly these inputs).

Rows sit where the kernels branch: volumes that are all halo, the edges of the 8 x 32 tile, the XCD column remap, the depth segments, the
generic and any-window passes, the value regimes in which `var = I2 - 2 u I + u u n` cancels, the second grid-stride pass of the Grad kernels,
the 16-byte lanes of their `_v4` variants, NaN / Inf voxels."""
import numpy as np

F32 = np.float32
HALF_ULP = 2.0 ** -24
MARGIN = 4.0
UPSTREAM = (1.0, -0.37)                    # every row runs with both upstream gradients
TODAY_NCC = (2.5e-7, 2.5e-6, 1e-4)         # NCC_LOSS_GATE, NCC_GRAD_GATE, NCC_GRAD_GATE_1D of tests/test_gpu_parity.py (compared in test_cpu_losses.py)
TODAY_GRAD = 1e-6                          # test_grad_loss_kernel_variants_vs_oracle there

# ---- restated from voxelmorph_amd/csrc/losses.hip (test_cpu_losses.py greps the constants in the source)
NF_TH, NF_TW, NF_SEG = 8, 32, 40           # tile of the fused march, (at most) slices per block along D
NCC_FUSED_WIN = (3, 9)                     # vxm_ncc_fused: odd cubic windows 3 .. 9 ...
NCC_MAX_GRID_B = 65535                     # ... and a batch that fits gridDim.z
# blocks of the four Grad kernels are capped; (cap, rows per block and pass)
GRAD_CAPS = {"fwd": (8192, 4), "fwd_v4": (1024, 16), "bwd": (16384, 4), "bwd_v4": (16384, 8)}


def ncc_segment(B, D, H, W):
    """`ncc_segment` of losses.hip: 40 slices per block, halved to 20 while the grid stays under 1024 blocks"""
    cols = -(-W // NF_TW) * -(-H // NF_TH) * B
    seg = NF_SEG
    while seg > 20 and cols * -(-D // seg) < 1024:
        seg = (seg + 1) // 2
    return seg


def ncc_path(B, vol, win):
    """which kernels losses.NCC takes: 'fused', 'generic' (odd cubic window), 'win' (any window), by the rules of losses.py / vxm_ncc_fused"""
    if len(set(win)) != 1 or win[0] % 2 == 0:
        return "win"
    if len(vol) == 3 and NCC_FUSED_WIN[0] <= win[0] <= NCC_FUSED_WIN[1] and B <= NCC_MAX_GRID_B:
        return "fused"
    return "generic"


def ncc_grid(B, vol):
    """(columns = gridDim.x, segment length, segments = gridDim.y, remap taken) of the fused launch"""
    D, H, W = vol
    cols = -(-W // NF_TW) * -(-H // NF_TH)
    seg = ncc_segment(B, D, H, W)
    return cols, seg, -(-D // seg), cols % 8 == 0


def grad_rows(shape):
    """W rows of a Grad field [B, C, (D,) H, W] per sample: what the grid-stride loops walk"""
    return int(np.prod(shape[1:-1]))


def grad_passes(shape, kernel):
    cap, per = GRAD_CAPS[kernel]
    return -(-grad_rows(shape) // (cap * per))


# ---- NCC rows: (id, B, vol, win, regime).  Regime 'uniform' is I ~ U[0,1), J = 0.6 I + 0.4 U; the others are built from it (ncc_arrays).
REG_VOL, REG_BOX = (20, 27, 40), (slice(4, 16), slice(5, 22), slice(8, 30))
REGIMES = ("x255", "offset", "zerobg", "plateau", "same", "ramp", "signed", "anti")
REG_WINS = ([9] * 3, [3] * 3, [11] * 3, [9, 9, 5])
WELL = ("uniform", "x255", "zerobg", "lowdim")          # well-conditioned: today's fixed gates of test_gpu_parity.py cap the class gate
MAXABS = ("same", "single", "single1d")                 # true gradient ~0 / ill-conditioned: gradients by max-abs error


def by_maxabs(row):
    """gradients of this row are judged by max-abs error: I == J and the one-voxel volumes and signals (the true gradient is ~0 / ill-conditioned), and a
    window of one voxel, where cross = IJ - I J is exactly 0 and with it the true gradient (a relative error has no denominator)"""
    return row[4] in MAXABS or set(row[3]) == {1}


def _wt(win):
    return str(win[0]) if len(set(win)) == 1 else "x".join(map(str, win))


def _row(tag, B, vol, win, regime="uniform"):
    win = [win] * len(vol) if isinstance(win, int) else list(win)
    return ("%s_%dx%s_w%s" % (tag, B, "x".join(map(str, vol)), _wt(win)), B, tuple(vol), win, regime)


NCC_ROWS = (
    [_row("halo", 2, (2, 3, 5), w) for w in (3, 5, 7, 9)]                                   # all four fused instances, everything is halo
    + [_row("single", 1, (1, 1, 1), w, "single") for w in (3, 9)]
    + [_row("tile", 1, v, w) for v in ((4, 8, 32), (5, 9, 33)) for w in (3, 9)]             # exactly one tile / four ragged blocks
    + [_row("remap", 1, (9, 27, 40), 9), _row("remap", 1, (9, 27, 40), 5), _row("remap", 2, (6, 60, 33), 7),
       _row("noremap", 1, (9, 19, 40), 9)]
    + [_row("seg20", 1, (D, 8, 32), w) for D in (20, 21, 41) for w in (9, 7)]
    + [_row("seg40", 8, (41, 2, 2048), 9)]
    + [_row("generic", 1, v, w) for v in ((5, 9, 33), (2, 3, 5)) for w in (1, 11, 13)]
    + [_row("batch", 65536, (2, 3, 4), 3)]                                                   # B > 65535: the generic passes
    + [_row("anywin", 1, (5, 9, 33), w) for w in ([9, 9, 5], [4, 6, 8], [3, 11, 11])]
    + [_row("planar", 2, v, w, "lowdim") for v in ((2, 3), (13, 37)) for w in (9, 11)]
    + [_row("signal", 3, (L,), 9, "single1d" if L == 1 else "lowdim") for L in (1, 8, 777)]     # L = 1: a single-voxel row, as (1,1,1)
    + [_row(r, 1, REG_VOL, w, r) for r in REGIMES for w in REG_WINS]
)
NCC_IDS = [r[0] for r in NCC_ROWS]


def ncc_class(row):
    return "%s/%s" % (row[4], _wt(row[3]))


NCC_CLASSES = sorted(set(ncc_class(r) for r in NCC_ROWS))


def ncc_arrays(row):
    """I, J [B, 1, *vol] fp32, one fixed seed per row"""
    name, B, vol, win, regime = row
    rng = np.random.default_rng(5100 + NCC_IDS.index(name))
    I = rng.random((B, 1) + vol).astype(F32)
    J = (0.6 * I + 0.4 * rng.random((B, 1) + vol)).astype(F32)
    if regime == "x255":
        I, J = I * F32(255), J * F32(255)
    elif regime == "offset":
        I, J = I + F32(100), J + F32(100)
    elif regime == "zerobg":
        keep = np.zeros(vol, dtype=bool)
        keep[REG_BOX] = True
        I, J = np.where(keep, I, F32(0)), np.where(keep, J, F32(0))
    elif regime == "plateau":
        I[..., 20:], J[..., 20:] = F32(0.3), F32(0.7)
    elif regime == "same":
        J = I.copy()
    elif regime == "ramp":
        g = np.meshgrid(*[np.linspace(0.0, 1.0, s) for s in vol], indexing="ij")
        I = np.broadcast_to((sum(g) / len(vol)).astype(F32), (B, 1) + vol).copy()
        J = I * I
    elif regime == "signed":
        I, J = I - F32(0.5), J - F32(0.5)
    elif regime == "anti":
        J = F32(1) - I
    else:
        assert regime in ("uniform", "lowdim", "single", "single1d"), regime
    return np.ascontiguousarray(I, dtype=F32), np.ascontiguousarray(J, dtype=F32)


# ---- NCC non-finite rows: one voxel of I or of J of a uniform (24,12,40) volume set to NaN / +Inf / -Inf
NF_VOL = (24, 12, 40)
NF_WINS = ([3] * 3, [9] * 3, [11] * 3, [9, 9, 5])
NF_POS = {"interior": (10, 5, 15), "first": (0, 0, 0), "last": (23, 11, 39), "tile_lo": (10, 7, 31), "tile_hi": (10, 8, 32),
          "seg_lo": (19, 5, 15), "seg_hi": (20, 5, 15)}
NF_VALUES = (np.nan, np.inf, -np.inf)
NF_CASES = [(pos, which, val) for pos in NF_POS for which in ("I", "J") for val in NF_VALUES]


def ncc_nf_arrays(win, case):
    pos, which, val = case
    rng = np.random.default_rng(5900 + NF_WINS.index(list(win)))
    I = rng.random((1, 1) + NF_VOL).astype(F32)
    J = (0.6 * I + 0.4 * rng.random((1, 1) + NF_VOL)).astype(F32)
    (I if which == "I" else J)[(0, 0) + NF_POS[pos]] = val
    return I, J


def clipped_box(vol, pos, reach):
    """bool mask of the voxels within `reach` of pos on every axis"""
    m = np.zeros(vol, dtype=bool)
    m[tuple(slice(max(0, p - reach), min(s, p + reach + 1)) for p, s in zip(pos, vol))] = True
    return m


# ---- Grad rows: (id, shape, regime).  Regimes: normal, big (x 1e4), const, ties (multiples of 0.5)
def _g(tag, shape, regime="normal"):
    return ("%s_%s" % (tag, "x".join(map(str, shape))), tuple(shape), regime)


GRAD_ROWS = (
    [_g("stride_v4", (1, 3, 210, 209, 4)), _g("stride_scalar", (1, 3, 148, 148, 3)), _g("stride_fwd_v4", (2, 3, 75, 74, 4))]
    + [_g("w_v4", (2, 3, 2, 2, W)) for W in (4, 8, 256, 260, 516)]
    + [_g("w_scalar", (2, 3, 2, 2, W)) for W in (2, 63, 65)]
    + [_g("planar", s) for s in ((2, 2, 2, 4), (1, 2, 9, 16), (1, 2, 9, 15))]
    + [_g("big", (2, 3, 5, 6, 8), "big"), _g("big", (2, 3, 5, 6, 7), "big")]
    + [_g("const", (2, 3, 5, 6, 8), "const"), _g("const", (2, 3, 5, 6, 7), "const")]
    + [_g("ties", (2, 3, 5, 6, 8), "ties"), _g("ties", (2, 3, 5, 6, 7), "ties")]
)
GRAD_IDS = [r[0] for r in GRAD_ROWS]
GRAD_MULTS = (None, 2, 0.01)
GRAD_UNALIGNED = (2, 3, 5, 6, 8)           # W % 4 == 0, run from a view one float into a larger buffer
GRAD_NF_SHAPES = ((1, 2, 4, 5, 8), (1, 2, 4, 5, 7), (1, 2, 5, 8))       # a _v4 and a scalar shape, and a planar _v4 one (no D axis: kd = 0)
GRAD_NF_VALUES = (np.inf, -np.inf, np.nan)


def grad_class(pen, regime):
    return "%s/%s" % (pen, regime)


GRAD_CLASSES = [grad_class(p, r) for p in ("l1", "l2") for r in ("normal", "ties")] + ["l2/big"]


def grad_arrays(row):
    name, shape, regime = row
    rng = np.random.default_rng(6100 + GRAD_IDS.index(name))
    y = rng.standard_normal(shape).astype(F32)
    if regime == "big":
        y = y * F32(1e4)
    elif regime == "const":
        y = np.full(shape, 0.7, dtype=F32)
    elif regime == "ties":
        y = (np.round(y * 2) / 2).astype(F32)
    return y


def grad_nf_positions(shape):
    """an interior voxel, and one on the first and the last plane of every axis (the other coordinates interior), channel 1"""
    dims = shape[2:]
    mid = tuple(d // 2 for d in dims)
    out = {"interior": mid}
    for a in range(len(dims)):
        out["first%d" % a] = mid[:a] + (0,) + mid[a + 1:]
        out["last%d" % a] = mid[:a] + (dims[a] - 1,) + mid[a + 1:]
    return out


def grad_nf_array(shape, pos, val):
    rng = np.random.default_rng(6500 + shape[-1])
    y = rng.standard_normal(shape).astype(F32)
    y[(0, 1) + tuple(pos)] = val
    return y


# ---- helpers shared by the three users
def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def max_abs(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def ncc_arbiter(I, J, win):
    """(loss, dL/dJ, dL/dI) in float64: oracle.ncc_explicit_win"""
    from oracle import vxm_oracle as orc
    with np.errstate(invalid="ignore", over="ignore"):
        return orc.ncc_explicit_win(I, J, win, grad=True)


def ncc_reference(I, J, win, dtype):
    """the reference's formula (oracle.ncc_loss: ATen's conv box sums and autograd on the CPU) in `dtype`: (loss, dJ, dI)"""
    import torch
    from oracle import vxm_oracle as orc
    It, Jt = (torch.from_numpy(a).to(dtype).requires_grad_() for a in (I, J))
    loss = orc.ncc_loss(It, Jt, win=win)
    loss.backward()
    return float(loss.detach()), Jt.grad.numpy(), It.grad.numpy()


def grad_reference(y, pen, dtype, mult=None, upstream=1.0):
    """oracle.grad_loss and its autograd on the CPU in `dtype`: (loss, dy)"""
    import torch
    from oracle import vxm_oracle as orc
    yt = torch.from_numpy(y).to(dtype).requires_grad_()
    loss = orc.grad_loss(yt, pen, mult)
    loss.backward(torch.tensor(upstream, dtype=dtype))
    return float(loss.detach()), yt.grad.numpy()


def ncc_errors(row):
    """(loss error, gradient rel-L2, gradient max-abs) of the reference's fp32 evaluation against the arbiter on one row: the worse of dJ, dI"""
    I, J = ncc_arrays(row)
    l64, gJ, gI = ncc_arbiter(I, J, row[3])
    l32, rJ, rI = ncc_reference(I, J, row[3], __import__("torch").float32)
    return abs(l32 - l64), max(rel_l2(rJ, gJ), rel_l2(rI, gI)), max(max_abs(rJ, gJ), max_abs(rI, gI))


def grad_errors(row, pen):
    """(relative loss error, gradient rel-L2) of the reference's fp32 evaluation against its float64 one"""
    import torch
    y = grad_arrays(row)
    l64, g64 = grad_reference(y, pen, torch.float64)
    l32, g32 = grad_reference(y, pen, torch.float32)
    return abs(l32 - l64) / abs(l64), rel_l2(g32, g64)


def ncc_class_gates(cls, today):
    """(loss gate, gradient gate) of one NCC class: 4 x the worst reference error over its rows, the loss floored at 4 x 2^-24 (|loss| <= 1),
    well-conditioned classes capped by today's fixed gates `today` = (NCC_LOSS_GATE, NCC_GRAD_GATE, NCC_GRAD_GATE_1D)"""
    rows = [r for r in NCC_ROWS if ncc_class(r) == cls]
    errs = [ncc_errors(r) for r in rows]
    regime = rows[0][4]
    loss = max(MARGIN * max(e[0] for e in errs), MARGIN * HALF_ULP)
    grad = MARGIN * max(e[2 if by_maxabs(rows[0]) else 1] for e in errs)
    if regime in WELL:
        loss, grad = min(loss, today[0]), min(grad, today[2] if regime == "lowdim" else today[1])
    return loss, grad, list(zip(rows, errs))


def grad_class_gates(cls, today=1e-6):
    pen, regime = cls.split("/")
    rows = [r for r in GRAD_ROWS if r[2] == regime]
    errs = [grad_errors(r, pen) for r in rows]
    loss = max(MARGIN * max(e[0] for e in errs), MARGIN * HALF_ULP)
    grad = MARGIN * max(e[1] for e in errs)
    if regime == "normal":
        loss, grad = min(loss, today), min(grad, today)
    return loss, grad, list(zip(rows, errs))
