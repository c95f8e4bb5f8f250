"""Case table and arbiter of the mutual information loss (voxelmorph_amd/csrc/mi.hip, `vxm.losses.MutualInformation`).  Imports no GPU code.
Used by tests/test_cpu_mi.py (the conditions of the table), tests/test_gpu_mi.py (the kernels) and tools/mi_gates.py (the committed gates).

The reference has this loss on its TensorFlow side only (voxelmorph/tf/losses.py:352-367) and shows only a wrapper around a class of another
package, so the definition is fixed by this project (include/vxm_hip.h).  `formulation(..., dtype=torch.float64)` below restates it
in plain torch ops with autograd: that is the ARBITER.  The same function at float32 is "the reference formulation": what a user would
write in ATen.  A class is a value regime; its gate is MARGIN x the worst error of the fp32 reference formulation against the arbiter over
the rows of the class (tools/mi_gates.py, CPU, one thread).  The loss is gated by absolute error, never below MARGIN x 2^-24 x max(1,
|loss|); gradients by rel-L2, except in the classes of ABS_L2 (true gradient ~0), which are gated by absolute L2 error.  That list is closed:
tests/test_cpu_mi.py asserts an arbiter gradient norm >= MIN_GRAD_NORM for every other row."""
import os
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATES_FILE = os.path.join(ROOT, "profiles", "pr08_mi_gates_cpu.txt")

MARGIN = 4.0
HALF_ULP = 2.0 ** -24
EPS = 1e-7
MIN_GRAD_NORM = 1e-3
ABS_L2 = ("const_true", "const_pred", "single")

# Voxels one forward workgroup takes when the sample is small (csrc/mi.hip: MI_CHUNK_MIN), restated: the GPU test asserts that the rows
# below straddle what vxm_mi_chunk reports for them; nothing here is imported from the library.
CHUNK = 2048

UNIFORM32 = 32
USER_CENTRES = (0.0, 0.08, 0.2, 0.38, 0.5, 0.71, 0.85, 1.0)           # not uniform
NARROW_CENTRES = tuple(float(v) for v in np.linspace(0.4, 0.6, 8))    # clip range [0, 1] far wider: exp(-alpha d^2) alone underflows

VOL = (2, 1, 12, 14, 16)


def row(name, cls, shape, bins=UNIFORM32, clip=(0.0, 1.0), gloss=1.0, grads="both", layout="contig"):
    return dict(name=name, cls=cls, shape=tuple(shape), bins=bins, clip=clip, gloss=gloss, grads=grads, layout=layout)


ROWS = [
    # ---- geometry x noisy
    row("n1", "single", (1, 1)),
    row("n63", "noisy", (1, 63)),
    row("n64", "noisy", (1, 64)),
    row("n65", "noisy", (1, 65)),
    row("chunk_minus_1", "noisy", (1, CHUNK - 1)),
    row("chunk", "noisy", (1, CHUNK)),
    row("chunk_plus_1", "noisy", (1, CHUNK + 1)),
    row("ragged_5_chunks", "noisy", (2, 5 * CHUNK + 77)),             # six workgroups per sample, the last one holds 77 voxels
    row("vol3d", "noisy", VOL),
    row("img2d", "noisy", (2, 1, 24, 20)),
    row("sig1d_3ch", "noisy", (2, 3, 40)),
    row("vol3d_2ch", "noisy", (1, 2, 6, 6, 6)),
    row("offset_one_float", "noisy", (2, 1, 24, 20), layout="offset1"),
    row("non_contiguous", "noisy", (2, 1, 24, 20), layout="noncontig"),
    # ---- bins
    row("k2", "noisy", (2, 1, 24, 20), bins=2),
    row("k5", "noisy", (2, 1, 24, 20), bins=5),
    row("k16", "noisy", (2, 1, 24, 20), bins=16),
    row("k31", "noisy", (2, 1, 24, 20), bins=31),
    row("user_centres", "noisy", (2, 1, 24, 20), bins=USER_CENTRES),
    row("clip_wider_than_centres", "wideclip", (2, 1, 24, 20), bins=NARROW_CENTRES),
    # ---- upstream gradient, which gradients
    row("gloss_minus_0.37", "noisy", VOL, gloss=-0.37),
    row("grad_pred_only", "noisy", VOL, grads="pred"),
    row("grad_true_only", "noisy", VOL, grads="true"),
    # ---- value regimes at one geometry
    row("indep", "indep", VOL),
    row("same", "same", VOL),
    row("anti", "anti", VOL),
    row("outside", "outside", VOL),
    row("x255", "x255", VOL),
    row("centres", "centres", VOL),
    row("const_true", "const_true", VOL),
    row("const_pred", "const_pred", VOL),
    row("real", "real", VOL),
    # ---- three regimes in one batch: the samples must not leak into each other (checked per sample through B = 1 calls on the GPU)
    row("batch3_mixed", "mixed", (3, 1, 12, 14, 16)),
]
MIXED = ("indep", "anti", "noisy")
IDS = [r["name"] for r in ROWS]
BY_NAME = {r["name"]: r for r in ROWS}
CLASSES = sorted({r["cls"] for r in ROWS})


def centres_of(r):
    bins = r["bins"]
    if isinstance(bins, int):
        lo, hi = r["clip"]
        step = (hi - lo) / (bins - 1)
        return tuple([lo + step * i for i in range(bins - 1)] + [hi])          # as MutualInformation(nb_bins=K) builds them
    return tuple(bins)


def real_pair(B, vol3, shift=1):
    """Crops of the T1 scan scaled to [0, 1], and a smoothly intensity-remapped (contrast inverted, as T1 -> T2) copy displaced by `shift`
    voxels along the last axis: the multi-modal pair the loss exists for."""
    scan = np.load(os.path.join(ROOT, "tests", "golden", "real_scan_u8.npz"), allow_pickle=False)["vol_u8"]
    d, h, w = vol3
    I = np.empty((B, 1, d, h, w), np.float32)
    J = np.empty_like(I)
    for b in range(B):
        z, y, x = 70 + 9 * b, 90 - 11 * b, 100 + 7 * b
        I[b, 0] = scan[z:z + d, y:y + h, x:x + w].astype(np.float32) / 255.0
        J[b, 0] = remap(scan[z:z + d, y:y + h, x + shift:x + shift + w].astype(np.float32) / 255.0)
    return I, J


def remap(x):
    return (0.95 - 0.8 * x ** 0.7 + 0.04 * np.sin(9.0 * x)).astype(np.float32)


def _values(cls, shape, rng, centres):
    u = rng.random(shape, dtype=np.float32)
    if cls == "indep":
        return u, rng.random(shape, dtype=np.float32)
    if cls == "same":
        return u, u.copy()
    if cls == "anti":
        return u, (1.0 - u).astype(np.float32)
    if cls in ("noisy", "single", "wideclip"):
        return u, (u + 0.05 * rng.standard_normal(shape).astype(np.float32)).astype(np.float32)
    if cls == "outside":                             # [-1, 2]: a third below, a third above the clip range; some exactly on a bound
        a = (3.0 * u - 1.0).astype(np.float32)
        b = (a + 0.05 * rng.standard_normal(shape).astype(np.float32)).astype(np.float32)
        a.reshape(-1)[::17] = 0.0
        a.reshape(-1)[5::19] = 1.0
        b.reshape(-1)[3::23] = 1.0
        b.reshape(-1)[7::29] = 0.0
        return a, b
    if cls == "x255":                                # unnormalised intensities: a dark background below 1, everything else clamped to 1
        a = (255.0 * u).astype(np.float32)
        dark = rng.random(shape) < 0.3
        a[dark] = rng.random(int(dark.sum()), dtype=np.float32)
        b = (a * (1.0 + 0.1 * rng.standard_normal(shape).astype(np.float32))).astype(np.float32)
        return a, np.abs(b)
    if cls == "centres":                             # every voxel exactly ON a bin centre
        c = np.asarray(centres, np.float32)
        ia = rng.integers(0, len(c), shape)
        ib = np.clip(ia + rng.integers(-2, 3, shape), 0, len(c) - 1)
        return c[ia], c[ib]
    if cls == "const_true":
        return np.full(shape, 0.3, np.float32), u
    if cls == "const_pred":
        return u, np.full(shape, 0.7, np.float32)
    raise KeyError(cls)


def inputs(r):
    """(y_true, y_pred): seeded fp32 numpy arrays of r['shape']"""
    rng = np.random.default_rng(zlib.crc32(r["name"].encode()))
    shape, cls = r["shape"], r["cls"]
    if cls == "real":
        return real_pair(shape[0], shape[2:])
    if cls == "mixed":
        pairs = [_values(c, (1,) + shape[1:], rng, centres_of(r)) for c in MIXED]
        return np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    return _values(cls, shape, rng, centres_of(r))


def soft_bins(x, c, alpha, lo, hi):
    """[B, N] -> [B, N, K]; the smallest squared distance is subtracted before exp (the same function; finite for any centres)"""
    d2 = (x.clamp(lo, hi)[..., None] - c) ** 2
    e = torch.exp(-alpha * (d2 - d2.min(-1, keepdim=True).values.detach()))
    return e / e.sum(-1, keepdim=True)


def formulation(y_true, y_pred, centres, sigma_ratio=0.5, min_clip=0.0, max_clip=1.0, dtype=torch.float64):
    """The definition in plain torch ops: the arbiter at float64, the reference formulation at float32.  Returns the 0-dim loss."""
    c64 = torch.tensor(centres, dtype=torch.float64)
    sigma = sigma_ratio * float((c64[1:] - c64[:-1]).mean())
    alpha = 1.0 / (2.0 * sigma * sigma)
    c = c64.to(dtype=dtype, device=y_true.device)
    B = y_true.shape[0]
    a, b = y_true.to(dtype).reshape(B, -1), y_pred.to(dtype).reshape(B, -1)
    N = a.shape[1]
    wa, wb = soft_bins(a, c, alpha, min_clip, max_clip), soft_bins(b, c, alpha, min_clip, max_clip)
    pab = torch.bmm(wa.transpose(1, 2), wb) / N
    pa, pb = wa.mean(1), wb.mean(1)
    papb = pa[:, :, None] * pb[:, None, :] + EPS
    mi = (pab * torch.log(pab / papb + EPS)).sum((1, 2))
    return -mi.mean()


def evaluate(r, dtype, yt=None, yp=None):
    """(loss, g_true, g_pred) as float64 numpy of row r at `dtype`, upstream gradient r['gloss']; a gradient the row does not ask for is None"""
    if yt is None:
        yt, yp = inputs(r)
    t = torch.from_numpy(np.ascontiguousarray(yt)).to(dtype).requires_grad_(r["grads"] in ("true", "both"))
    p = torch.from_numpy(np.ascontiguousarray(yp)).to(dtype).requires_grad_(r["grads"] in ("pred", "both"))
    lo, hi = r["clip"]
    loss = formulation(t, p, centres_of(r), 0.5, lo, hi, dtype)
    loss.backward(torch.tensor(r["gloss"], dtype=dtype))
    g = [None if v.grad is None else v.grad.double().numpy() for v in (t, p)]
    return float(loss.detach().double()), g[0], g[1]


_ARBITER = {}


def arbiter(r):
    """float64 evaluation of a row, computed once and shared (do not modify the arrays)"""
    if r["name"] not in _ARBITER:
        _ARBITER[r["name"]] = evaluate(r, torch.float64)
    return _ARBITER[r["name"]]


def _cat(gt, gp):
    return np.concatenate([g.reshape(-1) for g in (gt, gp) if g is not None])


def errors(r, loss, gt, gp):
    """(absolute loss error, gradient rel-L2, gradient absolute L2, arbiter gradient norm) of a result against the arbiter"""
    l64, t64, p64 = arbiter(r)
    want, got = _cat(t64, p64), _cat(gt, gp)
    assert want.shape == got.shape
    diff = float(np.linalg.norm(got.astype(np.float64) - want))
    norm = float(np.linalg.norm(want))
    return abs(loss - l64), diff / max(norm, 1e-300), diff, norm


def loss_floor(r):
    return MARGIN * HALF_ULP * max(1.0, abs(arbiter(r)[0]))


def class_gates(cls):
    """(loss gate, gradient gate, [(row name, loss error, rel-L2, abs-L2)]) from the fp32 reference formulation on this CPU; the loss gate
    is returned WITHOUT its floor (loss_floor is per row)"""
    rows, worst_l, worst_g = [], 0.0, 0.0
    for r in ROWS:
        if r["cls"] != cls:
            continue
        el, rel, ab, _ = errors(r, *evaluate(r, torch.float32))
        rows.append((r["name"], el, rel, ab))
        worst_l, worst_g = max(worst_l, el), max(worst_g, ab if cls in ABS_L2 else rel)
    return MARGIN * worst_l, MARGIN * worst_g, rows


def gate_keys(cls):
    return "%s loss_abs" % cls, "%s %s" % (cls, "grad_abs_l2" if cls in ABS_L2 else "grad_rel_l2")


def load_gates():
    out = {}
    with open(GATES_FILE) as f:
        for line in f:
            if line.startswith("GATE "):
                parts = line.split()
                out[" ".join(parts[1:-1])] = float(parts[-1])
    return out


def gates_of(r, gates):
    """(loss gate with its floor, gradient gate) of a row from the committed file"""
    kl, kg = gate_keys(r["cls"])
    return max(gates[kl], loss_floor(r)), gates[kg]
