"""The warp table shared by tests/test_cpu_host.py (the conditions that keep a row from going vacuous, the arbiter against the fp32 reference),
tests/test_gpu_warp.py (every warp kernel against the float64 arbiter oracle.warp_arbiter / vecint_arbiter) and tools/warp_gates.py (the
gates, from the reference's own fp32 error on exactly these inputs).  Samples are placed where the kernels branch: on lattice points (floor
flips, one weight is 0), on the last plane S - 1, in the half-covered rim (-1, 0) / (S - 1, S), far outside, at NaN / Inf displacements."""
import numpy as np

F32 = np.float32

# (id, dims, B, C, flow recipe, recipe parameter).  Parameter: noise / channels: sigma of the Gaussian flow, chosen per row so that 10 - 60 % of
# the samples have an outside corner and at most 60 % of the outputs are exactly zero (asserted in test_cpu_host.py); rim: sigma of the
# noise on the samples that are NOT moved into the rim; lattice / last_plane / far: unused.
CASES = [
    ("noise_7x9x70", (7, 9, 70), 2, 2, "noise", 1.0),                # W no multiple of 64, H W no multiple of 256
    ("noise_3x40x33", (3, 40, 33), 1, 1, "noise", 0.5),              # D below the 4-deep tile of the fused kernel
    ("lattice_6x7x33", (6, 7, 33), 1, 1, "lattice", None),           # every coordinate on a lattice or half-lattice point
    ("last_plane_5x6x40", (5, 6, 40), 3, 2, "last_plane", None),     # sample b: axis b exactly on S - 1, on 0, and just beyond each
    ("rim_5x6x40", (5, 6, 40), 2, 2, "rim", 0.3),
    ("far_5x6x40", (5, 6, 40), 1, 2, "far", None),
    ("channels_5x6x40", (5, 6, 40), 3, 5, "channels", 0.8),          # the channel loop and the batch stride
    ("noise_13x37", (13, 37), 2, 3, "noise", 2.0),
    ("noise_2x9", (2, 9), 2, 1, "noise", 0.25),
    ("lattice_13x37", (13, 37), 2, 1, "lattice", None),
    ("lattice_2x9", (2, 9), 2, 3, "lattice", None),
    ("rim_13x37", (13, 37), 2, 1, "rim", 0.3),
    ("rim_2x9", (2, 9), 2, 3, "rim", 0.3),
]
IDS = [c[0] for c in CASES]
BANDED = ("noise", "rim", "channels")                                # recipes the outside-corner / zero-output band is asserted for
FAR_VALUES = (1e4, -1e4, 1e9, -1e9, 3e38, -3e38, np.inf, -np.inf, np.nan)

# fused resize + warp rows: (id, low-resolution field, image, amplitude of the low-resolution noise).  The field is upsampled by 2 (int_downsize = 2:
# x2 rescale before the interpolation); the second image has an odd depth (ratio 1/3, a ragged 4-deep tile), reached through the C ABI.
FUSED = [
    ("fused_4x5x17_noise", (4, 5, 17), (8, 10, 34), 0.35),
    ("fused_4x5x17_rim", (4, 5, 17), (8, 10, 34), 0.8),
    ("fused_3x9x20_noise", (3, 9, 20), (7, 18, 40), 0.35),
    ("fused_3x9x20_rim", (3, 9, 20), (7, 18, 40), 0.8),
]
FUSED_IDS = [c[0] for c in FUSED]

# VecInt rows: (dims, sigma): 10 - 40 % of the first step's samples (v / 2^nsteps) at the rim for nsteps in {1, 3}
VECINT = [((6, 9, 40), 2.0), ((13, 37), 1.5)]
VECINT_STEPS = (1, 3)


def _rim_flow(rng, B, dims, sigma):
    """every axis of a sample is moved into (-1, 0) or (S - 1, S) with probability 1 - (2/3)^(1/nd) (at least one axis: a third of the samples, some
    on two axes at once); the other coordinates get |noise| pointing INTO the volume, so they add no outside corner of their own"""
    nd = len(dims)
    flow = np.empty((B, nd) + dims)
    for a, S in enumerate(dims):
        shp = [1] * (nd + 1)
        shp[a + 1] = S
        i = np.arange(S, dtype=np.float64).reshape(shp)
        inward = np.where(i < (S - 1) / 2.0, 1.0, -1.0) * np.minimum(np.abs(rng.standard_normal((B,) + dims)) * sigma, 0.45)
        pick = rng.random((B,) + dims) < 1.0 - (2.0 / 3.0) ** (1.0 / nd)
        high = rng.random((B,) + dims) < 0.5
        frac = rng.uniform(0.02, 0.98, size=(B,) + dims)
        flow[:, a] = np.where(pick, np.where(high, S - 1 + frac, -frac) - i, inward)
    return flow


def _last_plane_flow(rng, B, dims):
    """sample b: along axis b % nd, two thirds of the voxels land exactly on S - 1, exactly on 0, one fp32 ulp beyond S - 1 and inside it, and
    2^-12 / a sub-ulp step beyond either end (i + f is then exact in fp32, or rounds onto the plane); the other axes carry noise"""
    nd = len(dims)
    flow = rng.standard_normal((B, nd) + dims) * 1.2
    for b in range(B):
        a = b % nd
        S = dims[a]
        top = F32(S - 1)
        targets = np.array([top, 0.0, np.nextafter(top, F32(np.inf)), np.nextafter(top, F32(0)), float(top) + 2.0 ** -12, -2.0 ** -12,
                            -2.0 ** -20, -1e-45], dtype=np.float64)
        shp = [1] * nd
        shp[a] = S
        i = np.arange(S, dtype=np.float64).reshape(shp)
        t = targets[rng.integers(0, len(targets), size=dims)]
        pick = rng.random(dims) < 0.67
        flow[b, a] = np.where(pick, t - i, flow[b, a])
    return flow


def _far_flow(rng, B, dims):
    """a smooth, small field with every value of FAR_VALUES once per axis, at voxels of their own"""
    nd = len(dims)
    flow = rng.standard_normal((B, nd) + dims) * 0.4
    flat = flow.reshape(B, nd, -1)
    where = rng.choice(flat.shape[2], size=nd * len(FAR_VALUES), replace=False)
    for k, p in enumerate(where):
        flat[0, k % nd, p] = FAR_VALUES[k // nd]
    return flow


def arrays(case):
    """src [B, C, *dims] (standard normal), flow [B, nd, *dims], gout [B, C, *dims]: fp32, one fixed seed per case"""
    name, dims, B, C, recipe, par = case
    nd = len(dims)
    rng = np.random.default_rng(4100 + IDS.index(name))
    src = rng.standard_normal((B, C) + dims).astype(F32)
    gout = rng.standard_normal((B, C) + dims).astype(F32)
    if recipe in ("noise", "channels"):
        flow = rng.standard_normal((B, nd) + dims) * par
    elif recipe == "lattice":
        flow = rng.integers(-7, 8, size=(B, nd) + dims) * 0.5
    elif recipe == "last_plane":
        flow = _last_plane_flow(rng, B, dims)
    elif recipe == "rim":
        flow = _rim_flow(rng, B, dims, par)
    elif recipe == "far":
        flow = _far_flow(rng, B, dims)
    else:
        raise ValueError(recipe)
    with np.errstate(over="ignore"):
        return src, flow.astype(F32), gout


def fused_arrays(row):
    """img [B, C, *full], low-resolution field [B, 3, *low], gout [B, C, *full]; B = 2, C = 2"""
    name, low, full, amp = row
    rng = np.random.default_rng(4300 + FUSED_IDS.index(name))
    img = rng.standard_normal((2, 2) + full).astype(F32)
    fl = (rng.standard_normal((2, 3) + low) * amp).astype(F32)
    gout = rng.standard_normal((2, 2) + full).astype(F32)
    return img, fl, gout


def vecint_arrays(dims, nsteps):
    sigma = dict(VECINT)[dims]
    rng = np.random.default_rng(4400 + 10 * len(dims) + nsteps)
    B, nd = 2, len(dims)
    vec = (rng.standard_normal((B, nd) + dims) * sigma * 2 ** (nsteps - 1)).astype(F32)       # the first step sees vec / 2^nsteps: sigma / 2 for every nsteps
    gout = rng.standard_normal((B, nd) + dims).astype(F32)
    return vec, gout


def corner_stats(coords, dims):
    """(fraction of samples with at least one outside corner, fraction inside the rim on at least one axis and fully outside on none)
    from the per-axis source coordinates (oracle._src_coords_explicit)"""
    outside = np.zeros(coords[0].shape, dtype=bool)
    rim = np.zeros(coords[0].shape, dtype=bool)
    gone = np.zeros(coords[0].shape, dtype=bool)
    for x, S in zip(coords, dims):
        x = np.asarray(x, dtype=np.float64)
        f = np.floor(x)
        outside |= ~((f >= 0) & (f + 1 <= S - 1))
        rim |= ((x > -1) & (x < 0)) | ((x > S - 1) & (x < S))
        gone |= ~((x > -1) & (x < S))
    return float(outside.mean()), float((rim & ~gone).mean())


def poison(dims, B, C):
    """Where the non-finite-footprint tests put one NaN and one +Inf: border voxels of the sampled tensor, (sample, channel, *voxel)"""
    nd = len(dims)
    lo = (0, 0) + tuple([0] * (nd - 1) + [dims[-1] // 2])                    # first plane / row, mid column
    hi = (B - 1, C - 1) + tuple([d // 2 for d in dims[:-1]] + [dims[-1] - 1])  # last column
    return lo, hi


def clamped_poison_hits(coords, dims, mask):
    """Samples with an OUTSIDE corner whose index, clamped into the volume, names a voxel of `mask` ([B, *dims] bool: poisoned in any channel):
    the samples a kernel that loads the clamped voxel and multiplies it by a zero weight would turn non-finite.  [B, *dims] bool."""
    nd = len(dims)
    hit = np.zeros(coords[0].shape, dtype=bool)
    x64 = [np.asarray(x, dtype=np.float64) for x in coords]
    fin = np.all([np.isfinite(x) for x in x64], axis=0)
    x0 = [np.floor(np.where(fin, x, -2.0)) for x in x64]
    bidx = np.arange(coords[0].shape[0]).reshape((-1,) + (1,) * nd)
    for corner in range(2 ** nd):
        ok = np.ones(hit.shape, dtype=bool)
        js = []
        for a in range(nd):
            j = x0[a] + ((corner >> (nd - 1 - a)) & 1)
            ok &= (j >= 0) & (j <= dims[a] - 1)
            js.append(np.clip(j, 0, dims[a] - 1).astype(np.int64))
        hit |= ~ok & mask[(np.broadcast_to(bidx, hit.shape),) + tuple(js)]
    return hit


# ---- the non-finite footprint inputs: one NaN and one +Inf in border voxels of the sampled tensor, and samples placed outside the volume along
# the lines through them, so that an outside corner, CLAMPED into the volume, names a poisoned voxel
FOOTPRINT = ("warp3d", "fused", "warp2d", "vecint3d", "vecint2d")
FOOTPRINT_DIMS = {"warp3d": (5, 6, 40), "fused": (8, 10, 34), "warp2d": (13, 37), "vecint3d": (5, 6, 40), "vecint2d": (13, 37)}


def _aim_at(flow, b, q, dims):
    """Rewrite the displacement of the 9 voxels q + t e_s (t = -4 .. 4, s an axis along the border q lies on) of sample b so that they sample next
    to q from OUTSIDE: along the border axis a alternately 1.5 voxels out (every corner outside: the reference gives a clean 0) and 0.4 out (the rim:
    the corner inside the volume is q or its neighbour); along s within 0.8 of q_s; on q's index along every other axis."""
    nd = len(dims)
    a = next(k for k in range(nd) if q[k] in (0, dims[k] - 1))
    s = nd - 1 if a != nd - 1 else nd - 2
    outward = -1.0 if q[a] == 0 else 1.0
    for t in range(-4, 5):
        p = list(q)
        p[s] = q[s] + t
        if not 0 <= p[s] < dims[s] or t == 0:
            continue
        for k in range(nd):
            target = q[k] + outward * (1.5 if t % 2 else 0.4) if k == a else (q[k] + 0.2 * t if k == s else float(q[k]))
            flow[(b, k) + tuple(p)] = target - p[k]


def footprint_arrays(kind):
    """(sampled tensor [B, C, *dims] (clean), flow or low-resolution field (None for VecInt: the field is both), gout, the two poisoned
    (sample, channel, *voxel) indices: NaN first, +Inf second).  VecInt: nsteps = 1, the field returned is vec (= 2 v)."""
    dims = FOOTPRINT_DIMS[kind]
    nd = len(dims)
    rng = np.random.default_rng(4500 + FOOTPRINT.index(kind))
    B = 2
    C = nd if kind.startswith("vecint") else 2
    lo, hi = poison(dims, B, C)
    gout = rng.standard_normal((B, C) + dims).astype(F32)
    if kind == "fused":
        low = tuple(d // 2 for d in dims)
        fl = rng.standard_normal((B, 3) + low) * 0.05
        fl[:, 0] -= 0.75                                          # x2: the plane z = 0 samples 1.5 voxels outside, the plane z = 1 in the rim
        hi = (B - 1, C - 1, 0, dims[1] // 2, dims[2] - 1)        # both poisoned voxels on the plane the clamped corners of those samples name
        return rng.standard_normal((B, C) + dims).astype(F32), fl.astype(F32), gout, (lo, hi)
    flow = _rim_flow(rng, B, dims, 0.3)
    for q in (lo, hi):
        _aim_at(flow, q[0], q[2:], dims)
    if kind.startswith("vecint"):
        return (2.0 * flow).astype(F32), None, gout, (lo, hi)
    return rng.standard_normal((B, C) + dims).astype(F32), flow.astype(F32), gout, (lo, hi)


def poisoned(x, where):
    x = x.copy()
    x[where[0]] = np.nan
    x[where[1]] = np.inf
    return x
