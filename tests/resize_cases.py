"""The resize-backward table shared by tests/test_cpu_host.py (which kernel the dispatcher picks), tests/test_gpu_parity.py (each kernel
against the float64 oracle) and tools/resize_gates.py (the gates, from the reference's own fp32 error on exactly these inputs)."""
import math

import numpy as np

# the codes of vxm_resize3d_bwd_kernel (include/vxm_hip.h)
KERNELS = ("scatter", "gather_tiled", "down", "sep", "march")
SCATTER, GATHER_TILED, DOWN, SEP, MARCH = range(5)

# (id, input (D, H, W), vel_resize, output (D, H, W), kernel): ratios (in - 1) / (out - 1) per axis decide the kernel
CASES = [
    ("march_x2", (9, 17, 33), 0.5, (18, 34, 66), MARCH),
    ("march_r0.7", (7, 11, 37), 0.7, (10, 15, 52), MARCH),                   # ratios 0.667 - 0.714
    ("march_all_extent1", (3, 3, 3), 2, (1, 1, 1), MARCH),                   # every ratio 0
    ("sep_x2", (5, 9, 17), 0.5, (10, 18, 34), SEP),
    ("sep_tiles_fits_limit", (4, 20, 40), 0.5, (8, 40, 80), SEP),            # several H / W tiles, rd = 0.4286 at the `fits` limit
    ("sep_not_fits", (6, 10, 40), 0.45, (13, 22, 88), SEP),                  # ratios 0.417 - 0.448: full-width tiles take the direct gather
    ("gather_r0.8", (7, 11, 37), 0.8, (8, 13, 46), GATHER_TILED),
    ("scatter_rd0.4", (3, 5, 9), 0.5, (6, 10, 18), SCATTER),                 # rd = 0.4 exactly
    ("scatter_x3", (7, 11, 37), 1 / 3, (21, 33, 111), SCATTER),
    ("scatter_x4", (5, 6, 20), 0.25, (20, 24, 80), SCATTER),
    ("down_2", (35, 21, 70), 2, (17, 10, 35), DOWN),                         # 3 depth blocks, ragged W tile, odd extents
    ("down_3_skips", (35, 21, 70), 3, (11, 7, 23), DOWN),                    # input voxels no output names
    ("down_4_skips", (34, 19, 67), 4, (8, 4, 16), DOWN),                     # rh = 6 exactly: outputs that name a voxel with weight 0
    ("down_1.5", (17, 33, 65), 1.5, (11, 22, 43), DOWN),
    ("down_1.25", (20, 37, 70), 1.25, (16, 29, 56), DOWN),
    ("down_extent1", (3, 20, 37), 2, (1, 10, 18), DOWN),                     # one output axis of extent 1
]
IDS = [c[0] for c in CASES]
SKIPPING = ("down_3_skips", "down_4_skips")                                  # ratio >= 3 on every axis


def out_shape(inp, vel):
    """floor(n * (1 / vel_resize)) in Python doubles, as ResizeFn and F.interpolate compute it"""
    factor = 1.0 / vel
    return tuple(int(math.floor(n * factor)) for n in inp)


def arrays(case):
    """x [B, 3, *input], gout [B, 3, *output]: standard-normal noise, one fixed seed per case; B = 2 under ~20k voxels, else 1"""
    name, inp, vel, out, _ = case
    B = 2 if max(int(np.prod(inp)), int(np.prod(out))) < 20000 else 1
    rng = np.random.default_rng(2100 + IDS.index(name))
    x = rng.standard_normal((B, 3) + tuple(inp)).astype(np.float32)
    g = rng.standard_normal((B, 3) + tuple(out)).astype(np.float32)
    return x, g


# ResizeTransform(vel, 2): (H, W) x vel_resize.  (2, 9) at vel_resize = 3 has floor(2 / 3) = 0 output rows: the reference raises, so must the product.
PLANAR_SHAPES = [(13, 37), (2, 9)]
PLANAR_VELS = [0.8, 1 / 3, 3, 1.5]


def planar_arrays(shape, vel):
    out = out_shape(shape, vel)
    rng = np.random.default_rng(2200 + 10 * PLANAR_SHAPES.index(tuple(shape)) + PLANAR_VELS.index(vel))
    x = rng.standard_normal((2, 3) + tuple(shape)).astype(np.float32)
    g = rng.standard_normal((2, 3) + out).astype(np.float32) if min(out) > 0 else None
    return x, g


def adjoint_gap(y, g, x, gx):
    """|<y, g> - <x, gx>| / (|y| |g|), all sums in float64: 0 for an exact forward / backward pair (the Cauchy-Schwarz scale of the first
    product, not its value: the inner product of two noise volumes can itself be near zero)"""
    y, g, x, gx = (np.asarray(a, np.float64).ravel() for a in (y, g, x, gx))
    return float(abs(np.dot(y, g) - np.dot(x, gx)) / max(np.linalg.norm(y) * np.linalg.norm(g), 1e-300))
