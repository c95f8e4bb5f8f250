"""The affine-transform table shared by tests/test_cpu_affine.py (the arbiter against an independent restatement, the matrix helpers),
tests/test_gpu_affine.py (the kernels of csrc/affine.hip and `vxm.utils` against the float64 arbiter) and tools/affine_gates.py (the gates,
from the error of a plain fp32 evaluation of the same definition on exactly these inputs).

The definition (include/vxm_hip.h): fields [B,3,D,H,W], matrices [Bm,3,4] with Bm in {1, B}, c = 0.5 (S - 1) with shift_center, and
    q[k] = (float(i[k]) - c[k])  (+ w[b,k,i] with a right-composed field);   shift[b,a,i] = (M q + t)[a] - (float(i[a]) - c[a])

`shift_arbiter` is float64 throughout (there is no floor to agree on), from the float32 inputs."""
import numpy as np

F32 = np.float32

# (id, extents, B, C, sigma of the 3 x 3 noise, sigma of the translation, sigma of the right-composed field, seed): M = I + sigma N(0,1)
NOISE = [
    ("noise_7x9x70", (7, 9, 70), 2, 2, 0.03, 0.4, 0.45, 5101),            # W no multiple of 64, H W no multiple of 256: 3 blocks per plane
    ("noise_3x40x33", (3, 40, 33), 1, 1, 0.03, 0.3, 0.4, 5102),           # 1320 voxels per plane: 6 blocks, the last one ragged
    ("channels_5x6x40", (5, 6, 40), 3, 5, 0.04, 0.4, 0.45, 5103),         # the batch stride, one block per plane
    ("noise_6x11x37", (6, 11, 37), 2, 2, 0.04, 0.4, 0.45, 5104),
]
NOISE_IDS = [r[0] for r in NOISE]
VARIANTS = ("mat", "mat_field", "mat_b1", "mat_field_b1")        # matrix only / matrix + right-composed field, Bm = B / Bm = 1
LATTICE = ("lattice_6x7x33", (6, 7, 33), 2, 1, 5201)
ROUNDTRIP = ("roundtrip_12x14x16", (12, 14, 16), 5.0, 2)       # extents, degrees of rotation (about axis 0), interior margin


def variant(arr, name):
    """(mat, flow) of a variant: `_b1` passes the first sample's matrix alone (Bm = 1), `field` adds the right-composed field"""
    mat = arr["mat"][:1] if name.endswith("_b1") else arr["mat"]
    return mat, (arr["flow"] if "field" in name else None)


def noise_arrays(row):
    name, size, B, C, sm, st, sf, seed = row
    rng = np.random.default_rng(seed)
    mat = np.zeros((B, 3, 4))
    mat[:, :, :3] = np.eye(3) + sm * rng.standard_normal((B, 3, 3))
    mat[:, :, 3] = st * rng.standard_normal((B, 3))
    return dict(src=rng.standard_normal((B, C) + size).astype(F32), mat=mat.astype(F32),
                flow=(sf * rng.standard_normal((B, 3) + size)).astype(F32), gshift=rng.standard_normal((B, 3) + size).astype(F32), size=size)


def lattice_arrays():
    """M = identity, translations and a field that are multiples of 0.5: every value is exact in fp32, the shift equals the arbiter's bit for bit"""
    name, size, B, C, seed = LATTICE
    rng = np.random.default_rng(seed)
    mat = np.zeros((B, 3, 4))
    mat[:, :, :3] = np.eye(3)
    mat[:, :, 3] = rng.integers(-4, 5, size=(B, 3)) * 0.5
    return dict(src=rng.standard_normal((B, C) + size).astype(F32), mat=mat.astype(F32),
                flow=(rng.integers(-5, 6, size=(B, 3) + size) * 0.5).astype(F32), gshift=rng.standard_normal((B, 3) + size).astype(F32), size=size)


def roundtrip_arrays():
    """a smooth volume and a rotation by 5 degrees about axis 0 (through the centre: shift_center=True); (vol [1,1,*size], mat, its inverse)"""
    name, size, deg, margin = ROUNDTRIP
    z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in size], indexing="ij")
    vol = np.sin(0.5 * z + 0.3) * np.cos(0.4 * y - 0.2) + 0.5 * np.sin(0.35 * x + 0.25 * y) + 0.1 * z
    t = np.deg2rad(deg)
    m = np.eye(4)
    m[1, 1], m[1, 2], m[2, 1], m[2, 2] = np.cos(t), -np.sin(t), np.sin(t), np.cos(t)
    return vol[None, None].astype(F32), m[None, :3].astype(F32), np.linalg.inv(m)[None, :3].astype(F32)


def interior(a, margin):
    return a[..., margin:-margin, margin:-margin, margin:-margin]


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# --------------------------------------------------------------------------- the arbiter
def shift_arbiter(mat, size, shift_center=True, flow=None, gout=None):
    """float64 arbiter of affine -> dense shift.  Returns (shift [B,3,*size], gflow): gflow[b,k] = sum_a M[a,k] gout[b,a], None without
    `gout` or `flow`."""
    mat = np.asarray(mat, dtype=F32)
    B = flow.shape[0] if flow is not None else mat.shape[0]
    m = np.broadcast_to(mat[:, :3, :].astype(np.float64), (B, 3, 4))
    mesh = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) - (0.5 * (s - 1) if shift_center else 0.0) for s in size], indexing="ij"))
    q = np.broadcast_to(mesh, (B, 3) + tuple(size)).copy()
    if flow is not None:
        q += np.asarray(flow, dtype=np.float64)
    shift = np.einsum("bak,bk...->ba...", m[:, :, :3], q) + m[:, :, 3].reshape(B, 3, 1, 1, 1) - mesh
    gflow = None
    if gout is not None and flow is not None:
        gflow = np.einsum("bak,ba...->bk...", m[:, :, :3], np.asarray(gout, dtype=np.float64))
    return shift, gflow
