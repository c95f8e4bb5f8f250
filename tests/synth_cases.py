"""The table of the SynthMorph image synthesis shared by tests/test_cpu_synth.py (the arbiters against independent restatements),
tests/test_gpu_synth.py (the kernels of csrc/synth.hip and `vxm.synth` against the arbiters) and tools/synth_gates.py (the gates, from the
error of a plain fp32 torch-CPU evaluation of the same definition on exactly these inputs).

The definition (include/vxm_hip.h, "image synthesis from label maps"):
    draw     image = means[b, k] + stds[b, k] * noise,  k = index of the voxel's label in the sorted list; 0 for a label not in it
    one-hot  plane out_index[k] gets 1, every other plane 0; a dropped (-1) or unknown label gives zeros
    blur     per axis 0, 1, 2:  y[i] = sum_t taps[b, a, t] x[i + t - R],  zero padding, t ascending
    finish   y = clip(x * exp(log_bias), 0, 255);  out = ((y - min y) / (max y - min y)) ^ gamma[b];  zeros where max y == min y
The arbiters are float64 numpy, from the float32 inputs."""
import numpy as np

F32 = np.float32

LABELS = [0, 2, 3, 17, 41, 1024]                 # not contiguous
UNKNOWN = (7.0, 2000.0, 2.5)                     # a few voxels carry one of these: not in the list
OUT_LIST = [2, 17, 1024, 99]                     # out_label_list as a list: 0, 3, 41 are dropped, 99 is no input label
OUT_DICT = {0: 0, 2: 5, 3: 5, 41: 9, 55: 1}      # as a dict: 2 and 3 merge into 5, 17 and 1024 are dropped, 55 is no input label

# (id, extents, B, seed)
ROWS = [
    ("tiny_2x2x2", (2, 2, 2), 1, 7101),            # the smallest volume; at T = 7 every tap but the centre reaches outside
    ("wide_7x9x70", (7, 9, 70), 2, 7102),          # V = 4410 is no multiple of 4: the element-wise paths
    ("ragged_3x40x33", (3, 40, 33), 1, 7103),      # V = 3960: the 16-byte paths with a ragged last workgroup; W odd: the scalar blur
    ("batch_5x6x40", (5, 6, 40), 3, 7104),         # the per-sample table, taps and gamma strides; W a multiple of 4: the 16-byte blur
    ("seams_20x36x132", (20, 36, 132), 1, 7105),   # 93 workgroups of every kernel (1024 voxels: the blur of axes 0, 1, the finish chunk), 372 of the row blur
]
ROW_IDS = [r[0] for r in ROWS]
# draw, one-hot and finish only: more voxels than one pass of the table kernels' 2048 workgroups takes (524288 quads), and 436 partials per
# sample in the finish (more than its 256 threads)
BIG = ("stride_130x130x132", (130, 130, 132), 1, 7106)
BLUR_T = (3, 7, 13)
FINISH_VARIANTS = ("bias_g0.5", "bias_g1.7", "clip_both")
LATTICES = [("lattice_6x10x36", (6, 10, 36), 2, 7201), ("lattice_5x7x33", (5, 7, 33), 2, 7202)]
GATE_CLASSES = ("blur", "finish")
# tools/synth_gates.py (profiles/pr12_synth_gates_cpu.txt): 4 x the largest rel-L2 error of the plain fp32 torch-CPU evaluation of the class over
# the rows (tests/test_cpu_synth.py compares these figures with the recorded output)
GATES = dict(blur=2.993e-07, finish=3.508e-07)

E2E = dict(shape=(16, 24, 32), B=2, warp_res=(8,), bias_res=(8,), int_steps=5, seed=7301)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def label_map(rng, B, size):
    """[B,1,*size] fp32: labels of LABELS in runs along the last axis (a label map is piecewise constant), a few voxels not in the list"""
    V = int(np.prod(size))
    runs = rng.integers(1, 9, size=B * V)
    vals = np.repeat(rng.choice(np.asarray(LABELS, dtype=np.float64), size=B * V), runs)[:B * V]
    stray = rng.random(B * V) < 0.02
    vals[stray] = rng.choice(np.asarray(UNKNOWN), size=int(stray.sum()))
    vals[0] = UNKNOWN[0]
    return vals.reshape((B, 1) + tuple(size)).astype(F32)


def row_arrays(row):
    """the float32 inputs of a table row"""
    name, size, B, seed = row
    rng = np.random.default_rng(seed)
    L = len(LABELS)
    a = dict(size=tuple(size), B=B, labels=label_map(rng, B, size))
    a["means"] = rng.uniform(25, 225, (B, L)).astype(F32)
    a["stds"] = rng.uniform(5, 25, (B, L)).astype(F32)
    a["noise"] = rng.standard_normal((B, 1) + tuple(size)).astype(F32)
    a["x"] = rng.uniform(10, 240, (B, 1) + tuple(size)).astype(F32)                      # what a blurred image looks like
    a["sigma"] = rng.uniform(0.3, 2.0, (B, 3))
    a["log_bias"] = (0.2 * rng.standard_normal((B, 1) + tuple(size))).astype(F32)
    return a


def taps_for(sigma, T):
    """[B,3,T] fp32 Gaussian taps, float64 arithmetic (an independent restatement of vxm.synth.gaussian_taps)"""
    sigma = np.asarray(sigma, dtype=np.float64)
    R = (T - 1) // 2
    out = np.zeros(sigma.shape + (T,))
    for idx in np.ndindex(sigma.shape):
        if sigma[idx] <= 1e-6:
            out[idx][R] = 1.0
        else:
            g = np.exp(-0.5 * ((np.arange(T) - R) / sigma[idx]) ** 2)
            out[idx] = g / g.sum()
    return out.astype(F32)


def finish_inputs(a, variant):
    """(x, log_bias, gamma) of a finish variant of a row"""
    B = a["B"]
    if variant == "bias_g0.5":
        return a["x"], a["log_bias"], np.asarray([(0.5, 1.7)[b % 2] for b in range(B)], F32)
    if variant == "bias_g1.7":
        return a["x"], a["log_bias"], np.asarray([(1.7, 0.5)[b % 2] for b in range(B)], F32)
    assert variant == "clip_both"
    return (a["x"] * F32(1.5) - F32(60.0)).astype(F32), a["log_bias"], np.asarray([(1.7, 0.5)[b % 2] for b in range(B)], F32)      # -45 .. 300


def lattice_arrays(lat):
    """integers in [-8, 8] and dyadic taps, different per axis and per sample: every product and every sum is exact in fp32"""
    name, size, B, seed = lat
    rng = np.random.default_rng(seed)
    three, five = [0.0, 0.25, 0.5, 0.25, 0.0], [0.125, 0.25, 0.25, 0.25, 0.125]
    taps = np.asarray([[three, five, three], [five, three, five]], dtype=F32)[:B]
    return dict(x=rng.integers(-8, 9, size=(B, 2) + tuple(size)).astype(F32), taps=taps, size=tuple(size), B=B)


# --------------------------------------------------------------------------- the arbiters
def lookup(labels, label_list):
    """index of every voxel's label in the sorted list, -1 where it is not in it"""
    lst = np.asarray(label_list, dtype=np.float64)
    assert np.all(np.diff(lst) > 0)
    v = np.asarray(labels, dtype=np.float64)
    k = np.clip(np.searchsorted(lst, v), 0, len(lst) - 1)
    return np.where(lst[k] == v, k, -1)


def draw_arbiter(labels, label_list, means, stds, noise, dtype=np.float64):
    """float64 arbiter of the draw; with dtype=float32 the same two operations in numpy float32 (they reproduce bit for bit)"""
    k = lookup(labels, label_list)                                   # [B,1,*size]
    B = k.shape[0]
    m = np.asarray(means, dtype=F32).astype(dtype)
    s = np.asarray(stds, dtype=F32).astype(dtype)
    z = np.asarray(noise, dtype=F32).astype(dtype)
    out = np.zeros(k.shape, dtype=dtype)
    for b in range(B):
        kb = np.maximum(k[b], 0)
        out[b] = np.where(k[b] >= 0, m[b][kb] + s[b][kb] * z[b], dtype(0))
    return out


def out_table(label_list, out_labels):
    """(sorted output labels, out_index per input label, out value per input label) for out_labels None / list / dict"""
    lst = list(label_list)
    if out_labels is None:
        mapping = {v: v for v in lst}
    elif isinstance(out_labels, dict):
        mapping = {k: v for k, v in out_labels.items() if k in lst}
    else:
        mapping = {v: v for v in out_labels if v in lst}
    outs = sorted(set(mapping.values()))
    return outs, np.asarray([outs.index(mapping[v]) if v in mapping else -1 for v in lst], dtype=np.int32), \
        np.asarray([mapping.get(v, 0) for v in lst], dtype=F32)


def onehot_arbiter(labels, label_list, out_index, Lout):
    k = lookup(labels, label_list)[:, 0]                             # [B,*size]
    plane = np.where(k >= 0, np.asarray(out_index)[np.maximum(k, 0)], -1)
    return (plane[:, None] == np.arange(Lout).reshape((1, Lout) + (1,) * (k.ndim - 1))).astype(F32)


def blur_arbiter(x, taps, dtype=np.float64):
    """float64 arbiter of the blur: axis 0, then 1, then 2, taps ascending, zero padding.  x [B,C,D,H,W], taps [B,3,T]"""
    y = np.asarray(x, dtype=F32).astype(dtype)
    tp = np.asarray(taps, dtype=F32).astype(dtype)
    T = tp.shape[2]
    R = (T - 1) // 2
    for a in range(3):
        ax = 2 + a
        S = y.shape[ax]
        pad = [(0, 0)] * 5
        pad[ax] = (R, R)
        padded = np.pad(y, pad)
        acc = np.zeros_like(y)
        for t in range(T):
            sl = [slice(None)] * 5
            sl[ax] = slice(t, t + S)
            acc = acc + tp[:, a, t].reshape(-1, 1, 1, 1, 1) * padded[tuple(sl)]
        y = acc
    return y


def finish_arbiter(x, log_bias, gamma, dtype=np.float64):
    """float64 arbiter of the finish; with dtype=float32, log_bias None and gamma 1 the kernel's own operations in numpy float32"""
    v = np.asarray(x, dtype=F32).astype(dtype)
    if log_bias is not None:
        v = v * np.exp(np.asarray(log_bias, dtype=F32).astype(dtype))
    y = np.minimum(np.maximum(v, dtype(0)), dtype(255))
    out = np.zeros_like(y)
    for b in range(y.shape[0]):
        mn, mx = y[b].min(), y[b].max()
        if mx > mn:
            q = (y[b] - mn) / (mx - mn)
            g = dtype(np.asarray(gamma, dtype=F32)[b])
            out[b] = q if g == 1 else q ** g
    return out


# --------------------------------------------------------------------------- the same definitions as plain torch ops: the gates (fp32, CPU) and
# the ATen formulation that tools/synth_time.py races on the device
def draw_torch(labels, label_list_t, means, stds, noise):
    """a gather by label, then randn * std + mean; label_list_t: the sorted labels as a tensor"""
    import torch
    k = torch.bucketize(labels, label_list_t).clamp_(max=label_list_t.numel() - 1)
    known = label_list_t[k] == labels
    B = labels.shape[0]
    kb = k.reshape(B, -1)
    m = torch.gather(means, 1, kb).reshape(labels.shape)
    s = torch.gather(stds, 1, kb).reshape(labels.shape)
    return torch.where(known, noise * s + m, torch.zeros((), dtype=noise.dtype, device=noise.device))


def onehot_torch(labels, out_values_t):
    """L compares: the planes are `labels == value`, labels already recoded"""
    return (labels == out_values_t.view(1, -1, 1, 1, 1)).to(labels.dtype)


def blur_torch(x, taps):
    """three conv3d calls per sample (cross-correlation, zero padding), in the dtype of x"""
    import torch
    import torch.nn.functional as F
    B, C = x.shape[:2]
    T = taps.shape[2]
    R = (T - 1) // 2
    outs = []
    for b in range(B):
        y = x[b].unsqueeze(1)                                        # [C,1,D,H,W]: the channels as a batch of one-channel volumes
        for a in range(3):
            shape, pad = [1, 1, 1, 1, 1], [0, 0, 0]
            shape[2 + a], pad[a] = T, R
            y = F.conv3d(y, taps[b, a].to(x.dtype).reshape(shape), padding=pad)
        outs.append(y.squeeze(1))
    return torch.stack(outs)


def finish_torch(x, log_bias, gamma):
    """exp, mul, clamp, amin, amax, sub, div, pow"""
    import torch
    v = x if log_bias is None else x * torch.exp(log_bias)
    y = v.clamp(0, 255)
    dims = tuple(range(1, y.dim()))
    mn, mx = y.amin(dims, keepdim=True), y.amax(dims, keepdim=True)
    g = gamma.view((-1,) + (1,) * (y.dim() - 1))
    return torch.where(mx > mn, ((y - mn) / (mx - mn)).pow(g), torch.zeros((), dtype=y.dtype, device=y.device))
