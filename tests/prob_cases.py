"""The table of the probabilistic velocity field shared by tests/test_cpu_prob.py (the arbiters against independent restatements),
tests/test_gpu_prob.py (the kernels of csrc/prob.hip, `losses.KL` and `networks.VxmDenseProbabilistic` against the float64 arbiters) and
tools/prob_gates.py (the gates, from the error of a plain fp32 torch-CPU evaluation of the same definition on exactly these inputs).

The definition (include/vxm_hip.h, "probabilistic velocity field"): params [B,6,D,H,W], channels 0..2 the mean mu, 3..5 ls = log sigma^2,
    deg(i) = sum_a [(i_a > 0) + (i_a < S_a - 1)]
    loss   = 1.5 * ( mean(lambda deg exp(ls) - ls) + lambda (0.5 / 3) sum_a mean((mu[i + e_a] - mu[i])^2) )
    z      = mu + exp(ls / 2) eps
The arbiters are float64 numpy throughout, from the float32 inputs."""
import numpy as np

F32 = np.float32

# (id, extents, B, regime, seed)
ROWS = [
    ("edge_2x2x2", (2, 2, 2), 1, "wide", 6101),            # every voxel is an edge voxel on every axis: deg = 3
    ("wide_7x9x70", (7, 9, 70), 2, "wide", 6102),          # W no multiple of 4 or 64, V = 4410 no multiple of 4: the element-wise sampler
    ("ragged_3x40x33", (3, 40, 33), 1, "wide", 6103),      # V = 3960: four workgroups of the KL forward, the last one ragged; 16-byte sampler
    ("batch_5x6x40", (5, 6, 40), 3, "wide", 6104),         # the batch stride
    ("init_6x11x37", (6, 11, 37), 2, "init", 6105),        # how training starts: the sum of near-equal large terms
]
ROW_IDS = [r[0] for r in ROWS]
LAMBDAS = (10.0, 25.0)
UPSTREAM = (1.0, -0.37)
LATTICE = ("lattice_6x7x33", (6, 7, 33), 2, 8.0, 6201)
GATE_CLASSES = ("kl_loss", "kl_gmu", "kl_gls", "sample_z", "sample_gls")
LOSS_GATE_FLOOR = 2.0 ** -23        # the loss is ONE fp32 number: no gate below its rounding
# tools/prob_gates.py (profiles/pr11_prob_gates_cpu.txt): 4 x the largest error of the plain fp32 torch-CPU evaluation of the class over ROWS;
# kl_loss is the relative error of one number, the others rel-L2 (tests/test_cpu_prob.py compares these figures with the recorded output)
GATES = dict(kl_loss=4.444e-07, kl_gmu=2.711e-07, kl_gls=3.557e-07, sample_z=1.645e-07, sample_gls=1.892e-07)

# whole model (test_gpu_prob.py): tests/test_gpu_parity.py's tolerances for this depth.  24 is no multiple of 16, which the default four-level
# U-Net needs: this volume takes three pooling levels (encoder [16, 32, 32]), the decoder and the full-resolution convs as in the default.
MODEL = dict(inshape=(16, 24, 32), nb_unet_features=[[16, 32, 32], [32, 32, 32, 32, 16, 16]], int_steps=3, int_downsize=2, head_std=0.05, logsigma_bias=-2.0, image_sigma=0.5, prior_lambda=10.0,
             kl_weight=1.0, seed=6301)


def row_arrays(row):
    """dict(params [B,6,*size], eps, gz [B,3,*size]) of a table row, float32"""
    name, size, B, regime, seed = row
    rng = np.random.default_rng(seed)
    if regime == "wide":
        mu = 0.5 * rng.standard_normal((B, 3) + size)
        ls = rng.uniform(-12.0, 2.0, (B, 3) + size)
    else:
        mu = 1e-3 * rng.standard_normal((B, 3) + size)
        ls = -10.0 + 1e-3 * rng.standard_normal((B, 3) + size)
    return dict(params=np.concatenate([mu, ls], axis=1).astype(F32), eps=rng.standard_normal((B, 3) + size).astype(F32),
                gz=rng.standard_normal((B, 3) + size).astype(F32), size=size)


def lattice_arrays():
    """mu multiples of 0.5, ls = 0: every term and every sum of the KL loss is exact in fp32 and float64"""
    name, size, B, lam, seed = LATTICE
    rng = np.random.default_rng(seed)
    mu = rng.integers(-6, 7, size=(B, 3) + size) * 0.5
    return dict(params=np.concatenate([mu, np.zeros_like(mu)], axis=1).astype(F32), eps=np.zeros((B, 3) + size, F32),
                gz=rng.standard_normal((B, 3) + size).astype(F32), size=size, lam=lam)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# --------------------------------------------------------------------------- the arbiters
def degree(size):
    """closed form of the reference's degree matrix (tf/losses.py:280-292): neighbours inside the grid, float64 [*size]"""
    deg = np.zeros(size)
    for a, s in enumerate(size):
        i = np.arange(s).reshape([-1 if k == a else 1 for k in range(len(size))])
        deg = deg + (i > 0) + (i < s - 1)
    return deg


def kl_arbiter(params, lam, g=1.0):
    """float64 arbiter of the KL loss: (loss, gparams [B,6,*size]) for the upstream gradient g"""
    p = np.asarray(params, dtype=F32).astype(np.float64)
    B, size = p.shape[0], p.shape[2:]
    if any(s < 2 for s in size):
        raise ValueError("every extent must be at least 2")
    mu, ls = p[:, :3], p[:, 3:]
    deg = degree(size)
    V = int(np.prod(size))
    sig = np.sum(lam * deg * np.exp(ls) - ls) / (3 * B * V)
    gmu = np.zeros_like(mu)
    prec = []
    for a in range(3):
        ax = 2 + a
        hi = [slice(None)] * 5
        lo = [slice(None)] * 5
        hi[ax], lo[ax] = slice(1, None), slice(None, -1)
        df = mu[tuple(hi)] - mu[tuple(lo)]
        n_a = df.size
        assert n_a == 3 * B * V * (size[a] - 1) // size[a]
        prec.append(np.sum(df * df) / n_a)
        gmu[tuple(hi)] += df / n_a
        gmu[tuple(lo)] -= df / n_a
    loss = 1.5 * (sig + lam * (0.5 / 3) * ((prec[0] + prec[1]) + prec[2]))
    gp = np.concatenate([g * 0.5 * lam * gmu, g * (lam * deg * np.exp(ls) - 1.0) / (2 * B * V)], axis=1)
    return float(loss), gp


def sample_arbiter(params, eps, gz=None):
    """float64 arbiter of the sample: (z [B,3,*size], gparams [B,6,*size] or None)"""
    p = np.asarray(params, dtype=F32).astype(np.float64)
    e = np.asarray(eps, dtype=F32).astype(np.float64)
    mu, ls = p[:, :3], p[:, 3:]
    z = mu + np.exp(0.5 * ls) * e
    if gz is None:
        return z, None
    gz = np.asarray(gz, dtype=F32).astype(np.float64)
    return z, np.concatenate([gz, gz * 0.5 * np.exp(0.5 * ls) * e], axis=1)


# --------------------------------------------------------------------------- the same definition in plain fp32 torch (CPU): what sets the gates
_DEG = {}


def kl_torch(params, lam, dtype):
    """the definition as torch ops in `dtype` with autograd: params is a leaf tensor [B,6,*size]; returns the 0-dim loss"""
    import torch
    B, size = params.shape[0], tuple(params.shape[2:])
    mu, ls = params[:, :3], params[:, 3:]
    key = (size, str(params.device), dtype)
    if key not in _DEG:                                      # a resident buffer, as the reference keeps its degree matrix (self.D)
        _DEG.clear()
        _DEG[key] = torch.from_numpy(degree(size)).to(device=params.device, dtype=dtype)
    deg = _DEG[key]
    sig = (lam * deg * torch.exp(ls) - ls).mean()
    sm = 0
    for a in range(3):
        df = mu.narrow(2 + a, 1, size[a] - 1) - mu.narrow(2 + a, 0, size[a] - 1)
        sm = sm + (df * df).mean()
    return 0.5 * 3 * (sig + lam * (0.5 * sm / 3))


def sample_torch(params, eps):
    import torch
    return params[:, :3] + torch.exp(0.5 * params[:, 3:]) * eps


# --------------------------------------------------------------------------- whole model: composed from the oracle's pieces, not modified
def prob_forward_oracle(source, target, sd, noise, int_steps, int_downsize, bidir=False, nb_features=None):
    """`VxmDenseProbabilistic.forward` in training mode over state-dict tensors (float64 torch, autograd): (y_source, [y_target,] flow_params)"""
    import torch
    import torch.nn.functional as F
    from oracle import vxm_oracle as orc
    x = orc.unet_forward(torch.cat([source, target], dim=1), sd, nb_features=nb_features)
    mu = F.conv3d(x, sd["flow.weight"], sd["flow.bias"], padding=1)
    ls = F.conv3d(x, sd["flow_logsigma.weight"], sd["flow_logsigma.bias"], padding=1)
    flow_params = torch.cat([mu, ls], dim=1)
    z = mu + torch.exp(0.5 * ls) * noise
    pos = orc.resize_transform(z, int_downsize) if (int_steps > 0 and int_downsize > 1) else z
    neg = -pos if bidir else None

    def disp(v):
        if int_steps > 0:
            v = orc.vecint(v, int_steps)
            if int_downsize > 1:
                v = orc.resize_transform(v, 1 / int_downsize)
        return v
    y_source = orc.spatial_transformer(source, disp(pos))
    if bidir:
        return y_source, orc.spatial_transformer(target, disp(neg)), flow_params
    return y_source, flow_params
