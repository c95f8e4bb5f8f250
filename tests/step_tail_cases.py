"""The table of the end of the training step -- the flat Adam update, the MSE and Dice reductions, the loss combiner, vxm_add2,
vxm_fill_zero, vxm_lrelu_bwd -- shared by tests/test_gpu_step_tail.py (each kernel against float64), tests/test_cpu_step_tail.py (the
arbiters themselves) and tools/step_tail_gates.py (the gates, from the reference's own fp32 error on exactly these inputs)."""
import numpy as np

# ------------------------------------------------------------------ Adam kernel (vxm_adam_step / vxm_adam_step_dev)
ADAM_N = (1, 255, 256, 257, 4099, 327331)                  # block edges (256 threads) and the real bucket size
ADAM_K = 25
ADAM_HYPER = ((1e-4, 0.9, 0.999, 1e-8), (1e-2, 0.8, 0.95, 1e-6))            # lr, beta1, beta2, eps
ADAM_GSCALE = (1.0, 0.5, 1.0 / 3.0)
ADAM_CHECK = (1, 2, 3, ADAM_K)                             # steps after which p, exp_avg, exp_avg_sq are compared
ADAM_ZERO_EVERY = 97                                       # entries i % 97 == 96 have gradient 0 on every step
# late start: non-zero moments, the counter at 1000, three steps
ADAM_LATE = dict(n=4099, hyper=0, gscale=1.0, start=1000, steps=3)
ADAM_OFFSET_CASE = dict(n=4099, hyper=0, gscale=1.0)       # repeated with every pointer advanced by one float
SENTINELS = 64
SENTINEL = np.float32(-12345.678)


def f32(x):
    """the double that a Python float becomes when it crosses the C ABI as `float`"""
    return float(np.float32(x))


def adam_zero_mask(n):
    return np.arange(n) % ADAM_ZERO_EVERY == ADAM_ZERO_EVERY - 1


def adam_arrays(n, steps=ADAM_K, late=False):
    """p0 ~ N(0, 0.05^2) (the scale of the network's weights), gradients sign * 10^U(-10, 1) [steps, n] with exact zeros at the masked
    entries; late: moments of a run in progress (m of the gradients' scale, v its square, both 0 at the masked entries), else None"""
    rng = np.random.default_rng(3100 + n + (7 if late else 0))
    p0 = (0.05 * rng.standard_normal(n)).astype(np.float32)
    g = (rng.choice([-1.0, 1.0], size=(steps, n)) * 10.0 ** rng.uniform(-10.0, 1.0, size=(steps, n))).astype(np.float32)
    zero = adam_zero_mask(n)
    g[:, zero] = 0.0
    assert float(np.abs(g[:, ~zero]).min(initial=1.0)) >= 1e-12
    if not late:
        return p0, g, None, None
    m0 = (rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-6.0, 0.0, size=n)).astype(np.float32)
    v0 = (m0.astype(np.float64) ** 2 * rng.uniform(1.0, 4.0, size=n)).astype(np.float32)
    m0[zero] = 0.0
    v0[zero] = 0.0
    return p0, g, m0, v0


def adam_arbiter(p0, grads, hyper, gscale=1.0, m0=None, v0=None, start=0, check=None, rounded=True):
    """The float64 Adam recurrence (torch.optim.Adam: no amsgrad, no weight decay) over grads [K, n], counter starting at `start`.
    rounded: hyper-parameters and gscale first rounded to float32 -- what crosses the C ABI, so that the kernel is judged as the
    self-consistent Adam with beta = fl32(beta) that it is.  Returns {step: (p, exp_avg, exp_avg_sq)} for the steps in `check`
    (counted from 1 for the first gradient)."""
    lr, b1, b2, eps = (f32(x) for x in hyper) if rounded else hyper
    gs = f32(gscale) if rounded else float(gscale)
    p = np.asarray(p0, np.float64).copy()
    m = np.zeros_like(p) if m0 is None else np.asarray(m0, np.float64).copy()
    v = np.zeros_like(p) if v0 is None else np.asarray(v0, np.float64).copy()
    K = len(grads)
    check = (K,) if check is None else check
    out = {}
    for k in range(K):
        t = start + k + 1
        g = np.asarray(grads[k], np.float64) * gs
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        p = p - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
        if k + 1 in check:
            out[k + 1] = (p.copy(), m.copy(), v.copy())
    return out


def adam_torch(p0, grads, hyper, gscale, dtype, m0=None, v0=None, start=0, check=None):
    """torch.optim.Adam on CPU tensors of `dtype`, given the Python doubles of `hyper`; the gradient it sees is g * fl32(gscale) formed in
    `dtype`.  Returns what adam_arbiter returns."""
    import torch
    lr, b1, b2, eps = hyper
    p = torch.from_numpy(np.asarray(p0)).to(dtype).clone().requires_grad_()
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    if m0 is not None:
        opt.state[p] = {"step": torch.tensor(float(start)), "exp_avg": torch.from_numpy(np.asarray(m0)).to(dtype).clone(),
                        "exp_avg_sq": torch.from_numpy(np.asarray(v0)).to(dtype).clone()}
    gs = torch.tensor(f32(gscale), dtype=dtype)
    K = len(grads)
    check = (K,) if check is None else check
    out = {}
    for k in range(K):
        p.grad = torch.from_numpy(grads[k]).to(dtype) * gs
        opt.step()
        if k + 1 in check:
            st = opt.state[p]
            out[k + 1] = tuple(t.detach().numpy().astype(np.float64) for t in (p, st["exp_avg"], st["exp_avg_sq"]))
    return out


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def adam_errors(got, want, lr):
    """(max |p - p64| / lr, rel-L2 of exp_avg, rel-L2 of exp_avg_sq)"""
    return (float(np.abs(np.asarray(got[0], np.float64) - want[0]).max() / lr), rel_l2(got[1], want[1]), rel_l2(got[2], want[2]))


# ------------------------------------------------------------------ the whole model, several optimiser steps
TRAJ_SHAPE = (32, 32, 32)
TRAJ_INT_STEPS, TRAJ_INT_DOWNSIZE = 3, 2
TRAJ_SEED, TRAJ_FLOW_STD = 7, 0.05
TRAJ_LR = 1e-3
TRAJ_K = 4
# (source, target) of every step.  The seeds decide whether the REFERENCE is a yardstick at all: over nine such sets its fp32 and fp64
# evaluations ended 6e-4 .. 8e-2 apart (worst tensor, rel-L2 after 4 steps) -- a max-pool tie or a LeakyReLU sign that the two precisions
# resolve differently moves a gradient by percent.  This set is one where they stay together (tools/step_tail_gates.py asserts < 1e-2).
TRAJ_IMAGE_SEEDS = ((4201, 4202), (4203, 4204), (4205, 4206), (4207, 4208))
TRAJ_GRID = 6


def smooth_image(seed, shape=TRAJ_SHAPE, grid=TRAJ_GRID):
    """a U[0, 1) grid of `grid`^3 nodes interpolated trilinearly (corners aligned) to `shape`: [1, 1, *shape] float32"""
    rng = np.random.default_rng(seed)
    x = rng.random((grid,) * len(shape))
    for ax, n in enumerate(shape):
        c = np.arange(n) * ((grid - 1) / (n - 1))
        lo = np.minimum(np.floor(c).astype(int), grid - 2)
        f = (c - lo).reshape([-1 if a == ax else 1 for a in range(len(shape))])
        x = np.take(x, lo, axis=ax) * (1.0 - f) + np.take(x, lo + 1, axis=ax) * f
    return x[None, None].astype(np.float32)


def traj_pairs():
    return [(smooth_image(a), smooth_image(b)) for a, b in TRAJ_IMAGE_SEEDS]


def traj_oracle(dtype):
    """TRAJ_K steps of the reference's loop (oracle.train_step_loss: NCC + Grad('l2', x2), lambda 1; torch.optim.Adam) in `dtype` on the
    CPU.  Returns (losses [K], {name: (p_K - p_0, exp_avg, exp_avg_sq)} as float64 arrays) in state-dict order."""
    import torch
    from oracle import vxm_oracle as orc
    sd0 = orc.seeded_state_dict(TRAJ_SHAPE, seed=TRAJ_SEED, flow_std=TRAJ_FLOW_STD)
    sd = {k: v.to(dtype).clone().requires_grad_() for k, v in sd0.items()}
    opt = torch.optim.Adam(list(sd.values()), lr=TRAJ_LR)
    losses = []
    for src, trg in traj_pairs():
        opt.zero_grad()
        loss, _ = orc.train_step_loss(torch.from_numpy(src).to(dtype), torch.from_numpy(trg).to(dtype), sd, "ncc", 1.0,
                                      int_steps=TRAJ_INT_STEPS, int_downsize=TRAJ_INT_DOWNSIZE)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    out = {}
    for k, p in sd.items():
        st = opt.state[p]
        out[k] = (p.detach().double().numpy() - sd0[k].double().numpy(), st["exp_avg"].double().numpy(), st["exp_avg_sq"].double().numpy())
    return losses, out


# ------------------------------------------------------------------ MSE
MSE_N = (1, 255, 257, 2049, 2 ** 21 + 77)                  # the last one is past 1024 x 2048 (forward grid) and 8192 x 256 (backward grid)


def mse_arrays(n):
    rng = np.random.default_rng(3300 + n % 1000)
    return rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)


def mse_reference(a, b, dtype):
    """(loss, ga, gb) of oracle.mse_loss evaluated in `dtype` on the CPU"""
    import torch
    from oracle import vxm_oracle as orc
    ta, tb = (torch.from_numpy(x).to(dtype).requires_grad_() for x in (a, b))
    loss = orc.mse_loss(ta, tb)
    loss.backward()
    return float(loss.detach()), ta.grad.double().numpy(), tb.grad.double().numpy()


# ------------------------------------------------------------------ Dice
DICE_CASES = ((1, 1, 1), (2, 3, 255), (1, 5, 257), (2, 4, 70001), (1, 2, 2 ** 21 + 77))       # (B, C, V); 70001 > 256 blocks x 256
DICE_CLAMP = 1e-5
DICE_SUBCLAMP_SUM = 1e-6


def dice_arrays(case):
    """y_true binary, y_pred in [0, 1), [B, C, V].  Channel 1 (where there is one) is absent from both: the clamp branch with a zero
    numerator.  Channel 2 (where there is one) holds positive entries in both, scaled per case so that sum(y_true + y_pred) = 1e-6 for
    every batch entry: below the 1e-5 clamp at every V, with a non-zero numerator."""
    B, C, V = case
    rng = np.random.default_rng(3400 + DICE_CASES.index(tuple(case)))
    yt = (rng.random((B, C, V)) < 0.4).astype(np.float64)
    yp = rng.random((B, C, V))
    if case == (1, 1, 1):
        yt[...] = 1.0
    if C > 1:
        yt[:, 1] = 0.0
        yp[:, 1] = 0.0
    if C > 2:
        u, w = rng.uniform(0.1, 1.0, size=(B, V)), rng.uniform(0.1, 1.0, size=(B, V))
        s = DICE_SUBCLAMP_SUM / (u + w).sum(axis=1, keepdims=True)
        yt[:, 2], yp[:, 2] = u * s, w * s
    return yt.astype(np.float32), yp.astype(np.float32)


def dice_reference(yt, yp, dtype):
    """(loss, g_true, g_pred) of oracle.dice_loss evaluated in `dtype` on the CPU"""
    import torch
    from oracle import vxm_oracle as orc
    tt, tp = (torch.from_numpy(x).to(dtype).requires_grad_() for x in (yt, yp))
    loss = orc.dice_loss(tt, tp)
    loss.backward()
    return float(loss.detach()), tt.grad.double().numpy(), tp.grad.double().numpy()


# ------------------------------------------------------------------ loss combiner, add2, fill_zero, lrelu_bwd
LOSS_TERMS_MAX = 8                                         # VXM_LOSS_TERMS_MAX of include/vxm_hip.h


def combine_arrays(n):
    rng = np.random.default_rng(3500 + n)
    return rng.standard_normal(n).astype(np.float32), rng.uniform(0.01, 3.0, size=n).astype(np.float32)


def combine_reference(terms, weights, running=None):
    """scripts/torch/train.py:205-212 in float32, one rounding per operation: returns (total, running after the call)"""
    total = np.float32(0.0)
    run = None if running is None else np.array(running, np.float32)
    for i in range(len(terms)):
        cur = np.float32(terms[i]) * np.float32(weights[i])
        total = np.float32(total + cur)
        if run is not None:
            run[i] = np.float32(run[i] + cur)
    if run is not None:
        run[len(terms)] = np.float32(run[len(terms)] + total)
    return total, run


ADD2_N = (1, 3, 4, 5, 1027, 2 ** 20 + 3)
FILL_BYTES = (0, 4, 4099 * 4)
LRELU_CASE = dict(B=2, C=3, V=37, pad=(5, 11, 3), slope=0.2)     # batch strides C * V + pad of g, y, dz: all different, all > C * V
