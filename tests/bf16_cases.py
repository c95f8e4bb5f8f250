"""Case table, input generators and arbiters of the bit-exact bf16 conv-engine tests (tests/test_cpu_bf16.py, tests/test_gpu_bf16_exact.py).

The engine (voxelmorph_amd/csrc/conv_bf16.hip) multiplies bf16 operands exactly and accumulates in fp32.  Every input here is a small
integer in [-r, r] times a power of two, sized so that every partial sum of a case is an integer (times that power) below 2^24: every
fp32 accumulation is then exact in ANY order and on any tile shape, the value in front of the final rounding is a known integer, and the
stored value is its round-to-nearest-even bf16.  Kernels are therefore compared with `array_equal`, not with a tolerance.

No GPU is needed to import this module.  Layout helpers, the tap-by-tap arbiters (27 shifted channel contractions on a zero-padded copy:
deliberately not `F.conv3d`, which tests/test_cpu_bf16.py compares them with), and a Python restatement of the launch geometry
(`conv_geometry`, `bwb_tasks`) of conv_bf16.hip.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

TWO24 = 1 << 24
CUS_REF = 256            # compute units the quoted (NBLK, nseg, seg_len) were computed for
BF = torch.bfloat16


# --------------------------------------------------------------------------------------------------------------------------------
# layouts and small helpers
# --------------------------------------------------------------------------------------------------------------------------------
def pad16(c):
    return (c + 15) // 16 * 16


def blocked(x, cblk=None):
    """planar [B][C][D][H][W] (any float type, bf16-representable values) -> blocked bf16 [B][cblk/8][D][H][W][8], zero-padded channels"""
    B, C = x.shape[:2]
    dims = tuple(x.shape[2:])
    cblk = cblk or pad16(C)
    xp = torch.zeros((B, cblk) + dims, dtype=torch.float32)
    xp[:, :C] = x.to(torch.float32)
    return xp.reshape((B, cblk // 8, 8) + dims).permute(0, 1, 3, 4, 5, 2).contiguous().to(BF)


def planar(xb):
    """blocked [B][CB][D][H][W][8] -> planar [B][8 CB][D][H][W], same dtype"""
    B, CB, D, H, W, _ = xb.shape
    return xb.permute(0, 1, 5, 2, 3, 4).reshape(B, CB * 8, D, H, W)


def bits(t):
    """the 16 bits of every bf16 element (so that -0 and the rounding direction are compared)"""
    return t.contiguous().view(torch.int16)


def rne(v):
    return v.to(torch.float32).to(BF)


def is_bf16(t):
    t = t.to(torch.float32)
    return bool(torch.equal(t.to(BF).to(torch.float32), t))


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def ints(rng, shape, r, exp):
    """integers in [-r, r] times 2^exp, float64"""
    return torch.from_numpy(rng.integers(-r, r + 1, size=shape).astype(np.float64)) * 2.0 ** exp


def rounding_shares(v):
    """(share of fp32 values that a bf16 store has to round, share that are exact ties)"""
    u = v.to(torch.float32).contiguous().view(torch.int32) & 0xFFFF
    return float((u != 0).double().mean()), float((u == 0x8000).double().mean())


# --------------------------------------------------------------------------------------------------------------------------------
# arbiters
# --------------------------------------------------------------------------------------------------------------------------------
def conv_taps(x, wop, dtype=torch.float64):
    """z[b][o][v] = sum_t sum_i wop[o][i][t] x[b][i][v + t - 1]: 27 shifted channel contractions on a zero-padded copy.
    x [B][Ci][D][H][W], wop [Co][Ci][27] (tap t = 9 kd + 3 kh + kw)"""
    x, wop = x.to(dtype), wop.to(dtype)
    B, Ci, D, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    z = torch.zeros((B, wop.shape[0], D * H * W), dtype=dtype)
    for t in range(27):
        kd, kh, kw = t // 9, (t // 3) % 3, t % 3
        xs = xp[:, :, kd:kd + D, kh:kh + H, kw:kw + W].reshape(B, Ci, -1)
        z += torch.matmul(wop[:, :, t], xs)
    return z.reshape(B, -1, D, H, W)


def _f32(s):
    return torch.tensor(s, dtype=torch.float32)


def lrelu_grad(m, slope):
    """the engine's LeakyReLU'(m): 1 where m > 0, else the slope (so: -0, +0 and NaN take the slope)"""
    return torch.where(m.to(torch.float32) > 0, _f32(1.0), _f32(slope))


def epilogue(z, bias, slope, mask, mask_slope):
    """bias, LeakyReLU (`z > 0 ? z : fp32(z) * fp32(slope)`: one fp32 rounding), optional LeakyReLU' mask; the fp32 value in front of
    the store (blocked outputs round it once more, to bf16; the planar head stores it)"""
    v = z.to(torch.float32)
    if bias is not None:
        v = v + bias.to(torch.float32).view(1, -1, 1, 1, 1)
    v = torch.where(v > 0, v, v * _f32(slope))
    if mask is not None:
        v = v * lrelu_grad(mask, mask_slope)
    return v


def fused_up(z, mask_low, mask_slope):
    """vxm_bf16_conv_bwd_data_up after the convolution: every full-resolution value rounded to bf16, the 8 children summed exactly,
    the low-resolution mask, (the caller rounds to bf16 again)"""
    g = rne(z).to(torch.float64)
    B, C, D, H, W = g.shape
    s = g.reshape(B, C, D // 2, 2, H // 2, 2, W // 2, 2).sum(dim=(3, 5, 7)).to(torch.float32)
    if mask_low is not None:
        s = s * lrelu_grad(mask_low, mask_slope)
    return s


def wop_forward(w, ci_lo, ci_n, out_pad=None):
    """Wop[o][i][t] = w[o][ci_lo + i][t]; rows beyond Cw_out are zero"""
    co = w.shape[0]
    op = torch.zeros((out_pad or co, ci_n, 27), dtype=w.dtype)
    op[:co] = w.reshape(co, -1, 27)[:, ci_lo:ci_lo + ci_n]
    return op


def wop_flipped(w, ci_lo, ci_n, out_pad=None, in_pad=None):
    """Wop[o][i][t] = w[i][ci_lo + o][26 - t] (backward-data onto input channels [ci_lo, ci_lo + ci_n)); rows / columns beyond are zero"""
    co = w.shape[0]
    op = torch.zeros((out_pad or ci_n, in_pad or co, 27), dtype=w.dtype)
    op[:ci_n, :co] = w.reshape(co, -1, 27)[:, ci_lo:ci_lo + ci_n].permute(1, 0, 2).flip(2)
    return op


def virtual_input(x0, up0, x1):
    x = F.interpolate(x0, scale_factor=2, mode="nearest") if up0 else x0
    return x if x1 is None else torch.cat([x, x1], 1)


def wgrad_taps(x, dz, dtype=torch.float64):
    """gw[o][i][t] = sum_{b, v} dz[b][o][v] x[b][i][v + t - 1] as 27 per-tap matrix products, gb[o] = sum dz.  x is the virtual concat."""
    x, dz = x.to(dtype), dz.to(dtype)
    B, Ci, D, H, W = x.shape
    Co = dz.shape[1]
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    Z = dz.permute(1, 0, 2, 3, 4).reshape(Co, -1)
    gw = torch.zeros((Co, Ci, 27), dtype=dtype)
    for t in range(27):
        kd, kh, kw = t // 9, (t // 3) % 3, t % 3
        X = xp[:, :, kd:kd + D, kh:kh + H, kw:kw + W].permute(1, 0, 2, 3, 4).reshape(Ci, -1)
        gw[:, :, t] = Z @ X.T
    return gw.reshape(Co, Ci, 3, 3, 3), Z.sum(1)


# --------------------------------------------------------------------------------------------------------------------------------
# launch geometry, restated from conv_bf16.hip
# --------------------------------------------------------------------------------------------------------------------------------
def conv_geometry(cin_blocked, cout, vol, B, planar_out=False):
    """k_bf16_conv: NCT, ROWS, tiles, Q (16-channel chunks of the input), G (output-channel groups)"""
    nct = 1 if (planar_out or cout <= 16) else 2
    rows = 8 if nct == 1 else 6
    D, H, W = vol
    ntiles = B * ((D + 7) // 8) * ((H + rows - 1) // rows) * ((W + 15) // 16)
    return dict(NCT=nct, ROWS=rows, ntiles=ntiles, Q=cin_blocked // 16, G=(cout + 16 * nct - 1) // (16 * nct))


def bwb_tasks(Q, B, D, H, W, cus=CUS_REF):
    """`bwb_tasks` of conv_bf16.hip: (NBLK, nseg, seg_len) of k_bf16_conv_bwd_weight on a device with `cus` compute units"""
    nd, nh, nw = (D + 1) // 2, (H + 7) // 8, (W + 31) // 32
    ncol = B * nh * nw
    nb = max(cus // Q, 1)
    nseg = max(min((4 * nb + ncol - 1) // ncol, nd), 1)
    seg_len = (nd + nseg - 1) // nseg
    nseg = (nd + seg_len - 1) // seg_len
    return min(nb, ncol * nseg), nseg, seg_len


def workspace_nblk(nbytes, Q, NCO):
    """NBLK from vxm_bf16_conv_bwd_weight_workspace_bytes: NBLK x Q x 2 depth slices x 28 taps x 16 NCO x 16 floats"""
    per = Q * 2 * 28 * 16 * NCO * 16 * 4
    assert nbytes % per == 0
    return nbytes // per


def default_grid_w(cus):
    """W of the default-grid case (16 -> 16, B = 1, 64 x 64 x W): 64 ceil(W / 16) tiles, 128 more than the 2 x CUs blocks of the default grid"""
    return 16 * (2 * cus // 64 + 2)


# --------------------------------------------------------------------------------------------------------------------------------
# forward / backward-data operators
# --------------------------------------------------------------------------------------------------------------------------------
def _op(name, c0, up0, c1, cout, vol, B, r, ex, ew, slope, cw_in=None, planar_out=False, multi=False, note="", rdz=None):
    return dict(name=name, c0=c0, up0=up0, c1=c1, cout=cout, vol=vol, B=B, r=r, rdz=rdz or r, ex=ex, ew=ew, slope=slope, cw_in=cw_in or (c0 + c1),
                planar=planar_out, multi=multi, note=note)


OPS = [
    _op("centre_tap", 16, False, 0, 16, (1, 1, 1), 1, 24, 0, 0, 0.25, note="centre tap only"),
    _op("past_tile", 16, False, 0, 16, (9, 7, 17), 2, 8, -3, 2, 0.2, note="one voxel past a tile in D and W, H below a tile"),
    _op("six_rows", 16, False, 0, 32, (7, 13, 15), 1, 8, 1, -4, 0.25, note="the 6-row instance, two tiles and one row"),
    _op("two_chunks", 32, False, 0, 16, (8, 8, 16), 1, 6, -9, 6, 0.2, note="exactly one tile, two chunks"),
    _op("three_chunks", 32, True, 16, 32, (16, 12, 32), 1, 4, 6, -9, 0.25, rdz=8, note="three chunks"),
    _op("up_cat_32", 32, True, 32, 32, (4, 6, 34), 1, 4, -2, -2, 0.2, rdz=8),
    _op("coarsest", 32, False, 0, 32, (2, 2, 2), 1, 8, 0, -1, 0.25),
    _op("first_layer", 16, False, 0, 16, (9, 7, 17), 2, 24, -5, 0, 0.2, cw_in=2, rdz=3, note="2 real channels in a 16-channel blocked tensor"),
    _op("head_1", 16, False, 0, 1, (9, 7, 18), 2, 8, 0, -6, 0.2, planar_out=True, rdz=32),
    _op("head_2", 16, False, 0, 2, (9, 7, 18), 2, 8, -1, 0, 0.25, planar_out=True, rdz=24),
    _op("head_3", 16, False, 0, 3, (9, 7, 18), 2, 8, 2, -3, 1.0, planar_out=True, rdz=16),
    _op("two_groups", 16, False, 0, 48, (8, 8, 16), 2, 8, 0, 0, 0.25, note="G = 2, second group half empty, pb < CBo"),
    _op("mt_16_16", 16, False, 0, 16, (16, 32, 64), 2, 8, -1, 1, 0.2, multi=True, note="64 tiles"),
    _op("mt_16_32_odd", 16, False, 0, 32, (17, 26, 70), 2, 8, 3, -7, 0.25, multi=True, note="150 tiles, not a multiple of 8"),
    _op("mt_q3", 32, True, 16, 32, (16, 24, 64), 2, 4, 0, -2, 0.25, multi=True, rdz=8, note="64 tiles, Q = 3, weights re-fetched per chunk"),
    _op("mt_q1", 16, False, 0, 32, (16, 24, 64), 2, 8, -4, 4, 0.2, multi=True, note="64 tiles, Q = 1, weights stay in LDS"),
    _op("mt_head_3", 16, False, 0, 3, (16, 32, 64), 2, 8, 0, 0, 1.0, planar_out=True, multi=True, rdz=16, note="64 tiles"),
]
OP_BY_NAME = {o["name"]: o for o in OPS}


def op_tensors(op):
    """seeded: x0 (at its own resolution), x1, w [Cw_out][Cw_in][3][3][3], bias, all float64 and bf16-representable (bias: fp32-exact)"""
    rng = _rng("op:" + op["name"])
    D, H, W = op["vol"]
    lo = (D // 2, H // 2, W // 2)
    B, r = op["B"], op["r"]
    x0 = ints(rng, (B, op["c0"]) + (lo if op["up0"] else op["vol"]), r, op["ex"])
    x1 = ints(rng, (B, op["c1"]) + op["vol"], r, op["ex"]) if op["c1"] else None
    w = ints(rng, (op["cout"], op["cw_in"], 3, 3, 3), r, op["ew"])
    bias = ints(rng, (op["cout"],), 3 * r, op["ex"] + op["ew"])
    return x0, x1, w, bias


def conv_runs(op):
    """the launches one operator gives: forward, and its flipped operator onto each of its segments; each with and without the fused mask
    where the entry point takes one.  A run: (id, dir, masked)."""
    runs = [("fwd", False)] + ([] if op["planar"] else [("fwd", True)])
    runs += [("flip0", False), ("flip0", True)]
    if op["c1"]:
        runs += [("flip1", False), ("flip1", True)]
    return runs


def other_slope(s):
    return 0.25 if s == 0.2 else 0.2


def build_run(op, direction, masked):
    """Everything one launch needs and the arbiter's inputs.  Returns a dict:
       x0, x1 planar float64 [B][C blocked][..] (x0 at its own resolution), C0, up0, C1, pack = (ci_lo, ci_n, flip), w, bias, cout (the
       Cout argument), planar, slope, mask [B][cout][vol] or None, mask_slope, wop [cout padded][C0 + C1][27], bound (integer units), n_real (output channels the operator has)"""
    x0, x1, w, bias = op_tensors(op)
    rng = _rng("run:%s:%s" % (op["name"], direction))
    vol, B, r = op["vol"], op["B"], op["r"]
    cin_w, cout_w = op["cw_in"], op["cout"]
    if direction == "fwd":
        c0, c1 = op["c0"], op["c1"]
        X0 = torch.zeros((B, c0) + tuple(x0.shape[2:]), dtype=torch.float64)
        X0[:, :x0.shape[1]] = x0
        if cin_w < c0 + c1:                       # the first layer: the blocked input carries channels the operator does not read
            X0[:, cin_w:] = ints(rng, (B, c0 - cin_w) + tuple(x0.shape[2:]), r, op["ex"])
        cout = cout_w
        out_pad = cout if op["planar"] else pad16(cout)
        wop = torch.zeros((out_pad, c0 + c1, 27), dtype=torch.float64)
        wop[:, :cin_w] = wop_forward(w, 0, cin_w, out_pad)
        run = dict(x0=X0, x1=x1, C0=c0, up0=op["up0"], C1=c1, pack=(0, cin_w, False), bias=bias, cout=cout, planar=op["planar"],
                   slope=op["slope"], wop=wop, bound=27 * cin_w * r * r + 3 * r)
    else:
        seg = 0 if direction == "flip0" else 1
        ci_lo, ci_n = (0, min(op["c0"], cin_w)) if seg == 0 else (op["c0"], op["c1"])
        cdz = pad16(cout_w)
        dz = torch.zeros((B, cdz) + vol, dtype=torch.float64)
        rdz = op["rdz"]
        dz[:, :cout_w] = ints(rng, (B, cout_w) + vol, rdz, op["ex"])
        if cout_w < cdz:                          # the flow head: the blocked gradient carries channels the operator does not read
            dz[:, cout_w:] = ints(rng, (B, cdz - cout_w) + vol, rdz, op["ex"])
        cout = pad16(ci_n)
        run = dict(x0=dz, x1=None, C0=cdz, up0=False, C1=0, pack=(ci_lo, ci_n, True), bias=None, cout=cout, planar=False, slope=1.0,
                   wop=wop_flipped(w, ci_lo, ci_n, cout, cdz), bound=27 * cout_w * r * rdz)
    run.update(w=w, vol=vol, B=B, mask=None, mask_slope=1.0, op=op, dir=direction, n_real=run["cout"] if direction == "fwd" else run["pack"][1])
    if masked:
        run["mask"] = ints(rng, (B, run["cout"]) + vol, 2, 0)
        run["mask_slope"] = other_slope(op["slope"]) if direction == "fwd" else (op["slope"] if op["slope"] != 1.0 else 0.2)
    return run


def run_reference(run, dtype=torch.float64):
    """(z, v): the exact convolution and the fp32 value in front of the store"""
    x = virtual_input(run["x0"], run["up0"], run["x1"])
    z = conv_taps(x, run["wop"], dtype)
    return z, epilogue(z, run["bias"], run["slope"], run["mask"], run["mask_slope"])


CONV_IDS = [(o["name"], d, m) for o in OPS if not o["multi"] for (d, m) in conv_runs(o)]
MULTI_IDS = [(o["name"], d, m) for o in OPS if o["multi"] for (d, m) in conv_runs(o)]


def run_id(t):
    return "%s-%s%s" % (t[0], t[1], "-mask" if t[2] else "")


def default_grid_op(cus):
    return _op("mt_default_grid", 16, False, 0, 16, (64, 64, default_grid_w(cus)), 1, 8, 0, 0, 0.2, multi=True,
               note="more tiles than the 2 x CUs blocks of the default grid")


# ---- fused backward-data onto an upsampled segment (vxm_bf16_conv_bwd_data_up): Conv3d(cup + 16 -> cdz), segment 0 = upsampled
def _fu(name, cdz, cup, vol, B, r, ex, ew, slope, multi=False):
    return dict(name=name, cdz=cdz, cup=cup, vol=vol, B=B, r=r, ex=ex, ew=ew, slope=slope, multi=multi)


FUSED = [
    _fu("fu_32_32", 32, 32, (12, 6, 20), 2, 6, 0, 0, 0.2),
    _fu("fu_32_16", 32, 16, (8, 8, 16), 2, 6, -9, 3, 0.25),
    _fu("fu_16_32", 16, 32, (18, 10, 36), 2, 8, 6, -8, 0.2),
    _fu("fu_coarsest", 32, 32, (2, 2, 2), 2, 8, 0, 0, 0.25),
    _fu("fu_mt_32_32", 32, 32, (16, 24, 64), 2, 6, -1, -1, 0.2, multi=True),
]
FUSED_BY_NAME = {f["name"]: f for f in FUSED}
FUSED_IDS = [(f["name"], m) for f in FUSED for m in (False, True)]


def build_fused(fu, masked):
    rng = _rng("fused:" + fu["name"])
    D, H, W = fu["vol"]
    low = (D // 2, H // 2, W // 2)
    B, r = fu["B"], fu["r"]
    w = ints(rng, (fu["cdz"], fu["cup"] + 16, 3, 3, 3), r, fu["ew"])
    dz = ints(rng, (B, fu["cdz"]) + fu["vol"], r, fu["ex"])
    mask = ints(rng, (B, fu["cup"]) + low, 2, 0) if masked else None
    return dict(w=w, dz=dz, mask=mask, mask_slope=fu["slope"], wop=wop_flipped(w, 0, fu["cup"]), bound=27 * fu["cdz"] * r * r, low=low,
                vol=fu["vol"], B=B, cdz=fu["cdz"], cup=fu["cup"])


def fused_reference(fr, dtype=torch.float64):
    z = conv_taps(fr["dz"], fr["wop"], dtype)
    return z, fused_up(z, fr["mask"], fr["mask_slope"])


# ---- impulse case: one 1.0 per input channel, at voxels whose 3 x 3 x 3 boxes do not meet (steps of 4, 3, 4 along D, H, W)
IMPULSE_VOL, IMPULSE_B = (9, 7, 17), 1
IMPULSE_OPS = [(16, 16), (32, 16), (16, 32)]           # (Cw_out, Cw_in)


def impulse_positions(n):
    pos = [(d, h, w) for d in (0, 4, 8) for h in (0, 3, 6) for w in (0, 4, 8, 12, 16)]
    order = _rng("impulse").permutation(len(pos))
    # the first ones by hand: the volume's two opposite corners, the far side of a tile face (d = 8, w = 16), an interior voxel
    first = [(0, 0, 0), (8, 6, 16), (4, 3, 8), (8, 3, 4), (4, 6, 16), (0, 3, 12)]
    rest = [pos[i] for i in order if pos[i] not in first]
    return (first + rest)[:n]


def impulse_weights(cout, cin):
    """non-integer fp32 weights, all 27 taps different, with bf16 ties (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6), values that round up a
    binade (2 - 2^-10 -> 2) and their negatives sprinkled in"""
    rng = _rng("impulse_w:%d:%d" % (cout, cin))
    w = rng.standard_normal((cout, cin, 27)).astype(np.float32)
    special = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 2 - 2.0 ** -10, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), -(4 - 2.0 ** -9),
                        0.5 + 2.0 ** -9, 0.5 + 3 * 2.0 ** -9], np.float32)
    flat = w.reshape(-1)
    idx = rng.permutation(flat.size)[:flat.size // 3]
    flat[idx] = special[np.arange(idx.size) % special.size] * (1 + (np.arange(idx.size) // special.size % 4)).astype(np.float32)
    return torch.from_numpy(w.reshape(cout, cin, 3, 3, 3))


def impulse_case(cout_w, cin_w, flip):
    """x (planar, float64), the expected planar output as bf16 bits written out tap by tap (no convolution is evaluated), w fp32"""
    w = impulse_weights(cout_w, cin_w)
    wr = rne(w).to(torch.float64).reshape(cout_w, cin_w, 27)
    n_in, n_out = (cout_w, cin_w) if flip else (cin_w, cout_w)
    D, H, W = IMPULSE_VOL
    pos = impulse_positions(n_in)
    x = torch.zeros((IMPULSE_B, n_in, D, H, W), dtype=torch.float64)
    want = torch.zeros((IMPULSE_B, n_out, D, H, W), dtype=torch.float64)
    for i, (pd, ph, pw) in enumerate(pos):
        x[0, i, pd, ph, pw] = 1.0
        for t in range(27):
            kd, kh, kw = t // 9, (t // 3) % 3, t % 3
            d, h, ww = pd - (kd - 1), ph - (kh - 1), pw - (kw - 1)          # the output voxel whose tap t reads the impulse
            if 0 <= d < D and 0 <= h < H and 0 <= ww < W:
                want[0, :, d, h, ww] = wr[i, :, 26 - t] if flip else wr[:, i, t]
    return x, want, w


# --------------------------------------------------------------------------------------------------------------------------------
# weight-gradient cases
# --------------------------------------------------------------------------------------------------------------------------------
def _wg(name, c0, up0, c1, cdz, vol, B, r, ex, edz, cin_w=None, cout_w=None, big=False, note=""):
    return dict(name=name, c0=c0, up0=up0, c1=c1, cdz=cdz, vol=vol, B=B, r=r, ex=ex, edz=edz, cin_w=cin_w or (c0 + c1), cout_w=cout_w or cdz,
                big=big, note=note)


WGRAD = [
    _wg("wg_odd_d", 16, False, 0, 16, (3, 5, 7), 1, 8, 0, 0, note="odd D: the zlast slot"),
    _wg("wg_one_tile", 16, False, 0, 16, (2, 8, 32), 1, 8, -9, 6, note="one tile"),
    _wg("wg_past_tile", 16, False, 0, 16, (5, 9, 33), 2, 8, 3, -3, note="one voxel past a tile on every axis"),
    _wg("wg_up_cat", 32, True, 16, 32, (6, 10, 36), 2, 8, -2, 1),
    _wg("wg_cin2", 16, False, 0, 16, (4, 6, 10), 2, 8, 0, -1, cin_w=2, note="Cin_w = 2 of 16"),
    _wg("wg_cout3", 16, False, 0, 16, (4, 6, 10), 2, 8, 1, 0, cout_w=3, note="Cout_w = 3 of 16"),
    _wg("wg_ring", 32, False, 16, 32, (47, 60, 120), 2, 2, -1, 2, big=True,
        note="the 6-slot ring wraps, loads in flight, NBLK % 8 != 0, the last tile's second slice beyond D"),
    _wg("wg_task_rr", 16, False, 0, 16, (128, 128, 128), 1, 1, 0, 0, big=True, note="task_rr: D H W >= 2^21 and NBLK % 8 == 0"),
]
WGRAD_BY_NAME = {c["name"]: c for c in WGRAD}
# (NBLK, nseg, seg_len) on 256 compute units
WGRAD_TASKS_256 = {"wg_ring": (85, 6, 4), "wg_task_rr": (256, 16, 4)}


def wgrad_tensors(c):
    """x0 (own resolution), x1, dz: planar float64 with ALL blocked channels filled (those beyond Cin_w / Cout_w are read by the kernel and
    must not reach gw / gb)"""
    rng = _rng("wg:" + c["name"])
    D, H, W = c["vol"]
    lo = (D // 2, H // 2, W // 2)
    x0 = ints(rng, (c["B"], c["c0"]) + (lo if c["up0"] else c["vol"]), c["r"], c["ex"])
    x1 = ints(rng, (c["B"], c["c1"]) + c["vol"], c["r"], c["ex"]) if c["c1"] else None
    dz = ints(rng, (c["B"], c["cdz"]) + c["vol"], c["r"], c["edz"])
    return x0, x1, dz


def wgrad_bound(c):
    D, H, W = c["vol"]
    return c["B"] * D * H * W * c["r"] * c["r"]


def wgrad_reference(c, dtype=None):
    x0, x1, dz = wgrad_tensors(c)
    gw, gb = wgrad_taps(virtual_input(x0, c["up0"], x1), dz, dtype or (torch.float32 if c["big"] else torch.float64))
    return gw[:c["cout_w"], :c["cin_w"]].contiguous(), gb[:c["cout_w"]].contiguous()


# --------------------------------------------------------------------------------------------------------------------------------
# elementwise kernels: special values and plain references
# --------------------------------------------------------------------------------------------------------------------------------
def special_f32():
    """fp32 bit patterns a bf16 conversion can get wrong: ties to even both ways, the largest finite bf16, values that must round to
    +-Inf, fp32 and bf16 denormals, +-0, +-Inf, NaN (quiet, and one whose payload lies in the dropped half only)"""
    pos = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3FFF8000, 0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF,
           0x00000001, 0x00008000, 0x00008001, 0x00018000, 0x00400000, 0x007F8000, 0x007FFFFF, 0x00000000, 0x7F800000,
           0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x40490FDB, 0x3EAAAAAB]
    u = np.array(pos + [p | 0x80000000 for p in pos], dtype=np.uint32)
    return torch.from_numpy(u.view(np.float32).copy())


def same_or_both_nan(got, want):
    """bit equality where the reference is a number, NaN where it is NaN (payloads are not compared)"""
    nan = torch.isnan(want.to(torch.float32))
    g, w = (bits(got), bits(want)) if want.dtype == BF else (got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))
    return bool(torch.equal(torch.isnan(got.to(torch.float32)), nan) and torch.equal(g[~nan], w[~nan]))


def pool_inputs(vol, B=2, C=16, nan_every=37):
    """small integers (many ties inside the 2 x 2 x 2 blocks) with NaN at every child position of some block"""
    rng = _rng("pool:%s" % (vol,))
    x = ints(rng, (B, C) + vol, 3, 0).to(torch.float32)
    if nan_every:
        flat = x.reshape(-1)
        flat[torch.arange(5, flat.numel(), nan_every)] = float("nan")
        flat[torch.arange(6, flat.numel(), 16 * nan_every)] = float("nan")      # two NaN next to each other: the LAST one is the arg-max
    return x


def maxpool_children(x):
    """[8][B][C][D/2][H/2][W/2]: child k = 4 kd + 2 kh + kw of every whole 2 x 2 x 2 block (odd extents: the last plane / row / column is dropped)"""
    D2, H2, W2 = (s // 2 for s in x.shape[2:])
    return torch.stack([x[:, :, (k >> 2) & 1:2 * D2:2, (k >> 1) & 1:2 * H2:2, (k & 1):2 * W2:2] for k in range(8)])


def maxpool_reference(x):
    """ATen's rule, child by child: a later child replaces the maximum if `(v > m) || isnan(v)`.  Returns (max, arg)"""
    ch = maxpool_children(x)
    m, arg = ch[0].clone(), torch.zeros(ch[0].shape, dtype=torch.long)
    for k in range(1, 8):
        take = (ch[k] > m) | torch.isnan(ch[k])
        m = torch.where(take, ch[k], m)
        arg = torch.where(take, torch.full_like(arg, k), arg)
    return m, arg


def maxpool_bwd_reference(x, gp, gs, slope):
    """dz[child] = ((child is the arg-max ? gpool : 0) + gskip[child]) * LeakyReLU'(x[child]) in fp32 (even extents); the fp32 value"""
    _, arg = maxpool_reference(x)
    out = torch.zeros_like(x, dtype=torch.float32)
    for k in range(8):
        g = torch.where(arg == k, gp.to(torch.float32), _f32(0.0))
        out[:, :, (k >> 2) & 1::2, (k >> 1) & 1::2, (k & 1)::2] = g
    if gs is not None:
        out = out + gs.to(torch.float32)
    return out * lrelu_grad(x, slope)


def mask_values(shape, name):
    """LeakyReLU' arguments: small integers, +-0 and NaN (all three take the slope branch)"""
    rng = _rng("mask:" + name)
    m = ints(rng, shape, 2, 0).to(torch.float32)
    flat = m.reshape(-1)
    flat[torch.arange(3, flat.numel(), 11)] = -0.0
    flat[torch.arange(7, flat.numel(), 13)] = float("nan")
    return m


def upsample2_bwd_reference(g, y, slope):
    B, C, D, H, W = g.shape
    s = g.to(torch.float64).reshape(B, C, D // 2, 2, H // 2, 2, W // 2, 2).sum(dim=(3, 5, 7)).to(torch.float32)
    return s if y is None else s * lrelu_grad(y, slope)


# --------------------------------------------------------------------------------------------------------------------------------
# the per-case lines of profiles/pr09_bf16_cases_cpu.txt
# --------------------------------------------------------------------------------------------------------------------------------
MIN_ROUNDED, MIN_TIES = 0.10, 0.05


def report_lines():
    lines = ["# tests/bf16_cases.py: worst-case sum bound (integer units, must stay below 2^24 = %d), share of the blocked outputs that the bf16 store"
             % TWO24, "# has to round / that are exact ties (required: >= %.2f / >= %.2f), launch geometry.  Written by `python tests/bf16_cases.py`."
             % (MIN_ROUNDED, MIN_TIES)]
    ops = OPS + [default_grid_op(CUS_REF)]
    for op in ops:
        for d, m in conv_runs(op):
            if m:
                continue
            run = build_run(op, d, m)
            _, v = run_reference(run, torch.float32 if op["multi"] else torch.float64)
            g = conv_geometry(run["C0"] + run["C1"], run["cout"], run["vol"], run["B"], run["planar"])
            sh = rounding_shares(v[:, :run["n_real"]])          # (channels beyond the operator's are zero)
            lines.append("conv  %-16s %-5s bound %8d  rounded %.3f ties %.3f  NCT %d ROWS %d tiles %4d Q %d G %d%s"
                         % (op["name"], d, run["bound"], sh[0], sh[1], g["NCT"], g["ROWS"], g["ntiles"], g["Q"], g["G"],
                            "  (planar fp32: no rounding)" if run["planar"] else ""))
    for fu in FUSED:
        fr = build_fused(fu, False)
        z, s = fused_reference(fr, torch.float32 if fu["multi"] else torch.float64)
        g = conv_geometry(fr["cdz"], fr["cup"], fr["vol"], fr["B"])
        a, b = rounding_shares(z), rounding_shares(s)
        lines.append("fused %-16s       bound %8d  rounded %.3f ties %.3f  2x2x2 sums: rounded %.3f ties %.3f  NCT %d ROWS %d tiles %4d Q %d G %d"
                     % (fu["name"], fr["bound"], a[0], a[1], b[0], b[1], g["NCT"], g["ROWS"], g["ntiles"], g["Q"], g["G"]))
    for c in WGRAD:
        D, H, W = c["vol"]
        nblk, nseg, seg_len = bwb_tasks((c["c0"] + c["c1"]) // 16, c["B"], D, H, W)
        lines.append("wgrad %-16s       bound %8d  on %d CUs: NBLK %3d nseg %2d seg_len %d%s"
                     % (c["name"], wgrad_bound(c), CUS_REF, nblk, nseg, seg_len, "  task_rr" if nblk % 8 == 0 and D * H * W >= 1 << 21 else ""))
    return lines


if __name__ == "__main__":
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pr09_bf16_cases_cpu.txt")
    with open(path, "w") as f:
        f.write("\n".join(report_lines()) + "\n")
    print(open(path).read())
