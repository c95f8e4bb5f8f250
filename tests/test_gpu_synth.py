"""The SynthMorph image synthesis on the device: the kernels of csrc/synth.hip behind `vxm.synth` against the arbiters of
tests/synth_cases.py -- bit for bit where the definition reproduces exactly (the draw: a multiply and an add; the one-hot; the blur with
one tap and on a lattice of exactly summable numbers; the finish without bias and gamma), within a gate against the float64 arbiter
elsewhere.  Gates: tools/synth_gates.py (profiles/pr12_synth_gates_cpu.txt) -- 4 x the error of the plain fp32 evaluation of the same
definition on the same rows.  Then `labels_to_image` end to end, the loader and one training step of scripts/train_synthmorph.py's model.
Run with -s for the margins (profiles/pr12_synth_gpu_tests.log)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import synth_cases as sc                          # noqa: E402

ALL_IDS = sc.ROW_IDS + [sc.BIG[0]]


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def vxm():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    import voxelmorph_amd
    from voxelmorph_amd import _lib
    _lib.lib()
    return voxelmorph_amd


@pytest.fixture(scope="module")
def S(vxm):
    return vxm.synth


@pytest.fixture(scope="module")
def rows():
    return {r[0]: sc.row_arrays(r) for r in sc.ROWS + [sc.BIG]}


def check(name, what, got, want, gate):
    err = sc.rel_l2(got, want)
    print("%-38s %-8s rel-L2 %.3e  gate %.2e  margin %s" % (name, what, err, gate, "%.1fx" % (gate / err) if err else "exact"))
    assert np.isfinite(got).all() and err <= gate, (name, what, err, gate)


# --------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("name", ALL_IDS)
def test_draw_equals_numpy_float32_bit_for_bit(S, rows, name):
    a = rows[name]
    got = N(S.draw(G(a["labels"]), sc.LABELS, G(a["means"]), G(a["stds"]), G(a["noise"])))
    want = sc.draw_arbiter(a["labels"], sc.LABELS, a["means"], a["stds"], a["noise"], np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    unknown = ~np.isin(a["labels"], sc.LABELS)
    assert unknown.any() and not got[unknown].any() and np.abs(got[~unknown]).min() > 0


@pytest.mark.parametrize("out", [None, sc.OUT_LIST, sc.OUT_DICT], ids=["all", "list", "dict"])
@pytest.mark.parametrize("name", ALL_IDS)
def test_onehot_with_unknown_and_dropped_labels_as_zero_planes(S, rows, name, out):
    a = rows[name]
    outs, index, value = sc.out_table(sc.LABELS, out)
    lab = G(a["labels"])
    got = N(S.onehot(lab, sc.LABELS, out))
    assert got.shape == (a["B"], len(outs)) + a["size"]
    assert np.array_equal(got, sc.onehot_arbiter(a["labels"], sc.LABELS, index, len(outs)))
    dropped = ~np.isin(a["labels"][:, 0], [v for v, i in zip(sc.LABELS, index) if i >= 0])
    assert dropped.any() and not got.sum(1)[dropped].any() and np.all(got.sum(1)[~dropped] == 1)
    rec = N(S.recode(lab, sc.LABELS, out))                           # one_hot=False: the recoded map, dropped labels 0
    want = np.zeros_like(a["labels"])
    for v, w, i in zip(sc.LABELS, value, index):
        if i >= 0:
            want[a["labels"] == v] = w
    assert np.array_equal(rec, want)


@pytest.mark.parametrize("name", sc.ROW_IDS)
def test_blur_with_one_tap_is_the_input(S, rows, name):
    a = rows[name]
    x = np.concatenate([a["x"], a["noise"]], axis=1)                 # two channels
    assert np.array_equal(N(S.blur(G(x), torch.ones(a["B"], 3, 1, device="cuda"))), x)
    delta = np.zeros((a["B"], 3, 7), np.float32)
    delta[:, :, 3] = 1
    assert np.array_equal(N(S.blur(G(x), G(delta))), x)


@pytest.mark.parametrize("lat", sc.LATTICES, ids=[lat[0] for lat in sc.LATTICES])
def test_blur_on_a_lattice_is_exact(S, lat):
    a = sc.lattice_arrays(lat)
    got = N(S.blur(G(a["x"]), G(a["taps"])))
    want = sc.blur_arbiter(a["x"], a["taps"])
    assert np.array_equal(got, want.astype(np.float32)) and np.array_equal(want, want.astype(np.float32)) and got.any()


def test_blur_shifts_along_the_right_axis_in_the_right_direction(S, rows):
    a = rows["batch_5x6x40"]
    x = a["x"]
    for ax in range(3):
        taps = np.zeros((a["B"], 3, 3), np.float32)
        taps[:, :, 1] = 1
        taps[:, ax] = (1, 0, 0)                                      # y[i] = x[i - 1] along this axis, zero at i = 0
        got = N(S.blur(G(x), G(taps)))
        sl_to, sl_from, first = [slice(None)] * 5, [slice(None)] * 5, [slice(None)] * 5
        sl_to[2 + ax], sl_from[2 + ax], first[2 + ax] = slice(1, None), slice(None, -1), 0
        assert np.array_equal(got[tuple(sl_to)], x[tuple(sl_from)]) and not got[tuple(first)].any(), ax


@pytest.mark.parametrize("name", ALL_IDS)
def test_finish_without_bias_and_gamma_equals_numpy_float32(S, rows, name):
    a = rows[name]
    x, _, _ = sc.finish_inputs(a, "clip_both")
    one = np.ones(a["B"], np.float32)
    got = N(S.finish(G(x), None, G(one)))
    assert np.array_equal(got, sc.finish_arbiter(x, None, one, np.float32))
    for b in range(a["B"]):
        assert got[b].min() == 0 and got[b].max() == 1


def test_finish_of_a_constant_image_is_zero(S):
    for shape in ((2, 1, 3, 4, 5), (1, 1, 8, 8, 20)):
        const = torch.full(shape, 37.5, device="cuda")
        g = torch.full((shape[0],), 1.7, device="cuda")
        assert not S.finish(const, None, g).any() and not S.finish(const, torch.zeros_like(const), g).any()
        assert not S.finish(const + 500, None, g).any()              # clipped to a constant 255


@pytest.mark.parametrize("name", ["wide_7x9x70", "ragged_3x40x33", "batch_5x6x40", "seams_20x36x132"])
def test_every_kernel_twice_gives_the_same_bits(S, rows, name):
    a = rows[name]
    x, lb, gamma = sc.finish_inputs(a, "bias_g0.5")
    taps = G(sc.taps_for(a["sigma"], 7))
    runs = []
    for _ in range(2):
        lab = G(a["labels"])
        runs.append((N(S.draw(lab, sc.LABELS, G(a["means"]), G(a["stds"]), G(a["noise"]))), N(S.onehot(lab, sc.LABELS, sc.OUT_DICT)),
                     N(S.blur(G(a["x"]), taps)), N(S.finish(G(x), G(lb), G(gamma)))))
    for p, q in zip(*runs):
        assert np.array_equal(p, q)


# --------------------------------------------------------------------------- within a gate, against the float64 arbiter
@pytest.mark.parametrize("T", sc.BLUR_T)
@pytest.mark.parametrize("name", sc.ROW_IDS)
def test_blur_rows_against_the_arbiter(S, rows, name, T):
    a = rows[name]
    taps = sc.taps_for(a["sigma"], T)                                # differ per sample and per axis
    assert not np.array_equal(taps[0, 0], taps[0, 1]) and (a["B"] == 1 or not np.array_equal(taps[0], taps[1]))
    dev_taps = N(S.gaussian_taps(G(a["sigma"].astype(np.float32)), T))                  # float64 on the device: one fp32 ulp of the host's
    np.testing.assert_allclose(dev_taps, sc.taps_for(a["sigma"].astype(np.float32), T), rtol=0, atol=2.0 ** -24)
    got = N(S.blur(G(a["x"]), G(taps)))
    check("%s T=%d" % (name, T), "blur", got, sc.blur_arbiter(a["x"], taps), sc.GATES["blur"])


@pytest.mark.parametrize("variant", sc.FINISH_VARIANTS)
@pytest.mark.parametrize("name", ALL_IDS)
def test_finish_rows_against_the_arbiter(S, rows, name, variant):
    a = rows[name]
    x, lb, gamma = sc.finish_inputs(a, variant)
    got = N(S.finish(G(x), G(lb), G(gamma)))
    check("%s %s" % (name, variant), "finish", got, sc.finish_arbiter(x, lb, gamma), sc.GATES["finish"])
    for b in range(a["B"]):
        assert got[b].min() == 0 and got[b].max() == 1


# --------------------------------------------------------------------------- end to end
def _e2e_inputs(S, seed_offset=0, **kw):
    e = sc.E2E
    rng = np.random.default_rng(e["seed"])
    labels = sc.label_map(rng, e["B"], e["shape"])
    g = torch.Generator(device="cuda").manual_seed(e["seed"] + seed_offset)
    draws = S.draw_params(g, sc.LABELS, e["shape"], batch_size=e["B"], warp_res=e["warp_res"], bias_res=e["bias_res"], **kw)
    return labels, draws


def _synth(S, labels, draws, out=sc.OUT_DICT, **kw):
    e = sc.E2E
    return S.labels_to_image(G(labels), sc.LABELS, out, draws=draws, warp_res=e["warp_res"], bias_res=e["bias_res"], int_steps=e["int_steps"], **kw)


def test_labels_to_image_equals_its_public_pieces_bit_for_bit(vxm, S):
    from voxelmorph_amd.torch import functional as VF
    e = sc.E2E
    labels, draws = _e2e_inputs(S, warp_std=3.0)
    image, omap = _synth(S, labels, draws)
    assert tuple(image.shape) == (e["B"], 1) + e["shape"] and tuple(omap.shape) == (e["B"], 3) + e["shape"] and not image.requires_grad
    with torch.no_grad():
        half = tuple(s // 2 for s in e["shape"])
        vel = S.draw_perlin(half, [r / 2.0 for r in e["warp_res"]], draws.vel_std, draws.vel_noise)
        disp = VF.VecIntFn.apply(vel, e["int_steps"])
        lab = G(labels)
        assert VF.warp_up_ok(lab, disp)
        warped = VF.WarpUpFn.apply(lab, disp, 2.0, "nearest", False)
        two = VF.WarpFn.apply(lab, VF.ResizeFn.apply(disp, 2.0), "nearest")          # the pair the fused kernel stands for
        raw = S.draw(warped, sc.LABELS, draws.means, draws.stds, draws.noise)
        blurred = S.blur(raw, S.gaussian_taps(draws.blur_sigma, draws.T))
        bias = S.draw_perlin(e["shape"], e["bias_res"], draws.bias_std, draws.bias_noise)
        want = S.finish(blurred, bias, draws.gamma)
        want_map = S.onehot(warped, sc.LABELS, sc.OUT_DICT)
    assert torch.equal(warped, two) and not torch.equal(warped, lab)                     # the deformation moved labels
    assert torch.equal(image, want) and torch.equal(omap, want_map)
    assert set(np.unique(N(warped)).tolist()) <= set(np.unique(labels).tolist()) | {0.0}    # nearest: no new label values
    # the smooth fields against numpy float64 on the same draws
    v64 = N(draws.vel_noise[0]).astype(np.float64) * N(draws.vel_std[0]).astype(np.float64).reshape(-1, 1, 1, 1, 1)
    assert sc.rel_l2(N(vel), _upsample64(v64, half)) < 1e-6
    img, rmap = _synth(S, labels, draws, one_hot=False)
    assert torch.equal(img, image) and torch.equal(rmap, S.recode(warped, sc.LABELS, sc.OUT_DICT))


def _upsample64(x, shape):
    """linear, align_corners upsampling of [B,C,d,h,w] float64 to `shape`"""
    for ax, S_out in enumerate(shape):
        n = x.shape[2 + ax]
        pos = np.arange(S_out) * ((n - 1) / (S_out - 1) if S_out > 1 else 0.0)
        lo = np.minimum(np.floor(pos).astype(int), n - 1)
        hi = np.minimum(lo + 1, n - 1)
        f = (pos - lo).reshape([-1 if k == 2 + ax else 1 for k in range(5)])
        x = np.take(x, lo, axis=2 + ax) * (1 - f) + np.take(x, hi, axis=2 + ax) * f
    return x


def test_image_range_zero_velocity_and_determinism(S):
    e = sc.E2E
    labels, draws = _e2e_inputs(S)
    image, omap = _synth(S, labels, draws)
    im = N(image)
    assert np.isfinite(im).all()
    for b in range(e["B"]):
        assert im[b].min() == 0 and im[b].max() == 1
    again, omap2 = _synth(S, labels, draws)
    assert torch.equal(image, again) and torch.equal(omap, omap2)                        # the same draws: the same bits
    _, other = _e2e_inputs(S, seed_offset=1)
    assert not torch.equal(_synth(S, labels, other)[0], image)                           # other draws: another image
    for d in draws.vel_std:
        d.zero_()                                                                        # a velocity std of 0: the identity
    still, smap = _synth(S, labels, draws)
    _, index, _ = sc.out_table(sc.LABELS, sc.OUT_DICT)
    assert np.array_equal(N(smap), sc.onehot_arbiter(labels, sc.LABELS, index, 3))       # the map is the recoded input
    assert not torch.equal(still, image)
    none = S.draw_params(torch.Generator(device="cuda").manual_seed(3), sc.LABELS, e["shape"], batch_size=e["B"], warp_std=0, bias_std=0)
    plain, pmap = S.labels_to_image(G(labels), sc.LABELS, draws=none)
    assert tuple(pmap.shape) == (e["B"], len(sc.LABELS)) + e["shape"] and float(plain.min()) == 0 and float(plain.max()) == 1


def test_loader_yields_flipped_device_pairs(vxm):
    rng = np.random.default_rng(5)
    maps = [rng.choice(sc.LABELS, size=(4, 6, 8)).astype(np.int32) for _ in range(5)]
    loader = vxm.data.synthmorph(maps, batch_size=2, seed=3)
    seen = set()
    for _ in range(12):
        src, trg = next(loader)
        assert src.is_cuda and src.dtype == torch.float32 and tuple(src.shape) == tuple(trg.shape) == (2, 1, 4, 6, 8) and src.is_contiguous()
        ind, axes = loader.last_indices, loader.last_axes
        seen.add(tuple(axes.tolist()))
        want = np.stack([maps[i] for i in ind])[:, None].astype(np.float32)
        if len(axes):
            want = np.flip(want, axis=tuple(int(a) + 2 for a in axes))
        assert np.array_equal(N(src), want[:2]) and np.array_equal(N(trg), want[2:])
    assert len(seen) > 2
    same = vxm.data.synthmorph(maps, batch_size=2, same_subj=True, flip=False)
    src, trg = next(same)
    assert torch.equal(src, trg)


def test_one_training_step_of_the_script_on_synthesised_pairs(vxm, S):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import train_synthmorph as ts
    from voxelmorph_amd.optim import FlatAdam
    e = sc.E2E
    labels, d1 = _e2e_inputs(S, warp_std=3.0)
    _, d2 = _e2e_inputs(S, seed_offset=1, warp_std=3.0)
    ima_1, map_1 = _synth(S, labels, d1)
    ima_2, map_2 = _synth(S, labels[::-1].copy(), d2)
    torch.manual_seed(e["seed"])
    model = ts.build_model(vxm, e["shape"], 3, [16, 32, 32], [32, 32, 32, 16, 16], e["int_steps"]).cuda()
    with torch.no_grad():
        model.vxm_model.flow.weight.normal_(0, 0.05)
    before = model.vxm_model.flow.weight.detach().clone()
    opt = FlatAdam(model, lr=1e-3)
    flow, pred = ts.register(model, ima_1, ima_2, map_1)
    assert tuple(flow.shape) == (e["B"], 3) + e["shape"] and tuple(pred.shape) == tuple(map_2.shape)
    loss = ts.make_step(vxm, model, opt, 1.0)(ima_1, map_1, ima_2, map_2)
    torch.cuda.synchronize()
    g = opt._views[[k for k, p in enumerate(opt.params) if p is model.vxm_model.flow.weight][0]]      # the flat gradient bucket's view
    print("synthmorph step: loss %.6f, |flow-head grad| %.3e" % (float(loss.detach()), float(g.norm())))
    loss = loss.detach()
    assert np.isfinite(float(loss)) and 0 < float(loss) < 2 and torch.isfinite(g).all() and float(g.norm()) > 0
    assert not torch.equal(model.vxm_model.flow.weight.detach(), before)
