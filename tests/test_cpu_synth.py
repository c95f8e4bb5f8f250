"""CPU side of the SynthMorph image synthesis (csrc/synth.hip, voxelmorph_amd/synth.py, data.synthmorph, py.utils.load_labels): the float64
arbiters of tests/synth_cases.py agree with independent restatements, the gates are the recorded ones, the new entry points are declared,
bound and exported and refuse what they must before any launch, and the host pieces that need no device behave as the reference's."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import synth_cases as sc                          # noqa: E402
import voxelmorph_amd as vxm                      # noqa: E402
from voxelmorph_amd import _lib                   # noqa: E402

NEW_SYMBOLS = ("vxm_synth_draw_fwd", "vxm_onehot_fwd", "vxm_blur3d_fwd", "vxm_blur3d_workspace_bytes", "vxm_synth_finish_fwd",
               "vxm_synth_finish_workspace_bytes")


@pytest.fixture(scope="module")
def rows():
    return {r[0]: sc.row_arrays(r) for r in sc.ROWS}


def test_table_is_well_formed(rows):
    assert sc.ROW_IDS == ["tiny_2x2x2", "wide_7x9x70", "ragged_3x40x33", "batch_5x6x40", "seams_20x36x132"]
    assert [r[2] for r in sc.ROWS] == [1, 2, 1, 3, 1] and sc.BLUR_T == (3, 7, 13)
    assert sc.LABELS == sorted(sc.LABELS) and np.any(np.diff(sc.LABELS) > 1)                 # not contiguous
    V = [int(np.prod(r[1])) for r in sc.ROWS]
    assert V[1] % 4 == 2 and V[2] % 4 == 0 and V[2] % 1024 and any(r[1][2] % 4 == 0 for r in sc.ROWS) and any(r[1][2] % 4 for r in sc.ROWS)
    assert V[4] > 2 * 1024 and int(np.prod(sc.BIG[1])) // 4 > 2048 * 256 and int(np.prod(sc.BIG[1])) > 256 * 4096
    for r in sc.ROWS:
        a = rows[r[0]]
        assert a["labels"].dtype == np.float32 and a["labels"].shape == (r[2], 1) + r[1]
        known = np.isin(a["labels"], sc.LABELS)
        assert not known.all() and known.mean() > 0.9 or r[0] == "tiny_2x2x2"
        assert not known.reshape(-1)[0]                                                      # every row has a voxel that is not in the list
        assert set(np.unique(a["labels"][known]).tolist()) <= set(sc.LABELS)
        for v in sc.FINISH_VARIANTS:
            x, lb, g = sc.finish_inputs(a, v)
            assert x.dtype == lb.dtype == g.dtype == np.float32 and g.shape == (r[2],) and set(g.tolist()) <= {0.5, float(np.float32(1.7))}
    x, lb, _ = sc.finish_inputs(rows["seams_20x36x132"], "clip_both")
    assert (x * np.exp(lb)).min() < 0 and (x * np.exp(lb)).max() > 255                       # clips at both ends


def test_lattice_rows_are_exact_in_fp32():
    for lat in sc.LATTICES:
        a = sc.lattice_arrays(lat)
        assert np.array_equal(a["x"], np.round(a["x"])) and np.abs(a["x"]).max() <= 8
        assert set(np.unique(a["taps"]).tolist()) <= {0.0, 0.125, 0.25, 0.5}
        assert not np.array_equal(a["taps"][0, 0], a["taps"][0, 1]) and not np.array_equal(a["taps"][0], a["taps"][1])
        y64 = sc.blur_arbiter(a["x"], a["taps"])
        assert np.array_equal(y64, y64.astype(np.float32)) and np.array_equal(y64, sc.blur_arbiter(a["x"], a["taps"], np.float32))
    assert sc.LATTICES[0][1][2] % 4 == 0 and sc.LATTICES[1][1][2] % 4                        # both blur paths


@pytest.mark.parametrize("name", sc.ROW_IDS)
def test_blur_arbiter_equals_conv3d_in_float64(rows, name):
    a = rows[name]
    for T in sc.BLUR_T:
        taps = sc.taps_for(a["sigma"], T)
        want = sc.blur_torch(torch.from_numpy(a["x"]).double(), torch.from_numpy(taps)).numpy()
        assert sc.rel_l2(sc.blur_arbiter(a["x"], taps), want) < 1e-14, (name, T)
    # the order of the axes and of the taps: an asymmetric kernel on one axis only, against a shifted copy
    x = a["x"]
    taps = np.zeros((a["B"], 3, 3), np.float32)
    taps[:, :, 1] = 1
    taps[:, 2] = (1, 0, 0)                                                                   # y[w] = x[w - 1]
    y = sc.blur_arbiter(x, taps)
    assert np.array_equal(y[..., 1:], x[..., :-1]) and not y[..., 0].any()


def test_blur_arbiter_with_one_tap_is_the_input(rows):
    a = rows["wide_7x9x70"]
    assert np.array_equal(sc.blur_arbiter(a["x"], np.ones((a["B"], 3, 1), np.float32)), a["x"])


@pytest.mark.parametrize("name", sc.ROW_IDS)
def test_draw_and_onehot_arbiters_equal_the_compare_formulation(rows, name):
    a = rows[name]
    lab = a["labels"]
    want = np.zeros(lab.shape)
    for b in range(a["B"]):
        for k, v in enumerate(sc.LABELS):
            sel = lab[b] == v
            want[b][sel] = a["means"][b, k].astype(np.float64) + a["stds"][b, k].astype(np.float64) * a["noise"][b][sel].astype(np.float64)
    assert np.array_equal(sc.draw_arbiter(lab, sc.LABELS, a["means"], a["stds"], a["noise"]), want)
    t = torch.from_numpy
    got = sc.draw_torch(t(lab), torch.tensor(sc.LABELS, dtype=torch.float32), t(a["means"]), t(a["stds"]), t(a["noise"])).numpy()
    assert sc.rel_l2(got, want) < 2e-7 and not got[~np.isin(lab, sc.LABELS)].any()
    for out in (None, sc.OUT_LIST, sc.OUT_DICT):
        outs, index, value = sc.out_table(sc.LABELS, out)
        oh = sc.onehot_arbiter(lab, sc.LABELS, index, len(outs))
        recoded = np.zeros_like(lab)
        for v, w in zip(sc.LABELS, value):
            recoded[lab == v] = w
        kept = np.isin(lab, [v for v, i in zip(sc.LABELS, index) if i >= 0])
        for j, o in enumerate(outs):                                                         # one-hot against `==` on the recoded map
            assert np.array_equal(oh[:, j], ((recoded[:, 0] == o) & kept[:, 0]).astype(np.float32)), (out, o)
        assert np.array_equal(oh.sum(1), kept[:, 0].astype(np.float32))
    assert sc.out_table(sc.LABELS, sc.OUT_LIST)[0] == [2, 17, 1024] and sc.out_table(sc.LABELS, sc.OUT_DICT)[0] == [0, 5, 9]
    assert sc.out_table(sc.LABELS, sc.OUT_DICT)[1].tolist() == [0, 1, 1, -1, 2, -1]


@pytest.mark.parametrize("name", sc.ROW_IDS)
def test_finish_arbiter_equals_the_torch_formulation_in_float64(rows, name):
    a = rows[name]
    for variant in sc.FINISH_VARIANTS:
        x, lb, g = sc.finish_inputs(a, variant)
        want = sc.finish_torch(torch.from_numpy(x).double(), torch.from_numpy(lb).double(), torch.from_numpy(g).double()).numpy()
        got = sc.finish_arbiter(x, lb, g)
        assert sc.rel_l2(got, want) < 1e-14, (name, variant)
        for b in range(a["B"]):
            assert got[b].min() == 0 and got[b].max() == 1
    const = np.full((2, 1, 3, 4, 5), 7.0, np.float32)
    assert not sc.finish_arbiter(const, None, np.ones(2, np.float32)).any()
    assert not sc.finish_arbiter(const + 300, np.zeros_like(const), np.ones(2, np.float32)).any()          # clipped to a constant 255


def test_gates_are_the_recorded_output_of_the_tool():
    text = open(os.path.join(ROOT, "profiles", "pr12_synth_gates_cpu.txt")).read()
    for k in sc.GATE_CLASSES:
        m = re.search(r"largest %s\s+(\S+)\s+-> gate \(x4\): (\S+)" % k, text)
        assert m, k
        worst, gate = float(m.group(1)), float(m.group(2))
        assert gate == sc.GATES[k], (k, gate, sc.GATES[k])
        assert abs(gate - 4 * worst) <= 2e-3 * gate
    for r in sc.ROWS:
        assert len(re.findall(r"^%s\s" % r[0], text, re.M)) == len(sc.BLUR_T) + len(sc.FINISH_VARIANTS), r[0]


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "vxm_hip.h")).read()
    h = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES and re.search(r"\b%s\(" % s, header) and hasattr(h, s), s
    assert h.vxm_version() >= 507
    assert "synth.hip" in open(os.path.join(ROOT, "voxelmorph_amd", "csrc", "build.sh")).read()
    for name in ("gaussian_taps", "draw_perlin", "SynthDraws", "draw_params", "labels_to_image", "draw", "onehot", "blur", "finish", "recode"):
        assert hasattr(vxm.synth, name), name
    assert hasattr(vxm.data, "synthmorph") and hasattr(vxm.py.utils, "load_labels")


def test_c_entry_points_reject_bad_arguments_before_any_launch():
    h = _lib.lib()
    p = 16                                                   # never dereferenced: the argument checks come first
    assert h.vxm_synth_draw_fwd(p, p, p, p, p, p, 6, 0, 64, None) == 1 and h.vxm_synth_draw_fwd(p, p, p, p, p, p, 6, 1, 0, None) == 1
    assert h.vxm_synth_draw_fwd(p, p, p, p, p, p, 6, 1, 1 << 31, None) == 1
    assert h.vxm_synth_draw_fwd(p, p, p, p, p, p, 0, 1, 64, None) == 2 and h.vxm_synth_draw_fwd(p, p, p, p, p, p, 4097, 1, 64, None) == 2
    for k in range(6):
        args = [p] * 6
        args[k] = None
        assert h.vxm_synth_draw_fwd(*args, 6, 1, 64, None) == 3, k
    assert h.vxm_onehot_fwd(p, p, p, 6, 3, p, 0, 64, None) == 1 and h.vxm_onehot_fwd(p, p, p, 6, 3, p, 1, 1 << 31, None) == 1
    assert h.vxm_onehot_fwd(p, p, p, 6, 0, p, 1, 64, None) == 2 and h.vxm_onehot_fwd(p, p, p, 6, 257, p, 1, 64, None) == 2
    assert h.vxm_onehot_fwd(p, p, p, 4097, 3, p, 1, 64, None) == 2
    assert h.vxm_onehot_fwd(p, p, None, 6, 3, p, 1, 64, None) == 3 and h.vxm_onehot_fwd(p, p, p, 6, 3, None, 1, 64, None) == 3
    q, w = 32, 48
    big = 1 << 40
    for T in (0, 2, 26, 27, -1):
        assert h.vxm_blur3d_fwd(p, p, T, q, w, big, 1, 1, 8, 8, 8, None) == 1, T
        assert h.vxm_blur3d_workspace_bytes(T, 1, 1, 8, 8, 8) == 0
    assert h.vxm_blur3d_fwd(p, p, 7, q, w, big, 1, 1, 0, 8, 8, None) == 1 and h.vxm_blur3d_fwd(p, p, 7, q, w, big, 1, 1, 2048, 1024, 1024, None) == 1
    assert h.vxm_blur3d_fwd(p, p, 7, q, w, big, 65536, 1, 8, 8, 8, None) == 1
    assert h.vxm_blur3d_fwd(None, p, 7, q, w, big, 1, 1, 8, 8, 8, None) == 3 and h.vxm_blur3d_fwd(p, None, 7, q, w, big, 1, 1, 8, 8, 8, None) == 3
    assert h.vxm_blur3d_fwd(p, p, 7, q, None, big, 1, 1, 8, 8, 8, None) == 3
    assert h.vxm_blur3d_fwd(p, p, 7, p, w, big, 1, 1, 8, 8, 8, None) == 2                    # out == x
    need = h.vxm_blur3d_workspace_bytes(7, 2, 3, 8, 9, 10)
    assert need == 4 * 2 * 3 * 8 * 9 * 10 and h.vxm_blur3d_fwd(p, p, 7, q, w, need - 1, 2, 3, 8, 9, 10, None) == 4
    assert b"workspace" in h.vxm_last_error_string()
    assert h.vxm_synth_finish_fwd(p, p, p, q, w, big, 0, 64, None) == 1 and h.vxm_synth_finish_fwd(p, p, p, q, w, big, 1, 1 << 31, None) == 1
    assert h.vxm_synth_finish_fwd(None, p, p, q, w, big, 1, 64, None) == 3 and h.vxm_synth_finish_fwd(p, None, None, q, w, big, 1, 64, None) == 3
    assert h.vxm_synth_finish_fwd(p, None, p, q, None, big, 1, 64, None) == 3
    need = h.vxm_synth_finish_workspace_bytes(3, 4000)
    assert need == 4 * 2 * 3 * 4 and h.vxm_synth_finish_fwd(p, None, p, q, w, need - 1, 3, 4000, None) == 4
    assert h.vxm_synth_finish_workspace_bytes(0, 64) == 0 and h.vxm_synth_finish_workspace_bytes(1, 1 << 31) == 0
    # at most 512 partials per sample, whatever the volume
    assert h.vxm_synth_finish_workspace_bytes(1, 160 * 192 * 224) <= 4 * 2 * 512 and h.vxm_synth_finish_workspace_bytes(1, (1 << 31) - 1) <= 4 * 2 * 512


def test_host_wrappers_refuse_bad_shapes_and_cpu_tensors():
    S = vxm.synth
    lab = torch.zeros(2, 1, 4, 6, 8)
    with pytest.raises(ValueError, match="label map"):
        S.draw(torch.zeros(2, 4, 6, 8), sc.LABELS, torch.zeros(2, 6), torch.zeros(2, 6), torch.zeros(2, 4, 6, 8))
    with pytest.raises(ValueError, match=r"\[B,L\]"):
        S.draw(lab, sc.LABELS, torch.zeros(2, 5), torch.zeros(2, 6), torch.zeros_like(lab))
    with pytest.raises(ValueError, match="noise"):
        S.draw(lab, sc.LABELS, torch.zeros(2, 6), torch.zeros(2, 6), torch.zeros(2, 1, 4, 6, 7))
    with pytest.raises(_lib.VxmHipError, match="no CPU fallback"):
        S.draw(lab, sc.LABELS, torch.zeros(2, 6), torch.zeros(2, 6), torch.zeros_like(lab))
    with pytest.raises(_lib.VxmHipError, match="no CPU fallback"):
        S.onehot(lab, sc.LABELS)
    with pytest.raises(ValueError, match="no output label"):
        S.onehot(lab, sc.LABELS, [5, 6])
    with pytest.raises(ValueError, match="257"):
        S.onehot(lab, list(range(300)), list(range(257)))
    with pytest.raises(ValueError, match="taps"):
        S.blur(lab, torch.zeros(3, 3, 7))
    with pytest.raises(ValueError, match="odd"):
        S.blur(lab, torch.zeros(2, 3, 4))
    with pytest.raises(_lib.VxmHipError, match="no CPU fallback"):
        S.blur(lab, torch.zeros(2, 3, 7))
    with pytest.raises(ValueError, match="gamma"):
        S.finish(lab, None, torch.ones(3))
    with pytest.raises(ValueError, match="log_bias"):
        S.finish(lab, torch.zeros(2, 1, 4, 6, 7), torch.ones(2))
    with pytest.raises(_lib.VxmHipError, match="no CPU fallback"):
        S.finish(lab, None, torch.ones(2))
    with pytest.raises(ValueError, match="extents"):
        S.draw_perlin((4, 6, 8), [2], [1.0], [torch.zeros(2, 1, 2, 3, 5)])
    with pytest.raises(ValueError, match="draws"):
        S.labels_to_image(lab, sc.LABELS)
    with pytest.raises(ValueError, match="fp32"):
        S.LabelTable([0, (1 << 24) + 1])
    with pytest.raises(ValueError, match="25"):
        S.blur_taps_count(5.0)
    assert S.blur_taps_count(1) == 7 and S.blur_taps_count(0) == 1 and S.blur_taps_count(4) == 25
    assert S.perlin_extents((16, 24, 33), 8) == (2, 3, 5)


def test_label_table_recodes_lists_and_dicts():
    for out in (None, sc.OUT_LIST, sc.OUT_DICT):
        t = vxm.synth.LabelTable(list(reversed(sc.LABELS)) + [3], out)                       # unsorted, with a duplicate
        outs, index, value = sc.out_table(sc.LABELS, out)
        assert t.labels.tolist() == sc.LABELS and t.out_labels.tolist() == outs
        assert np.array_equal(t.out_index, index) and np.array_equal(t.out_value, value)


def test_gaussian_taps_sum_to_one_and_are_a_delta_at_sigma_zero():
    sigma = torch.tensor([[0.0, 1e-6, 0.4], [1.0, 2.5, 8.0]])
    for T in (1, 3, 7, 13, 25):
        taps = vxm.synth.gaussian_taps(sigma, T)
        assert taps.dtype == torch.float32 and tuple(taps.shape) == (2, 3, T)
        assert float((taps.double().sum(-1) - 1).abs().max()) < 2e-7
        R = (T - 1) // 2
        delta = torch.zeros(T)
        delta[R] = 1
        assert torch.equal(taps[0, 0], delta) and torch.equal(taps[0, 1], delta)
        assert torch.equal(taps, taps.flip(-1)) and np.array_equal(taps.numpy(), sc.taps_for(sigma.numpy(), T))
        if T >= 3:
            assert float(taps[1, 0, R]) > float(taps[1, 0, R + 1]) > 0
    w = vxm.synth.gaussian_taps(torch.tensor([[1.0, 1.0, 1.0]]), 7)[0, 0].double()
    g = torch.exp(-0.5 * torch.arange(-3, 4).double() ** 2)
    assert float((w - g / g.sum()).abs().max()) < 1e-7
    with pytest.raises(ValueError):
        vxm.synth.gaussian_taps(sigma, 4)
    with pytest.raises(ValueError):
        vxm.synth.gaussian_taps(torch.ones(3), 3)


def test_draw_params_ranges_on_the_cpu_generator():
    g = torch.Generator().manual_seed(5)
    d = vxm.synth.draw_params(g, sc.LABELS, (16, 24, 32), batch_size=64, warp_res=(8, 16), bias_res=(8,), device="cpu")
    L = len(sc.LABELS)
    assert tuple(d.means.shape) == (64, L) == tuple(d.stds.shape) and d.T == 7 and tuple(d.blur_sigma.shape) == (64, 3)
    zeroed = (d.means[:, 0] == 0) & (d.stds[:, 0] == 0)
    assert 2 <= int(zeroed.sum()) <= 30                                                      # probability 0.2 of 64
    assert float(d.means[:, 1:].min()) >= 25 and float(d.means.max()) <= 225 and float(d.means[~zeroed, 0].min()) < 25 + 40
    assert float(d.stds[:, 1:].min()) >= 5 and float(d.stds.max()) <= 25
    assert [tuple(n.shape) for n in d.vel_noise] == [(64, 3, 2, 3, 4), (64, 3, 1, 2, 2)]     # half resolution, scales 4 and 8 there
    assert [tuple(n.shape) for n in d.bias_noise] == [(64, 1, 2, 3, 4)]
    assert all(float(s.min()) >= 0 and float(s.max()) <= 0.5 for s in d.vel_std) and float(d.bias_std[0].max()) <= 0.3
    assert float(d.blur_sigma.min()) >= 0 and float(d.blur_sigma.max()) <= 1 and tuple(d.noise.shape) == (64, 1, 16, 24, 32)
    assert float(d.gamma.min()) > 0.3 and float(d.gamma.max()) < 3 and abs(float(d.gamma.log().mean())) < 0.15
    assert tuple(d.taps.shape) == (64, 3, 7)
    off = vxm.synth.draw_params(g, sc.LABELS, (16, 24, 32), warp_std=0, bias_std=0, blur_std=0, gamma_std=0, device="cpu")
    assert off.vel_noise is None and off.bias_noise is None and off.T == 1 and torch.equal(off.gamma, torch.ones(1))


def test_load_labels_follows_the_reference_contract(tmp_path):
    rng = np.random.default_rng(3)
    maps = [rng.choice(sc.LABELS[:k], size=(4, 5, 6)).astype(np.int32) for k in (3, 5, 6)]
    np.save(tmp_path / "a.npy", maps[0])
    np.savez_compressed(tmp_path / "b.npz", vol=maps[1])
    vxm.py.utils.save_volfile(maps[2].astype(np.int16), str(tmp_path / "c.nii.gz"))
    (tmp_path / "notes.txt").write_text("not a label map")
    labels, loaded = vxm.py.utils.load_labels(str(tmp_path))
    assert labels.tolist() == sorted(set(np.unique(np.stack(maps)).tolist())) and len(loaded) == 3
    for m, got in zip(maps, loaded):                                                         # sorted by file name
        assert np.array_equal(m, got) and np.issubdtype(got.dtype, np.integer)
    only, one = vxm.py.utils.load_labels([str(tmp_path / "*.npy")])
    assert len(one) == 1 and only.tolist() == np.unique(maps[0]).tolist()
    with pytest.raises(ValueError, match="no labels found"):
        vxm.py.utils.load_labels(str(tmp_path / "*.mgz"))
    np.save(tmp_path / "d.npy", maps[0].astype(np.float32))
    with pytest.raises(ValueError, match="non-integral"):
        vxm.py.utils.load_labels(str(tmp_path))
    np.save(tmp_path / "d.npy", maps[0][:3])
    with pytest.raises(ValueError, match="shape"):
        vxm.py.utils.load_labels(str(tmp_path))


def test_loader_draws_as_the_reference_and_refuses_the_cpu():
    maps = [np.full((4, 6, 8), k, np.int32) for k in range(5)]
    with pytest.raises(ValueError, match="HIP device"):
        vxm.data.synthmorph(maps, device="cpu")
    from voxelmorph_amd.data import SynthMorphLoader
    loader = SynthMorphLoader.__new__(SynthMorphLoader)                                      # the draw alone needs no device
    loader.n, loader.shape, loader.batch_size, loader.same_subj, loader.flip = 5, (4, 6, 8), 3, False, True
    loader.rng = np.random.default_rng(1)
    seen = set()
    for _ in range(200):
        ind, axes = loader._draw()
        assert ind.shape == (6,) and ind.min() >= 0 and ind.max() < 5
        assert len(set(axes.tolist())) == len(axes) <= 3 and all(0 <= a < 3 for a in axes)
        seen.add(tuple(sorted(axes.tolist())))
    assert seen == {(), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)}
    loader.same_subj, loader.flip = True, False
    ind, axes = loader._draw()
    assert np.array_equal(ind[:3], ind[3:]) and len(axes) == 0


def test_training_script_lists_the_reference_flags():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_synthmorph.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    for f in ("--label-dir", "--model-dir", "--same-subj", "--blur-std", "--gamma", "--vel-std", "--vel-res", "--bias-std", "--bias-res",
              "--out-labels", "--epochs", "--batch-size", "--init-weights", "--save-freq", "--reg-param", "--lr", "--int-steps", "--enc", "--dec",
              "--steps-per-epoch"):
        assert f in out.stdout, f
