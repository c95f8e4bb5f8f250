"""CPU side of the evaluation metrics (voxelmorph_amd/csrc/metrics.hip, voxelmorph_amd/metrics.py, scripts/test.py): the arbiters of
tests/eval_cases.py agree with the live reference, the host pieces behave as the reference's, the entry points are declared, bound and
exported and refuse bad arguments before any HIP call, the product refuses to run without a device, and the conditions the GPU tests
rely on hold for the case table (gate literals, the cap on what the non-positive band leaves undecided, the derived sizes)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import eval_cases as ec                           # noqa: E402
import voxelmorph_amd as vxm                      # noqa: E402
from voxelmorph_amd import _lib, metrics          # noqa: E402
from oracle import ref_loader                     # noqa: E402
from oracle import vxm_oracle as orc              # noqa: E402

NEW = ("vxm_label_overlap", "vxm_label_overlap_blocks", "vxm_warp3d_label_overlap", "vxm_jacdet3d", "vxm_jacdet2d", "vxm_jacdet3d_planes")
OK, BAD_SHAPE, UNSUPPORTED, NULL_POINTER = 0, 1, 2, 3
needs_reference = pytest.mark.skipif(not ref_loader.reference_available(), reason="reference tree not present")


@pytest.fixture(scope="module", autouse=True)
def built_library():
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["bash", os.path.join(ROOT, "voxelmorph_amd", "csrc", "build.sh")])


@pytest.fixture(scope="module")
def ref_utils():
    """the reference's voxelmorph.py.utils; its `nd.volsize2ndgrid` (pystrum, an import-time stub here) is given pystrum's meaning: the
    ij-indexed meshgrid of the volume's index ranges"""
    u = ref_loader.load_reference().py.utils
    if not hasattr(u.nd, "volsize2ndgrid"):
        u.nd.volsize2ndgrid = lambda volsize: np.meshgrid(*[np.arange(e) for e in volsize], indexing="ij")
    return u


# ---- the arbiters against the live reference
@needs_reference
def test_float64_jacobian_restatement_is_the_reference(ref_utils):
    for row in ec.JAC_ROWS:
        for d in ec.jac_arrays(row):
            disp = ec.to_last(d).astype(np.float64)
            assert np.array_equal(ec.ref_jacdet(disp, np.float64), ref_utils.jacobian_determinant(disp)), row[0]
    for vol in ec.EXACT_SHAPES:
        for kind in ec.EXACT_KINDS:
            disp = ec.to_last(ec.exact_field(vol, kind)[0]).astype(np.float64)
            assert np.array_equal(ec.ref_jacdet(disp), ref_utils.jacobian_determinant(disp)), (vol, kind)


@needs_reference
def test_dice_arbiter_is_the_reference(ref_utils, g_dice):
    for regime in ec.OVL_REGIMES:
        a, b = ec.label_maps(regime, 1, 4099, 5)
        for labels, zero in ((ec.LABELS30, False), ([5, 0, 3, 5, 99, -2], True), ([5, 0, 3, 5, 99, -2], False), (None, False), (None, True)):
            want = ref_utils.dice(a[0], b[0], labels=None if labels is None else np.array(labels), include_zero=zero)
            assert np.array_equal(orc.dice_metric(a[0], b[0], labels, zero), want), (regime, labels, zero)
    assert np.array_equal(orc.dice_metric(g_dice["a"], g_dice["b"], [1, 2, 3, 5]), g_dice["dice"])


def test_counts_arbiter_gives_the_dice_arbiter():
    a, b = ec.label_maps("runs", 2, 3001, 6)
    c = ec.np_counts(a, b, ec.LABELS30)
    for bi in range(2):
        assert np.array_equal(metrics._dice_from_counts(c[bi:bi + 1], np.arange(30))[0], orc.dice_metric(a[bi], b[bi], ec.LABELS30))


# ---- host pieces
@needs_reference
def test_read_pair_list_equals_the_reference(ref_utils, tmp_path):
    p = tmp_path / "pairs.txt"
    p.write_text("a/1 b/2\n\n  c/3\td/4  \ne/5   f/6\n")
    q = tmp_path / "pairs.csv"
    q.write_text("a 1,b 2\n\nc,d\n")
    mine = vxm.py.utils.read_pair_list
    for kw in ({}, {"prefix": "/data/"}, {"suffix": "/seg.npz"}, {"prefix": "x_", "suffix": ".nii.gz"}):
        assert mine(str(p), **kw) == ref_utils.read_pair_list(str(p), **kw), kw
        assert mine(str(q), delim=",", **kw) == ref_utils.read_pair_list(str(q), delim=",", **kw), kw
    assert mine(str(p), prefix="P")[1] == ["Pc/3", "Pd/4"]
    assert vxm.py.utils.read_file_list(str(p), suffix="!") == ref_utils.read_file_list(str(p), suffix="!")


def test_py_utils_mirrors_the_reference_path():
    from voxelmorph_amd import data
    u = vxm.py.utils
    assert u.load_volfile is data.load_volfile and u.save_volfile is data.save_volfile
    assert u.dice is metrics.dice and u.jacobian_determinant is metrics.jacobian_determinant
    import inspect
    assert list(inspect.signature(u.dice).parameters) == ["array1", "array2", "labels", "include_zero"]
    assert list(inspect.signature(u.read_pair_list).parameters) == ["filename", "delim", "prefix", "suffix"]
    assert list(inspect.signature(u.jacobian_determinant).parameters) == ["disp"]


def test_eval_script_carries_every_flag_of_the_reference_script():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "scripts", "test.py"), "--help"]).decode()
    flags = ["--gpu", "--model", "--pairs", "--img-suffix", "--seg-suffix", "--img-prefix", "--seg-prefix", "--labels", "--multichannel"]
    ref_script = os.path.join(ref_loader.REFERENCE_ROOT, "scripts", "tf", "test.py")
    if os.path.exists(ref_script):
        assert re.findall(r"add_argument\('(--[a-z-]+)'", open(ref_script).read()) == flags
    for f in flags + ["--jacobian"]:
        assert f in out, f


def test_label_plan_follows_the_reference_label_handling():
    labels, uniq, where = metrics._label_plan([5, 0, 3, 5, 99, -2, 0.1, np.nan], False)
    assert labels.tolist()[:6] == [5, 3, 5, 99, -2, 0.1] and np.isnan(labels[6])           # 0 dropped, order and duplicates kept
    assert uniq.tolist() == [-2, 3, 5, 99]                                                   # 0.1 is no fp32 value, NaN equals nothing
    assert where.tolist() == [2, 1, 2, 3, 0, -1, -1]
    labels, uniq, where = metrics._label_plan([5, 0, 3], True)
    assert uniq.tolist() == [0, 3, 5] and where.tolist() == [2, 0, 1]
    counts = np.array([[[0, 0, 0], [4, 4, 4], [1, 1, 3]]], np.int64)
    assert metrics._dice_from_counts(counts, where).tolist() == [[0.5, 0.0, 1.0]]            # absent label: 0 / eps = 0.0


# ---- the ABI
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "vxm_hip.h")).read()
    declared = set(re.findall(r"\b(vxm_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (vxm_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert re.search(r"#define\s+VXM_LABELS_MAX\s+1024\b", header) and metrics.LABELS_MAX == 1024
    assert _lib.lib().vxm_version() >= 503


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    h = _lib.lib()
    buf = ctypes.create_string_buffer(64)            # never dereferenced: every call below fails its validation first
    p = ctypes.addressof(buf)
    for L in (0, 1025, -1):
        assert h.vxm_label_overlap(p, p, p, L, p, 1, 8, None) == UNSUPPORTED, L
        assert h.vxm_warp3d_label_overlap(p, p, p, p, p, L, p, 1, 4, 4, 4, None) == UNSUPPORTED, L
    assert b"labels" in h.vxm_last_error_string()
    for vol in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4)):
        assert h.vxm_jacdet3d(p, p, p, 1, *vol, None) == BAD_SHAPE, vol
        assert h.vxm_warp3d_label_overlap(p, p, p, p, p, 3, p, 1, *vol, None) == BAD_SHAPE, vol
    for vol in ((1, 4), (4, 1)):
        assert h.vxm_jacdet2d(p, p, p, 1, *vol, None) == BAD_SHAPE, vol
    assert h.vxm_jacdet3d(p, p, p, 0, 4, 4, 4, None) == BAD_SHAPE and h.vxm_label_overlap(p, p, p, 3, p, 1, 0, None) == BAD_SHAPE
    assert b"np.gradient" in h.vxm_last_error_string() or b"bad shape" in h.vxm_last_error_string()
    for args in ((None, p, p, 3, p), (p, None, p, 3, p), (p, p, None, 3, p), (p, p, p, 3, None)):
        assert h.vxm_label_overlap(*args, 1, 8, None) == NULL_POINTER, args
    for args in ((None, p, p, p, p, 3, p), (p, None, p, p, p, 3, p), (p, p, None, p, p, 3, p), (p, p, p, p, None, 3, p), (p, p, p, p, p, 3, None)):
        assert h.vxm_warp3d_label_overlap(*args, 1, 4, 4, 4, None) == NULL_POINTER, args
    assert h.vxm_jacdet3d(None, p, p, 1, 4, 4, 4, None) == NULL_POINTER and h.vxm_jacdet3d(p, None, None, 1, 4, 4, 4, None) == NULL_POINTER
    assert h.vxm_jacdet2d(None, p, p, 1, 4, 4, None) == NULL_POINTER and h.vxm_jacdet2d(p, None, None, 1, 4, 4, None) == NULL_POINTER
    assert b"null pointer" in h.vxm_last_error_string()


def test_metrics_have_no_cpu_fallback():
    with pytest.raises(_lib.VxmHipError, match="no CPU fallback"):
        metrics.label_overlap(torch.zeros(1, 8), torch.zeros(1, 8), [1, 2])
    with pytest.raises(_lib.VxmHipError, match="no CPU fallback"):
        metrics.dice(torch.zeros(8), torch.zeros(8), [1])
    with pytest.raises(_lib.VxmHipError, match="no CPU fallback"):
        metrics.jacobian_determinant(torch.zeros(3, 4, 4, 4))
    with pytest.raises(_lib.VxmHipError, match="no CPU fallback"):
        metrics.warped_dice(torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4), [1])
    with pytest.raises(ValueError, match="2\\^24"):
        metrics._as_f32_device(np.array([1 << 24]), "x", torch.device("cpu"))
    with pytest.raises(ValueError, match="exactly"):
        metrics._as_f32_device(np.array([0.1]), "x", torch.device("cpu"))


# ---- conditions of the case table
def test_overlap_sizes_are_derived_from_the_launch_geometry():
    h = _lib.lib()
    for n in ec.OVL_N + (1024, 2048, 2049, 1023 * 1024 + 1, 1 << 30):
        assert h.vxm_label_overlap_blocks(n) == ec.ovl_blocks(n), n
    n2 = ec.OVL_SECOND_PASS_N
    grid = h.vxm_label_overlap_blocks(n2)
    assert grid == ec.OVL_MAX_BLOCKS == 256
    assert n2 // ec.OVL_VEC > grid * ec.OVL_THREADS >= (n2 - ec.OVL_VEC) // ec.OVL_VEC          # the first N with a second pass
    assert h.vxm_label_overlap_blocks(n2 - ec.OVL_VEC) == grid
    assert any(n % ec.OVL_VEC for n in ec.OVL_N) and ec.OVL_BLOCK_SHARE + 1 in ec.OVL_N and set((1, 63, 64, 65, 255, 257)) <= set(ec.OVL_N)
    assert len(ec.LABELS30) == 30 and np.all(np.diff(ec.LABELS30) > 0) and len(ec.LABELS1024) == 1024 and ec.LABELS1024[0] < 0
    # the regimes are what they claim: distinct labels per 64 consecutive voxels
    a, _ = ec.label_maps("runs", 1, 64 * 200, 1)
    per = [len(np.unique(g)) for g in a.reshape(-1, 64)]
    assert 1 <= min(per) and max(per) <= 4 and np.mean(per) < 3
    a, _ = ec.label_maps("distinct", 1, 64 * 200, 1)
    assert min(len(np.unique(g)) for g in a.reshape(-1, 64)) > 2 * 4                             # far beyond the rounds a wave agrees on
    a, b = ec.label_maps("single", 1, 100, 1)
    assert len(np.unique(a)) == 1 and np.array_equal(a, b)


def test_jacobian_shapes_reach_every_launch_path():
    h = _lib.lib()
    rows = {r[0]: r for r in ec.JAC_ROWS}
    for r in ec.JAC_ROWS:
        if len(r[2]) == 3:
            assert h.vxm_jacdet3d_planes(*r[2]) == ec.jac_planes(r[2]), r[0]
    assert h.vxm_jacdet3d_planes(160, 192, 224) == ec.jac_planes((160, 192, 224)) == 27 and h.vxm_jacdet3d_planes(1, 4, 4) == 0
    D = rows["j3_chunks"][2][0]
    planes = ec.jac_planes(rows["j3_chunks"][2])
    assert planes == 2 and D % planes == 1                                    # blocks that march, and a partial last chunk
    assert all(ec.jac_planes(rows[n][2]) == 1 for n in ("j3_min", "j3_odd", "j3_wave", "j3_march"))
    assert int(np.prod(rows["j2_stride"][2])) > ec.JAC_MAX_BLOCKS * ec.JAC_THREADS > int(np.prod(rows["j2_march"][2]))
    assert rows["j3_wave"][2][2] > 64 and rows["j2_wave"][2][1] > 64


def test_warp_cases_reach_what_they_claim():
    for shape in ec.WARP_SHAPES:
        _, flow, _ = ec.warp_case(shape, "ties")
        assert np.all(np.abs(flow - np.floor(flow)) == 0.5)
        _, flow, _ = ec.warp_case(shape, "outside")
        loc = flow[0] + np.moveaxis(ec.grid_of(shape, np.float32), -1, 0)
        out = np.zeros(shape, bool)
        for ax, n in enumerate(shape):
            out |= (np.rint(loc[ax]) < 0) | (np.rint(loc[ax]) > n - 1)
        assert 0.2 < out.mean() < 0.9
        _, flow, _ = ec.warp_case(shape, "far")
        assert np.all(np.abs(flow) == 1e4)


def _recorded():
    out = {}
    for line in open(os.path.join(ROOT, "profiles", "pr06_eval_gates_cpu.txt")):
        if line.startswith("GATE"):
            key, value = line[4:].rsplit(None, 1)
            out[key.strip()] = float(value)
    return out


def test_gpu_gates_are_four_times_the_measured_reference_error():
    """Every literal of test_gpu_eval.py is a GATE line of the committed output of tools/eval_gates.py and the other way round, and
    recomputing them here gives the same figures (numpy's elementwise fp32 arithmetic; the norms may differ in the last digit)."""
    import test_gpu_eval as T
    used = {}
    for cls, (rel, mabs) in T.JAC_GATES.items():
        used["jac %s rel_l2" % cls] = rel
        used["jac %s max_abs" % cls] = mabs
    for name, m in T.JAC_BANDS.items():
        used["jac %s band" % name] = m
    assert used == _recorded()
    assert set(T.JAC_GATES) == set(ec.JAC_CLASSES) and set(T.JAC_BANDS) == set(ec.JAC_IDS)

    def close(new, lit):
        return float("%.3e" % new) == lit or lit / 1.05 <= new <= lit * 1.05
    for cls in ec.JAC_CLASSES:
        rel, mabs, rows = ec.jac_class_gates(cls)
        assert close(rel, T.JAC_GATES[cls][0]) and close(mabs, T.JAC_GATES[cls][1]), (cls, rel, mabs)
        for row, (_, ea) in rows:
            assert close(ec.BAND * ea, T.JAC_BANDS[row[0]]), row[0]
    assert ec.MARGIN == 4.0 and ec.BAND == 8.0 and ec.BAND_CAP == 1e-3


def test_nonpositive_band_leaves_at_most_a_thousandth_undecided():
    """from the float64 values alone: at most 0.1 % of a case's voxels have |det64| <= m, and every case with folds keeps them in the band"""
    import test_gpu_eval as T
    folds = 0
    for row in ec.JAC_ROWS:
        d64 = ec.jacdet64(ec.jac_arrays(row))
        m = T.JAC_BANDS[row[0]]
        assert (np.abs(d64) <= m).mean() <= ec.BAND_CAP, row[0]
        lo, hi = ec.count_band(d64, m)
        exact = (d64 <= 0).reshape(d64.shape[0], -1).sum(1)
        assert np.all(lo <= exact) and np.all(exact <= hi)
        folds += int(exact.sum())
    assert folds > 50000                                       # the table does fold: the count is tested on something


def test_exact_and_nonfinite_cases_are_what_they_claim():
    q = ec.exact_field((6, 7, 9), "quarters")
    assert np.all(q * 4 == np.rint(q * 4)) and np.abs(q).max() <= 4
    d64 = ec.jacdet64(q)
    assert np.array_equal(d64.astype(np.float32).astype(np.float64), d64) and (d64 <= 0).sum() > 100      # fp32 holds every determinant; it folds
    for vol in ec.EXACT_SHAPES:
        assert np.all(ec.jacdet64(ec.exact_field(vol, "minus_identity")) == 0) and np.all(ec.jacdet64(ec.exact_field(vol, "zero")) == 1)
    for vol in ec.NF_VOLS:
        for tag, pos in ec.nf_positions(vol).items():
            for val in ec.NF_VALUES:
                bad = ~np.isfinite(ec.jacdet64(ec.nf_field(vol, pos, val))[0])
                assert np.array_equal(bad, ec.stencil_readers(vol, pos)), (vol, tag, val)
            n = int(ec.stencil_readers(vol, pos).sum())
            assert n == {"interior": 2 * len(vol), "face": 2 * len(vol), "corner": len(vol) + 1}[tag], (vol, tag, n)
