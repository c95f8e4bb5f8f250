"""The evaluation kernels of voxelmorph_amd/csrc/metrics.hip -- k_label_overlap, k_warp3d_label_overlap, k_jacdet3d, k_jacdet2d -- through
voxelmorph_amd.metrics on the table of tests/eval_cases.py.  Run on the MI355X box: `pytest -m gpu tests/test_gpu_eval.py -s` prints the
margin of every gate.

Label counts are integers: array_equal to numpy's `array == label` sums, and Dice array_equal to oracle.dice_metric (the reference's
arithmetic on the host).  The fused warp + overlap is array_equal to SpatialTransformer(mode='nearest') followed by label_overlap.  The
Jacobian determinant is array_equal to float64 where fp32 arithmetic is exact, and otherwise within 4 x the error of the reference's own
formula in fp32, per class (tools/eval_gates.py, output committed as profiles/pr06_eval_gates_cpu.txt; tests/test_cpu_eval.py compares the
literals below with it); the non-positive count lies in the band [#(det64 < -m), #(det64 <= m)], m = 8 x that reference's max-abs error."""
import os

import numpy as np
import pytest
import torch

import eval_cases as ec
from oracle import vxm_oracle as orc

pytestmark = pytest.mark.gpu

# tools/eval_gates.py: class -> (rel-L2, max-abs) of det against float64
JAC_GATES = {
    "noise1/2d": (4.737e-07, 3.433e-06), "noise1/3d": (7.565e-07, 6.291e-06),
    "noise3/2d": (2.213e-06, 4.903e-05), "noise3/3d": (2.362e-06, 4.718e-04),
    "noise5/2d": (3.363e-06, 2.497e-04), "noise5/3d": (3.416e-06, 2.077e-03),
    "smooth5/2d": (1.163e-06, 6.995e-06), "smooth5/3d": (1.602e-06, 1.744e-05),
    "noise1@far/2d": (2.687e-05, 4.134e-04), "noise1@far/3d": (3.017e-05, 7.317e-04),
}
# tools/eval_gates.py: row -> m of the non-positive count's band
JAC_BANDS = {
    "j2_min": 1.034e-06, "j2_odd": 3.079e-06, "j2_batch": 6.865e-06, "j2_unaligned": 3.204e-06,
    "j3_min": 2.520e-06, "j3_odd": 1.258e-05, "j3_batch": 1.031e-05, "j3_unaligned": 8.031e-06,
    "j2_wave": 9.806e-05, "j3_wave": 9.436e-04, "j2_march": 4.993e-04, "j3_march": 4.154e-03,
    "j2_smooth": 1.399e-05, "j3_smooth": 3.488e-05, "j2_stride": 8.269e-04, "j3_chunks": 1.463e-03,
}
NF_CLASS = {3: "noise1/3d", 2: "noise1/2d"}


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from voxelmorph_amd import _lib, metrics
    _lib.lib()                     # fails loudly if libvxm_hip.so is missing
    return metrics


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def G1(a):
    """the same values in a view one float into a larger buffer: no 16-byte alignment"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4
    return view


def N(t):
    return t.detach().cpu().numpy()


def gate(what, measured, bound):
    """Assert measured <= bound and print the margin (`pytest -s` / the committed GPU log shows how tight the gate is)."""
    print("[gate] %-78s measured %.3e  bound %.3e" % (what, measured, bound))
    assert measured <= bound, "%s: %.3e > %.3e" % (what, measured, bound)


def check_overlap(M, a, b, labels, up=G):
    """counts against numpy, Dice against the arbiter per batch item; returns the device counts"""
    got = M.label_overlap(up(a), up(b), labels)
    assert got.dtype == torch.int64 and tuple(got.shape) == (a.shape[0], len(labels), 3)
    want = ec.np_counts(a, b, labels)
    assert np.array_equal(N(got), want), "counts differ at %s" % np.argwhere(N(got) != want)[:6].tolist()
    for bi in range(a.shape[0]):
        assert np.array_equal(M.dice(up(a[bi]), up(b[bi]), labels, include_zero=True), orc.dice_metric(a[bi], b[bi], labels, include_zero=True))
    return got


# ---- label overlap
@pytest.mark.parametrize("n", ec.OVL_N)
def test_label_overlap_sizes(M, n):
    """every size class of the launch: below / at / past a wave, a scalar tail, a second block, a second grid-stride pass; B = 1 and 3"""
    a, b = ec.label_maps("runs", 3, n, 100 + n % 97)
    check_overlap(M, a, b, ec.LABELS30)
    check_overlap(M, a[:1], b[:1], ec.LABELS30)


@pytest.mark.parametrize("regime", ec.OVL_REGIMES)
def test_label_overlap_regimes(M, regime):
    """one address for every lane; the agreed rounds; every lane distinct (the per-lane path); and each of them from unaligned rows"""
    n = 3 * ec.OVL_BLOCK_SHARE + 77
    a, b = ec.label_maps(regime, 3, n, 7)                    # n % 4 == 1: the three rows of a batch are aligned differently
    check_overlap(M, a, b, ec.LABELS64 if regime == "distinct" else ec.LABELS30)
    check_overlap(M, a, b, ec.LABELS30, up=G1)                # one float off: the scalar head
    x, y = G1(a), G(b)                                        # rows misaligned DIFFERENTLY: the all-scalar path
    assert np.array_equal(N(M.label_overlap(x, y, ec.LABELS30)), ec.np_counts(a, b, ec.LABELS30))


@pytest.mark.parametrize("L", (1, 30, 1024))
def test_label_overlap_list_lengths(M, L):
    labels = {1: ec.LABELS30[4:5], 30: ec.LABELS30, 1024: ec.LABELS1024}[L]
    rng = np.random.default_rng(L)
    n = 5000
    a = rng.integers(-600, 600, (2, n)).astype(np.float32) if L == 1024 else ec.label_maps("runs", 2, n, L)[0]
    b = np.where(rng.random((2, n)) < 0.7, a, np.roll(a, 11, 1)).astype(np.float32)
    got = check_overlap(M, a, b, labels)
    assert int(N(got)[..., 0].sum()) > 0


def test_dice_label_handling(M, g_dice):
    """unsorted lists with a duplicate and 0 (include_zero both ways), an absent label (0 / eps = 0.0), negative labels, labels=None, the
    reference-generated golden, numpy and integer inputs"""
    a, b = ec.label_maps("runs", 1, 4099, 5)
    a, b = a[0].copy(), b[0].copy()
    a[::7] = -3.0
    b[::14] = -3.0
    for labels in ([5, 0, 3, 5, 99, -3], [54, 2, 17], [-3], [99], [0], []):
        for zero in (False, True):
            got = M.dice(G(a), G(b), labels, include_zero=zero)
            want = orc.dice_metric(a, b, labels, include_zero=zero)
            assert got.dtype == np.float64 and np.array_equal(got, want), (labels, zero, got, want)
    assert M.dice(G(a), G(b), [99])[0] == 0.0
    for zero in (False, True):
        assert np.array_equal(M.dice(G(a), G(b), include_zero=zero), orc.dice_metric(a, b, None, include_zero=zero))
    assert np.array_equal(M.dice(a, b.astype(np.int32), [5, 3, -3]), orc.dice_metric(a, b, [5, 3, -3]))        # numpy in, integer dtype
    assert np.array_equal(M.dice(G(a).to(torch.int32), G(b), [5, 3, -3]), orc.dice_metric(a, b, [5, 3, -3]))
    ga, gb = g_dice["a"], g_dice["b"]
    assert np.array_equal(M.dice(ga, gb, [1, 2, 3, 5]), g_dice["dice"])
    assert np.array_equal(M.dice(G(ga), G(gb), [1, 2, 3, 5]), g_dice["dice"])
    import voxelmorph_amd as vxm
    assert np.array_equal(vxm.py.utils.dice(G(ga), G(gb), labels=[1, 2, 3, 5]), g_dice["dice"])
    with pytest.raises(ValueError, match="strictly increasing"):
        M.label_overlap(G(a[None]), G(b[None]), [3, 2])


def test_label_overlap_special_values(M):
    """2.5, NaN, +Inf and -0.0 voxels: a value that is not in the list counts nowhere, -0.0 counts as 0 -- `array == label`"""
    a, b = ec.label_maps("runs", 1, 2051, 9)
    rng = np.random.default_rng(3)
    for k, v in enumerate(ec.SPECIAL_VALUES):
        a[0, rng.integers(0, a.shape[1], 40)] = v
        b[0, rng.integers(0, a.shape[1], 40)] = v
        a[0, 64 * k: 64 * k + 64] = v                         # a whole wave of it in one map
        b[0, 64 * k + 32: 64 * k + 96] = v
    a[0, 700:764] = np.nan
    b[0, 700:764] = np.nan                                    # NaN against NaN: still no match
    labels = np.concatenate([[0.0], ec.LABELS30]).astype(np.float32)
    got = check_overlap(M, a, b, labels)
    assert int(N(got)[0, 0, 1]) >= 64                         # the -0.0 voxels are counted as label 0
    with np.errstate(invalid="ignore"):
        assert np.array_equal(M.dice(G(a[0]), G(b[0]), [2.5, 3], include_zero=True), orc.dice_metric(a[0], b[0], [2.5, 3], include_zero=True))
        got_none, want_none = M.dice(G(a[0]), G(b[0])), orc.dice_metric(a[0], b[0])      # the union holds NaN and Inf
    assert np.array_equal(got_none, want_none)


def test_label_overlap_is_bit_reproducible(M):
    a, b = ec.label_maps("distinct", 2, 50001, 21)
    x, y = G(a), G(b)
    first = M.label_overlap(x, y, ec.LABELS64)
    assert torch.equal(first, M.label_overlap(x, y, ec.LABELS64))
    assert np.array_equal(N(first), ec.np_counts(a, b, ec.LABELS64))


# ---- fused warp + overlap
def two_kernels(M, seg, flow, fixed, labels):
    import voxelmorph_amd as vxm
    warped = vxm.layers.SpatialTransformer(seg.shape[2:], mode="nearest").cuda()(seg, flow)
    return warped, M.label_overlap(warped.reshape(seg.shape[0], -1), fixed.reshape(seg.shape[0], -1), labels)


def fused_counts(M, seg, flow, fixed, labels, warped):
    from voxelmorph_amd._lib import call, ptr, stream
    lab, L = M._device_labels(labels, seg.device)
    counts = torch.empty((seg.shape[0], L, 3), dtype=torch.int64, device=seg.device)
    call("vxm_warp3d_label_overlap", ptr(seg), ptr(flow), ptr(fixed), ptr(warped), ptr(lab), L, ptr(counts), seg.shape[0], *seg.shape[2:], stream())
    return counts


@pytest.mark.parametrize("kind", ec.WARP_FLOWS)
@pytest.mark.parametrize("shape", ec.WARP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_warp_overlap_equals_the_two_kernels(M, shape, kind):
    labels = np.concatenate([[0.0], ec.LABELS30]).astype(np.float32)          # 0 listed: samples pushed outside are counted
    seg, flow, fixed = (G(x) for x in ec.warp_case(shape, kind, seed=len(kind), B=2))
    want_w, want_c = two_kernels(M, seg, flow, fixed, labels)
    warped = torch.full_like(seg, -7.0)
    got_c = fused_counts(M, seg, flow, fixed, labels, warped)
    assert torch.equal(warped, want_w) and torch.equal(got_c, want_c)
    assert torch.equal(fused_counts(M, seg, flow, fixed, labels, None), want_c)               # warped = NULL: counts only
    if kind in ("outside", "far"):
        assert int(N(got_c)[:, 0, 1].sum()) >= (0.2 if kind == "outside" else 1.0) * seg.numel()
    # the public call: Dice of the fused counts against the arbiter on the two-kernel map
    d, w = M.warped_dice(seg, flow, fixed, ec.LABELS30, return_warped=True)
    assert torch.equal(w, want_w) and d.shape == (2, 30)
    for bi in range(2):
        assert np.array_equal(d[bi], orc.dice_metric(N(want_w)[bi, 0], N(fixed)[bi, 0], ec.LABELS30))
    assert np.array_equal(M.warped_dice(seg[:1], flow[:1], fixed[:1], ec.LABELS30), d[0])


def test_fused_warp_overlap_full_size_real_scan(M):
    """the evaluation protocol at 160 x 192 x 224 on the real scan: its 30 labels under the fixed smooth 5-voxel field of the parity tests"""
    import test_gpu_parity as P
    _, seg, labels = P._real_scan()
    seg30 = np.where(np.isin(seg, labels), seg, 0.0).astype(np.float32)[None, None]
    seg_d, flow = G(seg30), G(P._smooth_svf(seg.shape))
    want_w, want_c = two_kernels(M, seg_d, flow, seg_d, labels)
    d, w = M.warped_dice(seg_d, flow, seg_d, labels, return_warped=True)
    assert torch.equal(w, want_w)
    assert torch.equal(fused_counts(M, seg_d, flow, seg_d, labels.astype(np.float32), None), want_c)
    want = orc.dice_metric(N(want_w)[0, 0], seg30[0, 0], labels=labels)
    print("real scan, 30 labels, 5-voxel field: mean Dice %.6f" % d.mean())
    assert d.shape == (30,) and np.array_equal(d, want) and 0.2 < d.mean() < 0.99


# ---- Jacobian determinant
def run_jac(M, disp, up=G):
    """(det [B, *vol] numpy, stats [B, 2] numpy) through the public calls"""
    t = up(disp)
    return N(M.jacobian_determinant(t)), N(M.nonpositive_jacobian(t))


@pytest.mark.parametrize("vol", ec.EXACT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ec.EXACT_KINDS)
def test_jacobian_exact_cases(M, vol, kind):
    """where fp32 arithmetic is exact the determinant equals float64 and the counts are exact: quarter-valued fields (they fold), -identity
    (every det exactly 0: every voxel counts), zero (det 1, count 0); 2 x 2 (x 2): every voxel a border voxel on every axis"""
    disp = ec.exact_field(vol, kind)
    d64 = ec.jacdet64(disp)
    det, stats = run_jac(M, disp)
    assert det.dtype == np.float32 and np.array_equal(det.astype(np.float64), d64)
    assert stats.tolist() == [[int((d64 <= 0).sum()), 0]]
    if kind == "minus_identity":
        assert stats[0, 0] == d64.size
    if kind == "quarters" and vol == (6, 7, 9):
        assert stats[0, 0] > 100


@pytest.mark.parametrize("row", ec.JAC_ROWS, ids=ec.JAC_IDS)
def test_jacobian_gated_cases(M, row):
    name, B, vol, regime, seed, unaligned = row
    disp = ec.jac_arrays(row)
    d64 = ec.jacdet64(disp)
    det, stats = run_jac(M, disp, G1 if unaligned else G)
    rel, mabs = JAC_GATES[ec.jac_class(row)]
    gate("%s %s det rel-L2" % (name, ec.jac_class(row)), ec.rel_l2(det, d64), rel)
    gate("%s %s det max-abs" % (name, ec.jac_class(row)), ec.max_abs(det, d64), mabs)
    lo, hi = ec.count_band(d64, JAC_BANDS[name])
    print("[band] %-20s det <= 0: kernel %s, float64 %s, admissible [%s, %s]" % (
        name, stats[:, 0].tolist(), (d64 <= 0).reshape(B, -1).sum(1).tolist(), lo.tolist(), hi.tolist()))
    assert np.all(lo <= stats[:, 0]) and np.all(stats[:, 0] <= hi)
    assert np.array_equal(stats[:, 0], (det <= 0).reshape(B, -1).sum(1)) and np.all(stats[:, 1] == 0)       # the count is of the det it wrote
    assert M.nonpositive_jacobian_fraction(G(disp)) == stats[:, 0].sum() / float(B * np.prod(vol))


@pytest.mark.parametrize("val", ec.NF_VALUES, ids=("nan", "inf", "-inf"))
@pytest.mark.parametrize("where", ("interior", "face", "corner"))
@pytest.mark.parametrize("vol", ec.NF_VOLS, ids=lambda s: "x".join(map(str, s)))
def test_jacobian_nonfinite_displacement_poisons_its_stencil_only(M, vol, where, val):
    pos = ec.nf_positions(vol)[where]
    for channel in range(len(vol)):
        disp = ec.nf_field(vol, pos, val, channel)
        readers = ec.stencil_readers(vol, pos)
        det, stats = run_jac(M, disp)
        assert np.array_equal(~np.isfinite(det[0]), readers), "non-finite at %s, stencil readers %s" % (
            np.argwhere(~np.isfinite(det[0])).tolist(), np.argwhere(readers).tolist())
        assert stats[0, 1] == readers.sum()
        clean = disp.copy()
        clean[(0, channel) + tuple(pos)] = 0.0
        d64 = ec.jacdet64(clean)[0]                                    # elsewhere the bad value is not read: any finite value gives the same
        rel, mabs = JAC_GATES[NF_CLASS[len(vol)]]
        assert ec.max_abs(det[0][~readers], d64[~readers]) <= mabs and ec.rel_l2(det[0][~readers], d64[~readers]) <= rel


def test_jacobian_optional_outputs_layouts_and_reproducibility(M):
    from voxelmorph_amd._lib import call, ptr, stream
    for row in (r for r in ec.JAC_ROWS if r[0] in ("j3_wave", "j2_wave", "j3_chunks", "j2_stride")):
        disp = ec.jac_arrays(row)
        t = G(disp)
        det, stats = run_jac(M, disp)
        det2, stats2 = run_jac(M, disp)
        assert np.array_equal(det.view(np.uint32), det2.view(np.uint32)) and np.array_equal(stats, stats2)      # two runs, bit for bit
        # both outputs from one launch equal the det-only and stats-only launches
        both_d = torch.full(det.shape, -9.0, device="cuda")
        both_s = torch.full((1, 2), -9, dtype=torch.int64, device="cuda")
        call("vxm_jacdet3d" if len(row[2]) == 3 else "vxm_jacdet2d", ptr(t), ptr(both_d), ptr(both_s), 1, *row[2], stream())
        assert np.array_equal(N(both_d).view(np.uint32), det.view(np.uint32)) and np.array_equal(N(both_s), stats)
        # layouts: no batch axis; the reference's numpy layout [*vol, nd] equals the tensor path
        assert np.array_equal(N(M.jacobian_determinant(t[0])), det[0]) and np.array_equal(N(M.nonpositive_jacobian(t[0])), stats[0])
        out = M.jacobian_determinant(ec.to_last(disp[0]))
        assert isinstance(out, np.ndarray) and np.array_equal(out, det[0])
    with pytest.raises(Exception, match="extent|bad shape"):
        M.jacobian_determinant(torch.zeros(1, 3, 1, 4, 4, device="cuda"))


def test_eval_script_prints_the_reference_report(M, tmp_path):
    """scripts/test.py on a list of two npz pairs: the reference's per-pair line and its two summary lines, with the Dice of the protocol"""
    import subprocess
    import sys
    import voxelmorph_amd as vxm
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    vol = (16, 16, 16)
    torch.manual_seed(0)
    model = vxm.networks.VxmDense(vol, int_steps=7, int_downsize=2)
    with torch.no_grad():
        model.flow.weight.normal_(0, 0.05)
    model.save(str(tmp_path / "model.pt"))
    rng = np.random.default_rng(0)
    names = ["s0", "s1", "s2"]
    segs = {}
    for k, n in enumerate(names):
        os.makedirs(tmp_path / n)
        seg = ec.label_maps("runs", 1, int(np.prod(vol)), 50 + k)[0].reshape(vol)
        segs[n] = seg
        np.savez(tmp_path / n / "img.npz", vol=rng.random(vol).astype(np.float32))
        np.savez(tmp_path / n / "seg.npz", seg=seg.astype(np.int32))
    (tmp_path / "pairs.txt").write_text("s0 s1\ns2 s0\n")
    np.save(tmp_path / "labels.npy", ec.LABELS30.astype(np.int32))
    out = subprocess.check_output([sys.executable, os.path.join(root, "scripts", "test.py"), "--model", str(tmp_path / "model.pt"),
                                   "--pairs", str(tmp_path / "pairs.txt"), "--img-prefix", str(tmp_path) + "/", "--seg-prefix", str(tmp_path) + "/",
                                   "--img-suffix", "/img.npz", "--seg-suffix", "/seg.npz", "--labels", str(tmp_path / "labels.npy"), "--jacobian"],
                                  timeout=300).decode()
    print(out)
    lines = [ln for ln in out.splitlines() if ln.strip()]
    import re
    pair = [re.fullmatch(r"Pair (\d+)    Reg Time: (\d+\.\d{4})    Dice: (\d\.\d{4}) \+/- (\d\.\d{4})", ln) for ln in lines]
    pair = [m for m in pair if m]
    assert [m.group(1) for m in pair] == ["1", "2"]
    assert sum("non-positive Jacobian fraction" in ln for ln in lines) == 2
    assert re.fullmatch(r"Avg Reg Time: \d+\.\d{4} \+/- \d+\.\d{4}  \(skipping first prediction\)", lines[-2])
    avg = re.fullmatch(r"Avg Dice: (\d\.\d{4}) \+/- (\d\.\d{4})", lines[-1])
    assert avg
    # the same protocol in this process
    model = model.cuda().eval()
    means = []
    with torch.no_grad():
        for k, (mv, fx) in enumerate((("s0", "s1"), ("s2", "s0"))):
            load = lambda n: G(np.load(tmp_path / n / "img.npz")["vol"])[None, None]          # noqa: E731
            _, warp = model(load(mv), load(fx), registration=True)
            d = M.warped_dice(G(segs[mv])[None, None], warp, G(segs[fx])[None, None], ec.LABELS30)
            means.append(np.mean(d))
            assert pair[k].group(3) == "%.4f" % np.mean(d) and pair[k].group(4) == "%.4f" % np.std(d)
    assert avg.group(1) == "%.4f" % np.mean(means) and avg.group(2) == "%.4f" % np.std(means)
