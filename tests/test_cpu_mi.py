"""CPU-side conditions of the mutual information loss: the case table of tests/mi_cases.py and its gates, the arbiter against an independent
explicit-loop evaluation, the public class and its constructor checks, the no-CPU-fallback rule, the scripts' flags and the bound on the
workspace."""
import os
import sys

import numpy as np
import pytest
import torch

import mi_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import voxelmorph_amd as vxm                      # noqa: E402
from voxelmorph_amd import _lib                   # noqa: E402


def test_table_is_well_formed():
    assert len(mc.IDS) == len(set(mc.IDS))
    for r in mc.ROWS:
        yt, yp = mc.inputs(r)
        assert yt.shape == yp.shape == r["shape"] and yt.dtype == yp.dtype == np.float32 and len(r["shape"]) >= 2
        assert 2 <= len(mc.centres_of(r)) <= 32 and r["grads"] in ("pred", "true", "both")
    n = lambda name: int(np.prod(mc.BY_NAME[name]["shape"][1:]))
    assert [n(k) for k in ("n1", "n63", "n64", "n65")] == [1, 63, 64, 65]
    assert [n(k) for k in ("chunk_minus_1", "chunk", "chunk_plus_1")] == [mc.CHUNK - 1, mc.CHUNK, mc.CHUNK + 1]
    assert n("ragged_5_chunks") // mc.CHUNK == 5 and 0 < n("ragged_5_chunks") % mc.CHUNK < 256
    assert {len(mc.centres_of(r)) for r in mc.ROWS} >= {2, 5, 16, 31, 32}
    assert {r["shape"] for r in mc.ROWS} >= {(2, 1, 12, 14, 16), (2, 1, 24, 20), (2, 3, 40), (1, 2, 6, 6, 6)}
    assert {r["shape"][0] for r in mc.ROWS} >= {1, 3} and {r["gloss"] for r in mc.ROWS} == {1.0, -0.37}
    assert {r["layout"] for r in mc.ROWS} == {"contig", "offset1", "noncontig"}
    # the regimes are what their names say
    a, b = mc.inputs(mc.BY_NAME["outside"])
    for v in (a, b):
        assert 0.25 < np.mean((v < 0) | (v > 1)) < 0.75 and (v == 0).any() and (v == 1).any() and v.min() < -0.9 and v.max() > 1.9
    a, b = mc.inputs(mc.BY_NAME["x255"])
    assert a.max() > 200 and 0.5 < np.mean(a > 1) < 0.9
    c = np.asarray(mc.centres_of(mc.BY_NAME["centres"]), np.float32)
    assert all(np.isin(v, c).all() for v in mc.inputs(mc.BY_NAME["centres"]))
    a, b = mc.inputs(mc.BY_NAME["same"])
    assert np.array_equal(a, b)
    a, b = mc.inputs(mc.BY_NAME["real"])
    assert a.std() > 0.05 and b.std() > 0.05 and np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1] < -0.3          # contrast inverted
    # the narrow centres under the wide clip range: exp(-alpha d^2) alone underflows in fp32 for the far voxels
    r = mc.BY_NAME["clip_wider_than_centres"]
    cen = np.asarray(mc.centres_of(r))
    alpha = 1.0 / (2.0 * (0.5 * np.diff(cen).mean()) ** 2)
    assert np.exp(-np.float32(alpha) * np.float32(0.4) ** 2) == 0.0 and mc.inputs(r)[0].min() < 0.01


def test_gradient_norms_and_the_closed_list_of_absolute_gates():
    """rel-L2 is vacuous where the true gradient vanishes: exactly the classes of ABS_L2 are gated by absolute L2 error, and every other row
    has an arbiter gradient norm of at least 1e-3"""
    assert mc.ABS_L2 == ("const_true", "const_pred", "single")
    assert [r["name"] for r in mc.ROWS if r["cls"] == "single"] == ["n1"]
    for r in mc.ROWS:
        _, gt, gp = mc.arbiter(r)
        norm = mc.errors(r, *mc.arbiter(r))[3]
        if r["cls"] in mc.ABS_L2:
            assert norm < 1e-4, (r["name"], norm)
        else:
            assert norm >= mc.MIN_GRAD_NORM, (r["name"], norm)
        assert (gt is None) == (r["grads"] == "pred") and (gp is None) == (r["grads"] == "true")
    l_clip = mc.arbiter(mc.BY_NAME["clip_wider_than_centres"])
    assert np.isfinite(l_clip[0]) and np.isfinite(l_clip[1]).all() and np.isfinite(l_clip[2]).all()


def test_gates_file_is_what_the_tool_computes():
    """every class has its two GATE lines and nothing else is in the file; recomputed here: ATen's summation order depends on the CPU's vector
    width, so a recomputed gate has to agree with the committed one within a factor 1.5, not to the last digit"""
    torch.set_num_threads(1)
    recorded = mc.load_gates()
    assert set(recorded) == {k for cls in mc.CLASSES for k in mc.gate_keys(cls)}
    for cls in mc.CLASSES:
        gl, gg, rows = mc.class_gates(cls)
        assert len(rows) >= 1
        kl, kg = mc.gate_keys(cls)
        for new, lit in ((gl, recorded[kl]), (gg, recorded[kg])):
            assert lit / 1.5 <= new <= lit * 1.5 or max(new, lit) <= mc.MARGIN * mc.HALF_ULP, (cls, new, lit)
    assert mc.MARGIN == 4.0 and mc.loss_floor(mc.BY_NAME["vol3d"]) == 4.0 * 2.0 ** -24 * abs(mc.arbiter(mc.BY_NAME["vol3d"])[0])


def test_arbiter_against_an_explicit_loop_evaluation():
    """the definition, written out voxel by voxel and bin by bin in numpy float64, and its gradient by central differences"""
    r = mc.row("tiny", "noisy", (2, 1, 3, 4), bins=(0.0, 0.2, 0.55, 1.0), clip=(0.05, 0.9))
    yt, yp = mc.inputs(r)
    yt.reshape(-1)[3], yp.reshape(-1)[5] = -0.5, 1.4              # clamped voxels
    cen = np.asarray(mc.centres_of(r), np.float64)
    sigma = 0.5 * np.mean(np.diff(cen))
    alpha = 1.0 / (2.0 * sigma * sigma)

    def explicit(yt, yp):
        B, total = yt.shape[0], 0.0
        for b in range(B):
            a = np.clip(yt[b].reshape(-1).astype(np.float64), 0.05, 0.9)
            c = np.clip(yp[b].reshape(-1).astype(np.float64), 0.05, 0.9)
            N, K = a.size, cen.size
            wa, wb = np.zeros((N, K)), np.zeros((N, K))
            for n in range(N):
                for w, x in ((wa, a[n]), (wb, c[n])):
                    e = [np.exp(-alpha * (x - cen[k]) ** 2) for k in range(K)]
                    for k in range(K):
                        w[n, k] = e[k] / sum(e)
            mi = 0.0
            for i in range(K):
                for j in range(K):
                    pab = sum(wa[n, i] * wb[n, j] for n in range(N)) / N
                    papb = wa[:, i].mean() * wb[:, j].mean() + 1e-7
                    mi += pab * np.log(pab / papb + 1e-7)
            total += mi
        return -total / B
    loss, gt, gp = mc.evaluate(r, torch.float64, yt, yp)
    assert abs(loss - explicit(yt, yp)) < 1e-13
    h = 1e-6
    for arr, g in ((yt, gt), (yp, gp)):
        for idx in (0, 3, 5, 7, 13, 23):
            up, dn = [v.astype(np.float64) for v in (yt, yp)], [v.astype(np.float64) for v in (yt, yp)]
            which = 0 if arr is yt else 1
            up[which].reshape(-1)[idx] += h
            dn[which].reshape(-1)[idx] -= h
            fd = (explicit(*up) - explicit(*dn)) / (2 * h)
            assert abs(fd - g.reshape(-1)[idx]) < 1e-8, (which, idx, fd, g.reshape(-1)[idx])
    assert gt.reshape(-1)[3] == 0.0 and gp.reshape(-1)[5] == 0.0


def test_public_class_and_constructor_checks():
    MI = vxm.losses.MutualInformation
    assert vxm.torch.losses.MutualInformation is MI
    m = MI()
    assert len(m.bin_centers) == 32 and m.bin_centers[0] == 0.0 and m.bin_centers[-1] == 1.0
    assert np.allclose(m.bin_centers, np.linspace(0, 1, 32), atol=1e-15)
    assert abs(m.sigma - 0.5 / 31) < 1e-15 and abs(m.alpha - 1.0 / (2 * m.sigma ** 2)) < 1e-9
    assert len(MI(nb_bins=5, min_clip=-1.0, max_clip=3.0).bin_centers) == 5 and MI(nb_bins=5, min_clip=-1.0, max_clip=3.0).bin_centers[1] == 0.0
    assert MI(bin_centers=[0.0, 0.3, 1.0], nb_bins=3).bin_centers == (0.0, 0.3, 1.0)
    assert abs(MI(bin_centers=[0.0, 0.3, 1.0], sigma_ratio=0.25).sigma - 0.125) < 1e-15
    for kw in (dict(nb_bins=1), dict(nb_bins=33), dict(nb_bins=0), dict(bin_centers=[0.5]), dict(bin_centers=list(np.linspace(0, 1, 33))),
               dict(bin_centers=[0.0, 0.5, 0.5]), dict(bin_centers=[0.0, 0.6, 0.5]), dict(bin_centers=[0.0, 0.5, 1.0], nb_bins=4),
               dict(bin_centers=[0.0, float("nan")]), dict(nb_bins=2.5)):
        with pytest.raises(ValueError):
            MI(**kw)
    for text in ("tf/losses.py:352-367", "restatement", "Local (patch-wise)", "32 bins"):
        assert text in MI.__doc__, text


def test_cpu_tensors_raise():
    m = vxm.losses.MutualInformation()
    with pytest.raises(_lib.VxmHipError, match="no CPU fallback"):
        m.loss(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))


def test_c_entry_points_reject_bad_arguments_before_any_launch():
    import ctypes
    h = _lib.lib()
    assert h.vxm_version() >= 504
    cen = (ctypes.c_float * 3)(0.0, 0.5, 1.0)
    cp = ctypes.cast(cen, ctypes.c_void_p)
    assert h.vxm_mi_fwd(None, None, cp, 3, 8.0, 0.0, 1.0, None, None, None, 0, 1, 64, None) == 3
    assert b"null" in h.vxm_last_error_string()
    assert h.vxm_mi_fwd(None, None, cp, 33, 8.0, 0.0, 1.0, None, None, None, 0, 1, 64, None) == 2
    assert b"33 bins" in h.vxm_last_error_string()
    assert h.vxm_mi_fwd(None, None, cp, 1, 8.0, 0.0, 1.0, None, None, None, 0, 1, 64, None) == 2
    assert h.vxm_mi_bwd(None, None, cp, 3, 8.0, 0.0, 1.0, None, None, None, None, 1, 0, None) == 1
    bad = (ctypes.c_float * 3)(0.0, 0.5, 0.5)
    assert h.vxm_mi_bwd(None, None, ctypes.cast(bad, ctypes.c_void_p), 3, 8.0, 0.0, 1.0, None, None, None, None, 1, 64, None) == 2
    assert b"strictly increasing" in h.vxm_last_error_string()
    assert h.vxm_mi_workspace_bytes(0, 64, 32) == 0 and h.vxm_mi_workspace_bytes(1, 64, 33) == 0 and h.vxm_mi_chunk(0) == 0


def test_workspace_is_bounded_in_n():
    """O(workgroups x K^2): no buffer proportional to N x K"""
    h = _lib.lib()
    N = 160 * 192 * 224
    one, eight = h.vxm_mi_workspace_bytes(1, N, 32), h.vxm_mi_workspace_bytes(1, 8 * N, 32)
    assert 0 < one < 64 * 2 ** 20 and eight / one < 2.0
    assert one < 4 * N * 32 / 100                                   # a hundredth of ONE weight tensor
    assert h.vxm_mi_workspace_bytes(1, 1, 2) >= 8 + 4 * (32 * 32 + 64)
    for n in (1, mc.CHUNK - 1, mc.CHUNK, mc.CHUNK + 1, N, 8 * N):
        chunk = h.vxm_mi_chunk(n)
        parts = -(-n // chunk)
        assert chunk >= mc.CHUNK and chunk % 256 == 0 and parts <= 512
        assert h.vxm_mi_workspace_bytes(3, n, 32) == 8 * 4 + 3 * (4 * parts + 8 * -(-parts // 16)) * (32 * 32 + 64)


def test_scripts_accept_the_mutual_information_flags():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import train
        import train_semisupervised_seg as semi
    finally:
        sys.path.pop(0)
    a = train.parse(["--img-list", "x", "--image-loss", "mi", "--mi-bins", "16"])
    assert a.image_loss == "mi" and a.mi_bins == 16
    assert train.parse(["--img-list", "x"]).mi_bins == 32 and train.parse(["--img-list", "x"]).image_loss == "mse"
    b = semi.parse(["--img-list", "x", "--labels", "l.npy", "--image-loss", "mi", "--mi-bins", "16"])
    assert b.image_loss == "mi" and b.mi_bins == 16
    for mod in (train, semi):
        text = open(mod.__file__).read()
        assert '"mse", "ncc" or "mi"' in text and "'mse', 'ncc' or 'mi'" in text
