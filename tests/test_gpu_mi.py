"""The mutual information loss (csrc/mi.hip, vxm.losses.MutualInformation) on the device against the float64 arbiter of tests/mi_cases.py.

Every row of the table runs through the C ABI (MIFn -> vxm_mi_fwd / vxm_mi_bwd) and is held to the gates of its class: 4 x the error of the
fp32 reference formulation against the arbiter (profiles/pr08_mi_gates_cpu.txt, tools/mi_gates.py).  The margins are printed and written
to profiles/pr08_mi_gpu_tests.log.  Then: bit-repeatability, K padding, +-Inf / NaN voxels, batch independence, hipGraph replay, bidir +
weighted_sum, autocast, a sanity property of the loss on a real scan, and scripts/train.py --image-loss mi."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mi_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "profiles", "pr08_mi_gpu_tests.log")


@pytest.fixture(scope="module")
def vxm():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    import voxelmorph_amd
    from voxelmorph_amd import _lib
    _lib.lib()
    return voxelmorph_amd


@pytest.fixture(scope="module")
def gates():
    return mc.load_gates()


@pytest.fixture(scope="module")
def margins():
    """class -> [worst loss error / gate, worst gradient error / gate]; written to the log when the module is done"""
    seen = {}
    yield seen
    with open(LOG, "w") as f:
        f.write("# tests/test_gpu_mi.py: worst error / gate per class (a gate is 4 x the fp32 reference formulation's error, "
                "profiles/pr08_mi_gates_cpu.txt); < 1 passes\n")
        for cls in sorted(seen):
            f.write("mi class %-11s rows %2d  loss error / gate %.3f  gradient error / gate %.3f\n" % (cls, seen[cls][2], seen[cls][0], seen[cls][1]))


def device_tensor(x, layout):
    x = torch.from_numpy(np.ascontiguousarray(x))
    if layout == "contig":
        return x.cuda()
    if layout == "offset1":                          # starts one float into its storage: not aligned for 16-byte loads
        buf = torch.empty(x.numel() + 1, device="cuda")
        v = buf[1:].view(x.shape)
        v.copy_(x)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v.detach()
    assert layout == "noncontig"
    big = torch.empty(x.shape[:-1] + (2 * x.shape[-1],), device="cuda")
    v = big[..., ::2]
    v.copy_(x)
    assert not v.is_contiguous()
    return v.detach()


def loss_object(vxm, r):
    bins, (lo, hi) = r["bins"], r["clip"]
    if isinstance(bins, int):
        return vxm.losses.MutualInformation(nb_bins=bins, min_clip=lo, max_clip=hi)
    return vxm.losses.MutualInformation(bin_centers=bins, min_clip=lo, max_clip=hi)


def run(vxm, r, yt=None, yp=None, mi=None):
    """(loss, g_true, g_pred) of the HIP path as numpy; the gradients the row does not ask for are None"""
    if yt is None:
        yt, yp = mc.inputs(r)
    t = device_tensor(yt, r["layout"]).requires_grad_(r["grads"] in ("true", "both"))
    p = device_tensor(yp, r["layout"]).requires_grad_(r["grads"] in ("pred", "both"))
    loss = (mi or loss_object(vxm, r)).loss(t, p)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward(torch.tensor(r["gloss"], device="cuda"))
    torch.cuda.synchronize()
    g = [None if v.grad is None else v.grad.cpu().numpy() for v in (t, p)]
    assert all(v is None or v.shape == yt.shape for v in g)
    return float(loss.detach()), g[0], g[1]


@pytest.mark.parametrize("name", mc.IDS)
def test_every_row_within_the_gates_of_its_class(vxm, gates, margins, name):
    r = mc.BY_NAME[name]
    loss, gt, gp = run(vxm, r)
    el, rel, ab, norm = mc.errors(r, loss, gt, gp)
    gate_l, gate_g = mc.gates_of(r, gates)
    eg = ab if r["cls"] in mc.ABS_L2 else rel
    print("mi %-26s class %-11s loss error %.3e (gate %.3e)  gradient %s %.3e (gate %.3e)  arbiter gradient norm %.3e"
          % (name, r["cls"], el, gate_l, "abs-L2" if r["cls"] in mc.ABS_L2 else "rel-L2", eg, gate_g, norm))
    m = margins.setdefault(r["cls"], [0.0, 0.0, 0])
    m[0], m[1], m[2] = max(m[0], el / gate_l), max(m[1], eg / gate_g), m[2] + 1
    assert (gt is None) == (r["grads"] == "pred") and (gp is None) == (r["grads"] == "true")
    assert np.isfinite(loss) and all(g is None or np.isfinite(g).all() for g in (gt, gp))
    assert el <= gate_l, (name, el, gate_l)
    assert eg <= gate_g, (name, eg, gate_g)


def test_the_chunk_rows_straddle_what_the_library_reports(vxm):
    from voxelmorph_amd import _lib
    h = _lib.lib()
    n = {k: int(np.prod(mc.BY_NAME[k]["shape"][1:])) for k in ("chunk_minus_1", "chunk", "chunk_plus_1", "ragged_5_chunks")}
    chunk = int(h.vxm_mi_chunk(n["chunk"]))
    assert chunk == mc.CHUNK and all(int(h.vxm_mi_chunk(v)) == chunk for v in n.values())
    assert n["chunk_minus_1"] == chunk - 1 and n["chunk"] == chunk and n["chunk_plus_1"] == chunk + 1
    assert n["ragged_5_chunks"] > 5 * chunk and n["ragged_5_chunks"] % chunk not in (0, chunk - 1)


@pytest.mark.parametrize("name", ["vol3d", "ragged_5_chunks", "k5"])
def test_loss_and_gradients_repeat_bit_for_bit(vxm, name):
    r = mc.BY_NAME[name]
    first = run(vxm, r)
    for _ in range(2):
        again = run(vxm, r)
        assert again[0] == first[0] and np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])


@pytest.mark.parametrize("name", ["k5", "k31"])
def test_padded_bins_equal_the_call_with_explicit_centres(vxm, name):
    r = mc.BY_NAME[name]
    explicit = vxm.losses.MutualInformation(bin_centers=mc.centres_of(r))
    assert len(explicit.bin_centers) == r["bins"]
    a, b = run(vxm, r), run(vxm, r, mi=explicit)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_infinite_voxels_are_clamped_and_a_nan_voxel_makes_the_loss_nan(vxm):
    r = mc.BY_NAME["vol3d"]
    yt, yp = (v.copy() for v in mc.inputs(r))
    ct, cp = yt.copy(), yp.copy()
    for arr, clamped, big in ((yt, ct, np.inf), (yp, cp, 3.2e38)):
        arr.reshape(-1)[11], clamped.reshape(-1)[11] = big, 1.0
        arr.reshape(-1)[-5], clamped.reshape(-1)[-5] = -big, 0.0
    got, want = run(vxm, r, yt, yp), run(vxm, r, ct, cp)
    assert got[0] == want[0] and np.isfinite(got[0])
    for g, w in zip(got[1:], want[1:]):             # outside the clip range the gradient is zero; on the bound it passes: those four voxels only
        idx = [11, g.size - 5]
        assert np.all(g.reshape(-1)[idx] == 0.0)
        w = w.copy()
        w.reshape(-1)[idx] = 0.0
        assert np.array_equal(g, w)
    yp2 = mc.inputs(r)[1].copy()
    yp2.reshape(-1)[100] = np.nan
    assert np.isnan(run(vxm, r, mc.inputs(r)[0], yp2)[0])


def test_the_samples_of_a_batch_do_not_leak_into_each_other(vxm):
    """B = 3 with three regimes: the loss is the mean of the three B = 1 losses and each sample's gradient is a third of its B = 1 gradient.
    The per-sample statistics are the same numbers; only the scalar factor gloss / (N B) is rounded differently: a few ulp."""
    r = mc.BY_NAME["batch3_mixed"]
    yt, yp = mc.inputs(r)
    loss, gt, gp = run(vxm, r)
    singles = [run(vxm, r, yt[b:b + 1], yp[b:b + 1]) for b in range(3)]
    assert abs(loss - np.mean([s[0] for s in singles], dtype=np.float64)) <= 4 * 2.0 ** -24 * max(1.0, abs(loss))
    for b, s in enumerate(singles):
        for g, g1 in ((gt, s[1]), (gp, s[2])):
            rel = np.linalg.norm(g[b].astype(np.float64) - g1[0].astype(np.float64) / 3.0) / np.linalg.norm(g1[0].astype(np.float64) / 3.0)
            assert rel <= 2.0 ** -21, (b, rel)


def _model_setup(vxm, bidir=False, seed=3):
    from voxelmorph_amd.optim import FlatAdam
    shape = (16, 16, 16)
    torch.manual_seed(seed)
    model = vxm.networks.VxmDense(shape, int_steps=3, int_downsize=2, bidir=bidir).cuda()
    with torch.no_grad():
        model.flow.weight.mul_(2e4)                  # a field of ~0.2 voxels
    I, J = mc.real_pair(1, shape)
    return model, FlatAdam(model, lr=1e-3), torch.from_numpy(J).cuda(), torch.from_numpy(I).cuda()       # moving: the remapped copy


def test_graph_replay_changes_no_bit_of_a_step_with_the_loss(vxm):
    from voxelmorph_amd.graph import GraphedStep
    runs = []
    for enabled in (False, True):
        model, opt, src, trg = _model_setup(vxm)
        mi, reg = vxm.losses.MutualInformation().loss, vxm.losses.Grad("l2", loss_mult=2).loss

        def fwd():
            y, pre = model(src, trg)
            return mi(trg, y) + reg(None, pre)
        step = GraphedStep(fwd, opt, eager_steps=1, enabled=enabled)
        losses = [float(step().detach()) for _ in range(4)]
        torch.cuda.synchronize()
        runs.append((opt.flat_param.clone(), losses, step))
    assert runs[1][2].replays == 3 and runs[1][2].graph is not None and runs[0][2].replays == 0
    assert torch.equal(runs[0][0], runs[1][0]), float((runs[0][0] - runs[1][0]).abs().max())
    assert runs[0][1] == runs[1][1] and all(np.isfinite(runs[0][1])) and runs[0][1][-1] != runs[0][1][0]


def test_bidir_weighted_sum_parameter_gradients_against_the_formulation_on_the_device(vxm, gates):
    model, opt, src, trg = _model_setup(vxm, bidir=True)
    mi, reg = vxm.losses.MutualInformation(), vxm.losses.Grad("l2", loss_mult=2)
    weights = (0.5, 0.5, 0.01)

    def grads(total):
        opt.zero_grad()
        total.backward()
        torch.cuda.synchronize()
        return opt.flat_grad.double().cpu().numpy().copy()
    y_s, y_t, pre = model(src, trg)
    total = vxm.losses.weighted_sum([mi.loss(trg, y_s), mi.loss(src, y_t), reg.loss(None, pre)], weights)
    got_loss, got = float(total.detach()), grads(total)
    y_s, y_t, pre = model(src, trg)
    ref = vxm.losses.weighted_sum([mc.formulation(trg, y_s, mi.bin_centers).float(), mc.formulation(src, y_t, mi.bin_centers).float(),
                                   reg.loss(None, pre)], weights)
    want_loss, want = float(ref.detach()), grads(ref)
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("bidir + weighted_sum: loss %.7f / %.7f, parameter gradients rel-L2 %.3e (gate %.3e), norm %.3e"
          % (got_loss, want_loss, rel, gates["noisy grad_rel_l2"], np.linalg.norm(want)))
    assert np.linalg.norm(want) > 0 and abs(got_loss - want_loss) <= max(gates["noisy loss_abs"], 4 * 2.0 ** -24 * max(1.0, abs(want_loss)))
    assert rel <= gates["noisy grad_rel_l2"]


def test_the_loss_accepts_the_model_output_under_autocast(vxm):
    model, opt, src, trg = _model_setup(vxm)
    opt.zero_grad()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y, pre = model(src, trg)
        loss = vxm.losses.MutualInformation().loss(trg, y) + vxm.losses.Grad("l2", loss_mult=2).loss(None, pre)
    loss.backward()
    torch.cuda.synchronize()
    assert y.dtype == torch.float32 and np.isfinite(float(loss.detach())) and float(opt.flat_grad.abs().max()) > 0
    assert bool(torch.isfinite(opt.flat_grad).all())


def test_misalignment_lowers_the_mutual_information_and_the_gradient_step_lowers_the_loss(vxm):
    """On the real scan: the remapped (contrast-inverted) copy displaced by 2 voxels shares strictly less information with the scan than the
    aligned one, and a small step along -dLoss/dy_pred lowers the loss."""
    shape = (24, 24, 24)
    I, aligned = mc.real_pair(1, shape, shift=0)
    _, shifted = mc.real_pair(1, shape, shift=2)
    mi = vxm.losses.MutualInformation()
    t = torch.from_numpy(I).cuda()
    l_aligned = float(mi.loss(t, torch.from_numpy(aligned).cuda()))
    p = torch.from_numpy(shifted).cuda().requires_grad_()
    loss = mi.loss(t, p)
    loss.backward()
    l_shifted = float(loss.detach())
    print("MI aligned %.6f, displaced by 2 voxels %.6f" % (-l_aligned, -l_shifted))
    assert -l_shifted < -l_aligned and -l_aligned > 0.3
    g = p.grad
    step = 0.01 / float(g.abs().max())               # moves no voxel by more than 0.01 (a third of a bin)
    l_stepped = float(mi.loss(t, (p.detach() - step * g)))
    assert l_stepped < l_shifted, (l_stepped, l_shifted)


def test_train_cli_with_the_mutual_information_loss(vxm, tmp_path):
    rng = np.random.default_rng(3)
    base = rng.random((32, 32, 32)).astype(np.float32)
    names = []
    for i in range(4):
        v = np.roll(base, shift=i, axis=2) + 0.05 * rng.random(base.shape).astype(np.float32)
        np.savez(tmp_path / ("v%d.npz" % i), vol=v if i % 2 == 0 else 1.0 - 0.9 * v)
        names.append(str(tmp_path / ("v%d.npz" % i)))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--img-list", str(tmp_path / "list.txt"),
                        "--model-dir", str(tmp_path / "models"), "--epochs", "2", "--steps-per-epoch", "4", "--image-loss", "mi",
                        "--mi-bins", "16", "--lambda", "1", "--lr", "1e-3"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(ln.split("loss:")[1].split()[0]) for ln in r.stdout.splitlines() if "loss:" in ln]
    assert len(losses) == 2 and all(np.isfinite(losses)) and all(v < 0 for v in losses)          # -MI + a small smoothness term
