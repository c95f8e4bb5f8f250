"""CPU side of the probabilistic velocity field (csrc/prob.hip, losses.KL, networks.VxmDenseProbabilistic): the float64 arbiters of
tests/prob_cases.py agree with an independent restatement of the reference's TensorFlow formulation, the gates are the recorded ones, and the
host refuses what it must before any HIP call."""
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

import prob_cases as pc                           # noqa: E402
import voxelmorph_amd as vxm                      # noqa: E402
from voxelmorph_amd import _lib                   # noqa: E402

NEW_SYMBOLS = ("vxm_kl_workspace_bytes", "vxm_kl_fwd", "vxm_kl_bwd", "vxm_sample_logvar_fwd", "vxm_sample_logvar_bwd")


@pytest.fixture(scope="module")
def rows():
    return {r[0]: pc.row_arrays(r) for r in pc.ROWS}


def test_table_is_well_formed(rows):
    assert pc.ROW_IDS == ["edge_2x2x2", "wide_7x9x70", "ragged_3x40x33", "batch_5x6x40", "init_6x11x37"]
    assert [r[2] for r in pc.ROWS] == [1, 2, 1, 3, 2] and pc.LAMBDAS == (10.0, 25.0) and pc.UPSTREAM == (1.0, -0.37)
    for r in pc.ROWS:
        a = rows[r[0]]
        assert a["params"].dtype == np.float32 and a["params"].shape == (r[2], 6) + r[1] and a["eps"].shape == (r[2], 3) + r[1]
    assert np.all(pc.degree((2, 2, 2)) == 3)
    init = rows["init_6x11x37"]["params"]
    assert np.abs(init[:, 3:] + 10).max() < 0.01 and np.abs(init[:, :3]).max() < 0.01
    assert rows["wide_7x9x70"]["params"][:, 3:].min() < -11 and rows["wide_7x9x70"]["params"][:, 3:].max() > 1
    V = [int(np.prod(r[1])) for r in pc.ROWS]
    assert any(v % 4 for v in V) and any(v % 4 == 0 for v in V)       # both paths of the sampler
    assert pc.LATTICE[1:4] == ((6, 7, 33), 2, 8.0)


def test_lattice_row_is_exact_in_fp32():
    a = pc.lattice_arrays()
    p = a["params"].astype(np.float64)
    assert np.array_equal(2 * p[:, :3], np.round(2 * p[:, :3])) and not p[:, 3:].any() and not a["eps"].any()
    # every term and sum is an exact fp32 / float64 number: evaluating the sums in float32 gives the same integers
    for ax in (2, 3, 4):
        df = np.diff(a["params"][:, :3], axis=ax)
        assert float(np.sum((df * df).astype(np.float64))) * 4 == round(float(np.sum((df * df).astype(np.float64))) * 4)
    z, gp = pc.sample_arbiter(a["params"], a["eps"], a["gz"])
    assert np.array_equal(z, p[:, :3]) and not gp[:, 3:].any()


def _adjacency_degree(size):
    """the reference's degree matrix restated: a field of ones convolved (zero padding) with the 3 x 3 x 3 filter that is 1 on the six
    face neighbours"""
    filt = torch.zeros(1, 1, 3, 3, 3, dtype=torch.float64)
    for off in ((0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)):
        filt[(0, 0) + off] = 1
    return F.conv3d(torch.ones((1, 1) + tuple(size), dtype=torch.float64), filt, padding=1)[0, 0].numpy()


@pytest.mark.parametrize("size", [(2, 2, 2), (2, 3, 5), (6, 7, 33), (3, 40, 33)])
def test_closed_form_degree_is_the_conv_of_ones_with_the_neighbour_filter(size):
    assert np.array_equal(pc.degree(size), _adjacency_degree(size))


def _kl_restated(params, lam):
    """tf/losses.py:294-349 restated in torch float64, channels LAST as there: the axis moved to the front, the squared forward
    differences averaged, the sigma term with the convolved degree matrix"""
    y = params.permute(0, 2, 3, 4, 1)                           # [B, D, H, W, 6]
    ndims = 3
    mean, log_sigma = y[..., :ndims], y[..., ndims:]
    deg = torch.from_numpy(_adjacency_degree(tuple(y.shape[1:4])))[None, ..., None]
    sigma_term = (lam * deg * torch.exp(log_sigma) - log_sigma).mean()
    sm = 0
    for i in range(ndims):
        d = i + 1
        t = mean.permute([d] + [k for k in range(5) if k != d])
        df = t[1:] - t[:-1]
        sm = sm + (df * df).mean()
    prec_term = lam * (0.5 * sm / ndims)
    return 0.5 * ndims * (sigma_term + prec_term)


@pytest.mark.parametrize("name", pc.ROW_IDS)
def test_arbiters_equal_the_restated_reference_formulation(rows, name):
    a = rows[name]
    for lam in pc.LAMBDAS:
        for g in pc.UPSTREAM:
            p = torch.from_numpy(a["params"]).double().requires_grad_()
            loss = _kl_restated(p, lam)
            loss.backward(torch.tensor(g, dtype=torch.float64))
            l64, gp64 = pc.kl_arbiter(a["params"], lam, g)
            assert abs(float(loss.detach()) - l64) <= 1e-13 * abs(l64), (name, lam)
            assert pc.rel_l2(p.grad.numpy(), gp64) < 1e-13, (name, lam, g)
    p = torch.from_numpy(a["params"]).double().requires_grad_()
    mu, ls = p[:, :3], p[:, 3:]
    z = mu + torch.sqrt(torch.exp(ls)) * torch.from_numpy(a["eps"]).double()           # sigma = sqrt(exp(log sigma^2))
    z.backward(torch.from_numpy(a["gz"]).double())
    z64, gp64 = pc.sample_arbiter(a["params"], a["eps"], a["gz"])
    assert pc.rel_l2(z.detach().numpy(), z64) < 1e-14 and pc.rel_l2(p.grad.numpy(), gp64) < 1e-14


def test_arbiter_refuses_an_extent_below_two():
    with pytest.raises(ValueError):
        pc.kl_arbiter(np.zeros((1, 6, 1, 4, 4), np.float32), 10.0)


def test_gates_are_the_recorded_output_of_the_tool():
    text = open(os.path.join(ROOT, "profiles", "pr11_prob_gates_cpu.txt")).read()
    for k in pc.GATE_CLASSES:
        m = re.search(r"largest %s\s+(\S+)\s+-> gate \(x4[^)]*\): (\S+)" % k, text)
        assert m, k
        worst, gate = float(m.group(1)), float(m.group(2))
        assert gate == pc.GATES[k], (k, gate, pc.GATES[k])
        assert abs(gate - max(4 * worst, pc.LOSS_GATE_FLOOR if k == "kl_loss" else 0.0)) <= 2e-3 * gate
    assert pc.GATES["kl_loss"] >= pc.LOSS_GATE_FLOOR
    for r in pc.ROWS:
        assert len(re.findall(r"^%s\s" % r[0], text, re.M)) == len(pc.LAMBDAS) * len(pc.UPSTREAM) + 1, r[0]


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "vxm_hip.h")).read()
    h = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES and re.search(r"\b%s\(" % s, header) and hasattr(h, s), s
    assert h.vxm_version() >= 506
    assert "prob.hip" in open(os.path.join(ROOT, "voxelmorph_amd", "csrc", "build.sh")).read()
    from voxelmorph_amd.torch import functional as VF
    for name in ("KLFn", "SampleLogVarFn", "ProbHeadsFn"):
        assert hasattr(VF, name), name
    assert hasattr(vxm.losses, "KL") and hasattr(vxm.networks, "VxmDenseProbabilistic")


def test_c_entry_points_reject_bad_arguments_before_any_launch():
    h = _lib.lib()
    p = 16                                                   # never dereferenced: the argument checks come first
    for shape in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8)):
        assert h.vxm_kl_fwd(p, 10.0, p, p, 1 << 20, 1, *shape, None) == 1, shape
        assert h.vxm_kl_bwd(p, 10.0, p, p, 1, *shape, None) == 1, shape
        assert h.vxm_kl_workspace_bytes(1, *shape) == 0
    assert h.vxm_kl_fwd(p, 10.0, p, p, 1 << 20, 0, 8, 8, 8, None) == 1
    assert h.vxm_kl_fwd(p, 10.0, p, p, 1 << 20, 1, 2048, 2048, 1024, None) == 1          # 2^32 voxels
    assert h.vxm_kl_fwd(p, float("nan"), p, p, 1 << 20, 1, 8, 8, 8, None) == 2
    assert h.vxm_kl_fwd(None, 10.0, p, p, 1 << 20, 1, 8, 8, 8, None) == 3
    assert h.vxm_kl_fwd(p, 10.0, p, None, 1 << 20, 1, 8, 8, 8, None) == 3
    need = h.vxm_kl_workspace_bytes(2, 8, 8, 8)
    assert need == 8 * 4 * 2 and h.vxm_kl_fwd(p, 10.0, p, p, need - 1, 2, 8, 8, 8, None) == 4
    assert b"workspace" in h.vxm_last_error_string()
    assert h.vxm_kl_bwd(p, 10.0, None, p, 1, 8, 8, 8, None) == 3
    assert h.vxm_sample_logvar_fwd(p, p, p, 0, 64, None) == 1 and h.vxm_sample_logvar_fwd(p, p, p, 1, 0, None) == 1
    assert h.vxm_sample_logvar_fwd(p, None, p, 1, 64, None) == 3
    assert h.vxm_sample_logvar_bwd(p, p, p, p, 1, 0, None) == 1 and h.vxm_sample_logvar_bwd(p, p, p, None, 1, 64, None) == 3
    # at most 512 partials of four float64 sums per sample, whatever the volume (160 x 192 x 224: 508 chunks of 13568 voxels)
    assert h.vxm_kl_workspace_bytes(1, 160, 192, 224) == 8 * 4 * 508 and h.vxm_kl_workspace_bytes(3, 160, 192, 224) == 3 * 8 * 4 * 508
    assert h.vxm_kl_workspace_bytes(1, 1024, 1024, 1024) <= 8 * 4 * 512
    assert h.vxm_kl_workspace_bytes(1, 3, 40, 33) == 8 * 4 * 4                              # 3960 voxels: four chunks of 1024


def test_kl_class_refuses_bad_shapes_and_cpu_tensors():
    kl = vxm.losses.KL(10, (4, 5, 6))
    assert kl.prior_lambda == 10.0 and kl.flow_vol_shape == (4, 5, 6)
    with pytest.raises(ValueError, match="flow_vol_shape"):
        kl.loss(None, torch.zeros(1, 6, 4, 5, 7))
    with pytest.raises(ValueError, match="3-D"):
        kl.loss(None, torch.zeros(1, 4, 5, 6))
    with pytest.raises(ValueError, match="3-D"):
        vxm.losses.KL(10, (5, 6))
    with pytest.raises(ValueError, match="6-channel"):
        kl.loss(None, torch.zeros(1, 3, 4, 5, 6))
    with pytest.raises(ValueError, match="at least 2"):
        vxm.losses.KL(10, (1, 5, 6)).loss(None, torch.zeros(1, 6, 1, 5, 6))
    with pytest.raises(_lib.VxmHipError, match="no CPU fallback"):
        kl.loss(None, torch.zeros(1, 6, 4, 5, 6))
    from voxelmorph_amd.torch import functional as VF
    with pytest.raises(ValueError, match="noise"):
        VF.SampleLogVarFn.apply(torch.zeros(1, 6, 4, 5, 6), torch.zeros(1, 3, 4, 5, 5))
    with pytest.raises(_lib.VxmHipError, match="no CPU fallback"):
        VF.SampleLogVarFn.apply(torch.zeros(1, 6, 4, 5, 6), torch.zeros(1, 3, 4, 5, 6))
    with pytest.raises(_lib.VxmHipError, match="no CPU fallback"):
        VF.ProbHeadsFn.apply(torch.zeros(1, 16, 4, 4, 4), torch.zeros(3, 16, 3, 3, 3), torch.zeros(3), torch.zeros(3, 16, 3, 3, 3), torch.zeros(3))


def test_constructor_head_initialisation_and_checkpoint_round_trip(tmp_path):
    torch.manual_seed(11)
    model = vxm.networks.VxmDenseProbabilistic((16, 16, 16), int_steps=3, bidir=True)
    assert "use_probs" not in model.config and model.config["bidir"] is True and model.config["int_steps"] == 3
    names = [n for n, _ in model.named_children()]
    for n in ("unet_model", "flow", "flow_logsigma", "resize", "integrate", "fullsize", "transformer"):
        assert n in names, n
    assert tuple(model.flow.weight.shape) == (3, 16, 3, 3, 3) == tuple(model.flow_logsigma.weight.shape)
    assert 0 < float(model.flow.weight.std()) < 3e-5 and not model.flow.bias.any()
    assert 0 < float(model.flow_logsigma.weight.std()) < 3e-10 and torch.equal(model.flow_logsigma.bias, torch.full((3,), -10.0))
    assert model.noise is None and "noise" not in model.state_dict()
    n = model.draw_noise(torch.Generator().manual_seed(1), batch=2)
    assert tuple(n.shape) == (2, 3, 16, 16, 16) and n is model.noise and abs(float(n.std()) - 1) < 0.05
    assert "noise" not in model.state_dict()
    path = str(tmp_path / "prob.pt")
    model.save(path)
    again = vxm.networks.VxmDenseProbabilistic.load(path, "cpu")
    assert again.config == model.config and again.bidir
    sa, sb = model.state_dict(), again.state_dict()
    assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    # the deterministic model keeps refusing the flag, as the reference's torch side does
    with pytest.raises(NotImplementedError):
        vxm.networks.VxmDense((16, 16, 16), use_probs=True)
    with pytest.raises(NotImplementedError, match="3-D"):
        vxm.networks.VxmDenseProbabilistic((16, 16))
    with pytest.raises(NotImplementedError, match="3-D"):
        model(torch.zeros(1, 1, 16, 16), torch.zeros(1, 1, 16, 16))
    with pytest.raises(_lib.VxmHipError, match="no CPU fallback"):
        model(torch.zeros(1, 1, 16, 16, 16), torch.zeros(1, 1, 16, 16, 16))


def test_scripts_list_the_new_flags():
    for script, flags in (("train.py", ("--use-probs", "--kl-lambda", "--image-sigma", "0.02")), ("register.py", ("--use-probs", "--sigma"))):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--help"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        for f in flags:
            assert f in out.stdout, (script, f)
