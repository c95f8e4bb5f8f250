"""The probabilistic velocity field on the device: the kernels of csrc/prob.hip (`losses.KL`, `functional.SampleLogVarFn`), the two heads
(`functional.ProbHeadsFn`) and `networks.VxmDenseProbabilistic` against the float64 arbiters of tests/prob_cases.py.  Gates: tools/prob_gates.py
(profiles/pr11_prob_gates_cpu.txt) -- 4 x the error of the plain fp32 evaluation of the same definition on the same rows; the whole model
against the oracle with the tolerances tests/test_gpu_parity.py uses for this depth (atol 2e-5 forward, rel-L2 5e-4 parameter gradients).
Run with -s for the margins (profiles/pr11_prob_gpu_tests.log)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import prob_cases as pc                           # noqa: E402


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
def VF(vxm):
    from voxelmorph_amd.torch import functional
    return functional


@pytest.fixture(scope="module")
def rows():
    return {r[0]: pc.row_arrays(r) for r in pc.ROWS}


def check(name, what, got, want, gate):
    err = pc.rel_l2(got, want)
    print("%-34s %-10s rel-L2 %.3e  gate %.2e  margin %s" % (name, what, err, gate, "%.1fx" % (gate / err) if err else "exact"))
    assert np.isfinite(got).all() and err <= gate, (name, what, err, gate)


def kl_run(vxm, params, lam, g):
    p = G(params).requires_grad_()
    loss = vxm.losses.KL(lam, params.shape[2:]).loss(None, p)
    loss.backward(torch.tensor(g, dtype=torch.float32, device="cuda"))
    assert loss.dtype == torch.float32 and loss.dim() == 0
    return N(loss), N(p.grad)


@pytest.mark.parametrize("name", pc.ROW_IDS)
def test_kl_rows_against_the_arbiter(vxm, rows, name):
    a = rows[name]
    for lam in pc.LAMBDAS:
        for g in pc.UPSTREAM:
            loss, gp = kl_run(vxm, a["params"], lam, g)
            l64, gp64 = pc.kl_arbiter(a["params"], lam, g)
            tag = "%s l=%g g=%g" % (name, lam, g)
            check(tag, "loss", loss, l64, pc.GATES["kl_loss"])
            check(tag, "gmu", gp[:, :3], gp64[:, :3], pc.GATES["kl_gmu"])
            check(tag, "gls", gp[:, 3:], gp64[:, 3:], pc.GATES["kl_gls"])


@pytest.mark.parametrize("name", pc.ROW_IDS)
def test_sample_rows_against_the_arbiter(VF, rows, name):
    a = rows[name]
    p = G(a["params"]).requires_grad_()
    z = VF.SampleLogVarFn.apply(p, G(a["eps"]))
    z.backward(G(a["gz"]))
    z64, gp64 = pc.sample_arbiter(a["params"], a["eps"], a["gz"])
    check(name, "z", N(z), z64, pc.GATES["sample_z"])
    check(name, "sample-gls", N(p.grad)[:, 3:], gp64[:, 3:], pc.GATES["sample_gls"])
    assert np.array_equal(N(p.grad)[:, :3], a["gz"])                 # gmu = gz, written (not added into anything)


def test_lattice_row_is_bit_exact(vxm, VF):
    a = pc.lattice_arrays()
    loss, gp = kl_run(vxm, a["params"], a["lam"], 1.0)
    l64, gp64 = pc.kl_arbiter(a["params"], a["lam"], 1.0)
    print("lattice: loss %.9g, arbiter %.17g" % (float(loss), l64))
    assert np.array_equal(loss, np.float32(l64))
    check("lattice", "gmu", gp[:, :3], gp64[:, :3], pc.GATES["kl_gmu"])
    p = G(a["params"]).requires_grad_()
    z = VF.SampleLogVarFn.apply(p, G(a["eps"]))
    z.backward(G(a["gz"]))
    assert np.array_equal(N(z), a["params"][:, :3])                  # eps = 0: the sample IS the mean
    assert not N(p.grad)[:, 3:].any() and np.array_equal(N(p.grad)[:, :3], a["gz"])


@pytest.mark.parametrize("name", ["wide_7x9x70", "ragged_3x40x33", "batch_5x6x40"])
def test_two_runs_give_the_same_bits(vxm, VF, rows, name):
    a = rows[name]
    runs = []
    for _ in range(2):
        loss, gp = kl_run(vxm, a["params"], 25.0, -0.37)
        p = G(a["params"]).requires_grad_()
        z = VF.SampleLogVarFn.apply(p, G(a["eps"]))
        z.backward(G(a["gz"]))
        runs.append((loss, gp, N(z), N(p.grad)))
    for x, y in zip(*runs):
        assert np.array_equal(x, y)


def test_kl_and_the_sampler_through_a_fork_sum_their_gradients(vxm, VF, rows):
    a = rows["batch_5x6x40"]
    lam, g = 10.0, -0.37
    _, g_kl = kl_run(vxm, a["params"], lam, g)
    p = G(a["params"]).requires_grad_()
    VF.SampleLogVarFn.apply(p, G(a["eps"])).backward(G(a["gz"]))
    g_s = N(p.grad)
    p = G(a["params"]).requires_grad_()
    pa, pb = VF.ForkFn.apply(p)
    kl = vxm.losses.KL(lam, a["size"]).loss(None, pa)
    z = VF.SampleLogVarFn.apply(pb, G(a["eps"]))
    torch.autograd.backward([kl, z], [torch.tensor(g, device="cuda"), G(a["gz"])])
    assert np.array_equal(N(p.grad), g_kl + g_s)                     # one fp32 add per element (vxm_add2)
    _, k64 = pc.kl_arbiter(a["params"], lam, g)
    _, s64 = pc.sample_arbiter(a["params"], a["eps"], a["gz"])
    check("fork", "gparams", N(p.grad), k64 + s64, max(pc.GATES["kl_gls"], pc.GATES["sample_gls"]))


@pytest.mark.parametrize("B", [1, 2])
def test_heads_are_the_conv_launch_with_a_strided_destination(VF, B):
    rng = np.random.default_rng(6401 + B)
    shape = (8, 12, 16)
    x = rng.standard_normal((B, 16) + shape).astype(np.float32)
    w = [(0.1 * rng.standard_normal((3, 16, 3, 3, 3))).astype(np.float32) for _ in range(2)]
    b = [rng.standard_normal(3).astype(np.float32) for _ in range(2)]
    gp = rng.standard_normal((B, 6) + shape).astype(np.float32)
    leaves = [G(t).requires_grad_() for t in (x, w[0], b[0], w[1], b[1])]
    params = VF.ProbHeadsFn.apply(*leaves)
    assert tuple(params.shape) == (B, 6) + shape and params.is_contiguous()
    params.backward(G(gp))
    ref = [G(t).requires_grad_() for t in (x, w[0], b[0], w[1], b[1])]
    y_mu, y_ls = VF.ConvFn.apply(ref[0], ref[1], ref[2], 1.0), VF.ConvFn.apply(ref[0], ref[3], ref[4], 1.0)
    assert np.array_equal(N(params[:, :3]), N(y_mu)) and np.array_equal(N(params[:, 3:]), N(y_ls))
    gx = []
    for y, half in ((y_mu, gp[:, :3]), (y_ls, gp[:, 3:])):
        ref[0].grad = None
        y.backward(G(half))
        gx.append(N(ref[0].grad))
    for k in (1, 2, 3, 4):
        assert np.array_equal(N(leaves[k].grad), N(ref[k].grad)), k
    assert np.array_equal(N(leaves[0].grad), gx[0] + gx[1])          # the two backward-data results, one fp32 add (vxm_add2)
    x64 = torch.from_numpy(x).double()
    want = torch.cat([torch.nn.functional.conv3d(x64, torch.from_numpy(w[k]).double(), torch.from_numpy(b[k]).double(), padding=1)
                      for k in range(2)], 1).numpy()
    np.testing.assert_allclose(N(params), want, atol=2e-5, rtol=0)


def _model(vxm, bidir=False):
    m = pc.MODEL
    torch.manual_seed(m["seed"])
    model = vxm.networks.VxmDenseProbabilistic(m["inshape"], nb_unet_features=m["nb_unet_features"], int_steps=m["int_steps"],
                                               int_downsize=m["int_downsize"], bidir=bidir).cuda()
    with torch.no_grad():
        model.flow.weight.normal_(0, m["head_std"])
        model.flow_logsigma.weight.normal_(0, m["head_std"])
        model.flow_logsigma.bias.fill_(m["logsigma_bias"])
    rng = np.random.default_rng(m["seed"])
    src, trg = (rng.random((1, 1) + m["inshape"]).astype(np.float32) for _ in range(2))
    noise = rng.standard_normal((1, 3) + m["inshape"]).astype(np.float32)
    return model, src, trg, noise


@pytest.mark.parametrize("bidir", [False, True])
def test_whole_model_against_the_oracle(vxm, bidir):
    m = pc.MODEL
    model, src, trg, noise = _model(vxm, bidir)
    assert model.training
    sd = {k: v.detach().cpu().double().requires_grad_() for k, v in model.state_dict().items() if not k.endswith(".grid")}
    outs = model(G(src), G(trg), noise=G(noise))
    s64, t64 = torch.from_numpy(src).double(), torch.from_numpy(trg).double()
    outs64 = pc.prob_forward_oracle(s64, t64, sd, torch.from_numpy(noise).double(), m["int_steps"], m["int_downsize"], bidir,
                                    nb_features=m["nb_unet_features"])
    assert len(outs) == len(outs64) == (3 if bidir else 2) and tuple(outs[-1].shape) == (1, 6) + m["inshape"]
    for k, (got, want) in enumerate(zip(outs, outs64)):
        print("model bidir=%s output %d: max |diff| %.3e" % (bidir, k, float(np.abs(N(got) - want.detach().numpy()).max())))
        np.testing.assert_allclose(N(got), want.detach().numpy(), atol=2e-5, rtol=0)
    w_img = (0.5 if bidir else 1.0) / m["image_sigma"] ** 2
    mse, kl = vxm.losses.MSE().loss, vxm.losses.KL(m["prior_lambda"], m["inshape"]).loss
    loss = w_img * mse(G(trg), outs[0]) + m["kl_weight"] * kl(None, outs[-1])
    loss64 = w_img * ((outs64[0] - t64) ** 2).mean() + m["kl_weight"] * pc.kl_torch(outs64[-1], m["prior_lambda"], torch.float64)
    if bidir:
        loss = loss + w_img * mse(G(src), outs[1])
        loss64 = loss64 + w_img * ((outs64[1] - s64) ** 2).mean()
    loss.backward()
    loss64.backward()
    assert abs(float(loss.detach()) - float(loss64.detach())) < 1e-5 * abs(float(loss64.detach()))
    for name, p in model.named_parameters():
        err = pc.rel_l2(N(p.grad), sd[name].grad.numpy())
        print("model bidir=%s %-40s grad rel-L2 %.3e" % (bidir, name, err))
        assert err < 5e-4, name


def test_map_field_sampling_switches_and_the_distribution(vxm):
    model, src, trg, noise = _model(vxm)
    s, t = G(src), G(trg)
    with torch.no_grad():
        y_train, fp = model(s, t, noise=torch.zeros_like(G(noise)))          # training mode, zero noise: z = mu
        y_map, fp2 = model(s, t, sample=False)
        y_noisy, _ = model(s, t, noise=G(noise))
        model.eval()
        y_reg, disp = model(s, t, registration=True)
        y_eval, _ = model(s, t)
        mu, log_sigma = model.flow_distribution(s, t)
        y_drawn, _ = model(s, t, registration=True, sample=True)              # a warp drawn from the posterior at test time
        model.train()
    assert torch.equal(y_train, y_map) and torch.equal(y_reg, y_map) and torch.equal(y_eval, y_map) and torch.equal(fp, fp2)
    assert tuple(disp.shape) == (1, 3) + pc.MODEL["inshape"]
    assert not torch.equal(y_noisy, y_map) and not torch.equal(y_drawn, y_map)
    assert torch.equal(mu, fp[:, :3]) and torch.equal(log_sigma, fp[:, 3:])
    assert tuple(model.noise.shape) == (1, 3) + pc.MODEL["inshape"] and float(model.noise.std()) > 0.9
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(NotImplementedError, match="fp32"):
            model(s, t)


def test_captured_step_equals_the_eager_step_bit_for_bit(vxm):
    """three optimiser steps through GraphedStep (one eager, then capture and two replays), the noise buffer refilled from a seeded CPU
    generator before each: the parameters equal those of three eager steps on the same noise"""
    from voxelmorph_amd.graph import GraphedStep
    from voxelmorph_amd.optim import FlatAdam
    m = pc.MODEL
    steps = 3
    gen = torch.Generator().manual_seed(m["seed"] + 1)
    draws = [torch.randn((1, 3) + m["inshape"], generator=gen) for _ in range(steps)]
    finals = []
    for enabled in (False, True):
        model, src, trg, _ = _model(vxm)
        opt = FlatAdam(model, lr=1e-3)
        s, t = G(src), G(trg)
        model.draw_noise(batch=1)
        mse, kl = vxm.losses.MSE().loss, vxm.losses.KL(m["prior_lambda"], m["inshape"]).loss

        def fwd(model=model, s=s, t=t, mse=mse, kl=kl):
            y, fp = model(s, t, noise=model.noise)
            return vxm.losses.weighted_sum([mse(t, y), kl(None, fp)], [1.0 / m["image_sigma"] ** 2, m["kl_weight"]])
        step = GraphedStep(fwd, opt, eager_steps=1, enabled=enabled)
        losses = []
        for k in range(steps):
            model.noise.copy_(draws[k])
            losses.append(float(step().detach()))
        torch.cuda.synchronize()
        if enabled:
            assert step.capture_error is None and step.replays == steps - 1 and step.graph is not None
        assert opt.step_count == steps
        finals.append((opt.flat_param.clone(), opt.exp_avg.clone(), losses))
    assert torch.equal(finals[0][0], finals[1][0]), float((finals[0][0] - finals[1][0]).abs().max())
    assert torch.equal(finals[0][1], finals[1][1])
    assert max(abs(a - b) for a, b in zip(finals[0][2], finals[1][2])) < 1e-6 and finals[0][2][0] != finals[0][2][-1]
