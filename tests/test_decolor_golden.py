"""The decolorization package against vectors the UNMODIFIED reference produced (tests/golden/decolor/*.pt, written by
tests/golden/decolor/make_golden_decolor.py under the stubs of tests/decolor_ref.py):

 (a) where the reference tree exists, the generator reproduces every committed tensor -- `torch.equal` for everything without a network
     in it, 1e-6 for network outputs, thread count pinned to the one the fixtures were written with;
 (b) a CPU restatement built from oracle.cold_oracle's functional UNet and the sequential colour chain matches the fixtures;
 (c) the engine (simulator and MI355X) matches them: chains <= 1e-5, network outputs <= 1e-4 max-abs, gradients by
     tol * max(|g|max, 1e-2 * global max) with tol 1e-3, sampler finals <= 1e-4.
`to_lab=True` cases went through the RESTATED kornia functions when they were generated (labelled `restated_kornia` in the fixture) and are
held to the measured Lab tolerance of tests/test_color_kernels.py, relative to the channel scale; the Lab sampler's three images (back in
RGB) are held to 4 x their own measured errors.
Gradients: the fixtures store the two ends of the backward pass; the WHOLE gradient of every combination is checked through the CPU
restatement -- live reference against restatement where the reference tree exists, engine against restatement everywhere.
"""
import contextlib
import io
import os
import sys

import pytest
import torch

import decolor_ref as R
from oracle import cold_oracle as O
from test_color_kernels import LAB_CHAIN_TOL, LAB_SCALE, LAB_SINGLE_TOL

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decolor")
CHAIN_TOL, NET_TOL, GRAD_TOL, SAMPLER_TOL = 1e-5, 1e-4, 1e-3, 1e-4
T, SIZE = 6, 16


def load(name):
    return torch.load(os.path.join(GOLD, name), weights_only=False)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _generator():
    sys.path.insert(0, GOLD)
    try:
        import make_golden_decolor
    finally:
        sys.path.remove(GOLD)
    return make_golden_decolor


class MBE:
    def __init__(self, kind):
        self.kind = kind
        self.device = torch.device("cuda:0" if kind == "hip" else "cpu")

    def to(self, t):
        return t.to(self.device)


@pytest.fixture(params=[pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)])
def mbe(request):
    from colddiff import runtime
    if request.param == "emu":
        from emu_util import install_emu
        install_emu()
    else:
        runtime._lib_override = None
    yield MBE(request.param)
    runtime._lib_override = None


def err(a, b):
    return (a.detach().cpu() - b).abs().max().item()


def lab_err(a, b):
    return ((a.detach().cpu() - b).abs() / LAB_SCALE).max().item()


# ---------------------------------------------------------------------------------------------------------------------------------------
# (a) the fixtures are what the reference produces
# ---------------------------------------------------------------------------------------------------------------------------------------
def _compare(path, got, want, exact):
    if isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), path
        for k in want:
            _compare(path + "/" + str(k), got[k], want[k], exact)
    elif isinstance(want, (list, tuple)) and want and isinstance(want[0], torch.Tensor):
        assert len(got) == len(want), path
        for i, (a, b) in enumerate(zip(got, want)):
            _compare(f"{path}[{i}]", a, b, exact)
    elif isinstance(want, torch.Tensor):
        if exact:
            assert torch.equal(got, want), path
        else:
            assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item()), path
    else:
        assert got == want, path


@pytest.mark.skipif(not R.available(), reason="needs the reference tree")
def test_generator_reproduces_every_committed_fixture():
    M = _generator()
    fresh = quiet(M.generate)
    net, cases = load("decolor_net.pt"), load("decolor_cases.pt")
    _compare("net/state_dict", fresh["decolor_net.pt"]["state_dict"], net["state_dict"], True)
    _compare("net/loss", fresh["decolor_net.pt"]["loss"], net["loss"], False)
    _compare("chains", fresh["decolor_cases.pt"]["chains"], cases["chains"], True)              # no network in it: bit for bit
    for part in ("losses", "samplers", "variants", "lab"):
        _compare(part, fresh["decolor_cases.pt"][part], cases[part], False)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (b) CPU restatement: oracle UNet + sequential chain
# ---------------------------------------------------------------------------------------------------------------------------------------
def _oracle_loss(sd, x, t, routine, loss_type, table, mean_scale=False):
    def net(inp, tt):
        y = O.unet_forward(sd, inp, tt)
        if mean_scale:
            y = y - inp.mean([1, 2, 3], keepdim=True) + y.mean([1, 2, 3], keepdim=True)
        return y

    def q(tt):
        n, _ = R.q_sample_counts(tt)
        return R.chain_t(x, table, n)
    x_blur = q(t)
    if routine == "Final":
        pred, true = x, net(x_blur, t)
    elif routine == "Step":
        pred, true = q(t - 1), net(x_blur, t)
    else:
        pred, true = q(t - 1) - x_blur, net(x_blur, t)
    d = (pred - true)
    if loss_type == "l2":
        return (d * d).mean()
    return d.abs().mean() if loss_type == "l1" else d.abs().mean().sqrt()


def restatement_gradients(state_dict, x, t, routine, loss_type, mean_scale=False):
    """(loss, {parameter: gradient}) of the CPU restatement for EVERY parameter."""
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in state_dict.items()}
    loss = _oracle_loss(sd, x, t, routine, loss_type, R.table_of("Constant", T), mean_scale)
    loss.backward()
    return loss.item(), {k: v.grad for k, v in sd.items() if v.grad is not None}


def all_gradients_close(got, want, what):
    """Every tensor of `want` against `got` by tol * max(|g|max, 1e-2 * global max), tol 1e-3."""
    gmax = max(g.abs().max().item() for g in want.values())
    assert len(want) > 100, len(want)                               # (the whole network: 122 parameter tensors)
    for name, g in want.items():
        e = err(got[name], g)
        assert e <= GRAD_TOL * max(g.abs().max().item(), 1e-2 * gmax), (what, name, e)


@pytest.mark.skipif(not R.available(), reason="needs the reference tree")
def test_every_reference_gradient_matches_the_cpu_restatement():
    """The fixtures hold the gradients at the two ends of the backward pass only (a full set is 335 KB); here the live reference's WHOLE
    gradient of each of the nine combinations is compared, in memory, with the restatement the engine is then held to in full."""
    M = _generator()
    g = load("decolor_net.pt")
    threads = torch.get_num_threads()
    torch.set_num_threads(M.THREADS)
    try:
        live = quiet(M.loss_cases, g["state_dict"], full=True)
    finally:
        torch.set_num_threads(threads)
    assert sorted(live) == sorted(f"{r}_{l}" for r in M.ROUTINES for l in M.LOSSES)
    for key, c in live.items():
        routine, lt = key.rsplit("_", 1)
        loss, grads = restatement_gradients(g["state_dict"], g["x"], g["t"], routine, lt)
        assert abs(loss - c["loss"].item()) <= 1e-5, key
        assert sorted(grads) == sorted(c["grads"]), key
        all_gradients_close(grads, c["grads"], key)


def test_cpu_restatement_matches_the_fixtures():
    net, cases = load("decolor_net.pt"), load("decolor_cases.pt")
    x = cases["chains"]["x"]
    for key, c in cases["chains"].items():
        if not key.startswith("T"):
            continue
        Tn, routine, remove = key.split("_")
        table = R.table_of(routine, int(Tn[1:]), total_remove=bool(int(remove)))
        assert torch.equal(table, c["table"]), key                                             # the weights are bit-equal
        n, nmax = R.q_sample_counts(c["t"])
        assert err(R.chain_t(x, table, n), c["q"]) <= CHAIN_TOL and err(R.chain_t(x, table, nmax), c["total"]) <= CHAIN_TOL, key
        n, nmax = R.q_sample_counts(c["t_neg"])
        assert err(R.chain_t(x, table, n), c["q_neg"]) <= CHAIN_TOL, key
        assert err(R.chain_t(x, table, [nmax if v >= 0 else -1 for v in n]), c["total_neg"]) <= CHAIN_TOL, key
    assert torch.equal(cases["chains"]["all_minus_one"], x)
    assert err(R.mix_t(x, torch.ones(3, 3) / 3.0), cases["chains"]["total_forward"]) <= CHAIN_TOL
    table = R.table_of("Constant", T)
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in net["state_dict"].items()}
    for key, c in cases["losses"].items():
        routine, lt = key.rsplit("_", 1)
        for v in sd.values():
            v.grad = None
        loss = _oracle_loss(sd, net["x"], net["t"], routine, lt, table)
        loss.backward()
        assert abs(loss.item() - c["loss"].item()) <= 1e-5, key
        gmax = max(g.abs().max().item() for g in c["grads"].values())
        for name, g in c["grads"].items():
            assert err(sd[name].grad, g) <= GRAD_TOL * max(g.abs().max().item(), 1e-2 * gmax), (key, name)
    v = cases["variants"]
    with torch.no_grad():
        plain = {k: t_.detach() for k, t_ in sd.items()}
        y = O.unet_forward(plain, v["x"], v["t"])
        y = y - v["x"].mean([1, 2, 3], keepdim=True) + y.mean([1, 2, 3], keepdim=True)
        assert err(y, v["mean_scale"]["out"]) <= NET_TOL
        no_time = {k: t_ for k, t_ in plain.items() if k in v["no_time"]["keys"]}
        assert err(O.unet_forward(no_time, v["x"], None), v["no_time"]["out"]) <= NET_TOL
        assert torch.equal(v["no_time"]["out"], v["no_time"]["out_with_t"])                    # a network without time MLP ignores t
    lab = cases["lab"]
    assert lab["restated_kornia"] is True
    assert lab_err(R.rgb2lab_t(lab["x"]), lab["x_lab"]) <= LAB_SINGLE_TOL and err(R.lab2rgb_t(lab["x_lab"]), lab["rgb_back"]) <= LAB_SINGLE_TOL


# ---------------------------------------------------------------------------------------------------------------------------------------
# (c) the engine
# ---------------------------------------------------------------------------------------------------------------------------------------
def _engine(mbe, sd, T_=T, net_kw=None, **kw):
    D = R.mine()
    net = quiet(D.UnetConvNextBlock, dim=8, dim_mults=(1, 2), **(net_kw or {}))
    if sd is not None:
        net.load_state_dict({k: v for k, v in sd.items() if k in net.state_dict()}, strict=True)
    net = net.to(mbe.device)
    gd = D.GaussianDiffusion(net, image_size=(SIZE, SIZE), device_of_kernel='cuda', channels=3, timesteps=T_, **kw).to(mbe.device)
    return net, gd


def test_engine_state_dict_layout():
    net = load("decolor_net.pt")
    D = R.mine()
    mine = quiet(D.UnetConvNextBlock, dim=8, dim_mults=(1, 2))
    assert list(mine.state_dict().keys()) == list(net["state_dict"].keys())
    assert all(mine.state_dict()[k].shape == v.shape for k, v in net["state_dict"].items())
    v = load("decolor_cases.pt")["variants"]["no_time"]
    assert sorted(quiet(D.UnetConvNextBlock, dim=8, dim_mults=(1, 2), with_time_emb=False).state_dict().keys()) == v["keys"]


def test_engine_chains(mbe):
    cases = load("decolor_cases.pt")["chains"]
    x = mbe.to(cases["x"])
    D = R.mine()
    for key, c in cases.items():
        if not key.startswith("T"):
            continue
        Tn, routine, remove = key.split("_")
        gd = D.GaussianDiffusion(None, image_size=(5, 5), device_of_kernel='cuda', timesteps=int(Tn[1:]), decolor_routine=routine,
                                 decolor_total_remove=bool(int(remove)))
        assert torch.equal(gd.forward_process.table.cpu(), c["table"]), key
        assert all(torch.equal(k_[:, :, 0, 0], c["table"][i]) for i, k_ in enumerate(gd.forward_process.kernels))
        q, tot = gd.q_sample(x, mbe.to(c["t"]), return_total_blur=True)
        assert err(q, c["q"]) <= CHAIN_TOL and err(tot, c["total"]) <= CHAIN_TOL, key
        assert err(gd.q_sample(x, mbe.to(c["t"])), c["q"]) <= CHAIN_TOL, key
        q, tot = gd.q_sample(x, mbe.to(c["t_neg"]), return_total_blur=True)
        assert err(q, c["q_neg"]) <= CHAIN_TOL and err(tot, c["total_neg"]) <= CHAIN_TOL, key
    gd = D.GaussianDiffusion(None, image_size=(5, 5), device_of_kernel='cuda', timesteps=T)
    assert torch.equal(gd.q_sample(x, mbe.to(torch.full((4,), -1))).cpu(), cases["x"])
    assert err(gd.forward_process.total_forward(x), cases["total_forward"]) <= CHAIN_TOL
    assert err(gd.forward_process.forward(x, 2), R.mix_t(cases["x"], gd.forward_process.table.cpu()[2])) <= CHAIN_TOL


@pytest.mark.parametrize("routine", ["Final", "Step", "Step_Gradient"])
@pytest.mark.parametrize("loss_type", ["l1", "l2", "sqrt"])
def test_engine_losses_and_gradients(mbe, routine, loss_type):
    g, c = load("decolor_net.pt"), load("decolor_cases.pt")["losses"][f"{routine}_{loss_type}"]
    net, gd = _engine(mbe, g["state_dict"], train_routine=routine, loss_type=loss_type)
    loss = gd.p_losses(mbe.to(g["x"]), mbe.to(g["t"]))
    loss.backward()
    e = abs(loss.item() - c["loss"].item())
    print(f"{routine} {loss_type} [{mbe.kind}]: loss {loss.item():.6f} (reference {c['loss'].item():.6f})")
    assert e <= 1e-5 * max(1.0, abs(c["loss"].item()))
    grads = dict(net.named_parameters())
    gmax = max(v.abs().max().item() for v in c["grads"].values())
    for name, r in c["grads"].items():
        assert err(grads[name].grad, r) <= GRAD_TOL * max(r.abs().max().item(), 1e-2 * gmax), (name, err(grads[name].grad, r))
    if routine == "Final" and loss_type == "l1":
        assert abs(c["loss"].item() - g["loss"].item()) <= 1e-6
    # ... and EVERY parameter gradient against the CPU restatement (pinned to the reference: at the subset by the fixture, in full by
    # test_every_reference_gradient_matches_the_cpu_restatement where the reference tree exists)
    _, want = restatement_gradients(g["state_dict"], g["x"], g["t"], routine, loss_type)
    all_gradients_close({k: p.grad for k, p in grads.items()}, want, f"{routine}_{loss_type}")


def test_engine_samplers(mbe):
    g, c = load("decolor_net.pt"), load("decolor_cases.pt")["samplers"]
    sd = g["state_dict"]
    x4 = mbe.to(c["x"])
    x = x4[:2].clone()
    with torch.no_grad():
        for train, samp in (("Final", "default"), ("Final", "x0_step_down"), ("Step", "default"), ("Step_Gradient", "default")):
            net, gd = _engine(mbe, sd, train_routine=train, sampling_routine=samp)
            out = quiet(gd.sample, batch_size=2, img=x.clone())
            want = c[f"sample_{train}_{samp}"]
            assert sorted(out) == sorted(want) == ["direct_recons", "recon", "xt"]
            assert err(out["xt"], want["xt"]) <= CHAIN_TOL
            assert err(out["direct_recons"], want["direct_recons"]) <= NET_TOL
            e = err(out["recon"], want["recon"])
            print(f"sample {train} {samp} [{mbe.kind}]: final {e:.3g}")
            assert e <= SAMPLER_TOL, (train, samp, e)
        net, gd = _engine(mbe, sd, sampling_routine="x0_step_down")
        X0, Xt, init_pred, fwd = gd.all_sample(batch_size=2, img=x.clone(), times=2)
        assert init_pred is None and fwd == [] and len(X0) == len(Xt) == 2 and all(not v.is_cuda for v in X0 + Xt)
        for a, b in zip(X0 + Xt, c["all_sample"]["X_0s"] + c["all_sample"]["X_ts"]):
            assert err(a, b) <= SAMPLER_TOL
        F, B, last = gd.forward_and_backward(batch_size=2, img=x.clone())
        w = c["forward_and_backward"]
        assert (len(F), len(B)) == tuple(w["lengths"])
        assert err(F[-1], w["Forward_last"]) <= CHAIN_TOL and err(F[3], w["Forward_3"]) <= CHAIN_TOL
        assert err(B[-1], w["Backward_last"]) <= SAMPLER_TOL and err(last, w["img"]) <= SAMPLER_TOL
        w = c["sample_multi_step"]
        assert err(gd.sample_multi_step(x4.clone(), mbe.to(w["t_start"]), mbe.to(w["t_end"])), w["out"]) <= SAMPLER_TOL
        for samp in ("default", "x0_step_down"):
            net, gd = _engine(mbe, sd, sampling_routine=samp)
            w = c[f"one_step_{samp}"]
            a, b = gd.sample_one_step(x4.clone(), mbe.to(w["t"]))
            assert err(b, w["direct_recons"]) <= NET_TOL and err(a, w["x"]) <= SAMPLER_TOL, samp


def test_engine_network_variants(mbe):
    g, v = load("decolor_net.pt"), load("decolor_cases.pt")["variants"]
    x, t = mbe.to(v["x"]), mbe.to(v["t"])
    net, gd = _engine(mbe, g["state_dict"], net_kw=dict(output_mean_scale=True))
    assert err(net(x, t), v["mean_scale"]["out"]) <= NET_TOL
    loss = gd.p_losses(x, t)
    loss.backward()
    assert abs(loss.item() - v["mean_scale"]["loss"].item()) <= 1e-5
    grads = dict(net.named_parameters())
    gmax = max(r.abs().max().item() for r in v["mean_scale"]["grads"].values())
    for name, r in v["mean_scale"]["grads"].items():
        assert err(grads[name].grad, r) <= GRAD_TOL * max(r.abs().max().item(), 1e-2 * gmax), name
    _, want = restatement_gradients(g["state_dict"], v["x"], v["t"], "Final", "l1", mean_scale=True)
    all_gradients_close({k: p.grad for k, p in grads.items()}, want, "mean_scale")
    net, _ = _engine(mbe, g["state_dict"], net_kw=dict(with_time_emb=False))
    with torch.no_grad():
        assert err(net(x), v["no_time"]["out"]) <= NET_TOL and err(net(x, t), v["no_time"]["out_with_t"]) <= NET_TOL


def test_engine_lab_cases(mbe):
    """to_lab=True: generated through the restated kornia functions (unpinned boundary), held to the measured Lab tolerance."""
    g, lab = load("decolor_net.pt"), load("decolor_cases.pt")["lab"]
    D = R.mine()
    xl = D.diffusion.rgb2lab(mbe.to(lab["x"]))
    assert lab_err(xl, lab["x_lab"]) <= LAB_SINGLE_TOL
    assert err(D.diffusion.lab2rgb(mbe.to(lab["x_lab"])), lab["rgb_back"]) <= LAB_SINGLE_TOL
    for Tn in (6, 50):
        net, gd = _engine(mbe, g["state_dict"], T_=Tn, to_lab=True, sampling_routine="x0_step_down")
        c = lab[f"T{Tn}"]
        q, tot = gd.q_sample(mbe.to(lab["x_lab"]), mbe.to(c["t"]), return_total_blur=True)
        e = max(lab_err(q, c["q"]), lab_err(tot, c["total"]))
        print(f"lab q_sample T={Tn} [{mbe.kind}]: {e:.3g} of the channel scale")
        assert e <= LAB_CHAIN_TOL
    net, gd = _engine(mbe, g["state_dict"], to_lab=True, sampling_routine="x0_step_down")
    with torch.no_grad():
        out = quiet(gd.sample, batch_size=2, img=mbe.to(lab["x_lab"]).clone())
    want = lab["sample"]
    # Measured, like every Lab bound (tests/test_color_kernels.py): max-abs error in RGB units against the fixture, simulator / MI355X:
    #     xt (one Lab chain + lab2rgb, no network)   1.91e-6 / 2.15e-6
    #     direct_recons (one network call + lab2rgb) 1.79e-7 / 1.19e-7
    #     recon (T reverse steps + lab2rgb)          1.85e-6 / 2.15e-6
    # asserted at 4 x the larger of the two.
    xt_tol, dr_tol, final_tol = 4 * 2.15e-6, 4 * 1.79e-7, 4 * 2.15e-6
    e_xt, e_dr, e = err(out["xt"], want["xt"]), err(out["direct_recons"], want["direct_recons"]), err(out["recon"], want["recon"])
    print(f"lab sample [{mbe.kind}]: xt {e_xt:.3g} (bound {xt_tol:.3g}), direct_recons {e_dr:.3g} (bound {dr_tol:.3g}), final {e:.3g} (bound {final_tol:.3g})")
    assert e_xt <= xt_tol
    assert e_dr <= dr_tol
    assert e <= final_tol
