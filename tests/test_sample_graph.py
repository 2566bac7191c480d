"""Sampler graph mode (`graph=True` / `core.sample_graph` / COLDDIFF_SAMPLE_GRAPH=1, colddiff/graphsample.py): a sampler call that replays
ONE captured reverse step returns what the eager call returns, bit for bit.

Every comparison is torch.equal against the eager call of the same core from the same seeds: xt, direct_recons, the final image, the
NEXT draw of the default CUDA generator and of the CPU generator (a capture pass that consumed a draw fails there), and the network's
`training` flag afterwards.  Shapes: Unet(dim=16, dim_mults=(1, 2)) and the small `Model` of test_graph_train.py, 16 x 16 images,
B = 4, T = 6."""
import contextlib
import io

import pytest
import torch

DEV = "cuda:0"
W = 2                       # graphsample.SAMPLE_GRAPH_WARMUP, asserted below
T, B = 6, 4
NEW = {"cdf_noise_step_dev", "cdf_blend_step_dev", "cdf_steps_advance", "cdf_traj_put"}
pytestmark = pytest.mark.gpu


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _net(kind):
    from colddiff.model2 import Model
    from colddiff.unet import Unet
    if kind == "model":
        return Model(resolution=16, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(8,), dropout=0.1)
    return Unet(dim=16, dim_mults=(1, 2), channels=3)


def make(core, kind="unet", **kw):
    """A core of the named family from fixed seeds, on the device."""
    from colddiff import diffusion as CD
    assert CD.TwoPhase.sample_graph is False                       # the switch is off unless the environment variable asks
    torch.manual_seed(20240607)
    net = _quiet(_net, kind)
    if core == "deblur":
        args = dict(image_size=16, device_of_kernel="cuda", channels=3, timesteps=T, kernel_std=1.0, kernel_size=3, blur_routine="Constant",
                    train_routine="Final")
        args.update(kw)
        if args["blur_routine"] == "Exponential_reflect":
            args["kernel_std"] = 0.1
        d = CD.DeblurDiffusion(net, **args)
    elif core in ("denoise", "demix"):
        d = (CD.DenoiseDiffusion if core == "denoise" else CD.DemixDiffusion)(net, image_size=16, channels=3, timesteps=T, **kw)
    elif core == "defadegen":
        d = CD.DefadeGenDiffusion(net, image_size=16, channels=3, timesteps=T, kernel_std=0.15, initial_mask=2, **kw)
    elif core == "resolution":
        d = CD.ResolutionDiffusion(net, image_size=16, device_of_kernel="cuda", channels=3, timesteps=T, resolution_routine="Incremental", **kw)
    elif core == "defade":
        d = CD.DefadeDiffusion(net, image_size=16, device_of_kernel="cuda", channels=3, timesteps=T, kernel_std=0.3, initial_mask=2, **kw)
    else:
        raise ValueError(core)
    return d.to(DEV)


def image(seed=3, b=B):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((b, 3, 16, 16), generator=g) * 2 - 1).to(DEV)


def call(d, method, graph, img=None, **kw):
    """One sampler call from fixed generator states -> everything the two modes must agree on."""
    img = image() if img is None else img
    torch.manual_seed(77)
    key = "faded_recon_sample" if hasattr(d, "defade_fn") and method in ("sample", "all_sample") else "img"
    out = _quiet(getattr(d, method), batch_size=img.shape[0], graph=graph, **{key: img.clone()}, **kw)
    torch.cuda.synchronize()
    res = {"out%d" % i: o for i, o in enumerate(out)}
    res.update(next_cuda=torch.rand(8, device=DEV).cpu(), next_cpu=torch.rand(8), training=torch.tensor(d._network().training))
    return res


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], (list, tuple)):
            assert len(a[k]) == len(b[k]), (k, len(a[k]), len(b[k]))
            for i, (x, y) in enumerate(zip(a[k], b[k])):
                assert torch.equal(x, y), (k, i)
        elif a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (k, a[k].reshape(-1)[:6], b[k].reshape(-1)[:6])


def graphed(d, captures, replays):
    st = d.sample_graph_state()
    assert st["mode"] == "graph" and st["captures"] == captures and st["replays"] == replays, st


def both(d, method, img=None, **kw):
    e = call(d, method, False, img, **kw)
    g = call(d, method, True, img, **kw)
    same(e, g)
    return e


# ---- equality, family by family ---------------------------------------------------------------------------------------------------
CASES = {
    "deblur-constant-default": ("deblur", dict(sampling_routine="default"), "sample", {}),
    "deblur-constant-alg2": ("deblur", dict(sampling_routine="x0_step_down"), "sample", {}),
    "deblur-expreflect-default": ("deblur", dict(blur_routine="Exponential_reflect", sampling_routine="default"), "gen_sample", dict(noise_level=0.1)),
    "deblur-expreflect-alg2": ("deblur", dict(blur_routine="Exponential_reflect", sampling_routine="x0_step_down"), "gen_sample_2", dict(noise_level=0.1)),
    "deblur-discrete-alg2": ("deblur", dict(sampling_routine="x0_step_down", discrete=True), "gen_sample", dict(noise_level=0.002)),
    "deblur-discrete-default": ("deblur", dict(sampling_routine="default", discrete=True), "sample", {}),
    "denoise-sample": ("denoise", dict(sampling_routine="default"), "sample", {}),
    "denoise-gen-ddim": ("denoise", dict(sampling_routine="ddim"), "gen_sample", {}),
    "denoise-gen-alg2": ("denoise", dict(sampling_routine="x0_step_down"), "gen_sample", {}),
    "demix-sample": ("demix", {}, "sample", {}),
    "demix-gen": ("demix", {}, "gen_sample", dict(noise_level=0.1)),
    "defadegen-sample": ("defadegen", {}, "sample", {}),
    "defadegen-gen": ("defadegen", {}, "gen_sample", dict(noise_level=0.1)),
    "resolution-default-sample": ("resolution", dict(sampling_routine="default"), "sample", {}),
    "resolution-alg2-sample": ("resolution", dict(sampling_routine="x0_step_down"), "sample", {}),
    "resolution-default-gen": ("resolution", dict(sampling_routine="default"), "gen_sample", dict(times=5, noise_level=0.1)),
    "resolution-alg2-gen": ("resolution", dict(sampling_routine="x0_step_down"), "gen_sample", dict(times=5, noise_level=0.1)),
    "defade-default": ("defade", dict(sampling_routine="default"), "sample", {}),
    "defade-alg2": ("defade", dict(sampling_routine="x0_step_down"), "sample", {}),
}


@pytest.mark.parametrize("kind", ["unet", "model"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_graph_call_equals_eager(case, kind):
    from colddiff import graphsample
    assert graphsample.SAMPLE_GRAPH_WARMUP == W
    core, kw, method, ckw = CASES[case]
    d = make(core, kind, **kw)
    assert d.sample_graph_state() == {"mode": "off", "reason": "not requested", "captures": 0, "replays": 0}
    if kind == "model" and core in ("resolution", "defade"):
        # these two samplers do not call eval() (upstream does not): the `Model` in training mode draws its dropout seeds on the host
        # at every step, so the call runs eager and says so; in eval mode it is captured like the others
        both(d, method, **ckw)
        st = d.sample_graph_state()
        assert st["mode"] == "eager" and "dropout" in st["reason"] and st["captures"] == st["replays"] == 0, st
        d.eval()
    e = both(d, method, **ckw)
    assert torch.isfinite(e["out2"]).all() and not torch.equal(e["out2"], e["out0"])
    n = ckw.get("times", T)
    graphed(d, 1, n - W)
    same(e, call(d, method, True, **ckw))                          # ... and again, every step a replay
    graphed(d, 1, 2 * n - W)


# ---- step counts ------------------------------------------------------------------------------------------------------------------
def test_step_counts():
    """t = warm-up and warm-up + 1 never capture; warm-up + 2 captures and replays twice; t below and at num_timesteps; a start > 0."""
    d = make("deblur", sampling_routine="x0_step_down")
    for t in (W, W + 1):
        both(d, "sample", t=t)
        st = d.sample_graph_state()
        assert st["mode"] == "graph" and st["captures"] == st["replays"] == 0, st
    both(d, "sample", t=W + 2)
    graphed(d, 1, 2)
    both(d, "sample", t=T)
    graphed(d, 1, 2 + T)
    both(d, "sample", t=W)                                         # with a valid graph the short call replays too
    graphed(d, 1, 2 + T + W)
    both(d, "sample_from_blur", t=T - 1, start=2)
    graphed(d, 1, 2 + T + W + T - 1)
    d.drop_sample_graph()
    assert d.sample_graph_state()["captures"] == 0
    both(d, "sample_from_blur", t=T, start=2)
    graphed(d, 1, T - W)


def test_counters_and_reuse_with_another_image():
    d = make("denoise", "model", sampling_routine="x0_step_down")
    both(d, "gen_sample")
    graphed(d, 1, T - W)
    other = image(11)
    e = call(d, "gen_sample", False, other)
    g = call(d, "gen_sample", True, other)
    same(e, g)
    graphed(d, 1, 2 * T - W)
    assert not torch.equal(e["out2"], call(d, "gen_sample", False)["out2"])


# ---- what drops the graph ---------------------------------------------------------------------------------------------------------
def test_recapture_after_a_train_step_and_ema_update(tmp_path):
    from test_graph_train import build
    tr = build("unet3", False, tmp_path / "t", sample_graph=True)
    d = tr.ema_core
    assert d.sample_graph is True and tr.core.sample_graph is False
    e = call(d, "sample", False)
    same(e, call(d, "sample", None))                               # None reads the core's switch
    graphed(d, 1, tr.core.num_timesteps - W)
    _quiet(tr.train_step)
    tr.step = 5
    tr.step_ema()                                                  # past step_start_ema: the EMA kernel rewrites the arena behind torch
    e2 = call(d, "sample", False)
    assert not torch.equal(e2["out2"], e["out2"])
    same(e2, call(d, "sample", None))
    graphed(d, 2, 2 * (tr.core.num_timesteps - W))


def test_recapture_after_load_state_dict_batch_size_and_precision():
    from colddiff import runtime as rt
    d = make("resolution", "model", sampling_routine="x0_step_down").eval()
    e = both(d, "sample")
    graphed(d, 1, T - W)
    torch.manual_seed(5)
    sd = {k: (v + 0.01 * torch.randn_like(v) if v.is_floating_point() else v) for k, v in d.state_dict().items()}
    d.load_state_dict(sd)
    e2 = both(d, "sample")
    assert not torch.equal(e2["out2"], e["out2"])
    graphed(d, 2, 2 * (T - W))
    both(d, "sample", image(4, b=3))                               # another batch size
    graphed(d, 3, 3 * (T - W))
    d2 = make("deblur", "unet", sampling_routine="default")
    e = both(d2, "sample")
    graphed(d2, 1, T - W)
    with rt.precision_scope("bf16"):
        e3 = both(d2, "sample")
    assert not torch.equal(e3["out2"], e["out2"])
    graphed(d2, 2, 2 * (T - W))


# ---- all_sample -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("core,kw", [("deblur", dict(sampling_routine="x0_step_down")), ("deblur", dict(sampling_routine="default", discrete=True)),
                                     ("resolution", dict(sampling_routine="default")), ("defade", dict(sampling_routine="x0_step_down"))])
def test_all_sample_lists_equal_eager(core, kw):
    d = make(core, **kw)
    e = both(d, "all_sample")
    assert len(e["out1"]) == T and len(e["out0"]) == T + (core == "deblur")
    graphed(d, 1, T - W)
    both(d, "all_sample", times=T - 1)                             # fewer steps than t: rows times-1 .. 0 of the same slabs, all replays
    graphed(d, 1, 2 * T - W - 1)
    both(d, "all_sample", image(9))
    graphed(d, 1, 3 * T - W - 1)


# ---- cores and methods that stay eager --------------------------------------------------------------------------------------------
def _color_core(which):
    from colddiff.decolor import DecolorDiffusion, UnetConvNextBlock
    from colddiff.snow import SnowDiffusion
    torch.manual_seed(20240607)
    net = _quiet(UnetConvNextBlock, dim=16, dim_mults=(1, 2), channels=3)
    kw = dict(image_size=(16, 16), device_of_kernel="cuda", channels=3, timesteps=T, sampling_routine="x0_step_down", batch_size=B)
    if which == "snow":
        return SnowDiffusion(net, forward_process_type="Snow", snow_level=1, **kw).to(DEV)
    return DecolorDiffusion(net, forward_process_type="Decolorization", **kw).to(DEV)


@pytest.mark.parametrize("which", ["individual", "decolor", "snow"])
def test_ineligible_cores_run_eager_with_a_reason(which):
    import numpy as np
    from colddiff import runtime as rt
    from test_gpu_invariance import Recorder
    d = make("deblur", blur_routine="Individual_Incremental", sampling_routine="x0_step_down") if which == "individual" else _color_core(which)

    def run(graph):
        np.random.seed(3)
        img = image()
        torch.manual_seed(77)
        out = _quiet(d.sample, batch_size=B, img=img, graph=graph)
        torch.cuda.synchronize()
        return {"out": list(out.values()) if isinstance(out, dict) else list(out), "next_cuda": torch.rand(8, device=DEV).cpu(), "next_cpu": torch.rand(8)}
    e = run(False)
    with Recorder(rt.lib()) as rec:
        g = run(True)
    same(e, g)
    st = d.sample_graph_state()
    assert st["mode"] == "eager" and st["reason"] and st["captures"] == st["replays"] == 0, st
    assert not rec.names() & NEW, sorted(rec.names() & NEW)


def test_methods_that_are_not_captured_say_why():
    d = make("denoise", sampling_routine="x0_step_down")
    e = _quiet(d.all_sample, batch_size=B, img=image(), graph=False)
    g = _quiet(d.all_sample, batch_size=B, img=image(), graph=True)
    assert all(torch.equal(a, b) for x, y in zip(e, g) for a, b in zip(x, y))
    st = d.sample_graph_state()
    assert st["mode"] == "eager" and "host" in st["reason"] and st["replays"] == 0, st
    d = make("deblur", sampling_routine="x0_step_down")
    e = _quiet(d.forward_and_backward, batch_size=B, img=image(), graph=False)
    g = _quiet(d.forward_and_backward, batch_size=B, img=image(), graph=True)
    assert torch.equal(e[2], g[2]) and all(torch.equal(a, b) for a, b in zip(e[1], g[1]))
    st = d.sample_graph_state()
    assert st["mode"] == "eager" and "forward_and_backward" in st["reason"], st
    both(d, "sample")                                              # a covered method of the same core is captured all the same
    graphed(d, 1, T - W)


# ---- the default path stays the default path --------------------------------------------------------------------------------------
def test_new_entry_points_only_in_graph_mode():
    from colddiff import runtime as rt
    from test_gpu_invariance import Recorder
    d = make("denoise", sampling_routine="x0_step_down")
    with Recorder(rt.lib()) as rec:
        _quiet(d.gen_sample, batch_size=B, img=image())
    assert "cdf_noise_step" in rec.names() and not rec.names() & NEW, sorted(rec.names() & NEW)
    assert d.sample_graph_state()["mode"] == "off"
    with Recorder(rt.lib()) as rec:
        _quiet(d.gen_sample, batch_size=B, img=image(), graph=True)
    torch.cuda.synchronize()
    assert rec.names() & NEW == {"cdf_noise_step_dev", "cdf_steps_advance", "cdf_traj_put"} and "cdf_noise_step" not in rec.names()
    assert sum(n == "cdf_steps_advance" for n, _ in rec.calls) == W + 1          # the warm-up steps and the capture pass; replays call nothing
    graphed(d, 1, T - W)


# ---- a capture pass that raises ---------------------------------------------------------------------------------------------------
def test_capture_that_raises_finishes_the_call_eagerly(monkeypatch):
    from colddiff.graphstep import GraphStep
    calls = []

    def boom(self, table, generators=()):
        calls.append(1)
        torch.rand(3)
        torch.rand(3, device=DEV)
        raise RuntimeError("boom at capture")
    d = make("defadegen", "model")
    e = call(d, "gen_sample", False, noise_level=0.1)
    monkeypatch.setattr(GraphStep, "capture", boom)
    g = call(d, "gen_sample", True, noise_level=0.1)
    same(e, g)                                                     # the generators' next draws are among the compared values
    st = d.sample_graph_state()
    assert calls == [1] and st["mode"] == "eager" and "boom at capture" in st["reason"] and st["captures"] == 1 and st["replays"] == 0, st
    same(e, call(d, "gen_sample", True, noise_level=0.1))
    assert calls == [1], "a capture was tried twice"


# ---- the sweeps -------------------------------------------------------------------------------------------------------------------
def test_graph_sampler_on_poisoned_memory_twice():
    from poison import poisoned_allocations
    d = make("deblur", "model", sampling_routine="x0_step_down")
    e = call(d, "sample", False)
    with poisoned_allocations():
        a = call(d, "sample", True)
        b = call(d, "sample", True)
    same(a, b)
    same(e, a)
    graphed(d, 1, 2 * T - W)


def test_fid_sweep_with_sample_graph_returns_the_same_dict(tmp_path):
    from deblurring_diffusion_pytorch import GaussianDiffusion, Trainer, Unet
    from test_data import _write_images
    folder = str(tmp_path / "imgs")
    _write_images(folder, 8)
    res = {}
    for name, sg in (("e", None), ("g", True)):
        torch.manual_seed(0)
        net = _quiet(Unet, dim=16, dim_mults=(1, 2), channels=3).to(DEV)
        d = GaussianDiffusion(net, image_size=16, device_of_kernel=DEV, channels=3, timesteps=T, kernel_size=3, kernel_std=0.5,
                              sampling_routine="x0_step_down").to(DEV)
        tr = _quiet(Trainer, d, folder, image_size=16, train_batch_size=4, train_num_steps=1, dataset="train", results_folder=str(tmp_path / name),
                    num_workers=0, device_data=True, sample_graph=sg)
        res[name] = _quiet(tr.fid_distance_decrease_from_manifold, fid_func=None, start=-1, end=7, batch=4)
        if sg:
            st = tr.ema_core.sample_graph_state()
            assert st["mode"] == "graph" and st["captures"] == 1 and st["replays"] == 2 * T - W, st
    assert res["e"] == res["g"] and len(res["e"]) >= 6, res
