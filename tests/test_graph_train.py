"""Trainer graph mode (Trainer(graph=True) / COLDDIFF_GRAPH=1): the optimizer step replayed as one captured graph is the SAME training
run as the eager Trainer's, bit for bit.

Every comparison is torch.equal.  For each case the eager run and the graph run are two Trainers built from the same seeds in this
process; after N steps every per-step loss, the parameter arena, Adam's two moment arenas, the EMA arena, the step counters and the
NEXT draw of the default CUDA generator, of the loader's generator and of the CPU generator must be equal -- which fails if a
capture pass consumed a draw, a dropout seed or Adam's bias corrections were baked into the graph, or an index slice was replayed.
The eager side runs with COLDDIFF_PREFETCH=0: the prefetching loop is bit-identical between milestones but has drawn the next
step's batches already when the comparison looks at the generators."""
import contextlib
import io
import os

import pytest
import torch

DEV = "cuda:0"
W = 3                       # Trainer.GRAPH_WARMUP, asserted below


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _net(kind):
    from deblurring_diffusion_pytorch import Model, Unet
    if kind == "model":
        return Model(resolution=16, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(8,), dropout=0.1), 3
    if kind == "unet3":
        return Unet(dim=16, dim_mults=(1, 2), channels=3), 3
    return Unet(dim=16, dim_mults=(1, 2), channels=1), 1


def build(kind, graph, folder, *, core="deblur", data=None, dataset="synthetic", batch=4, acc=2, core_kw=None, **kw):
    """A Trainer from fixed seeds (weights, CPU generator, default CUDA generator)."""
    from deblurring_diffusion_pytorch import GaussianDiffusion, Trainer
    torch.manual_seed(20240607)
    net, ch = _net(kind)
    net = net.to(DEV)
    if core == "denoise":
        import denoising_diffusion_pytorch as dn
        diff = dn.GaussianDiffusion(net, image_size=16, channels=ch, timesteps=5, sampling_routine="x0_step_down").to(DEV)
        Trainer = dn.Trainer
    else:
        ck = dict(kernel_size=3, blur_routine="Constant", train_routine="Final")
        ck.update(core_kw or {})
        diff = GaussianDiffusion(net, image_size=16, device_of_kernel="cuda", channels=ch, timesteps=5, loss_type="l1", kernel_std=1.0,
                                 sampling_routine="x0_step_down", **ck).to(DEV)
    args = dict(image_size=16, train_batch_size=batch, train_lr=2e-5, train_num_steps=10 ** 6, gradient_accumulate_every=acc, dataset=dataset,
                update_ema_every=2, step_start_ema=3, results_folder=str(folder), graph=graph)
    args.update(kw)
    tr = _quiet(Trainer, diff, data, **args)
    tr.quiet = True
    torch.manual_seed(77)                  # the run's draws start from one state on both sides
    return tr


def run(tr, N, bf16=(), halve_lr_before=None, before=None):
    """N optimizer steps as train() counts them (1-based step numbers in the arguments); -> everything the two sides must agree on."""
    from colddiff import runtime as rt
    losses = []
    for s in range(1, N + 1):
        if s == halve_lr_before:
            tr.opt.param_groups[0]["lr"] *= 0.5
        if before is not None:
            before(tr, s)
        with rt.precision_scope("bf16") if s in bf16 else contextlib.nullcontext():
            losses.append(_quiet(tr.train_step))
        tr.step += 1
    torch.cuda.synchronize()
    out = {"loss": torch.stack(losses).cpu(), "arena": tr.arena.data.cpu(), "exp_avg": tr.opt.exp_avg.cpu(), "exp_avg_sq": tr.opt.exp_avg_sq.cpu(),
           "ema": tr.ema_arena.data.cpu(), "counts": torch.tensor([tr.opt.step_count, tr.step]),
           "next_cuda": torch.rand(8, device=DEV).cpu(), "next_loader": torch.rand(8, generator=tr.dl.gen, device=DEV).cpu(), "next_cpu": torch.rand(8)}
    assert len({float(l) for l in out["loss"]}) == N and torch.isfinite(out["loss"]).all()         # a replayed step would repeat its loss
    return out


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (k, a[k].reshape(-1)[:8], b[k].reshape(-1)[:8])


def both(monkeypatch, tmp_path, N, kind, run_kw=None, **kw):
    from colddiff.trainer import Trainer
    assert Trainer.GRAPH_WARMUP == W
    monkeypatch.setenv("COLDDIFF_PREFETCH", "0")
    e = run(build(kind, False, tmp_path / "e", **kw), N, **(run_kw or {}))
    monkeypatch.delenv("COLDDIFF_PREFETCH")
    tg = build(kind, True, tmp_path / "g", **kw)
    g = run(tg, N, **(run_kw or {}))
    same(e, g)
    return tg


def graphed(tr, N, captures=1, replays=None):
    st = tr.graph_state()
    assert st["mode"] == "graph", st
    assert st["captures"] == captures and st["replays"] == (N - W if replays is None else replays), st


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_unet_steps_equal_eager(monkeypatch, tmp_path):
    """Fused accumulation (2 x 4 images), both branches of step_ema, N = 8."""
    graphed(both(monkeypatch, tmp_path, 8, "unet"), 8)


@pytest.mark.gpu
def test_model_with_dropout_steps_equal_eager(monkeypatch, tmp_path):
    """`Model` in training mode: every ResnetBlock draws a dropout seed per step -- from the device seed table in graph mode."""
    tr = both(monkeypatch, tmp_path, 6, "model")
    graphed(tr, 6)
    assert tr._gs["table"].n_seeds >= 2


@pytest.mark.gpu
def test_denoise_core_steps_equal_eager(monkeypatch, tmp_path):
    """The denoising core (fresh Gaussian noise per micro-batch) declares graph_safe() too."""
    graphed(both(monkeypatch, tmp_path, 6, "unet3", core="denoise"), 6)


@pytest.fixture(scope="module")
def png_folder(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("imgs")
    g = torch.Generator().manual_seed(5)
    for i in range(10):
        arr = torch.randint(0, 256, (20, 20, 3), generator=g, dtype=torch.uint8).numpy()
        Image.fromarray(arr).save(str(d / f"im{i}.png"))
    return str(d)


@pytest.mark.gpu
@pytest.mark.parametrize("dataset", ["cifar10", "celebA_test"])     # Trainer.recipe_for: random crop + mirror / the centre crop
def test_folder_loader_steps_equal_eager(monkeypatch, tmp_path, png_folder, dataset):
    """10 images, batch 4, drop_last: a new permutation every two steps; the indices travel through the static index buffer."""
    from colddiff.trainer import DeviceLoader, Trainer
    assert Trainer.recipe_for(dataset).crop == ("random" if dataset == "cifar10" else "center")
    tr = both(monkeypatch, tmp_path, 7, "unet3", data=png_folder, dataset=dataset, acc=1)
    assert isinstance(tr.dl, DeviceLoader) and tr.dl.epoch == 4
    graphed(tr, 7)


@pytest.mark.gpu
def test_recapture_on_precision_change_not_on_lr(monkeypatch, tmp_path):
    """Steps 4-6 in bf16, lr halved before step 3: the arithmetic mode is baked into the graph (a change warms up again), the
    learning rate travels in the uploaded scalars."""
    tr = both(monkeypatch, tmp_path, 8, "unet", run_kw=dict(bf16=(4, 5, 6), halve_lr_before=3))
    graphed(tr, 8, captures=3, replays=0)        # every change came within the warm-up of the graph before: see the next test


@pytest.mark.gpu
def test_recapture_replays_in_every_phase(monkeypatch, tmp_path):
    """The same with room for each of the three graphs to run: 1-3 warm up, 4-5 replay | bf16: 6-8 warm up, 9-10 replay | 11-13 warm
    up, 14-16 replay; lr halved before step 5, between two replays."""
    tr = both(monkeypatch, tmp_path, 16, "unet", run_kw=dict(bf16=(6, 7, 8, 9, 10), halve_lr_before=5))
    graphed(tr, 16, captures=3, replays=7)


@pytest.mark.gpu
def test_milestones_equal_eager(monkeypatch, tmp_path):
    """train() for 7 steps with a milestone every 3: checkpoints and sample grids of both modes are the same bytes."""
    outs = {}
    for name, graph in (("e", False), ("g", True)):
        monkeypatch.setenv("COLDDIFF_PREFETCH", "0")
        tr = build("unet", graph, tmp_path / name, train_num_steps=7, save_and_sample_every=3)
        _quiet(tr.train)
        torch.cuda.synchronize()
        files = sorted(os.listdir(tmp_path / name))
        assert "model.pt" in files and "sample-recon-2.png" in files, files
        outs[name] = (tr, files)
    (te, fe), (tg, fg) = outs["e"], outs["g"]
    assert fe == fg
    for f in fe:
        if f.endswith(".png"):
            assert open(tmp_path / "e" / f, "rb").read() == open(tmp_path / "g" / f, "rb").read(), f
        else:
            a, b = (torch.load(str(tmp_path / n / f), map_location="cpu") for n in ("e", "g"))
            assert a["step"] == b["step"]
            for part in ("model", "ema"):
                assert a[part].keys() == b[part].keys() and all(torch.equal(a[part][k], b[part][k]) for k in a[part]), (f, part)
    assert torch.equal(te.arena.data, tg.arena.data) and te.opt.step_count == tg.opt.step_count == 7
    graphed(tg, 7)


# ---- fallbacks -------------------------------------------------------------------------------------------------------------------
def _fallback(monkeypatch, tmp_path, N, prepare, **kw):
    monkeypatch.setenv("COLDDIFF_PREFETCH", "0")
    te = build("unet", False, tmp_path / "e", **kw)
    prepare(te)
    e = run(te, N)
    tg = build("unet", True, tmp_path / "g", **kw)
    prepare(tg)
    same(e, run(tg, N))
    return tg


@pytest.mark.gpu
def test_instance_loss_runs_eager(monkeypatch, tmp_path):
    def prepare(tr):
        tr._loss = lambda batch: tr.core(batch)
    st = _fallback(monkeypatch, tmp_path, 4, prepare).graph_state()
    assert st["mode"] == "eager" and "_loss" in st["reason"] and st["captures"] == st["replays"] == 0, st


@pytest.mark.gpu
def test_core_with_host_reads_runs_eager(monkeypatch, tmp_path):
    """Kernels of varying size: q_sample is the per-step fallback that reads max(t) on the host."""
    tr = _fallback(monkeypatch, tmp_path, 4, lambda tr: None, core_kw=dict(blur_routine="Individual_Incremental"))
    st = tr.graph_state()
    assert not tr.core.can_prepare_async() and not tr.core.graph_safe()
    assert st["mode"] == "eager" and "graph_safe" in st["reason"] and st["replays"] == 0, st


@pytest.mark.gpu
def test_capture_that_raises_falls_back_at_the_same_step(monkeypatch, tmp_path):
    """The capture method raises (a Python exception, nothing on the device) after it moved the loader and the CPU generator: the
    Trainer puts the host state back and runs the ordinary step from this very step on."""
    calls = []

    def prepare(tr):
        def boom(table):
            calls.append(tr.opt.step_count)
            tr._next_batch()
            torch.rand(3)
            tr.opt.step_count += 5
            raise RuntimeError("boom at capture")
        if tr._graph_req:
            tr._graph_capture = boom
    st = _fallback(monkeypatch, tmp_path, 7, prepare).graph_state()
    assert calls == [W], calls                                   # tried once, at the first step after the warm-up, never again
    assert st["mode"] == "eager" and "boom at capture" in st["reason"] and st["captures"] == 1 and st["replays"] == 0, st


@pytest.mark.gpu
def test_load_drops_the_graph(monkeypatch, tmp_path):
    tr = build("unet", True, tmp_path / "g")
    run(tr, 5)
    graphed(tr, 5)
    tr.save()
    _quiet(tr.load, str(tmp_path / "g" / "model.pt"))
    assert tr._gs["graph"] is None and tr.graph_state()["captures"] == 2
    _quiet(tr.train_step)
    assert tr.graph_state()["replays"] == 2


@pytest.mark.gpu
def test_another_trainer_stepping_between_replays(monkeypatch, tmp_path):
    """A second (eager) Trainer of another model steps between the replays: the packed-weight cache rebuilds its record table for that
    model's layouts and drops the one the graph was captured with -- the graph keeps its own alive and rewrites its layouts itself."""
    monkeypatch.setenv("COLDDIFF_PREFETCH", "0")
    e = run(build("unet", False, tmp_path / "e"), 8)
    cpu, cuda = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    other = build("unet3", False, tmp_path / "o")
    torch.set_rng_state(cpu), torch.cuda.set_rng_state(cuda, DEV)

    def between(tr, s):
        if s <= W + 1:                               # (stepping during the warm-up makes the capture pass build that table: it raises,
            return                                   #  and the Trainer runs eager -- test_capture_that_raises_... covers that path)
        state = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
        _quiet(other.train_step)                     # (its draws are taken back: the two runs compare their generators at the end)
        torch.set_rng_state(state[0]), torch.cuda.set_rng_state(state[1], DEV)
    tg = build("unet", True, tmp_path / "g")
    same(e, run(tg, 8, before=between))
    graphed(tg, 8)


# ---- GraphStep without a Trainer ---------------------------------------------------------------------------------------------------
def _standalone(raise_in_capture):
    """buf <- 2 buf + s on 1024 floats, s = the step's uploaded scalar (0.5 n at step n): upload -> capture -> replay at its smallest."""
    from colddiff import flat
    from colddiff.graphstep import GraphStep
    buf = torch.ones(1024, device=DEV)
    host = {"n": 0, "capture_passes": 0}

    def upload(table):
        host["n"] += 1
        table.upload(torch.tensor([0.5 * host["n"]] + [0.0] * 7), None, None)

    def step(table):
        if torch.cuda.is_current_stream_capturing():
            host["capture_passes"] += 1
            if raise_in_capture:
                host["n"] += 7                       # host state and a CPU draw the pass must not keep
                torch.rand(3)
                raise RuntimeError("boom in the capture pass")
        buf.mul_(2).add_(table.hp[0])
        table.end_step()
        return buf.sum()

    def snapshot():
        n = host["n"]
        return lambda: host.update(n=n)
    gs = _quiet(GraphStep, W, reason=lambda: None, signature=lambda: 0, table=lambda: flat.StepTable(torch.device(DEV), 0), upload=upload, step=step,
                snapshot=snapshot)
    return gs, buf, host


def _recurrence(n_steps):
    want = torch.ones(1024)
    for n in range(1, n_steps + 1):
        want = want * 2 + 0.5 * n
    return want


@pytest.mark.gpu
def test_graphstep_standalone_upload_capture_replay():
    gs, buf, host = _standalone(False)
    for n in range(1, W + 4):                        # W eager graph-form steps, then the capture and three replays
        out = _quiet(gs.step)
        assert torch.equal(out.cpu(), _recurrence(n).sum()), n
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), _recurrence(W + 3)) and host == {"n": W + 3, "capture_passes": 1}
    assert gs.state() == {"mode": "graph", "reason": f"the step is captured after {W} warm-up steps", "captures": 1, "replays": 3}


@pytest.mark.gpu
def test_graphstep_standalone_capture_that_raises():
    gs, buf, host = _standalone(True)
    for _ in range(W):
        assert _quiet(gs.step) is not None
    torch.manual_seed(9)
    cpu, cuda = torch.get_rng_state(), torch.cuda.get_rng_state(DEV)
    for _ in range(3):                               # the pass that raises, and two more steps: no second attempt
        assert _quiet(gs.step) is None
    assert host == {"n": W, "capture_passes": 1}
    assert torch.equal(torch.get_rng_state(), cpu) and torch.equal(torch.cuda.get_rng_state(DEV), cuda)
    st = gs.state()
    assert st["mode"] == "eager" and "boom in the capture pass" in st["reason"] and st["captures"] == 1 and st["replays"] == 0, st
    assert gs.graph is None and gs.table is None
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), _recurrence(W))    # the pass launched nothing


# ---- the default path stays the default path --------------------------------------------------------------------------------------
NEW = {"cdf_adam_step_dev", "cdf_groupnorm_fwd_ex_sd", "cdf_groupnorm_bwd_ex_sd", "cdf_dropout_sd", "cdf_adam_params"}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["unet", "model"])
def test_new_entry_points_only_in_graph_mode(monkeypatch, tmp_path, kind):
    from colddiff import runtime as rt
    from test_gpu_invariance import Recorder
    tr = build(kind, False, tmp_path / "e")
    with Recorder(rt.lib()) as rec:
        _quiet(tr.train_step)
    assert "cdf_adam_step" in rec.names() and not rec.names() & NEW, sorted(rec.names() & NEW)
    tr = build(kind, True, tmp_path / "g")
    with Recorder(rt.lib()) as rec:
        for _ in range(W + 1):                                   # the warm-up and the capture pass
            _quiet(tr.train_step)
            tr.step += 1
    torch.cuda.synchronize()
    want = {"cdf_adam_step_dev", "cdf_adam_params"} | ({"cdf_groupnorm_fwd_ex_sd", "cdf_groupnorm_bwd_ex_sd"} if kind == "model" else set())
    # (cdf_dropout_sd, like cdf_dropout, is the standalone form no network of the package launches: ops.dropout, test_graph_kernels.py)
    assert rec.names() & NEW == want and "cdf_adam_step" not in rec.names(), sorted(rec.names() & NEW)
    assert sum(n == "cdf_adam_step_dev" for n, _ in rec.calls) == W + 1
    graphed(tr, W + 1)


# ---- without a GPU ----------------------------------------------------------------------------------------------------------------
def _cpu_trainer(tmp_path, **kw):
    from deblurring_diffusion_pytorch import GaussianDiffusion, Trainer, Unet
    torch.manual_seed(0)
    net = _quiet(Unet, dim=8, dim_mults=(1, 2), channels=1)
    diff = GaussianDiffusion(net, image_size=8, device_of_kernel="cpu", channels=1, timesteps=3, loss_type="l1", kernel_std=1.0, kernel_size=3,
                             blur_routine="Constant", train_routine="Final", sampling_routine="x0_step_down")
    return _quiet(Trainer, diff, None, image_size=8, train_batch_size=2, gradient_accumulate_every=2, dataset="synthetic",
                  results_folder=str(tmp_path / "r"), **kw)


def test_simulator_runs_eager_and_env_is_read_only_for_none(monkeypatch, tmp_path, capsys):
    from emu_util import install_emu, uninstall_emu
    install_emu()
    try:
        monkeypatch.delenv("COLDDIFF_GRAPH", raising=False)
        tr = _cpu_trainer(tmp_path, graph=True)
        loss = tr.train_step()
        st = tr.graph_state()
        assert st["mode"] == "eager" and st["reason"] in ("no HIP device", "library override") and st["captures"] == st["replays"] == 0, st
        assert torch.isfinite(loss) and tr.opt.step_count == 1
        tr.train_step()
        assert capsys.readouterr().out.count("graph mode:") == 1           # printed once, when it is decided
        assert _cpu_trainer(tmp_path).graph_state() == {"mode": "off", "reason": "not requested", "captures": 0, "replays": 0}
        monkeypatch.setenv("COLDDIFF_GRAPH", "1")
        assert _cpu_trainer(tmp_path).graph_state()["mode"] == "eager"          # None reads the variable ...
        assert _cpu_trainer(tmp_path, graph=False).graph_state()["mode"] == "off"   # ... an explicit argument does not
        monkeypatch.setenv("COLDDIFF_GRAPH", "yes")
        assert _cpu_trainer(tmp_path).graph_state()["mode"] == "off"            # only "1" turns it on
        assert _cpu_trainer(tmp_path, graph=True).graph_state()["mode"] == "eager"
    finally:
        uninstall_emu()
