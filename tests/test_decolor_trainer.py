"""`Trainer` of the decolorization package on a folder of generated PNGs (16 x 16 crops of 20 x 20 files): a few optimizer steps with
`gradient_accumulate_every=2` against the CPU restatement of the same steps with `t` replayed (bounds of the existing Trainer tests: loss
1e-5, every weight 1e-6), the checkpoint round trip with the reference's dict keys, a milestone's four PNGs, Lab batches with
`to_lab=True`, and the launch count of `q_sample`.  Simulator (CPU tensors, host DataLoader) and MI355X (device image cache).
"""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import decolor_ref as R
from oracle import cold_oracle as O
from test_color_kernels import LAB_SCALE, LAB_SINGLE_TOL

T, SIZE, FILE = 6, 16, 20


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


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def png_folder(path, n=8, seed=5):
    """n random RGB PNGs of FILE x FILE; -> the [n,3,SIZE,SIZE] centre crops in (-1, 1) as CenterCrop + ToTensor + t * 2 - 1 yield them."""
    from PIL import Image
    os.makedirs(path, exist_ok=True)
    rng = np.random.RandomState(seed)
    crops = []
    o = int(round((FILE - SIZE) / 2.0))
    for i in range(n):
        a = rng.randint(0, 256, (FILE, FILE, 3), dtype=np.uint8)
        Image.fromarray(a).save(os.path.join(path, f"img{i:02d}.png"))
        crops.append(torch.from_numpy(a[o:o + SIZE, o:o + SIZE].copy()).permute(2, 0, 1).float().div(255) * 2 - 1)
    return torch.stack(crops)


def make(mbe, tmp_path, name, seed=0, **kw):
    D = R.mine()
    torch.manual_seed(seed)
    net = quiet(D.UnetConvNextBlock, dim=8, dim_mults=(1, 2)).to(mbe.device)
    gd_kw = {k: kw.pop(k) for k in list(kw) if k in ("to_lab", "sampling_routine", "train_routine")}
    diff = D.GaussianDiffusion(net, image_size=(SIZE, SIZE), device_of_kernel='cuda', channels=3, timesteps=T, loss_type='l1', **gd_kw).to(mbe.device)
    crops = png_folder(str(tmp_path / "imgs"))
    tr = quiet(D.Trainer, diff, str(tmp_path / "imgs"), image_size=(SIZE, SIZE), train_batch_size=2, train_lr=2e-5, gradient_accumulate_every=2,
               results_folder=str(tmp_path / name / "nested"), num_workers=0, to_lab=gd_kw.get("to_lab", False), **kw)
    return net, diff, tr, crops


def rows_are_crops(batch, crops, tol=0.0):
    b = batch.detach().cpu()
    return all(min((b[i] - c).abs().max().item() for c in crops) <= tol for i in range(b.shape[0]))


def test_optimizer_steps_match_the_cpu_restatement(mbe, tmp_path):
    net, diff, tr, crops = make(mbe, tmp_path, "res", train_num_steps=3)
    assert tr.device_data == (mbe.kind == "hip") and tr._can_fuse()
    assert tr.image_size == (SIZE, SIZE) and tr.num_timesteps == T and tr.batch_size == 2
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    table = R.table_of("Constant", T)
    otr = O.OracleTrainer(sd0, lambda p, x, t: O.loss_fn(x, O.unet_forward(p, R.chain_t(x, table, (t + 1).tolist()), t)), lr=2e-5, accumulate=2)
    g = torch.Generator().manual_seed(1)
    for s in range(3):
        micro = []
        for _ in range(2):
            x = tr._next_batch()
            assert x.shape == (2, 3, SIZE, SIZE) and rows_are_crops(x, crops), "a batch row is not a centre crop of a file"
            micro.append((x, torch.randint(0, T, (2,), generator=g)))
        it = iter(micro)
        tr._prepare_micro = lambda it=it: (lambda x, t: tr.core.prepare(x, t=mbe.to(t)))(*next(it))
        loss = tr.train_step()
        tr.step += 1
        lo = otr.train_step([(x.cpu(), t) for x, t in micro])
        print(f"step {s} [{mbe.kind}]: loss {loss.item():.6f} (restatement {lo:.6f})")
        assert abs(loss.item() - lo) <= 1e-5
        for k in sd0:
            assert (net.state_dict()[k].cpu() - otr.params[k].detach()).abs().max() <= 1e-6, k
    ema_sd = tr.ema_core.denoise_fn.state_dict()
    for k in sd0:
        assert (ema_sd[k].cpu() - otr.ema[k]).abs().max() <= 1e-6
    # checkpoint round trip: the reference's dict keys, model.pt / model_<step>.pt
    tr.save()
    tr.save(save_with_time_stamp=True)
    res = tmp_path / "res" / "nested"
    ck = torch.load(str(res / "model.pt"), map_location="cpu", weights_only=False)
    assert sorted(ck) == ["ema", "model", "step"] and ck["step"] == 3 and os.path.exists(res / "model_3.pt")
    assert "denoise_fn.time_mlp.1.weight" in ck["model"] and "denoise_fn.final_conv.1.bias" in ck["ema"]
    before = {k: v.clone() for k, v in tr.model.state_dict().items()}
    with torch.no_grad():
        for p in tr.model.parameters():
            p.add_(1.0)
    tr.step = 0
    quiet(tr.load, str(res / "model.pt"))
    assert tr.step == 3 and all(torch.equal(v, tr.model.state_dict()[k]) for k, v in before.items())


def test_train_loop_writes_the_milestone_files(mbe, tmp_path):
    net, diff, tr, crops = make(mbe, tmp_path, "mile", sampling_routine="x0_step_down", train_num_steps=2, save_and_sample_every=1,
                                save_with_time_stamp_every=1)
    quiet(tr.train)
    res = tmp_path / "mile" / "nested"
    for k in ("xt", "direct_recons", "recon", "og"):
        assert os.path.exists(res / f"sample-{k}-1.png"), k
    assert os.path.exists(res / "model.pt") and os.path.exists(res / "model_1.pt") and tr.step == 2
    from PIL import Image
    og = np.asarray(Image.open(res / "sample-og-1.png"))
    assert og.ndim == 3 and og.shape[2] == 3 and og.max() > 0


def test_to_lab_feeds_lab_batches(mbe, tmp_path):
    net, diff, tr, crops = make(mbe, tmp_path, "lab", to_lab=True, train_num_steps=1)
    x = tr._next_batch()
    lab_crops = R.rgb2lab_t(crops)
    b = x.detach().cpu()
    worst = max(min(((b[i] - c).abs() / LAB_SCALE[0]).max().item() for c in lab_crops) for i in range(b.shape[0]))
    print(f"Lab batch against the CPU restatement [{mbe.kind}]: {worst:.3g} of the channel scale")
    assert worst <= LAB_SINGLE_TOL
    assert tr._process_item([crops[:1].to(x.device)]).shape == (1, 3, SIZE, SIZE)
    loss = tr.train_step()
    assert torch.isfinite(loss).item()


class Recorder:
    def __init__(self, lib):
        self.lib, self.calls, self.orig = lib, [], {}

    def __enter__(self):
        for name in list(vars(self.lib)):
            if name.startswith("cdf_"):
                fn = self.orig[name] = getattr(self.lib, name)
                setattr(self.lib, name, (lambda n, f: lambda *a: (self.calls.append(n), f(*a))[1])(name, fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self.orig.items():
            setattr(self.lib, name, fn)


@pytest.mark.parametrize("lab", [False, True])
def test_q_sample_is_one_launch_whatever_t_max_is(mbe, lab):
    from colddiff import runtime as rt
    D = R.mine()
    gd = D.GaussianDiffusion(None, image_size=(8, 8), device_of_kernel='cuda', timesteps=50, to_lab=lab)
    x = mbe.to(torch.rand(4, 3, 8, 8) * 2 - 1)
    for t in ([0, 0, 0, 0], [49, 3, 20, 0], [5, -1, 2, -1]):
        with Recorder(rt.lib()) as rec:
            gd.q_sample(x, mbe.to(torch.tensor(t)), return_total_blur=True)
            gd.q_sample(x, mbe.to(torch.tensor(t)))
        assert rec.calls == ["cdf_color_chain", "cdf_color_chain"], (t, rec.calls)
    with Recorder(rt.lib()) as rec:                       # the training path: the step vector is built on the device
        gd.prepare(x, t=mbe.to(torch.tensor([49, 3, 20, 0])))
    assert rec.calls == ["cdf_color_chain"]
    # a step vector left on the host is moved to the images' device, not handed to the kernel as it is
    t_host = torch.tensor([49, 3, 20, 0])
    assert torch.equal(gd.q_sample(x, t_host), gd.q_sample(x, mbe.to(t_host)))
    gd2 = D.GaussianDiffusion(None, image_size=(8, 8), device_of_kernel='cuda', timesteps=50, to_lab=lab, sampling_routine="x0_step_down")
    gd2.denoise_fn = lambda img, t: img                    # (the reverse step's own launches: one chain with the combine fused in)
    with Recorder(rt.lib()) as rec:
        gd2.sample_one_step(x, mbe.to(torch.tensor([49, 3, 20, 0])))
    assert rec.calls == ["cdf_color_chain"]
    assert torch.equal(gd2.sample_one_step(x, t_host)[0], gd2.sample_one_step(x, mbe.to(t_host))[0])
    gd2.sampling_routine = "default"                       # (this routine never needs t.max())
    with Recorder(rt.lib()) as rec:
        gd2.sample_one_step(x, mbe.to(t_host))
    assert rec.calls == ["cdf_color_chain"]
