"""`Trainer` of the snowification package on a folder of generated PNGs (16 x 16 crops of 20 x 20 files): one optimizer step with
`gradient_accumulate_every=2` (`Final`) against the CPU restatement of the same step -- `state_t` on the planes the engine built (held to
the reference's by tests/test_snow_golden.py) and the oracle's functional UNet, `t` replayed -- under the bounds of the decolorization
trainer test (loss 1e-5, every weight 1e-6); the fused two-micro-batch pass against COLDDIFF_FUSE_ACCUM=0; the checkpoint round trip;
and the launch count of the forward process.  Simulator (CPU tensors, host DataLoader) and MI355X (device image cache).
"""
import os

import pytest
import torch

import snow_ref as R
from oracle import cold_oracle as O
from test_decolor_trainer import MBE, Recorder, mbe, png_folder, quiet, rows_are_crops  # noqa: F401  (mbe: the fixture)

pytest.importorskip("scipy.ndimage")
T, SIZE = 6, 16


def make(mbe, tmp_path, name, seed=0, **kw):
    D = R.mine()
    torch.manual_seed(seed)
    net = quiet(D.UnetConvNextBlock, dim=8, dim_mults=(1, 2)).to(mbe.device)
    gd_kw = {k: kw.pop(k) for k in list(kw) if k in ("sampling_routine", "train_routine", "random_snow", "snow_level")}
    diff = D.GaussianDiffusion(net, image_size=(SIZE, SIZE), device_of_kernel='cuda', channels=3, timesteps=T, loss_type='l1',
                               forward_process_type='Snow', batch_size=2, results_folder=str(tmp_path / name), **gd_kw).to(mbe.device)
    crops = png_folder(str(tmp_path / "imgs"))
    tr = quiet(D.Trainer, diff, str(tmp_path / "imgs"), image_size=(SIZE, SIZE), train_batch_size=2, train_lr=2e-5, gradient_accumulate_every=2,
               results_folder=str(tmp_path / name / "nested"), num_workers=0, **kw)
    return net, diff, tr, crops


def _replay(tr, mbe, micro):
    it = iter(micro)
    tr._prepare_micro = lambda it=it: (lambda x, t: tr.core.prepare(x, t=mbe.to(t)))(*next(it))


def test_one_optimizer_step_matches_the_cpu_restatement(mbe, tmp_path, monkeypatch):
    net, diff, tr, crops = make(mbe, tmp_path, "res", train_num_steps=1)
    assert tr.device_data == (mbe.kind == "hip") and tr._can_fuse() and tr.num_timesteps == T
    fp = diff.forward_process
    planes, br = fp.planes(mbe.device).cpu().clone(), fp.br_coef_list
    assert (planes != 0).any()
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    otr = O.OracleTrainer(sd0, lambda p, x, t: O.loss_fn(x, O.unet_forward(p, R.state_t(x, None, (t + 1).tolist(), planes, br), t)), lr=2e-5,
                          accumulate=2)
    g = torch.Generator().manual_seed(1)
    micro = []
    for _ in range(2):
        x = tr._next_batch()
        assert x.shape == (2, 3, SIZE, SIZE) and rows_are_crops(x, crops)
        micro.append((x, torch.randint(0, T, (2,), generator=g)))
    some = R.state_t(micro[0][0].cpu(), None, [T, T], planes, br)
    assert 0.0 < (some == 1.0).float().mean().item() < 1.0                       # the clip is on the path, not everywhere
    _replay(tr, mbe, micro)
    loss = tr.train_step()
    lo = otr.train_step([(x.cpu(), t) for x, t in micro])
    print(f"snow trainer step [{mbe.kind}]: loss {loss.item():.6f} (restatement {lo:.6f})")
    assert abs(loss.item() - lo) <= 1e-5
    for k in sd0:
        assert (net.state_dict()[k].cpu() - otr.params[k].detach()).abs().max() <= 1e-6, k
    # the same step, one micro-batch at a time
    monkeypatch.setenv("COLDDIFF_FUSE_ACCUM", "0")
    net2, diff2, tr2, _ = make(mbe, tmp_path, "res2", train_num_steps=1)
    assert not tr2._can_fuse()
    net2.load_state_dict(sd0)
    it = iter(micro)
    tr2._loss = lambda batch: (lambda x, t: tr2.core.loss_prepared(tr2.core.prepare(x, t=mbe.to(t))))(*next(it))
    loss2 = tr2.train_step()
    print(f"snow trainer step, COLDDIFF_FUSE_ACCUM=0 [{mbe.kind}]: loss {loss2.item():.6f}")
    assert abs(loss2.item() - loss.item()) <= 1e-5
    for k in sd0:
        assert (net2.state_dict()[k].cpu() - net.state_dict()[k].cpu()).abs().max() <= 1e-6, k


def test_checkpoint_round_trip(mbe, tmp_path):
    net, diff, tr, crops = make(mbe, tmp_path, "ck", train_num_steps=1)
    tr.step = 3
    tr.save()
    tr.save(save_with_time_stamp=True)
    res = tmp_path / "ck" / "nested"
    ck = torch.load(str(res / "model.pt"), map_location="cpu", weights_only=False)
    assert sorted(ck) == ["ema", "model", "step"] and ck["step"] == 3 and os.path.exists(res / "model_3.pt")
    assert "denoise_fn.time_mlp.1.weight" in ck["model"] and all(k.startswith("denoise_fn.") for k in ck["model"])
    assert not os.path.exists(tmp_path / "ck" / "snow_base.npy")                 # upstream computes the path and never writes it
    before = {k: v.clone() for k, v in tr.model.state_dict().items()}
    with torch.no_grad():
        for p in tr.model.parameters():
            p.add_(1.0)
    tr.step = 0
    quiet(tr.load, str(res / "model.pt"))
    assert tr.step == 3 and all(torch.equal(v, tr.model.state_dict()[k]) for k, v in before.items())


def test_the_forward_process_is_one_launch_per_call(mbe):
    from colddiff import runtime as rt
    D = R.mine()
    gd = D.GaussianDiffusion(None, image_size=(8, 8), device_of_kernel='cuda', timesteps=50, forward_process_type='Snow', results_folder=None)
    x = mbe.to(torch.rand(4, 3, 8, 8) * 2 - 1)
    gd.forward_process.planes(mbe.device)                                         # built once, on first use
    for t in ([0, 0, 0, 0], [49, 3, 20, 0], [5, -1, 2, -1]):
        with Recorder(rt.lib()) as rec:
            gd.q_sample(x, mbe.to(torch.tensor(t)), return_total_blur=True)
            gd.q_sample(x, mbe.to(torch.tensor(t)))
        assert rec.calls == ["cdf_snow_chain", "cdf_snow_chain"], (t, rec.calls)
    with Recorder(rt.lib()) as rec:
        gd.prepare(x, t=mbe.to(torch.tensor([49, 3, 20, 0])))
        gd.forward_process.forward(None, 49, og=x)
        gd.forward_process.total_forward(x)
    assert rec.calls == ["cdf_snow_chain"] * 3
    gd.denoise_fn = lambda img, t: img
    t_host = torch.tensor([49, 3, 20, 0])
    for samp in ("x0_step_down", "default"):
        gd.sampling_routine = samp
        with Recorder(rt.lib()) as rec:
            a = gd.sample_one_step(x, mbe.to(t_host))[0]
        assert rec.calls == ["cdf_snow_chain"], samp
        assert torch.equal(a, gd.sample_one_step(x, t_host)[0])                   # a step vector left on the host is moved, not handed over
    gd.recon_noise_std = 0.1                                                      # the noise reaches the kernel as `start`: still one launch
    gd.sampling_routine = "x0_step_down"
    with Recorder(rt.lib()) as rec:
        gd.sample_one_step(x, mbe.to(torch.tensor([0, 3, 0, 2])))
    assert rec.calls == ["cdf_snow_chain"]
    gd2 = D.GaussianDiffusion(None, image_size=(8, 8), device_of_kernel='cuda', timesteps=50, forward_process_type='Snow', results_folder=None,
                              random_snow=True)
    with Recorder(rt.lib()) as rec:                                               # random_snow: the layers are part of the training step
        gd2.prepare(x, t=mbe.to(t_host))
    assert rec.calls == ["cdf_snow_layers", "cdf_snow_chain"]
