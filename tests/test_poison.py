"""Memory nobody wrote must not matter: every network-level path, run once on ordinary allocations and once with every
`torch.empty` / `torch.empty_like` of the package pre-filled with NaN (tests/poison.py), must give BIT-identical results.

A kernel that skips a ragged tile, the last split-K slab or the last chunk, or that reads a pad column it never wrote (even to
multiply it by a zero weight: 0 * NaN = NaN), passes an ordinary run whenever the recycled memory happens to hold harmless
values; under poison it turns the result into NaN.  Fixture `mbe` (tests/test_modules.py): the simulator on CPU tensors and,
gpu-marked, the MI355X -- where the allocator really does hand back recycled memory.
"""
import contextlib

import pytest
import torch

from poison import poisoned_allocations
from test_modules import mbe, quiet  # noqa: F401


def _twice(fn):
    """fn() on ordinary allocations, then under poison: every returned tensor bit for bit the same (and finite)."""
    from colddiff import runtime as rt
    outs = []
    for ctx in (contextlib.nullcontext(), poisoned_allocations()):
        rt.bump_weights_epoch()                       # (fresh packed-weight layouts: their buffers are poisoned too)
        with ctx:
            outs.append([t.detach().cpu().clone() for t in fn()])
            if torch.cuda.is_available():
                torch.cuda.synchronize()
    assert len(outs[0]) == len(outs[1])
    for i, (a, b) in enumerate(zip(*outs)):
        assert torch.isfinite(a).all(), i
        assert torch.equal(a, b), (i, (a - b).abs().max().item())


def _fwd_bwd(mbe, make, x, t, gy):
    """A fresh network from the same state each time (its packed weights are allocated anew), forward + backward: the output,
    the input gradient and every parameter gradient."""
    def run():
        net = make().to(mbe.device)
        xd = mbe.to(x).clone().requires_grad_(True)
        y = net(xd, mbe.to(t))
        y.backward(mbe.to(gy))
        return [y, xd.grad] + [p.grad for p in net.parameters()]
    return run


def _unet(sd, **kw):
    from deblurring_diffusion_pytorch import Unet

    def make():
        net = quiet(Unet, **kw)
        net.load_state_dict(sd)
        return net
    return make


def _state(cls, **kw):
    torch.manual_seed(7)
    return quiet(cls, **kw).state_dict()


@pytest.mark.parametrize("kw,size", [(dict(dim=8, dim_mults=(1, 2), channels=3), 16),
                                     (dict(dim=64, dim_mults=(1, 2, 4), channels=3), 16),     # pre-split, halo, LN-backward epilogue
                                     (dict(dim=16, dim_mults=(1, 2), channels=1), 16)])       # one channel: 1 -> 4 padded columns
def test_unet_poisoned_bit_identical(mbe, kw, size):
    from deblurring_diffusion_pytorch import Unet
    sd = _state(Unet, **kw)
    torch.manual_seed(1)
    c = kw["channels"]
    x, t, gy = torch.rand(2, c, size, size) * 2 - 1, torch.tensor([3, 17]), torch.randn(2, c, size, size)
    _twice(_fwd_bwd(mbe, _unet(sd, **kw), x, t, gy))


def test_model_with_attention_poisoned_bit_identical(mbe):
    from deblurring_diffusion_pytorch import Model
    kw = dict(resolution=8, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(4,), dropout=0.0)
    sd = _state(Model, **kw)

    def make():
        net = Model(**kw)
        net.load_state_dict(sd)
        return net
    torch.manual_seed(1)
    x, t, gy = torch.rand(2, 3, 8, 8) * 2 - 1, torch.tensor([3, 17]), torch.randn(2, 3, 8, 8)
    _twice(_fwd_bwd(mbe, make, x, t, gy))


@pytest.mark.parametrize("mode", ["f32", "bf16"])          # bf16: the bf16 activation-storage stream
def test_precision_modes_poisoned_bit_identical(mbe, mode):
    from colddiff import runtime as rt, bf16store as BFS
    from deblurring_diffusion_pytorch import Unet
    kw = dict(dim=16, dim_mults=(1, 2, 4), channels=3)
    sd = _state(Unet, **kw)
    torch.manual_seed(1)
    x, t, gy = torch.rand(2, 3, 16, 16) * 2 - 1, torch.tensor([3, 17]), torch.randn(2, 3, 16, 16)
    with rt.precision_scope(mode):
        assert BFS.enabled() == (mode == "bf16")
        _twice(_fwd_bwd(mbe, _unet(sd, **kw), x, t, gy))


def test_trainer_fused_step_poisoned_bit_identical(mbe, tmp_path):
    """One Trainer._fused_step (two micro-batches as one pass), then the Adam update: loss, every gradient, the new weights."""
    from denoising_diffusion_pytorch import GaussianDiffusion, Trainer, Unet
    kw = dict(dim=8, dim_mults=(1, 2), channels=3)
    sd = _state(Unet, **kw)
    g = torch.Generator().manual_seed(2)
    xs, es, ts = torch.rand(4, 3, 16, 16, generator=g) * 2 - 1, torch.randn(4, 3, 16, 16, generator=g), torch.randint(0, 10, (4,), generator=g)

    def run():
        net = quiet(Unet, **kw)
        net.load_state_dict(sd)
        diff = GaussianDiffusion(net.to(mbe.device), image_size=16, channels=3, timesteps=10).to(mbe.device)
        tr = quiet(Trainer, diff, None, image_size=16, train_batch_size=2, train_lr=1e-3, train_num_steps=1, gradient_accumulate_every=2,
                   dataset="synthetic", results_folder=str(tmp_path / "res"))
        assert tr._can_fuse()
        xi, ei, ti = iter(xs.split(2)), iter(es.split(2)), iter(ts.split(2))
        tr._next_batch = lambda: mbe.to(next(xi))
        tr._second = lambda batch: mbe.to(next(ei))
        tr.core._draw_t = lambda x: mbe.to(next(ti))
        loss = tr._fused_step(2, False)
        grads = [p.grad.clone() for p in net.parameters()]
        tr.opt.step()
        return [loss.reshape(1)] + grads + [p for p in net.parameters()]
    _twice(run)


def test_gen_sample_poisoned_bit_identical(mbe):
    """A few reverse steps of Algorithm 2 (denoising package, x0_step_down)."""
    from denoising_diffusion_pytorch import GaussianDiffusion, Unet
    kw = dict(dim=8, dim_mults=(1, 2), channels=3)
    sd = _state(Unet, **kw)
    torch.manual_seed(1)
    noise = torch.randn(2, 3, 16, 16)

    def run():
        net = quiet(Unet, **kw)
        net.load_state_dict(sd)
        d = GaussianDiffusion(net.to(mbe.device), image_size=16, channels=3, timesteps=4, sampling_routine="x0_step_down").to(mbe.device)
        with torch.no_grad():
            return list(quiet(d.gen_sample, batch_size=2, img=mbe.to(noise)))
    _twice(run)


def test_degradation_chains_poisoned_bit_identical(mbe):
    """One call each of the blur, pixelate and mask degradation chains (q_sample at mixed per-sample t)."""
    from deblurring_diffusion_pytorch import GaussianDiffusion as Blur
    from resolution_diffusion_pytorch import GaussianDiffusion as Pix
    from defading_diffusion_pytorch import GaussianDiffusion as Fade
    torch.manual_seed(1)
    x, t = torch.rand(3, 3, 16, 16) * 2 - 1, torch.tensor([4, 0, 2])
    ident = torch.nn.Identity()

    def run():
        blur = Blur(ident, image_size=16, device_of_kernel="cuda", channels=3, timesteps=5, kernel_std=0.3, kernel_size=5,
                    blur_routine="Incremental").to(mbe.device)
        pix = Pix(ident, image_size=16, device_of_kernel="cuda", channels=3, timesteps=3, resolution_routine="Incremental_factor_2")
        fade = Fade(ident, image_size=16, device_of_kernel="cuda", channels=3, timesteps=5, kernel_std=0.6, initial_mask=1,
                    fade_routine="Incremental")
        with torch.no_grad():
            xd = mbe.to(x)
            return [blur.q_sample(xd, mbe.to(t)), pix.q_sample(xd, mbe.to(t.clamp(max=2))), fade.q_sample(xd, mbe.to(t))]
    _twice(run)
