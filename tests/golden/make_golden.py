"""Generate the golden vectors under tests/golden/ by running the UNMODIFIED reference
(/root/reference, imported through oracle/ref_shim.py) on CPU with seed 123457
(deblurring-diffusion-pytorch/celebA_128_test.py:14).  Build-container only; the .pt fixtures it
writes are committed and travel to the GPU box.

    python tests/golden/make_golden.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from oracle import ref_shim  # noqa: E402

SEED = 123457


def images(B, C, H, g):
    return torch.randint(0, 256, (B, C, H, H), generator=g).float() / 255 * 2 - 1


def unet_case(ref):
    torch.manual_seed(SEED)
    net = ref.Unet(dim=8, dim_mults=(1, 2, 4), channels=3)
    g = torch.Generator().manual_seed(SEED)
    x, t = images(2, 3, 16, g), torch.tensor([3, 17])
    y = net(x, t)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    grads = {k: p.grad.clone() for k, p in net.named_parameters()}
    return {"cfg": dict(dim=8, dim_mults=(1, 2, 4), channels=3), "sd": {k: v.clone() for k, v in net.state_dict().items()},
            "x": x, "t": t, "y": y.detach(), "gy": gy, "grads": grads}


def model_case(ref, **extra):
    torch.manual_seed(SEED)
    cfg = dict(resolution=8, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(4,), dropout=0.0, **extra)
    net = ref.Model(**cfg)
    g = torch.Generator().manual_seed(SEED)
    x, t = images(2, 3, 8, g), torch.tensor([0, 9])
    y = net(x, t)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    return {"cfg": cfg, "sd": {k: v.clone() for k, v in net.state_dict().items()}, "x": x, "t": t, "y": y.detach(), "gy": gy,
            "grads": {k: p.grad.clone() for k, p in net.named_parameters()}}


def diffusion_cases():
    out = {}
    g = torch.Generator().manual_seed(SEED)
    # ---- deblurring ------------------------------------------------------------------------------
    ref = ref_shim.load("deblurring")
    torch.manual_seed(SEED)
    net = ref.Unet(dim=8, dim_mults=(1, 2), channels=3)
    for routine, ks, std in (("Incremental", 3, 0.4), ("Constant", 5, 1.0), ("Exponential_reflect", 5, 0.2), ("Special_6_routine", 11, 0)):
        for sampling in ("default", "x0_step_down"):
            T = 4
            d = ref.GaussianDiffusion(net, image_size=16, device_of_kernel="cpu", channels=3, timesteps=T, kernel_std=std, kernel_size=ks,
                                      blur_routine=routine, sampling_routine=sampling)
            x, t = images(3, 3, 16, g), torch.tensor([0, 3, 2])
            with torch.no_grad():
                xq = d.q_sample(x, t)
                xt, direct, img = d.sample(batch_size=3, img=x)
            out[f"deblur/{routine}/{sampling}"] = dict(T=T, ks=ks, std=std, x=x, t=t, q=xq, xt=xt, direct=direct, img=img,
                                                       kernels=[m.weight.detach().clone() for m in d.gaussian_kernels],
                                                       modes=[m.padding_mode for m in d.gaussian_kernels])
    out["deblur/net_sd"] = {k: v.clone() for k, v in net.state_dict().items()}
    # ---- denoising ------------------------------------------------------------------------------------
    ref = ref_shim.load("denoising")
    for sampling in ("x0_step_down", "ddim"):
        T = 5
        d = ref.GaussianDiffusion(net, image_size=16, channels=3, timesteps=T, sampling_routine=sampling)
        x, eps, t = images(3, 3, 16, g), torch.randn(3, 3, 16, 16, generator=g), torch.tensor([0, 4, 2])
        with torch.no_grad():
            xq = d.q_sample(x, eps, t)
            n1, d1, i1 = d.gen_sample(batch_size=3, img=eps)
            n2, d2, i2 = d.sample(batch_size=3, img=eps)
        out[f"denoise/{sampling}"] = dict(T=T, x=x, eps=eps, t=t, q=xq, gen=i1, sample=i2, ca=d.sqrt_alphas_cumprod.clone(),
                                          cb=d.sqrt_one_minus_alphas_cumprod.clone())
    # ---- resolution -----------------------------------------------------------------------------------
    ref = ref_shim.load("resolution")
    for routine in ("Incremental", "Incremental_area", "Incremental_factor_2", "Incremental_area_factor_2", "Incremental_bilinear_factor_2"):
        T = 3
        d = ref.GaussianDiffusion(net, image_size=16, device_of_kernel="cpu", channels=3, timesteps=T, resolution_routine=routine,
                                  sampling_routine="x0_step_down")
        x, t = images(3, 3, 16, g), torch.tensor([0, 2, 1])
        with torch.no_grad():
            xq = d.q_sample(x, t)
            xt, direct, img = d.sample(batch_size=3, img=x)
        out[f"resolution/{routine}"] = dict(T=T, x=x, t=t, q=xq, xt=xt, img=img)
    # ---- defading -------------------------------------------------------------------------------------
    ref = ref_shim.load("defading")
    for sampling in ("default", "x0_step_down"):
        T = 5
        d = ref.GaussianDiffusion(net, image_size=16, device_of_kernel="cpu", channels=3, timesteps=T, kernel_std=0.6, initial_mask=1,
                                  fade_routine="Incremental", sampling_routine=sampling)
        x, t = images(3, 3, 16, g), torch.tensor([0, 4, 2])
        with torch.no_grad():
            xq = d.q_sample(x, t)
            xt, direct, img = d.sample(batch_size=3, faded_recon_sample=x)
        out[f"defade/{sampling}"] = dict(T=T, x=x, t=t, q=xq, xt=xt, img=img, masks=d.fade_kernels.clone())
    return out


def variant_cases(net_sd):
    """Sampler variants (SURVEY §8 row C1 "and variants") and the resolution training routines (row A6)."""
    import contextlib
    import io
    out = {}
    g = torch.Generator().manual_seed(SEED + 1)
    cpu = lambda L: [z.clone() for z in L]
    quiet = lambda: contextlib.redirect_stdout(io.StringIO())       # the reference prints its loop counters
    # ---- deblurring: forward_and_backward, forward_and_backward_2, sample_from_blur, all_sample ------------
    ref = ref_shim.load("deblurring")
    net = ref.Unet(dim=8, dim_mults=(1, 2), channels=3)
    net.load_state_dict(net_sd)
    for routine, ks, std in (("Incremental", 3, 0.4), ("Exponential_reflect", 5, 0.2)):
        for sampling in ("default", "x0_step_down"):
            T = 4
            d = ref.GaussianDiffusion(net, image_size=16, device_of_kernel="cpu", channels=3, timesteps=T, kernel_std=std, kernel_size=ks,
                                      blur_routine=routine, sampling_routine=sampling)
            x = images(2, 3, 16, g)
            with torch.no_grad(), quiet():
                F1, B1, i1 = d.forward_and_backward(batch_size=2, img=x)
                F2, Ba, Bb, ia, ib = d.forward_and_backward_2(batch_size=2, img=x)
                half = x
                for i in range(2):
                    half = d.gaussian_kernels[i](half)
                xt, direct, i3 = d.sample_from_blur(batch_size=2, img=half, start=2)
                X0, Xt = d.all_sample(batch_size=2, img=x, times=3)
            out[f"deblur/{routine}/{sampling}"] = dict(
                T=T, ks=ks, std=std, x=x, fab=(cpu(F1), cpu(B1), i1), fab2=(cpu(F2), cpu(Ba), cpu(Bb), ia, ib), half=half,
                from_blur=(xt, direct, i3), all_sample=(cpu(X0), cpu(Xt)),
                kernels=[m.weight.detach().clone() for m in d.gaussian_kernels], modes=[m.padding_mode for m in d.gaussian_kernels])
    # ---- denoising: forward_and_backward (its randn_like draw replayed from the same seed) -----------------
    ref = ref_shim.load("denoising")
    d = ref.GaussianDiffusion(net, image_size=16, channels=3, timesteps=5, sampling_routine="x0_step_down")
    x = images(2, 3, 16, g)
    torch.manual_seed(SEED + 2)
    noise = torch.randn_like(x)
    torch.manual_seed(SEED + 2)
    with torch.no_grad(), quiet():
        F1, B1, i1 = d.forward_and_backward(batch_size=2, img=x)
    out["denoise/fab"] = dict(T=5, x=x, noise=noise, fab=(cpu(F1), cpu(B1), i1))
    # ---- resolution: all_sample, forward_and_backward, gen_sample(times), train routines ------------------
    ref = ref_shim.load("resolution")
    for routine in ("Incremental_factor_2", "Incremental_area_factor_2"):
        for sampling in ("default", "x0_step_down"):
            T = 3
            d = ref.GaussianDiffusion(net, image_size=16, device_of_kernel="cpu", channels=3, timesteps=T, resolution_routine=routine,
                                      sampling_routine=sampling)
            x = images(2, 3, 16, g)
            with torch.no_grad(), quiet():
                X0, Xt = d.all_sample(batch_size=2, img=x)
                F1, B1, i1 = d.forward_and_backward(batch_size=2, img=x)
                gs = d.gen_sample(batch_size=2, img=x, times=2)
            out[f"resolution/{routine}/{sampling}"] = dict(T=T, x=x, all_sample=(cpu(X0), cpu(Xt)), fab=(cpu(F1), cpu(B1), i1), gen_times2=gs)
    x, t = images(3, 3, 16, g), torch.tensor([1, 0, 2])
    for tr in ("Final", "Final_small_noise", "Final_random_mean", "Final_random_mean_and_actual", "Step"):
        for loss_type in ("l1", "l2"):
            d = ref.GaussianDiffusion(net, image_size=16, device_of_kernel="cpu", channels=3, timesteps=3, loss_type=loss_type,
                                      resolution_routine="Incremental_factor_2", train_routine=tr)
            torch.manual_seed(SEED + 3)
            noise, _ = torch.randn_like(x), torch.manual_seed(SEED + 3)
            new_mean, _ = torch.randn_like(x.mean((2, 3))), torch.manual_seed(SEED + 3)
            net.zero_grad()
            loss = d.p_losses(x, t)
            loss.backward()
            out[f"resolution/train/{tr}/{loss_type}"] = dict(x=x, t=t, noise=noise, new_mean=new_mean, loss=loss.detach().clone(),
                                                             grads=({k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
                                                                    if loss_type == "l1" else None))
    return out


def mixing_cases(net_sd):
    """The forward(x1, x2) packages: demixing and defading generation."""
    import contextlib
    import io
    out = {}
    g = torch.Generator().manual_seed(SEED + 5)
    cpu = lambda L: [z.clone() for z in L]
    quiet = lambda: contextlib.redirect_stdout(io.StringIO())
    # ---- demixing ------------------------------------------------------------------------------------------
    ref = ref_shim.load("demixing")
    net = ref.Unet(dim=8, dim_mults=(1, 2), channels=3)
    net.load_state_dict(net_sd)
    d = ref.GaussianDiffusion(net, image_size=16, channels=3, timesteps=5)
    x1, x2, t = images(2, 3, 16, g), images(2, 3, 16, g), torch.tensor([4, 1])
    with torch.no_grad(), quiet():
        q = d.q_sample(x1, x2, t)
        gen = d.gen_sample(batch_size=2, img=x2, noise_level=0)
        smp = d.sample(batch_size=2, img=x2)
        F1, B1, i1 = d.forward_and_backward(batch_size=2, img1=x1, img2=x2)
        X0, Xt = d.all_sample(batch_size=2, img=x2)
    net.zero_grad()
    loss = d.p_losses(x1, x2, t)
    loss.backward()
    out["demix"] = dict(T=5, x1=x1, x2=x2, t=t, q=q, gen=gen, sample=smp, fab=(cpu(F1), cpu(B1), i1), all_sample=(cpu(X0), cpu(Xt)),
                        loss=loss.detach().clone(), grads={k: p.grad.clone() for k, p in net.named_parameters()})
    # ---- defading generation -----------------------------------------------------------------------------------
    ref = ref_shim.load("defading_generation")
    net = ref.Unet(dim=8, dim_mults=(1, 2), channels=3)
    net.load_state_dict(net_sd)
    for reverse in (False, True):
        d = ref.GaussianDiffusion(net, image_size=16, channels=3, timesteps=5, reverse=reverse, kernel_std=0.3, initial_mask=2)
        x1 = images(2, 3, 16, g)
        x2 = (torch.rand((2, 3), generator=g) - 0.5)[:, :, None, None].expand(2, 3, 16, 16).contiguous()
        t = torch.tensor([3, 0])
        with torch.no_grad(), quiet():
            q = d.q_sample(x1, x2, t)
            smp = d.sample(batch_size=2, img=x2)
            gen = d.gen_sample(batch_size=2, img=x2, noise_level=0)
            F1, B1, i1 = d.forward_and_backward(batch_size=2, img1=x1, img2=x2)
            X0, Xt = d.all_sample(batch_size=2, img=x2)
        net.zero_grad()
        loss = d.p_losses(x1, x2, t)
        loss.backward()
        out[f"defgen/{int(reverse)}"] = dict(T=5, kernel_std=0.3, initial_mask=2, x1=x1, x2=x2, t=t, alphas=d.alphas.clone(),
                                             one_minus=d.one_minus_alphas.clone(), q=q, sample=smp, gen=gen, fab=(cpu(F1), cpu(B1), i1),
                                             all_sample=(cpu(X0), cpu(Xt)), loss=loss.detach().clone(),
                                             grads={k: p.grad.clone() for k, p in net.named_parameters()} if not reverse else None)
    return out


def extra_cases(net_sd):
    """Branches round 1 only checked against the oracle (VERDICT r1 weak #4 iv): `discrete=True` (DEBLUR:413-415, 441-444,
    937-940, 954-958), blur_routine 'Individual_Incremental' (DEBLUR:380-383, 402-403, 427-428), defade 'Constant' and
    'Random_Incremental' with the RNG seeded so that the crop offsets can be replayed (DEFADE:343-350, 359-368, 501-516)."""
    import contextlib
    import io
    out = {}
    g = torch.Generator().manual_seed(SEED + 9)
    quiet = lambda: contextlib.redirect_stdout(io.StringIO())
    ref = ref_shim.load("deblurring")
    net = ref.Unet(dim=8, dim_mults=(1, 2), channels=3)
    net.load_state_dict(net_sd)
    for routine, ks, std, discrete in (("Constant", 5, 1.0, True), ("Exponential_reflect", 5, 0.2, True), ("Individual_Incremental", 0, 0, False)):
        for sampling in ("default", "x0_step_down"):
            T = 4
            d = ref.GaussianDiffusion(net, image_size=16, device_of_kernel="cpu", channels=3, timesteps=T, kernel_std=std, kernel_size=ks,
                                      blur_routine=routine, sampling_routine=sampling, discrete=discrete)
            x, t = images(3, 3, 16, g), torch.tensor([0, 3, 2])
            with torch.no_grad(), quiet():
                xq = d.q_sample(x, t)
                xt, direct, img = d.sample(batch_size=3, img=x)
            out[f"deblur/{routine}/{sampling}"] = dict(T=T, ks=ks, std=std, discrete=discrete, x=x, t=t, q=xq, xt=xt, direct=direct, img=img,
                                                       kernels=[m.weight.detach().clone() for m in d.gaussian_kernels])
    ref = ref_shim.load("defading")
    for routine, discrete in (("Constant", False), ("Random_Incremental", False), ("Random_Incremental", True)):
        for sampling in ("default", "x0_step_down"):
            T = 4
            d = ref.GaussianDiffusion(net, image_size=16, device_of_kernel="cpu", channels=3, timesteps=T, kernel_std=0.5, initial_mask=1,
                                      fade_routine=routine, sampling_routine=sampling, discrete=discrete)
            x, t = images(3, 3, 16, g), torch.tensor([3, 0, 2])
            offs = {}
            for what in ("q", "sample"):
                torch.manual_seed(SEED + 11)                            # replay the two randint draws (DEFADE:501-502 / 359-360)
                offs[what] = (torch.randint(0, 17, (3,)), torch.randint(0, 17, (3,)))
            assert all(torch.equal(a, b) for a, b in zip(offs["q"], offs["sample"]))
            with torch.no_grad(), quiet():
                torch.manual_seed(SEED + 11)
                xq = d.q_sample(x, t)
                torch.manual_seed(SEED + 11)
                xt, direct, img = d.sample(batch_size=3, faded_recon_sample=x)
            out[f"defade/{routine}/{int(discrete)}/{sampling}"] = dict(T=T, x=x, t=t, q=xq, xt=xt, direct=direct, img=img, masks=d.fade_kernels.clone(),
                                                                      rand_x=offs["q"][0], rand_y=offs["q"][1])
    ref = ref_shim.load("resolution")                                   # the *_with_blur routines (RESOL:354-385, 399-404)
    for routine in ("Incremental_bicubic_with_blur", "Incremental_area_with_blur"):
        T = 3
        d = ref.GaussianDiffusion(net, image_size=16, device_of_kernel="cpu", channels=3, timesteps=T, resolution_routine=routine,
                                  sampling_routine="x0_step_down")
        x, t = images(3, 3, 16, g), torch.tensor([0, 2, 1])
        with torch.no_grad(), quiet():
            xq = d.q_sample(x, t)
            xt, direct, img = d.sample(batch_size=3, img=x)
        out[f"resolution/{routine}"] = dict(T=T, x=x, t=t, q=xq, xt=xt, img=img)
    return out


def fullsize_cases(net_sd):
    """Defading 'Random_Incremental' (+- discrete) at the 128 x 128 size of BASELINE config 5 with the README's schedule
    (README.md:125-126: T = 50, kernel_std 0.1, initial_mask 1): q_sample and a six-step `sample(t=6)` of the UNMODIFIED reference
    with its two randint draws replayed (DEFADE:359-368, 496-516).  Images come from the seeded generator (stored as uint8 levels)."""
    import contextlib
    import io
    out = {}
    g = torch.Generator().manual_seed(SEED + 21)
    ref = ref_shim.load("deblurring")
    net = ref.Unet(dim=8, dim_mults=(1, 2), channels=3)
    net.load_state_dict(net_sd)
    ref = ref_shim.load("defading")
    S, T, B = 128, 50, 2
    for discrete in (False, True):
        d = ref.GaussianDiffusion(net, image_size=S, device_of_kernel="cpu", channels=3, timesteps=T, kernel_std=0.1, initial_mask=1,
                                  fade_routine="Random_Incremental", sampling_routine="x0_step_down", discrete=discrete)
        lv = torch.randint(0, 256, (B, 3, S, S), generator=g)
        x, t = lv.float() / 255 * 2 - 1, torch.tensor([T - 1, 17])
        torch.manual_seed(SEED + 23)
        rx, ry = torch.randint(0, S + 1, (B,)), torch.randint(0, S + 1, (B,))
        with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
            torch.manual_seed(SEED + 23)
            xq = d.q_sample(x, t)
            torch.manual_seed(SEED + 23)
            xt, direct, img = d.sample(batch_size=B, faded_recon_sample=x, t=6)
        out[f"defade128/Random_Incremental/{int(discrete)}"] = dict(T=T, levels=lv.to(torch.uint8), t=t, q=xq, xt=xt, direct=direct, img=img,
                                                                    rand_x=rx, rand_y=ry, kernel_std=0.1, initial_mask=1, sample_t=6)
    # The masks are 1 - k / max(k) with k = g g^T, g the normalised 1-D Gaussian whose taps come from torch.exp -- which is NOT
    # correctly rounded and differs by an ulp between CPU vector ISAs (the GPU box's host gave other masks than this container, and with
    # them 230 of 98304 q values one or two ulps away).  The fixture therefore carries the reference's OWN 1-D Gaussians (50 x 257
    # floats; everything after the exp is exactly rounded IEEE arithmetic, so the [50, 257, 257] table is rebuilt bit-exactly from them).
    g1 = torch.stack([ref_shim.gaussian_1d(2 * S + 1, 0.1 * (i + 1)) for i in range(T)])
    assert torch.equal(masks_from_g1(g1), d.fade_kernels)
    out["defade128/g1d"] = g1
    return out


def masks_from_g1(g1):
    """[T, n] normalised 1-D Gaussians -> the fade masks of DEFADE:328-352: (1 - g g^T / max(g g^T))[1:, 1:] per step."""
    ks = []
    for g in g1:
        k = torch.matmul(g.unsqueeze(-1), g.unsqueeze(-1).t())
        ks.append((torch.ones_like(k) - k / torch.max(k))[1:, 1:])
    return torch.stack(ks)


def ssim_msssim(X, Y, data_range=1.0, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03)):
    """pytorch_msssim 0.2.x `ssim` restated with torch ops (the package is not installed; the reference imports it at DEBLUR:1570):
    _fspecial_gauss_1d, gaussian_filter = grouped 'valid' conv along H then W, _ssim.  Third-party, unpinned upstream."""
    import torch.nn.functional as F
    coords = torch.arange(win_size, dtype=torch.float32) - win_size // 2
    g = torch.exp(-(coords ** 2) / (2 * win_sigma ** 2))
    g = g / g.sum()
    C = X.shape[1]

    def filt(z):
        z = F.conv2d(z, g.view(1, 1, -1, 1).repeat(C, 1, 1, 1), groups=C)
        return F.conv2d(z, g.view(1, 1, 1, -1).repeat(C, 1, 1, 1), groups=C)

    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mu1, mu2 = filt(X), filt(Y)
    s1, s2, s12 = filt(X * X) - mu1 * mu1, filt(Y * Y) - mu2 * mu2, filt(X * Y) - mu1 * mu2
    m = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * ((2 * s12 + C2) / (s1 + s2 + C2))
    per = m.flatten(2).mean(-1)
    return per.mean() if size_average else per.mean(1)


def evaluation_cases(net_sd):
    """The deterministic parts of the reference Trainer's evaluation methods, captured by
    running the UNMODIFIED methods on a reference Trainer object whose dataset is a fixed in-memory list of images:
      * sample_as_a_mean_blur_torch_gmm_ablation (DEBLUR:1391-1456): the channel-mean matrix handed to the GMM's fit()
      * sample_as_a_blur_torch_gmm (DEBLUR:1514-1564): the opt()-feature matrix handed to fit(), and -- with the GMM's sample() fixed --
        the og / xt / direct_recons / recon images it saves
      * fid_distance_decrease_from_manifold (DEBLUR:1567-1702): the four image sets handed to fid_func and to ssim, and the RMSE / SSIM
        numbers it prints (SSIM through the restatement of pytorch_msssim above)
    Harness notes: the GMM (pycave upstream) is a capturing stand-in; `pdb.set_trace()` (DEBLUR:1420) is a no-op; `utils.save_image`
    captures; `torch.cuda.FloatTensor` is torch.FloatTensor on this CPU-only box; and F.interpolate's hard-coded `size=128`
    (DEBLUR:1546: CelebA's image size) is mapped to this case's image_size 16 -- a 128 x 128 fixture set would be 20 MB."""
    import contextlib
    import io
    import pathlib
    import pdb
    import tempfile
    import types
    out = {}
    ref = ref_shim.load("deblurring")
    mod = ref_shim.submodule(ref, ref.Trainer.__module__)
    S, T = 16, 3
    g = torch.Generator().manual_seed(SEED + 21)
    imgs = images(104, 3, S, g)                                   # 104 images: one DataLoader batch of 100 (drop_last) + 4 dropped
    net = ref.Unet(dim=8, dim_mults=(1, 2), channels=3)
    net.load_state_dict(net_sd)
    d = ref.GaussianDiffusion(net, image_size=S, device_of_kernel="cpu", channels=3, timesteps=T, kernel_std=0.5, kernel_size=3,
                              blur_routine="Incremental", sampling_routine="x0_step_down")
    out["cfg"] = dict(image_size=S, T=T, kernel_std=0.5, kernel_size=3, blur_routine="Incremental", sampling_routine="x0_step_down")
    out["images"] = imgs
    out["kernels"] = [m.weight.detach().clone() for m in d.gaussian_kernels]

    class ListDS(torch.utils.data.Dataset):
        def __len__(self):
            return imgs.shape[0]

        def __getitem__(self, i):
            return imgs[i]

    tr = object.__new__(ref.Trainer)
    tr.ds, tr.batch_size, tr.image_size = ListDS(), 4, S
    tr.ema_model = types.SimpleNamespace(module=d)
    tmp = tempfile.mkdtemp()
    tr.results_folder = pathlib.Path(tmp) / "res"

    saved = []
    F_real = mod.F

    class FProxy:
        def __getattr__(self, k):
            return getattr(F_real, k)

        @staticmethod
        def interpolate(x, size=None, **kw):
            return F_real.interpolate(x, size=S if size == 128 else size, **kw)

    class Stop(Exception):
        pass

    fixed = {}

    class CaptureGMM:
        last_fit = None

        def __init__(self, **kw):
            self.kw = kw

        def fit(self, x):
            CaptureGMM.last_fit = x.detach().clone()
            if fixed.get("stop"):
                raise Stop()

        def sample(self, num_datapoints):
            return fixed["og_x"][:num_datapoints].clone()

        def get_params(self):
            return {}

    old = (mod.F, mod.utils.save_image, pdb.set_trace, torch.cuda.FloatTensor, sys.modules["pytorch_msssim"].ssim, mod.create_folder)
    mod.F = FProxy()
    mod.utils.save_image = lambda t, path, **kw: saved.append((os.path.basename(str(path)), t.detach().clone()))
    pdb.set_trace = lambda *a, **k: None
    torch.cuda.FloatTensor = torch.FloatTensor
    ssim_calls = []

    def ssim_capture(X, Y, **kw):
        v = ssim_msssim(X, Y, **kw)
        ssim_calls.append(v.clone())
        return v

    sys.modules["pytorch_msssim"].ssim = ssim_capture
    mod.create_folder = lambda p: None
    quiet = contextlib.redirect_stdout(io.StringIO())
    try:
        with torch.no_grad(), quiet:
            # -- channel means (the ablation sampler stops at fit: its 6400-sample loop at 128 x 128 is not run) ------------
            fixed["stop"] = True
            try:
                tr.sample_as_a_mean_blur_torch_gmm_ablation(CaptureGMM, ch=3, clusters=2, noise=0)
            except Stop:
                pass
            out["channel_means"] = CaptureGMM.last_fit
            # -- opt features + sample_from_blur with a fixed GMM sample -----------------------------------------------
            fixed["stop"] = False
            siz, sample_at = 4, 1
            fixed["og_x"] = torch.randn(48, 3 * siz * siz, generator=g) * 0.3
            saved.clear()
            tr.sample_as_a_blur_torch_gmm(CaptureGMM, siz=siz, ch=3, clusters=2, sample_at=sample_at)
            out["blur_gmm"] = dict(siz=siz, sample_at=sample_at, clusters=2, feats=CaptureGMM.last_fit, og_x=fixed["og_x"],
                                   saved={name.split("-")[1]: t for name, t in saved})
            # -- the metric sweep ------------------------------------------------------------------------------------
            fid_calls = []

            def fid_func(samples):
                fid_calls.append([z.clone() for z in samples])
                return float(len(fid_calls))

            saved.clear()
            cwd = os.getcwd()
            os.chdir(tmp)                                                # (the method writes ./sanity_check/)
            try:
                tr.fid_distance_decrease_from_manifold(fid_func, start=0, end=40)
            finally:
                os.chdir(cwd)
            orig = fid_calls[0][0]
            sets = dict(orig=orig, blur=fid_calls[0][1], deblur=fid_calls[1][1], direct_deblur=fid_calls[2][1])
            out["sweep"] = dict(start=0, end=40, sets=sets,
                                rmse={k: torch.sqrt(torch.mean((orig - sets[k]) ** 2)) for k in ("blur", "deblur", "direct_deblur")},
                                ssim=dict(zip(("blur", "deblur", "direct_deblur"), ssim_calls)))
    finally:
        mod.F, mod.utils.save_image, pdb.set_trace, torch.cuda.FloatTensor, sys.modules["pytorch_msssim"].ssim, mod.create_folder = old
    return out


def sampler_cases():
    """The reference side of tests/test_oracle.py::test_oracle_vs_live_reference_degradations_and_samplers, same seeds and calls:
    q_sample + sample of the four packages at 24 x 24 with a Unet(dim=8, (1, 2)) -> live_samplers.pt.  Kept small: the seeded
    weights are stored as their sd_digest (the test redraws them), every output the test compares bit for bit as its tensor_digest,
    and only the network outputs it compares to a tolerance as values, each distinct tensor once."""
    import contextlib
    import io
    S, B = 24, 2
    g = torch.Generator().manual_seed(4242)
    x = torch.randint(0, 256, (B, 3, S, S), generator=g).float() / 255 * 2 - 1
    quiet = lambda: contextlib.redirect_stdout(io.StringIO())
    shared = {}
    keep = lambda t: shared.setdefault(tensor_digest(t), t.clone())      # (the same object -> torch.save stores it once)
    walk = lambda r: [tensor_digest(r[0]), keep(r[1]), keep(r[2])]       # (x_t or the start: exact; direct, img: values)
    ref = ref_shim.load("deblurring")
    torch.manual_seed(99)
    with quiet():
        rnet = ref.Unet(dim=8, dim_mults=(1, 2), channels=3)
    out = {"x": x, "sd_sha256": sd_digest(rnet.state_dict())}
    with torch.no_grad(), quiet():
        for routine, ks, std in (("Incremental", 5, 0.3), ("Exponential_reflect", 7, 0.05)):
            for sampling in ("default", "x0_step_down"):
                T, t = 6, torch.tensor([5, 2])
                d = ref.GaussianDiffusion(rnet, image_size=S, device_of_kernel="cpu", channels=3, timesteps=T, kernel_std=std, kernel_size=ks,
                                          blur_routine=routine, sampling_routine=sampling)
                ws = [keep(m.weight.detach()) for m in d.gaussian_kernels]
                modes = [m.padding_mode for m in d.gaussian_kernels]
                out[f"blur/{routine}/{sampling}"] = dict(T=T, t=t, ws=ws, modes=modes, q=tensor_digest(d.q_sample(x, t)),
                                                         sample=walk(d.sample(batch_size=B, img=x)))
        ref = ref_shim.load("denoising")
        T, t = 7, torch.tensor([6, 1])
        e = torch.randn(B, 3, S, S, generator=g)
        out["noise/e"] = e
        for sampling in ("x0_step_down", "ddim"):
            d = ref.GaussianDiffusion(rnet, image_size=S, channels=3, timesteps=T, sampling_routine=sampling)
            out[f"noise/{sampling}"] = dict(T=T, t=t, q=tensor_digest(d.q_sample(x, e, t)), gen=walk(d.gen_sample(batch_size=B, img=e)),
                                            sample=walk(d.sample(batch_size=B, img=e)), ca=d.sqrt_alphas_cumprod.clone(),
                                            cb=d.sqrt_one_minus_alphas_cumprod.clone())
        ref = ref_shim.load("resolution")
        for routine, mode in (("Incremental", "bicubic"), ("Incremental_area_factor_2", "area")):
            T, t = 3, torch.tensor([2, 0])
            d = ref.GaussianDiffusion(rnet, image_size=S, device_of_kernel="cpu", channels=3, timesteps=T, resolution_routine=routine,
                                      sampling_routine="x0_step_down")
            out[f"resolution/{routine}"] = dict(T=T, t=t, mode=mode, q=tensor_digest(d.q_sample(x, t)), sample=walk(d.sample(batch_size=B, img=x)))
        ref = ref_shim.load("defading")
        for routine in ("Incremental", "Constant"):
            for sampling in ("default", "x0_step_down"):
                T, t = 5, torch.tensor([4, 1])
                d = ref.GaussianDiffusion(rnet, image_size=S, device_of_kernel="cpu", channels=3, timesteps=T, kernel_std=0.4, initial_mask=2,
                                          fade_routine=routine, sampling_routine=sampling)
                out[f"fade/{routine}/{sampling}"] = dict(T=T, t=t, masks=keep(d.fade_kernels), q=tensor_digest(d.q_sample(x, t)),
                                                         sample=walk(d.sample(batch_size=B, faded_recon_sample=x)))
    return out


def tensor_digest(t):
    """sha256 over a tensor's dtype, shape and bytes: equal digests <=> torch.equal (and the same dtype)."""
    import hashlib
    t = t.detach().cpu().contiguous()
    h = hashlib.sha256(("%s %s;" % (t.dtype, tuple(t.shape))).encode())
    h.update(t.numpy().tobytes())
    return h.hexdigest()


def bitexact_cases():
    """The reference side of tests/test_oracle.py::test_oracle_bit_exact_vs_live_reference, same seeds and calls: a Unet(dim=8,
    (1, 2, 4, 8), channels=1) at 32 x 32 and a Model(ch=32, (1, 2, 2), 2 res blocks, attention at 8) at 16 x 16 -> live_bitexact.pt.
    The 10 MB of seeded initial weights are not stored, only their sd_digest: the test redraws them from the same seed."""
    ref = ref_shim.load("deblurring")
    torch.manual_seed(7)
    net = ref.Unet(dim=8, dim_mults=(1, 2, 4, 8), channels=1)
    x, t = torch.randn(2, 1, 32, 32), torch.tensor([5, 11])
    with torch.no_grad():
        unet = dict(sd_sha256=sd_digest(net.state_dict()), x=x, t=t, y=net(x, t))
    m = ref.Model(resolution=16, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 2, 2), num_res_blocks=2, attn_resolutions=(8,), dropout=0.1).eval()
    x = torch.randn(2, 3, 16, 16)
    with torch.no_grad():
        model = dict(sd_sha256=sd_digest(m.state_dict()), x=x, t=t, y=m(x, t))
    return {"unet": unet, "model": model}


def sd_digest(sd):
    """sha256 over a state dict's names, dtypes, shapes and bytes, in its order."""
    import hashlib
    h = hashlib.sha256()
    for k, v in sd.items():
        v = v.detach().cpu().contiguous()
        h.update(("%s %s %s;" % (k, v.dtype, tuple(v.shape))).encode())
        h.update(v.numpy().tobytes())
    return h.hexdigest()


# the classes tests/test_boundary.py compares, per reference package (ref_shim name)
SIGNATURE_CLASSES = {
    "deblurring": ("Unet", "Model", "GaussianDiffusion", "Trainer"),
    "denoising": ("Unet", "GaussianDiffusion", "Trainer"),
    "resolution": ("Unet", "Model", "GaussianDiffusion", "Trainer"),
    "defading": ("Unet", "Model", "GaussianDiffusion", "Trainer"),
    "demixing": ("Unet", "GaussianDiffusion", "Trainer"),
    "defading_generation": ("Unet", "GaussianDiffusion", "Trainer"),
}


def own_methods(cls):
    """public callables the class itself (not nn.Module / object) defines, plus __init__ and forward"""
    out = {}
    for klass in cls.__mro__:
        if klass.__module__.startswith("torch") or klass is object:
            continue
        for name, v in vars(klass).items():
            if callable(v) and (not name.startswith("_") or name == "__init__") and name not in out:
                out[name] = v
    return out


def signature_params(fn):
    """[[name, kind, default]] of a callable: kind = inspect.Parameter kind name, default = repr() of it, None when there is none."""
    import inspect
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


def signature_case(which):
    """{class: {method: [[name, kind, default repr]]}} of every public method one reference package defines on its exported classes."""
    ref = ref_shim.load(which)
    return {c: {m: signature_params(fn) for m, fn in sorted(own_methods(getattr(ref, c)).items())} for c in SIGNATURE_CLASSES[which]}


def signature_cases():
    """signature_case() of every package tests/test_boundary.py compares -> reference_signatures.json."""
    return {which: signature_case(which) for which in SIGNATURE_CLASSES}



def write_live_cases():
    """The fixtures that let the live-reference tests run where the reference tree is absent."""
    import json
    torch.save(sampler_cases(), os.path.join(HERE, "live_samplers.pt"))
    torch.save(bitexact_cases(), os.path.join(HERE, "live_bitexact.pt"))
    with open(os.path.join(HERE, "reference_signatures.json"), "w") as f:
        json.dump(signature_cases(), f, indent=1, sort_keys=True)
        f.write("\n")
    for f in ("live_samplers.pt", "live_bitexact.pt", "reference_signatures.json"):
        print(f, os.path.getsize(os.path.join(HERE, f)) // 1024, "KiB")


def main():
    assert ref_shim.available(), "needs /root/reference (build container)"
    if "--live" in sys.argv:                                          # only (re)write live_samplers.pt, live_bitexact.pt, reference_signatures.json
        write_live_cases()
        return
    if "--mixing" in sys.argv:                                        # only (re)write mixing.pt
        sd = torch.load(os.path.join(HERE, "diffusion.pt"), weights_only=False)["deblur/net_sd"]
        torch.save(mixing_cases(sd), os.path.join(HERE, "mixing.pt"))
        print("mixing.pt", os.path.getsize(os.path.join(HERE, "mixing.pt")) // 1024, "KiB")
        return
    if "--extras" in sys.argv:                                        # only (re)write extras.pt
        sd = torch.load(os.path.join(HERE, "diffusion.pt"), weights_only=False)["deblur/net_sd"]
        torch.save(extra_cases(sd), os.path.join(HERE, "extras.pt"))
        print("extras.pt", os.path.getsize(os.path.join(HERE, "extras.pt")) // 1024, "KiB")
        return
    if "--model-noconv" in sys.argv:                                  # only (re)write model_noconv.pt: Model(resamp_with_conv=False), MODEL2:36-73
        torch.save(model_case(ref_shim.load("deblurring"), resamp_with_conv=False), os.path.join(HERE, "model_noconv.pt"))
        print("model_noconv.pt", os.path.getsize(os.path.join(HERE, "model_noconv.pt")) // 1024, "KiB")
        return
    if "--fullsize" in sys.argv:                                      # only (re)write fullsize.pt
        sd = torch.load(os.path.join(HERE, "diffusion.pt"), weights_only=False)["deblur/net_sd"]
        torch.save(fullsize_cases(sd), os.path.join(HERE, "fullsize.pt"))
        print("fullsize.pt", os.path.getsize(os.path.join(HERE, "fullsize.pt")) // 1024, "KiB")
        return
    if "--evaluation" in sys.argv:                                    # only (re)write evaluation.pt
        sd = torch.load(os.path.join(HERE, "diffusion.pt"), weights_only=False)["deblur/net_sd"]
        torch.save(evaluation_cases(sd), os.path.join(HERE, "evaluation.pt"))
        print("evaluation.pt", os.path.getsize(os.path.join(HERE, "evaluation.pt")) // 1024, "KiB")
        return
    if "--variants" in sys.argv:                                      # only (re)write variants.pt
        sd = torch.load(os.path.join(HERE, "diffusion.pt"), weights_only=False)["deblur/net_sd"]
        torch.save(variant_cases(sd), os.path.join(HERE, "variants.pt"))
        print("variants.pt", os.path.getsize(os.path.join(HERE, "variants.pt")) // 1024, "KiB")
        return
    ref = ref_shim.load("deblurring")
    torch.save(unet_case(ref), os.path.join(HERE, "unet_dim8.pt"))
    torch.save(model_case(ref), os.path.join(HERE, "model_ch32.pt"))
    torch.save(model_case(ref, resamp_with_conv=False), os.path.join(HERE, "model_noconv.pt"))
    dc = diffusion_cases()
    torch.save(dc, os.path.join(HERE, "diffusion.pt"))
    torch.save(variant_cases(dc["deblur/net_sd"]), os.path.join(HERE, "variants.pt"))
    torch.save(mixing_cases(dc["deblur/net_sd"]), os.path.join(HERE, "mixing.pt"))
    torch.save(extra_cases(dc["deblur/net_sd"]), os.path.join(HERE, "extras.pt"))
    torch.save(evaluation_cases(dc["deblur/net_sd"]), os.path.join(HERE, "evaluation.pt"))
    torch.save(fullsize_cases(dc["deblur/net_sd"]), os.path.join(HERE, "fullsize.pt"))
    write_live_cases()
    # torchgeometry boundary: values observed when the reference builds its kernels through the shim
    k = ref_shim.get_gaussian_kernel2d((11, 11), (7.0, 7.0))
    print("k=11 sigma=7 centre %.10f corner %.10f" % (k[5, 5].item(), k[0, 0].item()))
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".pt"):
            print(f, os.path.getsize(os.path.join(HERE, f)) // 1024, "KiB")


if __name__ == "__main__":
    main()
