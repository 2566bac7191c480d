"""Round-2 hardware parity cases: the configurations and kernel selections the bench / the
BASELINE configs actually run, checked against the CPU oracle on the MI355X.

  * cfg1 network `Unet(dim=64, channels=1)` at 32x32 (mnist_train.py:64-92)
  * the BENCH shape: the fused 2 x 32-image, 128x128 pass of one optimizer step (Trainer._fused_step), loss + every gradient
  * bicubic / bilinear `Incremental_factor_2` pixelation at 128x128 against ATen (RESOL:371-372)
  * split-precision (bf16x3) GEMMs on wide-dynamic-range operands, and the other arithmetic modes at module level
  * multi-step sampler drift on a real net (T=50, 32x32)
  * the gradient-exchange engine on one rank over RCCL
"""
import contextlib
import io
import os
import socket

import pytest
import torch

from oracle import cold_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _grad_check(net, ref_grads, tol=1e-3, floor=1e-2):
    gmax = max(g.abs().max().item() for g in ref_grads.values())
    worst = 0.0
    for name, p in net.named_parameters():
        r = ref_grads[name]
        e = (p.grad.cpu() - r).abs().max().item()
        lim = tol * max(r.abs().max().item(), floor * gmax)
        worst = max(worst, e / lim)
        assert e <= lim, (name, e, r.abs().max().item())
    return worst


def test_cfg1_unet_one_channel_32():
    """BASELINE config 1 network: Unet(dim=64, (1,2,4,8), channels=1) on 32x32 images, forward + backward."""
    from deblurring_diffusion_pytorch import Unet
    torch.manual_seed(123457)
    net = quiet(Unet, dim=64, dim_mults=(1, 2, 4, 8), channels=1)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x = torch.randint(0, 256, (8, 1, 32, 32)).float() / 255 * 2 - 1
    t = torch.tensor([0, 19, 3, 7, 11, 1, 18, 5])
    gy = torch.randn(8, 1, 32, 32) / 1000
    net = net.to(DEV)
    y = net(x.to(DEV), t.to(DEV))
    y.backward(gy.to(DEV))
    ps = {k: v.clone().requires_grad_() for k, v in sd.items()}
    yr = O.unet_forward(ps, x, t)
    yr.backward(gy)
    assert (y.cpu() - yr.detach()).abs().max().item() <= 1e-4
    _grad_check(net, {k: v.grad for k, v in ps.items()})


BENCH_B, BENCH_ACC, BENCH_T = 32, 2, 200     # bench.py's optimizer step: gradient_accumulate_every = 2 micro-batches of 32 images


def bench_step_inputs():
    """The state and the data / noise / t draws of the bench-shape step (shared by the oracle comparison here and the run-to-run
    invariance tests of test_gpu_invariance.py)."""
    from denoising_diffusion_pytorch import Unet
    torch.manual_seed(123457)
    net = quiet(Unet, dim=64, dim_mults=(1, 2, 4, 8), channels=3)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(123457)
    n = BENCH_B * BENCH_ACC
    x = torch.randint(0, 256, (n, 3, 128, 128), generator=g).float() / 255 * 2 - 1
    e = torch.randn(n, 3, 128, 128, generator=g)
    t = torch.randint(0, BENCH_T, (n,), generator=g)
    return {"sd": sd, "x": x, "e": e, "t": t}


@pytest.fixture(scope="module")
def bench_step_oracle():
    """The oracle side of the step bench.py times, computed ONCE for the bf16x3 and the bf16 test (a thread, so the CPU works while
    the MI355X does): the reference's optimizer-step semantics (DEBLUR:1188-1195) -- two micro-batches of 32, (loss_i / 2).backward()
    each -- i.e. loss = mean of the two micro-batch losses, gradient = the sum of both backward passes; 16 chunks of 4 images
    (gradients of a mean are additive over samples)."""
    from concurrent.futures import ThreadPoolExecutor
    f = bench_step_inputs()
    sd, x, e, t = f["sd"], f["x"], f["e"], f["t"]

    def run():
        ca, cb = O.cosine_tables(BENCH_T)
        ps = {k: v.clone().requires_grad_() for k, v in sd.items()}
        micro = []
        for m in range(BENCH_ACC):
            tot = 0.0
            for i in range(m * BENCH_B, (m + 1) * BENCH_B, 4):
                s = slice(i, i + 4)
                li = (x[s] - O.unet_forward(ps, O.noise_q_sample(x[s], e[s], t[s], ca, cb), t[s])).abs().sum() / (BENCH_B * 3 * 128 * 128)
                (li / BENCH_ACC).backward()
                tot += li.item()
            micro.append(tot)
        return sum(micro) / BENCH_ACC, {k: v.grad for k, v in ps.items()}

    ex = ThreadPoolExecutor(max_workers=1)
    yield {"sd": sd, "x": x, "e": e, "t": t, "oracle": ex.submit(run)}
    ex.shutdown(wait=True)


def _fused_bench_step(f):
    """One optimizer step's forward / backward through `Trainer._fused_step` -- the ONE 64-image pass bench.py times (tile selection,
    halo_bm, split-K nsplit and the resident grids all depend on M = B H W) -- with the data / noise / t draws replaced by the fixture's."""
    from denoising_diffusion_pytorch import GaussianDiffusion, Trainer, Unet
    net = quiet(Unet, dim=64, dim_mults=(1, 2, 4, 8), channels=3)
    net.load_state_dict(f["sd"])
    diff = GaussianDiffusion(net.to(DEV), image_size=128, channels=3, timesteps=BENCH_T, loss_type='l1').to(DEV)
    tr = quiet(Trainer, diff, None, image_size=128, train_batch_size=BENCH_B, train_lr=2e-5, train_num_steps=1, gradient_accumulate_every=BENCH_ACC,
               dataset="synthetic", results_folder="/tmp/cdf_bench_shape_res")
    assert tr._can_fuse(), "the bench's step must take the fused path"
    xs = iter(f["x"].split(BENCH_B))
    es = iter(f["e"].split(BENCH_B))
    ts = iter(f["t"].split(BENCH_B))
    tr._next_batch = lambda: next(xs).to(DEV)
    tr._second = lambda batch: next(es).to(DEV)
    tr.core._draw_t = lambda x: next(ts).to(DEV)
    loss = tr._fused_step(BENCH_ACC, False)
    torch.cuda.synchronize()
    return tr, net, loss.item()


def test_bench_shape_fused_step_vs_oracle(bench_step_oracle):
    """The pass bench.py times -- Unet128, 2 x 32 images at 128 x 128 as ONE 64-image pass (`Trainer._fused_step`), denoising package:
    q_sample -> UNet -> L1 -> backward -- against the oracle's two separate micro-steps: loss to 2e-5 relative, every gradient."""
    _, net, loss = _fused_bench_step(bench_step_oracle)
    total, grads = bench_step_oracle["oracle"].result()
    worst = _grad_check(net, grads)
    print("bench-shape fused step (B=64): loss", loss, "oracle", total, "rel", abs(loss - total) / abs(total), "worst grad error / limit", worst)
    assert abs(loss - total) <= 2e-5 * abs(total), (loss, total)


@pytest.mark.parametrize("routine,mode", [("Incremental_factor_2", "bicubic"), ("Incremental_bilinear_factor_2", "bilinear")])
def test_interpolating_pixelation_128(routine, mode):
    """cfg5's default degradation at its real size: F.interpolate(mode) down, nearest-exact up, T=4 (128 -> 64/32/16/8)."""
    from resolution_diffusion_pytorch import GaussianDiffusion as RD
    import torch.nn.functional as F
    torch.manual_seed(2)
    B = 16
    x = torch.rand(B, 3, 128, 128) * 2 - 1
    r = RD(torch.nn.Identity(), image_size=128, device_of_kernel="cuda", channels=3, timesteps=4, resolution_routine=routine)
    with torch.no_grad():
        for i in range(4):
            y = r.func[i](x.to(DEV)).cpu()
            ref = F.interpolate(F.interpolate(x, size=128 // 2 ** (i + 1), mode=mode, antialias=False), size=128, mode="nearest-exact")
            assert (y - ref).abs().max().item() <= 1e-5, (i, (y - ref).abs().max().item())
        t = torch.randint(0, 4, (B,))
        t[0], t[1] = 0, 3
        q = r.q_sample(x.to(DEV), t.to(DEV)).cpu()
        sizes = O.pixelate_sizes(routine, 4, 128)
        ref = O.pixelate_q_sample(x, t, sizes, mode)
        assert (q - ref).abs().max().item() <= 2e-5


def test_bf16x3_wide_dynamic_range():
    """Split precision keeps 16 mantissa bits per operand (hi + lo bf16: representation error <= 2^-17 relative) and drops
    a_lo*b_lo (2^-16): per product <= ~2^-15 relative, and the error must stay RELATIVE to the operand scale whatever the
    dynamic range.  Weights x8, inputs x4 and a 900.0 outlier pixel on a conv stack, against an fp64 reference, normalised by
    the output scale.  Bound: 4e-5 of |y|max (measured 2.1e-5; torch's own fp32 path: 7e-7).  Consequence, stated in DESIGN.md:
    the north_star 1e-4 max-abs bound holds for image-scale outputs (|y| <~ 2.5), which is what every parity test checks."""
    from deblurring_diffusion_pytorch import Unet
    from colddiff import runtime as rt
    assert rt.precision == "bf16x3"
    torch.manual_seed(5)
    net = quiet(Unet, dim=64, dim_mults=(1, 2), channels=3)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if p.dim() == 4 and p.shape[-1] == 3:           # the 3x3 convs (the bf16x3 GEMMs): 8x the default init
                p.mul_(8.0)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x = (torch.rand(2, 3, 64, 64) * 2 - 1) * 4
    # a few large outliers: exercises hi/lo splitting of operands 2^10 apart in one dot product
    x[0, :, 5, 7] = 900.0
    t = torch.tensor([3, 17])
    net = net.to(DEV)
    with torch.no_grad():
        y = net(x.to(DEV), t.to(DEV)).cpu()
        torch.set_default_dtype(torch.float64)
        try:
            yr = O.unet_forward({k: v.double() for k, v in sd.items()}, x.double(), t)
        finally:
            torch.set_default_dtype(torch.float32)
        y32 = O.unet_forward(sd, x, t)
    scale = yr.abs().max().item()
    e_hip = (y.double() - yr).abs().max().item() / scale
    e_f32 = (y32.double() - yr).abs().max().item() / scale
    print("wide range: |y|max", scale, "hip rel err", e_hip, "torch fp32 rel err", e_f32)
    assert e_hip <= 4e-5, (e_hip, e_f32)


# bf16 mode (COLDDIFF_PRECISION=bf16: single bf16 GEMM operands, fp32 accumulate / master weights / norms) -- its stated tolerance,
# the SAME numbers bench.py prints in `bf16_mode.tolerance_vs_fp32_oracle`:
from colddiff.runtime import BF16_TOLERANCE  # noqa: E402

BF16_FWD_TOL = BF16_TOLERANCE["forward_max_abs"]           # UNet output, max-abs vs the fp32 oracle (image scale: |y| <~ 2.5)
BF16_GRAD_TOL = BF16_TOLERANCE["grad_rel_of_tensor_max"]   # every gradient tensor: max-abs error / max(its |g|max, 1e-2 of the largest |g|max)
BF16_LOSS_TOL = BF16_TOLERANCE["loss_rel"]                 # micro-step loss, relative


@contextlib.contextmanager
def _precision(mode):
    from colddiff import runtime as rt
    saved = rt.precision
    rt.set_precision(mode)
    rt.bump_weights_epoch()
    try:
        yield
    finally:
        rt.set_precision(saved)
        rt.bump_weights_epoch()


@pytest.mark.parametrize("mode,tol,gtol", [("f32", 1e-4, 1e-3), ("bf16", BF16_FWD_TOL, BF16_GRAD_TOL)])
def test_other_precision_modes_module_level(mode, tol, gtol):
    """COLDDIFF_PRECISION=f32 (exact fp32 MFMA everywhere) must meet the parity bound; =bf16 (single-pass bf16 operands, the mode
    BASELINE configs 3 / 5 name) must stay within its stated tolerance -- forward AND every gradient tensor.  64x64 UNet."""
    from deblurring_diffusion_pytorch import Unet
    with _precision(mode):
        torch.manual_seed(9)
        net = quiet(Unet, dim=64, dim_mults=(1, 2, 4), channels=3)
        sd = {k: v.clone() for k, v in net.state_dict().items()}
        x, t = torch.rand(2, 3, 64, 64) * 2 - 1, torch.tensor([1, 40])
        gy = torch.randn(2, 3, 64, 64) / 1000
        net = net.to(DEV)
        y = net(x.to(DEV), t.to(DEV))
        y.backward(gy.to(DEV))
        ps = {k: v.clone().requires_grad_() for k, v in sd.items()}
        yr = O.unet_forward(ps, x, t)
        yr.backward(gy)
        err = (y.cpu() - yr.detach()).abs().max().item()
        assert err <= tol, err
        worst = _grad_check(net, {k: v.grad for k, v in ps.items()}, tol=gtol)
        print(mode, "forward max-abs error", err, "worst gradient error / limit", worst, "(limit", gtol, ")")


def test_bf16_mode_bench_shape_fused_step(bench_step_oracle):
    """The bf16 line of bench.py at ITS shape: the same fused 64-image pass in COLDDIFF_PRECISION=bf16 against the fp32 oracle:
    loss within BF16_LOSS_TOL relative, every gradient tensor within BF16_GRAD_TOL."""
    with _precision("bf16"):
        _, net, loss = _fused_bench_step(bench_step_oracle)
    total, grads = bench_step_oracle["oracle"].result()
    worst = _grad_check(net, grads, tol=BF16_GRAD_TOL)
    print("bf16 bench-shape fused step (B=64): loss", loss, "oracle", total, "rel", abs(loss - total) / abs(total), "worst grad error / limit", worst)
    assert abs(loss - total) <= BF16_LOSS_TOL * abs(total), (loss, total)


def test_sampler_drift_real_net_T50():
    """Alg. 2 over 50 reverse steps with a real (random-init, dim 64) network at 32x32: the error of a single UNet call must not
    leave the 1e-4 parity bound over the whole trajectory (measured 5e-6) (compared with the oracle's sampler)."""
    from denoising_diffusion_pytorch import GaussianDiffusion, Unet
    torch.manual_seed(11)
    net = quiet(Unet, dim=64, dim_mults=(1, 2, 4, 8), channels=3)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    T = 50
    noise = torch.randn(2, 3, 32, 32)
    d = GaussianDiffusion(net, image_size=32, channels=3, timesteps=T, sampling_routine="x0_step_down").to(DEV)
    with torch.no_grad():
        _, direct, img = quiet(d.gen_sample, batch_size=2, img=noise.to(DEV))
        ca, cb = O.cosine_tables(T)
        _, rdirect, rimg = O.noise_sample(lambda z, s: O.unet_forward(sd, z, s), noise, T, ca, cb, fixed_noise=True)
    e0, e1 = (direct.cpu() - rdirect).abs().max().item(), (img.cpu() - rimg).abs().max().item()
    print("T=50 sampler: first-step error", e0, "final-image error", e1, "|img|max", rimg.abs().max().item())
    assert e0 <= 1e-4 and e1 <= 1e-4


def test_gradsync_single_rank_rccl():
    """The gradient-exchange engine over RCCL on one rank (world_size 1 group): bucket issue, side stream, stream joins.
    A sum all-reduce over one rank is the identity, so the step must equal the plain single-process step bit for bit."""
    import torch.distributed as dist
    from denoising_diffusion_pytorch import GaussianDiffusion, Trainer, Unet
    from colddiff import parallel
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        results = []
        for use_sync in (False, True):
            torch.manual_seed(0)
            net = quiet(Unet, dim=16, dim_mults=(1, 2), channels=3).to(DEV)
            diff = GaussianDiffusion(net, image_size=32, channels=3, timesteps=10).to(DEV)
            tr = Trainer(diff, None, image_size=32, train_batch_size=4, train_lr=1e-3, train_num_steps=2, gradient_accumulate_every=2,
                         dataset="synthetic", results_folder="/tmp/cdf_gradsync_res")
            if use_sync:
                tr.sync = parallel.GradSync(tr.arena, bucket_bytes=64 << 10)
                tr.sync.world = 2                # arm as a multi-rank run would (the group still has one member)
                parallel.set_engine(tr.sync)
                assert len(tr.sync.bounds) >= 4
            torch.manual_seed(1)
            for _ in range(2):
                tr.train_step()
                tr.step += 1
            torch.cuda.synchronize()
            results.append(tr.arena.data.clone())
            parallel.set_engine(None)
        assert torch.equal(results[0], results[1])
    finally:
        parallel.set_engine(None)
        dist.destroy_process_group()


def test_degradation_prefetch_is_bit_identical(monkeypatch):
    """Trainer's side-stream prefetch of q_sample (deblurring) must not change a single bit of the training trajectory."""
    from deblurring_diffusion_pytorch import GaussianDiffusion, Trainer, Unet
    out = []
    for pf in ("0", "1"):
        monkeypatch.setenv("COLDDIFF_PREFETCH", pf)
        torch.manual_seed(3)
        net = quiet(Unet, dim=16, dim_mults=(1, 2), channels=3).to(DEV)
        d = GaussianDiffusion(net, image_size=32, device_of_kernel="cuda", channels=3, timesteps=20, kernel_size=5, kernel_std=0.3,
                              blur_routine="Exponential_reflect").to(DEV)
        tr = Trainer(d, None, image_size=32, train_batch_size=8, train_lr=1e-3, train_num_steps=4, gradient_accumulate_every=2,
                     dataset="synthetic", results_folder="/tmp/cdf_prefetch_res")
        assert tr._can_prefetch() == (pf == "1")
        torch.manual_seed(5)
        losses = []
        for _ in range(4):
            losses.append(tr.train_step())
            tr.step += 1
        torch.cuda.synchronize()
        out.append((tr.arena.data.clone(), torch.stack(losses).cpu()))
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][0], out[1][0])
