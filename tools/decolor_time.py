"""Timings of the decolorization package on the MI355X (HIP events, warm-up, median over repeated windows in one process):

  (a) q_sample at 64 x 3 x 128 x 128, T = 50, random t, RGB and Lab, in us: the training path (`prepare`), the public method, and the
      kernel launch alone -- with the HBM floor (8 B per element per output written: one read + one write);
  (b) the same q_sample composed the way the reference does it, on the same device: max(t) + 1 torch.nn.functional.conv2d 1 x 1 launches
      plus torch.stack and a gather per row (context only: it is not this project's code path);
  (c) one x0_step_down reverse step at 16 images WITHOUT the network call (the chain + combine launch);
  (d) the decolor `Final` train step at 2 x 32 images of 128 x 128 with get_model's UnetConvNext, in img/s.

    python tools/decolor_time.py [--out profiles/decolor_timing.json] [--skip-train]

No GPU: fails (a CPU run cannot give a time)."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "cold-diffusion-models_amd", "decolor_diffusion"), os.path.join(REPO, "cold-diffusion-models_amd")):
    sys.path.insert(0, p)

HBM_ACHIEVABLE = 6.3e12        # B/s


def timed(fn, iters, windows=7, warmup=3):
    """Median (and min / max) over `windows` event-timed windows of `iters` calls each, in microseconds per call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(1000.0 * e0.elapsed_time(e1) / iters)
    return {"median_us": statistics.median(out), "min_us": min(out), "max_us": max(out), "iters": iters, "windows": windows}


def reference_composition(x, weights, t):
    """q_sample as the reference composes it (diffusion.py:344-388), on torch ops of the same device."""
    import torch.nn.functional as F
    cur, blurs = x, []
    for i in range(int(t.max()) + 1):
        cur = F.conv2d(cur, weights[i])
        blurs.append(cur)
    blurs = torch.stack(blurs)
    return torch.stack([blurs[t[b], b] for b in range(x.shape[0])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-train", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "decolor_time.py measures on the MI355X; a CPU run cannot give a time"
    from diffusion import GaussianDiffusion
    from diffusion.model.get_model import get_model
    from colddiff import decolor, flat
    from colddiff import runtime as rt
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0)}
    B, H, T = 64, 128, 50
    x = torch.rand(B, 3, H, H, device=dev) * 2 - 1
    t = torch.randint(0, T, (B,), device=dev)
    floor_us = x.numel() * 8 / HBM_ACHIEVABLE * 1e6
    for lab in (False, True):
        gd = GaussianDiffusion(None, image_size=(H, H), device_of_kernel='cuda', timesteps=T, to_lab=lab)
        xin = decolor.rgb2lab(x) if lab else x
        r = timed(lambda: gd._q_sample_nonneg(xin, t), iters=200 if not lab else 50)
        r["hbm_floor_us"] = floor_us
        r["floor_share"] = floor_us / r["median_us"]
        res["train_q_sample_64x3x128x128_T50_" + ("lab" if lab else "rgb")] = r          # the training path (prepare): t >= 0, n_b = t + 1
        print(("lab" if lab else "rgb"), "training-path q_sample (_q_sample_nonneg):", r, flush=True)
        r = timed(lambda: gd.q_sample(xin, t), iters=200 if not lab else 50)                 # the public method: + the t == -1 index arithmetic
        r["hbm_floor_us"] = floor_us
        res["public_q_sample_64x3x128x128_T50_" + ("lab" if lab else "rgb")] = r
        print(("lab" if lab else "rgb"), "public q_sample:", r, flush=True)
        # the launch alone: outputs allocated once, the step vector given (what is left of the figure above is the Python layer's
        # allocation, the t + 1 kernel and the ctypes call)
        nb, y, table = (t + 1).contiguous(), torch.empty_like(xin), gd._table(dev)
        L, st = rt.lib(), rt.stream(xin)
        args = (xin.data_ptr(), y.data_ptr(), 0, 0, 0, table.data_ptr(), nb.data_ptr(), B, 3, H * H, T, 0, 0, 1 if lab else 0, st)
        r = timed(lambda: L.cdf_color_chain(*args), iters=200 if not lab else 50)
        r["hbm_floor_us"] = floor_us
        r["floor_share"] = floor_us / r["median_us"]
        res["color_chain_launch_64x3x128x128_T50_" + ("lab" if lab else "rgb")] = r
        print(("lab" if lab else "rgb"), "cdf_color_chain launch alone:", r, flush=True)
    gd = GaussianDiffusion(None, image_size=(H, H), device_of_kernel='cuda', timesteps=T)
    weights = [k.to(dev) for k in gd.forward_process.kernels]
    got, want = gd._q_sample_nonneg(x, t), reference_composition(x, weights, t)
    res["q_sample_vs_reference_composition_max_abs"] = (got - want).abs().max().item()      # same results before the times are compared
    res["q_sample_reference_composition_rgb"] = timed(lambda: reference_composition(x, weights, t), iters=5, windows=5, warmup=2)
    print("reference composition:", res["q_sample_reference_composition_rgb"], "max-abs difference", res["q_sample_vs_reference_composition_max_abs"], flush=True)
    x16, img16 = x[:16].contiguous(), torch.rand(16, 3, H, H, device=dev) * 2 - 1
    table = gd._table(dev)
    for lab in (False, True):
        a16, i16 = (decolor.rgb2lab(x16), decolor.rgb2lab(img16)) if lab else (x16, img16)
        r = timed(lambda: decolor.color_chain(a16, table, nsteps=T - 1, nmax=T - 1, img=i16, lab=lab), iters=200 if not lab else 50)
        r["hbm_floor_us"] = x16.numel() * 16 / HBM_ACHIEVABLE * 1e6                         # two reads, two writes
        res["x0_step_down_chain_16x3x128x128_step49_" + ("lab" if lab else "rgb")] = r
        print(("lab" if lab else "rgb"), "reverse-step chain:", r, flush=True)
    if not a.skip_train:
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            net = get_model(types.SimpleNamespace(model="UnetConvNext", dataset="celebA")).to(dev)
        gd = GaussianDiffusion(net, image_size=(H, H), device_of_kernel='cuda', timesteps=T, train_routine='Final', loss_type='l1').to(dev)
        opt = flat.FusedAdam(list(gd.parameters()), lr=2e-5)
        batch = [torch.rand(32, 3, H, H, device=dev) * 2 - 1 for _ in range(2)]

        def step():
            preps = [gd.prepare(b) for b in batch]
            loss = gd.loss_prepared(tuple(torch.cat(p) for p in zip(*preps)))
            loss.backward()
            opt.step()
            opt.zero_grad()
        r = timed(step, iters=5, windows=5, warmup=3)
        r["img_per_s"] = 64 / (r["median_us"] * 1e-6)
        res["final_train_step_2x32_128x128_UnetConvNext"] = r
        print("train step:", r, flush=True)
    line = json.dumps(res, indent=1, sort_keys=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
