"""Timings of the snowification package on the MI355X (HIP events, warm-up, median over repeated windows in one process):

  (a) `cdf_snow_chain` at 64 x 3 x 128 x 128 and 32 x 3 x 32 x 32, T = 50, random t, with one snow layer (L = 1) and one per row
      (`single_snow`, L = B), in us: the launch alone and the training path (`prepare` without regeneration) -- with the HBM floor of
      24 B per pixel (the three channels read once and written once; the 8 B of snow per pixel come from tables that stay in L2);
  (b) `cdf_snow_layers` for T = 50 at both sizes and both L: what `random_snow` adds to every training step on the device, and next to
      it the whole regeneration with its host part (numpy normal field, scipy zoom, upload);
  (c) context only: the same q_sample composed the way the reference does it, on the same device -- max(t) + 1 passes of its elementwise
      expressions, torch.stack and a gather per row (it is not this project's code path);
  (d) one `Final` train step at 2 x 32 images of 32 x 32 (the package's default dataset size) with get_model's UnetConvNext, in img/s.

    python tools/snow_time.py [--out profiles/snow_timing.json] [--skip-train]

No GPU: fails (a CPU run cannot give a time)."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "cold-diffusion-models_amd", "snowification"), os.path.join(REPO, "cold-diffusion-models_amd")):
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


def reference_composition(x, t, snow, br):
    """q_sample as the reference composes it (diffusion.py:344-388 over forward_process_impl.py:362-372), on torch ops of the same device;
    snow: [T,L,3,H,W] planes."""
    blurs = []
    for i in range(int(t.max()) + 1):
        og_r = (x + 1.) / 2.
        gray = (0.299 * og_r[:, 0:1] + 0.587 * og_r[:, 1:2] + 0.114 * og_r[:, 2:3]) * 1.5 + 0.5
        gray = torch.maximum(og_r, gray)
        scaled = br[i] * og_r + (1 - br[i]) * gray
        blurs.append(torch.clip(scaled + snow[i] + torch.rot90(snow[i], k=2, dims=[2, 3]), 0.0, 1.0) * 2. - 1.)
    blurs = torch.stack(blurs)
    return torch.stack([blurs[t[b], b] for b in range(x.shape[0])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-train", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "snow_time.py measures on the MI355X; a CPU run cannot give a time"
    from diffusion import GaussianDiffusion
    from diffusion.model.get_model import get_model
    from colddiff import flat
    from colddiff import runtime as rt
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0)}
    T = 50
    lib = rt.lib()
    for B, H in ((64, 128), (32, 32)):
        x = torch.rand(B, 3, H, H, device=dev) * 2 - 1
        t = torch.randint(0, T, (B,), device=dev)
        floor_us = B * H * H * 24 / HBM_ACHIEVABLE * 1e6
        for single in (False, True):
            tag = f"{B}x3x{H}x{H}_T50_L{B if single else 1}"
            gd = GaussianDiffusion(None, image_size=(H, H), device_of_kernel='cuda', timesteps=T, forward_process_type='Snow',
                                   single_snow=single, batch_size=B, results_folder=None)
            fp = gd.forward_process
            planes = fp.planes(dev)
            br, omb = fp._tables
            nb, y, st = (t + 1).contiguous(), torch.empty_like(x), rt.stream(x)
            args = (x.data_ptr(), 0, y.data_ptr(), 0, 0, 0, planes.data_ptr(), br.data_ptr(), omb.data_ptr(), nb.data_ptr(), 0, B, H * H,
                    planes.shape[1], T, 0, 0, 0, st)
            r = timed(lambda: lib.cdf_snow_chain(*args), iters=200)
            r["hbm_floor_us"], r["floor_share"] = floor_us, floor_us / r["median_us"]
            res["snow_chain_launch_" + tag] = r
            print(tag, "cdf_snow_chain launch alone:", r, flush=True)
            r = timed(lambda: gd.prepare(x, t=t), iters=200)                    # (random_snow off: reset_parameters regenerates nothing)
            r["hbm_floor_us"] = floor_us
            res["train_q_sample_" + tag] = r
            print(tag, "training-path q_sample (prepare):", r, flush=True)
            base, thres = fp.snow_base.to(dev), fp._host[0].to(dev)
            taps, vert, out = fp.taps.to(dev), fp.vertical.to(dev), torch.empty_like(planes)
            largs = (base.data_ptr(), thres.data_ptr(), taps.data_ptr(), vert.data_ptr(), out.data_ptr(), H, H, planes.shape[1], T,
                     taps.shape[1], st)
            r = timed(lambda: lib.cdf_snow_layers(*largs), iters=50)
            r["bytes_written"] = out.numel() * 4
            res["snow_layers_launch_" + tag] = r
            print(tag, "cdf_snow_layers launch alone:", r, flush=True)
            assert torch.equal(out, planes)
            fp.random_snow = True                                                # the whole regeneration, host part included (wall clock)
            wall = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fp.reset_parameters()
                fp.planes(dev)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e6)
            fp.random_snow = False
            res["random_snow_regeneration_wall_" + tag] = {"median_us": sorted(wall)[2], "min_us": min(wall), "max_us": max(wall)}
            print(tag, "random_snow regeneration (host + device, wall):", res["random_snow_regeneration_wall_" + tag], flush=True)
            if not single:
                snow = torch.stack(fp.snow)                                      # [T,1,3,H,W], as the reference keeps them
                got, want = gd.q_sample(x, t), reference_composition(x, t, snow, fp.br_coef_list)
                res["q_sample_vs_reference_composition_max_abs_" + tag] = (got - want).abs().max().item()
                res["q_sample_reference_composition_" + tag] = timed(lambda: reference_composition(x, t, snow, fp.br_coef_list), iters=5,
                                                                     windows=5, warmup=2)
                print(tag, "reference composition:", res["q_sample_reference_composition_" + tag], "max-abs difference",
                      res["q_sample_vs_reference_composition_max_abs_" + tag], flush=True)
    if not a.skip_train:
        import contextlib
        import io
        H = 32
        with contextlib.redirect_stdout(io.StringIO()):
            net = get_model(types.SimpleNamespace(model="UnetConvNext", dataset="cifar10")).to(dev)
        gd = GaussianDiffusion(net, image_size=(H, H), device_of_kernel='cuda', timesteps=T, train_routine='Final', loss_type='l1',
                               forward_process_type='Snow', batch_size=32, results_folder=None).to(dev)
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
        res["final_train_step_2x32_32x32_UnetConvNext"] = r
        print("train step:", r, flush=True)
    line = json.dumps(res, indent=1, sort_keys=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
