#!/usr/bin/env python3
"""Golden vectors of the snowification package, written by the UNMODIFIED reference `snowification/diffusion` on CPU under the stubs of
tests/snow_ref.py (where the reference tree exists):

    python tests/golden/snow/make_golden_snow.py      ->  snow_cases.pt, signatures.json  (this directory)

Nothing of the reference is copied: the file holds tensors, lists and scalars its code produced (the base layer and the blur directions
are recorded at the calls the reference makes -- `clipped_zoom`, `np.random.uniform`, `torch.randperm` -- by wrappers that pass them
through), and the parameter lists `inspect` reads off it.  The motion-blur taps come from the RESTATED 1-D torchgeometry Gaussian
(`restated_torchgeometry`: an unpinned boundary, like the 2-D one).

T = 20 everywhere; levels 1-4 at 13 x 13 and 32 x 32, plain and `single_snow` with 4 layers.  To stay under 1 MB the planes are stored
at a subset of the steps (all 20 only for the plain 13 x 13 cases; the lists, flags and bases are complete), the `q_sample` cases use
three to five images and the cases with a network in them two 32 x 32 images and the tiny network of tests/golden/decolor/decolor_net.pt
with one thread (the fixture is compared bit for bit when it is regenerated).
"""
import contextlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
REPO = os.path.dirname(TESTS)
DECOLOR = os.path.join(os.path.dirname(HERE), "decolor")
for p in (DECOLOR, TESTS, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import snow_ref as R  # noqa: E402
from make_golden_decolor import images, own_methods, signature_params  # noqa: E402

SEED = 123457
THREADS = 1
T, L = 20, 4
LEVELS, SIZES = (1, 2, 3, 4), (13, 32)
SIGNATURE_CLASSES = ("GaussianDiffusion", "Trainer", "UnetConvNextBlock", "DeColorization", "Snow")
ROUTINES = ("Final", "Step", "Step_Gradient")
SAMPLERS = ("default", "x0_step_down")
SAMPLE_T, FB_T = 4, 3                     # steps of the sample() / forward_and_backward() cases


def plane_steps(size, single):
    if size == 13:
        return (0, 3, 7, 12, 19) if single else tuple(range(T))
    return (7, 19) if single else (0, 7, 13, 19)


@contextlib.contextmanager
def recording(fpi, rec):
    """Pass-through wrappers around the three calls whose results the reference keeps in local variables."""
    zoom, uniform, randperm = fpi.clipped_zoom, np.random.uniform, torch.randperm

    def w_zoom(img, factor):
        out = zoom(img, factor)
        rec["zoom"].append(np.array(out))
        return out

    def w_uniform(*a, **k):
        out = uniform(*a, **k)
        rec["uniform"].append(out)
        return out

    def w_randperm(*a, **k):
        out = randperm(*a, **k)
        rec["randperm"].append(out.clone())
        return out

    fpi.clipped_zoom, np.random.uniform, torch.randperm = w_zoom, w_uniform, w_randperm
    try:
        yield
    finally:
        fpi.clipped_zoom, np.random.uniform, torch.randperm = zoom, uniform, randperm


def make_snow(ref, size, level, single, **kw):
    """(reference Snow, base [L,H,W] fp32, vertical [T,L] uint8) with torch seeded."""
    fpi = ref._cdf_ref_modules["diffusion.forward_process_impl"]
    rec = {"zoom": [], "uniform": [], "randperm": []}
    torch.manual_seed(SEED)
    with recording(fpi, rec):
        fp = fpi.Snow(image_size=(size, size), snow_level=level, num_timesteps=T, single_snow=single, batch_size=L, **kw)
    base = torch.Tensor(np.concatenate(rec["zoom"], axis=2)).permute(2, 0, 1).contiguous()
    n = base.shape[0]
    vertical = torch.full((T, n), 1 if rec["uniform"][0] > 0.5 else 0, dtype=torch.uint8)
    if single:
        for i, perm in enumerate(rec["randperm"]):
            vertical[i] = 0
            vertical[i, perm[:int(n / 2)]] = 1
    return fp, base, vertical


def layer_cases():
    ref = R.load()
    out = {"restated_torchgeometry": True}
    for level in LEVELS:
        for size in SIZES:
            for single in (False, True):
                fp, base, vertical = make_snow(ref, size, level, single)
                c = {"base": base, "vertical": vertical, "snow_thres_list": fp.snow_thres_list, "mb_sigma_list": fp.mb_sigma_list,
                     "br_coef_list": fp.br_coef_list, "steps": plane_steps(size, single),
                     "planes": torch.stack([fp.snow[i][:, 0] for i in plane_steps(size, single)]).clone()}
                assert all(torch.equal(fp.snow[i][:, 0], fp.snow[i][:, 1]) and torch.equal(fp.snow[i][:, 0], fp.snow[i][:, 2]) and
                           torch.equal(fp.snow_rot[i], torch.flip(fp.snow[i], dims=[2, 3])) for i in range(T))
                if single:
                    c["rng_probe"] = torch.rand(8)                       # the torch generator after construction ...
                    if level == 1 and size == 13:
                        torch.manual_seed(SEED)
                        make_snow(ref, size, level, single)
                        c["rng_state"] = torch.get_rng_state()          # ... and, for level 1, its whole state
                out[f"L{level}_{size}_{'single' if single else 'plain'}"] = c
    return out


def _gd(ref, net, size, **kw):
    GD = ref._cdf_ref_modules["diffusion.diffusion"].GaussianDiffusion
    torch.manual_seed(SEED)
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        return GD(net, image_size=(size, size), device_of_kernel='cuda', channels=3, timesteps=T, forward_process_type='Snow',
                  results_folder=tempfile.gettempdir(), **kw)


def forward_cases():
    """Snow.forward / total_forward and q_sample without a network in them."""
    ref = R.load()
    x13, x32 = images(3, 11, size=13), images(2, 12, size=32)
    t, t_neg = torch.tensor([0, T - 1, 7]), torch.tensor([6, -1, T - 2])
    out = {"x13": x13, "x32": x32, "t": t, "t_neg": t_neg}
    for key, kw in (("L1", dict(snow_level=1)), ("L1_fix", dict(snow_level=1, fix_brightness=True)), ("L3", dict(snow_level=3))):
        gd = _gd(ref, None, 13, **kw)
        q, tot = gd.q_sample(x13, t, return_total_blur=True)
        qn, totn = gd.q_sample(x13, t_neg, return_total_blur=True)
        out[key] = {"q": q.clone(), "total": tot.clone(), "q_neg": qn.clone(), "total_neg": totn.clone()}
    gd = _gd(ref, None, 13, snow_level=1)
    out["forward_7"] = gd.forward_process.forward(None, 7, og=x13).clone()
    out["total_forward"] = gd.forward_process.total_forward(x13).clone()
    out["all_minus_one"] = gd.q_sample(x13, torch.full((3,), -1)).clone()
    gd = _gd(ref, None, 32, snow_level=1)
    t32 = torch.tensor([7, T - 1])
    q, tot = gd.q_sample(x32, t32, return_total_blur=True)
    out["L1_32"] = {"t": t32, "q": q.clone(), "forward_7": gd.forward_process.forward(None, 7, og=x32).clone()}
    x4 = images(L, 13, size=13)
    t4 = torch.tensor([3, T - 1, 0, 12])                                 # (steps whose single_snow planes are stored)
    gd = _gd(ref, None, 13, snow_level=1, single_snow=True, batch_size=L)
    q, tot = gd.q_sample(x4, t4, return_total_blur=True)
    out["L1_single"] = {"x": x4, "t": t4, "q": q.clone(), "total": tot.clone()}
    return out


def _net(ref, sd):
    U = ref._cdf_ref_modules["diffusion.model.unet_convnext"].UnetConvNextBlock
    torch.manual_seed(SEED)
    with contextlib.redirect_stdout(open(os.devnull, "w")):
        net = U(dim=8, dim_mults=(1, 2))
    net.load_state_dict(sd, strict=True)
    return net


def network_cases():
    """Everything with the tiny network in it: the three train routines' q_sample outputs and losses, sample / all_sample /
    forward_and_backward with both sampling routines."""
    ref = R.load()
    sd = torch.load(os.path.join(DECOLOR, "decolor_net.pt"), weights_only=False)["state_dict"]
    x = images(2, 14, size=32)
    t = torch.tensor([0, 7])                                             # t - 1 has a -1 row: the Step routines' q_sample quirk
    out = {"x": x, "t": t, "routines": {}, "samplers": {}}
    for routine in ROUTINES:
        gd = _gd(ref, _net(ref, sd), 32, train_routine=routine)
        out["routines"][routine] = {"loss": gd.p_losses(x, t).detach().clone()}
    out["x_blur"], out["x_blur_sub"] = gd.q_sample(x, t).clone(), gd.q_sample(x, t - 1).clone()      # what every routine hands on
    with torch.no_grad():
        for samp in SAMPLERS:
            with contextlib.redirect_stdout(open(os.devnull, "w")):
                gd = _gd(ref, _net(ref, sd).eval(), 32, sampling_routine=samp)
                got = gd.sample(batch_size=2, img=x.clone(), t=SAMPLE_T)
                # xt and the first prediction do not depend on the sampling routine: stored once
                for k in ("xt", "direct_recons"):
                    assert k not in out or torch.equal(out[k], got[k])
                    out[k] = got[k].clone()
                X0, Xt, _, _ = gd.all_sample(batch_size=2, img=x.clone(), times=2)
                ts = torch.tensor([5, 5])
                out["samplers"][samp] = {"recon": got["recon"].clone(), "all_sample_X_t_last": Xt[-1].clone(), "one_step_t": ts,
                                         "one_step_x": gd.sample_one_step(x.clone(), ts)[0].clone()}
                F, B, last = gd.forward_and_backward(batch_size=2, img=x.clone(), t=FB_T)
                fb = {"lengths": (len(F), len(B)), "Forward_last": F[-1].clone(), "img": last.clone()}
                assert "forward_and_backward" not in out or all(torch.equal(out["forward_and_backward"][k], fb[k]) for k in ("Forward_last", "img"))
                out["forward_and_backward"] = fb                     # (no sampling routine in it)
    return out


def signature_case():
    ref = R.load()
    m = ref._cdf_ref_modules
    classes = {"GaussianDiffusion": m["diffusion.diffusion"].GaussianDiffusion, "Trainer": m["diffusion.diffusion"].Trainer,
               "UnetConvNextBlock": m["diffusion.model.unet_convnext"].UnetConvNextBlock,
               "DeColorization": m["diffusion.forward_process_impl"].DeColorization, "Snow": m["diffusion.forward_process_impl"].Snow}
    return {c: {name: signature_params(fn) for name, fn in sorted(own_methods(classes[c]).items())} for c in SIGNATURE_CLASSES}


def generate():
    threads = torch.get_num_threads()
    torch.set_num_threads(THREADS)
    state = torch.get_rng_state()
    try:
        return {"layers": layer_cases(), "forward": forward_cases(), "network": network_cases()}
    finally:
        torch.set_num_threads(threads)
        torch.set_rng_state(state)


def main():
    assert R.available(), "needs the reference tree"
    torch.save(generate(), os.path.join(HERE, "snow_cases.pt"))
    with open(os.path.join(HERE, "signatures.json"), "w") as f:
        json.dump(signature_case(), f, indent=1, sort_keys=True)
        f.write("\n")
    for name in sorted(os.listdir(HERE)):
        print(name, os.path.getsize(os.path.join(HERE, name)) // 1024, "KiB")


if __name__ == "__main__":
    main()
