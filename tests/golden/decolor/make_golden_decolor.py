#!/usr/bin/env python3
"""Golden vectors of the decolorization package, written by the UNMODIFIED reference `decolor-diffusion/diffusion` on CPU under the stubs
of tests/decolor_ref.py (where the reference tree exists):

    python tests/golden/decolor/make_golden_decolor.py      ->  decolor_net.pt, decolor_cases.pt, signatures.json  (this directory)

Nothing of the reference is copied: the files hold tensors and scalars its code produced, and the parameter lists `inspect` reads off it.
Fixed seed; UnetConvNextBlock(dim=8, dim_mults=(1, 2)) at 16 x 16; T = 6, and T = 50 for the chain-only cases.  The `lab` entries come
from `to_lab=True` runs, i.e. through the kornia functions RESTATED in decolor_ref.py (kornia is not installed): they are labelled
`restated_kornia` and held to the measured Lab tolerance by the tests, not to the RGB bounds.

Size: one full set of parameter gradients is 335 KB -- as much as the state_dict -- so the nine train-routine x loss combinations store the
loss and the gradients of the tensors at the two ends of the backward pass: the first block's `ds_conv` / first conv / `res_conv` (what arrives after the WHOLE backward path),
`time_mlp.*` (the sum over every block's time bias) and `final_conv.1.*`.  Every other gradient is checked without fixture bytes
(tests/test_decolor_golden.py): where the reference tree exists, `loss_cases(sd, full=True)` is compared in memory with the CPU
restatement, and everywhere the engine's whole gradient is compared with that restatement, which the fixture pins at the subset.  The chain-only cases use 5 x 5 images (a pixel count that is not a multiple of 4), the
sampler cases two images.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
REPO = os.path.dirname(TESTS)
for p in (TESTS, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import decolor_ref as R  # noqa: E402

SEED = 123457
THREADS = 8                       # the thread count the fixtures were written with (conv weight-gradient summation order)
T_SMALL, T_LONG, SIZE = 6, 50, 16
GRAD_SUBSET = ("downs.0.0.ds_conv.", "downs.0.0.net.1.", "downs.0.0.res_conv.", "time_mlp.", "final_conv.1.")
SIGNATURE_CLASSES = ("GaussianDiffusion", "Trainer", "UnetConvNextBlock", "DeColorization")
ROUTINES = ("Final", "Step", "Step_Gradient")
LOSSES = ("l1", "l2", "sqrt")


def images(n, seed, size=SIZE):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, 3, size, size), generator=g).float() / 255 * 2 - 1


def _classes(ref):
    m = ref._cdf_ref_modules
    return (m["diffusion.diffusion"].GaussianDiffusion, m["diffusion.model.unet_convnext"].UnetConvNextBlock,
            m["diffusion.forward_process_impl"].DeColorization, m["diffusion.utils"])


def _net(ref, sd=None, **kw):
    U = _classes(ref)[1]
    torch.manual_seed(SEED)
    net = U(dim=8, dim_mults=(1, 2), **kw)
    if sd is not None:
        net.load_state_dict({k: v for k, v in sd.items() if k in net.state_dict()}, strict=True)
    return net


def _gd(ref, net, T=T_SMALL, **kw):
    GD = _classes(ref)[0]
    return GD(net, image_size=(SIZE, SIZE), device_of_kernel='cuda', channels=3, timesteps=T, **kw)


def net_cases():
    """The network's state_dict and one Final / l1 loss on it."""
    ref = R.load()
    net = _net(ref)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    x, t = images(4, 1), torch.tensor([0, 5, 2, 3])
    gd = _gd(ref, net, train_routine='Final', loss_type='l1')
    loss = gd.p_losses(x, t)
    loss.backward()
    return {"state_dict": sd, "x": x, "t": t, "loss": loss.detach().clone()}


def chain_cases():
    """q_sample without a network in it: both decolor routines, total removal on / off, T = 6 and T = 50, a batch with t == -1 rows."""
    ref = R.load()
    net = _net(ref)
    out = {"x": images(4, 2, size=5)}
    x = out["x"]
    for T in (T_SMALL, T_LONG):
        t = torch.tensor([0, T - 1, T // 2, 1])
        t_neg = torch.tensor([2, -1, T - 2, -1])
        for routine in ("Constant", "Linear"):
            for remove in (True, False):
                gd = _gd(ref, net, T=T, decolor_routine=routine, decolor_total_remove=remove)
                q, tot = gd.q_sample(x, t, return_total_blur=True)
                qn, totn = gd.q_sample(x, t_neg, return_total_blur=True)
                out[f"T{T}_{routine}_{int(remove)}"] = {"t": t, "q": q.clone(), "total": tot.clone(), "t_neg": t_neg, "q_neg": qn.clone(),
                                                        "total_neg": totn.clone(),
                                                        "table": torch.stack([k.weight.detach()[:, :, 0, 0] for k in gd.forward_process.kernels])}
    gd = _gd(ref, net)
    out["all_minus_one"] = gd.q_sample(x, torch.full((4,), -1)).clone()
    out["total_forward"] = gd.forward_process.total_forward(x).detach().clone()
    return out


def loss_cases(sd, full=False):
    """Loss and gradients of the nine train-routine x loss combinations: the GRAD_SUBSET tensors for the fixture, every parameter with
    `full` (kept in memory by the test that compares the reference's whole gradient with the CPU restatement)."""
    ref = R.load()
    x, t = images(4, 1), torch.tensor([0, 5, 2, 3])          # t - 1 has a -1 row: the Step routines' q_sample quirk is on the path
    out = {}
    for routine in ROUTINES:
        for lt in LOSSES:
            net = _net(ref, sd)
            gd = _gd(ref, net, train_routine=routine, loss_type=lt)
            loss = gd.p_losses(x, t)
            loss.backward()
            out[f"{routine}_{lt}"] = {"loss": loss.detach().clone(),
                                      "grads": {k: p.grad.detach().clone() for k, p in net.named_parameters() if full or k.startswith(GRAD_SUBSET)}}
    return out


def sampler_cases(sd):
    ref = R.load()
    x4 = images(4, 3)
    x = x4[:2].clone()
    out = {"x": x4}
    with torch.no_grad():
        for train, samp in (("Final", "default"), ("Final", "x0_step_down"), ("Step", "default"), ("Step_Gradient", "default")):
            net = _net(ref, sd).eval()
            gd = _gd(ref, net, train_routine=train, sampling_routine=samp)
            out[f"sample_{train}_{samp}"] = {k: v.clone() for k, v in gd.sample(batch_size=2, img=x.clone()).items()}
        net = _net(ref, sd).eval()
        gd = _gd(ref, net, sampling_routine="x0_step_down")
        X0, Xt, _, _ = gd.all_sample(batch_size=2, img=x.clone(), times=2)
        out["all_sample"] = {"X_0s": [v.clone() for v in X0], "X_ts": [v.clone() for v in Xt]}
        F, B, last = gd.forward_and_backward(batch_size=2, img=x.clone())
        out["forward_and_backward"] = {"lengths": (len(F), len(B)), "Forward_last": F[-1].clone(), "Forward_3": F[3].clone(),
                                       "Backward_last": B[-1].clone(), "img": last.clone()}
        t_start, t_end = torch.tensor([5, 3, 0, 2]), torch.tensor([2, 3, 0, 0])
        out["sample_multi_step"] = {"t_start": t_start, "t_end": t_end, "out": gd.sample_multi_step(x4.clone(), t_start, t_end).clone()}
        for samp in ("default", "x0_step_down"):
            gd = _gd(ref, net, sampling_routine=samp)
            t = torch.tensor([3, 5, 0, 5])
            a, b = gd.sample_one_step(x4.clone(), t)
            out[f"one_step_{samp}"] = {"t": t, "x": a.clone(), "direct_recons": b.clone()}
    return out


def variant_cases(sd):
    """The two other networks: output_mean_scale=True (same parameters) and with_time_emb=False (the same weights minus the time MLPs)."""
    ref = R.load()
    x, t = images(2, 4), torch.tensor([1, 4])
    out = {"x": x, "t": t}
    net = _net(ref, sd, output_mean_scale=True)
    gd = _gd(ref, net)
    y = net(x, t)
    loss = gd.p_losses(x, t)
    loss.backward()
    out["mean_scale"] = {"out": y.detach().clone(), "loss": loss.detach().clone(),
                         "grads": {k: p.grad.detach().clone() for k, p in net.named_parameters() if k.startswith(GRAD_SUBSET)}}
    net = _net(ref, sd, with_time_emb=False)
    y0, y1 = net(x), net(x, t)
    out["no_time"] = {"keys": sorted(net.state_dict().keys()), "out": y0.detach().clone(), "out_with_t": y1.detach().clone()}
    return out


def lab_cases(sd):
    ref = R.load()
    utils = _classes(ref)[3]
    x = images(2, 5)
    xl = utils.rgb2lab(x)
    out = {"restated_kornia": True, "x": x, "x_lab": xl.clone(), "rgb_back": utils.lab2rgb(xl).clone()}
    with torch.no_grad():
        for T in (T_SMALL, T_LONG):
            net = _net(ref, sd).eval()
            gd = _gd(ref, net, T=T, to_lab=True, sampling_routine="x0_step_down")
            t = torch.tensor([T // 2, T - 1])
            q, tot = gd.q_sample(xl, t, return_total_blur=True)
            out[f"T{T}"] = {"t": t, "q": q.clone(), "total": tot.clone()}
        net = _net(ref, sd).eval()
        gd = _gd(ref, net, to_lab=True, sampling_routine="x0_step_down")
        out["sample"] = {k: v.clone() for k, v in gd.sample(batch_size=2, img=xl.clone()).items()}
    return out


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
    import inspect
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


def signature_case():
    ref = R.load()
    m = ref._cdf_ref_modules
    classes = {"GaussianDiffusion": m["diffusion.diffusion"].GaussianDiffusion, "Trainer": m["diffusion.diffusion"].Trainer,
               "UnetConvNextBlock": m["diffusion.model.unet_convnext"].UnetConvNextBlock,
               "DeColorization": m["diffusion.forward_process_impl"].DeColorization}
    return {c: {name: signature_params(fn) for name, fn in sorted(own_methods(classes[c]).items())} for c in SIGNATURE_CLASSES}


def generate():
    """{file name: contents} of the two .pt fixtures, with the thread count pinned."""
    threads = torch.get_num_threads()
    torch.set_num_threads(THREADS)
    try:
        net = net_cases()
        sd = net["state_dict"]
        cases = {"chains": chain_cases(), "losses": loss_cases(sd), "samplers": sampler_cases(sd), "variants": variant_cases(sd),
                 "lab": lab_cases(sd)}
    finally:
        torch.set_num_threads(threads)
    return {"decolor_net.pt": net, "decolor_cases.pt": cases}


def main():
    assert R.available(), "needs the reference tree"
    for name, obj in generate().items():
        torch.save(obj, os.path.join(HERE, name))
    with open(os.path.join(HERE, "signatures.json"), "w") as f:
        json.dump(signature_case(), f, indent=1, sort_keys=True)
        f.write("\n")
    for name in sorted(os.listdir(HERE)):
        print(name, os.path.getsize(os.path.join(HERE, name)) // 1024, "KiB")


if __name__ == "__main__":
    main()
