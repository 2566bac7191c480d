#!/usr/bin/env python3
"""The sequence of cdf_* calls the Python layer issues, written down so that two revisions of that layer can be compared line for line.
TEST INFRASTRUCTURE: runs on the SIMT-simulator build (CPU tensors, no GPU), so the numbers it saves are the kernels' own.

  python tools/call_trace.py OUTDIR [scenario ...]          (no scenario: all of them; --list prints the names)

Per scenario OUTDIR/<name>.trace holds one line per call -- name, integers / floats as they are, pointers as 0 / 1 (null or not:
addresses depend on the allocator), ctypes int arrays (phase / tap descriptors) by content -- and OUTDIR/<name>.pt the outputs and
every parameter gradient.  Compare two OUTDIRs with `--compare A B` (traces equal as text, tensors torch.equal).

Scenarios: Unet(dim=64, dim_mults=(1, 2, 4)) at 16 x 16, B = 2, forward + backward in every arithmetic mode ("bf16" = bf16 activation
storage), then a forward after a weights-epoch bump (the cdf_pack_many path) and the no-grad forward a sampler step makes; the same net
with the attention block's alternative forms switched on; the DDPM `Model` of tests/golden/model_ch32.pt likewise.

Sampler scenarios (`--list`: the names after `model`): every sampler method and `forward` of the six `GaussianDiffusion` cores and of the
decolorization / snowification cores, through their public methods only, on Unet(dim=8, dim_mults=(1, 2)) at 8 x 8, B = 2, T = 4
(`Incremental_factor_2`: T = 3, a fourth halving of 8 pixels is a plane of none).  One scenario is one configuration; its trace has a
`# call` line in front of every method call and a `! ExceptionName` line where a call raises, its .pt every returned tensor and, per
call, the next draw of the CPU generator after it (the generator is re-seeded before every call).
"""
import contextlib
import ctypes
import io
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "cold-diffusion-models_amd"), os.path.join(REPO, "tests"), REPO):
    sys.path.insert(0, p)
import torch  # noqa: E402
from colddiff import functions as F_, ops, runtime as rt  # noqa: E402
from emu_util import install_emu  # noqa: E402
from test_gpu_invariance import Recorder  # noqa: E402

# name -> (network, arithmetic mode, _ATTN_FUSED, _ATTN_QFOLD, ops._ATTN_KV_FUSED)
SCENARIOS = {"unet_%s" % m: ("unet", m, 1, True, True) for m in ("bf16x3", "f32", "bf16")}
for m in ("bf16x3", "bf16"):
    for tag, fused, qfold, kvf in (("plain", 0, False, True), ("project", 2, False, True), ("fold", 2, True, True),
                                   ("kvsplit", 1, True, False), ("project_kvsplit", 2, False, False)):
        SCENARIOS["unet_%s_%s" % (m, tag)] = ("unet", m, fused, qfold, kvf)
SCENARIOS["model"] = ("model", "bf16x3", 1, True, True)

# ---- sampler scenarios: name -> (family, constructor keywords) ---------------------------------------------------------------------------
B, T, SIZE = 2, 4, 8
for tag, kw in (("const_default", dict(blur_routine="Constant", sampling_routine="default")),
                ("const_x0", dict(blur_routine="Constant", sampling_routine="x0_step_down")),
                ("discrete_default", dict(blur_routine="Incremental", sampling_routine="default", discrete=True)),
                ("discrete_x0", dict(blur_routine="Incremental", sampling_routine="x0_step_down", discrete=True)),
                ("expreflect", dict(blur_routine="Exponential_reflect", sampling_routine="x0_step_down")),
                ("individual_default", dict(blur_routine="Individual_Incremental", sampling_routine="default")),
                ("individual_x0", dict(blur_routine="Individual_Incremental", sampling_routine="x0_step_down")),
                ("individual_other", dict(blur_routine="Individual_Incremental", sampling_routine="other")),
                ("step", dict(blur_routine="Constant", sampling_routine="default", train_routine="Step"))):
    SCENARIOS["deblur_" + tag] = ("deblur", kw)
for routine in ("Incremental", "Incremental_factor_2", "Incremental_bilinear_with_blur"):
    for s in ("default", "x0_step_down"):
        SCENARIOS["resolution_%s_%s" % (routine, s)] = ("resolution", dict(resolution_routine=routine, sampling_routine=s))
for tag, kw in (("incremental", dict(fade_routine="Incremental")), ("random", dict(fade_routine="Random_Incremental", discrete=True))):
    for s in ("default", "x0_step_down", "other"):
        SCENARIOS["defade_%s_%s" % (tag, s)] = ("defade", dict(sampling_routine=s, **kw))
for fam in ("denoise", "demix"):
    for s in ("ddim", "x0_step_down"):
        SCENARIOS["%s_%s" % (fam, s)] = (fam, dict(sampling_routine=s))
SCENARIOS["defgen"] = ("defgen", dict(reverse=False))
SCENARIOS["defgen_reverse"] = ("defgen", dict(reverse=True))
for fam in ("decolor", "snow"):
    SCENARIOS[fam + "_default"] = (fam, dict(sampling_routine="default"))
    SCENARIOS[fam + "_x0"] = (fam, dict(sampling_routine="x0_step_down"))
SCENARIOS["decolor_lab"] = ("decolor", dict(sampling_routine="x0_step_down", to_lab=True))


def line(lib, name, args):
    out = [name]
    for a, ct in zip(args, lib.protos[name][1]):
        if isinstance(a, ctypes.Array):
            out.append("[" + " ".join(str(v) for v in a) + "]")
        elif ct in (ctypes.c_void_p, ctypes.c_char_p):
            out.append("0" if not a else "1")
        else:
            out.append(repr(a))
    return " ".join(out)


def _flat(prefix, v, out):
    """Every tensor of a nested return value under a path name (None and other leaves by repr, as a byte tensor)."""
    if isinstance(v, torch.Tensor):
        out[prefix] = v.detach().cpu()
    elif isinstance(v, dict):
        for k, u in v.items():
            _flat("%s/%s" % (prefix, k), u, out)
    elif isinstance(v, (list, tuple)):
        out[prefix + "/len"] = torch.tensor(len(v))
        for k, u in enumerate(v):
            _flat("%s/%d" % (prefix, k), u, out)
    else:
        out[prefix] = torch.tensor(list(repr(v).encode()), dtype=torch.uint8)


def sampler_calls(family, kw):
    """-> [(label, callable)] on a fresh core of `family`."""
    from colddiff import decolor, diffusion as CD, snow
    from colddiff.unet import Unet
    torch.manual_seed(20260)
    net = decolor.UnetConvNextBlock(dim=8, dim_mults=(1, 2)) if family in ("decolor", "snow") else Unet(dim=8, dim_mults=(1, 2), channels=3)
    g = torch.Generator().manual_seed(31)
    x, x2 = (torch.rand(B, 3, SIZE, SIZE, generator=g) * 2 - 1 for _ in range(2))
    S = dict(batch_size=B)
    if family == "deblur":
        mk = lambda **k: CD.DeblurDiffusion(net, image_size=SIZE, device_of_kernel="cuda", channels=3, timesteps=T, kernel_std=0.5,
                                            kernel_size=3, **{**kw, **k})
        d = mk()
        return [("sample", lambda: d.sample(img=x, **S)), ("gen_sample", lambda: d.gen_sample(img=x, noise_level=0.1, **S)),
                ("sample_from_blur", lambda: d.sample_from_blur(img=x, start=1, **S)), ("all_sample", lambda: d.all_sample(img=x, **S)),
                ("forward_and_backward", lambda: d.forward_and_backward(img=x, noise_level=0.1, **S)),
                ("forward_and_backward_2", lambda: d.forward_and_backward_2(img=x, noise_level=0.1, **S)),
                ("opt", lambda: d.opt(x)), ("forward", lambda: d(x))]
    if family == "resolution":
        steps = 3 if "factor_2" in kw["resolution_routine"] else T
        mk = lambda **k: CD.ResolutionDiffusion(net, image_size=SIZE, device_of_kernel="cuda", channels=3, timesteps=steps, **{**kw, **k})
        d = mk()
        calls = [("sample", lambda: d.sample(img=x, **S)), ("gen_sample", lambda: d.gen_sample(img=x, times=3, noise_level=0.1, **S)),
                 ("all_sample", lambda: d.all_sample(img=x, **S)), ("forward_and_backward", lambda: d.forward_and_backward(img=x, **S)),
                 ("opt", lambda: d.opt(x))]
        return calls + [("forward_" + r, (lambda r=r: mk(train_routine=r)(x))) for r in ("Final", "Step", "Final_random_mean_and_actual")]
    if family == "defade":
        d = CD.DefadeDiffusion(net, image_size=SIZE, device_of_kernel="cuda", channels=3, timesteps=T, kernel_std=0.2, initial_mask=3, **kw)
        return [("sample", lambda: d.sample(faded_recon_sample=x, **S)), ("all_sample", lambda: d.all_sample(faded_recon_sample=x, times=3, **S)),
                ("forward", lambda: d(x))]
    if family in ("denoise", "demix", "defgen"):
        cls = {"denoise": CD.DenoiseDiffusion, "demix": CD.DemixDiffusion, "defgen": CD.DefadeGenDiffusion}[family]
        d = cls(net, image_size=SIZE, channels=3, timesteps=T, **kw)
        two = dict(img1=x, img2=x2) if family != "denoise" else dict(img=x)
        lvl = dict(noise_level=0.1) if family != "denoise" else {}
        return [("sample", lambda: d.sample(img=x, **S)), ("gen_sample", lambda: d.gen_sample(img=x, **lvl, **S)),
                ("all_sample", lambda: d.all_sample(img=x, **S)), ("forward_and_backward", lambda: d.forward_and_backward(**two, **S)),
                ("forward", lambda: d(x, x2))]
    cls, more = (decolor.DecolorDiffusion, {}) if family == "decolor" else (snow.SnowDiffusion, dict(forward_process_type="Snow", results_folder=None))
    d = cls(net, image_size=(SIZE, SIZE), device_of_kernel="cuda", channels=3, timesteps=T, **more, **kw)
    if kw.get("to_lab"):
        x = decolor.rgb2lab(x)
    return [("sample", lambda: d.sample(img=x, **S)), ("all_sample", lambda: d.all_sample(img=x, **S)),
            ("all_sample_ends_only", lambda: d.all_sample(img=x, ends_only=True, **S)),
            ("forward_and_backward", lambda: d.forward_and_backward(img=x, **S)), ("forward", lambda: d(x))]


def run_sampler(name, outdir):
    family, kw = SCENARIOS[name]
    lib = rt.lib()
    rt.set_precision("bf16x3")
    rt.bump_weights_epoch()
    rt.tuning()
    lines, out, raised = [], {}, []
    with contextlib.redirect_stdout(io.StringIO()):
        calls = sampler_calls(family, kw)
    for label, fn in calls:
        torch.manual_seed(7)
        error = None
        with Recorder(lib) as rec, contextlib.redirect_stdout(io.StringIO()):
            try:
                _flat(label, fn(), out)
            except Exception as e:                           # (part of the behaviour: an unknown routine, a routine upstream leaves unbuilt)
                error = type(e).__name__
                raised.append("%s: %s" % (label, error))
        lines += ["# %s\n" % label] + [line(lib, n, a) + "\n" for n, a in rec.calls] + (["! %s\n" % error] if error else [])
        out[label + "/next_draw"] = torch.rand(3)
    with open(os.path.join(outdir, name + ".trace"), "w") as f:
        f.writelines(lines)
    torch.save(out, os.path.join(outdir, name + ".pt"))
    print(name, sum(not l.startswith(("#", "!")) for l in lines), "calls", "raised: %s" % raised if raised else "", flush=True)


def run(name, outdir):
    if len(SCENARIOS[name]) == 2:
        return run_sampler(name, outdir)
    kind, mode, F_._ATTN_FUSED, F_._ATTN_QFOLD, ops._ATTN_KV_FUSED = SCENARIOS[name]
    lib = rt.lib()
    rt.set_precision(mode)
    rt.bump_weights_epoch()
    torch.manual_seed(20260)
    with contextlib.redirect_stdout(io.StringIO()):
        if kind == "unet":
            from deblurring_diffusion_pytorch import Unet
            net = Unet(dim=64, dim_mults=(1, 2, 4), channels=3)
            x, t, gy = torch.rand(2, 3, 16, 16) * 2 - 1, torch.tensor([1, 40]), torch.randn(2, 3, 16, 16) / 1000
        else:
            from deblurring_diffusion_pytorch import Model
            g = torch.load(os.path.join(REPO, "tests", "golden", "model_ch32.pt"), weights_only=False)
            net = Model(**g["cfg"])
            net.load_state_dict(g["sd"])
            x, t, gy = g["x"], g["t"], g["gy"]
    rt.tuning()                                              # (its first use in a process calls cdf_gemm_tuning_default once)
    with Recorder(lib) as rec:
        y = net(x, t)
        y.backward(gy)
        rt.bump_weights_epoch()                              # as after an optimizer step: one cdf_pack_many refreshes every layout
        y2 = net(x, t)
        with torch.no_grad():
            y3 = net(x, t)
    with open(os.path.join(outdir, name + ".trace"), "w") as f:
        f.writelines(line(lib, n, a) + "\n" for n, a in rec.calls)
    torch.save({"y": y.detach(), "y2": y2.detach(), "y3": y3, **{"grad/" + k: p.grad for k, p in net.named_parameters()}},
               os.path.join(outdir, name + ".pt"))
    print(name, len(rec.calls), "calls", flush=True)


def compare(a, b):
    bad = 0
    for name in SCENARIOS:
        have = [os.path.exists(os.path.join(d, name + ".trace")) for d in (a, b)]
        if not all(have):                                    # (a scenario that neither run made is no difference)
            bad += any(have)
            if any(have):
                print(name, "DIFFERENT: in one directory only")
            continue
        ta, tb =(open(os.path.join(d, name + ".trace")).read().splitlines() for d in (a, b))
        diff = [i for i, (u, v) in enumerate(zip(ta, tb)) if u != v]
        pa, pb = (torch.load(os.path.join(d, name + ".pt")) for d in (a, b))
        neq = [k for k in pa if k not in pb or not torch.equal(pa[k], pb[k])]
        ok = len(ta) == len(tb) and not diff and not neq and pa.keys() == pb.keys()
        bad += not ok
        print(name, len(ta), len(tb), "same" if ok else "DIFFERENT: first lines %s, tensors %s" % (diff[:5], neq[:5]))
        for i in diff[:5]:
            print("  -", ta[i], "\n  +", tb[i])
    return bad


def main(argv):
    if argv[:1] == ["--list"]:
        print("\n".join(SCENARIOS))
        return 0
    if argv[:1] == ["--compare"]:
        return 1 if compare(argv[1], argv[2]) else 0
    os.makedirs(argv[0], exist_ok=True)
    install_emu()
    for name in argv[1:] or SCENARIOS:
        run(name, argv[0])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
