"""The drop-in boundary of the decolorization package (`cold-diffusion-models_amd/decolor_diffusion/diffusion`), checked against the reference's
signatures: LIVE where the reference tree exists and everywhere against tests/golden/decolor/signatures.json, which
tests/golden/decolor/make_golden_decolor.py records from it (the live run requires the two to be equal).  The rule is the prefix rule
stated at the top of tests/test_boundary.py: the reference's parameters are a prefix of ours with the same names, order, kinds and
defaults; what this engine adds comes after, defaulted.  Of `Trainer`, the constructor and train / save / load / step_ema /
reset_parameters are required; its figure and evaluation methods that are not built are printed, not failed.
"""
import contextlib
import inspect
import io
import json
import os
import sys
import types

import pytest
import torch

import decolor_ref as R
from test_boundary import TRAINER_REQUIRED, _accepts_every_reference_call, _forwards_keywords, _shown

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decolor")
CLASSES = ("GaussianDiffusion", "Trainer", "UnetConvNextBlock", "DeColorization")


def _generator():
    sys.path.insert(0, GOLD)
    try:
        import make_golden_decolor
    finally:
        sys.path.remove(GOLD)
    return make_golden_decolor


def _reference_signatures():
    with open(os.path.join(GOLD, "signatures.json")) as f:
        recorded = json.load(f)
    if R.available():
        assert _generator().signature_case() == recorded, "tests/golden/decolor/signatures.json is stale: run make_golden_decolor.py"
    return recorded


def test_signatures_equal_the_reference():
    M = _generator()
    ref = _reference_signatures()
    D = R.mine()
    assert set(ref) == set(CLASSES) == set(M.SIGNATURE_CLASSES)
    missing, different, optional = [], [], []
    for cname in CLASSES:
        mc = getattr(D, cname)
        mm = M.own_methods(mc)
        not_built = set(getattr(mc, "NOT_BUILT", ()))
        for mname, rparams in ref[cname].items():
            built = (mname in mm or hasattr(mc, mname)) and mname not in not_built
            if not built and not (cname == "Trainer" and mname not in TRAINER_REQUIRED):
                missing.append(cname + "." + mname)
                continue
            if not built:
                optional.append(cname + "." + mname)
            if mname in mm or hasattr(mc, mname):           # (a closed evaluation method still carries the reference's signature)
                mparams = M.signature_params(mm.get(mname, getattr(mc, mname)))
                if not (_accepts_every_reference_call(rparams, mparams) or (mname == "__init__" and _forwards_keywords(rparams, mparams))):
                    different.append((cname + "." + mname, _shown(rparams), _shown(mparams)))
    print("figure / evaluation methods of the reference Trainer that are not built:", sorted(optional))
    assert not missing, "reference methods without a counterpart: %s" % missing
    assert not different, "signatures differ from the reference:\n" + "\n".join("%s\n   ref  %s\n   here %s" % d for d in different)
    for name in TRAINER_REQUIRED:
        assert name in M.own_methods(D.Trainer) or hasattr(D.Trainer, name)


def test_reference_import_lines_and_driver_calls_bind(tmp_path):
    """train.py:1-5 and 59-119 of the reference: its import lines resolve against the package, `get_dataset.get_image_size` answers, and the
    constructor calls bind with the script's keywords (bound, not executed: this test needs no device; execution on hardware is
    tests/test_decolor_trainer.py)."""
    R.mine()
    ns = {}
    exec("from diffusion import GaussianDiffusion, Trainer, get_dataset\nfrom diffusion.model.get_model import get_model", ns)
    assert ns["get_dataset"].get_image_size("cifar10") == (32, 32) and ns["get_dataset"].get_image_size("celebA") == (128, 128)
    args = types.SimpleNamespace(model="UnetConvNext", dataset="celebA")
    with contextlib.redirect_stdout(io.StringIO()):
        model = ns["get_model"](args, with_time_emb=True)
        one_shot = ns["get_model"](args, with_time_emb=False)
    assert model.time_mlp is not None and one_shot.time_mlp is None and model.channels == 3
    with pytest.raises(NotImplementedError, match="UnetResNet"):
        ns["get_model"](types.SimpleNamespace(model="UnetResNet", dataset="cifar10"))
    inspect.signature(ns["GaussianDiffusion"].__init__).bind(
        None, model, image_size=(128, 128), device_of_kernel='cuda', channels=3, one_shot_denoise_fn=one_shot, timesteps=50, loss_type='l1',
        train_routine='Final', sampling_routine='x0_step_down', forward_process_type='Decolorization', decolor_routine='Constant',
        decolor_ema_factor=0.9, decolor_total_remove=True, snow_level=1, single_snow=False, batch_size=16, random_snow=False, to_lab=False,
        load_path=None, results_folder=str(tmp_path), fix_brightness=False)
    inspect.signature(ns["Trainer"].__init__).bind(
        None, object(), './root_celebA', image_size=(128, 128), train_batch_size=16, train_lr=2e-5, train_num_steps=700000,
        gradient_accumulate_every=2, ema_decay=0.995, fp16=False, results_folder=str(tmp_path), load_path=None, random_aug=False,
        torchvision_dataset=False, dataset='celebA', to_lab=False)
    with pytest.raises(NotImplementedError, match="Snow"):
        ns["GaussianDiffusion"](model, image_size=(128, 128), device_of_kernel='cuda', forward_process_type='Snow')


def test_attribute_names_of_the_diffusion_class():
    D = R.mine()
    gd = D.GaussianDiffusion(None, image_size=(32, 32), device_of_kernel='cuda', timesteps=20, to_lab=True, recon_noise_std=0.1,
                             decolor_routine='Linear', decolor_total_remove=False)
    for name in ("channels", "image_size", "denoise_fn", "device_of_kernel", "num_timesteps", "loss_type", "train_routine", "sampling_routine",
                 "snow_level", "random_snow", "batch_size", "single_snow", "to_lab", "recon_noise_std", "forward_process"):
        assert hasattr(gd, name), name
    fp = gd.forward_process
    assert isinstance(fp, D.DeColorization) and len(fp.kernels) == 20 and fp.to_lab is True and fp.decolor_routine == 'Linear'
    assert fp.reset_parameters() is None and fp.reset_parameters(batch_size=4) is None
    assert torch.equal(fp.table, R.table_of('Linear', 20, total_remove=False))


@pytest.mark.skipif(not R.available(), reason="needs the reference tree")
@pytest.mark.parametrize("kw", [dict(), dict(with_time_emb=False), dict(output_mean_scale=True, channels=3, out_dim=3)])
def test_same_seed_gives_the_reference_initial_weights(kw):
    ref = R.load()
    U = ref._cdf_ref_modules["diffusion.model.unet_convnext"].UnetConvNextBlock
    D = R.mine()
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(77)
        theirs = U(dim=8, dim_mults=(1, 2), **kw)
        torch.manual_seed(77)
        ours = D.UnetConvNextBlock(dim=8, dim_mults=(1, 2), **kw)
    a, b = theirs.state_dict(), ours.state_dict()
    assert list(a.keys()) == list(b.keys())
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert [n for n, _ in theirs.named_parameters()] == [n for n, _ in ours.named_parameters()]


@pytest.mark.skipif(not R.available(), reason="needs the reference tree")
def test_weight_tables_are_bit_equal_to_the_live_reference():
    ref = R.load()
    RD = ref._cdf_ref_modules["diffusion.forward_process_impl"].DeColorization
    D = R.mine()
    for routine in ("Constant", "Linear"):
        for remove in (True, False):
            for T in (1, 6, 50):
                theirs = RD(decolor_routine=routine, decolor_ema_factor=0.9, decolor_total_remove=remove, num_timesteps=T)
                ours = D.DeColorization(decolor_routine=routine, decolor_ema_factor=0.9, decolor_total_remove=remove, num_timesteps=T)
                assert len(theirs.kernels) == len(ours.kernels) == T
                for i in range(T):
                    assert torch.equal(theirs.kernels[i].weight.detach(), ours.kernels[i]), (routine, remove, T, i)
                    assert torch.equal(ours.table[i], ours.kernels[i][:, :, 0, 0])
