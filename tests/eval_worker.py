"""Worker for tests/test_eval_sharded.py: one rank of a sharded evaluation sweep under `torch.distributed.run`, and the builders of the
Trainers, which the test's single-process reference runs share.

argv: out_path backend case folder
  backend  "emu": CPU tensors on the simulator, gloo;  "hip": every rank on cuda:0 with the product library, gloo carrying the device
           tensors;  "rccl": rank r on cuda:r, RCCL
  case     "deblur": the deblurring Trainer on the images of `folder`; the sweep with shard=True for batches of 2, 3 and 8 with a
                     DeviceFid on the stand-in extractor, with fid_func=None, and with a plain callable (which must be refused)
           "decolor": the decolorization Trainer on its 20-image fixture, eval_batch_size=8, numpy seeded per rank
           "save":   sample_and_save_for_fid(shard=True, num_samples=8, bs=2) of the denoising Trainer
Every rank stores {name: {"out": the dict, "text": what it printed, "stats": the four FidStats as (n, pivot, sum, outer)}} in
out_path.rank<r>.
"""
import contextlib
import io
import os
import pathlib
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, "cold-diffusion-models_amd"), HERE, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEBLUR_BATCHES = (2, 3, 8)
DECOLOR_BATCH = 8
SAVE_N, SAVE_BS = 8, 2


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


class Dev:
    def __init__(self, device):
        self.device = torch.device(device)
        self.kind = "hip" if self.device.type == "cuda" else "emu"

    def to(self, t):
        return t.to(self.device)


def keeping_fid(device):
    """A DeviceFid on the 12-feature stand-in extractor that remembers the FidStats it hands out."""
    from colddiff import metrics
    from test_fid_device import feat12

    class KeepingFid(metrics.DeviceFid):
        def __init__(self):
            super().__init__(model=feat12, dims=12, batch_size=50, device=str(device))
            self.made = []

        def new_stats(self):
            self.made.append(super().new_stats())
            return self.made[-1]

    return KeepingFid()


def stats_of(fid):
    return [(st.n, st.pivot.cpu().clone(), st.sum.cpu().clone(), st.outer.cpu().clone()) for st in fid.made[-4:]]


def build_deblur(device, folder, res):
    """The Trainer of tests/test_fid_device.py::test_eval_mixin_sweep_fed_per_batch."""
    from deblurring_diffusion_pytorch import GaussianDiffusion, Trainer, Unet
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        net = Unet(dim=8, dim_mults=(1, 2), channels=3).to(device)
        d = GaussianDiffusion(net, image_size=16, device_of_kernel=str(device), channels=3, timesteps=3, kernel_size=3, kernel_std=0.5,
                              sampling_routine="x0_step_down").to(device)
        return Trainer(d, folder, image_size=16, train_batch_size=4, train_num_steps=1, dataset="train", results_folder=res, num_workers=0,
                       device_data=True)


def build_decolor(device, res):
    """The Trainer of tests/test_fid_device.py::test_decolor_sweep_fed_per_batch -> (trainer, the generator module with its constants)."""
    from test_decolor_snow_eval import trainer_of
    os.makedirs(res, exist_ok=True)
    tr, _, M = trainer_of(Dev(device), "decolor", "rgb", pathlib.Path(res))
    return tr, M


def build_denoise(device, folder, res):
    from denoising_diffusion_pytorch import GaussianDiffusion, Trainer, Unet
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        net = Unet(dim=8, dim_mults=(1, 2), channels=3).to(device)
        d = GaussianDiffusion(net, image_size=16, channels=3, timesteps=3).to(device)
        return Trainer(d, folder, image_size=16, train_batch_size=2, results_folder=res, device_data=False, num_workers=0)


def run_sweep(sweep, fid, **kw):
    """-> {"out", "text", "stats"} of one sweep call."""
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        out = sweep(fid, **kw)
    return {"out": out, "text": text.getvalue(), "stats": stats_of(fid) if fid is not None else None}


def deblur_sweeps(tr, device, shard):
    """The sub-cases of "deblur" by name (also what the single-process reference runs, with shard=False)."""
    res = {}
    sweep = lambda fid, **kw: tr.fid_distance_decrease_from_manifold(fid_func=fid, start=-1, end=7, shard=shard, **kw)
    for b in DEBLUR_BATCHES:
        res[f"batch{b}"] = run_sweep(sweep, keeping_fid(device), batch=b)
    res["none"] = run_sweep(sweep, None, batch=2)
    return res


def main():
    out_path, backend, case, folder = sys.argv[1:5]
    rccl, on_hip = backend == "rccl", backend in ("hip", "rccl")
    device = torch.device("cuda:%d" % (int(os.environ.get("LOCAL_RANK", "0")) if rccl else 0)) if on_hip else torch.device("cpu")
    if not on_hip:
        from emu_util import install_emu
        install_emu()
    from colddiff import parallel
    parallel.init_distributed("nccl" if rccl else "gloo")
    rank = parallel.rank()
    res_dir = os.path.join(os.path.dirname(out_path), "res_" + case)                  # (one folder for every rank: `save` fills it together)
    if case == "deblur":
        tr = build_deblur(device, folder, res_dir)
        res = deblur_sweeps(tr, device, shard=True)
        try:
            quiet(tr.fid_distance_decrease_from_manifold, fid_func=lambda samples: 0.0, start=-1, end=7, batch=2, shard=True)
            res["plain"] = "no error"
        except ValueError as e:
            res["plain"] = "ValueError: " + str(e)
    elif case == "decolor":
        tr, M = build_decolor(device, res_dir)
        np.random.seed(M.NP_SEED + 1000 * rank)                                       # rank 0's permutation must be the one every rank walks
        res = {"decolor": run_sweep(lambda fid, **kw: tr.fid_distance_decrease_from_manifold(fid, **kw), keeping_fid(device),
                                    start=M.START, end=M.END, eval_batch_size=DECOLOR_BATCH, shard=True)}
        res["next_numpy_draw"] = float(np.random.rand())                              # ... while this rank's numpy stream advanced by its own
    else:
        assert case == "save"
        tr = build_denoise(device, folder, res_dir)
        names, save = [], tr._save

        def logged(img, name, nrow=6):
            names.append(os.path.basename(str(name)))
            return save(img, name, nrow=nrow)

        tr._save = logged
        count = quiet(tr.sample_and_save_for_fid, shard=True, num_samples=SAVE_N, bs=SAVE_BS)
        res = {"count": count, "names": names, "folder": f"{tr.results_folder}_out"}
    if on_hip:
        torch.cuda.synchronize()
    torch.save(res, out_path + f".rank{rank}")
    torch.distributed.barrier()


if __name__ == "__main__":
    main()
