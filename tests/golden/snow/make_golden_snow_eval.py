"""Generator of tests/golden/snow/snow_eval.pt: the evaluation methods of the reference Trainer of snowification/diffusion
(diffusion.py:764-959, 1000-1145), unmodified, on a fixed in-memory dataset -- the harness, sizes and records of
tests/golden/decolor/make_golden_decolor_eval.py (`run_case` is imported from there) around a `forward_process_type='Snow'` diffusion.
Needs the reference tree and scipy; the tests read only the .pt file.

    python tests/golden/snow/make_golden_snow_eval.py

Cases: `snow_level=1` with `fix_brightness` off ("plain": sweep, test_from_data, the two windows of paper_invert_section_images) and on
("fix": sweep, test_from_data), `sampling_routine='x0_step_down'`, 16 x 16, T = 3, the network of decolor_net.pt.  The snow planes are
the ones the constructor draws after `torch.manual_seed(SEED)` (tests/test_snow_golden.py holds the engine's to them); the motion-blur
taps go through torchgeometry's RESTATED Gaussian (snow_ref.py), like every snow fixture.
"""
import contextlib
import io
import os
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(os.path.dirname(HERE))
REPO = os.path.dirname(TESTS)
DECOLOR = os.path.join(os.path.dirname(HERE), "decolor")
for p in (TESTS, REPO, DECOLOR):
    if p not in sys.path:
        sys.path.insert(0, p)

import snow_ref as R  # noqa: E402
from make_golden_decolor_eval import S, SAMPLING, SEED, T, THREADS, run_case  # noqa: E402


def _gd(ref, sd, **kw):
    m = ref._cdf_ref_modules
    with contextlib.redirect_stdout(io.StringIO()):
        net = m["diffusion.model.unet_convnext"].UnetConvNextBlock(dim=8, dim_mults=(1, 2))
        net.load_state_dict(sd, strict=True)
        torch.manual_seed(SEED)
        return m["diffusion.diffusion"].GaussianDiffusion(net.eval(), image_size=(S, S), device_of_kernel='cuda', channels=3, timesteps=T,
                                                          sampling_routine=SAMPLING, forward_process_type='Snow', snow_level=1,
                                                          results_folder=tempfile.gettempdir(), **kw)


def generate():
    ref = R.load()
    sd = torch.load(os.path.join(DECOLOR, "decolor_net.pt"), weights_only=False)["state_dict"]
    threads, state = torch.get_num_threads(), torch.get_rng_state()
    torch.set_num_threads(THREADS)
    try:
        shared = {}
        return {"restated_torchgeometry": True,
                "plain": run_case(ref._cdf_ref_modules, _gd(ref, sd), False, True, shared),
                "fix": run_case(ref._cdf_ref_modules, _gd(ref, sd, fix_brightness=True), False, False, shared)}
    finally:
        torch.set_num_threads(threads)
        torch.set_rng_state(state)


def main():
    assert R.available(), "needs the reference tree"
    path = os.path.join(HERE, "snow_eval.pt")
    torch.save(generate(), path)
    print(os.path.basename(path), os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
