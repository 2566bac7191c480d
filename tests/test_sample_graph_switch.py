"""The switch of sampler graph mode without a GPU: on the host simulator a graph-mode call runs the ordinary loop and says why, the
default path reports 'off', and the Trainer's `sample_graph` argument sets the attribute on its EMA core only."""
import contextlib
import io

import torch


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _core():
    from deblurring_diffusion_pytorch import GaussianDiffusion, Unet
    torch.manual_seed(0)
    net = _quiet(Unet, dim=8, dim_mults=(1, 2), channels=1)
    return GaussianDiffusion(net, image_size=8, device_of_kernel="cpu", channels=1, timesteps=4, loss_type="l1", kernel_std=1.0, kernel_size=3,
                             blur_routine="Constant", train_routine="Final", sampling_routine="x0_step_down")


def test_simulator_runs_eager_and_says_why(tmp_path):
    from emu_util import install_emu, uninstall_emu
    from colddiff import diffusion as CD
    install_emu()
    try:
        assert CD.TwoPhase.sample_graph is False                   # COLDDIFF_SAMPLE_GRAPH is not set in the test environment
        d = _core()
        off = {"mode": "off", "reason": "not requested", "captures": 0, "replays": 0}
        img = torch.rand(2, 1, 8, 8) * 2 - 1
        e = d.sample(batch_size=2, img=img)
        assert d.sample_graph_state() == off
        g = d.sample(batch_size=2, img=img, graph=True)
        assert all(torch.equal(a, b) for a, b in zip(e, g))
        assert d.sample_graph_state() == {"mode": "eager", "reason": "library override", "captures": 0, "replays": 0}
        d.drop_sample_graph()
        d2 = _core()
        d2.sample_graph = True                                     # the attribute, read where `graph` is None
        g2 = d2.sample(batch_size=2, img=img)
        assert all(torch.equal(a, b) for a, b in zip(e, g2)) and d2.sample_graph_state()["mode"] == "eager"
        assert _core().sample_graph_state() == off                 # ... set on the instance, not on the class
        d2.all_sample(batch_size=2, img=img, graph=False)          # an explicit False is a plain call: the state keeps the last requested one
        assert d2.sample_graph_state()["reason"] == "library override"
        # the Trainer's argument: the EMA core alone, and None leaves the cores as they are
        from deblurring_diffusion_pytorch import Trainer
        kw = dict(image_size=8, train_batch_size=2, gradient_accumulate_every=1, dataset="synthetic")
        tr = _quiet(Trainer, _core(), None, results_folder=str(tmp_path / "a"), sample_graph=True, **kw)
        assert tr.ema_core.sample_graph is True and tr.core.sample_graph is False
        tr = _quiet(Trainer, _core(), None, results_folder=str(tmp_path / "b"), **kw)
        assert "sample_graph" not in tr.ema_core.__dict__ and tr.ema_core.sample_graph is False
        import copy
        c = copy.deepcopy(d2)                                      # a core that asked for graph mode still copies; the copy captures its own
        assert c.sample_graph is True and c._sample_graph is not d2._sample_graph and c._sample_graph.core is c
    finally:
        uninstall_emu()
