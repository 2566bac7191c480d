"""LPIPS on the device: `colddiff.lpips.AlexNetFeatures` / `LPIPS`, `metrics.LpipsStats` / `DeviceLpips` and the two
`fid_distance_decrease_from_manifold` sweeps with `lpips=`.  Simulator and MI355X.

Reference: tests/lpips_ref.py, the definition in torch, fp32 and fp64, with a random AlexNet whose biases keep every feature vector away
from zero (asserted on the reference alone before anything is compared: every pixel norm at every tap >= 0.1 x that tap's median).
* taps: 2e-4 * max(1, |ref|max) against the fp32 restatement, the tolerance tests/test_inception.py holds the same GEMM kernels to; in
  the default arithmetic mode nothing tighter applies.
* end to end under precision_scope('f32'): g = the largest relative gap between the restatement's own fp32 and fp64 distances over all
  cases (32 ... 128 pixels, both weight seeds); |d - d64| <= 8 g d64, the factor 8 being the margin tests/test_gmm_device.py gives
  summation-order noise.
"""
import contextlib
import copy
import io
import os
import socket
import subprocess
import sys

import pytest
import torch

import lpips_ref as R
import lpips_worker as W
from test_decolor_trainer import MBE, Recorder, mbe, quiet  # noqa: F401  (mbe: the fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
B = 3
SEEDS = (11, 12)
SIZES = (32, 48, 64, 128)
GPU = pytest.mark.gpu
# (backend, size): the simulator runs the two small sizes, the hardware all four
WHERE = [pytest.param("emu", s, id=f"emu-{s}") for s in SIZES[:2]] + [pytest.param("hip", s, marks=GPU, id=f"hip-{s}") for s in SIZES]
NAMES = ("blur", "deblur", "direct_deblur")
_cases, _models = {}, {}


def weights(seed):
    return R.random_alexnet(seed), R.random_lins(seed + 100)


def case(size, seed):
    """Originals and two candidate sets [B,3,size,size] in [-1, 1], the restatement's fp32 taps of the originals and its fp32 / fp64
    distances; made once."""
    key = (size, seed)
    if key not in _cases:
        g = torch.Generator().manual_seed(1000 * seed + size)
        yy, xx = torch.meshgrid(torch.linspace(-1, 1, size), torch.linspace(-1, 1, size), indexing="ij")
        base = torch.stack([xx, yy, (xx + yy) / 2])[None] * torch.rand(B, 3, 1, 1, generator=g)
        x = (base + 0.5 * (torch.rand(B, 3, size, size, generator=g) - 0.5)).clamp(-1, 1)
        cands = [(x + s * torch.randn(x.shape, generator=g)).clamp(-1, 1) for s in (0.5, 0.05)]
        sd, lins = weights(seed)
        d32 = torch.stack([R.lpips(sd, lins, x, c).flatten() for c in cands])
        d64 = torch.stack([R.lpips(sd, lins, x, c, dtype=torch.float64).flatten() for c in cands])
        ratio = min(R.norm_ratio(sd, z) for z in [x] + cands)
        _cases[key] = dict(x=x, cands=cands, taps=R.taps(sd, R.scale_input(x)), d32=d32, d64=d64, ratio=ratio)
    return _cases[key]


def model_of(mbe, seed):
    from colddiff.lpips import LPIPS
    key = (mbe.kind, seed)
    if key not in _models:
        sd, lins = weights(seed)
        _models[key] = LPIPS(weights=sd, lin=lins).to(mbe.device)
    return _models[key]


# ---- taps ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("mbe,size", WHERE, indirect=["mbe"])
def test_the_five_taps_match_the_fp32_restatement(mbe, size, seed):
    c = case(size, seed)
    taps = model_of(mbe, seed).features(mbe.to(c["x"]))
    assert [t.shape[-1] for t in taps] == [64, 192, 384, 256, 256]
    for k, (got, want) in enumerate(zip(taps, c["taps"])):
        assert got.shape == want.permute(0, 2, 3, 1).shape
        err = (got.cpu() - want.permute(0, 2, 3, 1)).abs().max().item()
        tol = 2e-4 * max(1.0, want.abs().max().item())
        print(f"tap {k} [{mbe.kind}, {size} px, seed {seed}] {tuple(got.shape)}: error {err:.3g} (tolerance {tol:.3g})")
        assert err <= tol


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def fp32_gap():
    """g: the largest relative gap between the restatement's fp32 and fp64 distances over every case, after the condition of the data."""
    worst = 0.0
    for size in SIZES:
        for seed in SEEDS:
            c = case(size, seed)
            assert c["ratio"] >= 0.1, f"a pixel norm of the {size}-pixel case, seed {seed}, is {c['ratio']:.3g} x its tap's median"
            worst = max(worst, float(((c["d32"].double() - c["d64"]).abs() / c["d64"]).max()))
    return worst


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("mbe,size", WHERE, indirect=["mbe"])
def test_distances_in_f32_mode_within_eight_times_the_restatements_own_fp32_gap(mbe, size, seed):
    from colddiff import runtime as rt
    g = fp32_gap()
    c = case(size, seed)
    with rt.precision_scope('f32'):
        d = model_of(mbe, seed).distances(mbe.to(c["x"]), [mbe.to(z) for z in c["cands"]])
    assert d.shape == (2, B) and d.dtype == torch.float64 and d.device.type == mbe.device.type
    rel = ((d.cpu() - c["d64"]).abs() / c["d64"]).max().item()
    print(f"lpips [{mbe.kind}, f32 mode, {size} px, seed {seed}]: distances {c['d64'].min().item():.4g} ... {c['d64'].max().item():.4g}, "
          f"largest relative error {rel:.3g}, g = {g:.3g}, smallest norm ratio {c['ratio']:.3g}")
    assert rel <= 8 * g


# ---- API -----------------------------------------------------------------------------------------------------------------------------------
def test_forward_distances_normalize_and_one_channel_input_agree(mbe):
    c = case(32, SEEDS[0])
    m = model_of(mbe, SEEDS[0])
    x, y = mbe.to(c["x"][:2]), mbe.to(c["cands"][0][:2])
    d = m.distances(x, [y, x])
    assert torch.equal(d[1], torch.zeros(2, dtype=torch.float64, device=d.device)), "an image against itself is not at distance 0"
    out = m(x, y)
    assert out.shape == (2, 1, 1, 1) and out.dtype == torch.float32
    assert torch.equal(out.flatten(), d[0].float()), "forward and distances differ, or a distance depends on the other candidates"
    # normalize=True on [0, 1] input: (x + 1) / 2 then 2 x - 1 is within an ulp of x, so equal up to that
    d01 = m.distances((x + 1) * 0.5, [(y + 1) * 0.5], normalize=True)[0]
    assert ((d01 - d[0]).abs() <= 1e-5 * d[0]).all()
    back = lambda z: 2 * ((z + 1) * 0.5) - 1
    assert torch.equal(d01, m.distances(back(x), [back(y)])[0]), "normalize=True is not 2 x - 1 in front of the same arithmetic"
    # one channel, as the sweeps repeat it to three
    g1, h1 = x[:, :1].contiguous(), y[:, :1].contiguous()
    assert torch.equal(m.distances(g1, [h1]), m.distances(g1.repeat(1, 3, 1, 1), [h1.repeat(1, 3, 1, 1)]))


def test_loading_the_two_layouts_missing_files_and_what_is_not_built(mbe, tmp_path, monkeypatch):
    from colddiff import lpips as LP
    sd, lins = weights(SEEDS[1])
    m = LP.LPIPS(weights=sd, lin=lins)                                        # dicts; `classifier.*` of the torchvision dict is ignored
    own = m.net.state_dict()
    assert sorted(own) == sorted(k for k in sd if k.startswith("features."))
    assert all(torch.equal(own[k], sd[k]) for k in own)
    assert all(torch.equal(m.lins[k], lins[f"lin{k}.model.1.weight"].flatten()) for k in range(5))
    wfile, lfile = str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth")
    torch.save(sd, wfile)
    torch.save(lins, lfile)
    for args in (dict(weights=wfile, lin=lfile), dict()):                     # paths; then the two environment variables
        if not args:
            monkeypatch.setenv("COLDDIFF_LPIPS_WEIGHTS", wfile)
            monkeypatch.setenv("COLDDIFF_LPIPS_LIN", lfile)
        m2 = LP.LPIPS(**args)
        assert all(torch.equal(v, own[k]) for k, v in m2.net.state_dict().items()) and all(torch.equal(a, b) for a, b in zip(m2.lins, m.lins))
    monkeypatch.delenv("COLDDIFF_LPIPS_WEIGHTS")
    monkeypatch.delenv("COLDDIFF_LPIPS_LIN")
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    for args in (dict(), dict(weights=str(tmp_path / "nothing.pth"), lin=lfile), dict(weights=wfile), dict(weights="random")):
        with pytest.raises(FileNotFoundError, match=r"(?s)alexnet-owt-7be5be79\.pth.*alex\.pth"):
            LP.LPIPS(**args)
    bad = dict(lins)
    del bad["lin3.model.1.weight"]
    with pytest.raises(AssertionError, match="lin3"):
        LP.LPIPS(weights=sd, lin=bad)
    with pytest.raises(AssertionError, match="missing"):
        LP.LPIPS(weights={k: v for k, v in sd.items() if k != "features.8.bias"}, lin=lins)
    for kw in (dict(net="vgg"), dict(net="squeeze"), dict(spatial=True)):
        with pytest.raises(NotImplementedError):
            LP.LPIPS(weights="random", lin="random", **kw)
    x = mbe.to(case(32, SEEDS[0])["x"])
    with pytest.raises(NotImplementedError, match="gradient"):
        model_of(mbe, SEEDS[0])(x.clone().requires_grad_(), x)
    from colddiff import metrics
    with pytest.raises(FileNotFoundError):
        metrics.DeviceLpips(device=str(mbe.device))
    held = metrics.DeviceLpips(device=str(mbe.device), weights=sd, lin=lins)
    assert isinstance(held.model, LP.LPIPS) and held.new_stats(NAMES).names == NAMES


# ---- LpipsStats ----------------------------------------------------------------------------------------------------------------------------
def test_batches_of_unequal_size_and_merge_in_either_order_equal_the_one_pass_mean(mbe):
    from colddiff import metrics
    c = case(32, SEEDS[0])
    m = model_of(mbe, SEEDS[0])
    x, cands = mbe.to(c["x"]), [mbe.to(z) for z in c["cands"]]
    want = m.distances(x, cands).cpu()
    mean = {f"lpips_{n}": want[k].sum().item() / B for k, n in enumerate(("blur", "deblur"))}

    def part(lo, hi):
        st = metrics.LpipsStats(("blur", "deblur"))
        st.add(x[lo:hi], [z[lo:hi] for z in cands], m)
        return st

    p02, p23 = part(0, 2), part(2, 3)
    st = copy.deepcopy(p02)
    st.add(x[2:], [z[2:] for z in cands], m)
    assert st.count == B and st.sums.dtype == torch.float64 and st.sums.device.type == mbe.device.type
    empty = lambda: metrics.LpipsStats(("blur", "deblur"))
    for got in (st.result(), copy.deepcopy(p02).merge(p23).result(), copy.deepcopy(p23).merge(p02).result(),
                empty().merge(st).result(), copy.deepcopy(st).merge(empty()).result()):
        assert list(got) == list(mean)
        assert all(got[k] == pytest.approx(mean[k], rel=1e-14) for k in mean)            # (the same fp64 terms in another order)
    with pytest.raises(AssertionError):
        metrics.LpipsStats(("blur",)).result()
    with pytest.raises(AssertionError):
        p02.merge(metrics.LpipsStats(("blur",)))


def test_two_ranks_with_unequal_counts_give_the_single_process_numbers(mbe, tmp_path):
    """One `torch.distributed.run` launch of tests/lpips_worker.py (gloo; both ranks on cuda:0 in the hardware run, as
    tests/test_eval_sharded.py): rank 0 holds one image, rank 1 two."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "w.pt")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(HERE, "lpips_worker.py"), out, mbe.kind]
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0", COLDDIFF_SHARE_GPU="1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ranks = [torch.load(out + f".rank{i}", weights_only=False) for i in range(2)]
    model = W.model_on(mbe.device)
    single = W.stats_of(0, model, mbe.device).merge(W.stats_of(1, model, mbe.device))   # rank order, as all_reduce adds
    want = single.result()
    assert single.count == sum(W.IMAGES) and all(v > 0 for v in want.values())
    for rank, res in enumerate(ranks):
        assert res["count"] == single.count and torch.equal(res["sums"], single.sums.cpu()) and res["result"] == want, (rank, res, want)


# ---- the two Trainer sweeps ----------------------------------------------------------------------------------------------------------------
class KeepingLpips:
    """A DeviceLpips whose LpipsStats remembers the batches it was fed."""

    def __init__(self, model):
        from colddiff import metrics
        self.model, self.fed = model, []
        outer = self

        class Keeping(metrics.LpipsStats):
            def add(self, orig, cands, model):
                outer.fed.append((orig.clone(), [c.clone() for c in cands]))
                return super().add(orig, cands, model)

        self.new_stats = Keeping


def check_sweep(mbe, run, word_of):
    """`run(**kw)` -> result dict, printing.  With lpips= the sweep adds `lpips_<name>` and one line per name and nothing else changes;
    the values are LPIPS.distances of the very sets the sweep fed, averaged; without it no cdf_lpips_* entry point is called."""
    from colddiff import runtime as rt
    model = model_of(mbe, SEEDS[0])
    keep = KeepingLpips(model)
    texts, outs = [], []
    for kw in (dict(lpips=keep), dict(lpips=None), dict()):
        text = io.StringIO()
        with contextlib.redirect_stdout(text), Recorder(rt.lib()) as rec:
            outs.append(run(**kw))
        texts.append(text.getvalue())
        called = sorted({n for n in rec.calls if n.startswith("cdf_lpips")})
        assert called == (["cdf_lpips_layer", "cdf_lpips_layer_blocks", "cdf_lpips_prep_nhwc"] if kw.get("lpips") else []), called
    with_lpips, none, plain = outs
    assert none == plain and texts[1] == texts[2]
    assert sorted(with_lpips) == sorted(list(plain) + [f"lpips_{n}" for n in NAMES])
    assert all(with_lpips[k] == plain[k] for k in plain)
    lines = [ln for ln in texts[0].splitlines() if ln.startswith("The LPIPS of")]
    assert len(lines) == 3 and "LPIPS" not in texts[1]
    assert [ln for ln in texts[0].splitlines() if ln not in lines] == texts[1].splitlines()
    for n, ln in zip(NAMES, lines):
        assert ln == f"The LPIPS of {word_of[n]} images with original image is {with_lpips[f'lpips_{n}']}"
    assert len(keep.fed) == 2 and [o.shape[0] for o, _ in keep.fed] == [2, 1], "the sweep did not feed two batches of 2 and 1 images"
    assert all(o.shape[1] == 3 and float(o.min()) >= -1 and float(o.min()) < 0 and len(cs) == 3 for o, cs in keep.fed)
    total = sum(model.distances(o, cs).sum(1) for o, cs in keep.fed).cpu()
    for k, n in enumerate(NAMES):
        assert with_lpips[f"lpips_{n}"] == pytest.approx(total[k].item() / 3, rel=1e-12) and with_lpips[f"lpips_{n}"] > 0
    return with_lpips


def test_eval_mixin_sweep_adds_lpips_and_changes_nothing_else(mbe, tmp_path):
    """The deblurring Trainer of tests/eval_worker.py at 32 pixels: 3 images in batches of 2."""
    from deblurring_diffusion_pytorch import GaussianDiffusion, Trainer, Unet
    from test_data import _write_images
    folder = str(tmp_path / "imgs")
    _write_images(folder, 8)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        net = Unet(dim=8, dim_mults=(1, 2), channels=3).to(mbe.device)
        d = GaussianDiffusion(net, image_size=32, device_of_kernel=str(mbe.device), channels=3, timesteps=3, kernel_size=3, kernel_std=0.5,
                              sampling_routine="x0_step_down").to(mbe.device)
        tr = Trainer(d, folder, image_size=32, train_batch_size=4, train_num_steps=1, dataset="train", results_folder=str(tmp_path / "res"),
                     num_workers=0, device_data=True)
    from colddiff import metrics
    from test_fid_device import feat12
    # beside a DeviceFid: the run without lpips= is then on the same per-batch path, and every other number must be the same number
    fid = metrics.DeviceFid(model=feat12, dims=12, batch_size=50, device=str(mbe.device))
    out = check_sweep(mbe, lambda **kw: tr.fid_distance_decrease_from_manifold(fid_func=fid, start=-1, end=2, batch=2, **kw), {n: n for n in NAMES})
    # without a fid_func lpips= alone sends the sweep down that path: the same LPIPS, RMSE / SSIM within the bounds tests/test_eval.py holds
    # the per-batch sums to against the whole-set metrics
    alone = quiet(tr.fid_distance_decrease_from_manifold, fid_func=None, start=-1, end=2, batch=2, lpips=metrics.DeviceLpips(model_of(mbe, SEEDS[0])))
    whole = quiet(tr.fid_distance_decrease_from_manifold, fid_func=None, start=-1, end=2, batch=2)
    assert sorted(alone) == sorted(list(whole) + [f"lpips_{n}" for n in NAMES])
    for n in NAMES:
        assert alone[f"lpips_{n}"] == out[f"lpips_{n}"]
        assert abs(alone[f"rmse_{n}"] - whole[f"rmse_{n}"]) <= 2e-5 and abs(alone[f"ssim_{n}"] - whole[f"ssim_{n}"]) <= 1e-4
    with pytest.raises(ValueError, match="new_stats"):
        tr.fid_distance_decrease_from_manifold(fid_func=lambda samples: 0.0, start=-1, end=2, batch=2, lpips=KeepingLpips(None))


@pytest.mark.parametrize("pkg", ["decolor", "snow"])
def test_decolor_and_snow_sweeps_add_lpips_and_change_nothing_else(mbe, tmp_path, pkg):
    """The decolorization / snowification Trainer on 32-pixel images: 3 images in batches of 2."""
    import decolor_ref
    import snow_ref
    from test_decolor_snow_eval import HAVE_SCIPY, numpy_seed
    if pkg == "snow" and not HAVE_SCIPY:
        pytest.skip("the host part of Snow needs scipy")
    D = decolor_ref.mine() if pkg == "decolor" else snow_ref.mine()
    torch.manual_seed(5)
    net = quiet(D.UnetConvNextBlock, dim=8, dim_mults=(1, 2)).to(mbe.device).eval()
    kw = {} if pkg == "decolor" else dict(forward_process_type='Snow', snow_level=1, results_folder=None)
    gd = quiet(D.GaussianDiffusion, net, image_size=(32, 32), device_of_kernel='cuda', channels=3, timesteps=3,
               sampling_routine='x0_step_down', **kw).to(mbe.device)
    tr = quiet(D.Trainer, gd, None, image_size=(32, 32), train_batch_size=2, train_num_steps=1, dataset='synthetic',
               results_folder=str(tmp_path / "res"), num_workers=0)
    imgs = case(32, SEEDS[1])["x"]

    class ListDS(torch.utils.data.Dataset):
        def __len__(self):
            return 8

        def __getitem__(self, i):
            return imgs[i % B].roll(i, 2)

    tr.ds = ListDS()

    def run(**kw):
        torch.manual_seed(9)
        with numpy_seed(77):
            return tr.fid_distance_decrease_from_manifold(None, start=0, end=3, eval_batch_size=2, **kw)

    check_sweep(mbe, run, dict(blur="blurry", deblur="deblurred", direct_deblur="direct deblurred"))
    with pytest.raises(ValueError, match="new_stats"):
        tr.fid_distance_decrease_from_manifold(lambda samples: 0.0, start=0, end=3, eval_batch_size=2, lpips=KeepingLpips(None))
