"""The snowification package against vectors the UNMODIFIED reference produced (tests/golden/snow/snow_cases.pt, written by
tests/golden/snow/make_golden_snow.py under the stubs of tests/snow_ref.py):

 (a) where the reference tree exists, the generator reproduces every committed tensor, list and scalar bit for bit (one thread);
 (b) the CPU restatement `state_t` is bit-equal to the fixture wherever the fixture holds the planes of the steps involved;
 (c) the host part of `Snow` (needs scipy) yields the fixture's base layers, blur directions and lists bit for bit, leaves numpy's global
     state alone with `random_snow=False`, and leaves torch's generator where the reference leaves it with `single_snow`;
 (d) the engine (simulator and MI355X): planes <= 2e-6 (tests/test_snow_kernels.py derives the bound); `forward`, `total_forward` and
     `q_sample` <= 4e-6 -- a plane at p and its mirror, 2e-6 each, pass through a sum and a scale by 2 -- and BIT-EQUAL once the
     fixture's planes are injected; losses 1e-5 relative; single network calls 1e-4 (the project's bound).

Trajectories (several network calls fed back through the forward process) follow the measured-tolerance rule of the decolorization
golden tests: the max-abs error against the fixture is printed on both backends and asserted at 4 x the larger value.  Measured
(two 32 x 32 images, T = 20, the tiny network), simulator / MI355X:
                                                   default               x0_step_down
    sample(t=4) `recon`                            3.58e-7 / 3.58e-7     4.77e-7 / 4.17e-7
    all_sample(times=2) last X_t                   4.77e-7 / 4.77e-7     3.58e-7 / 2.98e-7
    forward_and_backward(t=3) final image          4.17e-7 / 3.58e-7     (no sampling routine in it)
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

import snow_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snow")
DECOLOR_GOLD = os.path.join(os.path.dirname(GOLD), "decolor")
PLANE_TOL, STATE_TOL, NET_TOL = 2e-6, 4e-6, 1e-4
T, L = 20, 4
# 4 x max(simulator, MI355X) of the figures in the module docstring
TRAJECTORY_TOL = {("sample", "default"): 4 * 3.58e-7, ("sample", "x0_step_down"): 4 * 4.77e-7, ("all_sample", "default"): 4 * 4.77e-7,
                  ("all_sample", "x0_step_down"): 4 * 3.58e-7, ("forward_and_backward", None): 4 * 4.17e-7}

try:
    import scipy.ndimage  # noqa: F401
    HAVE_SCIPY = True
except ImportError:
    HAVE_SCIPY = False
needs_scipy = pytest.mark.skipif(not HAVE_SCIPY, reason="the host part of Snow needs scipy")

_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = torch.load(os.path.join(GOLD, "snow_cases.pt"), weights_only=False)
    return _cases


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _generator():
    sys.path.insert(0, GOLD)
    try:
        import make_golden_snow
    finally:
        sys.path.remove(GOLD)
    return make_golden_snow


class MBE:
    def __init__(self, kind):
        self.kind = kind
        self.device = torch.device("cuda:0" if kind == "hip" else "cpu")

    def to(self, t):
        return t.to(self.device)


@pytest.fixture(params=[pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)])
def mbe(request):
    from colddiff import runtime
    if request.param == "emu":
        from emu_util import install_emu
        install_emu()
    else:
        runtime._lib_override = None
    yield MBE(request.param)
    runtime._lib_override = None


def err(a, b):
    return (a.detach().cpu() - b).abs().max().item()


def layer_key(level, size, single):
    return f"L{level}_{size}_{'single' if single else 'plain'}"


def fixture_planes(c):
    """[T,L,H,W] with the fixture's planes at the steps it stores (zero elsewhere: a case that read one of those would not be bit-equal)."""
    full = torch.zeros((T,) + tuple(c["planes"].shape[1:]))
    full[list(c["steps"])] = c["planes"]
    return full


# ---------------------------------------------------------------------------------------------------------------------------------------
# (a) the fixture is what the reference produces
# ---------------------------------------------------------------------------------------------------------------------------------------
def _same(path, got, want):
    if isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), path
        for k in want:
            _same(path + "/" + str(k), got[k], want[k])
    elif isinstance(want, torch.Tensor):
        assert got.dtype == want.dtype and torch.equal(got, want), path
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), path
        for i, (a, b) in enumerate(zip(got, want)):
            _same(f"{path}[{i}]", a, b)
    else:
        assert got == want, path


@pytest.mark.skipif(not R.available(), reason="needs the reference tree")
def test_generator_reproduces_the_committed_fixture_bit_for_bit():
    M = _generator()
    _same("snow_cases", quiet(M.generate), cases())
    with open(os.path.join(GOLD, "signatures.json")) as f:
        assert M.signature_case() == json.load(f), "tests/golden/snow/signatures.json is stale: run make_golden_snow.py"
    assert os.path.getsize(os.path.join(GOLD, "snow_cases.pt")) < 1000000


# ---------------------------------------------------------------------------------------------------------------------------------------
# (b) the CPU restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def forward_checks(state, fw, lay):
    """Every no-network case whose planes the fixture stores, as (name, got, want); `state(og, n, key, fix)` -> the rows after n steps
    with the planes of layers[key]."""
    t, t_neg, x13 = fw["t"], fw["t_neg"], fw["x13"]
    n, nmax = R.q_sample_counts(t)
    nn, nnmax = R.q_sample_counts(t_neg)
    out = []
    for key, lk, fix in (("L1", "L1_13_plain", False), ("L1_fix", "L1_13_plain", True), ("L3", "L3_13_plain", False)):
        c = fw[key]
        out += [(key + "/q", state(x13, n, lk, fix), c["q"]), (key + "/total", state(x13, nmax, lk, fix), c["total"]),
                (key + "/q_neg", state(x13, nn, lk, fix), c["q_neg"]),
                (key + "/total_neg", state(x13, [nnmax if v >= 0 else -1 for v in nn], lk, fix), c["total_neg"])]
    out += [("forward_7", state(x13, 8, "L1_13_plain", False), fw["forward_7"]),
            ("total_forward", state(x13, T, "L1_13_plain", False), fw["total_forward"])]
    c = fw["L1_32"]
    out += [("L1_32/q", state(fw["x32"], R.q_sample_counts(c["t"])[0], "L1_32_plain", False), c["q"]),
            ("L1_32/forward_7", state(fw["x32"], 8, "L1_32_plain", False), c["forward_7"])]
    c = fw["L1_single"]
    n4, n4max = R.q_sample_counts(c["t"])
    out += [("L1_single/q", state(c["x"], n4, "L1_13_single", False), c["q"]),
            ("L1_single/total", state(c["x"], n4max, "L1_13_single", False), c["total"])]
    return out


def test_cpu_restatement_is_bit_equal_to_the_fixture():
    fw, lay = cases()["forward"], cases()["layers"]
    assert lay["restated_torchgeometry"] is True

    def state(og, n, key, fix):
        return R.state_t(og, None, n, fixture_planes(lay[key]), lay[key]["br_coef_list"], fix=fix)
    for name, got, want in forward_checks(state, fw, lay):
        assert torch.equal(got, want), name
    assert torch.equal(fw["all_minus_one"], fw["x13"])
    # the planes: the sequential restatement against the reference's convolution
    worst = 0.0
    for key, c in lay.items():
        if not isinstance(c, dict):
            continue
        k = 5 if key.startswith("L1_") else 11
        taps = torch.stack([R.get_gaussian_kernel(k, s) for s in c["mb_sigma_list"]])
        got = R.layers_t(c["base"], torch.tensor(c["snow_thres_list"]), taps, c["vertical"])
        worst = max(worst, err(got[list(c["steps"])], c["planes"]))
    print(f"layers_t against the reference's planes: max-abs {worst:.3g}")
    assert worst <= PLANE_TOL
    # coverage: level 1 step 7 at 32 x 32 clips 9 ... 10 % of the pixels; level 3 step 0 is an empty plane
    assert 0.09 <= (fw["L1_32"]["forward_7"] == 1.0).float().mean().item() <= 0.10
    c = lay["L3_32_plain"]
    assert not (c["planes"][c["steps"].index(0)] != 0).any()


# ---------------------------------------------------------------------------------------------------------------------------------------
# (c) the host part
# ---------------------------------------------------------------------------------------------------------------------------------------
@needs_scipy
def test_host_part_yields_the_reference_draws():
    M = _generator()
    D = R.mine()
    lay = cases()["layers"]
    torch_state, numpy_state = torch.get_rng_state(), np.random.get_state()
    try:
        for level in M.LEVELS:
            for size in M.SIZES:
                for single in (False, True):
                    c = lay[layer_key(level, size, single)]
                    before = np.random.get_state()
                    torch.manual_seed(M.SEED)
                    fp = D.Snow(image_size=(size, size), snow_level=level, num_timesteps=T, single_snow=single, batch_size=L)
                    after = np.random.get_state()
                    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
                    assert torch.equal(fp.snow_base, c["base"]) and torch.equal(fp.vertical, c["vertical"]), (level, size, single)
                    assert fp.snow_thres_list == c["snow_thres_list"] and fp.mb_sigma_list == c["mb_sigma_list"]
                    assert fp.br_coef_list == c["br_coef_list"]
                    if single:
                        if "rng_state" in c:
                            assert torch.equal(torch.get_rng_state(), c["rng_state"])
                        assert torch.equal(torch.rand(8), c["rng_probe"])
        # random_snow=True draws from numpy's global state instead (and moves it)
        np.random.seed(7)
        a = D.Snow(image_size=(13, 13), num_timesteps=T, random_snow=True).snow_base
        moved = np.random.get_state()[1].copy()
        np.random.seed(7)
        b = D.Snow(image_size=(13, 13), num_timesteps=T, random_snow=True).snow_base
        assert torch.equal(a, b) and not torch.equal(a, lay["L1_13_plain"]["base"])
        np.random.seed(7)
        assert not np.array_equal(np.random.get_state()[1], moved)
    finally:
        torch.set_rng_state(torch_state)
        np.random.set_state(numpy_state)


def test_missing_scipy_is_an_import_error_naming_the_option(monkeypatch):
    D = R.mine()
    monkeypatch.setitem(sys.modules, "scipy.ndimage", None)
    with pytest.raises(ImportError, match="forward_process_type='Snow'"):
        D.Snow(image_size=(13, 13), num_timesteps=T)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (d) the engine
# ---------------------------------------------------------------------------------------------------------------------------------------
def _snow_gd(mbe, net, size, **kw):
    D = R.mine()
    torch.manual_seed(_generator().SEED)
    return D.GaussianDiffusion(net, image_size=(size, size), device_of_kernel='cuda', channels=3, timesteps=T, forward_process_type='Snow',
                               results_folder=None, **kw).to(mbe.device)


@needs_scipy
def test_engine_planes(mbe):
    M = _generator()
    D = R.mine()
    lay = cases()["layers"]
    worst = 0.0
    for level in M.LEVELS:
        for size in M.SIZES:
            for single in (False, True):
                c = lay[layer_key(level, size, single)]
                torch.manual_seed(M.SEED)
                fp = D.Snow(image_size=(size, size), snow_level=level, num_timesteps=T, single_snow=single, batch_size=L)
                planes = fp.planes(mbe.device)
                assert planes.shape == (T, L if single else 1, size, size) and planes.device.type == mbe.device.type
                e = err(planes[list(c["steps"])], c["planes"])
                worst = max(worst, e)
                assert e <= PLANE_TOL, (level, size, single, e)
                # the public lists: [L,3,H,W] views of that storage, the rotated ones its 180 degree turn
                assert len(fp.snow) == len(fp.snow_rot) == T and fp.snow[3].shape == (planes.shape[1], 3, size, size)
                assert fp.snow[3].untyped_storage().data_ptr() == planes.untyped_storage().data_ptr()
                assert torch.equal(fp.snow_rot[3], torch.flip(fp.snow[3], dims=[2, 3]))
    print(f"engine planes against the reference's [{mbe.kind}]: max-abs {worst:.3g} (bound {PLANE_TOL:.3g})")


@needs_scipy
@pytest.mark.parametrize("inject", [False, True])
def test_engine_forward_and_q_sample(mbe, inject):
    """Own planes: within 4e-6 of the fixture.  The fixture's planes injected: bit-equal."""
    fw, lay = cases()["forward"], cases()["layers"]
    made = {}

    def gd_for(key, fix):
        if (key, fix) not in made:
            level, size, kind = int(key[1]), int(key.split("_")[1]), key.split("_")[2]
            gd = _snow_gd(mbe, None, size, snow_level=level, fix_brightness=fix, single_snow=kind == "single", batch_size=L)
            if inject:
                gd.forward_process.set_planes(mbe.to(fixture_planes(lay[key])))
            made[(key, fix)] = gd
        return made[(key, fix)]

    def check(name, got, want):
        if inject:
            assert torch.equal(got.cpu(), want), name
        else:
            assert err(got, want) <= STATE_TOL, (name, err(got, want))

    x13 = mbe.to(fw["x13"])
    for key, lk, fix in (("L1", "L1_13_plain", False), ("L1_fix", "L1_13_plain", True), ("L3", "L3_13_plain", False)):
        gd, c = gd_for(lk, fix), fw[key]
        q, tot = gd.q_sample(x13, mbe.to(fw["t"]), return_total_blur=True)
        check(key + "/q", q, c["q"])
        check(key + "/total", tot, c["total"])
        check(key + "/q alone", gd.q_sample(x13, mbe.to(fw["t"])), c["q"])
        q, tot = gd.q_sample(x13, mbe.to(fw["t_neg"]), return_total_blur=True)
        check(key + "/q_neg", q, c["q_neg"])
        check(key + "/total_neg", tot, c["total_neg"])
    gd = gd_for("L1_13_plain", False)
    check("forward_7", gd.forward_process.forward(None, 7, og=x13), fw["forward_7"])
    check("forward_7 (x is ignored)", gd.forward_process.forward(x13 * 0, 7, og=x13), fw["forward_7"])
    check("total_forward", gd.forward_process.total_forward(x13), fw["total_forward"])
    assert torch.equal(gd.q_sample(x13, mbe.to(torch.full((3,), -1))).cpu(), fw["all_minus_one"])
    c = fw["L1_32"]
    gd = gd_for("L1_32_plain", False)
    check("L1_32/q", gd.q_sample(mbe.to(fw["x32"]), mbe.to(c["t"])), c["q"])
    check("L1_32/forward_7", gd.forward_process.forward(None, 7, og=mbe.to(fw["x32"])), c["forward_7"])
    c = fw["L1_single"]
    gd = gd_for("L1_13_single", False)
    q, tot = gd.q_sample(mbe.to(c["x"]), mbe.to(c["t"]), return_total_blur=True)
    check("L1_single/q", q, c["q"])
    check("L1_single/total", tot, c["total"])


def _engine(mbe, **kw):
    D = R.mine()
    sd = torch.load(os.path.join(DECOLOR_GOLD, "decolor_net.pt"), weights_only=False)["state_dict"]
    net = quiet(D.UnetConvNextBlock, dim=8, dim_mults=(1, 2))
    net.load_state_dict(sd, strict=True)
    net = net.to(mbe.device)
    return net, _snow_gd(mbe, net, 32, **kw)


@needs_scipy
@pytest.mark.parametrize("routine", ["Final", "Step", "Step_Gradient"])
def test_engine_train_routines(mbe, routine):
    nc = cases()["network"]
    x, t = mbe.to(nc["x"]), mbe.to(nc["t"])
    net, gd = _engine(mbe, train_routine=routine)
    assert err(gd.q_sample(x, t), nc["x_blur"]) <= STATE_TOL
    assert err(gd.q_sample(x, t - 1), nc["x_blur_sub"]) <= STATE_TOL             # a t == -1 row: the q_sample quirk is on the path
    loss = gd.p_losses(x, t)
    want = nc["routines"][routine]["loss"].item()
    print(f"snow {routine} [{mbe.kind}]: loss {loss.item():.6f} (reference {want:.6f})")
    assert abs(loss.item() - want) <= 1e-5 * max(1.0, abs(want))
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    if routine == "Final":                                                        # forward(): prepare + loss_prepared, same kernels
        torch.manual_seed(3)
        a = gd(x)
        torch.manual_seed(3)
        b = gd.p_losses(x, gd._draw_t(x))
        assert abs(a.item() - b.item()) <= 1e-6


@needs_scipy
@pytest.mark.parametrize("samp", ["default", "x0_step_down"])
def test_engine_trajectories(mbe, samp):
    M = _generator()
    nc = cases()["network"]
    c = nc["samplers"][samp]
    x = mbe.to(nc["x"])
    net, gd = _engine(mbe, sampling_routine=samp)
    net.eval()
    with torch.no_grad():
        out = quiet(gd.sample, batch_size=2, img=x.clone(), t=M.SAMPLE_T)
        assert sorted(out) == ["direct_recons", "recon", "xt"]
        assert err(out["xt"], nc["xt"]) <= STATE_TOL
        assert err(out["direct_recons"], nc["direct_recons"]) <= NET_TOL
        a, _ = gd.sample_one_step(x.clone(), mbe.to(c["one_step_t"]))
        assert err(a, c["one_step_x"]) <= NET_TOL                                 # one network call, one chain
        X0, Xt, init_pred, fwd = gd.all_sample(batch_size=2, img=x.clone(), times=2)
        assert init_pred is None and fwd == [] and len(X0) == len(Xt) == 2 and all(not v.is_cuda for v in X0 + Xt)
    figures = {("sample", samp): err(out["recon"], c["recon"]), ("all_sample", samp): err(Xt[-1], c["all_sample_X_t_last"])}
    if samp == "default":                                                         # (no sampling routine in it: run once)
        with torch.no_grad():
            F, B, last = gd.forward_and_backward(batch_size=2, img=x.clone(), t=M.FB_T)
        w = nc["forward_and_backward"]
        assert (len(F), len(B)) == tuple(w["lengths"]) and err(F[-1], w["Forward_last"]) <= STATE_TOL
        figures[("forward_and_backward", None)] = err(last, w["img"])
    for key, e in figures.items():
        print(f"snow trajectory {key[0]} {samp} [{mbe.kind}]: max-abs {e:.3g} (bound {TRAJECTORY_TOL[key]:.3g})")
    for key, e in figures.items():
        assert e <= TRAJECTORY_TOL[key], (key, e)


@needs_scipy
def test_random_snow_regenerates(mbe):
    nc = cases()["network"]
    x, t = mbe.to(nc["x"]), mbe.to(nc["t"])
    state = np.random.get_state()
    try:
        np.random.seed(11)
        net, gd = _engine(mbe, random_snow=True, batch_size=2)
        fp = gd.forward_process
        seen = []
        for _ in range(2):                                                        # every p_losses rebuilds all T layers
            gd.p_losses(x, t)
            seen.append(fp.planes(mbe.device).cpu().clone())
        assert not torch.equal(seen[0], seen[1]) and (seen[0] != 0).any() and (seen[1] != 0).any()
        gd(x)                                                                     # ... and so does forward() through prepare()
        assert not torch.equal(fp.planes(mbe.device).cpu(), seen[1])
        seen.append(fp.planes(mbe.device).cpu().clone())
        net.eval()
        with torch.no_grad():
            out = quiet(gd.sample, batch_size=2, img=x.clone(), t=1)
        assert fp.batch_size == 2 and not torch.equal(fp.planes(mbe.device).cpu(), seen[2])
        # xt is the forward process on the planes sample() made
        assert torch.equal(out["xt"].cpu(), R.state_t(nc["x"], None, 1, fp.planes(mbe.device).cpu(), fp.br_coef_list))
        # without random_snow nothing is regenerated and batch_size follows only when it is given
        net, gd = _engine(mbe)
        fp = gd.forward_process
        first = fp.planes(mbe.device)
        fp.reset_parameters()
        assert fp.batch_size == 32 and fp.planes(mbe.device) is first
        fp.reset_parameters(batch_size=5)
        assert fp.batch_size == 5 and fp.planes(mbe.device) is first
    finally:
        np.random.set_state(state)


@needs_scipy
def test_single_snow_misuse_raises(mbe):
    gd = _snow_gd(mbe, None, 13, single_snow=True, batch_size=L)
    x = mbe.to(cases()["forward"]["L1_single"]["x"])
    with pytest.raises(RuntimeError, match="single_snow"):                        # t == -1 rows: fewer forwarded rows than layers
        gd.q_sample(x, mbe.to(torch.tensor([3, -1, 0, 9])))
    with pytest.raises(RuntimeError, match="single_snow"):                        # a batch different from batch_size
        gd.q_sample(x[:3], mbe.to(torch.tensor([3, 1, 0])))
    with pytest.raises(RuntimeError, match="single_snow"):
        gd.forward_process.forward(None, 2, og=x[:2])
    gd.denoise_fn = lambda img, t: img
    for samp in ("default", "x0_step_down"):
        gd.sampling_routine = samp
        with pytest.raises(RuntimeError, match="single_snow"):                    # unequal t: rows leave the loop at different steps
            gd.sample_one_step(x, mbe.to(torch.tensor([5, 3, 5, 5])))
        a, b = gd.sample_one_step(x, mbe.to(torch.tensor([5, 5, 5, 5])))          # equal t is the pairing upstream has
        assert a.shape == x.shape and torch.equal(b, x)
    assert torch.equal(gd.q_sample(x, mbe.to(torch.full((4,), -1))), x)           # all rows left out: nothing is forwarded
