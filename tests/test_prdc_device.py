"""Precision / recall / density / coverage on the device: `metrics.knn_sq`, `ball_counts`, `prdc_device`, `DeviceFidKidPrdc` and the two
`fid_distance_decrease_from_manifold` sweeps with it.  Simulator and MI355X.

Reference: tests/prdc_ref.py -- the definitions by brute force in numpy fp64 and the rounding bound of a squared distance derived in that
file's docstring.  The four numbers are ratios of integer counts; a count is exact when no pair lies within its bound of its radius, which
every comparison here first asserts of its data on the reference alone (`ambiguous_prdc(...) == 0`), so all five numbers must `==`.
"""
import contextlib
import io
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import prdc_ref as R
import prdc_worker as W
from test_decolor_trainer import MBE, mbe, quiet  # noqa: F401  (mbe: the fixture)
from test_fid_device import feat12

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("precision", "recall", "density", "coverage", "f_score")
_sets = {}


def feats(n, d, seed, scale=1.0, shift=0.0):
    return torch.randn(n, d, generator=torch.Generator().manual_seed(seed)) * scale + shift


def two_sets():
    """The originals X [130, 72] and the candidates Y [70, 72] with the reference's five numbers per k; made once."""
    if not _sets:
        x, y = feats(130, 72, 41), feats(70, 72, 42, 1.1, 0.1)
        hx, hy = x.double().numpy(), y.double().numpy()
        _sets.update(x=x, y=y, hx=hx, hy=hy, want={k: R.prdc(hx, hy, k) for k in (3, 5)})
        assert all(R.ambiguous_prdc(hx, hy, k) == 0 for k in (3, 5)), "a pair of the case lies within the rounding bound of its radius"
    return _sets


def kid_stats(mbe, rows):
    from colddiff import metrics
    return metrics.KidStats(rows.shape[1], mbe.device).add(mbe.to(rows))


@pytest.mark.parametrize("k", [3, 5])
def test_prdc_device_equals_the_numpy_statement(mbe, k):
    from colddiff import metrics
    c = two_sets()
    got = metrics.prdc_device(kid_stats(mbe, c["x"]), kid_stats(mbe, c["y"]), k)
    print(f"prdc_device [{mbe.kind}, k = {k}]: {got} (numpy {c['want'][k]})")
    assert tuple(got) == KEYS and all(isinstance(got[q], float) for q in KEYS)
    assert got == c["want"][k]
    assert 0 < got["precision"] < 1 and 0 < got["coverage"] < 1 and got["density"] > 0, "the case does not exercise the counts"
    assert metrics.prdc_device(kid_stats(mbe, c["x"]), kid_stats(mbe, c["y"]), k) == got


def test_wrappers_take_any_row_pitch_and_return_none_for_the_side_not_asked_for(mbe):
    from colddiff import metrics
    c = two_sets()
    wide = torch.full((130, 80), float("nan"), dtype=torch.float64)
    wide[:, :72] = c["x"].double()
    x, y = mbe.to(wide)[:, :72], mbe.to(c["y"].double())
    assert x.stride(0) == 80
    knn = metrics.knn_sq(x, 3)
    assert knn.shape == (130, 3) and knn.dtype == torch.float64
    assert (np.abs(knn.cpu().numpy() - R.knn(c["hx"], 3)).max(1) <= R.knn_bound(c["hx"])).all()
    assert torch.equal(knn, metrics.knn_sq(x, 3, norms=metrics.row_norms_sq(x)))
    rho_x, rho_y = mbe.to(torch.from_numpy(R.knn(c["hx"], 3)[:, 2].copy())), mbe.to(torch.from_numpy(R.knn(c["hy"], 3)[:, 2].copy()))
    col, row = metrics.ball_counts(x, y, rcol=rho_y, rrow=rho_x)
    wcol, wrow = R.ball_counts(c["hx"], c["hy"], rho_y.cpu().numpy(), rho_x.cpu().numpy())
    assert col.dtype == row.dtype == torch.int32 and np.array_equal(col.cpu().numpy(), wcol) and np.array_equal(row.cpu().numpy(), wrow)
    only_col, none = metrics.ball_counts(x, y, rcol=rho_y)
    assert none is None and torch.equal(only_col, col)
    none, only_row = metrics.ball_counts(x, y, rrow=rho_x, anorm=metrics.row_norms_sq(x), bnorm=metrics.row_norms_sq(y))
    assert none is None and torch.equal(only_row, row)


def test_known_values_a_set_against_itself_and_against_a_far_copy(mbe):
    from colddiff import metrics
    x = feats(70, 40, 21)
    s = kid_stats(mbe, x)
    same = metrics.prdc_device(s, kid_stats(mbe, x), 3)
    print(f"prdc(s, s) [{mbe.kind}] = {same}")
    assert same["precision"] == same["recall"] == same["coverage"] == same["f_score"] == 1.0 and same["density"] >= 1.0
    far = metrics.prdc_device(s, kid_stats(mbe, x + 100.0), 3)
    assert far == dict(precision=0.0, recall=0.0, density=0.0, coverage=0.0, f_score=0.0)


def test_permuting_the_rows_of_either_set_changes_nothing(mbe):
    from colddiff import metrics
    c = two_sets()
    px, py = torch.randperm(130, generator=torch.Generator().manual_seed(1)), torch.randperm(70, generator=torch.Generator().manual_seed(2))
    for x, y in ((c["x"][px], c["y"]), (c["x"], c["y"][py]), (c["x"][px], c["y"][py])):
        assert metrics.prdc_device(kid_stats(mbe, x), kid_stats(mbe, y), 3) == c["want"][3]


def test_add_in_batches_and_merge_equal_the_concatenation(mbe):
    from colddiff import metrics
    c = two_sets()
    sx = metrics.KidStats(72, mbe.device)
    for part in (c["x"][:7], c["x"][7:64], c["x"][64:64], c["x"][64:]):
        sx.add(mbe.to(part))
    sy = kid_stats(mbe, c["y"][:33]).merge(kid_stats(mbe, c["y"][33:]))
    assert sx.n == 130 and sy.n == 70
    assert metrics.prdc_device(sx, sy, 3) == c["want"][3]


def test_small_sets_and_k_out_of_range_are_a_value_error(mbe):
    from colddiff import metrics
    s4, s9 = kid_stats(mbe, feats(4, 16, 31)), kid_stats(mbe, feats(9, 16, 32))
    assert set(metrics.prdc_device(s4, s9, 3)) == set(KEYS)                               # n = k + 1 is enough
    with pytest.raises(ValueError, match=r"k = 4 .* k \+ 1 rows \(got 4 and 9\)"):
        metrics.prdc_device(s4, s9, 4)
    with pytest.raises(ValueError, match=r"k = 4 .* k \+ 1 rows \(got 9 and 4\)"):
        metrics.prdc_device(s9, s4, 4)
    with pytest.raises(ValueError, match=r"k = 3 .* \(got 9 and 0\)"):
        metrics.prdc_device(s9, metrics.KidStats(16, mbe.device))
    for k in (0, 9, -1):
        with pytest.raises(ValueError, match=r"k = %d must be in 1\.\.\.8" % k):
            metrics.prdc_device(kid_stats(mbe, feats(20, 16, 33)), kid_stats(mbe, feats(20, 16, 34)), k)


def test_device_fid_kid_prdc_feeds_every_metric_from_one_extractor_pass(mbe):
    from colddiff import metrics
    from test_fid_device import Counting
    g = torch.Generator().manual_seed(9)
    A = mbe.to(torch.rand(40, 3, 8, 8, generator=g))
    B = mbe.to(torch.rand(40, 3, 8, 8, generator=g) * 0.5 + 0.1 * torch.rand(40, 3, 1, 1, generator=g))
    model = Counting(feat12)
    kw = dict(dims=12, batch_size=16, device=str(mbe.device), kid_subsets=3, kid_subset_size=25, kid_seed=4)
    full = metrics.DeviceFidKidPrdc(model=model, prdc_k=2, **kw)
    sa, sb = full.stats(A), full.stats(B)
    assert model.images == 80, "more than one extractor pass per set"
    kid = metrics.DeviceFidKid(model=feat12, **kw)
    ka, kb = kid.stats(A), kid.stats(B)
    assert full.distance(sa, sb) == kid.distance(ka, kb) and full.kid(sa, sb) == kid.kid(ka, kb)
    got = full.prdc(sa, sb)
    assert model.images == 80
    assert got == metrics.prdc_device(ka.kid_stats, kb.kid_stats, 2)
    ha, hb = (t.kid_stats.rows().cpu().numpy() for t in (ka, kb))
    assert R.ambiguous_prdc(ha, hb, 2) == 0 and got == R.prdc(ha, hb, 2)
    assert not hasattr(kid, "prdc")
    dflt = metrics.DeviceFidKidPrdc(model=feat12, dims=12, device=str(mbe.device))
    assert (dflt.kid_subsets, dflt.kid_subset_size, dflt.kid_seed, dflt.prdc_k) == (100, 1000, 2020, 3)
    assert metrics.DeviceFidKidPrdc(feat12, 12, 16, str(mbe.device), 3, 25, 4, 5).prdc_k == 5             # trailing, after DeviceFidKid's


# ---- the two Trainer sweeps -----------------------------------------------------------------------------------------------------------
def check_sweep(mbe, run):
    """`run(fid_func)` -> result dict, printing.  A DeviceFidKidPrdc adds the five keys per candidate set after kid_std_*; a DeviceFidKid
    returns and prints exactly what the DeviceFidKidPrdc run does without those keys and lines."""
    from colddiff import metrics
    kw = dict(model=feat12, dims=12, batch_size=50, device=str(mbe.device), kid_subsets=3, kid_subset_size=None, kid_seed=7)
    texts, outs = [], []
    for fid in (metrics.DeviceFidKidPrdc(prdc_k=2, **kw), metrics.DeviceFidKid(**kw)):
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            outs.append(run(fid))
        texts.append(text.getvalue())
    with_prdc, plain = outs
    names = ("blur", "deblur", "direct_deblur")
    assert sorted(plain) == sorted(f"{m}_{n}" for m in ("fid", "kid", "kid_std", "rmse", "ssim") for n in names)
    assert sorted(with_prdc) == sorted(list(plain) + [f"{m}_{n}" for m in KEYS for n in names])
    keys = list(with_prdc)
    for n in names:
        assert [keys.index(f"{m}_{n}") - keys.index(f"kid_std_{n}") for m in KEYS] == [1, 2, 3, 4, 5]
        assert all(isinstance(with_prdc[f"{m}_{n}"], float) and with_prdc[f"{m}_{n}"] >= 0 for m in KEYS)
        assert all(with_prdc[f"{m}_{n}"] <= 1 for m in ("precision", "recall", "coverage", "f_score"))
    assert [k for k in keys if k in plain] == list(plain) and all(with_prdc[k] == plain[k] for k in plain)
    lines = [ln for ln in texts[0].splitlines() if ln.startswith("The precision / recall / density / coverage / F-score of")]
    assert len(lines) == 3 and "precision" not in texts[1]
    assert [ln for ln in texts[0].splitlines() if ln not in lines] == texts[1].splitlines()
    for n, ln in zip(names, lines):
        assert ln.endswith(" images with original image is " + " / ".join(str(with_prdc[f"{m}_{n}"]) for m in KEYS))
    kid_at = [i for i, ln in enumerate(texts[0].splitlines()) if ln.startswith("The KID of")]
    assert all(texts[0].splitlines()[i + 1] in lines for i in kid_at), "the line does not follow the KID line"
    return with_prdc


def test_eval_mixin_sweep_adds_the_five_keys_beside_fid_and_kid(mbe, tmp_path):
    """The Trainer of tests/test_kid_device.py::test_eval_mixin_sweep_adds_kid_beside_fid: 4 images in batches of 2."""
    import eval_worker
    from test_data import _write_images
    folder = str(tmp_path / "imgs")
    _write_images(folder, 8)
    tr = eval_worker.build_deblur(mbe.device, folder, str(tmp_path / "res"))
    check_sweep(mbe, lambda fid: tr.fid_distance_decrease_from_manifold(fid_func=fid, start=-1, end=3, batch=2))


def test_decolor_sweep_adds_the_five_keys_beside_fid_and_kid(mbe, tmp_path):
    """The Trainer of tests/test_kid_device.py::test_decolor_sweep_adds_kid_beside_fid: 4 images in batches of 2."""
    from test_decolor_snow_eval import numpy_seed, trainer_of
    tr, imgs, M = trainer_of(mbe, "decolor", "rgb", tmp_path)

    def run(fid):
        with numpy_seed(M.NP_SEED):
            return tr.fid_distance_decrease_from_manifold(fid, start=M.START, end=M.START + 4, eval_batch_size=2)

    out = check_sweep(mbe, run)
    assert out["precision_blur"] == out["precision_blur"]                                 # (a float, not NaN)


# ---- two ranks --------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_with_unequal_row_counts_give_the_single_process_numbers(mbe, tmp_path):
    """One `torch.distributed.run` launch of tests/prdc_worker.py (gloo; both ranks on cuda:0 in the hardware run, as
    tests/test_kid_device.py): the candidates' rows come together through `FidKidStats.all_reduce`."""
    from colddiff import metrics
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "w.pt")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(HERE, "prdc_worker.py"), out, mbe.kind]
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0", COLDDIFF_SHARE_GPU="1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ranks = [torch.load(out + f".rank{i}", weights_only=False) for i in range(2)]
    single = torch.cat([W.rows_of(rank) for rank in range(2)])
    orig = W.originals(mbe.device)
    hx, hy = orig.rows().cpu().numpy(), single.double().numpy()
    for k in W.KS:
        want = metrics.prdc_device(orig, kid_stats(mbe, single), k)
        assert R.ambiguous_prdc(hx, hy, k) == 0 and want == R.prdc(hx, hy, k)
        for rank, res in enumerate(ranks):
            assert res["n"] == sum(W.ROWS) and res["prdc"][k] == want, (k, rank, res["prdc"][k], want)
