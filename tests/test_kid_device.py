"""KID on the device: `metrics.KidStats`, `kid_distance_device`, `DeviceFidKid` and the two `fid_distance_decrease_from_manifold` sweeps
with it.  Simulator and MI355X.

Reference: tests/kid_ref.py -- the whole procedure in numpy fp64 with torch-fidelity's draws (one RandomState(seed); per subset
choice(n1, m), then choice(n2, m), without replacement) and the rounding-error bound derived in that file's docstring, the one
tests/test_kid_kernel.py holds the kernel to.  `mean` is within the mean of the subsets' bounds of the reference's mean; `std` within their
largest (the standard deviation moves by at most the root mean square of what its inputs move by).
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

import kid_ref as R
import kid_worker as W
from test_decolor_trainer import MBE, mbe, quiet  # noqa: F401  (mbe: the fixture)
from test_fid_device import feat12

HERE = os.path.dirname(os.path.abspath(__file__))


def feats(n, d, seed, scale=1.0, shift=0.0):
    return torch.randn(n, d, generator=torch.Generator().manual_seed(seed)) * scale + shift


def kid_stats(mbe, rows):
    from colddiff import metrics
    return metrics.KidStats(rows.shape[1], mbe.device).add(mbe.to(rows))


def test_accumulation_in_batches_and_merge_equal_the_concatenation(mbe):
    from colddiff import metrics
    d = 40
    parts = [feats(3, d, 1), feats(50, d, 2), feats(0, d, 3), feats(4, d, 4)]
    st = metrics.KidStats(d, mbe.device)
    for p in parts:
        assert st.add(mbe.to(p)) is st
    one = kid_stats(mbe, torch.cat(parts))
    assert st.n == one.n == 57 and torch.equal(st.rows(), one.rows())
    assert st.rows().dtype == torch.float64 and st.rows().device.type == mbe.device.type and st.rows().shape == (57, d)
    assert torch.equal(st.rows().cpu(), torch.cat(parts).double())                          # fp32 features, widened exactly
    # the extractor's other output forms: a list, a not yet pooled 4-D map
    maps = mbe.to(torch.rand(6, d, 2, 3))
    assert torch.equal(metrics.KidStats(d, mbe.device).add([maps]).rows(), kid_stats(mbe, maps.mean((2, 3))).rows())
    # merge: the other's rows below one's own, the other left as it is
    a, b = kid_stats(mbe, parts[0]), kid_stats(mbe, parts[1])
    assert a.merge(b) is a and a.merge(metrics.KidStats(d, mbe.device)) is a
    assert a.n == 53 and b.n == 50 and torch.equal(a.rows(), kid_stats(mbe, torch.cat(parts[:2])).rows())
    assert torch.equal(b.rows().cpu(), parts[1].double())
    empty = metrics.KidStats(d, mbe.device)
    assert empty.n == 0 and empty.rows().shape == (0, d) and empty.all_reduce() is empty
    with pytest.raises(ValueError, match="dims"):
        a.merge(metrics.KidStats(d + 1, mbe.device))
    with pytest.raises(AssertionError):
        a.add(mbe.to(feats(2, d + 1, 5)))
    # add_images: the extractor batch by batch, the trailing partial batch included
    imgs = mbe.to(torch.rand(7, 3, 8, 8, generator=torch.Generator().manual_seed(6)))
    by_images = metrics.KidStats(12, mbe.device).add_images(imgs, feat12, batch_size=3)
    assert by_images.n == 7 and torch.equal(by_images.rows(), kid_stats(mbe, feat12(imgs)).rows())


def test_subset_draws_against_the_numpy_statement_and_the_global_stream_untouched(mbe):
    from colddiff import metrics
    n1, n2, d, subsets, m, seed = 90, 75, 40, 4, 60, 2020
    x, y = feats(n1, d, 11), feats(n2, d, 12, 1.2, 0.1)
    s1, s2 = kid_stats(mbe, x), kid_stats(mbe, y)
    np.random.seed(123)
    state = np.random.get_state()
    mean, std = metrics.kid_distance_device(s1, s2, subsets=subsets, subset_size=m, seed=seed)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:], "numpy's global stream moved"
    vals, bnds = R.kid(x.double().numpy(), y.double().numpy(), subsets, m, seed)
    print(f"kid_distance_device [{mbe.kind}]: mean {mean:.12g} (numpy {np.mean(vals):.12g}, bound {bnds.mean():.3g}), "
          f"std {std:.12g} (numpy {np.std(vals):.12g}, bound {bnds.max():.3g})")
    assert isinstance(mean, float) and isinstance(std, float)
    assert abs(mean - np.mean(vals)) <= bnds.mean() and abs(std - np.std(vals)) <= bnds.max()
    assert std > 1e3 * bnds.max(), "the subsets do not differ: the draws are not exercised"
    assert metrics.kid_distance_device(s1, s2, subsets=subsets, subset_size=m, seed=seed) == (mean, std)
    assert metrics.kid_distance_device(s1, s2, subsets=subsets, subset_size=m, seed=seed + 1) != (mean, std)
    ix, iy = metrics.kid_subset_indices(n1, n2, subsets, m, seed)
    rng = np.random.RandomState(seed)
    for s in range(subsets):
        assert np.array_equal(ix[s], rng.choice(n1, m, replace=False)) and np.array_equal(iy[s], rng.choice(n2, m, replace=False))


def test_known_values_identical_sets_and_shifted_means(mbe):
    from colddiff import metrics
    d, n = 40, 70
    x = feats(n, d, 21)
    s = kid_stats(mbe, x)
    same, same_std = metrics.kid_distance_device(s, kid_stats(mbe, x), subsets=3, subset_size=50, seed=1)
    _, bnds = R.kid(x.double().numpy(), x.double().numpy(), 3, 50, 1)
    print(f"kid(s, s) [{mbe.kind}] = {same:.6g} +- {same_std:.3g} (bound {bnds.mean():.3g})")
    assert same <= bnds.mean(), "the unbiased estimator of identical sets came out clearly positive"
    # every row on both sides (one subset, the whole sets): sxx = syy and sxy = sxx + the diagonal, so mmd2 = -2 (mean k(x_i, x_i) - mean
    # off-diagonal k) / m < 0 whatever the draw order
    whole, _ = metrics.kid_distance_device(s, kid_stats(mbe, x), subsets=1, subset_size=None, seed=1)
    assert whole < 0
    far, _ = metrics.kid_distance_device(s, kid_stats(mbe, x + 1.0), subsets=3, subset_size=50, seed=1)
    print(f"kid(s, s + 1) [{mbe.kind}] = {far:.6g}")
    assert far > 0.5 and far > 1e6 * bnds.mean()


def test_subset_size_contract(mbe):
    from colddiff import metrics
    s1, s2 = kid_stats(mbe, feats(30, 16, 31)), kid_stats(mbe, feats(20, 16, 32))
    mean, std = metrics.kid_distance_device(s1, s2, subsets=2, subset_size=None, seed=3)      # None: min(n1, n2) = 20
    assert (mean, std) == metrics.kid_distance_device(s1, s2, subsets=2, subset_size=20, seed=3)
    with pytest.raises(ValueError, match=r"subset_size = 21 .* min\(30, 20\) = 20"):
        metrics.kid_distance_device(s1, s2, subsets=2, subset_size=21, seed=3)
    with pytest.raises(ValueError, match=r"subset_size = 1000 .* min\(30, 20\) = 20"):       # the default against small sets
        metrics.kid_distance_device(s1, s2)
    with pytest.raises(ValueError, match=r"subset_size = 1 must be at least 2"):
        metrics.kid_distance_device(s1, s2, subset_size=1)


def test_device_fid_kid_feeds_both_metrics_from_one_extractor_pass(mbe):
    from colddiff import metrics
    from test_fid_device import Counting
    g = torch.Generator().manual_seed(9)
    A = mbe.to(torch.rand(40, 3, 8, 8, generator=g))
    B = mbe.to(torch.rand(40, 3, 8, 8, generator=g) * 0.5 + 0.1 * torch.rand(40, 3, 1, 1, generator=g))
    model = Counting(feat12)
    both = metrics.DeviceFidKid(model=model, dims=12, batch_size=16, device=str(mbe.device), kid_subsets=3, kid_subset_size=25, kid_seed=4)
    sa, sb = both.stats(A), both.stats(B)
    assert model.images == 80, "more than one extractor pass per set"
    assert isinstance(sa, metrics.FidStats) and sa.n == sa.kid_stats.n == 40
    plain = metrics.DeviceFid(model=feat12, dims=12, batch_size=16, device=str(mbe.device))
    assert both.distance(sa, sb) == plain.distance(plain.stats(A), plain.stats(B)) == both(samples=[A, B])
    ka, kb = metrics.KidStats(12, mbe.device).add_images(A, feat12, 16), metrics.KidStats(12, mbe.device).add_images(B, feat12, 16)
    assert torch.equal(sa.kid_stats.rows(), ka.rows())
    assert both.kid(sa, sb) == metrics.kid_distance_device(ka, kb, subsets=3, subset_size=25, seed=4)
    assert not hasattr(plain, "kid")
    dflt = metrics.DeviceFidKid(model=feat12, dims=12, device=str(mbe.device))
    assert (dflt.kid_subsets, dflt.kid_subset_size, dflt.kid_seed) == (100, 1000, 2020)      # torch-fidelity's defaults
    merged = both.new_stats().merge(sa).merge(sb)
    assert merged.n == merged.kid_stats.n == 80 and torch.equal(merged.kid_stats.rows(), torch.cat((ka.rows(), kb.rows())))


# ---- the two Trainer sweeps -----------------------------------------------------------------------------------------------------------
def check_sweep(mbe, run):
    """`run(fid_func)` -> result dict, printing.  A DeviceFidKid adds kid_* / kid_std_* beside every fid_*; a plain DeviceFid returns and
    prints exactly what the DeviceFidKid run does without those keys and lines."""
    from colddiff import metrics
    kw = dict(model=feat12, dims=12, batch_size=50, device=str(mbe.device))
    texts, outs = [], []
    for fid in (metrics.DeviceFidKid(kid_subsets=3, kid_subset_size=None, kid_seed=7, **kw), metrics.DeviceFid(**kw)):
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            outs.append(run(fid))
        texts.append(text.getvalue())
    with_kid, plain = outs
    names = ("blur", "deblur", "direct_deblur")
    assert sorted(plain) == sorted(f"{m}_{n}" for m in ("fid", "rmse", "ssim") for n in names)
    assert sorted(with_kid) == sorted(list(plain) + [f"{m}_{n}" for m in ("kid", "kid_std") for n in names])
    keys = list(with_kid)
    for n in names:
        assert keys.index(f"kid_{n}") == keys.index(f"fid_{n}") + 1 and keys.index(f"kid_std_{n}") == keys.index(f"fid_{n}") + 2
        assert isinstance(with_kid[f"kid_{n}"], float) and isinstance(with_kid[f"kid_std_{n}"], float) and with_kid[f"kid_std_{n}"] >= 0
    assert [k for k in keys if k in plain] == list(plain) and all(with_kid[k] == plain[k] for k in plain)
    kid_lines = [ln for ln in texts[0].splitlines() if ln.startswith("The KID of")]
    assert len(kid_lines) == 3 and "The KID of" not in texts[1]
    assert [ln for ln in texts[0].splitlines() if not ln.startswith("The KID of")] == texts[1].splitlines()
    for n, ln in zip(names, kid_lines):
        assert ln.endswith(f" images with original image is {with_kid[f'kid_{n}']} +- {with_kid[f'kid_std_{n}']}")
    return with_kid


def test_eval_mixin_sweep_adds_kid_beside_fid(mbe, tmp_path):
    """The Trainer of tests/test_fid_device.py::test_eval_mixin_sweep_fed_per_batch on 4 of its 8 images, in batches of 2."""
    import eval_worker
    from test_data import _write_images
    folder = str(tmp_path / "imgs")
    _write_images(folder, 8)
    tr = eval_worker.build_deblur(mbe.device, folder, str(tmp_path / "res"))
    check_sweep(mbe, lambda fid: tr.fid_distance_decrease_from_manifold(fid_func=fid, start=-1, end=3, batch=2))


def test_decolor_sweep_adds_kid_beside_fid(mbe, tmp_path):
    """The Trainer of tests/test_fid_device.py::test_decolor_sweep_fed_per_batch on 4 of its 20 images, in batches of 2."""
    from test_decolor_snow_eval import numpy_seed, trainer_of
    tr, imgs, M = trainer_of(mbe, "decolor", "rgb", tmp_path)

    def run(fid):
        with numpy_seed(M.NP_SEED):
            return tr.fid_distance_decrease_from_manifold(fid, start=M.START, end=M.START + 4, eval_batch_size=2)

    check_sweep(mbe, run)


# ---- two ranks --------------------------------------------------------------------------------------------------------------------------
def test_all_reduce_on_two_ranks_gives_every_rank_the_single_process_matrix(mbe, tmp_path):
    """One `torch.distributed.run` launch of tests/kid_worker.py (gloo; both ranks on cuda:0 in the hardware run, as
    tests/test_eval_sharded.py): unequal row counts through FidKidStats, one rank empty, every rank empty."""
    from colddiff import metrics
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "w.pt")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(HERE, "kid_worker.py"), out, mbe.kind]
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0", COLDDIFF_SHARE_GPU="1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ranks = [torch.load(out + f".rank{i}", weights_only=False) for i in range(2)]
    other = W.other_set(mbe.device)
    for case in ("unequal", "one_empty"):
        single = torch.cat([W.rows_of(case, rank) for rank in range(2)]).double()
        want = metrics.kid_distance_device(kid_stats(mbe, single.float()), other, **W.KID)
        for rank, res in enumerate(ranks):
            assert res[case]["n"] == single.shape[0] and torch.equal(res[case]["rows"], single), (case, rank)
            assert res[case]["kid"] == want, (case, rank, res[case]["kid"], want)
        assert ranks[0][case]["kid"] == ranks[1][case]["kid"]
    assert ranks[0]["unequal"]["fid_n"] == ranks[1]["unequal"]["fid_n"] == sum(W.ROWS["unequal"])
    assert torch.equal(ranks[0]["unequal"]["mean"], ranks[1]["unequal"]["mean"])
    assert all(res["all_empty"] == {"n": 0, "shape": (0, W.DIMS)} for res in ranks)
