"""Evaluation sweeps sharded over ranks: `FidStats.merge` / `all_reduce`, `PairStats.merge` / `all_reduce`, and the `shard=True` keyword of
the two `fid_distance_decrease_from_manifold` sweeps and of `sample_and_save_for_fid`.  Simulator and MI355X.

Single process: merged statistics against ONE instance fed every row -- `==` on dyadic features (integers in [-8, 8], power-of-two first
batches: every term is a small dyadic rational, see tests/test_fid_merge_kernel.py), within that file's derived bound
(|dcov| <= 16 n 2^-53 R^2, |dmean| <= 8 n 2^-53 R) on the random features of tests/test_fid_device.py.

Two ranks: launched through `torch.distributed.run` as tests/test_dp.py::_two_rank_case launches its runs (COLDDIFF_SHARE_GPU=1, gloo,
both ranks on cuda:0 in the hardware runs; a subprocess timeout); one launch per Trainer runs its sub-cases (tests/eval_worker.py).  The
parent runs the same sweeps in one process and checks
  * both ranks return `==` dicts and hold bit-identical merged FidStats;
  * RMSE / SSIM within 2 K 2^-53 relative of the single-process PairStats values, K = the number of batches: the same K same-sign fp64
    per-batch sums, added in two orders, each order rounding at most K - 1 times;
  * every FID within 2e-6 Tr sqrt(C1 C2) (tests/test_fid_device.py's `fid_tolerance`, the trace by the eigenvalue route on the
    single-process statistics) of the single-process value;
  * rank 1 printed none of the result lines, rank 0 all of them.
"""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_worker as W
from test_decolor_trainer import MBE, mbe, quiet  # noqa: F401  (mbe: the fixture)
from test_fid_device import eig_route, features
from test_fid_kernels import U

HERE = os.path.dirname(os.path.abspath(__file__))
RESULT_WORDS = ("The RMSE of", "The SSIM of", "The FID of", "Hence the improvement")


# ---- one process ------------------------------------------------------------------------------------------------------------------------
def dyadic(n, d, seed):
    return torch.randint(-8, 9, (n, d), generator=torch.Generator().manual_seed(seed)).float()


def fed(mbe, d, batches):
    from colddiff import metrics
    st = metrics.FidStats(d, mbe.device)
    for b in batches:
        st.add(mbe.to(b))
    return st


def same_stats(a, b):
    return a.n == b.n and torch.equal(a.pivot, b.pivot) and torch.equal(a.mean(), b.mean()) and torch.equal(a.cov(), b.cov()) \
        and torch.equal(a.sum, b.sum)


def test_merge_equals_one_instance_fed_everything_on_dyadic_features(mbe):
    """d = 72 (two tiles); first batches of 8 and 4 rows; three parts, chained."""
    d = 72
    a, b, c = [dyadic(8, d, 1), dyadic(13, d, 2)], [dyadic(4, d, 3), dyadic(21, d, 4)], [dyadic(2, d, 5)]
    one = fed(mbe, d, a + b + c)
    sb = fed(mbe, d, b)
    keep = (sb.n, sb.pivot.clone(), sb.sum.clone(), sb.outer.clone())
    merged = fed(mbe, d, a)
    assert merged.merge(sb) is merged and merged.merge(fed(mbe, d, c)) is merged
    assert same_stats(merged, one), "merge differs from one instance fed every batch"
    assert sb.n == keep[0] and all(torch.equal(x, y) for x, y in zip((sb.pivot, sb.sum, sb.outer), keep[1:])), "merge changed `other`"


def test_merge_of_random_features_within_the_derived_bound(mbe):
    from colddiff import metrics
    d, n_a, n_b = 72, 50, 37
    fa, fb = features(d, n_a, 31, 0.1), features(d, n_b, 32, 0.25)
    merged, other = fed(mbe, d, [fa]), fed(mbe, d, [fb])
    merged.merge(other)
    allf = torch.cat((fa, fb)).numpy().astype(np.longdouble)
    n = n_a + n_b
    mean = allf.mean(0)
    cov = ((allf - mean).T @ (allf - mean)) / (n - 1)
    R = max(np.abs(allf - p.cpu().numpy().astype(np.longdouble)).max() for p in (merged.pivot, other.pivot))
    dm = float(np.abs(merged.mean().cpu().numpy() - mean).max())
    dc = float(np.abs(merged.cov().cpu().numpy() - cov).max())
    print(f"FidStats.merge [{mbe.kind}] (50 + 37, 72): |dmean| {dm:.3g} (bound {8 * n * U * R:.3g}), |dcov| {dc:.3g} (bound {16 * n * U * R * R:.3g})")
    assert merged.n == n and dm <= 8 * n * U * R and dc <= 16 * n * U * R * R
    # the distance of merged against unmerged statistics of the same rows: zero within fid_tolerance
    one = fed(mbe, d, [fa, fb])
    ref = fed(mbe, d, [features(d, 60, 33, 0.4)])
    (m1, c1), (m2, c2) = one.result(), ref.result()
    tol = 2e-6 * eig_route(m1, c1, m2, c2)[1]
    got, want = metrics.frechet_distance_device(merged, ref), metrics.frechet_distance_device(one, ref)
    print(f"    fid(merged, ref) {got:.9g}, fid(one, ref) {want:.9g}, difference {abs(got - want):.3g} (tolerance {tol:.3g})")
    assert abs(got - want) <= tol


def test_merge_empty_frozen_mismatched_and_loaded_statistics(mbe, tmp_path):
    from colddiff import metrics
    d = 40
    a, b = dyadic(8, d, 11), dyadic(16, d, 12)
    sa, sb = fed(mbe, d, [a]), fed(mbe, d, [b])
    # other empty: a no-op
    before = (sa.n, sa.pivot.clone(), sa.sum.clone(), sa.outer.clone())
    sa.merge(metrics.FidStats(d, mbe.device))
    assert sa.n == before[0] and all(torch.equal(x, y) for x, y in zip((sa.pivot, sa.sum, sa.outer), before[1:]))
    # self empty: adopts a COPY
    fresh = metrics.FidStats(d, mbe.device).merge(sb)
    assert same_stats(fresh, sb) and fresh.pivot.data_ptr() != sb.pivot.data_ptr() and fresh.outer.data_ptr() != sb.outer.data_ptr()
    fresh.add(mbe.to(a))
    assert sb.n == 16 and fresh.n == 24
    # dims mismatch
    with pytest.raises(ValueError, match="dims"):
        sa.merge(metrics.FidStats(d + 1, mbe.device))
    # loaded statistics: frozen as a target, pivot = mu / sum = 0 / outer = (n - 1) sigma as a source
    path = str(tmp_path / "b.npz")
    sb.save(path)
    loaded = metrics.FidStats.load(path, mbe.device)
    with pytest.raises(RuntimeError, match="frozen"):
        loaded.merge(sa)
    with pytest.raises(RuntimeError, match="frozen"):
        loaded.add(mbe.to(a))
    via_file, direct = fed(mbe, d, [a]).merge(loaded), fed(mbe, d, [a]).merge(sb)
    n = 24                                                        # (`direct` is exact on this data; the file's mu / sigma carry a few roundings)
    R = float(max((torch.cat((a, b)).double() - p.cpu()).abs().max() for p in (sa.pivot, sb.pivot, loaded.mean())))
    assert via_file.n == n
    assert (via_file.mean() - direct.mean()).abs().max().item() <= 8 * n * U * R
    assert (via_file.cov() - direct.cov()).abs().max().item() <= 16 * n * U * R * R
    # a file without n cannot be weighed
    mu, sigma = sb.result()
    bare = str(tmp_path / "bare.npz")
    with open(bare, "wb") as f:
        np.savez(f, mu=mu, sigma=sigma)
    with pytest.raises(ValueError, match="without n"):
        fed(mbe, d, [a]).merge(metrics.FidStats.load(bare, mbe.device))


def test_all_reduce_without_a_process_group_returns_self_unchanged(mbe):
    from colddiff import metrics
    assert not torch.distributed.is_initialized()
    st = fed(mbe, 40, [dyadic(8, 40, 21)])
    before = (st.pivot, st.sum, st.outer, st.sum.clone(), st.outer.clone())
    assert st.all_reduce() is st and st.n == 8
    assert all(x is y for x, y in zip((st.pivot, st.sum, st.outer), before[:3])), "all_reduce replaced a tensor without a process group"
    assert torch.equal(st.sum, before[3]) and torch.equal(st.outer, before[4])
    ps = metrics.PairStats(("a",))
    assert ps.all_reduce() is ps and ps.sums is None and ps.count == 0


def test_pair_stats_merge_equals_one_instance_fed_every_batch(mbe):
    from colddiff import metrics
    g = torch.Generator().manual_seed(77)
    x = mbe.to(torch.randint(0, 256, (7, 3, 20, 21), generator=g).float() / 255 * 2 - 1)
    cands = [(x + s * mbe.to(torch.randn(x.shape, generator=g))).clamp(-1, 1) for s in (0.6, 0.05)]
    names = ("blur", "deblur")
    one, a, b = metrics.PairStats(names), metrics.PairStats(names), metrics.PairStats(names)
    for st, (lo, hi) in ((one, (0, 3)), (one, (3, 7)), (a, (0, 3)), (b, (3, 7))):
        st.add(x[lo:hi], [c[lo:hi] for c in cands])
    assert a.merge(b) is a and a.merge(metrics.PairStats(names)) is a                        # (an instance without a batch adds nothing)
    assert torch.equal(a.sums, one.sums) and a.count == one.count and a.positions == one.positions and a.result() == one.result()
    empty = metrics.PairStats(names).merge(b)
    assert torch.equal(empty.sums, b.sums) and empty.count == b.count and empty.sums.data_ptr() != b.sums.data_ptr()


# ---- two ranks --------------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gpu_count():
    return torch.cuda.device_count() if torch.cuda.is_available() else 0


_runs = {}


def two_ranks(tmp_path_factory, backend, case):
    """One `torch.distributed.run` launch of tests/eval_worker.py per (backend, case) -> ([rank 0's results, rank 1's], image folder)."""
    key = (backend, case)
    if key not in _runs:
        from test_data import _write_images
        tmp = tmp_path_factory.mktemp(f"sharded_{backend}_{case}")
        folder = str(tmp / "imgs")
        _write_images(folder, 8)
        out = str(tmp / "w.pt")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), os.path.join(HERE, "eval_worker.py"), out, backend, case, folder]
        env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
        if backend != "rccl":
            env["COLDDIFF_SHARE_GPU"] = "1"                       # (both ranks on cuda:0 in the hip runs)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        _runs[key] = ([torch.load(out + f".rank{i}", weights_only=False) for i in range(2)], folder, tmp)
    return _runs[key]


_refs = {}


def deblur_reference(mbe, folder, tmp):
    """The single-process sweeps of the same Trainer: the DeviceFid sweeps per batch size and the plain fid_func=None sweep."""
    if mbe.kind not in _refs:
        tr = W.build_deblur(mbe.device, folder, str(tmp / "res_single"))
        _refs[mbe.kind] = W.deblur_sweeps(tr, mbe.device, shard=False)
    return _refs[mbe.kind]


def check_sharded(ranks, ref, nbatch, fid_ref=None, what=""):
    """`ranks`: the two ranks' {"out", "text", "stats"}; `ref`: the single-process one whose RMSE / SSIM come from PairStats; `fid_ref`:
    the single-process one with the FIDs and the four FidStats (None: a sweep without FID)."""
    r0, r1 = ranks
    assert r0["out"] == r1["out"], what + ": the ranks return different dicts"
    if fid_ref is not None:
        assert list(r0["out"]) == list(fid_ref["out"]), what
    rel = 2 * nbatch * U
    for k, v in r0["out"].items():
        if k.startswith("fid_"):
            continue
        want = ref["out"][k]
        print(f"sharded {what} {k}: {v!r} against {want!r}, relative difference {abs(v - want) / abs(want):.3g} (bound {rel:.3g})")
        assert abs(v - want) <= rel * abs(want), (what, k, v, want)
    if fid_ref is not None:
        assert sorted(k for k in r0["out"] if k.startswith("fid_")) == ["fid_blur", "fid_deblur", "fid_direct_deblur"]
        for (n0, *t0), (n1, *t1), (ns, *_) in zip(r0["stats"], r1["stats"], fid_ref["stats"]):
            assert n0 == n1 == ns and all(torch.equal(x, y) for x, y in zip(t0, t1)), what + ": the ranks' merged FidStats differ"
        single = []
        for n, pivot, s, outer in fid_ref["stats"]:
            from colddiff import metrics
            st = metrics.FidStats(12, "cpu")
            st.n, st.pivot, st.sum, st.outer = n, pivot, s, outer
            single.append(st.result())
        for j, name in enumerate(("blur", "deblur", "direct_deblur")):
            tol = 2e-6 * eig_route(*single[0], *single[j + 1])[1]
            got, want = r0["out"][f"fid_{name}"], fid_ref["out"][f"fid_{name}"]
            print(f"sharded {what} fid_{name}: {got:.9g} against {want:.9g}, difference {abs(got - want):.3g} (tolerance {tol:.3g})")
            assert isinstance(got, float) and abs(got - want) <= tol, (what, name)
    assert all(w in r0["text"] for w in RESULT_WORDS[:2]) and not any(w in r1["text"] for w in RESULT_WORDS), (what, r1["text"])
    assert ("The FID of" in r0["text"]) == (fid_ref is not None)


def run_deblur_case(mbe, tmp_path_factory, backend, sub):
    ranks, folder, tmp = two_ranks(tmp_path_factory, backend, "deblur")
    ref = deblur_reference(mbe, folder, tmp)
    if sub == "none":
        # fid_func=None: RMSE / SSIM only.  Sharded they are PairStats' (fp64 sums of the per-tile partials): held to the single-process
        # PairStats values of the same four batches; the single-process fid_func=None path reduces the concatenated sets in fp32 and is
        # met within 1e-5 relative, the bound tests/test_fid_device.py::test_eval_mixin_sweep_fed_per_batch derives for the two routes.
        check_sharded([r["none"] for r in ranks], ref["batch2"], 4, what="deblur fid_func=None")
        assert sorted(ranks[0]["none"]["out"]) == sorted(ref["none"]["out"])
        for k, v in ranks[0]["none"]["out"].items():
            assert abs(v - ref["none"]["out"][k]) <= 1e-5 * abs(ref["none"]["out"][k]), k
    elif sub == "plain":
        for r in ranks:
            assert r["plain"].startswith("ValueError") and "DeviceFid" in r["plain"], r["plain"]
    else:
        b = int(sub)
        check_sharded([r[f"batch{b}"] for r in ranks], ref[f"batch{b}"], -(-8 // b), fid_ref=ref[f"batch{b}"], what=f"deblur batches of {b}")


DEBLUR_SUBS = ["2", "3", "8", "none", "plain"]      # 4 batches, 2 per rank; 3 batches, rank 1 one short batch; 1 batch, rank 1 none


def test_deblur_sweep_on_two_ranks(mbe, tmp_path_factory):
    """One launch, five sweeps (every sub-case is checked and named in its failure message)."""
    for sub in DEBLUR_SUBS:
        run_deblur_case(mbe, tmp_path_factory, mbe.kind, sub)


def test_shard_keyword_alone_in_the_world_is_switched_off():
    """shard=True without a process group is rank 0 of 1 -- the sweeps then take the very path they take without the keyword -- and a
    plain callable is not refused there."""
    from colddiff import evaluate
    assert not torch.distributed.is_initialized()
    assert evaluate.shard_ranks(True, lambda samples: 0.0) == (0, 1) and evaluate.shard_ranks(False) == (0, 1)


@pytest.mark.gpu
@pytest.mark.skipif(_gpu_count() < 2, reason="RCCL needs one GPU per rank: runs the day a lease has >= 2 devices (the driver's boxes have one)")
def test_deblur_sweep_over_rccl(tmp_path_factory):
    """Rank r on cuda:r, the accumulators carried by RCCL: batches of 3 (rank 1 gets one short batch)."""
    from colddiff import runtime
    runtime._lib_override = None
    run_deblur_case(MBE("hip"), tmp_path_factory, "rccl", "3")


def test_decolor_sweep_on_two_ranks_walks_rank_zeros_permutation(mbe, tmp_path_factory):
    """The 20-image fixture in batches of 8, 8, 4; rank 1 seeds numpy differently: the result is the single-process run under rank 0's
    seed, and rank 1's numpy stream is where its OWN permutation draw left it."""
    from test_decolor_snow_eval import numpy_seed
    ranks, _, tmp = two_ranks(tmp_path_factory, mbe.kind, "decolor")
    tr, M = W.build_decolor(mbe.device, str(tmp / "res_single"))
    with numpy_seed(M.NP_SEED):
        ref = W.run_sweep(lambda fid, **kw: tr.fid_distance_decrease_from_manifold(fid, **kw), W.keeping_fid(mbe.device),
                          start=M.START, end=M.END, eval_batch_size=W.DECOLOR_BATCH)
    check_sharded([r["decolor"] for r in ranks], ref, 3, fid_ref=ref, what="decolor")
    for rank, r in enumerate(ranks):
        with numpy_seed(M.NP_SEED + 1000 * rank):
            np.random.permutation(len(tr.ds))
            assert r["next_numpy_draw"] == float(np.random.rand()), rank


def test_sample_and_save_for_fid_on_two_ranks_writes_every_file_once(mbe, tmp_path_factory):
    ranks, _, _ = two_ranks(tmp_path_factory, mbe.kind, "save")
    want = [f"sample-x0-{i}.png" for i in range(W.SAVE_N)]
    assert [r["count"] for r in ranks] == [W.SAVE_N, W.SAVE_N]
    for rank, r in enumerate(ranks):                                                        # round k is rank k % 2's: files k bs ... k bs + bs - 1
        assert r["names"] == [f"sample-x0-{k * W.SAVE_BS + i}.png" for k in range(rank, W.SAVE_N // W.SAVE_BS, 2) for i in range(W.SAVE_BS)]
    assert sorted(ranks[0]["names"] + ranks[1]["names"]) == sorted(want)
    assert sorted(os.listdir(ranks[0]["folder"])) == sorted(want)
