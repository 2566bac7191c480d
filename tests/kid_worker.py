"""Worker for tests/test_kid_device.py: one rank of `KidStats.all_reduce` / `FidKidStats.all_reduce` under `torch.distributed.run`.

argv: out_path backend      ("emu": CPU tensors on the simulator, gloo;  "hip": every rank on cuda:0 with the product library, gloo)
Rank r adds ROWS[case][r] rows of `rows_of(case, r)`; every rank stores {case: {"rows", "n", "kid", ...}} in out_path.rank<r>.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, "cold-diffusion-models_amd"), HERE, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

DIMS = 12
ROWS = {"unequal": (5, 9), "one_empty": (7, 0)}                      # rows per rank
OTHER_N = 11                                                       # the second set of the distance, the same on every rank
KID = dict(subsets=3, subset_size=6, seed=5)


def rows_of(case, rank, n=None):
    g = torch.Generator().manual_seed(1000 * sorted(ROWS).index(case) + rank)
    return torch.randn(ROWS[case][rank] if n is None else n, DIMS, generator=g)


def other_set(device):
    from colddiff import metrics
    return metrics.KidStats(DIMS, device).add((rows_of("unequal", 7, OTHER_N) * 1.3 + 0.4).to(device))


def main():
    out_path, backend = sys.argv[1:3]
    device = torch.device("cuda:0" if backend == "hip" else "cpu")
    if backend != "hip":
        from emu_util import install_emu
        install_emu()
    from colddiff import metrics, parallel
    parallel.init_distributed("gloo")
    rank = parallel.rank()
    res = {}
    # rows of unequal counts through the combined statistics the sweeps use: the FID half and the KID half are both reduced
    st = metrics.FidKidStats(DIMS, device)
    st.add(rows_of("unequal", rank).to(device))
    assert st.all_reduce() is st
    res["unequal"] = {"rows": st.kid_stats.rows().cpu().clone(), "n": st.kid_stats.n, "fid_n": st.n, "mean": st.mean().cpu().clone(),
                      "kid": metrics.kid_distance_device(st.kid_stats, other_set(device), **KID)}
    # one rank without a row
    ks = metrics.KidStats(DIMS, device)
    if ROWS["one_empty"][rank]:
        ks.add(rows_of("one_empty", rank).to(device))
    assert ks.all_reduce() is ks
    res["one_empty"] = {"rows": ks.rows().cpu().clone(), "n": ks.n, "kid": metrics.kid_distance_device(ks, other_set(device), **KID)}
    # nobody has a row
    none = metrics.KidStats(DIMS, device).all_reduce()
    res["all_empty"] = {"n": none.n, "shape": tuple(none.rows().shape)}
    if backend == "hip":
        torch.cuda.synchronize()
    torch.save(res, out_path + f".rank{rank}")
    torch.distributed.barrier()


if __name__ == "__main__":
    main()
