"""Worker for tests/test_prdc_device.py: one rank of `FidKidStats.all_reduce` followed by `prdc_device` under `torch.distributed.run`.

argv: out_path backend      ("emu": CPU tensors on the simulator, gloo;  "hip": every rank on cuda:0 with the product library, gloo)
Rank r adds ROWS[r] rows of `rows_of(r)`; every rank stores {"n", "prdc": {k: the five numbers}} in out_path.rank<r>.
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
ROWS = (23, 48)                                                    # rows per rank: 71 together, one row past a tile
OTHER_N = 40                                                       # the originals, the same on every rank
KS = (1, 3)


def rows_of(rank, n=None):
    g = torch.Generator().manual_seed(500 + rank)
    return torch.randn(ROWS[rank] if n is None else n, DIMS, generator=g) * 1.2 + 0.3


def originals(device):
    from colddiff import metrics
    return metrics.KidStats(DIMS, device).add(torch.randn(OTHER_N, DIMS, generator=torch.Generator().manual_seed(499)).to(device))


def main():
    out_path, backend = sys.argv[1:3]
    device = torch.device("cuda:0" if backend == "hip" else "cpu")
    if backend != "hip":
        from emu_util import install_emu
        install_emu()
    from colddiff import metrics, parallel
    parallel.init_distributed("gloo")
    rank = parallel.rank()
    st = metrics.FidKidStats(DIMS, device)                          # the combined statistics the sweeps use
    st.add(rows_of(rank).to(device))
    assert st.all_reduce() is st
    res = {"n": st.kid_stats.n, "prdc": {k: metrics.prdc_device(originals(device), st.kid_stats, k) for k in KS}}
    if backend == "hip":
        torch.cuda.synchronize()
    torch.save(res, out_path + f".rank{rank}")
    torch.distributed.barrier()


if __name__ == "__main__":
    main()
