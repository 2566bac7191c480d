"""Worker for tests/test_lpips_device.py: one rank of `LpipsStats.all_reduce` under `torch.distributed.run`.

argv: out_path backend      ("emu": CPU tensors on the simulator, gloo;  "hip": every rank on cuda:0 with the product library, gloo)
Rank r adds its IMAGES[r] images (one batch; rank 0 fewer than rank 1) of `batch_of(r)` through the real network; every rank stores
{"count", "sums", "result"} in out_path.rank<r>.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, "cold-diffusion-models_amd"), HERE, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

IMAGES = (1, 2)                                                    # images per rank
NAMES = ("blur", "deblur")
SIZE = 32
NET_SEED, LIN_SEED = 21, 22


def batch_of(rank):
    """(originals, [candidates]) of a rank, in [-1, 1]."""
    g = torch.Generator().manual_seed(700 + rank)
    x = torch.rand(IMAGES[rank], 3, SIZE, SIZE, generator=g) * 2 - 1
    cands = [(x + s * torch.randn(x.shape, generator=g)).clamp(-1, 1) for s in (0.4, 0.1)]
    return x, cands


def model_on(device):
    import lpips_ref as R
    from colddiff.lpips import LPIPS
    return LPIPS(weights=R.random_alexnet(NET_SEED), lin=R.random_lins(LIN_SEED)).to(device)


def stats_of(rank, model, device):
    from colddiff import metrics
    x, cands = batch_of(rank)
    st = metrics.LpipsStats(NAMES)
    st.add(x.to(device), [c.to(device) for c in cands], model)
    return st


def main():
    out_path, backend = sys.argv[1:3]
    device = torch.device("cuda:0" if backend == "hip" else "cpu")
    if backend != "hip":
        from emu_util import install_emu
        install_emu()
    from colddiff import parallel
    parallel.init_distributed("gloo")
    rank = parallel.rank()
    st = stats_of(rank, model_on(device), device)
    assert st.all_reduce() is st
    res = {"count": st.count, "sums": st.sums.cpu().clone(), "result": st.result()}
    if backend == "hip":
        torch.cuda.synchronize()
    torch.save(res, out_path + f".rank{rank}")
    torch.distributed.barrier()


if __name__ == "__main__":
    main()
