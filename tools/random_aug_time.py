"""Time of the `random_aug` data launch on the MI355X (HIP events): `cdf_augment_jitter_batch` for a 64-image 128 x 128 batch from a
218 x 178 RGB cache (CelebA's aligned size) with the decisions the loader draws under a fixed seed, next to the existing
`cdf_augment_batch_pad` launch (crop + mirror + convert) at the same batch from the same cache.  Each launch is timed by its own event pair:
the median, minimum and maximum of 20 launches after 5 warm-ups, in microseconds.

    python tools/random_aug_time.py [--out profiles/random_aug_timing.json]

No GPU: fails (a CPU run cannot give a time)."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cold-diffusion-models_amd"))


def timed(fn, launches=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(1000.0 * e0.elapsed_time(e1))
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "launches": launches, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "random_aug_time.py measures on the MI355X; a CPU run cannot give a time"
    from colddiff import runtime as rt
    from colddiff.trainer import draw_random_aug, jitter_lds_bytes
    dev = torch.device("cuda:0")
    N, SH, SW, B, S = 256, 218, 178, 64, 128
    g = torch.Generator().manual_seed(123457)
    cache = torch.randint(0, 256, (N, SH, SW, 3), generator=g, dtype=torch.uint8).to(dev)
    idx = torch.randperm(N, generator=g)[:B].to(dev)
    params = draw_random_aug(g, B, SH, SW)
    dparams = params.to(dev)
    out = torch.empty((B, 3, S, S), device=dev)
    L, st = rt.lib(), rt.stream(out)
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "cache": [SH, SW], "size": S, "lds_bytes": jitter_lds_bytes(SH, SW, S, S),
           "rows_with_jitter": int((params[:, 5] >= 0).sum()),
           "bytes_per_image": {"read_at_most": SH * SW * 3, "written": 3 * S * S * 4}}

    def jitter():
        L.cdf_augment_jitter_batch(cache.data_ptr(), N, SH, SW, 3, idx.data_ptr(), dparams.data_ptr(), params.data_ptr(), out.data_ptr(), B, S, S, st)

    jitter()
    first = out.clone()
    jitter()
    assert torch.equal(first, out), "two launches on the same decisions differ"
    res["cdf_augment_jitter_batch"] = timed(jitter)
    print("cdf_augment_jitter_batch:", res["cdf_augment_jitter_batch"], flush=True)

    oy = torch.randint(0, SH - S + 1, (B,), generator=g, dtype=torch.int32).to(dev)
    ox = torch.randint(0, SW - S + 1, (B,), generator=g, dtype=torch.int32).to(dev)
    flip = params[:, 4].contiguous().to(dev)

    def plain():
        L.cdf_augment_batch_pad(cache.data_ptr(), N, SH, SW, 3, 0, idx.data_ptr(), oy.data_ptr(), ox.data_ptr(), flip.data_ptr(), out.data_ptr(), B, S, S, st)

    res["cdf_augment_batch_pad"] = timed(plain)
    print("cdf_augment_batch_pad:", res["cdf_augment_batch_pad"], flush=True)
    line = json.dumps(res, indent=1, sort_keys=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
