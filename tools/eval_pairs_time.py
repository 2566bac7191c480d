"""Time of the evaluation sweep's metric step on the MI355X (HIP events), in one process, at 2000 x 3 x 128 x 128 and 2000 x 3 x 32 x 32
with three candidate sets:

  * the sequence `EvalMixin.fid_distance_decrease_from_manifold` runs (colddiff/evaluate.py): four `(z + 1) * 0.5` shifts that materialise
    the sets, then three `metrics.rmse` and three `metrics.ssim` against the shifted originals;
  * one `metrics.eval_pairs` launch (`cdf_eval_pairs_partial`) on the stored sets, its fp64 sums of the partials included.

Each is timed as a whole by one event pair per repetition: the median, minimum and maximum of 20 repetitions after 5 warm-ups, in
microseconds, and the ratio of the medians.  From bytes alone (about 80 against 16 B per pixel) the expectation is about 5 x.

    python tools/eval_pairs_time.py [--out profiles/eval_pairs_time.json]

No GPU: fails (a CPU run cannot give a time)."""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cold-diffusion-models_amd"))


def timed(fn, reps=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(1000.0 * e0.elapsed_time(e1))
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "reps": reps, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "eval_pairs_time.py measures on the MI355X; a CPU run cannot give a time"
    from colddiff import metrics
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "candidates": 3}
    for N, S in ((2000, 128), (2000, 32)):
        g = torch.Generator().manual_seed(123457)
        x = (torch.rand((N, 3, S, S), generator=g) * 2 - 1).to(dev)
        cands = [(x + s * torch.randn(x.shape, device=dev)).clamp(-1, 1) for s in (0.5, 0.1, 0.02)]
        out = {}

        def sequence():
            sets = [(z + 1) * 0.5 for z in [x] + cands]
            out["seq"] = [(metrics.rmse(sets[0], z), metrics.ssim(sets[0], z, data_range=1, size_average=True)) for z in sets[1:]]

        def one_launch():
            out["one"] = metrics.eval_pairs(x, cands, shift=True)

        sequence()
        one_launch()
        sse, ss = out["one"]
        for k in range(3):                                   # the two compute the same numbers
            rmse = float((sse[k] / x.numel()).sqrt())
            ssim = float(ss[k] / (N * 3 * (S - 10) * (S - 10)))
            assert abs(rmse - float(out["seq"][k][0])) <= 2e-5 and abs(ssim - float(out["seq"][k][1])) <= 1e-4, (k, rmse, ssim, out["seq"][k])
        r = {"sequence": timed(sequence), "eval_pairs": timed(one_launch)}
        r["ratio_of_medians"] = r["sequence"]["median_us"] / r["eval_pairs"]["median_us"]
        r["pixels"] = N * 3 * S * S
        res[f"{N}x3x{S}x{S}"] = r
        print(f"{N}x3x{S}x{S}:", r, flush=True)
        del x, cands, out
        torch.cuda.empty_cache()
    line = json.dumps(res, indent=1, sort_keys=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
