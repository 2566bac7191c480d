"""Time of the LPIPS metric step on the MI355X at 128 x 128, in one process, with an untrained AlexNet (the arithmetic does not depend on
the weight values):

  * device: `LPIPS.distances` of a batch of 64 originals against three candidate sets (what a sweep's `LpipsStats.add` runs per batch):
    four passes through the network on the conv GEMM kernels, five `cdf_lpips_layer` launches, nothing read back; wall time around a
    device synchronisation, median after warm-up, in the default arithmetic mode and in f32 mode;
  * `cdf_lpips_layer` per launch between HIP events (layer kernel + fold), at the five tap shapes of that batch, against its read-once HBM
    floor: (1 + K) maps of B HW C floats over the measured copy bandwidth of the chip (6.29 TB/s; 8 TB/s is the specification).  The maps
    of one launch total 2 ... 63 MB and were just written: they may be served by the 256 MB last-level cache, so a launch can beat that
    floor, which is for data that comes from HBM;
  * for context, the CPU restatement (tests/lpips_ref.py: torch fp32 on the host's CPUs) of the same three distances.

    python tools/lpips_time.py [--out profiles/lpips_device.md] [--reps 10] [--host-reps 2] [--batch 64] [--size 128]

Writes the tables to --out as markdown with the provenance stamp and prints the numbers as one JSON object.  No GPU: fails."""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cold-diffusion-models_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fid_time import events, wall  # noqa: E402
import provenance  # noqa: E402

HBM_COPY_TBS = 6.29                                     # measured float4 copy bandwidth of the MI355X (8.0 TB/s specification)
K = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lpips_device.md"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=128)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "lpips_time.py measures on the MI355X; a CPU run cannot give a time"
    import lpips_ref as R
    from colddiff import lpips as LP
    from colddiff import runtime as rt
    dev = torch.device("cuda:0")
    B, S = a.batch, a.size
    sd, lins = R.random_alexnet(1), R.random_lins(2)
    model = LP.LPIPS(weights=sd, lin=lins).to(dev)
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, 3, S, S, generator=g) * 2 - 1
    cands = [(x + s * torch.randn(x.shape, generator=g)).clamp(-1, 1) for s in (0.5, 0.1, 0.02)]
    dx, dc = x.to(dev), [c.to(dev) for c in cands]
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "size": S, "candidates": K, "provenance": provenance.stamp(),
           "cpus": min(len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS", "0")) or 1 << 30)}

    out = {}
    for mode in ("bf16x3", "f32"):
        with rt.precision_scope(mode):
            def run():
                out[mode] = model.distances(dx, dc)
            res[f"distances_{mode}"] = wall(run, a.reps, 3)
    # the layer launches alone, on the taps of this batch
    with rt.precision_scope("bf16x3"):
        fa = model.features(dx)
        fc = [model.features(c) for c in dc]
    dist = torch.zeros((K, B), device=dev, dtype=torch.float64)
    res["layers"] = []
    for k, t in enumerate(fa):
        _, H, W, C = t.shape
        v = events(lambda: LP.layer_distance(t, [f[k] for f in fc], model.lins[k], dist), reps=20, warmup=5)
        nbytes = (1 + K) * B * H * W * C * 4
        v.update(tap=k, HW=H * W, C=C, bytes=nbytes, floor_us=nbytes / (HBM_COPY_TBS * 1e12) * 1e6)
        v["tbs"] = nbytes / v["median_us"] * 1e-6
        v["floor_over_time"] = v["floor_us"] / v["median_us"]
        res["layers"].append(v)
    # the CPU restatement, for context
    host = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        ref = torch.stack([R.lpips(sd, lins, x, c).flatten() for c in cands])
        host.append(time.perf_counter() - t0)
    res["host"] = {"median_s": sorted(host)[len(host) // 2], "reps": a.host_reps}
    res["max_rel_diff_to_host"] = {m: float(((out[m].cpu() - ref.double()).abs() / ref.double()).max()) for m in out}
    res["mean_distances"] = [float(v) for v in out["bf16x3"].mean(1).cpu()]

    p = res["provenance"]
    lines = ["# LPIPS metric step on the device", "",
             f"`python tools/lpips_time.py` on {res['device']} -- one process, an untrained AlexNet, {B} originals of 3 x {S} x {S} against {K} "
             "candidate sets, medians after warm-up.", "",
             f"Sources: git {p['git_head'] or 'head unknown (a tree without .git)'}, csrc digest {p['csrc_sha16']}.", "",
             "`LPIPS.distances` per batch (four passes through the network, five `cdf_lpips_layer` launches, nothing read back), wall time "
             "around a device synchronisation:", "", "| arithmetic mode | median | min | max | reps |", "|---|---|---|---|---|"]
    for mode in ("bf16x3", "f32"):
        r = res[f"distances_{mode}"]
        lines.append(f"| {mode}{' (default)' if mode == 'bf16x3' else ''} | {r['median_s'] * 1e3:.2f} ms | {r['min_s'] * 1e3:.2f} ms | "
                     f"{r['max_s'] * 1e3:.2f} ms | {r['reps']} |")
    lines += ["", f"For context, the CPU restatement of the same {K} x {B} distances (tests/lpips_ref.py, torch fp32 on {res['cpus']} CPUs): "
              f"{res['host']['median_s']:.2f} s (median of {res['host']['reps']}).  Largest relative difference of the device distances to it: "
              + ", ".join(f"{m} {v:.2g}" for m, v in res["max_rel_diff_to_host"].items()) + ".", "",
              f"`cdf_lpips_layer` per launch (layer kernel + fold) between HIP events, against its read-once floor: the {1 + K} maps of the "
              f"launch over {HBM_COPY_TBS} TB/s, the measured copy bandwidth of the chip.  The maps were written just before and are smaller than the "
              "256 MB last-level cache, so part of the reads may not come from HBM; which part was not measured.", "",
              "| tap | HW | C | bytes read | median | floor | floor / median | rate |", "|---|---|---|---|---|---|---|---|"]
    for v in res["layers"]:
        lines.append(f"| {v['tap']} | {v['HW']} | {v['C']} | {v['bytes'] / 1e6:.1f} MB | {v['median_us']:.1f} us | {v['floor_us']:.1f} us | "
                     f"{100 * v['floor_over_time']:.0f} % | {v['tbs']:.2f} TB/s |")
    total = sum(v["median_us"] for v in res["layers"])
    lines += ["", f"The five launches together: {total:.0f} us, {100 * total * 1e-6 / res['distances_bf16x3']['median_s']:.1f} % of the batch's time "
              "in the default mode; the rest is the network (per pass: the input scaling, 8 + 2 + 3 conv GEMM launches, two activation "
              "launches, two pools).  How that remainder divides was not measured."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
