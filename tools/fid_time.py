"""Time of the FID metric step on the MI355X host + device, in one process, on stand-in features [N, 2048] (two sets per distance),
N = 1000 and 5000:

  * host route (what `calculate_fid_given_samples` runs after the extractor): `np.cov` of each [N, 2048] float64 matrix and
    `metrics.calculate_frechet_distance` (scipy `sqrtm` of the 2048 x 2048 product);
  * device route: `FidStats.add` in batches of 50 (`cdf_moments_f64`) for both sets and `metrics.frechet_distance_device` (two
    Newton-Schulz square roots on `cdf_gemm_f64`), the trace read of every step and the final host read included.

Both are wall-timed around a device synchronisation: medians of the repetitions after the warm-ups (the host route is seconds per call,
so it gets few).  The kernels are also event-timed alone: `cdf_moments_f64` at n = 50, d = 2048, `cdf_moments_merge_f64` at d = 2048
(`FidStats.merge` of two accumulators on different pivots) and `cdf_gemm_f64` at 2048^3.  `--kernels-only` stops after those.

    python tools/fid_time.py [--out profiles/fid_device.md] [--host-reps 3] [--reps 5] [--sizes 1000,5000]

Writes the tables to --out as markdown (whatever follows a line `## Recorded by the tests` in an existing file is kept) and prints the
numbers as one JSON object.  No GPU: fails (a CPU run cannot give a time)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cold-diffusion-models_amd"))

D = 2048
KEEP = "## Recorded by the tests"


def wall(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    s = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(s), "min_s": min(s), "max_s": max(s), "reps": reps, "warmup": warmup}


def events(fn, reps=20, warmup=5):
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


def features(n, seed, shift, dev):
    """max(G W + b, 0) in fp32 with a decaying column scale, as the tests' inputs."""
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(D, D, generator=g, dtype=torch.float64) * torch.arange(1, D + 1, dtype=torch.float64) ** -0.8).to(dev)
    b = (torch.randn(D, generator=g, dtype=torch.float64) * 0.3 + shift).to(dev)
    G = torch.randn(n, D, generator=g, dtype=torch.float64).to(dev)
    return torch.relu(G @ W + b).float().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fid_device.md"))
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,5000")
    ap.add_argument("--kernels-only", action="store_true", help="time the kernels alone, print the JSON line and leave --out as it is")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fid_time.py measures on the MI355X; a CPU run cannot give a time"
    from colddiff import metrics
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "dims": D, "batch": 50, "cpus": len(os.sched_getaffinity(0))}

    # the kernels alone
    x = features(50, 1, 0.1, dev)
    st = metrics.FidStats(D, dev).add(x)
    res["moments_50x2048"] = events(lambda: st.add(x))
    res["moments_50x2048"].update(flop=2 * 50 * D * D // 2, bytes=D * (D + 64) // 2 * 16 + 50 * D * 4)
    # the merge: b's triangle and a's are read, a's is written (3 x the triangle's tiles; the pivots and sums are 48 KB)
    other = metrics.FidStats(D, dev).add(features(50, 2, 0.25, dev))
    res["merge_2048"] = events(lambda: st.merge(other))
    res["merge_2048"].update(flop=8 * D * (D + 64) // 2, bytes=D * (D + 64) // 2 * 24 + 3 * D * 8)
    A, B, C = (torch.randn(D, D, device=dev, dtype=torch.float64) for _ in range(3))
    res["gemm_2048"] = events(lambda: metrics.gemm_f64(A, B, out=C, alpha=-0.5, diag=1.5), reps=10, warmup=3)
    res["gemm_2048"].update(flop=2 * D ** 3, bytes=3 * D * D * 8)
    res["gemm_2048"]["tflops"] = 2 * D ** 3 / res["gemm_2048"]["median_us"] * 1e-6
    print("kernels:", res["moments_50x2048"], res["merge_2048"], res["gemm_2048"], flush=True)
    del A, B, C
    if a.kernels_only:
        print(json.dumps(res, sort_keys=True))
        return

    for n in (int(v) for v in a.sizes.split(",")):
        fa, fb = features(n, 10, 0.1, dev), features(n, 11, 0.25, dev)
        ha, hb = fa.double().cpu().numpy(), fb.double().cpu().numpy()              # (the host route starts from the host matrices it holds)
        out = {}

        def host():
            out["host"] = float(metrics.calculate_frechet_distance(ha.mean(0), np.cov(ha, rowvar=False), hb.mean(0), np.cov(hb, rowvar=False)))

        def stats():
            both = []
            for f in (fa, fb):
                s = metrics.FidStats(D, dev)
                for i in range(0, n, 50):
                    s.add(f[i:i + 50])
                both.append(s)
            out["stats"] = both

        def device():
            stats()
            info = {}
            out["device"] = metrics.frechet_distance_device(*out["stats"], _info=info)
            out["info"] = info

        r = {"device": wall(device, a.reps, 1), "device_stats_only": wall(stats, a.reps, 1), "host": wall(host, a.host_reps, 1)}
        r["host_over_device"] = r["host"]["median_s"] / r["device"]["median_s"]
        r["fid_host"], r["fid_device"], r["steps"], r["fallback"] = out["host"], out["device"], list(out["info"]["iters"]), out["info"]["fallback"]
        r["rel_difference_of_tr_sqrt"] = abs(out["host"] - out["device"]) / (2 * out["info"]["tr_sqrt"]) if out["info"]["tr_sqrt"] else None
        res[f"N={n}"] = r
        print(f"N={n}:", r, flush=True)

    tail = ""
    if os.path.exists(a.out):
        text = open(a.out).read()
        if KEEP in text:
            tail = text[text.index(KEEP):]
    k, m, gm, mg = res, res["moments_50x2048"], res["gemm_2048"], res["merge_2048"]
    lines = ["# FID metric step: host route against device route", "",
             f"`python tools/fid_time.py` on {k['device']} ({k['cpus']} CPUs for the host route) -- one process, stand-in features [N, 2048] "
             "(two sets per distance), wall time around a device synchronisation, medians after one warm-up.", "",
             "* host: `np.cov` of both [N, 2048] float64 matrices + `calculate_frechet_distance` (scipy `sqrtm`);",
             "* device: `FidStats.add` in batches of 50 for both sets + `frechet_distance_device`, every trace read and the final read included.", "",
             "| N | host (median) | device (median) | of which statistics | host / device | Newton-Schulz steps (sqrt C1, sqrt M) | fid host | fid device | difference / 2 Tr sqrt |",
             "|---|---|---|---|---|---|---|---|---|"]
    for key in (q for q in res if q.startswith("N=")):
        r = res[key]
        lines.append(f"| {key[2:]} | {r['host']['median_s']:.3f} s ({r['host']['reps']} reps) | {r['device']['median_s']:.3f} s ({r['device']['reps']} reps) | "
                     f"{r['device_stats_only']['median_s'] * 1e3:.1f} ms | {r['host_over_device']:.1f} x | {r['steps'][0]} and {r['steps'][1]}"
                     f"{' (FELL BACK to the host)' if r['fallback'] else ''} | {r['fid_host']:.9g} | {r['fid_device']:.9g} | "
                     f"{'n/a' if r['rel_difference_of_tr_sqrt'] is None else format(r['rel_difference_of_tr_sqrt'], '.2g')} |")
    lines += ["", "The kernels alone (HIP events, medians):", "",
              "| kernel | shape | median | flop | bytes (compulsory) | rate |", "|---|---|---|---|---|---|",
              f"| `cdf_moments_f64` | n = 50, d = 2048 | {m['median_us']:.1f} us | {m['flop'] / 1e9:.2f} G | {m['bytes'] / 1e6:.1f} MB "
              f"(read + write of the triangle's tiles) | {m['bytes'] / m['median_us'] * 1e-6:.2f} TB/s |",
              f"| `cdf_moments_merge_f64` | d = 2048 | {mg['median_us']:.1f} us | {mg['flop'] / 1e9:.3f} G | {mg['bytes'] / 1e6:.1f} MB "
              f"(two triangles read, one written) | {mg['bytes'] / mg['median_us'] * 1e-6:.2f} TB/s |",
              f"| `cdf_gemm_f64` | 2048^3 | {gm['median_us'] / 1e3:.2f} ms | {gm['flop'] / 1e9:.1f} G | {gm['bytes'] / 1e6:.1f} MB | {gm['tflops']:.1f} TFLOP/s |", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n" + tail)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
