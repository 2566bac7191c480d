"""Time of the KID metric step on the MI355X host + device, in one process, on stand-in features [N, 2048] (two sets per distance),
N = 1000 and 5000, 100 subsets of min(N, 1000) rows (torch-fidelity's defaults):

  * host route (what a user without the kernel runs): both feature matrices copied to the host, then per subset three
    `sklearn.metrics.pairwise.polynomial_kernel(degree=3, coef0=1)` Gram matrices of the drawn rows and the unbiased MMD^2 of their sums,
    on the CPUs this process may use (its affinity mask, or OMP_NUM_THREADS when that is smaller);
  * device route: `metrics.kid_distance_device` of two `KidStats` -- the draws on the host, the index upload, one `cdf_kid_poly3_f64` launch
    pair, the read of the subset values.

Both draw the same index arrays (`metrics.kid_subset_indices`) and are wall-timed around a device synchronisation: medians of the
repetitions after one warm-up.  The launch pair is also event-timed alone; its rate counts 2 d (m (m + 1) + m^2) flop per subset (the
symmetric halves of XX and YY skipped, their diagonals included).

    python tools/kid_time.py [--out profiles/kid_device.md] [--host-reps 3] [--reps 5] [--sizes 1000,5000] [--subsets 100]

Writes the table to --out as markdown with the provenance stamp and prints the numbers as one JSON object.  No GPU: fails."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cold-diffusion-models_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fid_time import D, events, features, wall  # noqa: E402
import provenance  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kid_device.md"))
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,5000")
    ap.add_argument("--subsets", type=int, default=100)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kid_time.py measures on the MI355X; a CPU run cannot give a time"
    from sklearn.metrics.pairwise import polynomial_kernel
    from colddiff import metrics
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "dims": D, "subsets": a.subsets, "cpus": min(len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS", "0")) or 1 << 30),
           "provenance": provenance.stamp()}

    for n in (int(v) for v in a.sizes.split(",")):
        m = min(n, 1000)
        s1 = metrics.KidStats(D, dev).add(features(n, 10, 0.1, dev))
        s2 = metrics.KidStats(D, dev).add(features(n, 11, 0.25, dev))
        ix, iy = metrics.kid_subset_indices(n, n, a.subsets, m, 2020)
        out = {}

        def host():
            hx, hy = s1.rows().cpu().numpy(), s2.rows().cpu().numpy()                      # (the copy off the device is part of the route)
            off = ~np.eye(m, dtype=bool)
            vals = []
            for s in range(a.subsets):
                xs, ys = hx[ix[s]], hy[iy[s]]
                kxx, kyy, kxy = (polynomial_kernel(p, q, degree=3, coef0=1) for p, q in ((xs, xs), (ys, ys), (xs, ys)))
                vals.append((kxx[off].sum() + kyy[off].sum()) / (m * (m - 1.0)) - 2.0 * kxy.sum() / (float(m) * m))
            out["host"] = np.array(vals)

        def device():
            out["device"] = metrics.kid_distance_device(s1, s2, subsets=a.subsets, subset_size=m, seed=2020)

        dix, diy = torch.from_numpy(ix).to(dev), torch.from_numpy(iy).to(dev)

        def launch():
            out["values"] = metrics.kid_poly3(s1.rows(), s2.rows(), dix, diy)

        r = {"m": m, "device": wall(device, a.reps, 1), "kernels": events(launch, reps=10, warmup=2), "host": wall(host, a.host_reps, 1)}
        vals = out["values"][:, 3].cpu().numpy()
        r["flop"] = a.subsets * 2 * D * (m * (m + 1) + m * m)
        r["tflops"] = r["flop"] / r["kernels"]["median_us"] * 1e-6
        r["host_over_device"] = r["host"]["median_s"] / r["device"]["median_s"]
        r["kid_device"], r["kid_host"] = list(out["device"]), [float(np.mean(out["host"])), float(np.std(out["host"]))]
        r["max_abs_difference"] = float(np.abs(vals - out["host"]).max())
        assert out["device"] == (float(np.mean(vals)), float(np.std(vals)))
        res[f"N={n}"] = r
        print(f"N={n}:", r, flush=True)

    p = res["provenance"]
    lines = ["# KID metric step: host route against device route", "",
             f"`python tools/kid_time.py` on {res['device']} ({res['cpus']} CPUs for the host route) -- one process, stand-in features "
             f"[N, 2048] (two sets per distance), {a.subsets} subsets of m = min(N, 1000) rows, wall time around a device synchronisation, "
             "medians after one warm-up.", "",
             f"Sources: git {p['git_head'] or 'head unknown (a tree without .git)'}, csrc digest {p['csrc_sha16']}.", "",
             "* host: both matrices copied off the device, then per subset three `sklearn.metrics.pairwise.polynomial_kernel(degree=3, "
             "coef0=1)` Gram matrices and the unbiased MMD^2 of their sums;",
             "* device: `kid_distance_device` -- the draws, the index upload, one `cdf_kid_poly3_f64` launch pair, the read of the subset "
             "values; `launch pair` is that pair alone between HIP events, its rate on 2 d (m (m + 1) + m^2) flop per subset.", "",
             "| N | m | host (median) | device (median) | host / device | launch pair (median) | fp64 rate | KID host (mean, std) | "
             "KID device (mean, std) | largest \\|device - host\\| over the subsets |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for key in (q for q in res if q.startswith("N=")):
        r = res[key]
        lines.append(f"| {key[2:]} | {r['m']} | {r['host']['median_s']:.3f} s ({r['host']['reps']} reps) | {r['device']['median_s'] * 1e3:.1f} ms "
                     f"({r['device']['reps']} reps) | {r['host_over_device']:.0f} x | {r['kernels']['median_us'] / 1e3:.2f} ms | "
                     f"{r['tflops']:.1f} TFLOP/s | {r['kid_host'][0]:.9g}, {r['kid_host'][1]:.3g} | {r['kid_device'][0]:.9g}, "
                     f"{r['kid_device'][1]:.3g} | {r['max_abs_difference']:.3g} |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
