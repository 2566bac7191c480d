"""Time of the precision / recall / density / coverage metric step on the MI355X host + device, in one process, on stand-in features
[N, 2048] (two sets per evaluation), N = 1000, 5000 and 10 000, k = 3:

  * host route (what a user without the kernels runs): both feature matrices copied to the host, then the definitions of
    include/colddiff.h in numpy fp64 in column batches -- the k smallest squared distances of X to X and of Y to Y, and ONE walk of the
    X-to-Y distances that serves both ball passes (a host user would not compute that product twice): three N^2 d products, on the CPUs
    this process may use (its affinity mask, or OMP_NUM_THREADS when that is smaller);
  * device route: `metrics.prdc_device` of two `KidStats` -- two norm launches, two `knn_sq`, two `ball_counts`, the read of the four sums.

Both are wall-timed around a device synchronisation: medians of the repetitions after one warm-up.  The four GEMM-shaped launches (each a
main kernel and its fold) are also event-timed alone; a rate counts 2 r c d flop for r rows against c columns, the total 2 d (n^2 + m^2 +
2 n m) over the sum of the four.

    python tools/prdc_time.py [--out profiles/prdc_device.md] [--host-reps 3] [--reps 5] [--sizes 1000,5000,10000] [--k 3]

Writes the tables to --out as markdown with the provenance stamp and prints the numbers as one JSON object.  No GPU: fails."""
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

KEYS = ("precision", "recall", "density", "coverage", "f_score")
GEMM_F64_TFLOPS = 40.4                                  # cdf_gemm_f64 at 2048^3, profiles/fid_device.md: the yardstick of the two kernels
BATCH = 2048                                            # columns per host batch: an [N, 2048] block of distances at a time


def host_knn_radius(x, nx, k):
    """rho [n]: the k-th smallest D(x_j, x_l), l != j, walking the columns in batches and keeping the k smallest per row."""
    n = len(x)
    best = np.full((n, k), np.inf)
    for c0 in range(0, n, BATCH):
        c1 = min(c0 + BATCH, n)
        blk = np.maximum(0.0, (nx[:, None] + nx[None, c0:c1]) - 2.0 * (x @ x[c0:c1].T))
        blk[np.arange(c0, c1), np.arange(c1 - c0)] = np.inf                                # self, by position
        best = np.partition(np.concatenate((best, blk), axis=1), k - 1, axis=1)[:, :k]
    return best.max(1)


def host_prdc(x, y, k):
    n, m = len(x), len(y)
    nx, ny = (x * x).sum(1), (y * y).sum(1)
    rho_x, rho_y = host_knn_radius(x, nx, k), host_knn_radius(y, ny, k)
    in_x, in_y, own = np.zeros(m, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for c0 in range(0, m, BATCH):
        c1 = min(c0 + BATCH, m)
        blk = np.maximum(0.0, (nx[:, None] + ny[None, c0:c1]) - 2.0 * (x @ y[c0:c1].T))     # D(x_j, y_i), j down, i across
        inside = blk <= rho_x[:, None]
        in_x[c0:c1] = inside.sum(0)
        own += inside.sum(1)
        in_y += (blk <= rho_y[None, c0:c1]).sum(1)
    precision, recall = int((in_x > 0).sum()) / m, int((in_y > 0).sum()) / n
    return dict(precision=precision, recall=recall, density=int(in_x.sum()) / (k * m), coverage=int((own > 0).sum()) / n,
                f_score=2.0 * precision * recall / max(precision + recall, 1e-5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "prdc_device.md"))
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1000,5000,10000")
    ap.add_argument("--k", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "prdc_time.py measures on the MI355X; a CPU run cannot give a time"
    from colddiff import metrics
    dev = torch.device("cuda:0")
    k = a.k
    res = {"device": torch.cuda.get_device_name(0), "dims": D, "k": k,
           "cpus": min(len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS", "0")) or 1 << 30), "provenance": provenance.stamp()}

    for n in (int(v) for v in a.sizes.split(",")):
        s1 = metrics.KidStats(D, dev).add(features(n, 10, 0.1, dev))
        s2 = metrics.KidStats(D, dev).add(features(n, 11, 0.25, dev))
        out = {}

        def host():
            out["host"] = host_prdc(s1.rows().cpu().numpy(), s2.rows().cpu().numpy(), k)    # (the copy off the device is part of the route)

        def device():
            out["device"] = metrics.prdc_device(s1, s2, k)

        r = {"device": wall(device, a.reps, 1), "host": wall(host, a.host_reps, 1)}
        x, y = s1.rows(), s2.rows()
        nx, ny = metrics.row_norms_sq(x), metrics.row_norms_sq(y)
        rho_x, rho_y = (metrics.knn_sq(t, k, v)[:, k - 1].contiguous() for t, v in ((x, nx), (y, ny)))
        launches = {"knn_sq(X)": lambda: metrics.knn_sq(x, k, nx), "knn_sq(Y)": lambda: metrics.knn_sq(y, k, ny),
                    "ball_counts(Y, X)": lambda: metrics.ball_counts(y, x, rcol=rho_x, anorm=ny, bnorm=nx),
                    "ball_counts(X, Y)": lambda: metrics.ball_counts(x, y, rcol=rho_y, rrow=rho_x, anorm=nx, bnorm=ny)}
        r["launches"] = {name: events(fn, reps=5, warmup=1) for name, fn in launches.items()}
        flop = 2.0 * n * n * D                                                              # per launch: both sets have n rows here
        for v in r["launches"].values():
            v["tflops"] = flop / v["median_us"] * 1e-6
            v["share_of_device"] = v["median_us"] * 1e-6 / r["device"]["median_s"]
        r["tflops"] = 4 * flop / sum(v["median_us"] for v in r["launches"].values()) * 1e-6
        r["host_over_device"] = r["host"]["median_s"] / r["device"]["median_s"]
        r["prdc_device"], r["prdc_host"] = out["device"], out["host"]
        res[f"N={n}"] = r
        print(f"N={n}:", r, flush=True)

    p = res["provenance"]
    sizes = [q for q in res if q.startswith("N=")]
    lines = ["# Precision / recall / density / coverage metric step: host route against device route", "",
             f"`python tools/prdc_time.py` on {res['device']} ({res['cpus']} CPUs for the host route) -- one process, stand-in features "
             f"[N, 2048] (two sets per evaluation), k = {k}, wall time around a device synchronisation, medians after one warm-up.", "",
             f"Sources: git {p['git_head'] or 'head unknown (a tree without .git)'}, csrc digest {p['csrc_sha16']}.", "",
             "* host: both matrices copied off the device, then the same definitions in numpy fp64 in column batches of "
             f"{BATCH}: the k-th-neighbour radii of each set and one walk of the X-to-Y distances for both ball passes (three N^2 d products);",
             "* device: `prdc_device` -- two `cdf_rowsumsq_f64`, two `cdf_knn_sq_f64`, two `cdf_ball_counts_f64`, the read of the four "
             "integer sums (four N^2 d products: the full square per k-NN pass, each ball pass its own walk).", "",
             "| N | host (median) | device (median) | host / device | fp64 rate of the four launches | "
             f"share of `cdf_gemm_f64`'s {GEMM_F64_TFLOPS} TFLOP/s |", "|---|---|---|---|---|---|"]
    for key in sizes:
        r = res[key]
        lines.append(f"| {key[2:]} | {r['host']['median_s']:.3f} s ({r['host']['reps']} reps) | {r['device']['median_s'] * 1e3:.1f} ms "
                     f"({r['device']['reps']} reps) | {r['host_over_device']:.0f} x | {r['tflops']:.1f} TFLOP/s | "
                     f"{100 * r['tflops'] / GEMM_F64_TFLOPS:.0f} % |")
    lines += ["", "What separates the two kernels from `cdf_gemm_f64` by construction: per 64 x 64 tile the epilogue (k-NN: the tile of D through "
              "LDS, two barriers and the scan into the sorted lists; ball counts: 32 compares per lane) and a K loop that starts cold (the next "
              "tile's first operand fetch does not run under the previous tile's epilogue); per launch a grid of row tiles x S blocks whose last "
              "round does not fill the CUs.  How the remainder divides among these has not been measured."]
    lines += ["", "The four GEMM-shaped launches alone, between HIP events (main kernel + fold; 2 N^2 d flop each), and their share of the "
              "device route's wall time; what the shares leave is the two norm launches, the four reductions and the host read.", "",
              "| N | launch | median | fp64 rate | share of the device time |", "|---|---|---|---|---|"]
    for key in sizes:
        for name, v in res[key]["launches"].items():
            lines.append(f"| {key[2:]} | `{name}` | {v['median_us'] / 1e3:.2f} ms | {v['tflops']:.1f} TFLOP/s | {100 * v['share_of_device']:.0f} % |")
    lines += ["", "The numbers of both routes:", "", "| N | route | " + " | ".join(KEYS) + " |", "|---|---|" + "---|" * len(KEYS)]
    for key in sizes:
        for route in ("host", "device"):
            lines.append(f"| {key[2:]} | {route} | " + " | ".join(f"{res[key]['prdc_' + route][q]:.9g}" for q in KEYS) + " |")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
