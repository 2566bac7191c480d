"""Time of one Gaussian-mixture fit and one 10 000-row `sample` on the MI355X host + device, in one process, on the same data and the
same `weights_init / means_init / precisions_init`:

  * host route (the default of every Trainer method): `colddiff.evaluate.GMM` / scikit-learn's `GaussianMixture` on the box's CPUs;
  * device route: `colddiff.gmm.GaussianMixture` (csrc/k_gmm.hip + `cdf_gemm_f64`), every per-iteration host read included.

Shapes (N, D, K): (26 900, 3, 10) and (26 900, 48, 10) -- the channel-mean and 4 x 4 x 3 features of the torch_gmm scripts -- and
(1000, 12 288, 10), the vector samplers' default siz = 64, ch = 3, which needs ~40 GB of HBM (covariances, factors, inverses and the
row buffers): skipped with a printed line when less is free.  The data are K separated Gaussian blobs; at D = 12 288 with N = 1000 the
covariances are rank-deficient and the regulariser carries the factorisation, as with real image vectors.

Wall time around a device synchronisation, medians of the repetitions after one warm-up; the host fit is run `--host-reps` times (it is
seconds to minutes per call) and, with `--host-max-iter`, stopped after that many iterations and reported per iteration.  The kernels of
one EM iteration are also event-timed alone at each shape (the per-kernel split).

    python tools/gmm_time.py [--out profiles/gmm_device.md] [--shapes 26900x3x10,26900x48x10,1000x12288x10] [--reps 3] [--host-reps 1]
                             [--host-max-iter 0] [--host-max-d 4096]

Above --host-max-d the host side is not run (a printed line says so): scikit-learn validates `precisions_init` with one dense
eigenvalue problem per component before its first iteration, which alone is tens of minutes at D = 12 288.

Writes the tables to --out as markdown (whatever follows a line `## Recorded by the tests` in an existing file is kept) and prints the
numbers as one JSON object.  No GPU: fails (a CPU run cannot give a time)."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cold-diffusion-models_amd"))

KEEP = "## Recorded by the tests"


def wall(fn, reps, warmup=1):
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


def events(fn, reps=5, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def blobs(n, d, K, seed):
    """float32 rows of K blobs (label = row % K) and the initial parameters: label frequencies, the mean of each label's first five rows,
    identity precisions."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(K, d, generator=g) * 3.0
    labels = torch.arange(n) % K
    x = (centres[labels] + torch.randn(n, d, generator=g)).float()
    means0 = torch.stack([x[labels == k][:5].double().mean(0) for k in range(K)])
    w0 = torch.bincount(labels, minlength=K).double() / n
    return x, w0, means0


def kernel_split(x, model, G):
    """Event times (ms) of the launches of one EM iteration at this shape, on the fitted model's parameters; per component where the
    class loops over components."""
    from colddiff.metrics import gemm_f64
    n, d = x.shape
    K = model.num_components
    w = G._Work(n, d, K, x.device)
    w.resp.fill_(1.0 / K)
    w.nk.fill_(n / K)
    out = {}
    out["center_scale (E, per k)"] = events(lambda: G.center_scale(x, model.means_[0], w.z))
    out["gemm (x - mu) P^T (per k)"] = events(lambda: gemm_f64(w.z, model.precisions_cholesky_[0], out=w.y))
    out["rowsumsq (per k)"] = events(lambda: G.rowsumsq(w.y, w.maha[0]))
    w.maha.fill_(float(d))
    logw = torch.log(model.weights_)
    G.logdet_diag(model.precisions_cholesky_, w.logdet)
    out["logdet + resp (all k)"] = events(lambda: (G.logdet_diag(model.precisions_cholesky_, w.logdet),
                                                  G.responsibilities(w.maha, w.logdet, logw, d, w.resp, w.nk, w.lse_sum, w.partial)))
    xd = x.double()
    out["gemm resp X (all k)"] = events(lambda: gemm_f64(w.resp, xd))
    out["center_scale + Z^T (M, per k)"] = events(lambda: G.center_scale(x, model.means_[0], w.z, zt=w.zt, resp=w.resp[0], nk=w.nk[:1]))
    out["gemm Z^T Z (per k)"] = events(lambda: gemm_f64(w.zt, w.z, out=w.cov[0], diag=1e-6))
    out["potrf (all k)"] = events(lambda: G.potrf_(w.chol.copy_(model.covariances_), w.info))
    out["trtri (all k)"] = events(lambda: G.trtri_lower(model.cholesky_, out=w.pt))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gmm_device.md"))
    ap.add_argument("--shapes", default="26900x3x10,26900x48x10,1000x12288x10")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-max-iter", type=int, default=0, help="stop the host fit after this many iterations (0: run it to convergence)")
    ap.add_argument("--host-max-d", type=int, default=4096, help="above this D the host side is skipped with a printed line (it takes tens of minutes)")
    ap.add_argument("--samples", type=int, default=10000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "gmm_time.py measures on the MI355X; a CPU run cannot give a time"
    from colddiff import gmm as G
    from sklearn.mixture import GaussianMixture as SkGMM
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "cpus": min(len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS") or 1 << 30)), "samples": a.samples}
    for shape in a.shapes.split(","):
        n, d, K = (int(v) for v in shape.split("x"))
        need = 8 * (3 * K * d * d + 3 * n * d + d * d) * 1.15
        free = torch.cuda.mem_get_info()[0]
        if need > free:
            print(f"{shape}: skipped, needs ~{need / 1e9:.0f} GB of HBM, {free / 1e9:.0f} GB free", flush=True)
            res[shape] = {"skipped": f"needs ~{need / 1e9:.0f} GB, {free / 1e9:.0f} GB free"}
            continue
        x, w0, means0 = blobs(n, d, K, 7)
        xd = x.to(dev)
        prec0 = torch.eye(d, dtype=torch.float64).expand(K, d, d)
        keep = {}

        def device_fit():
            keep["m"] = G.GaussianMixture(num_components=K, weights_init=w0, means_init=means0, precisions_init=prec0.to(dev)).fit(xd)

        def device_sample():
            keep["s"] = keep["m"].sample(a.samples)

        print(f"{shape}: device fit ...", flush=True)              # (a line per stage: the large shape takes minutes, and a silent run looks hung)
        r = {"device_fit": wall(device_fit, a.reps), "device_sample": wall(device_sample, a.reps)}
        m = keep["m"]
        r["device_iters"], r["device_converged"], r["device_lower_bound"] = m.n_iter_, m.converged_, m.lower_bound_
        print(f"{shape}: device fit {r['device_fit']['median_s']:.3f} s, {m.n_iter_} iterations; kernels alone ...", flush=True)
        r["kernels_ms"] = kernel_split(xd, m, G)
        r["device_per_iter_s"] = r["device_fit"]["median_s"] / max(1, r["device_iters"])
        if d > a.host_max_d:
            # scikit-learn validates precisions_init with one eigvalsh per component before it starts (K dense d x d eigenproblems: tens of
            # minutes at d = 12 288 on 16 threads), then factors and inverts K covariances per iteration on the host
            r["host_skipped"] = f"D = {d} is above --host-max-d {a.host_max_d}"
            res[shape] = r
            print(shape, "host side skipped:", r["host_skipped"], r, flush=True)
            del keep, m, xd
            torch.cuda.empty_cache()
            continue
        print(f"{shape}: host fit ...", flush=True)
        xh = x.double().numpy()

        def host_fit():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                       # (ConvergenceWarning under --host-max-iter)
                keep["h"] = SkGMM(n_components=K, random_state=0, weights_init=w0.numpy(), means_init=means0.numpy(), precisions_init=prec0.numpy(),
                                  max_iter=a.host_max_iter or 100).fit(xh)

        def host_sample():
            keep["hs"] = keep["h"].sample(a.samples)

        r["host_fit"] = wall(host_fit, a.host_reps, warmup=0)
        r["host_sample"] = wall(host_sample, a.host_reps, warmup=0)
        h = keep["h"]
        r["host_iters"], r["host_converged"], r["host_lower_bound"] = int(h.n_iter_), bool(h.converged_), float(h.lower_bound_)
        r["host_per_iter_s"] = r["host_fit"]["median_s"] / max(1, r["host_iters"])
        if r["host_iters"] == r["device_iters"]:
            r["means_max_difference"] = float(np.abs(m.means_.cpu().numpy() - h.means_).max())
        res[shape] = r
        print(shape, r, flush=True)
        del keep, m, xd
        torch.cuda.empty_cache()

    tail = ""
    if os.path.exists(a.out):
        text = open(a.out).read()
        if KEEP in text:
            tail = text[text.index(KEEP):]
    lines = ["# Gaussian mixture: host route against device route", "",
             f"`python tools/gmm_time.py` on {res['device']} ({res['cpus']} CPU threads for the host route) -- one process, K blobs, the same "
             "`*_init` on both sides, wall time around a device synchronisation, medians after one warm-up (device) / no warm-up (host).", "",
             "| N x D x K | host fit | iterations | per iteration | device fit | iterations | per iteration | host / device per iteration | "
             f"host sample ({res['samples']}) | device sample |", "|---|---|---|---|---|---|---|---|---|---|"]
    shapes = [s for s in res if "x" in s and isinstance(res[s], dict)]
    for s in shapes:
        r = res[s]
        if "skipped" in r:
            lines.append(f"| {s} | skipped: {r['skipped']} | | | | | | | | |")
            continue
        if "host_skipped" in r:
            lines.append(f"| {s} | not run: {r['host_skipped']} | | | {r['device_fit']['median_s']:.3f} s | {r['device_iters']} | {r['device_per_iter_s']:.3f} s | | | "
                         f"{r['device_sample']['median_s'] * 1e3:.1f} ms |")
            continue
        lines.append(f"| {s} | {r['host_fit']['median_s']:.3f} s | {r['host_iters']}{'' if r['host_converged'] else ' (stopped)'} | {r['host_per_iter_s']:.3f} s | "
                     f"{r['device_fit']['median_s']:.3f} s | {r['device_iters']} | {r['device_per_iter_s']:.3f} s | "
                     f"{r['host_per_iter_s'] / r['device_per_iter_s']:.2f} x | {r['host_sample']['median_s'] * 1e3:.1f} ms | {r['device_sample']['median_s'] * 1e3:.1f} ms |")
    lines += ["", "The launches of one EM iteration alone (HIP events, medians, ms):", ""]
    for s in shapes:
        if "kernels_ms" in res[s]:
            lines += [f"* {s}: " + "; ".join(f"{k} {v:.3f}" for k, v in res[s]["kernels_ms"].items())]
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n" + tail)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
