"""Sampler graph mode against the eager sampler, in ONE process.

Cases: the MNIST `Unet` and CIFAR-10 `Model` samplers of BASELINE configs 1 and 2 (`sample`, tools/cfgbench.build) at 16 and 64 images,
and `gen_sample` of the CelebA-128 core (T = 200) at 16 and 64 x 3 x 128 x 128.  Per case one core, random-init weights, one fixed
input batch.  The first graph-mode call (warm-up steps, the capture pass, replays for the rest) is timed on its own: the capture cost
of a first call is that time minus the median replayed call.  Then, after one eager warm-up call, RUNS alternating calls -- eager,
graph, eager, graph, ... -- and per mode the median and spread (max - min) of the wall time per call (perf_counter around the call
including the final synchronize) and the host CPU time while enqueueing (time.process_time).  The yardstick is the eager sampler of
the same process: the default path.  Both modes return the same tensors bit for bit (tests/test_sample_graph.py); the tool checks the
final image once per case.  Writes profiles/graph_sample.md and .json with the tools/provenance stamp.

    python tools/graph_sample_time.py [--runs 5] [--out profiles] [--only cfg1,cfg2,celeba128]"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "cold-diffusion-models_amd"), REPO, os.path.join(REPO, "tools")]
import torch  # noqa: E402

import cfgbench  # noqa: E402
import provenance  # noqa: E402

CASES = (("cfg1", "1", "sample"), ("cfg2", "2", "sample"), ("celeba128", "4", "gen_sample"))


def timed(core, method, img, graph):
    """-> (wall seconds incl. the synchronize, host CPU seconds while enqueueing, the final image)."""
    torch.manual_seed(7)
    torch.cuda.synchronize()
    c0, t0 = time.process_time(), time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        out = getattr(core, method)(batch_size=img.shape[0], img=img, graph=graph)
    c1 = time.process_time()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, c1 - c0, out[2]


def measure(cfg, method, n, device, runs):
    torch.manual_seed(123457)
    core, size, _, desc = cfgbench.build(cfg, device)
    img = torch.rand((n, core.channels, size, size), device=device) * 2 - 1
    _, _, want = timed(core, method, img, False)                           # eager warm-up: kernels loaded, weights packed
    first, _, got = timed(core, method, img, True)                         # warm-up steps + capture pass + replays
    assert torch.equal(want, got), "graph mode and the eager sampler disagree"
    modes = {"eager": {"wall": [], "cpu": []}, "graph": {"wall": [], "cpu": []}}
    for _ in range(runs):
        for name in ("eager", "graph"):
            w, c, _ = timed(core, method, img, name == "graph")
            modes[name]["wall"].append(w)
            modes[name]["cpu"].append(c)
    out = {"workload": f"{desc.split(', batch')[0]}; {method}, {n} images, T = {core.num_timesteps}", "images": n, "steps": core.num_timesteps,
           "graph_state": core.sample_graph_state(), "first_graph_call_ms": round(1000 * first, 2)}
    for name, m in modes.items():
        med = statistics.median(m["wall"])
        out[name] = {"ms_per_call_median": round(1000 * med, 2), "ms_per_call_spread": round(1000 * (max(m["wall"]) - min(m["wall"])), 2),
                     "ms_per_call_runs": [round(1000 * w, 2) for w in m["wall"]], "ms_per_image": round(1000 * med / n, 3),
                     "ms_per_step": round(1000 * med / core.num_timesteps, 3), "host_cpu_ms_per_call": round(1000 * statistics.median(m["cpu"]), 2)}
    out["capture_cost_ms"] = round(out["first_graph_call_ms"] - out["graph"]["ms_per_call_median"], 2)
    core.drop_sample_graph()
    del core
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    assert a.runs >= 5
    only = set(a.only.split(",")) - {""}
    device = torch.device("cuda:0")
    doc = {"provenance": provenance.stamp(), "runs_per_mode": a.runs,
           "method": "one process; per case one eager warm-up call, the first graph call timed alone, then alternating calls eager / graph; wall = "
                     "perf_counter around the call incl. the final synchronize; host cpu = process_time while enqueueing", "cases": {}}
    for key, cfg, method in CASES:
        if only and key not in only:
            continue
        for n in (16, 64):
            doc["cases"][f"{key}_{n}"] = measure(cfg, method, n, device, a.runs)
            print(f"{key}_{n}", json.dumps(doc["cases"][f"{key}_{n}"]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    json.dump(doc, open(os.path.join(a.out, "graph_sample.json"), "w"), indent=1)
    with open(os.path.join(a.out, "graph_sample.md"), "w") as f:
        f.write("# Sampler graph mode vs the eager sampler (tools/graph_sample_time.py)\n\n")
        f.write(f"provenance: git {doc['provenance']['git_head']}, csrc {doc['provenance']['csrc_sha16']}\n\n")
        f.write(f"One process; per case an eager warm-up call, the first graph-mode call timed on its own, then {a.runs} alternating calls per mode. "
                "Median wall time per sampler call; spread = slowest - fastest call.  The yardstick is the eager sampler of the same process.\n\n")
        f.write("| case | mode | ms / call (median) | spread (ms) | ms / image | ms / step | host CPU ms / call |\n|---|---|---|---|---|---|---|\n")
        for key, c in doc["cases"].items():
            for name in ("eager", "graph"):
                m = c[name]
                f.write(f"| {key} | {name} | {m['ms_per_call_median']} | {m['ms_per_call_spread']} | {m['ms_per_image']} | {m['ms_per_step']} | "
                        f"{m['host_cpu_ms_per_call']} |\n")
        f.write("\n")
        for key, c in doc["cases"].items():
            ratio = c["graph"]["ms_per_call_median"] / c["eager"]["ms_per_call_median"]
            st = c["graph_state"]
            f.write(f"- {key}: {c['workload']}; mode {st['mode']} ({st['reason']}; {st['captures']} capture, {st['replays']} replays); graph / eager "
                    f"call time = {ratio:.3f}" + (" -- no gain here" if ratio > 0.99 else "") +
                    f"; first graph call {c['first_graph_call_ms']} ms, capture cost {c['capture_cost_ms']} ms over a replayed call\n")


if __name__ == "__main__":
    main()
