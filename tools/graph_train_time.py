"""Trainer graph mode against the eager step, BASELINE configs 1 and 2, in ONE process.

Two Trainers per configuration, built as bench.py builds them (tools/cfgbench.build, the constructor arguments of
bench.secondary_workloads): one eager (with its degradation prefetch, as the benchmark runs it), one with graph=True.  After 0.5 s of
warm-up steps each they run alternating windows -- eager, graph, eager, graph, ... -- of STEPS optimizer steps, WINDOWS windows per
mode.  Per mode: median and spread (max - min over the windows) of the wall time per step, and the host CPU time per step
(time.process_time: what the launching thread and the runtime's helper threads burn).  Writes profiles/graph_train.md and .json with
the tools/provenance stamp.

    python tools/graph_train_time.py [--windows 5] [--steps 50] [--out profiles]"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "cold-diffusion-models_amd"), REPO, os.path.join(REPO, "tools")]
import torch  # noqa: E402

import cfgbench  # noqa: E402
import provenance  # noqa: E402
from colddiff.trainer import Trainer  # noqa: E402


def make(cfg, device, graph, res):
    torch.manual_seed(123457)
    d, size, batch, desc = cfgbench.build(cfg, device)
    with contextlib.redirect_stdout(io.StringIO()):
        tr = Trainer(d, None, image_size=size, train_batch_size=batch, train_lr=2e-5, train_num_steps=10 ** 9, gradient_accumulate_every=2,
                     dataset='synthetic', results_folder=res, graph=graph)
    tr.quiet = True
    return tr, 2 * batch, desc


def steps(tr, n):
    for _ in range(n):
        tr.train_step()
        tr.step += 1


def warm(tr, seconds):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        steps(tr, 8)
        torch.cuda.synchronize()


def window(tr, n):
    torch.cuda.synchronize()
    c0, t0 = time.process_time(), time.perf_counter()
    steps(tr, n)
    c1 = time.process_time()                 # host time spent ENQUEUEING (before the wait for the device)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, (c1 - c0) / n


def measure(cfg, device, windows, nsteps, res):
    modes = {}
    trainers = {}
    for name, graph in (("eager", False), ("graph", True)):
        trainers[name], imgs, desc = make(cfg, device, graph, res)
        warm(trainers[name], 0.5)
        modes[name] = {"wall": [], "cpu": []}
    for _ in range(windows):
        for name in ("eager", "graph"):
            w, c = window(trainers[name], nsteps)
            modes[name]["wall"].append(w)
            modes[name]["cpu"].append(c)
    out = {"workload": desc + ", 2 micro-steps + Adam", "images_per_step": imgs, "graph_state": trainers["graph"].graph_state()}
    for name, m in modes.items():
        med = statistics.median(m["wall"])
        out[name] = {"ms_per_step_median": round(1000 * med, 3), "ms_per_step_spread": round(1000 * (max(m["wall"]) - min(m["wall"])), 3),
                     "ms_per_step_windows": [round(1000 * w, 3) for w in m["wall"]], "img_per_s": round(imgs / med, 1),
                     "host_cpu_ms_per_step": round(1000 * statistics.median(m["cpu"]), 3)}
    del trainers
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    a = ap.parse_args()
    assert a.windows >= 5 and a.steps >= 1
    device = torch.device("cuda:0")
    res = tempfile.mkdtemp(prefix="graph_train_time_")
    doc = {"provenance": provenance.stamp(), "windows_per_mode": a.windows, "steps_per_window": a.steps, "warmup_seconds": 0.5,
           "method": "one process, alternating windows eager / graph; wall = perf_counter around the window incl. the final synchronize; "
                     "host cpu = process_time while enqueueing"}
    for cfg, key in (("1", "cfg1_mnist32_deblur_train"), ("2", "cfg2_cifar10_deblur_train")):
        doc[key] = measure(cfg, device, a.windows, a.steps, res)
        print(key, json.dumps(doc[key]), flush=True)
    os.makedirs(a.out, exist_ok=True)
    json.dump(doc, open(os.path.join(a.out, "graph_train.json"), "w"), indent=1)
    with open(os.path.join(a.out, "graph_train.md"), "w") as f:
        f.write("# Trainer graph mode vs the eager step (tools/graph_train_time.py)\n\n")
        f.write(f"provenance: git {doc['provenance']['git_head']}, csrc {doc['provenance']['csrc_sha16']}\n\n")
        f.write(f"One process, alternating windows (eager, graph, ...), {a.windows} windows of {a.steps} optimizer steps per mode after 0.5 s of warm-up. "
                "Spread = slowest - fastest window.\n\n")
        f.write("| configuration | mode | ms / step (median) | spread (ms) | img/s | host CPU ms / step |\n|---|---|---|---|---|---|\n")
        for key in ("cfg1_mnist32_deblur_train", "cfg2_cifar10_deblur_train"):
            for name in ("eager", "graph"):
                m = doc[key][name]
                f.write(f"| {key} | {name} | {m['ms_per_step_median']} | {m['ms_per_step_spread']} | {m['img_per_s']} | {m['host_cpu_ms_per_step']} |\n")
        f.write("\n")
        for key in ("cfg1_mnist32_deblur_train", "cfg2_cifar10_deblur_train"):
            e, g = doc[key]["eager"], doc[key]["graph"]
            gain = e["ms_per_step_median"] / g["ms_per_step_median"]
            f.write(f"- {key}: {doc[key]['workload']}; graph mode {doc[key]['graph_state']['mode']} ({doc[key]['graph_state']['reason']}); "
                    f"graph / eager step time = {1 / gain:.3f}" + (" -- no gain here\n" if gain < 1.01 else "\n"))


if __name__ == "__main__":
    main()
