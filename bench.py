#!/usr/bin/env python3
"""bench.py — CelebA-128 cold-diffusion training throughput (+ 200-step sampling latency) on MI355X.

  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

A plain run sets up, runs W warm-up and K timed optimizer steps and prints the headline line (`value` img/s, `ms_per_step`).
--dump-outputs DIR writes what the last timed step produced (its loss, and a fixed seeded sample of the parameters, Adam moments
and EMA weights it left behind) as DIR/<name>.npy.  --full adds everything else the benchmark measures: the GEMM roofline pass,
step / per-class roofline figures, the gradient-exchange record (N > 1), the 200-step sampler, the unfused step, the self-check
against the CPU oracle, the bf16 / f32 mode lines, BASELINE configs 1, 2, 4 and 5 and the CPU baseline.

Workload (BASELINE.json config 3, the single-GPU CelebA-128 case):
  Unet(dim=64, dim_mults=(1,2,4,8), channels=3) at 128x128, denoising GaussianDiffusion(T=200,
  x0_step_down), synthetic 8-bit-quantised images, random-init weights.
A *step* is one optimizer step exactly as Trainer.train() does it (DEBLUR:1188-1204): 2 accumulation
micro-batches of 32 images (q_sample -> UNet fwd -> L1 -> bwd) + Adam (+ EMA every 10th step).  Since
round 4 the engine degrades the micro-batches one by one (the reference's data order and draws) and runs
them through the network as ONE 64-image pass -- the same gradient sum (colddiff/trainer.py: fused
accumulation; tests/test_modules.py::test_fused_accumulation_*); the line also carries the step with
separate micro-steps (`accumulation.unfused_*`, COLDDIFF_FUSE_ACCUM=0).  With N > 1 each rank does the
same work on its own shard and gradients are all-reduced over RCCL (weak scaling).  `value` = images/s
over all ranks.  Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(REPO, "cold-diffusion-models_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

# multi-process GPU work on these hosts needs dmabuf IPC (RCCL / hipIpcGetMemHandle fail with the legacy mode); the image exports it
# already -- keep it when somebody launches with a scrubbed environment.  Must be set before the HIP runtime starts.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402


def log(msg):
    sys.stderr.write("[bench %7.1fs] %s\n" % (time.perf_counter() - _T0, msg))
    sys.stderr.flush()


_T0 = time.perf_counter()
# Trainer(results_folder=) creates the folder; the benchmark never saves or samples into it, so it is a throw-away directory
_RESULTS = tempfile.TemporaryDirectory(prefix="colddiff_bench_")
PEAK_F32_MFMA_TFLOPS = 157.3       # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0     # MI355X_MICROARCH.md: v_mfma_f32_32x32x16_bf16, dense
PEAK_HBM_GBS = 8000.0              # MI355X_MICROARCH.md: HBM3E
MEASURED_MFMA_CEILING_TFLOPS = 1820.0   # tools/probes/mfma_power.hip on this part: v_mfma_f32_32x32x16_bf16, registers only, RANDOM bf16 operands
                                        # (zeros / small constants: 2490) -- profiles/round2_mfma_power.md


def npp_of(precision):
    """MFMAs per algorithmic product of the dense-conv GEMMs in an arithmetic mode."""
    return {"bf16x3": 3, "bf16": 1}.get(precision, 1)
UNET128_FWD_GFLOP = 67.41          # SURVEY.md §8(d), per image
UNET128_ACT_TRAIN_MB = {"f32": 1098.0, "bf16": 549.0}   # A_train = 2.5 x A_fwd, layer-boundary bytes per image
UNET128_PARAMS = 56615708
TIMESTEPS = 200


def step_roofline(batch, accum, ms_per_step, mfma_per_product, act="f32"):
    """bytes_step = B (A_train + D_bytes) accum + 3 W accum + 28 P (+ 1.2 P amortised EMA);
    flops_step = B (F_train + D_flops) accum; t_roof = max(bytes / BW_HBM, flops / PEAK_MFMA[bf16]) on ALGORITHMIC flops.
    The MFMA instructions actually issued (3 per product in split precision) are reported separately as `mfma_issue_*`:
    they say how busy the matrix pipe is, not how close the step is to its roofline."""
    P = UNET128_PARAMS
    W = 4.0 * P
    d_bytes = 3 * 3 * 128 * 128 * 4.0                       # noise q_sample: read x, read noise, write x_t (fp32)
    bytes_step = batch * (UNET128_ACT_TRAIN_MB[act] * 1e6 + d_bytes) * accum + 3 * W * accum + 28.0 * P + 1.2 * P
    flops_step = batch * accum * (3 * UNET128_FWD_GFLOP * 1e9 + 3 * 3 * 128 * 128)
    t = ms_per_step * 1e-3
    t_hbm = bytes_step / (PEAK_HBM_GBS * 1e9)
    t_mfma = flops_step / (PEAK_BF16_MFMA_TFLOPS * 1e12)
    t_issue = flops_step * mfma_per_product / (PEAK_BF16_MFMA_TFLOPS * 1e12)     # what the matrix pipe must ISSUE in this arithmetic mode
    return {"activation_bytes": act, "bytes_step": round(bytes_step), "flops_step": round(flops_step), "hbm_gbs": round(bytes_step / t / 1e9, 1),
            "hbm_frac_of_peak": round(bytes_step / t / 1e9 / PEAK_HBM_GBS, 4),
            "algorithmic_tflops": round(flops_step / t / 1e12, 2),
            "mfma_frac_of_bf16_peak": round(flops_step / t / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4),
            "t_roof_ms": round(1000 * max(t_hbm, t_mfma), 3), "t_roof_over_t": round(max(t_hbm, t_mfma) / t, 4),
            # `t_roof` prices ALGORITHMIC flops at one MFMA per product (conservative for bf16x3); the label says which pipe actually bounds
            # the step in this mode: the MFMAs that must be issued (flops x mfma_per_product) against the HBM bytes
            "t_roof_issue_ms": round(1000 * t_issue, 3), "t_hbm_ms": round(1000 * t_hbm, 3),
            "bound": "mfma" if t_issue >= t_hbm else "hbm",
            "mfma_per_product": mfma_per_product,
            "mfma_issue_frac_of_bf16_peak": round(flops_step * mfma_per_product / t / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4),
            "formula": "SURVEY 8(d): bytes = B(A_train+D)accum + 3W accum + 28P + 1.2P; flops = 3 x 67.41 GF/img (algorithmic); "
                       "t_roof = max(bytes/8 TB/s, flops/2.5 PF); mfma_issue_* = flops x mfma_per_product (pipe occupancy, not roofline)"}


def build_workload(args, device):
    from denoising_diffusion_pytorch import GaussianDiffusion, Trainer, Unet
    import contextlib
    import io
    torch.manual_seed(123457)
    with contextlib.redirect_stdout(io.StringIO()):
        model = Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=3).to(device)
    diffusion = GaussianDiffusion(model, image_size=128, channels=3, timesteps=TIMESTEPS, loss_type='l1',
                                  sampling_routine='x0_step_down').to(device)
    trainer = Trainer(diffusion, None, image_size=128, train_batch_size=args.batch, train_lr=2e-5, train_num_steps=10 ** 9,
                      gradient_accumulate_every=args.accum, ema_decay=0.995, fp16=False, dataset='synthetic',
                      results_folder=_RESULTS.name)
    trainer.quiet = True
    return model, diffusion, trainer


class GemmTimer:
    """HIP-event timing (on the launch stream) of every MFMA GEMM launch of the step with its
    ALGORITHMIC FLOPs (zero-padded taps / channels are not counted):
      conv_igemm_sp   cdf_conv_gemm_bf16(x)   dense conv fwd + dgrad, bf16x3 split-precision MFMA
      conv_wgrad_sp   cdf_conv_wgrad_bf16(x)  weight gradients of the wide layers, bf16x3 MFMA
      conv_igemm      cdf_conv_gemm           exact-fp32 MFMA (short-K 1x1 convs, K=32 attention GEMMs, linears)
      conv_wgrad      cdf_conv_wgrad          weight gradients of the thin layers, exact-fp32 MFMA
    """
    PEAK = {"conv_igemm_sp": 2500.0, "conv_wgrad_sp": 2500.0, "conv_igemm": 157.3, "conv_wgrad": 157.3}   # dense TFLOP/s, MI355X_MICROARCH.md
    _SP = "bf16 MFMA, 3 MFMAs per product (hi/lo split operands, fp32 accumulate)"
    DTYPE = {"conv_igemm_sp": _SP, "conv_wgrad_sp": _SP, "conv_igemm": "f32 MFMA", "conv_wgrad": "f32 MFMA"}
    ENTRY = {"cdf_conv_gemm": "conv_igemm", "cdf_conv_gemm_bf16": "conv_igemm_sp", "cdf_conv_gemm_bf16x": "conv_igemm_sp",
             "cdf_conv_wgrad": "conv_wgrad", "cdf_conv_wgrad_bf16": "conv_wgrad_sp", "cdf_conv_wgrad_bf16x": "conv_wgrad_sp",
             # the typed-operand forms (bf16 activation storage): same leading arguments as the entry points they extend
             "cdf_conv_gemm_io": "conv_igemm", "cdf_conv_gemm_bf16x_io": "conv_igemm_sp"}
    ALIAS = {"cdf_conv_gemm_io": "cdf_conv_gemm", "cdf_conv_gemm_bf16x_io": "cdf_conv_gemm_bf16x"}

    def __init__(self, lib):
        self.lib, self.enabled, self.records, self.taps = lib, False, {k: [] for k in self.PEAK}, {}
        self.orig = {}
        for entry in self.ENTRY:
            self.orig[entry] = getattr(lib, entry)
            setattr(lib, entry, (lambda e: lambda *a: self._call(e, a))(entry))

    def _ntaps(self, desc, nphase):
        key = id(desc)
        if key not in self.taps:
            tot, i = 0, 0
            for _ in range(nphase):
                tot += desc[i + 2]
                i += 3 + 3 * desc[i + 2]
            self.taps[key] = (tot, desc)          # keep desc alive so id() stays unique
        return self.taps[key][0]

    def _flops(self, kind, a):
        kind = self.ALIAS.get(kind, kind)
        if kind == "cdf_conv_gemm_bf16x":   # (xhi,xlo,ldx,zero,whi,wlo,ldk,y,ldy,B,H,W,Cin,OH,OW,Cout,QH,QW,os,is,nphase,desc,...)
            return 2.0 * a[9] * a[16] * a[17] * self._ntaps(a[21], a[20]) * a[12] * a[15]
        if kind == "cdf_conv_wgrad_bf16x":  # (ahi,alo,lda,bhi,blo,ldb,zero,ws,ldo,B,QH,QW,HA,WA,sa,HB,WB,sb,CA,CB,ntaps,...)
            return 2.0 * a[9] * a[10] * a[11] * a[18] * a[19] * a[20]
        if kind == "cdf_conv_wgrad_bf16":   # (xa,lda,xb,ldb,ws,ldo,B,QH,QW,HA,WA,sa,HB,WB,sb,CA,CB,ntaps,...)
            return 2.0 * a[6] * a[7] * a[8] * a[15] * a[16] * a[17]
        if kind == "cdf_conv_gemm":       # (x,ldx,w,ldw,y,ldy,B,H,W,Cin,OH,OW,Cout,QH,QW,os,is,nphase,desc,...,batch@32,...,batch2@36)
            return 2.0 * a[6] * a[13] * a[14] * self._ntaps(a[18], a[17]) * a[9] * a[12] * a[32] * a[36]
        if kind == "cdf_conv_gemm_bf16":    # (x,ldx,whi,wlo,ldk,y,ldy,B,H,W,Cin,OH,OW,Cout,QH,QW,os,is,nphase,desc,...)
            return 2.0 * a[7] * a[14] * a[15] * self._ntaps(a[19], a[18]) * a[10] * a[13]
        # conv_wgrad: (xa,lda,xb,ldb,ws,ldo,B,QH,QW,HA,WA,sa,HB,WB,sb,CA,CB,ntaps,desc,nsplit,batch,...)
        return 2.0 * a[6] * a[7] * a[8] * a[15] * a[16] * a[17] * a[20]

    def _bytes(self, kind, a):
        """ALGORITHMIC HBM bytes of a launch (SURVEY 8(d) counts layer-boundary tensors in fp32): input map + output map + weights,
        each once -- what `traffic` (PMC) is compared with."""
        kind = self.ALIAS.get(kind, kind)
        if kind == "cdf_conv_gemm_bf16x":
            return 4.0 * (a[9] * a[10] * a[11] * a[12] + a[9] * a[13] * a[14] * a[15] + self._ntaps(a[21], a[20]) * a[12] * a[15])
        if kind == "cdf_conv_gemm_bf16":
            return 4.0 * (a[7] * a[8] * a[9] * a[10] + a[7] * a[11] * a[12] * a[13] + self._ntaps(a[19], a[18]) * a[10] * a[13])
        return None

    def _call(self, entry, a):
        if not self.enabled:
            return self.orig[entry](*a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = self.orig[entry](*a)
        e1.record()
        self.records[self.ENTRY[entry]].append((e0, e1, self._flops(entry, a), (entry,) + tuple(x for x in a[6:21] if isinstance(x, int) and x < 1 << 20),
                                                self._bytes(entry, a)))
        return r

    def dump_shapes(self, steps):
        """Per-shape time table (stderr) — which GEMMs the step spends its time in."""
        agg = {}
        for recs in self.records.values():
            for e0, e1, f, key, *_ in recs:
                t, n, fl = agg.get(key, (0.0, 0, 0.0))
                agg[key] = (t + e0.elapsed_time(e1), n + 1, fl + f)
        for key, (t, n, fl) in sorted(agg.items(), key=lambda kv: -kv[1][0])[:int(os.environ.get("CDF_BENCH_SHAPES_N", "40"))]:
            log("%8.3f ms/step %4d launches %7.1f TF  %s" % (t / steps, n // steps, fl / (t * 1e-3) / 1e12 if t > 0 else 0, key))

    def summary(self, steps, elapsed_s):
        out = {}
        for kind, recs in self.records.items():
            if not recs:
                continue
            ms = sum(e0.elapsed_time(e1) for e0, e1, *_ in recs)
            fl = sum(r[2] for r in recs)
            tf = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            out[kind] = {"arithmetic": self.DTYPE[kind], "achieved": round(tf, 2), "peak": self.PEAK[kind], "unit": "TFLOP/s",
                         "frac": round(tf / self.PEAK[kind], 4), "launches_per_step": len(recs) // max(1, steps),
                         "avg_launch_ms": round(ms / len(recs), 4), "algorithmic_gflop_per_step": round(fl / max(1, steps) / 1e9, 1),
                         "share_of_step": round(ms / (1000 * elapsed_s), 3)}
            if all(r[4] is not None for r in recs):
                out[kind]["algorithmic_bytes_per_launch"] = round(sum(r[4] for r in recs) / len(recs))
            if kind == "conv_igemm_sp":
                # the group mixes two regimes: the pre-split 3x3 / 4x4 GEMMs (matrix-core-bound) and the in-kernel-split 1x1 attention
                # projections (K = 64 ... 512 against 256 ... 1536 output channels: HBM-bound streams) -- same figures per entry point
                sub = {}
                for entry, label in (("cdf_conv_gemm_bf16x", "pre_split_3x3_4x4"), ("cdf_conv_gemm_bf16", "in_kernel_split_1x1_attention")):
                    rs = [r for r in recs if self.ALIAS.get(r[3][0], r[3][0]) == entry]
                    if not rs:
                        continue
                    m = sum(e0.elapsed_time(e1) for e0, e1, *_ in rs)
                    f = sum(r[2] for r in rs)
                    t = f / (m * 1e-3) / 1e12 if m > 0 else 0.0
                    sub[label] = {"achieved": round(t, 2), "frac": round(t / self.PEAK[kind], 4), "launches_per_step": len(rs) // max(1, steps),
                                  "algorithmic_gflop_per_step": round(f / max(1, steps) / 1e9, 1), "share_of_step": round(m / (1000 * elapsed_s), 3)}
                out[kind]["by_entry_point"] = sub
        return out


def cpu_baseline(args):
    """The CPU oracle (port of the reference's PyTorch path) on the host cores: the same optimizer
    step on a bounded sample (2 micro-steps x 2 images)."""
    from oracle import cold_oracle as O
    from colddiff.unet import Unet
    import contextlib
    import io
    ncores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    ncores = max(1, min(ncores, 64, int(os.environ.get("OMP_NUM_THREADS") or 64)))     # a CPU allowance set for the process wins
    torch.set_num_threads(ncores)
    torch.manual_seed(123457)
    with contextlib.redirect_stdout(io.StringIO()):
        sd = {k: v.clone() for k, v in Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=3).state_dict().items()}
    ca, cb = O.cosine_tables(TIMESTEPS)
    Bc = 2

    def loss_of_batch(params, x, eps, t):
        return O.loss_fn(x, O.unet_forward(params, O.noise_q_sample(x, eps, t, ca, cb), t))

    tr = O.OracleTrainer(sd, loss_of_batch, lr=2e-5, accumulate=args.accum)
    g = torch.Generator().manual_seed(123457)

    def batches():
        out = []
        for _ in range(args.accum):
            x = torch.randint(0, 256, (Bc, 3, 128, 128), generator=g).float() / 255 * 2 - 1
            out.append((x, torch.randn(Bc, 3, 128, 128, generator=g), torch.randint(0, TIMESTEPS, (Bc,), generator=g)))
        return out

    t0 = time.perf_counter()
    tr.train_step(batches())                     # warm-up 1
    warm = time.perf_counter() - t0
    log(f"cpu baseline first warm-up step: {warm:.1f}s on {ncores} threads")
    nwarm, n = (3, 5) if warm < 4.5 else ((2, 3) if warm < 9 else (1, 1))     # 3 warm-up + 5 timed; bounded to ~35 s on a slow host
    for _ in range(nwarm - 1):
        tr.train_step(batches())
    t0 = time.perf_counter()
    for _ in range(n):
        tr.train_step(batches())
    dt = (time.perf_counter() - t0) / n
    out = {"value": round(Bc * args.accum / dt, 3), "unit": "img/s", "cores": ncores, "kind": "port", "batch_per_micro_step": Bc,
           "sample": f"oracle/cold_oracle.py = bit-exact port of the reference's PyTorch CPU path (tests/test_oracle.py pins it to the live "
                     f"reference; /root/reference does not exist on the GPU box): same optimizer step, {args.accum} micro-steps x {Bc} images "
                     f"at 128x128, {n} timed steps after {nwarm} warm-up, {ncores} threads"}
    # a 2-image convolution does not scale to 64 cores -- the same step at 8 images per micro-step (a batch the host's
    # threads can share), bounded to ~40 s: one warm-up + as many timed steps as fit; `value` above stays the comparable figure of rounds 1-4
    Bc = 8
    t0 = time.perf_counter()
    tr.train_step(batches())
    warm8 = time.perf_counter() - t0
    n8 = max(1, min(3, int(30.0 / max(warm8, 1e-3))))
    if warm8 < 25.0:
        t0 = time.perf_counter()
        for _ in range(n8):
            tr.train_step(batches())
        dt8 = (time.perf_counter() - t0) / n8
        timed = f"{n8} timed steps after 1 warm-up"
    else:
        dt8, timed = warm8, "the single (first) step: the host is too slow for a warm-up inside the 40 s bound"
    out["batch8"] = {"value": round(Bc * args.accum / dt8, 3), "unit": "img/s", "cores": ncores, "batch_per_micro_step": Bc,
                     "sample": f"same port, same optimizer step at {args.accum} micro-steps x {Bc} images, {timed}, {ncores} threads"}
    return out


def selfcheck(diffusion, device):
    """The benchmarked weights on a 2-image sub-batch: micro-step loss on the HIP path vs the CPU oracle."""
    from oracle import cold_oracle as O
    g = torch.Generator().manual_seed(99)
    x = torch.randint(0, 256, (2, 3, 128, 128), generator=g).float() / 255 * 2 - 1
    e = torch.randn(2, 3, 128, 128, generator=g)
    t = torch.tensor([17, 183])
    with torch.no_grad():
        lh = float(diffusion.p_losses(x.to(device), e.to(device), t.to(device)))
        sd = {k: v.detach().cpu() for k, v in diffusion.denoise_fn.state_dict().items()}
        ca, cb = O.cosine_tables(TIMESTEPS)
        lo = float(O.loss_fn(x, O.unet_forward(sd, O.noise_q_sample(x, e, t, ca, cb), t)))
    return {"microstep_loss_hip": lh, "microstep_loss_oracle": lo, "abs_diff": abs(lh - lo), "images": 2,
            "note": "p_losses (q_sample -> UNet -> L1) of the benchmarked weights on a 2-image sub-batch, HIP path vs oracle/cold_oracle.py"}


def timed_train(trainer, steps, warmup, reps=1, warm_seconds=0.0):
    """Seconds per step: `warmup` untimed steps (and, for the 10-ms steps of the 32 x 32 configurations, as many more as it takes to run
    `warm_seconds`), then the median over `reps` repetitions of `steps` timed steps.  (Config 1 is HOST-bound: ~700 launches in ~10.4 ms
    of device time -- enqueue time equals step time, 10.4 ... 15 ms depending on what else the box's cores do, so identical runs differ by
    up to 17 %; a whole-step hipGraph replays in 10.3 ms, tools/graph_train_try.py.)"""
    t_w = time.perf_counter()
    n = 0
    while n < warmup or (time.perf_counter() - t_w) < warm_seconds:
        trainer.train_step()
        trainer.step += 1
        n += 1
        if n >= warmup and n % 8 == 0:
            torch.cuda.synchronize()                        # (the host runs ahead of the device: measure the device's time)
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            trainer.train_step()
            trainer.step += 1
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps)
    return sorted(out)[len(out) // 2]


SEC_STEPS, SEC_WARMUP = 20, 5            # secondary workloads: timed steps / warm-up steps (the 32 x 32 ones: median of 3 repetitions)
SEC_TIMING = "%d timed steps after %d warm-up (32 x 32 configurations: after at least 0.5 s of warm-up steps)" % (SEC_STEPS, SEC_WARMUP)


# forward GFLOP per image of the three networks (SURVEY.md 8(a) [probe]); a train step = 3 x forward (fwd + dgrad + wgrad)
_FWD_GFLOP = {"unet128": 67.41, "unet32": 4.21, "model32": 12.44}


def _alg(net, img_per_s, mfma_per_product):
    """Algorithmic TFLOP/s of a secondary train line and its fraction of the dense bf16 MFMA peak (x the MFMAs each product issues =
    the matrix-pipe occupancy); exact-fp32 lines are priced against the 157.3 TFLOP/s fp32 MFMA peak."""
    tf = 3 * _FWD_GFLOP[net] * img_per_s / 1e3
    if mfma_per_product == 0:
        return {"algorithmic_tflops": round(tf, 1), "frac_of_f32_mfma_peak": round(tf / 157.3, 3)}
    return {"algorithmic_tflops": round(tf, 1), "frac_of_bf16_mfma_peak": round(tf / 2500.0, 4), "mfma_issue_frac_of_bf16_peak": round(mfma_per_product * tf / 2500.0, 4)}


def _mpp():
    from colddiff import runtime
    return {"f32": 0, "bf16x3": 3, "bf16": 1}[runtime.precision]


def _dtype_label():
    from colddiff import runtime
    if runtime.precision == "f32":
        return "f32 everywhere: exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) for every GEMM"
    return "f32 storage/accumulate; dense-conv GEMM operands " + runtime.precision


def secondary_workloads(device):
    """BASELINE configs 1, 2, 4 and 5 on the same engine (secondary keys; the judged line stays config 3).  Every entry names its
    arithmetic (`dtype`); configs 1 and 2 -- fp32 in BASELINE.json -- are ALSO timed in the exact-fp32 mode (`*_f32`)."""
    import contextlib
    import io
    from colddiff import runtime
    from colddiff.trainer import Trainer
    out = {}
    quiet = lambda: contextlib.redirect_stdout(io.StringIO())
    res = _RESULTS.name
    # ---- config 4: CelebA-128 deblurring, Exponential_reflect T=200 k=15 std=0.01 (celebA_128.py) ------------------------
    from deblurring_diffusion_pytorch import GaussianDiffusion, Model, Unet
    torch.manual_seed(123457)
    with quiet():
        net = Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=3).to(device)
        d = GaussianDiffusion(net, image_size=128, device_of_kernel='cuda', channels=3, timesteps=200, loss_type='l1', kernel_std=0.01,
                              kernel_size=15, blur_routine='Exponential_reflect', train_routine='Final', sampling_routine='x0_step_down').to(device)
        tr = Trainer(d, None, image_size=128, train_batch_size=32, train_lr=2e-5, train_num_steps=10 ** 9, gradient_accumulate_every=2,
                     dataset='synthetic', results_folder=res)
    tr.quiet = True
    dt = timed_train(tr, SEC_STEPS, SEC_WARMUP)
    out["cfg4_celeba128_deblur_train"] = {"img_per_s": round(64 / dt, 1), "ms_per_step": round(1000 * dt, 2), "timing": SEC_TIMING, "dtype": _dtype_label(),
                                          "roofline": _alg("unet128", 64 / dt, _mpp()),
                                          "workload": "Unet(64,(1,2,4,8)) @128x128, blur Exponential_reflect T=200 k=15 std=0.01, 2 x 32 img + Adam"}
    with torch.no_grad():
        x = tr._next_batch()[:16]
        with quiet():
            d.sample(batch_size=16, img=x, t=2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with quiet():
            d.sample(batch_size=16, img=x)
        torch.cuda.synchronize()
        dts = time.perf_counter() - t0
    out["cfg4_celeba128_deblur_sample"] = {"ms_per_img": round(1000 * dts / 16, 2), "batch": 16, "dtype": _dtype_label(),
                                           "workload": "Algorithm 2 (x0_step_down), T=200: 200 UNet calls + D(x0,t), D(x0,t-1) blur chains (T(T+1)/2 steps each) per image"}
    del tr, d, net
    torch.cuda.empty_cache()
    # ---- config 2: CIFAR-10 deblurring, Model(ch=128,(1,2,2,2)), Special_6_routine T=50, batch 128 (cifar10_train.py) -----
    def cfg2(key):
        torch.manual_seed(123457)
        with quiet():
            net = Model(resolution=32, in_channels=3, out_ch=3, ch=128, ch_mult=(1, 2, 2, 2), num_res_blocks=2, attn_resolutions=(16,), dropout=0.1).to(device)
            d = GaussianDiffusion(net, image_size=32, device_of_kernel='cuda', channels=3, timesteps=50, loss_type='l1', kernel_std=0.1, kernel_size=11,
                                  blur_routine='Special_6_routine', train_routine='Final', sampling_routine='x0_step_down').to(device)
            tr = Trainer(d, None, image_size=32, train_batch_size=128, train_lr=2e-5, train_num_steps=10 ** 9, gradient_accumulate_every=2,
                         dataset='synthetic', results_folder=res)
        tr.quiet = True
        dt = timed_train(tr, SEC_STEPS, SEC_WARMUP, reps=3, warm_seconds=0.5)
        out[key] = {"img_per_s": round(256 / dt, 1), "ms_per_step": round(1000 * dt, 2), "timing": SEC_TIMING + ", median of 3", "dtype": _dtype_label(),
                    "roofline": _alg("model32", 256 / dt, _mpp()),
                    "workload": "Model(ch=128,(1,2,2,2),attn@16,dropout 0.1) @32x32, blur Special_6_routine T=50, 2 x 128 img + Adam"}
        del tr, d, net
        torch.cuda.empty_cache()

    cfg2("cfg2_cifar10_deblur_train")
    if runtime.precision != "f32":
        with runtime.precision_scope("f32"):
            runtime.bump_weights_epoch()
            cfg2("cfg2_cifar10_deblur_train_f32")
        runtime.bump_weights_epoch()
    # ---- configs 1 and 5 (the remaining BASELINE configurations; the builders are those of tools/cfgbench.py) ---------------------------
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import cfgbench
    def other(cfg, key):
        torch.manual_seed(123457)
        d, size, batch, desc = cfgbench.build(cfg, device)
        with quiet():
            tr = Trainer(d, None, image_size=size, train_batch_size=batch, train_lr=2e-5, train_num_steps=10 ** 9, gradient_accumulate_every=2,
                         dataset='synthetic', results_folder=res)
        tr.quiet = True
        reps = 3 if cfg == "1" else 1
        dt = timed_train(tr, SEC_STEPS, SEC_WARMUP, reps=reps, warm_seconds=0.5 if cfg == "1" else 0.0)
        out[key] = {"img_per_s": round(2 * batch / dt, 1), "ms_per_step": round(1000 * dt, 2), "workload": desc + ", 2 micro-steps + Adam",
                    "timing": SEC_TIMING + (", median of 3" if reps > 1 else ""), "dtype": _dtype_label(),
                    "roofline": _alg("unet32" if cfg == "1" else "unet128", 2 * batch / dt, _mpp())}
        del tr, d
        torch.cuda.empty_cache()

    for cfg, key in (("1", "cfg1_mnist32_deblur_train"), ("5r", "cfg5_afhq128_resolution_train"), ("5f", "cfg5_afhq128_defading_train")):
        other(cfg, key)
    if runtime.precision != "f32":
        with runtime.precision_scope("f32"):
            runtime.bump_weights_epoch()
            other("1", "cfg1_mnist32_deblur_train_f32")
        runtime.bump_weights_epoch()
    return out


def _profile(name):
    """Newest committed profiles/round<N>_<name> (bench.py cannot run the profiler on itself)."""
    for rnd in (6, 5, 4, 3, 2, 1):
        path = os.path.join(REPO, "profiles", "round%d_%s" % (rnd, name))
        if os.path.exists(path):
            return path
    return None


def _provenance(path, doc):
    """Is this committed profile a measurement of the kernels this process runs?  tools/prof_summary.py / tools/pmc_traffic.py stamp the git
    HEAD and a digest of csrc/*.hip, csrc/*.h, include/*.h into what they write (tools/provenance.py); a profile without a stamp, or
    with another digest, describes other kernels and nothing is quoted from it."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import provenance
    st = doc.get("provenance") or doc.get("_provenance") or {}
    now = provenance.csrc_sha16()
    return {"file": os.path.relpath(path, REPO), "profile_git_head": st.get("git_head"), "profile_csrc_sha16": st.get("csrc_sha16"),
            "running_csrc_sha16": now, "match": st.get("csrc_sha16") == now}


def measured_bytes_step(profile_name):
    """HBM bytes per optimizer step as the PMC counters saw them (sum over every kernel of FETCH_SIZE x 2 + WRITE_SIZE per launch x its
    launches, divided by the Adam launches of the run): tools/pmc_traffic.py over two rocprofv3 --pmc passes of this same command, committed
    under profiles/.  None when there is no such profile or it was taken from other kernel sources."""
    tp = _profile(profile_name)
    if not tp:
        return None
    doc = json.load(open(tp))
    prov = _provenance(tp, doc)
    if not prov["match"] or not doc.get("hbm_bytes_per_optimizer_step"):
        return {"bytes_step": None, "provenance": prov}
    return {"bytes_step": round(doc["hbm_bytes_per_optimizer_step"]), "optimizer_steps_in_profile": doc["optimizer_steps"], "provenance": prov}


def bandwidth_classes():
    """HBM GB/s of the bandwidth-bound kernel classes: bytes per launch from the committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes
    (tools/pmc_traffic.py) divided by the average launch duration of the committed rocprofv3 --kernel-trace of the same command
    (bench.py cannot run the profiler on itself)."""
    tp, kp = _profile("pmc_traffic.json"), _profile("kernel_trace.json")
    if not (tp and kp):
        return None
    tdoc, trace = json.load(open(tp)), json.load(open(kp))
    prov = [_provenance(tp, tdoc), _provenance(kp, trace)]
    if not all(p["match"] for p in prov):
        return {"stale": True, "provenance": prov,
                "note": "the committed profiles were taken from other kernel sources than the ones running: no per-class figures quoted"}
    traffic = tdoc["kernels"]
    classes = {"depthwise 7x7": ("dwconv7_kernel", "dwconv7_wgrad_partial_kernel", "dwconv7_wgrad_partial_narrow_kernel"), "channel LayerNorm": ("layernorm_c_fwd_kernel", "layernorm_c_bwd_kernel"),
               "Adam": ("adam_kernel",), "operand split": ("split_bf16_kernel",), "split-K reduction": ("unpack_reduce_",),
               "linear attention": ("linattn_",)}
    out = {}
    for name, prefixes in classes.items():
        b = t = 0.0
        for k, v in traffic.items():
            if k.startswith(prefixes) and k in trace:
                b += v["hbm_bytes_per_launch"] * trace[k]["calls"]
                t += trace[k]["total_ms"] * 1e-3
        if t > 0:
            out[name] = {"hbm_gbs": round(b / t / 1e9, 1), "frac_of_peak": round(b / t / 1e9 / PEAK_HBM_GBS, 3)}
    out["source"] = "%s (FETCH_SIZE x2 + WRITE_SIZE per launch) / %s (avg duration): committed rocprofv3 passes over this same command" % (
        os.path.relpath(tp, REPO), os.path.relpath(kp, REPO))
    out["provenance"] = prov
    return out


TAIL_CLASSES = (   # (class, kernel-name prefixes) -- everything that is NOT one of the two pre-split GEMM groups
    ("pre_split_fwd_dgrad_gemm", ("conv_igemm_halo_kernel", "conv_igemm_rowhalo_stream_kernel", "conv_igemm_spx_kernel", "conv_splitk_finish_kernel")),
    ("pre_split_wgrad_gemm", ("conv_wgrad_row3_kernel", "conv_wgrad_spx_kernel")),
    ("depthwise_7x7", ("dwconv7_kernel", "dwconv7_wgrad_partial")),
    ("layernorm", ("layernorm_c_",)),
    ("in_kernel_split_gemm", ("conv_igemm_sp_kernel", "conv_wgrad_sp_kernel", "linattn_kvctx_kernel")),
    ("exact_fp32_gemm", ("conv_igemm_kernel", "conv_wgrad_kernel")),
    ("splitk_and_column_reductions", ("unpack_reduce", "colsum_", "norm_param_reduce_kernel", "dwconv7_wgrad_final_kernel")),
    ("operand_split_and_weight_packing", ("split_bf16_kernel", "widen_bf16_kernel", "pack_")),
    ("linear_attention", ("linattn_",)),
    ("direct_3_channel_convs", ("conv_cin4_", "tapsum3_kernel")),
    ("time_mlp", ("linear_small", "act_", "sinusoidal_kernel")),
    ("adam_ema", ("adam_kernel", "ema_kernel")),
    ("copies_and_fills", ("__amd_rocclr_", "at::native")),
)


def tail_ms_per_step(profile_name="kernel_trace.json"):
    """Kernel time per optimizer step by class from the committed rocprofv3 --kernel-trace of this same command (steps = adam_kernel
    launches), and `tail_ms` = everything outside the two pre-split GEMM groups (the tail as a driver-visible number).
    Quoted only from a profile of the kernel sources that are running."""
    kp = _profile(profile_name)
    if not kp:
        return None
    trace = json.load(open(kp))
    prov = _provenance(kp, trace)
    if not prov["match"]:
        return {"stale": True, "provenance": prov}
    steps = (trace.get("adam_kernel") or {}).get("calls") or 0
    if not steps:
        return None
    per = {c: 0.0 for c, _ in TAIL_CLASSES}
    per["other"] = 0.0
    launches = 0
    for name, v in trace.items():
        if not isinstance(v, dict) or "total_ms" not in v:
            continue
        launches += v["calls"]
        for c, prefixes in TAIL_CLASSES:
            if name.startswith(prefixes):
                per[c] += v["total_ms"]
                break
        else:
            per["other"] += v["total_ms"]
    out = {c: round(ms / steps, 3) for c, ms in per.items()}
    gemm = out["pre_split_fwd_dgrad_gemm"] + out["pre_split_wgrad_gemm"]
    total = sum(out.values())
    return {"by_class_ms": out, "kernel_ms": round(total, 3), "tail_ms": round(total - gemm, 3), "dispatches_per_step": round(launches / steps, 1),
            "steps_in_profile": steps, "source": os.path.relpath(kp, REPO) + " (rocprofv3 --kernel-trace of this command; the first steps of a run "
            "include initialisation copies / packs)", "provenance": prov}


DUMP_SAMPLE = 1 << 21          # arena elements sampled per dumped state vector (4 x 8 MB of float32)
DUMP_SEED = 20240913


def dump_outputs(folder, trainer, loss):
    """What the last timed optimizer step hands its caller: the step's loss, and the state it leaves behind -- parameters, Adam's
    two moments, the EMA weights.  The flat arenas hold 56.6 M values each, so the same fixed, seeded set of DUMP_SAMPLE positions
    (sorted) is taken from every one of them; `sample_index.npy` records those positions."""
    import numpy as np
    os.makedirs(folder, exist_ok=True)
    n = trainer.arena.numel
    idx = np.unique(np.random.default_rng(DUMP_SEED).integers(0, n, size=min(DUMP_SAMPLE, n)))
    sel = torch.from_numpy(idx).to(trainer.arena.data.device)
    arrays = {"loss": loss.detach().float().reshape(1),
              "params_sample": trainer.arena.data[sel],
              "adam_exp_avg_sample": trainer.opt.exp_avg[sel],
              "adam_exp_avg_sq_sample": trainer.opt.exp_avg_sq[sel],
              "ema_params_sample": trainer.ema_arena.data[sel]}
    for name, t in arrays.items():
        np.save(os.path.join(folder, name + ".npy"), t.cpu().numpy().astype(np.float32))
    np.save(os.path.join(folder, "sample_index.npy"), idx.astype(np.float64))
    log(f"outputs of the last timed step written to {folder}: {', '.join(sorted(arrays))}, sample_index")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32, help="images per micro-step per GPU (reference scripts: 32)")
    ap.add_argument("--accum", type=int, default=2, help="gradient_accumulate_every (reference scripts: 2)")
    ap.add_argument("--sample-batch", type=int, default=16)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-sample", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the bf16-mode line, the config 1 / 2 / 4 / 5 secondary workloads and the self-check")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's loss and a seeded sample of the state it leaves as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline figure: roofline pass, sampler, unfused step, self-check, "
                         "bf16 / f32 lines, secondary workloads, CPU baseline (each --no-* option still drops its part)")
    args = ap.parse_args()

    from colddiff import parallel, runtime
    world = parallel.world_size()
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world} (launch with torch.distributed.run)"
    assert torch.cuda.is_available(), "bench.py needs the MI355X (no CPU fallback)"
    if world > 1:
        # RCCL over xGMI; COLDDIFF_DIST_BACKEND=gloo exists only so that the multi-rank code path can be exercised with several ranks on
        # ONE GPU (RCCL refuses two ranks per device)
        parallel.init_distributed(os.environ.get("COLDDIFF_DIST_BACKEND", "nccl"))
    device = torch.device("cuda", parallel.local_rank() % torch.cuda.device_count())
    torch.cuda.set_device(device)

    log(f"building workload on {device} (world {world})")
    model, diffusion, trainer = build_workload(args, device)
    timer = GemmTimer(runtime.lib()) if args.full else None
    use_timer = args.full and os.environ.get("CDF_BENCH_NOTIMER", "0") != "1"
    log("workload built")

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for i in range(args.warmup):
        trainer.train_step()
        trainer.step += 1
        torch.cuda.synchronize()
        log(f"warm-up step {i} done")
    barrier()
    t0 = time.perf_counter()
    loss = None
    for _ in range(args.steps):
        loss = trainer.train_step()
        trainer.step += 1
    barrier()
    elapsed = time.perf_counter() - t0
    log(f"timed {args.steps} steps: {elapsed:.3f}s")
    if world > 1:
        tt = torch.tensor([elapsed], device=device, dtype=torch.float64)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        elapsed = tt.item()
    if args.dump_outputs and parallel.rank() == 0 and loss is not None:
        dump_outputs(args.dump_outputs, trainer, loss)        # before any --full pass below runs further steps on the same weights

    # Roofline pass: the SAME K steps again, now with a HIP-event pair around every MFMA GEMM launch (on the launch
    # stream).  Kept out of the timed region above because ~1000 event records per step cost 3 % of throughput; the
    # instrumented steps' own wall time is reported next to the kernel figures.
    dp_stats = None
    if args.full and world > 1 and trainer.sync is not None:
        # how much of the gradient exchange the backward pass hides: a few further steps with events around every bucket's all-reduce
        trainer.sync.profile = True
        barrier()
        for _ in range(min(args.steps, 4)):
            trainer.train_step()
            trainer.step += 1
        barrier()
        trainer.sync.profile = False
        dp_stats = trainer.sync.stats()
    elapsed_instr = None
    if use_timer:
        timer.enabled = True
        barrier()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            trainer.train_step()
            trainer.step += 1
        barrier()
        elapsed_instr = time.perf_counter() - t1
        timer.enabled = False
        log(f"instrumented {args.steps} steps: {elapsed_instr:.3f}s")

    imgs_per_step = args.batch * args.accum * world
    value = imgs_per_step * args.steps / elapsed
    kernels = timer.summary(args.steps, elapsed_instr if elapsed_instr else elapsed) if timer else {}
    if timer and os.environ.get("CDF_BENCH_SHAPES"):
        timer.dump_shapes(args.steps)

    out = {
        "metric": "unet_train_imgs_per_sec", "value": round(value, 2), "unit": "img/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(1000 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32" if runtime.precision == "f32" else ("f32 storage/accumulate; dense-conv GEMM operands " + runtime.precision),
        "data": "synthetic",
        "config": {"workload": "CelebA-128 denoising cold diffusion (BASELINE config 3): Unet(dim=64,(1,2,4,8),ch=3) @128x128, T=200, "
                               "optimizer step = %d micro-batches x %d img (%s) + Adam + EMA/10"
                               % (args.accum, args.batch, "one fused forward / backward pass over all of them: same draws, same gradient sum"
                                  if trainer._can_fuse() else "separate micro-steps"), "per_gpu_batch": args.batch,
                   "gradient_accumulate_every": args.accum, "global_images_per_step": imgs_per_step,
                   "parallelism": f"dp{world}" if world > 1 else "single"},
    }
    if dp_stats:
        out["gradient_exchange"] = dict(dp_stats, backend=torch.distributed.get_backend(),
                                        note="sum all-reduce of the flat fp32 gradient arena, bucketed in runs of whole tensors, issued on a side "
                                             "stream during backward of the last accumulation micro-step; exposed = after backward ended")
    if parallel.rank() == 0 and args.full:
        dom = max(kernels, key=lambda k: kernels[k]["share_of_step"]) if kernels else None
        if dom:
            d = kernels[dom]
            out["roofline"] = {"bound": "mfma", "kernel": dom, "arithmetic": d["arithmetic"], "achieved": d["achieved"], "peak": d["peak"],
                               "unit": "TFLOP/s", "frac": d["frac"], "traffic": None, "launches_per_step": d["launches_per_step"],
                               "avg_launch_ms": d["avg_launch_ms"], "algorithmic_gflop_per_step": d["algorithmic_gflop_per_step"],
                               "algorithmic_bytes_per_launch": d.get("algorithmic_bytes_per_launch"),
                               # the data-sheet peak above is what `frac` is taken against; the same instruction sustains 1.82 PF on random bf16
                               # operands with nothing else running (profiles/round2_mfma_power.md): MFMA issue rate against that ceiling
                               "mfma_issue_tflops": round(d["achieved"] * npp_of(runtime.precision), 1),
                               "measured_mfma_ceiling_random_operands_tflops": MEASURED_MFMA_CEILING_TFLOPS,
                               "mfma_issue_frac_of_measured_ceiling": round(d["achieved"] * npp_of(runtime.precision) / MEASURED_MFMA_CEILING_TFLOPS, 4),
                               "share_of_step": d["share_of_step"],
                               "measured": "HIP events around every launch of %d further steps run right after the timed region "
                                           "(%.1f ms/step with the ~1000 event records per step, %.1f ms/step without)"
                                           % (args.steps, 1000 * elapsed_instr / args.steps, 1000 * elapsed / args.steps)}
            # HBM traffic of that kernel group from the committed rocprofv3 --pmc passes over this same command
            # (tools/pmc_traffic.py; bench.py cannot run the profiler on itself)
            tpath = _profile("pmc_traffic.json")
            if tpath and dom == "conv_igemm_sp":
                tdoc = json.load(open(tpath))
                prov = _provenance(tpath, tdoc)
                out["roofline"]["traffic_provenance"] = prov
                g = tdoc.get("conv_igemm_sp")
                if g and prov["match"]:            # a profile of other kernel sources is not quoted: traffic stays null
                    out["roofline"]["traffic"] = round(g["hbm_bytes_per_launch"])
                    if d.get("algorithmic_bytes_per_launch"):
                        out["roofline"]["traffic_over_algorithmic_bytes"] = round(g["hbm_bytes_per_launch"] / d["algorithmic_bytes_per_launch"], 3)
                    out["roofline"]["traffic_unit"] = "HBM bytes per launch (FETCH_SIZE x2 + WRITE_SIZE, %s)" % os.path.relpath(tpath, REPO)
        out["gemm_kernels"] = kernels
        # whole-step view: layer-boundary bytes and 3 x F_fwd flops per image against the HBM / MFMA roofs
        npp = {"bf16x3": 3, "bf16": 1}.get(runtime.precision, 16)      # MFMAs per algorithmic product (f32: the 16x slower fp32 MFMA)
        out["step_roofline"] = step_roofline(args.batch, args.accum, 1000 * elapsed / args.steps, npp)
        mb = measured_bytes_step("pmc_traffic.json")
        if mb:
            out["step_roofline"]["measured_hbm_bytes_step"] = mb["bytes_step"]
            out["step_roofline"]["measured_over_algorithmic_bytes"] = round(mb["bytes_step"] / out["step_roofline"]["bytes_step"], 3) if mb["bytes_step"] else None
            out["step_roofline"]["measured_provenance"] = mb["provenance"]
        step_tflops = 3 * UNET128_FWD_GFLOP * args.batch * args.accum * args.steps / elapsed / 1e3
        out["step_algorithmic_tflops"] = round(step_tflops, 2)
        out["step_frac_of_f32_mfma_peak"] = round(step_tflops / PEAK_F32_MFMA_TFLOPS, 4)
        bw = bandwidth_classes()
        if bw:
            out["hbm_bound_kernel_classes"] = bw
        tail = tail_ms_per_step()
        if tail:
            out["tail_ms_per_step"] = tail
        if world == 1 and not args.no_sample:
            with torch.no_grad():
                noise = torch.randn(args.sample_batch, 3, 128, 128, device=device)
                trainer.ema_core.gen_sample(batch_size=args.sample_batch, img=noise, t=2)      # warm-up
                torch.cuda.synchronize()
                ts = time.perf_counter()
                trainer.ema_core.gen_sample(batch_size=args.sample_batch, img=noise)
                torch.cuda.synchronize()
                out["sample_ms_per_img_200step"] = round(1000 * (time.perf_counter() - ts) / args.sample_batch, 2)
                log(f"200-step gen_sample of {args.sample_batch} images: {time.perf_counter() - ts:.2f}s")
                out["sample_batch"] = args.sample_batch
                if not args.no_secondary:
                    # the same sampler at a batch that fills the deep 16 x 16 layers (at 16 images half of their tiles' CUs idle)
                    noise64 = torch.randn(64, 3, 128, 128, device=device)
                    torch.cuda.synchronize()
                    ts = time.perf_counter()
                    trainer.ema_core.gen_sample(batch_size=64, img=noise64)
                    torch.cuda.synchronize()
                    out["sample_ms_per_img_200step_batch64"] = round(1000 * (time.perf_counter() - ts) / 64, 2)
                    del noise64
        if world == 1 and not args.no_secondary and trainer._can_fuse():
            # the same optimizer step with the reference's separate micro-steps (what rounds 1-3 timed): labelled, beside `value`
            os.environ["COLDDIFF_FUSE_ACCUM"] = "0"
            dtu = timed_train(trainer, args.steps, 2)
            del os.environ["COLDDIFF_FUSE_ACCUM"]
            out["accumulation"] = {"fused": True, "unfused_img_per_s": round(args.batch * args.accum / dtu, 2), "unfused_ms_per_step": round(1000 * dtu, 3),
                                   "note": "fused = the %d micro-batches of a step as one pass (loss of the concatenated batch = mean of the micro-batch "
                                           "losses); unfused = (loss_i / %d).backward() per micro-batch as DEBLUR:1188-1195 writes it" % (args.accum, args.accum)}
            log(f"unfused accumulation: {out['accumulation']['unfused_img_per_s']} img/s")
        if world == 1 and not args.no_secondary:
            out["selfcheck"] = selfcheck(diffusion, device)
            log("self-check: loss hip %.6f oracle %.6f" % (out["selfcheck"]["microstep_loss_hip"], out["selfcheck"]["microstep_loss_oracle"]))
            if runtime.precision == "bf16x3":
                # second, LABELLED line: the same step with single-pass bf16 GEMM operands (BASELINE config 3 names bf16).  Not parity
                # grade (tolerance below); reported beside the parity-grade `value`, never instead of it.
                runtime.set_precision("bf16")
                runtime.bump_weights_epoch()
                from colddiff import bf16store
                stored_bf16 = bf16store.enabled_for(model)       # (asked while the mode is on: which engine the timed steps below run)
                dtb = timed_train(trainer, args.steps, args.warmup)
                sample_bf16 = None
                if not args.no_sample:
                    with torch.no_grad():
                        noise = torch.randn(args.sample_batch, 3, 128, 128, device=device)
                        trainer.ema_core.gen_sample(batch_size=args.sample_batch, img=noise, t=2)
                        torch.cuda.synchronize()
                        ts = time.perf_counter()
                        trainer.ema_core.gen_sample(batch_size=args.sample_batch, img=noise)
                        torch.cuda.synchronize()
                        sample_bf16 = round(1000 * (time.perf_counter() - ts) / args.sample_batch, 2)
                runtime.set_precision("bf16x3")
                runtime.bump_weights_epoch()
                out["bf16_mode"] = {"value": round(args.batch * args.accum / dtb, 2), "unit": "img/s", "ms_per_step": round(1000 * dtb, 3),
                                    "dtype": "bf16 GEMM operands (one MFMA per product) AND bf16 activation storage: one bf16 plane is the only stored form of "
                                             "every GEMM input, every activation saved for backward and the inter-block residual stream in both directions "
                                             "(colddiff/bf16store.py); fp32: accumulators, norm statistics, softmax / context, the image-side block's "
                                             "4-channel tensors, time biases, master weights, parameter gradients, degradation, loss, optimizer"
                                             if stored_bf16 else
                                             "bf16 GEMM operands (one MFMA per product), fp32 accumulate / master weights / norms / softmax / degradation / "
                                             "optimizer; fp32 tensors between kernels (COLDDIFF_BF16_STORAGE=0: the round 2-4 form of the mode)",
                                    "activation_storage": "bf16" if stored_bf16 else "f32",
                                    "tolerance_vs_fp32_oracle": dict(runtime.BF16_TOLERANCE, asserted_by="tests/test_gpu_parity2.py::"
                                                                     "test_other_precision_modes_module_level[bf16] and ::test_bf16_mode_bench_shape_fused_step "
                                                                     "(the fused 64-image pass), tests/test_bf16_storage.py"),
                                    "sample_ms_per_img_200step": sample_bf16, "sample_batch": args.sample_batch,
                                    # the accounting describes the engine that runs: SURVEY 8(d)'s bf16 column (A_train = 549 MB / image) now that the
                                    # tensors between kernels ARE bf16
                                    "step_roofline": step_roofline(args.batch, args.accum, 1000 * dtb, 1, act="bf16" if stored_bf16 else "f32")}
                tb = tail_ms_per_step("kernel_trace_bf16.json")
                if tb:
                    out["bf16_mode"]["tail_ms_per_step"] = tb
                mbb = measured_bytes_step("pmc_traffic_bf16.json")
                if mbb:
                    out["bf16_mode"]["step_roofline"]["measured_hbm_bytes_step"] = mbb["bytes_step"]
                    out["bf16_mode"]["step_roofline"]["measured_provenance"] = mbb["provenance"]
                log(f"bf16 mode: {out['bf16_mode']['value']} img/s")
                # third, LABELLED line: the lower anchor -- every GEMM on the exact-fp32 matrix-core instruction (v_mfma_f32_32x32x2_f32,
                # 157 TFLOP/s dense), i.e. IEEE fp32 products; `value` above keeps 16 mantissa bits per operand and drops a_lo b_lo
                runtime.set_precision("f32")
                runtime.bump_weights_epoch()
                dtf = timed_train(trainer, max(2, args.steps // 2), 1)
                runtime.set_precision("bf16x3")
                runtime.bump_weights_epoch()
                out["f32_mode"] = {"value": round(args.batch * args.accum / dtf, 2), "unit": "img/s", "ms_per_step": round(1000 * dtf, 3),
                                   "dtype": "f32 everywhere: exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) for every GEMM (COLDDIFF_PRECISION=f32)",
                                   "step_frac_of_f32_mfma_peak": round(3 * UNET128_FWD_GFLOP * args.batch * args.accum / dtf / 1e3 / PEAK_F32_MFMA_TFLOPS, 4)}
                log(f"f32 mode: {out['f32_mode']['value']} img/s")
            del trainer
            torch.cuda.empty_cache()
            out["secondary"] = secondary_workloads(device)
            log("secondary workloads done")
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args)
    if parallel.rank() == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
