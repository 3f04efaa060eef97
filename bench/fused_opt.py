#!/usr/bin/env python3
"""What does the fused optimizer pass cost at the config-5 bucket, and what
did the same update cost before it existed?

At 41 755 624 elements (the 4096-8192-1000 MLP: 167 MB of fp32 gradients), one
contributor, every variant one call between device events, all variants
alternating over the repetitions:

  fused   AllReduceOutput.optim_step_: SGD-momentum / AdamW, from an fp32 or a
          bf16 sum, with and without the bf16 shadow and the global-norm clip
          (the clip is a second launch: count_sqnorm over the sum), each with
          plain and with nontemporal accesses (``nt``)
  torch   the composition available without it: out.mean(out=flat), then
          clip_grad_norm_, then torch.optim.AdamW(fused=True) / SGD(momentum)
          over the model's four parameter tensors, then sflat.copy_(pflat)

Bytes are the ones the update must move, from the shapes: the sum (4 or 2 B,
twice with a clip), p and m read and written (16 B), v read and written for
AdamW (8 B), the shadow written (2 B).  The torch composition is charged the
same bytes, so its GB/s is a rate of useful work, not of traffic.

One JSON line per variant: median / min / max microseconds, GB/s at the median.
GPU only: without a device this fails.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SHAPES = ((8192, 4096), (8192,), (1000, 8192), (1000,))  # fc1.weight, fc1.bias, fc2.weight, fc2.bias


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench/fused_opt.py needs a GPU")
    if a.reps < 20:
        raise SystemExit("--reps: at least 20")
    from akka_allreduce_amd.data import AllReduceOutput, Geometry, sqnorm_workspace

    dev = torch.device("cuda", 0)
    n = sum(torch.Size(s).numel() for s in SHAPES)
    gen = torch.Generator(device=dev).manual_seed(0)
    sums = {"fp32": torch.randn(n, device=dev, generator=gen) * 1e-2}
    sums["bf16"] = sums["fp32"].bfloat16()
    geo = Geometry(n, 1, 1 << 20)
    pc = torch.ones((1, geo.kmax), device=dev, dtype=torch.int32)
    outs = {k: AllReduceOutput(s, counts_per_chunk=pc, geometry=geo) for k, s in sums.items()}
    pflat = torch.randn(n, device=dev, generator=gen)
    flat = torch.zeros(n, device=dev)
    sflat = torch.empty(n, device=dev, dtype=torch.bfloat16)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    t = torch.zeros(1, device=dev, dtype=torch.int32)
    ws = sqnorm_workspace(dev)
    max_norm = 1.0
    hyper = {"sgd": dict(momentum=0.9, weight_decay=1e-2), "adamw": dict(weight_decay=0.01)}
    lr = {"sgd": 0.05, "adamw": 1e-3}

    # the torch composition: parameters and gradients as views of the flat buffers
    params, off = [], 0
    for shp in SHAPES:
        k = torch.Size(shp).numel()
        p = torch.nn.Parameter(pflat[off:off + k].view(shp))
        p.grad = flat[off:off + k].view(shp)
        params.append(p)
        off += k
    topt, timpl = {}, {}
    for kind, cls, kw in (("sgd", torch.optim.SGD, dict(lr=lr["sgd"], momentum=0.9, weight_decay=1e-2)),
                          ("adamw", torch.optim.AdamW, dict(lr=lr["adamw"], weight_decay=0.01))):
        try:
            topt[kind], timpl[kind] = cls(params, fused=True, **kw), "fused"
        except (RuntimeError, TypeError, ValueError):
            topt[kind], timpl[kind] = cls(params, **kw), "default"

    def nbytes(kind, src, shadow, clip):
        sb = 4 if src == "fp32" else 2
        return n * (sb * (2 if clip else 1) + 16 + (8 if kind == "adamw" else 0) + (2 if shadow else 0))

    def fused(kind, src, shadow, clip, nt):
        def run():
            t.add_(1)
            outs[src].optim_step_(kind, pflat, m, v if kind == "adamw" else None, t, lr[kind],
                                  shadow=sflat if shadow else None, max_norm=max_norm if clip else None,
                                  norm_ws=ws if clip else None, nt=nt, **hyper[kind])
        return run

    def composed(kind, src, shadow, clip):
        def run():
            if src == "bf16":
                outs[src].mean(out=flat, dtype=torch.float32)
            else:
                outs[src].mean(out=flat)
            if clip:
                torch.nn.utils.clip_grad_norm_(params, max_norm)
            topt[kind].step()
            if shadow:
                sflat.copy_(pflat)
        return run

    variants = {}
    for kind in ("sgd", "adamw"):
        for src in ("fp32", "bf16"):
            for shadow in (False, True):
                for clip in (False, True):
                    tag = f"{kind}_{src}{'_shadow' if shadow else ''}{'_clip' if clip else ''}"
                    b = nbytes(kind, src, shadow, clip)
                    variants[f"fused_plain_{tag}"] = (fused(kind, src, shadow, clip, False), b, "plain")
                    variants[f"fused_nt_{tag}"] = (fused(kind, src, shadow, clip, True), b, "nontemporal")
                    variants[f"torch_{tag}"] = (composed(kind, src, shadow, clip), b, timpl[kind])
    us = {k: [] for k in variants}
    for rep in range(a.warmup + a.reps):
        for name, (fn, _, _) in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if rep >= a.warmup:
                us[name].append(t0.elapsed_time(t1) * 1e3)
    lines = []
    for name, (_, b, impl) in variants.items():
        med = statistics.median(us[name])
        lines.append(json.dumps({"variant": name, "impl": impl, "elements": n, "bytes": b, "reps": len(us[name]),
                                 "us_median": round(med, 1), "us_min": round(min(us[name]), 1),
                                 "us_max": round(max(us[name]), 1), "gbps_median": round(b / med / 1e3, 1)}))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
