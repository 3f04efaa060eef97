#!/usr/bin/env python3
"""What do bf16 moments save the fused optimizer pass at the config-5 bucket?

Same bucket and conventions as ``bench/fused_opt.py``: 41 755 624 elements
(the 4096-8192-1000 MLP), one contributor, every variant one call between
device events, all variants alternating over the repetitions.

  {SGD-momentum, AdamW} x {fp32 state, bf16 state} x {fp32 sum, bf16 sum},
  the bf16 shadow on; one AdamW pair (fp32 sum) with the global-norm clip

Bytes are the ones the update must move, from the shapes: the sum (4 or 2 B,
twice with a clip), p read and written (8 B), m read and written (8 or 4 B),
v read and written for AdamW (8 or 4 B), the shadow written (2 B).  AdamW with
the shadow from an fp32 sum: 30 B per element with fp32 state, 22 B with bf16
state; SGD: 22 and 18.  A pass that ran at the same rate would take 22/30 and
18/22 of the time.

One JSON line per variant: median / min / max microseconds, GB/s at the
median; then one line per fp32 / bf16 pair with the ratio of the medians, the
ratio of the bytes and whether the bf16-state median is below the fp32-state
median by more than the fp32 variant's own min-max spread.
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
STATE_BYTES = {"fp32": 4, "bf16": 2}


def nbytes(n: int, kind: str, state: str, src: str, clip: bool) -> int:
    sb = 4 if src == "fp32" else 2
    moments = 2 if kind == "adamw" else 1
    return n * (sb * (2 if clip else 1) + 8 + 2 * STATE_BYTES[state] * moments + 2)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench/fused_opt_state.py needs a GPU")
    if a.reps < 25:
        raise SystemExit("--reps: at least 25")
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
    sflat = torch.empty(n, device=dev, dtype=torch.bfloat16)
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16}
    m = {k: torch.zeros(n, device=dev, dtype=d) for k, d in dt.items()}
    v = {k: torch.zeros(n, device=dev, dtype=d) for k, d in dt.items()}
    t = torch.zeros(1, device=dev, dtype=torch.int32)
    ws = sqnorm_workspace(dev)
    hyper = {"sgd": dict(momentum=0.9, weight_decay=1e-2), "adamw": dict(weight_decay=0.01)}
    lr = {"sgd": 0.05, "adamw": 1e-3}

    def fused(kind, state, src, clip):
        def run():
            t.add_(1)
            outs[src].optim_step_(kind, pflat, m[state], v[state] if kind == "adamw" else None, t, lr[kind],
                                  shadow=sflat, max_norm=1.0 if clip else None, norm_ws=ws if clip else None,
                                  **hyper[kind])
        return run

    variants, pairs = {}, []
    cases = [(kind, src, False) for kind in ("sgd", "adamw") for src in ("fp32", "bf16")] + [("adamw", "fp32", True)]
    for kind, src, clip in cases:
        tag = f"{kind}_{src}_shadow{'_clip' if clip else ''}"
        for state in ("fp32", "bf16"):
            variants[f"{state}state_{tag}"] = (fused(kind, state, src, clip), nbytes(n, kind, state, src, clip), state)
        pairs.append(tag)
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
    lines, med = [], {}
    for name, (_, b, state) in variants.items():
        med[name] = statistics.median(us[name])
        lines.append(json.dumps({"variant": name, "state": state, "elements": n, "bytes": b, "reps": len(us[name]),
                                 "us_median": round(med[name], 1), "us_min": round(min(us[name]), 1),
                                 "us_max": round(max(us[name]), 1), "gbps_median": round(b / med[name] / 1e3, 1)}))
    for tag in pairs:
        f, h = f"fp32state_{tag}", f"bf16state_{tag}"
        spread = max(us[f]) - min(us[f])
        lines.append(json.dumps({"pair": tag, "time_ratio": round(med[h] / med[f], 4),
                                 "byte_ratio": round(variants[h][1] / variants[f][1], 4),
                                 "fp32state_spread_us": round(spread, 1),
                                 "saved_us": round(med[f] - med[h], 1), "keep": bool(med[f] - med[h] > spread)}))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
