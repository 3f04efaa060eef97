#!/usr/bin/env python3
"""Does the grouped optimizer pass (parameter groups, learning rate and weight
decay read from device memory) cost anything over the plain one?

At the config-5 bucket (41 755 624 elements: the four tensors of the
4096-8192-1000 MLP), one contributor, weights decayed and biases not -- 4
segments in 2 groups -- against the same update with one weight decay for the
whole buffer as launch arguments (``count_optim``, unchanged).  AdamW and
SGD-momentum, from an fp32 and from a bf16 sum, each writing the bf16 shadow.
Both passes move the same bytes (the tables are a few hundred bytes), so the
expectation is a ratio of 1.0.

Every variant is one call between device events; the legacy and the grouped
pass of a variant alternate inside every repetition.  One JSON line per pass:
median / min / max microseconds over the repetitions and GB/s at the median
(bytes as in bench/fused_opt.py: the sum, p and m read and written, v for
AdamW, the shadow written); then one line per variant with grouped / legacy at
the medians and the legacy pass's own min-max spread over its repetitions,
which is what the ratio is read against.
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
        raise SystemExit("bench/fused_opt_groups.py needs a GPU")
    if a.reps < 20:
        raise SystemExit("--reps: at least 20")
    from akka_allreduce_amd.data import AllReduceOutput, Geometry, OptimGroups

    dev = torch.device("cuda", 0)
    sizes = [torch.Size(s).numel() for s in SHAPES]
    n = sum(sizes)
    gen = torch.Generator(device=dev).manual_seed(0)
    sums = {"fp32": torch.randn(n, device=dev, generator=gen) * 1e-2}
    sums["bf16"] = sums["fp32"].bfloat16()
    geo = Geometry(n, 1, 1 << 20)
    pc = torch.ones((1, geo.kmax), device=dev, dtype=torch.int32)
    outs = {k: AllReduceOutput(s, counts_per_chunk=pc, geometry=geo) for k, s in sums.items()}
    pflat = torch.randn(n, device=dev, generator=gen)
    sflat = torch.empty(n, device=dev, dtype=torch.bfloat16)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    t = torch.zeros(1, device=dev, dtype=torch.int32)
    hyper = {"sgd": dict(momentum=0.9), "adamw": dict()}
    wd = {"sgd": 1e-2, "adamw": 0.01}
    lr = {"sgd": 0.05, "adamw": 1e-3}
    ends, off = [], 0
    for k in sizes:
        off += k
        ends.append(off)
    groups = {}
    for kind in ("sgd", "adamw"):
        g = OptimGroups(ends, [0, 1, 0, 1], 2, dev)  # weights, biases
        g.write_rows(OptimGroups.row_values(lr[kind], [(1.0, wd[kind]), (1.0, 0.0)]))
        groups[kind] = g

    def nbytes(kind, src):
        return n * ((4 if src == "fp32" else 2) + 16 + (8 if kind == "adamw" else 0) + 2)

    def run(kind, src, grouped):
        def f():
            t.add_(1)
            outs[src].optim_step_(kind, pflat, m, v if kind == "adamw" else None, t, lr[kind], shadow=sflat,
                                  weight_decay=wd[kind], groups=groups[kind] if grouped else None, **hyper[kind])
        return f

    variants = {}
    for kind in ("adamw", "sgd"):
        for src in ("fp32", "bf16"):
            for impl in ("legacy", "grouped"):
                variants[f"{impl}_{kind}_{src}_shadow"] = (run(kind, src, impl == "grouped"), nbytes(kind, src), impl)
    us = {k: [] for k in variants}
    for rep in range(a.warmup + a.reps):
        for name, (fn, _, _) in variants.items():  # legacy, grouped, legacy, grouped, ... inside every repetition
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
        lines.append(json.dumps({"variant": name, "impl": impl, "elements": n, "segments": len(ends), "groups": 2,
                                 "bytes": b, "reps": len(us[name]), "us_median": round(med, 1),
                                 "us_min": round(min(us[name]), 1), "us_max": round(max(us[name]), 1),
                                 "gbps_median": round(b / med / 1e3, 1)}))
    for name in variants:
        if not name.startswith("legacy_"):
            continue
        tag = name[len("legacy_"):]
        leg, grp = us[name], us["grouped_" + tag]
        lm, gm = statistics.median(leg), statistics.median(grp)
        spread = (max(leg) - min(leg)) / lm
        lines.append(json.dumps({"variant": tag, "grouped_over_legacy": round(gm / lm, 4),
                                 "legacy_spread": round(spread, 4),
                                 "grouped_spread": round((max(grp) - min(grp)) / gm, 4),
                                 "within_legacy_spread": bool(gm <= lm * (1 + spread))}))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
