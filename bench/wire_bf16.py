#!/usr/bin/env python3
"""Do the two ends of the compressed gradient wire stream at the rate of the
passes they sit next to?

At 128 Mi elements (every stream well past the 256 MiB Infinity Cache), one
launch each, device events, alternating over the repetitions:

  pack_res      ops.pack_bf16 with a residual      read g, r; write r, q   14 B/element
  pack_cast     ops.pack_bf16 without              read g; write q          6 B/element
  update_mixed  bf16 sum -> fp32 AXPY + bf16 shadow                        12 B/element
  update_fp32   the fp32 AXPY + shadow count_mean (comparator)             14 B/element
  copy_fp32     chunk_reduce of one fp32 source (comparator)                8 B/element

One JSON line per pass: bytes from the shapes, median / min / max ms, GB/s at
the median.  GPU only: without a device this fails.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=128 << 20)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench/wire_bf16.py needs a GPU")
    if a.reps < 20:
        raise SystemExit("--reps: at least 20")
    from akka_allreduce_amd.data import AllReduceOutput, Geometry
    from akka_allreduce_amd.ops import chunk_reduce, pack_bf16

    dev = torch.device("cuda", 0)
    n = a.elements
    g = torch.randn(n, device=dev)
    r = torch.zeros(n, device=dev)
    q = torch.empty(n, device=dev, dtype=torch.bfloat16)
    y = torch.randn(n, device=dev)
    shadow = torch.empty(n, device=dev, dtype=torch.bfloat16)
    x32 = g * 1e-3
    x16 = x32.bfloat16()
    dst = torch.empty(n, device=dev)
    geo = Geometry(n, 1, 1 << 20)
    pc = torch.ones((1, geo.kmax), device=dev, dtype=torch.int32)
    o16 = AllReduceOutput(x16, counts_per_chunk=pc, geometry=geo)
    o32 = AllReduceOutput(x32, counts_per_chunk=pc, geometry=geo)
    f32, b16 = 4, 2
    passes = {
        "pack_res": (lambda: pack_bf16(g, r, out=q), n * (2 * f32 + f32 + b16)),
        "pack_cast": (lambda: pack_bf16(g, out=q), n * (f32 + b16)),
        "update_mixed": (lambda: o16.axpy_mean_(y, -1e-3, shadow=shadow, wide=True), n * (b16 + 2 * f32 + b16)),
        "update_fp32": (lambda: o32.axpy_mean_(y, -1e-3, shadow=shadow), n * (f32 + 2 * f32 + b16)),
        "copy_fp32": (lambda: chunk_reduce([g], out=dst), n * 2 * f32),
    }
    ms = {k: [] for k in passes}
    for rep in range(a.warmup + a.reps):
        for name, (fn, _) in passes.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if rep >= a.warmup:
                ms[name].append(t0.elapsed_time(t1))
    lines = []
    for name, (_, nbytes) in passes.items():
        med = statistics.median(ms[name])
        lines.append(json.dumps({"pass": name, "elements": n, "bytes": nbytes, "reps": len(ms[name]),
                                 "ms_median": round(med, 4), "ms_min": round(min(ms[name]), 4),
                                 "ms_max": round(max(ms[name]), 4), "gbps_median": round(nbytes / med / 1e6, 1),
                                 "gbps_min": round(nbytes / max(ms[name]) / 1e6, 1),
                                 "gbps_max": round(nbytes / min(ms[name]) / 1e6, 1)}))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
