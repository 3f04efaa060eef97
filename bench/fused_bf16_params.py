#!/usr/bin/env python3
"""What do bf16 parameters save the fused optimizer pass at the config-5 bucket?

Same bucket and conventions as ``bench/fused_opt_state.py``: 41 755 624
elements (the 4096-8192-1000 MLP), one contributor, a bf16 sum, every variant
one call between device events, all variants alternating over the repetitions.
Before each timed call a 512 MiB buffer is overwritten, so nothing of the
call's streams is left in the 256 MiB Infinity Cache by the call before it.

  {SGD-momentum, AdamW} x {fp32 p + bf16 shadow, bf16 p}, bf16 moments in both;
  one AdamW pair with the global-norm clip

Bytes are the ones the update must move, from the shapes: the sum (2 B, twice
with a clip), p read and written (8 or 4 B), m read and written (4 B), v read
and written for AdamW (4 B), the shadow written (2 B, fp32 p only).  AdamW: 20 B
per element with fp32 p, 14 B with bf16 p; SGD: 16 and 10.  A pass that ran at
the same rate would take 14/20 and 10/16 of the time.

One JSON line per variant: median / min / max microseconds, GB/s at the
median; then one line per pair with the ratio of the medians (bf16 p over
fp32 p, the same run's own baseline), the ratio of the bytes and whether the
bf16-p median is below the fp32-p median by more than the fp32-p variant's own
min-max spread.  ``--md`` also writes the table as markdown.
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
FLUSH_BYTES = 512 << 20


def nbytes(n: int, kind: str, param: str, clip: bool) -> int:
    moments = 2 if kind == "adamw" else 1
    p = 8 + 2 if param == "fp32" else 4  # fp32 p with its shadow, or bf16 p alone
    return n * (2 * (2 if clip else 1) + p + 4 * moments)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--md", default=None, help="also write the table as markdown to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench/fused_bf16_params.py needs a GPU")
    if a.reps < 25:
        raise SystemExit("--reps: at least 25")
    from akka_allreduce_amd.data import AllReduceOutput, Geometry, sqnorm_workspace

    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    n = sum(torch.Size(s).numel() for s in SHAPES)
    gen = torch.Generator(device=dev).manual_seed(0)
    src = (torch.randn(n, device=dev, generator=gen) * 1e-2).to(bf)
    geo = Geometry(n, 1, 1 << 20)
    pc = torch.ones((1, geo.kmax), device=dev, dtype=torch.int32)
    out = AllReduceOutput(src, counts_per_chunk=pc, geometry=geo)
    p32 = torch.randn(n, device=dev, generator=gen)
    p = {"fp32": p32, "bf16": p32.to(bf)}
    sflat = torch.empty(n, device=dev, dtype=bf)
    # each parameter dtype its own moments: the two runs stay two independent optimizers
    m = {k: torch.zeros(n, device=dev, dtype=bf) for k in p}
    v = {k: torch.zeros(n, device=dev, dtype=bf) for k in p}
    t = torch.zeros(1, device=dev, dtype=torch.int32)
    ws = sqnorm_workspace(dev)
    flush = torch.empty(FLUSH_BYTES, device=dev, dtype=torch.uint8)
    hyper = {"sgd": dict(momentum=0.9, weight_decay=1e-2), "adamw": dict(weight_decay=0.01)}
    lr = {"sgd": 0.05, "adamw": 1e-3}

    def fused(kind, param, clip):
        def run():
            t.add_(1)
            out.optim_step_(kind, p[param], m[param], v[param] if kind == "adamw" else None, t, lr[kind],
                            shadow=sflat if param == "fp32" else None, max_norm=1.0 if clip else None,
                            norm_ws=ws if clip else None, **hyper[kind])
        return run

    variants, pairs = {}, []
    for kind, clip in (("sgd", False), ("adamw", False), ("adamw", True)):
        tag = f"{kind}_bf16sum{'_clip' if clip else ''}"
        for param in ("fp32", "bf16"):
            variants[f"{param}p_{tag}"] = (fused(kind, param, clip), nbytes(n, kind, param, clip), param)
        pairs.append(tag)
    us = {k: [] for k in variants}
    for rep in range(a.warmup + a.reps):
        for name, (fn, _, _) in variants.items():
            flush.fill_(rep & 0xFF)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if rep >= a.warmup:
                us[name].append(t0.elapsed_time(t1) * 1e3)
    lines, med, rows = [], {}, []
    for name, (_, b, param) in variants.items():
        med[name] = statistics.median(us[name])
        lines.append(json.dumps({"variant": name, "param": param, "elements": n, "bytes": b, "reps": len(us[name]),
                                 "us_median": round(med[name], 1), "us_min": round(min(us[name]), 1),
                                 "us_max": round(max(us[name]), 1), "gbps_median": round(b / med[name] / 1e3, 1)}))
    for tag in pairs:
        f, h = f"fp32p_{tag}", f"bf16p_{tag}"
        spread = max(us[f]) - min(us[f])
        row = {"pair": tag, "fp32p_us": round(med[f], 1), "bf16p_us": round(med[h], 1),
               "time_ratio": round(med[h] / med[f], 4), "byte_ratio": round(variants[h][1] / variants[f][1], 4),
               "fp32p_spread_us": round(spread, 1), "saved_us": round(med[f] - med[h], 1),
               "keep": bool(med[f] - med[h] > spread)}
        rows.append((row, variants[f][1] // n, variants[h][1] // n, variants[f][1] / med[f] / 1e6,
                     variants[h][1] / med[h] / 1e6))
        lines.append(json.dumps(row))
    print("\n".join(lines))
    for path, text in ((a.out, "\n".join(lines) + "\n"), (a.md, markdown(rows, a.reps))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


def markdown(rows, reps: int) -> str:
    out = [f"| Pair (medians of {reps}) | fp32 `p` + shadow, us | bf16 `p`, us | time ratio | B / element | byte ratio "
           "| TB/s fp32 `p` | TB/s bf16 `p` |", "|---|---|---|---|---|---|---|---|"]
    for r, bf, bh, tf, th in rows:
        out.append(f"| {r['pair']} | {r['fp32p_us']} | {r['bf16p_us']} | {r['time_ratio']:.3f} | {bf} -> {bh} | "
                   f"{r['byte_ratio']:.3f} | {tf:.2f} | {th:.2f} |")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    main()
