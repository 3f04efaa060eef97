#!/usr/bin/env python3
"""What does ``skip_nonfinite`` cost the fused optimizer step at the config-5 bucket?

Same bucket and conventions as ``bench/fused_opt_state.py``: 41 755 624
elements (the 4096-8192-1000 MLP), one contributor, fp32 sum, fp32 state, the
bf16 shadow on, every variant one step between device events, all variants
alternating over the repetitions of ONE process (machines differ by more than
any effect here: only ratios within one run count).  Before each timed step an
untimed 512 MiB fill pushes everything out of the 256 MiB Infinity Cache:
without it a variant's time depends on what the variant before it left there
(a skipped step leaves the whole sum; the step after it measured 7 % faster).

  {SGD-momentum, AdamW} x {no clip, clip} x
    off      the unguarded step: t += 1, [norm pass,] update pass
    on       the guarded step over a finite sum: norm pass (verdict, t), update pass
    skipped  the guarded step over a sum with one inf: norm pass, the update
             pass's early exit

Guard on with the clip has the launches of the clip alone less one (no
``t.add_``); guard on without the clip adds the norm pass, one more read of the
sum (4 B per element).  A skipped step is the norm pass and an empty grid.

``--baseline`` runs the ``off`` rows alone and needs nothing of the guard: the
same script, run on a checkout from before the guard in the same job, gives the
parent's pass to hold ``off`` against (the update kernel gained one argument
and one uniform branch).

One JSON line per variant: median / min / max microseconds; then one line per
pair with the ratio of the medians and the base's own min-max spread.
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
    ap.add_argument("--baseline", action="store_true", help="the unguarded rows only (a tree from before the guard)")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench/fused_opt_guard.py needs a GPU")
    if a.reps < 25:
        raise SystemExit("--reps: at least 25")
    from akka_allreduce_amd.data import AllReduceOutput, Geometry, sqnorm_workspace

    dev = torch.device("cuda", 0)
    n = sum(torch.Size(s).numel() for s in SHAPES)
    gen = torch.Generator(device=dev).manual_seed(0)
    good = torch.randn(n, device=dev, generator=gen) * 1e-2
    geo = Geometry(n, 1, 1 << 20)
    pc = torch.ones((1, geo.kmax), device=dev, dtype=torch.int32)
    outs = {"finite": AllReduceOutput(good, counts_per_chunk=pc, geometry=geo)}
    # parameters and state per kind: each kind's rows together are one consistent run of that optimizer
    pflat = {k: torch.randn(n, device=dev, generator=gen) for k in ("sgd", "adamw")}
    sflat = torch.empty(n, device=dev, dtype=torch.bfloat16)
    m = {k: torch.zeros(n, device=dev) for k in ("sgd", "adamw")}
    v = torch.zeros(n, device=dev)
    t = torch.zeros(1, device=dev, dtype=torch.int32)
    ws = sqnorm_workspace(dev)
    guard = None
    if not a.baseline:
        from akka_allreduce_amd.data import guard_state

        guard = guard_state(dev)
        bad = good.clone()
        bad[n // 2] = float("inf")
        outs["inf"] = AllReduceOutput(bad, counts_per_chunk=pc, geometry=geo)
    hyper = {"sgd": dict(momentum=0.9, weight_decay=1e-2), "adamw": dict(weight_decay=0.01)}
    lr = {"sgd": 0.05, "adamw": 1e-3}

    def step(kind, clip, mode):
        kw = dict(shadow=sflat, max_norm=1.0 if clip else None, **hyper[kind])
        pp, mm, vv = pflat[kind], m[kind], v if kind == "adamw" else None
        if mode == "off":
            def run():
                t.add_(1)
                outs["finite"].optim_step_(kind, pp, mm, vv, t, lr[kind], norm_ws=ws if clip else None, **kw)
        else:
            out = outs["finite" if mode == "on" else "inf"]

            def run():
                out.optim_step_(kind, pp, mm, vv, t, lr[kind], norm_ws=ws, guard=guard, **kw)
        return run

    modes = ("off",) if a.baseline else ("off", "on", "skipped")
    variants = {f"{mode}_{kind}{'_clip' if clip else ''}": step(kind, clip, mode)
                for kind in ("sgd", "adamw") for clip in (False, True) for mode in modes}
    flush = torch.empty(1 << 29, device=dev, dtype=torch.uint8)  # twice the Infinity Cache
    us = {k: [] for k in variants}
    for rep in range(a.warmup + a.reps):
        for name, fn in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            flush.zero_()  # every variant starts from the same cache state
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if rep >= a.warmup:
                us[name].append(t0.elapsed_time(t1) * 1e3)
    if guard is not None:
        # every skipped call was counted, every other guarded one applied
        record, calls = guard.tolist(), a.warmup + a.reps
        assert record[1] == 4 * calls and int(t) == 8 * calls, (record, int(t))
        assert all(bool(torch.isfinite(x).all()) for x in pflat.values())
    lines, med = [], {}
    for name in variants:
        med[name] = statistics.median(us[name])
        lines.append(json.dumps({"variant": name, "elements": n, "reps": len(us[name]),
                                 "us_median": round(med[name], 1), "us_min": round(min(us[name]), 1),
                                 "us_max": round(max(us[name]), 1)}))
    if not a.baseline:
        for kind in ("sgd", "adamw"):
            for clip in ("", "_clip"):
                base = f"off_{kind}{clip}"
                spread = max(us[base]) - min(us[base])
                for mode in ("on", "skipped"):
                    name = f"{mode}_{kind}{clip}"
                    lines.append(json.dumps({"pair": f"{name} / {base}", "time_ratio": round(med[name] / med[base], 4),
                                             "extra_us": round(med[name] - med[base], 1),
                                             "base_spread_us": round(spread, 1)}))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
