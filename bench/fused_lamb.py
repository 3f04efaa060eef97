#!/usr/bin/env python3
"""What does a fused LAMB step cost at the config-5 bucket?

Same bucket and conventions as ``bench/fused_opt_state.py``: 41 755 624
elements (the 4096-8192-1000 MLP, four layers), one contributor, an fp32 sum,
the bf16 shadow on, every variant one call between device events, all variants
alternating over the repetitions, medians of 25.

  lamb            the fused step: lamb_norms, lamb_trust, count_optim<LAMB>
  lamb_norms      the norm pass alone      (reads sum, p, m, v: 16 B per element)
  lamb_trust      the ratio kernel alone   (reads the partials: 8 B per tile)
  lamb_update     the update alone         (sum, p rw, m rw, v rw, shadow: 30 B)
  adamw           FusedAdamW's pass, plain (30 B per element)
  adamw_groups    the same through the four segments' rows, as LAMB runs
  torch_lamb      unfused: out.mean(), foreach moments and u, per-parameter
                  norms, the ratios kept on the device, foreach update, shadow copy

One JSON line per variant: median / min / max microseconds and GB/s of the
bytes the variant must move at the median (none for torch_lamb: its traffic is
whatever its temporaries make it); then one line with the ratios of the
medians, each against the comparator of the same run.
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
LR, WD, BETAS, EPS = 1e-3, 0.01, (0.9, 0.999), 1e-6


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench/fused_lamb.py needs a GPU")
    if a.reps < 25:
        raise SystemExit("--reps: at least 25")
    from akka_allreduce_amd._native_loader import load
    from akka_allreduce_amd.data import (DTYPE_NAME, AllReduceOutput, Geometry, OptimGroups, counts_table,
                                         lamb_workspace)

    nat = load()
    dev = torch.device("cuda", 0)
    sizes = [torch.Size(s).numel() for s in SHAPES]
    n = sum(sizes)
    gen = torch.Generator(device=dev).manual_seed(0)
    ssum = torch.randn(n, device=dev, generator=gen) * 1e-2
    geo = Geometry(n, 1, 1 << 20)
    pc = torch.ones((1, geo.kmax), device=dev, dtype=torch.int32)
    out = AllReduceOutput(ssum, counts_per_chunk=pc, geometry=geo)
    pflat = torch.randn(n, device=dev, generator=gen)
    sflat = torch.empty(n, device=dev, dtype=torch.bfloat16)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    t = torch.zeros(1, device=dev, dtype=torch.int32)
    # one segment per layer; the biases without decay and without adaptation
    ends = [sum(sizes[:i + 1]) for i in range(len(sizes))]
    gr = OptimGroups(ends, [0, 1, 0, 1], 2, dev)
    gr.write_rows(OptimGroups.row_values(LR, [(1.0, WD), (1.0, 0.0)]))
    adapt = torch.tensor([1, 0, 1, 0], dtype=torch.int32, device=dev)
    trust = torch.ones(len(ends), device=dev)
    ws = lamb_workspace(n, len(ends), dev)
    tiles = -(-n // nat.lamb_tile())

    def lamb():
        t.add_(1)
        out.optim_step_("lamb", pflat, m, v, t, 0.0, shadow=sflat, groups=gr, betas=BETAS, eps=EPS, lamb_ws=ws,
                        trust=trust, layer_adapt=adapt)

    def adamw(groups):
        def run():
            t.add_(1)
            out.optim_step_("adamw", pflat, m, v, t, 0.0 if groups else LR, shadow=sflat, betas=BETAS, eps=EPS,
                            groups=gr if groups else None, **({} if groups else {"weight_decay": WD}))
        return run

    keep, table = counts_table(pc, geo)
    g_args = (gr.seg_end.data_ptr(), gr.seg_group.data_ptr(), gr.rows.data_ptr(), gr.host_seg_end, gr.host_seg_group,
              gr.ngroups)

    def stream():
        return torch.cuda.current_stream(dev).cuda_stream

    def norms():
        nat.lamb_norms(ws.data_ptr(), ws.numel() // 2, pflat.data_ptr(), m.data_ptr(), v.data_ptr(), ssum.data_ptr(),
                       DTYPE_NAME[ssum.dtype], table, t.data_ptr(), 0, g_args, stream(), beta1=BETAS[0],
                       beta2=BETAS[1], eps=EPS)

    def ratios():
        nat.lamb_trust(trust.data_ptr(), ws.data_ptr(), ws.numel() // 2, g_args, n, adapt.data_ptr(), stream())

    def update():
        nat.count_optim("lamb", pflat.data_ptr(), m.data_ptr(), v.data_ptr(), sflat.data_ptr(), ssum.data_ptr(),
                        DTYPE_NAME[ssum.dtype], table, t.data_ptr(), 0, stream(), False, beta1=BETAS[0],
                        beta2=BETAS[1], eps=EPS, groups=g_args, trust=trust.data_ptr())

    # the unfused LAMB: its own state, so the fused variants' moments are not its inputs
    tp, tm, tv = pflat.clone(), torch.zeros_like(m), torch.zeros_like(v)
    ts = torch.empty_like(sflat)
    tstep = torch.zeros((), device=dev)
    split = lambda x: list(torch.split(x, sizes))  # noqa: E731
    ps, ms, vs = split(tp), split(tm), split(tv)
    wds, on = [WD, 0.0, WD, 0.0], [True, False, True, False]

    def torch_lamb():
        tstep.add_(1)
        gs = split(out.mean())
        torch._foreach_lerp_(ms, gs, 1 - BETAS[0])
        torch._foreach_mul_(vs, BETAS[1])
        torch._foreach_addcmul_(vs, gs, gs, 1 - BETAS[1])
        bc1, sbc2 = 1 - BETAS[0] ** tstep, (1 - BETAS[1] ** tstep).sqrt()
        den = torch._foreach_sqrt(vs)
        us = []
        for d, mi, pi, wd in zip(den, ms, ps, wds):
            d.div_(sbc2).add_(EPS)
            us.append((mi / bc1).div_(d).add_(pi, alpha=wd))
        pn, un = torch._foreach_norm(ps), torch._foreach_norm(us)
        for u, pi, a, b, adaptive in zip(us, ps, pn, un, on):
            r = torch.where((a > 0) & (b > 0), a / b, torch.ones_like(a)) if adaptive else torch.ones_like(a)
            pi.sub_(u.mul_(r * LR))
        ts.copy_(tp)

    variants = {
        "lamb": (lamb, 46 * n + 8 * tiles),
        "lamb_norms": (norms, 16 * n),
        "lamb_trust": (ratios, 8 * tiles),
        "lamb_update": (update, 30 * n),
        "adamw": (adamw(False), 30 * n),
        "adamw_groups": (adamw(True), 30 * n),
        "torch_lamb": (torch_lamb, None),
    }
    us_ = {k: [] for k in variants}
    for rep in range(a.warmup + a.reps):
        for name, (fn, _) in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            if rep >= a.warmup:
                us_[name].append(t0.elapsed_time(t1) * 1e3)
    lines, med = [], {}
    for name, (_, b) in variants.items():
        med[name] = statistics.median(us_[name])
        lines.append(json.dumps({"variant": name, "elements": n, "bytes": b, "reps": len(us_[name]),
                                 "us_median": round(med[name], 1), "us_min": round(min(us_[name]), 1),
                                 "us_max": round(max(us_[name]), 1),
                                 "gbps_median": None if b is None else round(b / med[name] / 1e3, 1)}))
    lines.append(json.dumps({"ratios": {"lamb/adamw": round(med["lamb"] / med["adamw"], 3),
                                        "lamb/adamw_groups": round(med["lamb"] / med["adamw_groups"], 3),
                                        "lamb/torch_lamb": round(med["lamb"] / med["torch_lamb"], 3),
                                        "bytes lamb/adamw": round(46 / 30, 3)},
                             "finite": bool(torch.isfinite(pflat).all() and torch.isfinite(tp).all())}))
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
