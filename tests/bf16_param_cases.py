"""What the tests of bf16 parameters in the fused optimizers share
(``test_bf16_params_*``): the tests' own copy of the second hash, inputs with a
bf16 start state, and one step of any kind on either device.

``_bits_p`` is numpy code written from the README's definition ("bf16
parameters"): ``h2(i) = mix(h(i) ^ 0x85ebca6b)``, ``p`` takes ``h2 & 0xffff``.
``h`` is put back together from ``optim_cases._bits``, the tests' copy of the
first hash (``m`` takes its low half, ``v`` its high half); nothing of it is
imported from the package.

The reference of one step is the pass that existed before bf16 parameters did:
fp32 ``p``, bf16 ``m`` / ``v``, run from the widened ``p`` with the same state,
step and seed.  ``p`` must be ``_sr(p_ref, r_p)`` and ``m``, ``v`` and LAMB's
trust ratios the reference's own bits."""
import functools
import math

import numpy as np
import torch

from akka_allreduce_amd.data import (AllReduceOutput, Geometry, OptimGroups, guard_state, lamb_workspace,
                                     sqnorm_workspace)
from optim_cases import BF, HYPER, _bits, _mix, _same_bits, _sr

KINDS = {**HYPER, "lamb": dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)}
P_SENTINEL, M_SENTINEL, V_SENTINEL = -3.5, 123.0, 77.5  # bf16-representable
SEED = 5
# 4 segments in 2 groups, no boundary a multiple of 8 (one segment where the buffer is a single element)
SEGMENTS = {1: ([1], [0]), 7: ([1, 3, 6, 7], [0, 1, 0, 1]), 1003: ([5, 130, 771, 1003], [0, 1, 0, 1]),
            300_001: ([5, 130_003, 200_001, 300_001], [0, 1, 0, 1])}


def _bits_p(n, t, seed):
    """r_p of the elements 0 .. n-1 at step t."""
    r_m, r_v = _bits(n, t, seed)
    h = r_m | (r_v << np.uint32(16))
    return _mix(h ^ np.uint32(0x85EBCA6B)) & np.uint32(0xFFFF)


@functools.lru_cache(maxsize=4)
def make_inputs(S, N, C, src, dev):
    """Counts (random in [0, N], one chunk 0 where there is more than one, one N), three sums and a bf16 start
    state that is not zero, with sentinels in the count-0 elements of p, m and v."""
    dev = torch.device(dev)
    geo = Geometry(S, N, C)
    g = torch.Generator().manual_seed(S * 31 + N)
    pc = torch.randint(0, N + 1, (N, geo.kmax), dtype=torch.int32, generator=g)
    if N > 1:
        pc[0, 0] = 0
    pc[N - 1, 0] = N
    count = geo.expand_counts(pc)
    missing = count == 0
    sums = []
    for _ in range(3):
        base = torch.randn(S, generator=g)
        sums.append(torch.where(missing, base, base * count).to(BF if src == "bf16" else torch.float32).to(dev))
    p0 = torch.where(missing, torch.full((S,), P_SENTINEL), torch.randn(S, generator=g)).to(BF)
    m0 = torch.where(missing, torch.full((S,), M_SENTINEL), 0.1 * torch.randn(S, generator=g)).to(BF)
    v0 = torch.where(missing, torch.full((S,), V_SENTINEL), 0.01 * torch.rand(S, generator=g)).to(BF)
    return dict(S=S, geo=geo, pc=pc.to(dev), missing=missing, sums=sums, p0=p0.to(dev), m0=m0.to(dev),
                v0=v0.to(dev), max_norm=0.1 * math.sqrt(S), dev=dev)


def start_state(inp):
    """[p, m, v, t]: bf16 copies of the inputs' state and the step at 0."""
    return [inp["p0"].clone(), inp["m0"].clone(), inp["v0"].clone(),
            torch.zeros(1, dtype=torch.int32, device=inp["dev"])]


class Opts:
    """One variant: the kind's hyper-parameters, with ``grouped`` the 4 segments in 2 groups of ``SEGMENTS``
    (group 1 at ``group1 = (lr_scale, weight_decay)``); LAMB always has segments, one alone when not grouped.
    ``clip`` / ``guard``: the norm pass's two uses."""

    def __init__(self, kind, inp, grouped=False, clip=False, guard=False, seed=SEED, group1=(0.5, 0.1)):
        h = dict(KINDS[kind])
        self.lr = h.pop("lr")
        self.kind = "sgd" if kind == "nesterov" else kind
        self.adam = self.kind in ("adamw", "lamb")
        self.clip, self.guard, self.seed, self.inp = clip, guard, seed, inp
        self.groups = None
        if grouped or self.kind == "lamb":
            S, dev = inp["S"], inp["dev"]
            ends, owner = SEGMENTS[S] if grouped else ([S], [0])
            self.groups = OptimGroups(ends, owner, 2, dev)
            self.groups.write_rows(OptimGroups.row_values(self.lr, [(1.0, h["weight_decay"]), group1]))
            self.lr = 0.0  # from the rows
        self.hyper = h

    def buffers(self):
        """What one run owns beside its state: the norm workspace, the guard's record and LAMB's tables."""
        dev = self.inp["dev"]
        b = dict(norm_ws=sqnorm_workspace(dev) if (self.clip or self.guard) else None,
                 guard=guard_state(dev) if self.guard else None, lamb={})
        if self.kind == "lamb":
            nseg = len(self.groups.host_seg_end)
            b["lamb"] = dict(trust=torch.full((nseg,), -7.0, device=dev),
                             layer_adapt=torch.ones(nseg, dtype=torch.int32, device=dev),
                             lamb_ws=lamb_workspace(self.inp["S"], nseg, dev))
        return b

    def step(self, bufs, state, i, src=None):
        """One step from the inputs' sum ``i`` (``src``: another sum).  With a guard the pass advances the step."""
        p, m, v, t = state
        inp = self.inp
        out = AllReduceOutput(inp["sums"][i % 3] if src is None else src, counts_per_chunk=inp["pc"],
                              geometry=inp["geo"])
        if bufs["guard"] is None:
            t.add_(1)
        out.optim_step_(self.kind, p, m, v if self.adam else None, t, self.lr, groups=self.groups, seed=self.seed,
                        max_norm=inp["max_norm"] if self.clip else None, norm_ws=bufs["norm_ws"],
                        guard=bufs["guard"], **bufs["lamb"], **self.hyper)


def _sync(inp):
    if inp["dev"].type == "cuda":
        torch.cuda.synchronize()


def check_steps(o, steps=3):
    """``steps`` steps on the evolving bf16 state, each against the fp32-``p`` pass from the widened ``p``.
    Returns the final state and the run's buffers."""
    inp = o.inp
    S, missing = inp["S"], inp["missing"]
    live = ~missing
    st = start_state(inp)
    p, m, v, t = st
    ours, theirs = o.buffers(), o.buffers()
    for i in range(steps):
        ref = [p.float(), m.clone(), v.clone(), t.clone()]
        o.step(theirs, ref, i)
        o.step(ours, st, i)
        _sync(inp)
        assert p.dtype == BF and ref[0].dtype == torch.float32
        assert int(t) == i + 1 and int(ref[3]) == i + 1
        r_p = _bits_p(S, i + 1, o.seed)
        got, want = p.cpu(), _sr(ref[0], r_p)
        assert _same_bits(got[live], want[live]), f"p at step {i + 1}"
        assert _same_bits(m, ref[1]), f"m at step {i + 1}"
        assert _same_bits(v, ref[2]), f"v at step {i + 1}"
        if o.kind == "lamb":
            assert _same_bits(ours["lamb"]["trust"], theirs["lamb"]["trust"]), f"trust at step {i + 1}"
        if o.guard:
            assert ours["guard"].tolist() == [1, 0, 0, 0]
        # count-0 regions: the sentinels, in p, m and v
        assert bool((got[missing].float() == P_SENTINEL).all())
        assert bool((m.cpu()[missing].float() == M_SENTINEL).all())
        assert bool((v.cpu()[missing].float() == V_SENTINEL).all())
    if bool(live.any()):
        assert not _same_bits(m.cpu()[live], inp["m0"].cpu()[live])
    if S >= 1003:
        # AdamW's step of 1e-3 is a small part of an ulp: a few elements may all stay, a thousand do not
        assert not _same_bits(p.cpu()[live], inp["p0"].cpu()[live])
    return st, ours


def stall_run(dev, S=4096, steps=1000, lr=1e-4, seed=0):
    """p0 = 1, a gradient of 1, plain SGD (momentum 0, no decay) at ``lr`` for ``steps`` steps on bf16 p."""
    dev = torch.device(dev)
    out = AllReduceOutput(torch.ones(S, device=dev), counts_per_chunk=torch.ones((1, 1), dtype=torch.int32, device=dev),
                          geometry=Geometry(S, 1, S))
    p, m = torch.ones(S, dtype=BF, device=dev), torch.zeros(S, dtype=BF, device=dev)
    t = torch.zeros(1, dtype=torch.int32, device=dev)
    for _ in range(steps):
        t.add_(1)
        out.optim_step_("sgd", p, m, None, t, lr, momentum=0.0, weight_decay=0.0, seed=seed)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return p.cpu()


def check_stall(p):
    """The bounds of the 1000-step run (the CPU test's docstring derives them); returns the mean."""
    f = p.double()
    mean = float(f.mean())
    print(f"STALL mean={mean:.9f} min={float(f.min()):.6f} max={float(f.max()):.6f}")
    assert abs(mean - 0.9) <= 2e-3, mean
    assert bool(((f - 0.9).abs() <= 0.15).all()), (float(f.min()), float(f.max()))
    return mean
