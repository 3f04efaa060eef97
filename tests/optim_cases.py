"""What the tests of the fused optimizer pass share (``test_fused_optim_*``,
``test_param_groups_*``, ``test_bf16_state_*``): hyper-parameters, the stub
round and bucket of the CPU files, the inputs, state and step of the GPU files,
the MLP run, and the tests' own copy of the stochastic rounding.

``_mix`` / ``_bits`` / ``_sr`` are that copy: the definition at the top of the
bf16 code in ``csrc/kernels/optim.hip`` in numpy (uint32 arithmetic that
wraps), written from the documentation; nothing of it is imported from the
package."""
import functools
import math

import numpy as np
import pytest
import torch

from akka_allreduce_amd.data import AllReduceOutput, Geometry
from akka_allreduce_amd.parallel.dp import GradientBucket

BF = torch.bfloat16
HYPER = {
    "sgd": dict(lr=0.05, momentum=0.9, nesterov=False, weight_decay=1e-2),
    "nesterov": dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-2),
    "adamw": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01),
}
# what the count-0 elements of the fp32 start state hold (``_inputs``), and those of every shadow
M_SENTINEL, V_SENTINEL, H_SENTINEL = 123.25, 77.5, -3.5


def _dev():
    return torch.device("cuda", 0)


# the rounding definition ---------------------------------------------------------------------------------------------
def _mix(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


@functools.lru_cache(maxsize=16)
def _bits(n, t, seed):
    """(r_m, r_v) of the elements 0 .. n-1 at step t."""
    key = _mix(np.array([seed], np.uint32) ^ _mix(np.array([t], np.uint32)))
    i = np.arange(n, dtype=np.uint64)
    lo, hi = (i & np.uint64(0xFFFFFFFF)).astype(np.uint32), (i >> np.uint64(32)).astype(np.uint32)
    h = _mix(lo ^ (hi * np.uint32(0x9E3779B9)) ^ key)
    return h & np.uint32(0xFFFF), h >> np.uint32(16)


def _sr(x, r):
    """fp32 tensor -> bf16 tensor (on the CPU) with the 16-bit r: the upper half of bits + r where x is finite,
    else the cast."""
    x = x.detach().cpu().contiguous()
    b = x.numpy().view(np.uint32)
    up = ((b.astype(np.uint64) + np.asarray(r).astype(np.uint64)) >> np.uint64(16)).astype(np.uint16)
    cast = x.to(BF).contiguous().view(torch.int16).numpy().view(np.uint16)
    out = np.where((b & np.uint32(0x7F800000)) != np.uint32(0x7F800000), up, cast)
    return torch.from_numpy(out.view(np.int16).copy()).view(BF)


def _same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    it = torch.int16 if a.dtype == BF else torch.int32
    return a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


# the CPU files --------------------------------------------------------------------------------------------------------
class StubAllreduce:
    """A round whose per-chunk counts are given: every contributor of a chunk
    sent this rank's values, so the sum is ``count * t`` and 0 where the
    count is 0."""

    def __init__(self, S, N, C, seed=1):
        self.geometry = Geometry(S, N, C)
        g = torch.Generator().manual_seed(seed)
        pc = torch.randint(0, N + 1, (N, self.geometry.kmax), dtype=torch.int32, generator=g)
        pc[0, 0] = 0      # a missing chunk
        pc[1, 0] = N - 1  # a partial one
        pc[2, 1] = N      # a complete one
        self.counts = pc
        self.count = self.geometry.expand_counts(pc)
        self.last = None

    def __call__(self, t, out=None):
        data = (t.float() * self.count).to(t.dtype)
        self.last = data
        return AllReduceOutput(data, counts_per_chunk=self.counts, geometry=self.geometry)

    def mean(self):
        c = self.count.float()
        return torch.where(c > 0, self.last.float() / c.clamp(min=1), torch.zeros_like(c))


def _bucket(wire=False, sizes=(640, 60, 300, 3)):
    """1003 elements as "weight, bias, weight, bias"."""
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(n)) for n in sizes]
    return GradientBucket(ps, flatten_params=True, wire_dtype=BF if wire else None)


def _close(got, want, what):
    # per step a few fp32 roundings (2**-24) of operands no larger than the largest value
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6 * float(want.abs().max()) + 1e-12,
                               msg=lambda m: f"{what}: {m}")


# the GPU files --------------------------------------------------------------------------------------------------------
NGRAD = 4


@functools.lru_cache(maxsize=2)
def _inputs(S, N, C, src):
    """Counts (random in [0, N], one chunk forced to 0 and one to N), NGRAD
    sums of the source dtype with their fp32 means, and the initial fp32 state
    with sentinels in the count-0 elements."""
    dev = _dev()
    geo = Geometry(S, N, C)
    g = torch.Generator(device="cpu").manual_seed(S * 31 + N)
    pc = torch.randint(0, N + 1, (N, geo.kmax), dtype=torch.int32, generator=g)
    pc[0, 0] = 0
    pc[N - 1, 0] = N
    count = geo.expand_counts(pc).to(dev)
    pc = pc.to(dev)
    missing = count == 0
    sums, means = [], []
    for i in range(NGRAD):
        base = torch.randn(S, generator=g).to(dev)
        if i == 2:
            base = base * 1e-2  # a round whose norm is below max_norm: the clip coefficient clamps to 1
        # count-0 elements keep a non-zero sum: it must not be read
        s = torch.where(missing, base, base * count).to(BF if src == "bf16" else torch.float32)
        sums.append(s)
        out = AllReduceOutput(s, counts_per_chunk=pc, geometry=geo)
        means.append((out.mean(dtype=torch.float32) if src == "bf16" else out.mean()).clone())
    p0 = torch.randn(S, generator=g).to(dev)
    m0 = torch.where(missing, torch.full_like(p0, M_SENTINEL), torch.zeros_like(p0))
    v0 = torch.where(missing, torch.full_like(p0, V_SENTINEL), torch.zeros_like(p0))
    torch.cuda.synchronize()
    return dict(geo=geo, pc=pc, count=count, missing=missing, sums=sums, means=means, p0=p0, m0=m0, v0=v0,
                max_norm=0.1 * math.sqrt(S))


def _kernel_state(inp, shadow=True, dtype=None):
    """[p, m, v, t, shadow] at the start: copies of the inputs' state (m and v as ``dtype`` if given), the step
    at 0 and a shadow of sentinels (or none)."""
    p = inp["p0"].clone()
    m, v = (inp[k].to(dtype or inp[k].dtype, copy=True) for k in ("m0", "v0"))
    t = torch.zeros(1, dtype=torch.int32, device=p.device)
    sh = torch.full_like(p, H_SENTINEL, dtype=BF) if shadow else None
    return [p, m, v, t, sh]


def _step(inp, kind, state, i, ws=None, groups=None, geo=None, pc=None, seed=0):
    """One step from the inputs' sum ``i`` (``geo`` / ``pc``: another geometry and other counts than the
    inputs'); ``ws``: with the clip.  With ``groups`` the learning rate and the decay come from their rows (the
    arguments are unused: 0 is passed)."""
    p, m, v, t, sh = state
    h = dict(HYPER[kind])
    lr = h.pop("lr")
    if groups is not None:
        lr = 0.0
        h.pop("weight_decay")
    out = AllReduceOutput(inp["sums"][i % len(inp["sums"])], counts_per_chunk=inp["pc"] if pc is None else pc,
                          geometry=inp["geo"] if geo is None else geo)
    t.add_(1)
    out.optim_step_("adamw" if kind == "adamw" else "sgd", p, m, v if kind == "adamw" else None, t, lr, shadow=sh,
                    max_norm=inp["max_norm"] if ws is not None else None, norm_ws=ws, groups=groups, seed=seed, **h)


def _mlp_run(graphed, wire, steps=5, lrs=(1e-2,) * 5, bias_decay=None, state_dtype=None, load=None, save_at=None):
    """``steps`` steps of the 64-128-10 MLP at N = 1 with FusedAdamW, eager or as a GraphedDPStep, at the
    learning rates ``lrs``.  ``bias_decay``: the biases in a group of their own with that decay (a device-resident
    learning rate); ``state_dtype``: of m and v.  ``save_at``: also return the state after that many steps;
    ``load``: such a state, loaded after 2 steps (the run then continues from step ``save_at``).  A graphed run
    ends with a step that must refuse a moved state buffer."""
    from akka_allreduce_amd.models.mlp import MLP, GraphedDPStep, dp_sgd_step, synthetic_batch
    from akka_allreduce_amd.parallel import FusedAdamW, ThresholdAllreduce

    dev = _dev()
    gen = torch.Generator(device=dev).manual_seed(5)
    batches = [synthetic_batch(32, 64, 10, device=dev, generator=gen) for _ in range(steps)]
    torch.manual_seed(0)
    model = MLP(64, 128, 10).to(dev)
    bucket = GradientBucket(list(model.parameters()), flatten_params=True, wire_dtype=BF if wire else None)
    kw = {}
    if bias_decay is not None:
        kw["param_groups"] = [{"params": [model.fc1.bias, model.fc2.bias], "weight_decay": bias_decay}]
    if state_dtype is not None:
        kw["state_dtype"] = state_dtype
    opt = FusedAdamW(bucket, weight_decay=0.01, max_grad_norm=1.0, **kw)
    assert opt.m.dtype == opt.v.dtype == (state_dtype or torch.float32)
    if bias_decay is not None:
        assert opt.device_lr and len(opt.param_groups) == 2 and len(opt.groups.host_seg_end) == 4
    ar = ThresholdAllreduce(bucket.numel, max_chunk_size=4096, device=dev, **({"dtype": BF} if wire else {}))
    step = None
    if graphed:
        step = GraphedDPStep(model, bucket, *batches[0], compute_dtype=BF, optimizer=opt)
        assert int(opt.t) == 0  # warmup and capture ran forward + backward only

    def one(i):
        x, y = batches[i]
        if graphed:
            return float(step(x, y, lrs[i], ar))
        return dp_sgd_step(model, x, y, lrs[i], ar, bucket, compute_dtype=BF, optimizer=opt)

    losses, order, extra = [], list(range(steps)), {}
    if load is not None:
        order = [0, 1] + list(range(load["at"], steps))
    for n, i in enumerate(order):
        if load is not None and n == 2:
            ptrs = step._pointers() if graphed else None
            with torch.no_grad():
                bucket.pflat.copy_(load["pflat"])
            bucket.invalidate_shadow()
            opt.load_state_dict(load["opt"])
            if graphed:
                assert step._pointers() == ptrs
            assert int(opt.t) == load["at"]
        losses.append(one(i))
        if n == 0:
            extra["after1"] = bucket.pflat.clone()
        if save_at is not None and n + 1 == save_at:
            extra["saved"] = {"at": save_at, "pflat": bucket.pflat.clone(), "opt": opt.state_dict()}
    if graphed:
        keep = opt.m
        opt.m = torch.zeros_like(keep)
        with pytest.raises(RuntimeError, match="moved"):
            step(*batches[0], 1e-2, ar)
        opt.m = keep
    torch.cuda.synchronize()
    assert int(opt.t) == steps and bucket._shadow_on
    if bias_decay is not None:
        assert opt.lr == lrs[order[-1]]
    spans = dict(zip(("w1", "b1", "w2", "b2"), bucket.spans()))
    return dict(losses=losses, pflat=bucket.pflat.clone(), sflat=bucket.sflat.clone(), m=opt.m.clone(),
                v=opt.v.clone(), t=int(opt.t), spans=spans, **extra)
