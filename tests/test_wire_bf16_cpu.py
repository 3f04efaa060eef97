"""bf16 wire compression with error feedback, CPU side: the torch expression
of ``ops.pack_bf16`` (the numerics reference of the gfx950 kernel), the
compressed ``GradientBucket``, the fp32 results of ``AllReduceOutput`` from a
bf16 sum, and the DDP hook's wire option."""
import pytest
import torch

from akka_allreduce_amd.data import AllReduceOutput, Geometry
from akka_allreduce_amd.ops import pack_bf16

# e = g (+ 0): +-0, fp32 denormals, large, bf16 max, a finite value that rounds to inf, inf, nan
SPECIAL = [0.0, -0.0, 1e-39, -1e-39, 1e30, -1e30, 3.3895314e38, -3.3895314e38, 3.4e38, -3.4e38,
           float("inf"), float("-inf"), float("nan"), 1.0 + 2.0 ** -10]


def test_pack_matches_the_expression():
    g = torch.randn(1001)
    r = torch.randn(1001) * 1e-3
    e = g + r
    r_new = r.clone()
    q = pack_bf16(g, r_new)
    assert q.dtype == torch.bfloat16 and torch.equal(q, e.bfloat16())
    assert torch.equal(q.float() + r_new, e)  # exact: g + r and e - q are single fp32 operations
    assert torch.equal(r_new, e - q.float())


def test_pack_special_values():
    g = torch.tensor(SPECIAL)
    r = torch.zeros_like(g)
    q = pack_bf16(g, r)
    want = (g + torch.zeros_like(g)).bfloat16()  # e = g + r: -0 + 0 is +0
    assert torch.equal(q.view(torch.int16), want.view(torch.int16))  # bit for bit, nan included
    assert torch.equal(pack_bf16(g).view(torch.int16), g.bfloat16().view(torch.int16))  # no residual: -0 stays
    bad = ~(torch.isfinite(g) & torch.isfinite(want.float()))
    assert bad.tolist() == [False] * 8 + [True] * 5 + [False]  # 3.4e38 is finite and rounds to inf
    assert bool((r[bad] == 0).all())
    ok = ~bad
    assert torch.equal(q.float()[ok] + r[ok], g[ok])
    assert float(r[2]) != 0.0  # a denormal's rounding error is kept, not flushed


def test_pack_without_residual_is_a_cast_and_out_is_filled():
    g = torch.randn(77)
    out = torch.empty(77, dtype=torch.bfloat16)
    assert pack_bf16(g, out=out) is out and torch.equal(out, g.bfloat16())


def test_pack_validates():
    g = torch.randn(8)
    with pytest.raises(TypeError):
        pack_bf16(g.double())
    with pytest.raises(TypeError):
        pack_bf16(g, residual=torch.zeros(8, dtype=torch.bfloat16))
    with pytest.raises(TypeError):
        pack_bf16(g, out=torch.empty(8))
    with pytest.raises(ValueError):
        pack_bf16(g, residual=torch.zeros(9))
    with pytest.raises(ValueError):
        pack_bf16(g, out=torch.empty(4, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        pack_bf16(torch.randn(8, 2).t())


def accumulate(pack, device, steps=64, n=257):
    """sum_t q_t + r_T against sum_t g_t in float64 (constant 1 + 2**-10 in
    element 0, which bf16 rounds to 1): relative error with a residual, and
    the absolute miss of element 0 without one."""
    gen = torch.Generator().manual_seed(3)
    r = torch.zeros(n, device=device)
    sq = {True: torch.zeros(n, dtype=torch.float64), False: torch.zeros(n, dtype=torch.float64)}
    sg = torch.zeros(n, dtype=torch.float64)
    for _ in range(steps):
        g = torch.randn(n, generator=gen) * 1e-3
        g[0] = 1.0 + 2.0 ** -10
        sg += g.double()
        gd = g.to(device)
        sq[True] += pack(gd, r).double().cpu()
        sq[False] += pack(gd).double().cpu()
    with_r = sq[True] + r.double().cpu()
    rel = float(((with_r - sg).abs() / sg.abs().clamp(min=1e-3)).max())
    return rel, float(sg[0] - sq[False][0])


def test_accumulation_with_and_without_residual():
    rel, miss = accumulate(pack_bf16, "cpu")
    assert rel <= 1e-6, rel
    assert abs(miss - 64 * 2.0 ** -10) < 1e-6, miss  # without a residual the 2**-10 is lost every step


# ---- GradientBucket ----------------------------------------------------------------

def _emulate(steps, lr, batches, feedback):
    from akka_allreduce_amd.models.mlp import MLP

    torch.manual_seed(0)
    m = MLP(256, 512, 10)
    ps = list(m.parameters())
    rs = [torch.zeros_like(p) for p in ps]
    for x, y in batches[:steps]:
        for p in ps:
            p.grad = None
        torch.nn.functional.cross_entropy(m(x), y).backward()
        with torch.no_grad():
            for p, r in zip(ps, rs):
                e = p.grad + r if feedback else p.grad
                q = e.bfloat16()
                if feedback:
                    r.copy_(e - q.float())
                # p -= lr * q as torch's SGD spells it (sgd_step): the rounding of the product is the
                # library's, so both runs see the same parameters, hence the same gradients, every step
                p.add_(q.float(), alpha=-lr)
    return [p.detach().clone() for p in ps]


@pytest.mark.parametrize("flatten", [False, True])
@pytest.mark.parametrize("feedback", [True, False])
def test_bucket_matches_torch_emulation(feedback, flatten):
    from akka_allreduce_amd.models.mlp import MLP, dp_sgd_step, synthetic_batch
    from akka_allreduce_amd.parallel import ThresholdAllreduce
    from akka_allreduce_amd.parallel.dp import GradientBucket

    gen = torch.Generator().manual_seed(11)
    batches = [synthetic_batch(64, 256, 10, device="cpu", generator=gen) for _ in range(6)]
    torch.manual_seed(0)
    m = MLP(256, 512, 10)
    b = GradientBucket(list(m.parameters()), flatten_params=flatten, wire_dtype=torch.bfloat16,
                       error_feedback=feedback)
    assert b.wire.dtype == torch.bfloat16 and b.wire.numel() == b.numel
    assert (b.residual is not None) == feedback
    ar = ThresholdAllreduce(b.numel, dtype=torch.bfloat16, device="cpu", rank=0, world_size=1)
    for x, y in batches:
        dp_sgd_step(m, x, y, 0.1, ar, b)
    for got, want in zip(m.parameters(), _emulate(6, 0.1, batches, feedback)):
        torch.testing.assert_close(got.detach(), want, rtol=1e-6, atol=1e-7)
    if feedback:
        assert float(b.residual.abs().max()) > 0
        b.reset_residual()
        assert float(b.residual.abs().max()) == 0


def test_bucket_average_writes_the_fp32_mean():
    from akka_allreduce_amd.parallel import ThresholdAllreduce
    from akka_allreduce_amd.parallel.dp import GradientBucket

    p = torch.nn.Parameter(torch.zeros(300))
    b = GradientBucket([p], wire_dtype=torch.bfloat16)
    g = torch.randn(300)
    b.flat.copy_(g)
    ar = ThresholdAllreduce(b.numel, dtype=torch.bfloat16, device="cpu", rank=0, world_size=1)
    b.average(ar)
    assert torch.equal(b.flat, g.bfloat16().float())
    assert torch.equal(b.residual, g - g.bfloat16().float())


def test_bucket_refuses_wrong_dtypes():
    from akka_allreduce_amd.parallel import ThresholdAllreduce
    from akka_allreduce_amd.parallel.dp import GradientBucket

    with pytest.raises(ValueError):
        GradientBucket([torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16))], wire_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        GradientBucket([torch.nn.Parameter(torch.zeros(8))], wire_dtype=torch.float16)
    b = GradientBucket([torch.nn.Parameter(torch.zeros(8))], wire_dtype=torch.bfloat16)
    ar32 = ThresholdAllreduce(8, device="cpu", rank=0, world_size=1)
    with pytest.raises(RuntimeError, match="dtype=torch.bfloat16"):
        b.sgd_from(lambda w: ar32(w.float()), 0.1)
    with pytest.raises(ValueError):
        b.sgd_from(lambda w, out=None: None, 0.1, out_buf=torch.empty(8))


# ---- AllReduceOutput ---------------------------------------------------------------

def _output(S=1000, N=4, C=64):
    g = Geometry(S, N, C)
    x = torch.randn(S).bfloat16()
    pc = torch.randint(0, N + 1, (N, g.kmax), dtype=torch.int32)
    pc[0, 0] = 0
    pc[1, 0] = 3
    return AllReduceOutput(x, counts_per_chunk=pc, geometry=g), x, g.expand_counts(pc)


def test_output_fp32_mean_from_bf16_sum():
    o, x, c = _output()
    cf = c.float()
    want = torch.where(cf > 0, x.float() / cf.clamp(min=1), torch.zeros(x.numel()))
    got = o.mean(dtype=torch.float32)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    buf = torch.empty(x.numel())
    assert o.mean(out=buf, dtype=torch.float32) is buf and torch.equal(buf, want)
    y0 = torch.randn(x.numel())
    y = y0.clone()
    shadow = torch.empty(x.numel(), dtype=torch.bfloat16)
    assert o.axpy_mean_(y, -0.1, shadow=shadow, wide=True) is y
    assert torch.equal(y, y0.add(want, alpha=-0.1))
    assert torch.equal(shadow, y.bfloat16())
    assert not torch.equal(want, o.mean().float())  # the unrounded mean differs from the bf16 one
    with pytest.raises(ValueError):
        o.mean(dtype=torch.float16)
    with pytest.raises(ValueError):
        o.mean(out=torch.empty(x.numel(), dtype=torch.bfloat16), dtype=torch.float32)


def test_output_without_the_keywords_is_unchanged():
    o, x, c = _output()
    cb = c.to(torch.bfloat16)
    old = torch.where(cb > 0, x / cb.clamp(min=1), torch.zeros_like(x))  # the division in bf16
    got = o.mean()
    assert got.dtype == torch.bfloat16 and torch.equal(got, old)
    assert torch.equal(o.mean(dtype=torch.bfloat16), old)
    y0 = torch.randn(x.numel())
    y = y0.clone()
    o.axpy_mean_(y, -0.1)
    assert torch.equal(y, y0.add(old.float(), alpha=-0.1))
    # wide is about a bf16 sum: an fp32 one keeps its path
    o32 = AllReduceOutput(x.float(), counts_per_chunk=o.counts_per_chunk, geometry=o.geometry)
    y = y0.clone()
    o32.axpy_mean_(y, -0.1, wide=True)
    assert torch.equal(y, y0.add(o32.mean(), alpha=-0.1))


# ---- DDP hook ----------------------------------------------------------------------

class _Bucket:
    """The part of dist.GradBucket the hook reads."""

    def __init__(self, t, index=0):
        self._t, self._i = t, index

    def buffer(self):
        return self._t

    def index(self):
        return self._i


def test_hook_packs_per_bucket_and_returns_the_fp32_mean():
    from akka_allreduce_amd.parallel.ddp import ThresholdHookState, threshold_allreduce_hook

    state = ThresholdHookState(max_chunk_size=64, wire_dtype=torch.bfloat16)
    r_want = {0: torch.zeros(500), 1: torch.zeros(300)}
    for step in range(2):
        for idx, n in ((0, 500), (1, 300)):
            g = torch.randn(n)
            t = g.clone()
            got = threshold_allreduce_hook(state, _Bucket(t, idx)).wait()
            e = g + r_want[idx]
            q = e.bfloat16()
            r_want[idx] = e - q.float()
            assert got.dtype == torch.float32 and torch.equal(got, q.float())  # N=1: the mean is the packed input
            assert torch.equal(t, q.float())  # written into the bucket
    assert sorted(state.wire_bufs) == [0, 1]
    for idx in (0, 1):
        wire, res = state.wire_bufs[idx]
        assert wire.dtype == torch.bfloat16 and torch.equal(res, r_want[idx])
    assert all(k[1] == torch.bfloat16 for k in state.engines)
    # a bucket that is already bf16 ignores the option
    tb = torch.randn(64).bfloat16()
    assert torch.equal(threshold_allreduce_hook(state, _Bucket(tb.clone(), 2)).wait(), tb)
    assert 2 not in state.wire_bufs


def test_hook_without_feedback_and_with_reactive():
    from akka_allreduce_amd.parallel.ddp import ThresholdHookState, threshold_allreduce_hook

    state = ThresholdHookState(wire_dtype=torch.bfloat16, error_feedback=False)
    g = torch.randn(100)
    for _ in range(2):
        assert torch.equal(threshold_allreduce_hook(state, _Bucket(g.clone())).wait(), g.bfloat16().float())
    assert state.wire_bufs[0][1] is None
    with pytest.raises(ValueError):
        ThresholdHookState(transport="reactive", wire_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ThresholdHookState(wire_dtype=torch.float16)
