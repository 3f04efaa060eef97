"""bf16 wire compression on the GPU: the gfx950 pack kernel bit for bit
against the torch expression (ops.pack_bf16 on CPU tensors), the mixed
count-mean (bf16 sum -> fp32) against the fp32 kernel fed the same values,
the compressed GradientBucket / GraphedDPStep at N=1, and two processes on
the ipc data plane."""
import functools
import os
import socket
import subprocess
import sys
import tempfile

import pytest
import torch

from akka_allreduce_amd.data import AllReduceOutput, Geometry
from akka_allreduce_amd.ops import pack_bf16

from test_wire_bf16_cpu import SPECIAL, accumulate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 24


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Same bits (-0 is not +0), any NaN equal to any NaN."""
    a, b = a.cpu(), b.cpu()
    nan = torch.isnan(a)
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return torch.equal(nan, torch.isnan(b)) and torch.equal(a.view(it)[~nan], b.view(it)[~nan])


def _check_pack(g_cpu, r_cpu, offs):
    """Pack views at element offsets ``offs`` = (g, r, q) of padded device
    buffers; everything, the padding included, must equal the CPU expression."""
    n = g_cpu.numel()
    og, orr, oq = offs
    gb = torch.full((n + PAD,), 7.0, device="cuda")
    rb = torch.full((n + PAD,), 9.0, device="cuda")
    qb = torch.full((n + PAD,), 5.0, device="cuda", dtype=torch.bfloat16)
    gb[og:og + n] = g_cpu.cuda()
    res = None
    if r_cpu is not None:
        rb[orr:orr + n] = r_cpu.cuda()
        res = rb[orr:orr + n]
    out = pack_bf16(gb[og:og + n], res, out=qb[oq:oq + n])
    torch.cuda.synchronize()
    r_want = None if r_cpu is None else r_cpu.clone()
    q_want = pack_bf16(g_cpu, r_want)
    assert out.data_ptr() == qb[oq:oq + n].data_ptr()
    assert _bits_equal(out, q_want), offs
    assert bool((qb[:oq] == 5.0).all()) and bool((qb[oq + n:] == 5.0).all()), offs  # nothing outside the view
    assert bool((gb[:og] == 7.0).all()) and torch.equal(gb[og:og + n].cpu().view(torch.int32), g_cpu.view(torch.int32))
    if r_cpu is not None:
        assert _bits_equal(res, r_want), offs
        assert bool((rb[:orr] == 9.0).all()) and bool((rb[orr + n:] == 9.0).all()), offs
        e = g_cpu + r_cpu
        fin = torch.isfinite(e) & torch.isfinite(q_want.float())
        assert torch.equal(out.cpu().float()[fin] + res.cpu()[fin], e[fin])  # float(q) + r_new == e, exactly
        assert bool((res.cpu()[~fin] == 0).all())
    else:
        assert bool((rb == 9.0).all())


# every stream at the same offset: the vector body behind a head of (8 - off) % 8 elements; (1, 0, 0) and
# (0, 3, 0) share no aligned element and (0, 0, 1) puts q on an odd element: the scalar path
OFFSETS = [(0, 0, 0), (1, 1, 1), (3, 3, 3), (8, 8, 8), (1, 0, 0), (0, 3, 0), (0, 0, 1), (4, 4, 8)]


@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("n", [1, 7, 8, 1023, 4096 + 3, 1 << 18])
def test_pack_kernel_bitwise(n, residual):
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen)
    r = torch.randn(n, generator=gen) * 2.0 ** -9 if residual else None
    for offs in OFFSETS:
        _check_pack(g, r, offs)


@pytest.mark.parametrize("residual", [True, False])
def test_pack_kernel_special_values(residual):
    # in the scalar head and tail, and (repeated) in the vector body
    for reps, offs in ((1, (0, 0, 0)), (40, (0, 0, 0)), (40, (3, 3, 3)), (40, (1, 0, 0))):
        g = torch.tensor(SPECIAL * reps)
        r = torch.zeros_like(g) if residual else None
        _check_pack(g, r, offs)
    if residual:
        # a residual that pushes a finite gradient over bf16's range, and a poisoned one
        g = torch.tensor([3.3895314e38, 1.0, 1.0, -3.3895314e38] * 16)
        r = torch.tensor([1e36, float("inf"), float("nan"), -1e36] * 16)
        _check_pack(g, r, (0, 0, 0))


def test_pack_kernel_accumulates_and_repeats():
    rel, miss = accumulate(pack_bf16, "cuda")
    assert rel <= 1e-6, rel
    assert abs(miss - 64 * 2.0 ** -10) < 1e-6, miss
    g = torch.randn(100_003, device="cuda")
    r0 = torch.randn(100_003, device="cuda") * 1e-3
    ra, rb = r0.clone(), r0.clone()
    qa, qb = pack_bf16(g, ra), pack_bf16(g, rb)
    assert torch.equal(qa, qb) and torch.equal(ra, rb) and not torch.equal(ra, r0)  # in place, and repeatable


def test_pack_validates_on_the_gpu():
    g = torch.randn(16, device="cuda")
    with pytest.raises(ValueError):
        pack_bf16(g, residual=torch.zeros(16))  # another device
    with pytest.raises(ValueError):
        pack_bf16(g, out=torch.empty(32, dtype=torch.bfloat16, device="cuda")[::2])
    with pytest.raises(TypeError):
        pack_bf16(g.bfloat16())


# ---- mixed count-mean ---------------------------------------------------------------

@pytest.mark.parametrize("S,N,C", [(1000, 4, 64), (100_003, 3, 777), (5, 4, 1), (77, 2, 100), (1 << 20, 8, 1 << 14)])
def test_mixed_count_mean(S, N, C):
    geo = Geometry(S, N, C)
    gen = torch.Generator(device="cuda").manual_seed(S + N)
    x = torch.randn(S, device="cuda", generator=gen).bfloat16()
    pc = torch.randint(0, N + 1, (N, geo.kmax), device="cuda", dtype=torch.int32, generator=gen)
    pc[0, 0], pc[-1, -1] = 0, N  # a region nobody reached, and one everybody did
    c = geo.expand_counts(pc.cpu()).cuda().float()
    want = torch.where(c > 0, x.float() / c.clamp(min=1), torch.zeros_like(c))
    o = AllReduceOutput(x, counts_per_chunk=pc, geometry=geo)
    got = o.mean(dtype=torch.float32)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    buf = torch.empty(S, device="cuda")
    assert o.mean(out=buf, dtype=torch.float32) is buf and torch.equal(buf, want)
    assert torch.equal(o.mean(), AllReduceOutput(x, counts_per_chunk=pc, geometry=geo).mean())  # bf16 mean as before

    # the update: against the fp32 kernel (the existing code path) fed the same values
    o32 = AllReduceOutput(x.float(), counts_per_chunk=pc, geometry=geo)
    y0 = torch.randn(S, device="cuda", generator=gen)
    for with_shadow in (False, True):
        ya, yb = y0.clone(), y0.clone()
        sa = torch.zeros(S, device="cuda", dtype=torch.bfloat16) if with_shadow else None
        sb = torch.zeros(S, device="cuda", dtype=torch.bfloat16) if with_shadow else None
        o.axpy_mean_(ya, -0.1, shadow=sa, wide=True)
        o32.axpy_mean_(yb, -0.1, shadow=sb)
        assert torch.equal(ya, yb) and not torch.equal(ya, y0)
        if with_shadow:
            assert torch.equal(sa, ya.to(torch.bfloat16)) and torch.equal(sa, sb)

    # a destination off 16 B leaves the fused pass: same mean; the update is then torch's
    # y + alpha * m, which may round the product first: within one rounding of each term
    pad = torch.empty(S + 4, device="cuda")
    assert torch.equal(o.mean(out=pad[1:1 + S], dtype=torch.float32), want)
    ym = pad[1:1 + S]
    ym.copy_(y0)
    sm = torch.zeros(S, device="cuda", dtype=torch.bfloat16)
    o.axpy_mean_(ym, -0.1, shadow=sm, wide=True)
    bound = 2.0 ** -23 * (ya.abs() + (0.1 * want).abs())
    assert bool(((ym - ya).abs() <= bound).all())
    assert torch.equal(sm, ym.to(torch.bfloat16))


# ---- the compressed bucket at N=1 -----------------------------------------------------

def _batches(dev):
    from akka_allreduce_amd.models.mlp import synthetic_batch

    gen = torch.Generator(device=dev).manual_seed(5)
    return [synthetic_batch(64, 256, 10, device=dev, generator=gen) for _ in range(6)]


@functools.lru_cache(maxsize=None)
def _eager_compressed(cdt):
    """6 eager steps with a compressed, flattened bucket on a bf16 engine:
    (losses, parameters, shadow == bf16(parameters))."""
    from akka_allreduce_amd.models.mlp import MLP, dp_sgd_step
    from akka_allreduce_amd.parallel import ThresholdAllreduce
    from akka_allreduce_amd.parallel.dp import GradientBucket

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = MLP(256, 512, 10).to(dev)
    bucket = GradientBucket(list(model.parameters()), flatten_params=True, wire_dtype=torch.bfloat16)
    ar = ThresholdAllreduce(bucket.numel, max_chunk_size=4096, dtype=torch.bfloat16, device=dev)
    losses = [dp_sgd_step(model, x, y, 0.1, ar, bucket, compute_dtype=cdt) for x, y in _batches(dev)]
    torch.cuda.synchronize()
    shadow_ok = bucket.sflat is None or torch.equal(bucket.sflat, bucket.pflat.to(torch.bfloat16))
    return losses, bucket.pflat.clone(), shadow_ok, bucket.sflat is not None


@pytest.mark.parametrize("cdt", [None, torch.bfloat16])
def test_compressed_bucket_equals_emulated_wire(cdt):
    """The comparison run is the plain fp32 bucket and engine, its allreduce
    input replaced by the torch-emulated bf16(g + r): pack kernel and mixed
    update against torch's arithmetic and the fp32 update kernel."""
    from akka_allreduce_amd.models.mlp import MLP, dp_sgd_step
    from akka_allreduce_amd.parallel import ThresholdAllreduce
    from akka_allreduce_amd.parallel.dp import GradientBucket

    losses, params, shadow_ok, has_shadow = _eager_compressed(cdt)
    assert shadow_ok and has_shadow == (cdt is not None)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = MLP(256, 512, 10).to(dev)
    bucket = GradientBucket(list(model.parameters()), flatten_params=True)
    ar = ThresholdAllreduce(bucket.numel, max_chunk_size=4096, device=dev)
    r = torch.zeros(bucket.numel, device=dev)

    def emulated(t, out=None):
        e = t + r
        q = e.bfloat16()
        r.copy_(e - q.float())
        return ar(q.float())

    ref_losses = [dp_sgd_step(model, x, y, 0.1, emulated, bucket, compute_dtype=cdt) for x, y in _batches(dev)]
    torch.cuda.synchronize()
    assert torch.equal(params, bucket.pflat)
    assert losses == ref_losses


@pytest.mark.parametrize("cdt", [None, torch.bfloat16])
def test_graphed_compressed_step_matches_eager(cdt):
    from akka_allreduce_amd.models.mlp import MLP, GraphedDPStep
    from akka_allreduce_amd.parallel import ThresholdAllreduce
    from akka_allreduce_amd.parallel.dp import GradientBucket

    losses, params, _, _ = _eager_compressed(cdt)
    dev = torch.device("cuda", 0)
    batches = _batches(dev)
    torch.manual_seed(0)
    model = MLP(256, 512, 10).to(dev)
    bucket = GradientBucket(list(model.parameters()), flatten_params=True, wire_dtype=torch.bfloat16)
    ar = ThresholdAllreduce(bucket.numel, max_chunk_size=4096, dtype=torch.bfloat16, device=dev)
    step = GraphedDPStep(model, bucket, *batches[0], compute_dtype=cdt)
    got = [float(step(x, y, 0.1, ar)) for x, y in batches]
    torch.cuda.synchronize()
    for a, b in zip(losses, got):
        assert abs(a - b) <= 1e-5 * abs(a) + 1e-6, (losses, got)
    torch.testing.assert_close(bucket.pflat, params, rtol=1e-5, atol=1e-6)
    if cdt is None:
        # the graph bakes the wire and the residual in (a captured update reads them): moving either raises
        for name in ("wire", "residual"):
            keep = getattr(bucket, name)
            setattr(bucket, name, torch.empty_like(keep))
            with pytest.raises(RuntimeError, match="moved"):
                step(*batches[0], 0.1, ar)
            setattr(bucket, name, keep)
        step(*batches[0], 0.1, ar)


class _Bucket:
    """The part of dist.GradBucket the hook reads."""

    def __init__(self, t, index=0):
        self._t, self._i = t, index

    def buffer(self):
        return self._t

    def index(self):
        return self._i


@pytest.mark.parametrize("async_op", [True, False])
def test_hook_compressed_on_the_gpu(async_op):
    """N=1: the bucket becomes float(bf16(g + r)) in place, pack, round and
    mixed mean queued in stream order, one residual per bucket index."""
    from akka_allreduce_amd.parallel.ddp import ThresholdHookState, threshold_allreduce_hook

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    state = ThresholdHookState(max_chunk_size=1 << 14, async_op=async_op, wire_dtype=torch.bfloat16)
    r_want = torch.zeros(100_003, device=dev)
    for _ in range(3):
        g = torch.randn(100_003, device=dev)
        t = g.clone()
        got = threshold_allreduce_hook(state, _Bucket(t, 4)).wait()
        e = g + r_want
        q = e.bfloat16()
        r_want = e - q.float()
        torch.cuda.synchronize()
        assert got.data_ptr() == t.data_ptr() and torch.equal(t, q.float())
    assert list(state.wire_bufs) == [4] and torch.equal(state.wire_bufs[4][1], r_want)
    assert state.rounds == 3 and all(k[1] == torch.bfloat16 for k in state.engines)


# ---- two processes, ipc data plane ----------------------------------------------------------

def _port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _emulate_scheme(n, steps, dev, keep):
    """The whole scheme with torch alone: per-rank gradients (plain autograd),
    bf16(g + r) with a residual per rank, the sum rounded once to bf16, the
    fp32 mean of that, SGD.  Returns the flat parameters after ``keep`` and
    after ``steps`` steps."""
    from akka_allreduce_amd.models.mlp import MLP, synthetic_batch

    torch.manual_seed(0)
    model = MLP(256, 512, 10).to(dev)
    ps = list(model.parameters())
    res = [[torch.zeros_like(p) for p in ps] for _ in range(n)]
    snaps = []
    for s in range(steps):
        acc = [torch.zeros_like(p) for p in ps]
        for r in range(n):
            g = torch.Generator(device=dev).manual_seed(100 * s + r)
            x, y = synthetic_batch(64, 256, 10, device=dev, generator=g)
            model.zero_grad(set_to_none=True)
            torch.nn.functional.cross_entropy(model(x), y).backward()
            for i, p in enumerate(ps):
                e = p.grad + res[r][i]
                q = e.bfloat16()
                res[r][i] = e - q.float()
                acc[i] += q.float()
        with torch.no_grad():
            for p, a in zip(ps, acc):
                p -= 0.1 * (a.bfloat16().float() / n)
        if s + 1 in (keep, steps):
            snaps.append(torch.cat([p.detach().reshape(-1).cpu() for p in ps]))
    return snaps


def test_compressed_dp_two_processes_ipc():
    n, steps = 2, 3
    with tempfile.TemporaryDirectory() as out:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
               "--master-addr", "127.0.0.1", "--master-port", str(_port()),
               os.path.join(ROOT, "tests", "wire_ranks.py"), "--out-dir", out, "--steps", str(steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        res = [torch.load(os.path.join(out, f"rank{i}.pt"), weights_only=True) for i in range(n)]
    for d in res:
        assert d["ipc_error"] == 0 and d["replays"] == steps and len(d["wire_in"]) == steps
        assert tuple(d["after_capture"]) == (True, True)  # the capture's warm-up left parameters and residual alone
        resid = torch.zeros_like(d["grads"][0])
        for s in range(steps):
            # this rank's wire input is the emulation from its recorded fp32 gradients
            e = d["grads"][s] + resid
            q = e.bfloat16()
            resid = e - q.float()
            assert torch.equal(d["wire_in"][s], q), s
            # a two-term fp32 sum has no order: one rounding of q0 + q1
            want = (res[0]["wire_in"][s].float() + res[1]["wire_in"][s].float()).bfloat16()
            assert torch.equal(d["wire_out"][s], want), s
        assert torch.equal(d["eager"], res[0]["eager"]) and torch.equal(d["graphed"], res[0]["graphed"])
        assert not torch.equal(d["eager"], d["graphed"])
    want_eager, want_graphed = _emulate_scheme(n, 2 * steps, torch.device("cuda", 0), keep=steps)
    torch.testing.assert_close(res[0]["eager"], want_eager, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(res[0]["graphed"], want_graphed, rtol=1e-4, atol=1e-5)
