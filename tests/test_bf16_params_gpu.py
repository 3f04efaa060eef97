"""bf16 parameters on the GPU (``optim.hip``: the ``TP = bf16_t`` instantiations
of ``count_optim`` and ``lamb_norms``).

The reference of one step is the kernel that existed before: fp32 ``p`` with
bf16 ``m`` / ``v``, run from the widened ``p`` with the same state, step and
seed.  ``p`` must be ``_sr(p_ref, r_p)`` bit for bit with the bits of
``_bits_p`` -- the tests' own numpy copy of the second hash
(``bf16_param_cases.py``), written from the README's definition and not
imported from the package -- and ``m``, ``v`` and LAMB's trust table the
reference's own bits."""
import functools
import math

import pytest
import torch

from akka_allreduce_amd.data import DTYPE_NAME, AllReduceOutput, Geometry, counts_table
from bf16_param_cases import Opts, check_stall, check_steps, make_inputs, stall_run, start_state
from optim_cases import BF, _same_bits

pytestmark = pytest.mark.gpu

# one element; regions shorter than a unit; unaligned regions, no multiple of 8; few regions, so that several
# workgroups share one (gridDim.y > 1) and run the unrolled loop and its remainder
SHAPES = [(1, 1, 1), (7, 3, 2), (1003, 4, 67), (300_001, 2, 150_000)]
DEV = "cuda:0"


# ---- 1. the kernel against the existing kernel ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sgd", "adamw", "lamb"])
@pytest.mark.parametrize("src", ["fp32", "bf16"])
@pytest.mark.parametrize("S,N,C", SHAPES)
def test_one_step_is_the_fp32_p_kernel_then_sr(S, N, C, src, kind):
    """Plain, then with 4 segments in 2 groups (SGD's grouped run with Nesterov momentum); three steps each."""
    inp = make_inputs(S, N, C, src, DEV)
    check_steps(Opts(kind, inp))
    check_steps(Opts("nesterov" if kind == "sgd" else kind, inp, grouped=True))


# ---- 2. clip and guard ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sgd", "adamw", "lamb"])
def test_clip_and_guard_applied_then_skipped(kind):
    S, N, C = 1003, 4, 67
    inp = make_inputs(S, N, C, "fp32", DEV)
    o = Opts(kind, inp, grouped=True, clip=True, guard=True)
    st, bufs = check_steps(o, steps=2)  # applied steps: the norm pass advances t
    assert float(bufs["norm_ws"][0]) > 0
    before = [x.clone() for x in st]
    trust = bufs["lamb"]["trust"].clone() if kind == "lamb" else None
    bad = inp["sums"][2].clone()
    bad[(~inp["missing"]).nonzero().flatten()[17]] = math.nan
    o.step(bufs, st, 2, src=bad)
    torch.cuda.synchronize()
    assert bufs["guard"].tolist() == [0, 1, 1, 0]
    for name, a, b in zip("pmvt", st, before):
        assert _same_bits(a, b) if a.is_floating_point() else torch.equal(a, b), name
    if trust is not None:
        assert _same_bits(bufs["lamb"]["trust"], trust)
    o.step(bufs, st, 2)
    torch.cuda.synchronize()
    assert bufs["guard"].tolist() == [1, 1, 0, 0] and int(st[3]) == 3
    assert not _same_bits(st[1], before[1])


# ---- 3. kernel equals torch path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_kernel_and_torch_path_agree(kind):
    """Both implement one definition, but the existing fp32 tests pin the kernel and the torch path to
    torch's optimizers within a tolerance (``optim_cases._close``: rtol 1e-5, atol 1e-6 of the largest value),
    not to each other bit for bit, so ``p`` is compared here within that tolerance plus one bf16 ulp: where the
    two fp32 results differ in their last bits, the same r may carry in one and not in the other.  The
    authoritative bitwise check is test 1.  ``m`` and ``v`` likewise.  (Measured: no element differs.)"""
    S, N, C = 1003, 4, 67
    results = []
    for dev in ("cpu", DEV):
        inp = make_inputs(S, N, C, "fp32", dev)
        o = Opts(kind, inp)
        st, bufs = start_state(inp), o.buffers()
        for i in range(3):
            o.step(bufs, st, i)
        results.append([x.cpu() for x in st])
    torch.cuda.synchronize()
    for name, a, b in zip("pmv", *results):
        a, b = a.float(), b.float()
        ulp = torch.exp2(torch.floor(torch.log2(b.abs().clamp(min=1e-30))) - 7)
        tol = 1e-5 * b.abs() + 1e-6 * float(b.abs().max()) + ulp
        diff = (a - b).abs()
        print(f"PATHS kind={kind} {name}: {int((diff != 0).sum())} of {S} elements differ, worst {float(diff.max()):.3e}")
        assert bool((diff <= tol).all()), (name, float((diff - tol).max()))
    assert int(results[0][3]) == int(results[1][3]) == 3


# ---- 4. fixed points on the device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("S,N,C", [(1003, 4, 67), (300_001, 2, 150_000)])
def test_a_zero_update_keeps_p_bitwise(S, N, C):
    inp = make_inputs(S, N, C, "fp32", DEV)
    p, m, v, t = start_state(inp)
    p0 = p.clone()
    m.zero_()
    out = AllReduceOutput(torch.zeros(S, device=DEV), counts_per_chunk=inp["pc"], geometry=inp["geo"])
    for _ in range(3):
        t.add_(1)
        out.optim_step_("sgd", p, m, None, t, 0.05, momentum=0.0, weight_decay=0.0, seed=3)
    torch.cuda.synchronize()
    assert _same_bits(p, p0)


@pytest.mark.parametrize("kind", ["sgd", "adamw", "lamb"])
def test_a_group_at_lr_zero_keeps_p_bitwise_and_advances_the_state(kind):
    S, N, C = 1003, 4, 67
    inp = make_inputs(S, N, C, "fp32", DEV)
    o = Opts(kind, inp, grouped=True, group1=(0.0, 0.1))
    (p, m, v, t), _ = check_steps(o)
    p, m, v = p.cpu(), m.cpu(), v.cpu()
    still = torch.zeros(S, dtype=torch.bool)
    still[5:130] = still[771:] = True
    live = ~inp["missing"]
    assert _same_bits(p[still], inp["p0"].cpu()[still])
    assert not _same_bits(m[still & live], inp["m0"].cpu()[still & live])
    if o.adam:
        assert not _same_bits(v[still & live], inp["v0"].cpu()[still & live])
    assert bool((p[~still & live] != inp["p0"].cpu()[~still & live]).any())


# ---- 5. the stall --------------------------------------------------------------------------------------------------
def test_p_does_not_stall():
    """The 1000-step run of test_bf16_params_cpu.py on the kernel, same bounds.  With a gradient of 1 every
    operation of the step is exact but the one product-sum ``p - 1e-4``, which kernel and torch path round
    once from the same exact value: the bits, and so the mean, are the CPU run's."""
    from test_bf16_params_cpu import OBSERVED_MEAN

    p = stall_run(DEV)
    assert p.dtype == BF
    mean = check_stall(p)
    assert mean == OBSERVED_MEAN, (mean, OBSERVED_MEAN)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------
def test_refusals_in_optim_step_and_in_the_launcher():
    from akka_allreduce_amd._native_loader import load

    S = 64
    dev = torch.device(DEV)
    pc = torch.ones((1, 1), dtype=torch.int32, device=dev)
    geo = Geometry(S, 1, S)
    out = AllReduceOutput(torch.ones(S, device=dev), counts_per_chunk=pc, geometry=geo)
    p, t = torch.ones(S, dtype=BF, device=dev), torch.ones(1, dtype=torch.int32, device=dev)
    bf = lambda: torch.zeros(S, dtype=BF, device=dev)  # noqa: E731
    f32 = lambda: torch.zeros(S, device=dev)  # noqa: E731
    with pytest.raises(ValueError, match="bfloat16 m and v"):
        out.optim_step_("adamw", p, f32(), f32(), t, 1e-3)
    with pytest.raises(ValueError, match="shadow"):
        out.optim_step_("adamw", p, bf(), bf(), t, 1e-3, shadow=bf())
    with pytest.raises(ValueError, match="nt"):
        out.optim_step_("sgd", p, bf(), None, t, 1e-3, nt=True)

    nat = load()
    keep, table = counts_table(pc, geo)
    stream = torch.cuda.current_stream().cuda_stream

    def native(m, v, shadow=None, nt=False):
        nat.count_optim("adamw", p.data_ptr(), m.data_ptr(), v.data_ptr(), shadow.data_ptr() if shadow is not None else 0,
                        out.data.data_ptr(), "float32", table, t.data_ptr(), 0, stream, nt, lr=1e-3,
                        state_dtype=DTYPE_NAME[m.dtype], param_dtype="bfloat16")

    with pytest.raises(RuntimeError, match="bfloat16 parameters need bfloat16 state"):
        native(f32(), f32())
    with pytest.raises(RuntimeError, match="no shadow with bfloat16 parameters"):
        native(bf(), bf(), shadow=bf())
    with pytest.raises(RuntimeError, match="no nontemporal variant"):
        native(bf(), bf(), nt=True)
    with pytest.raises(RuntimeError, match="bfloat16 parameters need bfloat16 state"):
        nat.lamb_norms(f32().data_ptr(), S // 2, p.data_ptr(), f32().data_ptr(), f32().data_ptr(), out.data.data_ptr(),
                       "float32", table, t.data_ptr(), 0,
                       (0, 0, 0, [S], [0], 1), stream, state_dtype="float32", param_dtype="bfloat16")
    torch.cuda.synchronize()
    assert torch.equal(p, torch.ones(S, dtype=BF, device=dev))  # nothing ran


# ---- 7. a captured step --------------------------------------------------------------------------------------------
# In ONE fresh child process, as the graph cases of test_fused_lamb_gpu.py and for their reason: a capture's side
# stream stays live in the process with a hardware queue, and the suite's process keeps its queues for the lanes.
def _graph_child():
    from akka_allreduce_amd.parallel import FusedAdamW
    from akka_allreduce_amd.parallel.dp import GradientBucket

    dev = torch.device(DEV)
    lr = 1e-2

    def fresh():
        torch.manual_seed(0)
        ps = [torch.nn.Parameter(torch.randn(n, device=dev).to(BF)) for n in (150_000, 60, 150_001, 3)]
        b = GradientBucket(ps, flatten_params=True)
        b.flat.copy_(torch.randn(b.numel, generator=torch.Generator().manual_seed(1)).to(dev))
        opt = FusedAdamW(b, weight_decay=0.01, max_grad_norm=1.0, state_dtype=BF, seed=7, device_lr=True,
                         param_groups=[{"params": [ps[1], ps[3]], "weight_decay": 0.0}])
        opt.set_lr(lr)
        return b, opt

    b_e, o_e = fresh()
    for _ in range(3):
        o_e.step_from(None, lr)
    b_g, o_g = fresh()
    p0 = b_g.pflat.clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        o_g.step_from(None, lr)
    torch.cuda.current_stream(dev).wait_stream(side)
    assert _same_bits(b_g.pflat, p0) and int(o_g.t) == 0  # capturing ran nothing
    after = []
    for _ in range(3):
        graph.replay()
        after.append(b_g.pflat.clone())
    torch.cuda.synchronize()
    assert int(o_g.t) == 3 and int(o_e.t) == 3
    assert b_g.pflat.dtype == BF and o_g.param_dtype == BF
    for name, a, b in (("p", b_e.pflat, b_g.pflat), ("m", o_e.m, o_g.m), ("v", o_e.v, o_g.v)):
        assert _same_bits(a, b), name
    # each replay drew new bits and moved p again
    assert not _same_bits(after[0], p0) and not _same_bits(after[1], after[0]) and not _same_bits(after[2], after[1])
    print("graph ok bf16 params", flush=True)


@functools.lru_cache(maxsize=1)
def _graph_child_output():
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", "import test_bf16_params_gpu as t; t._graph_child()"], cwd=here,
                       env=dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here,
                                                                         os.environ.get("PYTHONPATH", "")])),
                       capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


def test_captured_step_replays_as_eager_steps():
    rc, out, err = _graph_child_output()
    assert "graph ok bf16 params" in out and rc == 0, (rc, out[-2000:], err[-3000:])


# ---- sentinels under every kind, all chunks missing ----------------------------------------------------------------
def test_all_chunks_missing_keeps_everything():
    S, N, C = 1003, 4, 67
    inp = dict(make_inputs(S, N, C, "bf16", DEV))
    inp["pc"] = torch.zeros_like(inp["pc"])
    for kind in ("sgd", "adamw", "lamb"):
        o = Opts(kind, inp)
        st = start_state(inp)
        before = [x.clone() for x in st]
        o.step(o.buffers(), st, 0)
        torch.cuda.synchronize()
        for name, a, b in zip("pmv", st, before):
            assert _same_bits(a, b), (kind, name)
