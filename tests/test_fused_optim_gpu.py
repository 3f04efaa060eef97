"""The fused optimizer pass on the GPU (``optim.hip``: ``count_optim`` and
``count_sqnorm``) against torch's optimizers.

Numerics: from the same fp32 inputs, torch's optimizer in float64 is the
reference and torch's optimizer in fp32 on the GPU (``foreach=False``; AdamW
``capturable=True``) the comparator; the gradient of both is
``out.mean(dtype=torch.float32)`` (the ``count_mean`` kernel).  The kernel's
worst error against the reference may be at most 4x the comparator's, for p,
m and v, after 1 step and after 20, over every element.  Elements of count-0
chunks keep parameters and state in all three runs (the torch runs put them
back after each step).  Every case prints its ratios before it asserts;
profiles/r08/fused_opt/README.md holds the measured ones."""
import functools
import math

import pytest
import torch

import loop_cases as L
from akka_allreduce_amd.data import AllReduceOutput, sqnorm_workspace
from optim_cases import (H_SENTINEL, HYPER, M_SENTINEL, NGRAD, V_SENTINEL, _dev, _inputs, _kernel_state, _mlp_run,
                         _step)

pytestmark = pytest.mark.gpu

# the smallest shapes that reach each path of the region walk but the pipelined loop: one element; regions shorter
# than a unit (all head and tail); unaligned regions, no multiple of 4 or 8; few regions, so several workgroups share
# one (gridDim.y > 1: 74 of them at (300_001, 2, 150_000), a stride of 18 944 units against the region's 18 750, so
# every thread takes at most one unit, in the remainder loop); many regions with bodies, heads and tails.  None runs
# update_range's two-unit loop or wraps the grid (test_loop_cases_cpu.py); AT_DEPTH below does.
SHAPES = [(1, 1, 1), (7, 3, 2), (1003, 4, 67), (300_001, 2, 150_000), (1_000_003, 4, 4099)]
STEPS = (1, 20)
# loop_cases.DEEP: every thread runs the two-unit loop at least twice per region; loop_cases.WRAP: more regions than
# the grid has workgroups
AT_DEPTH = {L.DEEP: L.require_deep, L.WRAP: L.require_wrap}


def _torch_run(kind, inp, dtype, clip):
    """torch's optimizer on the means, count-0 elements put back after every
    step; (p, m, v) snapshots at STEPS."""
    h = HYPER[kind]
    p = torch.nn.Parameter(inp["p0"].to(dtype).clone())
    m, v = inp["m0"].to(dtype).clone(), inp["v0"].to(dtype).clone()
    if kind == "adamw":
        cap = dtype == torch.float32  # the float64 reference keeps the step (and the bias corrections) in double
        opt = torch.optim.AdamW([p], lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"],
                                foreach=False, capturable=cap)
        step = torch.zeros((), dtype=torch.float32, device=p.device if cap else "cpu")
        opt.state[p] = {"step": step, "exp_avg": m, "exp_avg_sq": v}
    else:
        opt = torch.optim.SGD([p], lr=h["lr"], momentum=h["momentum"], nesterov=h["nesterov"],
                              weight_decay=h["weight_decay"], foreach=False)
        opt.state[p] = {"momentum_buffer": m}
    missing = inp["missing"]
    snaps = {}
    for s in range(max(STEPS)):
        p.grad = inp["means"][s % NGRAD].to(dtype).clone()
        if clip:
            torch.nn.utils.clip_grad_norm_([p], inp["max_norm"], foreach=False)
        prev = [x.detach().clone() for x in (p, m, v)]
        opt.step()
        with torch.no_grad():
            for x, x0 in zip((p, m, v), prev):
                x.copy_(torch.where(missing, x0, x))
        if s + 1 in STEPS:
            snaps[s + 1] = tuple(x.detach().clone() for x in (p, m, v))
    return snaps


@functools.lru_cache(maxsize=2)
def _references(S, N, C, src, kind, clip):
    inp = _inputs(S, N, C, src)
    r = _torch_run(kind, inp, torch.float64, clip), _torch_run(kind, inp, torch.float32, clip)
    torch.cuda.synchronize()
    return r


# the topmost parameter varies fastest: both shadow cases share one reference, every case of a shape its inputs
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("kind", ["sgd", "nesterov", "adamw"])
@pytest.mark.parametrize("src", ["fp32", "bf16"])
@pytest.mark.parametrize("S,N,C", SHAPES)
def test_update_matches_torch(shadow, clip, kind, src, S, N, C):
    _check_update_matches_torch(shadow, clip, kind, src, S, N, C)


# DEEP first, one source dtype after the other, so its inputs are built once each
@pytest.mark.parametrize("clip,shadow", [(False, False), (True, True)])
@pytest.mark.parametrize("kind", ["sgd", "nesterov", "adamw"])
@pytest.mark.parametrize("src", ["fp32", "bf16"])
def test_update_matches_torch_in_the_pipelined_loop(src, kind, clip, shadow):
    AT_DEPTH[L.DEEP]()
    _check_update_matches_torch(shadow, clip, kind, src, *L.DEEP)


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_update_matches_torch_where_the_grid_wraps(kind):
    AT_DEPTH[L.WRAP]()
    _check_update_matches_torch(True, True, kind, "fp32", *L.WRAP)


def _check_update_matches_torch(shadow, clip, kind, src, S, N, C):
    inp = _inputs(S, N, C, src)
    ref64, ref32 = _references(S, N, C, src, kind, clip)
    missing = inp["missing"]
    assert bool(missing.any()) or N == 1
    state = _kernel_state(inp, shadow)
    ws = sqnorm_workspace(_dev()) if clip else None
    p, m, v, t, sh = state
    failures = []
    for i in range(max(STEPS)):
        _step(inp, kind, state, i, ws)
        if i + 1 not in STEPS:
            continue
        torch.cuda.synchronize()
        # count-0 regions: bitwise what they were
        assert torch.equal(p[missing], inp["p0"][missing])
        assert bool((m[missing] == M_SENTINEL).all())
        if kind == "adamw":
            assert bool((v[missing] == V_SENTINEL).all())
        else:
            assert torch.equal(v, inp["v0"])  # SGD has no second moment: untouched everywhere
        if shadow:
            assert bool((sh[missing].float() == H_SENTINEL).all())
            assert torch.equal(sh[~missing], p[~missing].to(torch.bfloat16))
        assert int(t) == i + 1
        for name, got, r64, r32 in zip("pmv", (p, m, v), ref64[i + 1], ref32[i + 1]):
            err = float((got.double() - r64).abs().max())
            cmp_err = float((r32.double() - r64).abs().max())
            ratio = err / cmp_err if cmp_err > 0 else (0.0 if err == 0 else math.inf)
            print(f"RATIO S={S} src={src} kind={kind} clip={int(clip)} shadow={int(shadow)} step={i + 1} {name} "
                  f"kernel={err:.3e} torch32={cmp_err:.3e} ratio={ratio:.3f}")
            if not err <= 4 * cmp_err:
                failures.append((i + 1, name, err, cmp_err))
    assert not failures, failures


@pytest.mark.parametrize("S,N,C", SHAPES)
@pytest.mark.parametrize("src", ["fp32", "bf16"])
def test_sqnorm_matches_float64_and_is_deterministic(src, S, N, C):
    inp = _inputs(S, N, C, src)
    ws = sqnorm_workspace(_dev())
    out = AllReduceOutput(inp["sums"][0], counts_per_chunk=inp["pc"], geometry=inp["geo"])
    got = [out.sqnorm(ws).clone() for _ in range(3)]
    c = inp["count"].double()
    mean64 = torch.where(c > 0, inp["sums"][0].double() / c.clamp(min=1), torch.zeros_like(c))
    want = float((mean64 * mean64).sum())
    torch.cuda.synchronize()
    # non-negative terms, add chains < 100 long: relative error <= 100 * 2**-24 < 1e-5
    assert abs(float(got[0]) - want) <= 1e-5 * want, (float(got[0]), want)
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])  # the ticket re-arms
    assert float(ws[1]) == 0.0


def test_all_chunks_missing_is_a_no_op():
    S, N, C = 1003, 4, 67
    inp = _inputs(S, N, C, "fp32")
    pc = torch.zeros_like(inp["pc"])
    p, m, v, t, sh = _kernel_state(inp, True)
    ws = sqnorm_workspace(_dev())
    t.add_(1)
    out = AllReduceOutput(inp["sums"][0], counts_per_chunk=pc, geometry=inp["geo"])
    out.optim_step_("adamw", p, m, v, t, 1e-3, shadow=sh, max_norm=1.0, norm_ws=ws)
    torch.cuda.synchronize()
    assert float(ws[0]) == 0.0
    assert torch.equal(p, inp["p0"]) and torch.equal(m, inp["m0"]) and torch.equal(v, inp["v0"])
    assert bool((sh.float() == H_SENTINEL).all())


def test_cuda_tensors_never_fall_back():
    inp = _inputs(1003, 4, 67, "fp32")
    out = AllReduceOutput(inp["sums"][0], counts_per_chunk=inp["pc"], geometry=inp["geo"])
    base = torch.zeros(1003 + 1, device=_dev())
    m, t = torch.zeros(1003, device=_dev()), torch.ones(1, dtype=torch.int32, device=_dev())
    with pytest.raises(ValueError, match="aligned"):
        out.optim_step_("sgd", base[1:], m, None, t, 0.1)  # p is not 16-B aligned
    _ = out.count  # per-element counts expanded: the fused conditions of axpy_mean_ no longer hold
    with pytest.raises(ValueError, match="fused pass"):
        out.optim_step_("sgd", base[:1003], m, None, t, 0.1)


@pytest.mark.parametrize("src", ["fp32", "bf16"])
def test_graph_replay_of_the_adamw_pass(src):
    """t.add_(1), the norm pass and the update captured once: three replays
    are three steps (the step counter is on the device, the norm workspace
    re-arms itself), bitwise the three eager calls from the same start."""
    S, N, C = 300_001, 2, 150_000
    inp = _inputs(S, N, C, src)
    dev = _dev()
    eager = _kernel_state(inp, True)
    ws_e = sqnorm_workspace(dev)
    for _ in range(3):
        _step(inp, "adamw", eager, 0, ws_e)
    graphed = _kernel_state(inp, True)
    ws_g = sqnorm_workspace(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _step(inp, "adamw", graphed, 0, ws_g)
    torch.cuda.current_stream(dev).wait_stream(side)
    for x, x0 in zip(graphed[:3], (inp["p0"], inp["m0"], inp["v0"])):
        assert torch.equal(x, x0)  # capturing ran nothing
    assert int(graphed[3]) == 0
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(graphed[3]) == 3 and int(eager[3]) == 3
    for name, a, b in zip(("p", "m", "v", "t", "shadow"), eager, graphed):
        assert torch.equal(a, b), name
    assert torch.equal(ws_e[:2], ws_g[:2])


@pytest.mark.parametrize("wire", [False, True])
def test_graphed_mlp_step_with_fused_adamw_matches_eager(wire):
    eager = _mlp_run(False, wire)
    graphed = _mlp_run(True, wire)
    assert eager["losses"] == graphed["losses"], (eager["losses"], graphed["losses"])
    for name in ("pflat", "sflat", "m", "v"):
        assert torch.equal(eager[name], graphed[name]), name
    assert torch.equal(graphed["sflat"], graphed["pflat"].to(torch.bfloat16))
