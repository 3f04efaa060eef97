"""The grouped optimizer pass on the GPU (``optim.hip``: ``count_optim`` with a
group table) and what is built on it: per-group weight decay and learning rate
read from a device table when the kernel runs.

Numerics as in ``test_fused_optim_gpu.py``: from the same fp32 inputs torch's
optimizer in float64 is the reference and torch's optimizer in fp32 on the GPU
(``foreach=False``; AdamW ``capturable=True``) the comparator, both with one
Parameter per segment and the groups' ``lr * lr_scale`` / ``weight_decay``; the
kernel's worst error against the reference may be at most 4x the comparator's,
for p, m and v, after 1 step and after 20, over every element.  Elements of
count-0 chunks keep parameters and state in all three runs.  Every case prints
its ratios before it asserts; profiles/r09/param_groups/README.md holds the
measured ones."""
import functools
import math

import pytest
import torch

from akka_allreduce_amd.data import OptimGroups, sqnorm_workspace
from optim_cases import (H_SENTINEL, HYPER, M_SENTINEL, NGRAD, V_SENTINEL, _dev, _inputs, _kernel_state, _mlp_run,
                         _step)

pytestmark = pytest.mark.gpu


def _random_cuts(S, n, seed):
    g = torch.Generator().manual_seed(seed)
    cuts = (torch.randperm(S - 1, generator=g)[:n] + 1).sort().values.tolist()  # distinct, in [1, S)
    return tuple(cuts) + (S,)


# (S, N, C), segment ends: one element; everything through the scalar path; blocks of 251 with one-element first and
# last segments, a segment shorter than a unit, ends on a region and on a block boundary, four segments inside one
# region, segments spanning regions and blocks; regions shared by several workgroups with unaligned segment starts
# (the unrolled loop and its remainder per sub-range); many regions per segment; many segments (the binary search)
CASES = {
    "one": ((1, 1, 1), (1,)),
    "scalar": ((7, 3, 2), (1, 2, 7)),
    "blocks": ((1003, 4, 67), (1, 5, 67, 70, 71, 72, 251, 640, 1002, 1003)),
    "shared": ((300_001, 2, 150_000), (9, 70_003, 150_000, 150_001, 299_999, 300_001)),
    "regions": ((1_000_003, 4, 4099), (12_302, 250_001, 600_000, 1_000_003)),
    "search": ((1_000_003, 4, 4099), _random_cuts(1_000_003, 257, 11)),
}
assert len(CASES["search"][1]) == 258 and len(set(CASES["search"][1])) == 258
# groups round-robin over the segments, so neighbours always differ
GROUP_SCALE, GROUP_WD = (1.0, 0.1, 2.5), (0.01, 0.0, 0.1)
STEPS = (1, 20)


def _groups(ends, lr, scales=GROUP_SCALE, wds=GROUP_WD):
    g = OptimGroups(ends, [i % len(scales) for i in range(len(ends))], len(scales), _dev())
    g.write_rows(OptimGroups.row_values(lr, list(zip(scales, wds))))
    return g


def _torch_run(kind, inp, ends, dtype, clip):
    """torch's optimizer with one Parameter per segment (views of one flat
    buffer, like the state) and the groups' lr and weight decay, count-0
    elements put back after every step; (p, m, v) snapshots at STEPS."""
    h = HYPER[kind]
    p, m, v = (inp[k].to(dtype).clone() for k in ("p0", "m0", "v0"))
    cap = dtype == torch.float32  # the float64 reference keeps the step (and the bias corrections) in double
    params, pgs, lo = [], [], 0
    for i, hi in enumerate(ends):
        q = torch.nn.Parameter(p[lo:hi])  # shares p's memory
        params.append((q, lo, hi))
        pgs.append({"params": [q], "lr": h["lr"] * GROUP_SCALE[i % 3], "weight_decay": GROUP_WD[i % 3]})
        lo = hi
    if kind == "adamw":
        opt = torch.optim.AdamW(pgs, lr=h["lr"], betas=h["betas"], eps=h["eps"], foreach=False, capturable=cap)
        for q, lo, hi in params:
            opt.state[q] = {"step": torch.zeros((), dtype=torch.float32, device=p.device if cap else "cpu"),
                            "exp_avg": m[lo:hi], "exp_avg_sq": v[lo:hi]}
    else:
        opt = torch.optim.SGD(pgs, lr=h["lr"], momentum=h["momentum"], nesterov=h["nesterov"], foreach=False)
        for q, lo, hi in params:
            opt.state[q] = {"momentum_buffer": m[lo:hi]}
    missing = inp["missing"]
    snaps = {}
    for s in range(max(STEPS)):
        grad = inp["means"][s % NGRAD].to(dtype).clone()
        for q, lo, hi in params:
            q.grad = grad[lo:hi]
        if clip:
            torch.nn.utils.clip_grad_norm_([q for q, _, _ in params], inp["max_norm"], foreach=False)
        prev = [x.clone() for x in (p, m, v)]
        opt.step()
        with torch.no_grad():
            for x, x0 in zip((p, m, v), prev):
                x.copy_(torch.where(missing, x0, x))
        if s + 1 in STEPS:
            snaps[s + 1] = tuple(x.clone() for x in (p, m, v))
    return snaps


@functools.lru_cache(maxsize=2)
def _references(case, src, kind, clip):
    (S, N, C), ends = CASES[case]
    inp = _inputs(S, N, C, src)
    r = _torch_run(kind, inp, ends, torch.float64, clip), _torch_run(kind, inp, ends, torch.float32, clip)
    torch.cuda.synchronize()
    return r


# 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("kind", ["sgd", "nesterov", "adamw"])
@pytest.mark.parametrize("src", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_one_group_equals_the_legacy_pass_bitwise(shadow, clip, kind, src, case):
    (S, N, C), _ = CASES[case]
    inp = _inputs(S, N, C, src)
    h = HYPER[kind]
    groups = _groups((S,), h["lr"], scales=(1.0,), wds=(h["weight_decay"],))
    legacy, grouped = _kernel_state(inp, shadow), _kernel_state(inp, shadow)
    ws_l, ws_g = (sqnorm_workspace(_dev()), sqnorm_workspace(_dev())) if clip else (None, None)
    for i in range(3):
        _step(inp, kind, legacy, i, ws_l)
        _step(inp, kind, grouped, i, ws_g, groups)
    torch.cuda.synchronize()
    assert int(grouped[3]) == 3
    assert not torch.equal(grouped[0], inp["p0"]) or S == 1
    for name, a, b in zip(("p", "m", "v", "t", "shadow"), legacy, grouped):
        if a is not None:
            assert torch.equal(a, b), name


# 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("kind", ["sgd", "nesterov", "adamw"])
@pytest.mark.parametrize("src", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_groups_match_torch(clip, kind, src, case):
    (S, N, C), ends = CASES[case]
    inp = _inputs(S, N, C, src)
    ref64, ref32 = _references(case, src, kind, clip)
    missing = inp["missing"]
    assert bool(missing.any()) or N == 1
    groups = _groups(ends, HYPER[kind]["lr"])
    state = _kernel_state(inp, True)
    ws = sqnorm_workspace(_dev()) if clip else None
    p, m, v, t, sh = state
    failures = []
    for i in range(max(STEPS)):
        _step(inp, kind, state, i, ws, groups)
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
        assert bool((sh[missing].float() == H_SENTINEL).all())
        assert torch.equal(sh[~missing], p[~missing].to(torch.bfloat16))
        assert int(t) == i + 1
        for name, got, r64, r32 in zip("pmv", (p, m, v), ref64[i + 1], ref32[i + 1]):
            err = float((got.double() - r64).abs().max())
            cmp_err = float((r32.double() - r64).abs().max())
            ratio = err / cmp_err if cmp_err > 0 else (0.0 if err == 0 else math.inf)
            print(f"RATIO case={case} S={S} segs={len(ends)} src={src} kind={kind} clip={int(clip)} step={i + 1} "
                  f"{name} kernel={err:.3e} torch32={cmp_err:.3e} ratio={ratio:.3f}")
            if not err <= 4 * cmp_err:
                failures.append((i + 1, name, err, cmp_err))
    assert not failures, failures


# 3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["fp32", "bf16"])
def test_a_group_with_lr_zero(src):
    (S, N, C), ends = CASES["blocks"]
    inp = _inputs(S, N, C, src)
    missing = inp["missing"]
    in_group = torch.zeros(S, dtype=torch.bool, device=_dev())
    lo = 0
    for i, hi in enumerate(ends):
        if i % 3 == 1:
            in_group[lo:hi] = True
        lo = hi
    live = in_group & ~missing
    assert bool(live.any()) and bool((inp["v0"][live] == 0).all())  # AdamW from v == 0: the step is 0 / -0
    runs = []
    for scale in (0.0, 1.0):
        groups = _groups(ends, HYPER["adamw"]["lr"], scales=(1.0, scale, 2.5))
        state = _kernel_state(inp, True)
        _step(inp, "adamw", state, 0, sqnorm_workspace(_dev()), groups)
        runs.append(state)
    torch.cuda.synchronize()
    (p, m, v, t, sh), (p1, m1, v1, _, _) = runs
    for name, x in zip("pmv", (p, m, v)):
        fin = float(torch.isfinite(x).float().mean())
        print(f"RATIO zero-lr src={src} {name} finite={fin:.6f}")
        assert fin == 1.0, name
    assert bool(torch.isfinite(sh.float()).all())
    assert torch.equal(p[in_group], inp["p0"][in_group])
    assert torch.equal(sh[live], p[live].to(torch.bfloat16)) and bool((sh[missing].float() == H_SENTINEL).all())
    assert torch.equal(m[in_group], m1[in_group]) and torch.equal(v[in_group], v1[in_group])
    assert bool((m[live] != 0).any()) and bool((v[live] != 0).any())  # the state advanced
    assert not torch.equal(p1[live], inp["p0"][live])  # with a positive lr the group moves
    others = ~in_group
    assert torch.equal(p[others], p1[others]) and not torch.equal(p[others & ~missing], inp["p0"][others & ~missing])


# 4 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["fp32", "bf16"])
def test_a_schedule_under_replay(src):
    """t.add_(1), the norm pass and the grouped update captured once; the rows
    are rewritten between the replays, outside the graph: three replays are
    the three eager steps with those learning rates, bitwise."""
    (S, N, C), ends = CASES["shared"]
    inp = _inputs(S, N, C, src)
    dev = _dev()
    lrs = (1e-3, 5e-4, 0.0)
    hyper = list(zip(GROUP_SCALE, GROUP_WD))
    eager, g_e, ws_e = _kernel_state(inp, True), _groups(ends, lrs[0]), sqnorm_workspace(dev)
    for lr in lrs:
        g_e.write_rows(OptimGroups.row_values(lr, hyper))
        _step(inp, "adamw", eager, 0, ws_e, g_e)
    graphed, g_g, ws_g = _kernel_state(inp, True), _groups(ends, lrs[0]), sqnorm_workspace(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _step(inp, "adamw", graphed, 0, ws_g, g_g)
    torch.cuda.current_stream(dev).wait_stream(side)
    for x, x0 in zip(graphed[:3], (inp["p0"], inp["m0"], inp["v0"])):
        assert torch.equal(x, x0)  # capturing ran nothing
    rows_ptr = g_g.rows.data_ptr()
    for lr in lrs:
        g_g.write_rows(OptimGroups.row_values(lr, hyper))
        graph.replay()
    torch.cuda.synchronize()
    assert g_g.rows.data_ptr() == rows_ptr
    assert int(graphed[3]) == 3 and int(eager[3]) == 3
    for name, a, b in zip(("p", "m", "v", "t", "shadow"), eager, graphed):
        assert torch.equal(a, b), name
    assert torch.equal(ws_e[:2], ws_g[:2]) and float(ws_g[1]) == 0.0  # the ticket is zero again
    assert bool(torch.isfinite(graphed[0]).all())


# 5 -----------------------------------------------------------------------------------------------------------------
MLP_LRS = (1e-2, 8e-3, 6e-3, 3e-3, 1e-3)


def _groups_mlp_run(graphed, wire, bias_decay=0.0, **kw):
    """A different lr each step, the biases in a group of their own."""
    return _mlp_run(graphed, wire, lrs=MLP_LRS, bias_decay=bias_decay, **kw)


@pytest.mark.parametrize("wire", [False, True])
def test_graphed_mlp_step_with_param_groups_matches_eager(wire):
    eager = _groups_mlp_run(False, wire)
    graphed = _groups_mlp_run(True, wire)
    assert eager["t"] == 5 and graphed["t"] == 5
    assert eager["losses"] == graphed["losses"], (eager["losses"], graphed["losses"])
    for name in ("pflat", "sflat", "m", "v"):
        assert torch.equal(eager[name], graphed[name]), name
    assert torch.equal(graphed["sflat"], graphed["pflat"].to(torch.bfloat16))
    # the biases are out of the decay: after one step they differ from the run that decays them, the weights do not
    decayed = _groups_mlp_run(False, wire, bias_decay=0.01, steps=1)
    for name, (o, n) in eager["spans"].items():
        same = torch.equal(eager["after1"][o:o + n], decayed["after1"][o:o + n])
        assert same == name.startswith("w"), name


def test_load_state_dict_into_a_graphed_step_mid_run():
    eager = _groups_mlp_run(False, False, save_at=3)
    graphed = _groups_mlp_run(True, False, load=eager["saved"])
    assert graphed["t"] == 5
    assert eager["losses"][3:] == graphed["losses"][2:], (eager["losses"], graphed["losses"])
    for name in ("pflat", "sflat", "m", "v"):
        assert torch.equal(eager[name], graphed[name]), name
