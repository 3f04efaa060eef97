"""``skip_nonfinite`` on the GPU: the norm pass's verdict and the update pass's
early exit.  With finite sums the guarded pass gives the bits of the unguarded
one; a poisoned sum leaves every buffer (the shadow's sentinels included) and
the step as they were, in every workgroup of every variant; a captured pass
skips and applies replay by replay; the MLP step and the bucket's shadow follow.
Every comparison is bitwise."""
import pytest
import torch

from akka_allreduce_amd.data import AllReduceOutput, OptimGroups, guard_state, sqnorm_workspace
from optim_cases import BF, H_SENTINEL, HYPER, _dev, _inputs, _kernel_state, _same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(7, 3, 2), (1003, 4, 67), (300_001, 2, 150_000)]
KINDS = ["sgd", "nesterov", "adamw"]
VALUES = {"inf": float("inf"), "nan": float("nan"), "2e19": 2e19}


def _gstep(inp, kind, state, data, ws, clip, guard=None, groups=None, pc=None, seed=9):
    """One step from the sum ``data``.  Without a guard the caller advances the step, as ``apply`` does; with
    one the norm pass does."""
    p, m, v, t, sh = state
    h = dict(HYPER[kind])
    lr = h.pop("lr")
    if groups is not None:
        lr = 0.0
        h.pop("weight_decay")
    out = AllReduceOutput(data, counts_per_chunk=inp["pc"] if pc is None else pc, geometry=inp["geo"])
    if guard is None:
        t.add_(1)
    adam = kind == "adamw"
    out.optim_step_("adamw" if adam else "sgd", p, m, v if adam else None, t, lr, shadow=sh,
                    max_norm=inp["max_norm"] if clip else None, norm_ws=ws, groups=groups, seed=seed, guard=guard,
                    **h)


def _groups(kind, S):
    # two groups over four segments; group 1 has lr 0 (its state advances and its p stays)
    g = OptimGroups([5, 130, 771, S], [0, 1, 0, 1], 2, _dev())
    g.write_rows(OptimGroups.row_values(HYPER[kind]["lr"], [(1.0, HYPER[kind]["weight_decay"]), (0.0, 0.1)]))
    return g


def _assert_same(got, want, what):
    for name, a, b in zip(("p", "m", "v", "t", "shadow"), got, want):
        assert (a is None and b is None) or _same_bits(a, b), f"{what}: {name} differs"


def _finite_case(S, N, C, kind, src, bf_state, shadow, grouped):
    inp = _inputs(S, N, C, src)
    dev = _dev()
    groups = _groups(kind, S) if grouped else None
    for clip in (False, True):
        off = _kernel_state(inp, shadow, BF if bf_state else None)
        on = _kernel_state(inp, shadow, BF if bf_state else None)
        ws_off, ws_on, guard = (sqnorm_workspace(dev) if clip else None), sqnorm_workspace(dev), guard_state(dev)
        for i in range(3):
            _gstep(inp, kind, off, inp["sums"][i], ws_off, clip, groups=groups)
            _gstep(inp, kind, on, inp["sums"][i], ws_on, clip, guard=guard, groups=groups)
        torch.cuda.synchronize()
        assert guard.tolist() == [1, 0, 0, 0] and int(on[3]) == 3
        _assert_same(on, off, f"clip={clip}")
        assert not bool((on[0] == inp["p0"]).all())
        if clip:
            assert _same_bits(ws_on[:2], ws_off[:2]) and float(ws_on[0]) > 0  # sq's bits, the ticket re-armed


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("shadow", [False, True])
@pytest.mark.parametrize("bf_state", [False, True])
@pytest.mark.parametrize("src", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_guard_on_equals_guard_off_over_finite_sums(kind, src, bf_state, shadow, grouped):
    _finite_case(1003, 4, 67, kind, src, bf_state, shadow, grouped)


@pytest.mark.parametrize("src", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S,N,C", [SHAPES[0], SHAPES[2]])
def test_guard_on_equals_guard_off_at_the_other_shapes(S, N, C, kind, src):
    _finite_case(S, N, C, kind, src, False, True, False)


@pytest.mark.parametrize("src", ["fp32", "bf16"])
@pytest.mark.parametrize("S,N,C", SHAPES)
def test_sq_has_the_same_bits_with_and_without_the_guard(S, N, C, src):
    inp = _inputs(S, N, C, src)
    dev = _dev()
    out = AllReduceOutput(inp["sums"][0], counts_per_chunk=inp["pc"], geometry=inp["geo"])
    ws0, ws1, guard, t = sqnorm_workspace(dev), sqnorm_workspace(dev), guard_state(dev), \
        torch.zeros(1, dtype=torch.int32, device=dev)
    a, b = out.sqnorm(ws0).clone(), out.sqnorm(ws1, guard, t).clone()
    torch.cuda.synchronize()
    assert _same_bits(a, b) and float(a) > 0 and int(t) == 1 and guard.tolist() == [1, 0, 0, 0]


def _poison_places(inp, pc, S):
    """An element in a region's scalar head, one in a vector body and the buffer's last one, all with count > 0
    (where the shape has no such region, the first element that has a contributor)."""
    geo = inp["geo"]
    host = pc.cpu()
    first = head = body = None
    for j in range(geo.workerNum):
        for k in range(geo.num_chunks(j)):
            cs, ce = geo.chunk_range(j, k)
            if int(host[j, k]) <= 0 or cs >= ce:
                continue
            a = (cs + 7) & ~7
            first = cs if first is None else first
            if head is None and cs < min(a, ce):
                head = cs
            if body is None and a + 16 <= ce:
                body = a + 9
    return {"head": first if head is None else head, "body": first if body is None else body, "last": S - 1}


@pytest.mark.parametrize("src", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,bf_state,grouped", [("sgd", False, False), ("adamw", True, False),
                                                   ("nesterov", True, True), ("adamw", False, True)])
@pytest.mark.parametrize("S,N,C", SHAPES)
def test_poisoned_sum_leaves_every_buffer_and_the_step_as_they_were(S, N, C, kind, bf_state, grouped, src):
    if grouped and S != 1003:
        grouped = False  # the segments are laid out for 1003 elements: the plain tail at the other shapes
    inp = _inputs(S, N, C, src)
    dev = _dev()
    geo = inp["geo"]
    # the region of the last element gets a contributor
    pc = inp["pc"].clone()
    jl = min((S - 1) // geo.step, N - 1)
    pc[jl, (S - 1 - jl * geo.step) // C] = N
    count = geo.expand_counts(pc)
    places = _poison_places(inp, pc, S)
    assert all(int(count[i]) > 0 for i in places.values())
    groups = _groups(kind, S) if grouped else None
    cpu_groups = None
    if grouped:
        cpu_groups = OptimGroups(groups.host_seg_end, groups.host_seg_group, 2, "cpu")
        cpu_groups.write_rows(groups.rows.cpu())
    state = _kernel_state(inp, True, BF if bf_state else None)
    start = [x.clone() for x in state]
    ws, guard = sqnorm_workspace(dev), guard_state(dev)
    # the CPU path over the same inputs: only its record is compared
    cpu_inp = dict(pc=pc.cpu(), geo=geo, max_norm=inp["max_norm"])
    cpu_state = [x.cpu() for x in start]
    cpu_ws, cpu_guard = sqnorm_workspace("cpu"), guard_state("cpu")
    skipped = 0
    for clip in (True, False):
        for where, at in places.items():
            for name, value in VALUES.items():
                data = inp["sums"][1].clone()
                data[at] = value * float(count[at]) if name == "2e19" else value
                _gstep(inp, kind, state, data, ws, clip, guard=guard, groups=groups, pc=pc)
                _gstep(cpu_inp, kind, cpu_state, data.cpu(), cpu_ws, clip, guard=cpu_guard, groups=cpu_groups)
                skipped += 1
                torch.cuda.synchronize()
                what = f"{name} in the {where}, clip={clip}"
                assert guard.tolist() == [0, skipped, skipped, 0] == cpu_guard.tolist(), what
                assert not bool(torch.isfinite(ws[0])), what
                _assert_same(state, start, what)
    assert bool((state[4] == H_SENTINEL).all()) and int(state[3]) == 0
    # the next finite sum is applied, as the first step of a run that saw none of the above
    _gstep(inp, kind, state, inp["sums"][0], ws, True, guard=guard, groups=groups, pc=pc)
    _gstep(cpu_inp, kind, cpu_state, inp["sums"][0].cpu(), cpu_ws, True, guard=cpu_guard, groups=cpu_groups)
    ref = [x.clone() for x in start]
    _gstep(inp, kind, ref, inp["sums"][0], sqnorm_workspace(dev), True, groups=groups, pc=pc)
    torch.cuda.synchronize()
    assert guard.tolist() == [1, skipped, 0, 0] == cpu_guard.tolist() and int(state[3]) == 1
    _assert_same(state, ref, "the applied step after the skipped ones")


def test_nonfinite_value_in_a_count_0_chunk_skips_nothing():
    S, N, C = 1003, 4, 67
    inp = _inputs(S, N, C, "fp32")
    dev = _dev()
    at = int(inp["missing"].nonzero()[3])
    data = inp["sums"][0].clone()
    data[at] = float("nan")
    data[at + 1] = float("inf")
    on, off = _kernel_state(inp), _kernel_state(inp)
    ws, guard = sqnorm_workspace(dev), guard_state(dev)
    _gstep(inp, "adamw", on, data, ws, True, guard=guard)
    _gstep(inp, "adamw", off, inp["sums"][0], sqnorm_workspace(dev), True)
    torch.cuda.synchronize()
    assert guard.tolist() == [1, 0, 0, 0] and int(on[3]) == 1
    _assert_same(on, off, "a count-0 chunk is never read")


@pytest.mark.parametrize("bf_state", [False, True])
def test_graph_replay_skips_and_applies_replay_by_replay(bf_state):
    """The norm pass and the AdamW pass captured once, with the guard; replays over finite, inf, finite, NaN,
    finite sums copied into the static sum are the three eager unguarded steps over the finite ones."""
    S, N, C = 300_001, 2, 150_000
    inp = _inputs(S, N, C, "fp32")
    dev = _dev()
    dt = BF if bf_state else None
    at = int((inp["count"] > 0).nonzero()[-1])
    eager, ws_e = _kernel_state(inp, True, dt), sqnorm_workspace(dev)
    for i in range(3):
        _gstep(inp, "adamw", eager, inp["sums"][i], ws_e, True)
    graphed, ws_g, guard = _kernel_state(inp, True, dt), sqnorm_workspace(dev), guard_state(dev)
    static = inp["sums"][0].clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _gstep(inp, "adamw", graphed, static, ws_g, True, guard=guard)
    torch.cuda.current_stream(dev).wait_stream(side)
    assert int(graphed[3]) == 0 and guard.tolist() == [0, 0, 0, 0]  # capturing ran nothing
    records = []
    for i, poison in ((0, None), (3, float("inf")), (1, None), (3, float("nan")), (2, None)):
        static.copy_(inp["sums"][i])
        if poison is not None:
            static[at] = poison
        graph.replay()
        records.append(guard.tolist())
    torch.cuda.synchronize()
    assert records == [[1, 0, 0, 0], [0, 1, 1, 0], [1, 1, 0, 0], [0, 2, 1, 0], [1, 2, 0, 0]]
    assert int(graphed[3]) == 3 and int(eager[3]) == 3
    _assert_same(graphed, eager, "replays against the eager finite steps")
    assert _same_bits(ws_g[:2], ws_e[:2])


def test_the_launcher_refuses_a_guard_without_the_norm_pass():
    from akka_allreduce_amd._native_loader import load
    from akka_allreduce_amd.data import counts_table

    inp = _inputs(1003, 4, 67, "fp32")
    p, m, v, t, sh = _kernel_state(inp)
    guard, ws = guard_state(_dev()), sqnorm_workspace(_dev())
    keep, table = counts_table(inp["pc"], inp["geo"])
    data = inp["sums"][0]
    with pytest.raises(Exception, match="guard"):
        load().count_optim("sgd", p.data_ptr(), m.data_ptr(), 0, 0, data.data_ptr(), "float32", table, t.data_ptr(),
                           0, torch.cuda.current_stream().cuda_stream, False, lr=0.1, guard=guard.data_ptr())
    with pytest.raises(Exception, match="guard"):
        load().count_sqnorm(ws.data_ptr(), data.data_ptr(), "float32", table, ws.data_ptr() + 8, ws.data_ptr() + 4,
                            torch.cuda.current_stream().cuda_stream, guard.data_ptr(), 0)
    torch.cuda.synchronize()
    assert _same_bits(p, inp["p0"]) and guard.tolist() == [0, 0, 0, 0]


# the MLP ------------------------------------------------------------------------------------------------------------
def _mlp(graphed, bad, guard=True, steps=6):
    """Six batches of the 64-128-10 MLP at N = 1 with FusedAdamW under the clip; ``bad``: the third batch holds
    one inf in x, else it is left out.  ``graphed``: a GraphedDPStep with the update eager."""
    from akka_allreduce_amd.models.mlp import MLP, GraphedDPStep, dp_sgd_step, synthetic_batch
    from akka_allreduce_amd.parallel import FusedAdamW, ThresholdAllreduce
    from akka_allreduce_amd.parallel.dp import GradientBucket

    dev = _dev()
    gen = torch.Generator(device=dev).manual_seed(5)
    batches = [synthetic_batch(32, 64, 10, device=dev, generator=gen) for _ in range(steps)]
    if bad:
        batches[2][0][3, 11] = float("inf")
    else:
        del batches[2]
    torch.manual_seed(0)
    model = MLP(64, 128, 10).to(dev)
    bucket = GradientBucket(list(model.parameters()), flatten_params=True)
    opt = FusedAdamW(bucket, weight_decay=0.01, max_grad_norm=1.0, **({"skip_nonfinite": True} if guard else {}))
    ar = ThresholdAllreduce(bucket.numel, max_chunk_size=4096, device=dev)
    step = GraphedDPStep(model, bucket, *batches[0], compute_dtype=BF, optimizer=opt) if graphed else None
    for x, y in batches:
        if graphed:
            step(x, y, 1e-2, ar)
        else:
            dp_sgd_step(model, x, y, 1e-2, ar, bucket, compute_dtype=BF, optimizer=opt, sync_loss=False)
    torch.cuda.synchronize()
    assert bucket._shadow_on
    rec = opt.guard.tolist() if guard else None
    return dict(pflat=bucket.pflat.clone(), sflat=bucket.sflat.clone(), m=opt.m.clone(), v=opt.v.clone(),
                t=int(opt.t), record=rec)


@pytest.fixture(scope="module")
def clean_mlp_run():
    """The five clean batches, eager and unguarded: computed once, read only."""
    return _mlp(False, False, guard=False)


@pytest.mark.parametrize("graphed", [False, True])
def test_mlp_run_with_a_bad_batch_equals_the_run_over_the_clean_ones(graphed, clean_mlp_run):
    got = _mlp(graphed, True)
    assert got["record"] == [1, 1, 0, 0] and got["t"] == clean_mlp_run["t"] == 5
    for name in ("pflat", "sflat", "m", "v"):
        assert _same_bits(got[name], clean_mlp_run[name]), name
    assert bool(torch.isfinite(got["pflat"]).all())
    assert _same_bits(got["sflat"], got["pflat"].to(BF))


def test_a_skipped_step_never_marks_a_stale_shadow_current():
    from akka_allreduce_amd.models.mlp import MLP, dp_sgd_step, synthetic_batch
    from akka_allreduce_amd.parallel import FusedAdamW, ThresholdAllreduce
    from akka_allreduce_amd.parallel.dp import GradientBucket

    dev = _dev()
    gen = torch.Generator(device=dev).manual_seed(5)
    x, y = synthetic_batch(32, 64, 10, device=dev, generator=gen)
    bad = x.clone()
    bad[0, 0] = float("inf")
    torch.manual_seed(0)
    model = MLP(64, 128, 10).to(dev)
    bucket = GradientBucket(list(model.parameters()), flatten_params=True)
    opt = FusedAdamW(bucket, max_grad_norm=1.0, skip_nonfinite=True)
    ar = ThresholdAllreduce(bucket.numel, max_chunk_size=4096, device=dev)
    dp_sgd_step(model, x, y, 1e-2, ar, bucket, compute_dtype=BF, optimizer=opt)
    assert bucket._shadow_on and _same_bits(bucket.sflat, bucket.pflat.to(BF))

    def rewrite():
        # a write the version counters do not see
        bucket.pflat.data.mul_(1.5)
        bucket.invalidate_shadow()
        assert not _same_bits(bucket.sflat, bucket.pflat.to(BF))

    # a forward (it refreshes the shadow) and a skipped step
    rewrite()
    p0 = bucket.pflat.clone()
    dp_sgd_step(model, bad, y, 1e-2, ar, bucket, compute_dtype=BF, optimizer=opt)
    assert opt.skipped_steps == 1 and not opt.last_step_applied and _same_bits(bucket.pflat, p0)
    assert _same_bits(bucket.sflat, p0.to(BF))
    # no forward in between: the skipped pass wrote no shadow and the stale one must not pass for current
    rewrite()
    p0 = bucket.pflat.clone()
    bucket.flat.fill_(float("nan"))
    opt.step_from(ar, 1e-2)
    assert opt.skipped_steps == 2 and opt.skipped_in_a_row == 2 and _same_bits(bucket.pflat, p0)
    assert bucket.use_shadow(BF)
    assert _same_bits(bucket.sflat, p0.to(BF))
    assert float(opt.grad_norm()) != float(opt.grad_norm())  # NaN: the norm of the skipped round
