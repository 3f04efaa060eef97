"""bf16 moments with stochastic rounding on the GPU (``optim.hip``, the
``bf16_t`` state instantiations of ``count_optim``, with and without a group table).

The reference of one step is the fp32-state kernel run from the widened copies
of the same bf16 state: ``p`` and the shadow must be its ``p`` and shadow bit
for bit, and ``m`` / ``v`` its ``m'`` / ``v'`` rounded by ``_sr`` with the bits
of ``_bits`` -- the tests' own numpy copy (``optim_cases.py``) of the definition
at the top of the bf16 code in ``csrc/kernels/optim.hip``, written from the
documentation and not imported from the package."""
import functools
import math

import numpy as np
import pytest
import torch

import optim_cases
from akka_allreduce_amd.data import AllReduceOutput, Geometry, OptimGroups, sqnorm_workspace
from optim_cases import BF, H_SENTINEL, HYPER, _bits, _dev, _kernel_state, _mlp_run, _same_bits, _sr

pytestmark = pytest.mark.gpu

# one element; regions shorter than a unit; unaligned regions, no multiple of 8; few regions, so that several
# workgroups share one (gridDim.y > 1) and run the unrolled loop and its remainder
SHAPES = [(1, 1, 1), (7, 3, 2), (1003, 4, 67), (300_001, 2, 150_000)]
M_SENTINEL, V_SENTINEL = 123.0, 77.5  # bf16-representable
SEED = 5
_step = functools.partial(optim_cases._step, seed=SEED)


@functools.lru_cache(maxsize=2)
def _inputs(S, N, C, src):
    """Counts (random in [0, N], one chunk 0 where there is more than one, one N), three sums and a bf16 start
    state that is not zero, with sentinels in the count-0 elements."""
    dev = _dev()
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
    p0 = torch.randn(S, generator=g)
    m0 = torch.where(missing, torch.full((S,), M_SENTINEL), 0.1 * torch.randn(S, generator=g)).to(BF)
    v0 = torch.where(missing, torch.full((S,), V_SENTINEL), 0.01 * torch.rand(S, generator=g)).to(BF)
    torch.cuda.synchronize()
    return dict(geo=geo, pc=pc.to(dev), missing=missing.to(dev), sums=sums, p0=p0.to(dev), m0=m0.to(dev),
                v0=v0.to(dev), max_norm=0.1 * math.sqrt(S))


def _check_steps(inp, kind, S, ws_pair=(None, None), groups=None):
    """Three steps on the evolving bf16 state, each against the fp32-state kernel from the widened state."""
    adam = kind == "adamw"
    missing = inp["missing"]
    st = _kernel_state(inp)
    p, m, v, t, sh = st
    for i in range(3):
        ref = [p.clone(), m.float(), v.float(), t.clone(), sh.clone()]
        _step(inp, kind, ref, i, ws_pair[0], groups)
        _step(inp, kind, st, i, ws_pair[1], groups)
        torch.cuda.synchronize()
        assert m.dtype == BF and v.dtype == BF and int(t) == i + 1 and int(ref[3]) == i + 1
        r_m, r_v = _bits(S, i + 1, SEED)
        assert _same_bits(p, ref[0]), f"p at step {i + 1}"
        assert _same_bits(sh, ref[4]), f"shadow at step {i + 1}"
        assert torch.equal(sh[~missing], p[~missing].to(BF))
        assert _same_bits(m, _sr(ref[1], r_m)), f"m at step {i + 1}"
        if adam:
            assert _same_bits(v, _sr(ref[2], r_v)), f"v at step {i + 1}"
        else:
            assert _same_bits(v, inp["v0"])  # no second moment: untouched everywhere
        # count-0 regions: bitwise what they were
        assert torch.equal(p[missing], inp["p0"][missing])
        assert bool((m[missing].float() == M_SENTINEL).all()) and bool((v[missing].float() == V_SENTINEL).all())
        assert bool((sh[missing].float() == H_SENTINEL).all())
    if S > 1:
        assert not torch.equal(m[~missing], inp["m0"][~missing])
    return st


@pytest.mark.parametrize("kind", ["sgd", "nesterov", "adamw"])
@pytest.mark.parametrize("src", ["fp32", "bf16"])
@pytest.mark.parametrize("S,N,C", SHAPES)
def test_one_step_is_the_fp32_kernel_then_sr(S, N, C, src, kind):
    _check_steps(_inputs(S, N, C, src), kind, S)


@pytest.mark.parametrize("src", ["fp32", "bf16"])
def test_one_step_with_the_clip(src):
    S, N, C = 1003, 4, 67
    inp = _inputs(S, N, C, src)
    ws = sqnorm_workspace(_dev()), sqnorm_workspace(_dev())
    _check_steps(inp, "adamw", S, ws)
    assert torch.equal(ws[0][:2], ws[1][:2]) and float(ws[0][0]) > 0


def _rows(groups, kind, scales_and_decays):
    groups.write_rows(OptimGroups.row_values(HYPER[kind]["lr"], scales_and_decays))
    return groups


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
@pytest.mark.parametrize("S,N,C", [(1003, 4, 67), (300_001, 2, 150_000)])
def test_one_group_is_the_plain_pass(S, N, C, kind):
    inp = _inputs(S, N, C, "fp32")
    plain, grouped = _kernel_state(inp), _kernel_state(inp)
    groups = _rows(OptimGroups([S], [0], 1, _dev()), kind, [(1.0, HYPER[kind]["weight_decay"])])
    for i in range(3):
        _step(inp, kind, plain, i)
        _step(inp, kind, grouped, i, groups=groups)
    torch.cuda.synchronize()
    for name, a, b in zip(("p", "m", "v", "t", "shadow"), plain, grouped):
        assert _same_bits(a, b) if a.is_floating_point() else torch.equal(a, b), name


@pytest.mark.parametrize("src", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["sgd", "nesterov", "adamw"])
def test_groups_are_the_fp32_groups_kernel_then_sr(kind, src):
    S, N, C = 1003, 4, 67
    inp = _inputs(S, N, C, src)
    # group 1 has lr 0: its state advances and its p stays
    groups = _rows(OptimGroups([5, 130, 771, 1003], [0, 1, 0, 1], 2, _dev()), kind,
                   [(1.0, HYPER[kind]["weight_decay"]), (0.0, 0.1)])
    p, m, v, t, sh = _check_steps(inp, kind, S, groups=groups)
    still = torch.zeros(S, dtype=torch.bool, device=_dev())
    still[5:130] = still[771:] = True
    live = ~inp["missing"]
    assert torch.equal(p[still], inp["p0"][still])
    assert not torch.equal(m[still & live], inp["m0"][still & live])
    assert bool((p[~still & live] != inp["p0"][~still & live]).any())


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_the_result_does_not_depend_on_the_geometry(kind):
    """The bits are keyed by the element's index in the bucket: one region of 1003 elements and 4 blocks of
    chunks of 67 give the same p, m and v from the same sums when every count is 1."""
    S = 1003
    inp = _inputs(S, 4, 67, "fp32")
    results = []
    for N, C in ((1, 1003), (4, 67)):
        geo = Geometry(S, N, C)
        pc = torch.ones((N, geo.kmax), dtype=torch.int32, device=_dev())
        st = _kernel_state(inp)
        for i in range(3):
            _step(inp, kind, st, i, geo=geo, pc=pc)
        torch.cuda.synchronize()
        results.append(st)
    for name, a, b in zip(("p", "m", "v"), *results):
        assert _same_bits(a, b), name
    assert not _same_bits(results[0][1], inp["m0"])


@pytest.mark.parametrize("src", ["fp32", "bf16"])
def test_graph_replay_of_the_bf16_state_pass(src):
    """t.add_(1), the norm pass and the update captured once: three replays are three steps with three draws
    of bits (the key reads t on the device), bitwise the three eager calls from the same start."""
    S, N, C = 300_001, 2, 150_000
    inp = _inputs(S, N, C, src)
    dev = _dev()
    eager = _kernel_state(inp)
    ws_e = sqnorm_workspace(dev)
    for _ in range(3):
        _step(inp, "adamw", eager, 0, ws_e)
    graphed = _kernel_state(inp)
    ws_g = sqnorm_workspace(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _step(inp, "adamw", graphed, 0, ws_g)
    torch.cuda.current_stream(dev).wait_stream(side)
    for x, x0 in zip(graphed[:3], (inp["p0"], inp["m0"], inp["v0"])):
        assert _same_bits(x, x0)  # capturing ran nothing
    assert int(graphed[3]) == 0
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(graphed[3]) == 3 and int(eager[3]) == 3
    for name, a, b in zip(("p", "m", "v", "t", "shadow"), eager, graphed):
        assert _same_bits(a, b) if a.is_floating_point() else torch.equal(a, b), name
    assert torch.equal(ws_e[:2], ws_g[:2])


def _drift_run(state_dtype, S=4096, steps=1000):
    dev = _dev()
    geo = Geometry(S, 1, S)
    pc = torch.ones((1, 1), dtype=torch.int32, device=dev)
    out = AllReduceOutput(torch.ones(S, device=dev), counts_per_chunk=pc, geometry=geo)
    p = torch.zeros(S, device=dev)
    m, v = torch.zeros(S, device=dev, dtype=state_dtype), torch.zeros(S, device=dev, dtype=state_dtype)
    t = torch.zeros(1, dtype=torch.int32, device=dev)
    for _ in range(steps):
        t.add_(1)
        out.optim_step_("adamw", p, m, v, t, 1e-3, betas=(0.9, 0.999), weight_decay=0.0)
    torch.cuda.synchronize()
    return v.float().cpu()


def test_v_does_not_stall():
    """The drift case of test_bf16_state_cpu.py on the kernel, same bounds: g = 1, beta2 = 0.999, 1000 steps;
    the mean of the bf16 v over 4096 elements within 1 % of the fp32 v and above 0.5 (nearest: 0.25)."""
    v32 = _drift_run(torch.float32)
    assert bool((v32 == v32[0]).all()) and abs(float(v32[0]) - 0.6323) < 1e-3
    vbf = _drift_run(BF)
    mean = float(vbf.double().mean())
    print(f"DRIFT gpu fp32={float(v32[0]):.6f} bf16_mean={mean:.6f} rel={mean / float(v32[0]) - 1:+.3e} "
          f"worst_elem={float((vbf / v32[0] - 1).abs().max()):.3e}")
    assert mean > 0.5
    assert abs(mean - float(v32[0])) <= 0.01 * float(v32[0])


def test_non_finite_gradients_reach_m_as_they_are_and_nt_is_refused():
    dev = _dev()
    big = float(np.finfo(np.float32).max)
    x = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, big, -big, 1.0, 1e-40, -1e-40], device=dev)
    S = x.numel()
    out = AllReduceOutput(x, counts_per_chunk=torch.ones((1, 1), dtype=torch.int32, device=dev),
                          geometry=Geometry(S, 1, S))
    p, m = torch.zeros(S, device=dev), torch.zeros(S, device=dev, dtype=BF)
    t = torch.ones(1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="nt"):
        out.optim_step_("sgd", p, m, None, t, 0.1, momentum=0.0, nt=True)
    out.optim_step_("sgd", p, m, None, t, 0.1, momentum=0.0, seed=3)  # m' is the gradient itself
    torch.cuda.synchronize()
    f = m.float().cpu()
    assert bool(torch.isnan(f[0])) and float(f[1]) == float("inf") and float(f[2]) == float("-inf")
    r_m, _ = _bits(S, 1, 3)
    assert _same_bits(m[3:7], _sr(x[3:7], r_m[3:7]))  # the largest finite values round to themselves or to inf
    assert torch.equal(torch.signbit(f[4:]), torch.signbit(x[4:].cpu()))  # no sign flips
    assert not bool(torch.isnan(f[3:]).any()) and bool((f[7:].abs() <= 2e-40).all())


@pytest.mark.parametrize("wire", [False, True])
def test_graphed_mlp_step_with_bf16_state_matches_eager(wire):
    eager = _mlp_run(False, wire, state_dtype=BF)
    graphed = _mlp_run(True, wire, state_dtype=BF)
    assert eager["losses"] == graphed["losses"], (eager["losses"], graphed["losses"])
    for name in ("pflat", "sflat", "m", "v"):
        assert _same_bits(eager[name], graphed[name]), name
        assert bool(torch.isfinite(eager[name].float()).all()), name
    assert all(math.isfinite(x) for x in graphed["losses"])
    assert torch.equal(graphed["sflat"], graphed["pflat"].to(torch.bfloat16))
    assert float(graphed["v"].float().max()) > 0  # v moved
