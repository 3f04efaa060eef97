"""The region-walk kernels (``counts.hip``: ``count_expand``, ``count_mean``;
``optim.hip``: ``count_sqnorm``, ``count_optim``) where their pipelined main
loops run and where the capped grid wraps: the shapes of ``loop_cases.py``,
each guarded by the launch arithmetic mirrored there.

Inputs are ``optim_cases._inputs``: random counts in [0, N] with one chunk
forced to 0 and one to N, random normal sums -- every value depends on its
position, so a vector read from or written to the wrong place changes the
result.

``count_optim`` at depth has two oracles.  The torch criterion is in
``test_fused_optim_gpu.py`` and ``test_fused_lamb_gpu.py``.  The sharp one is
here: per element the update is one inlined function of that element's values,
and the stochastic-rounding bits depend on (index, step, seed) alone, so the
chunk geometry decides which loop touches an element and never what it gets.
``DEEP`` sends nearly every element through the two-unit pipelined loop,
``SHALLOW`` (every DEEP chunk cut in five, the counts repeated) through the
remainder loop and the scalar heads and tails; p, m, v and the shadow must
agree bit for bit.  What does depend on the geometry is the order of the two
reductions in front of the update -- the clip's squared norm and LAMB's
per-layer norms -- so both runs read ONE ``sq`` and ONE trust table, computed
once from the DEEP geometry."""
import pytest
import torch

import loop_cases as L
from akka_allreduce_amd.data import (DTYPE_NAME, AllReduceOutput, Geometry, OptimGroups, counts_table,
                                     lamb_workspace, sqnorm_workspace)
from akka_allreduce_amd.ops import count_expand
from optim_cases import BF, HYPER, _dev, _inputs, _kernel_state

pytestmark = pytest.mark.gpu

GUARD = {L.DEEP: L.require_deep, L.WRAP: L.require_wrap}
AT_DEPTH = [L.DEEP, L.WRAP]
ALPHA = -0.05


def _bits_equal(a, b):
    it = torch.int16 if a.dtype == BF else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))


# ---- count_expand --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,N,C", AT_DEPTH)
def test_count_expand_at_depth(S, N, C):
    GUARD[(S, N, C)]()
    g = Geometry(S, N, C)
    per = torch.randint(0, 9, (N, g.kmax), dtype=torch.int32, generator=torch.Generator().manual_seed(S + C))
    want = g.expand_counts(per)
    got = count_expand(per.cuda(), g).cpu()
    assert torch.equal(got, want)


# ---- count_mean ----------------------------------------------------------------------------------------------------------
def _mean_want(x, count, dtype):
    c = count.to(dtype)
    return torch.where(c > 0, x.to(dtype) / c.clamp(min=1), torch.zeros_like(c))


@pytest.mark.parametrize("variant", ["fp32", "bf16", "bf16 into fp32"])
@pytest.mark.parametrize("S,N,C", AT_DEPTH)
def test_count_mean_at_depth(S, N, C, variant):
    """``mean()``, ``mean(out=buf)`` and the in-place ``mean(out=data)`` against torch's expression."""
    GUARD[(S, N, C)]()
    inp = _inputs(S, N, C, "fp32" if variant == "fp32" else "bf16")
    x = inp["sums"][0].clone()
    o = AllReduceOutput(x, counts_per_chunk=inp["pc"], geometry=inp["geo"])
    if variant == "bf16 into fp32":
        want = _mean_want(x, inp["count"], torch.float32)
        assert torch.equal(o.mean(dtype=torch.float32), want)
        buf = torch.full((S,), 7.0, device=_dev())
        assert o.mean(out=buf, dtype=torch.float32) is buf and torch.equal(buf, want)
        return
    want = _mean_want(x, inp["count"], x.dtype)
    assert torch.equal(o.mean(), want)
    buf = torch.full_like(x, 7.0)
    assert o.mean(out=buf) is buf and torch.equal(buf, want)
    assert o.mean(out=x) is x and torch.equal(x, want)  # the reduced buffer averaged in place
    assert bool((want[inp["missing"]] == 0).all()) and bool((want != 0).any())


@pytest.mark.parametrize("src", ["fp32", "bf16"])
@pytest.mark.parametrize("S,N,C", AT_DEPTH)
def test_count_mean_axpy_at_depth(S, N, C, src):
    """``y += alpha * mean`` (bf16 sum: the mixed pass into fp32 ``y``), alone and with the bf16 shadow.

    The two agree bit for bit and the shadow is ``bf16(y)``, as in
    ``test_count_mean_shadow_is_bf16_of_updated_params``.  Against float64: ``alpha * m`` is exact there (two
    24-bit factors) and the sum is rounded to 53 bits, so the kernel's fp32 result -- one rounding with a fused
    multiply-add, two without -- lies within ``2**-24 * (|alpha * m| + |y|)`` of it, whichever the compiler chose;
    the bound below is twice that, which covers ``|y|`` against the reference's own ``|y|``.  An element from the
    wrong vector is off by the order of the data itself."""
    GUARD[(S, N, C)]()
    inp = _inputs(S, N, C, src)
    d = inp["sums"][0]
    wide = src == "bf16"
    y0 = inp["p0"]
    mean = _mean_want(d, inp["count"], torch.float32)  # fp32 mean of the sum: exact operands of the update
    plain = AllReduceOutput(d, counts_per_chunk=inp["pc"], geometry=inp["geo"]).axpy_mean_(y0.clone(), ALPHA, wide=wide)
    y = y0.clone()
    shadow = torch.full((S,), 7.0, device=_dev(), dtype=BF)
    AllReduceOutput(d, counts_per_chunk=inp["pc"], geometry=inp["geo"]).axpy_mean_(y, ALPHA, shadow=shadow, wide=wide)
    torch.cuda.synchronize()
    assert torch.equal(y, plain)  # the fp32 update is unchanged by the extra store
    assert torch.equal(shadow, y.to(BF))  # RNE, as torch's cast
    alpha = float(torch.tensor(ALPHA, dtype=torch.float32))  # the kernel's argument is a float
    step = alpha * mean.double()
    want = y0.double() + step
    bound = 2.0 ** -23 * (step.abs() + want.abs())
    worst = float(((y.double() - want).abs() - bound).max())
    assert worst <= 0, worst
    assert torch.equal(y[inp["missing"]], y0[inp["missing"]]) and not torch.equal(y, y0)


# ---- count_sqnorm --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["fp32", "bf16"])
@pytest.mark.parametrize("S,N,C", AT_DEPTH)
def test_sqnorm_at_depth(S, N, C, src):
    GUARD[(S, N, C)]()
    inp = _inputs(S, N, C, src)
    ws = sqnorm_workspace(_dev())
    out = AllReduceOutput(inp["sums"][0], counts_per_chunk=inp["pc"], geometry=inp["geo"])
    got = [out.sqnorm(ws).clone() for _ in range(3)]
    c = inp["count"].double()
    mean64 = torch.where(c > 0, inp["sums"][0].double() / c.clamp(min=1), torch.zeros_like(c))
    want = float((mean64 * mean64).sum())
    torch.cuda.synchronize()
    # The longest add chain of one thread, recounted from count_sqnorm_kernel for these shapes.  DEEP: one region per
    # workgroup (no wrap); a thread adds at most one head and one tail element and 4 elements for each of its
    # ceil(2348 / 256) = 10 fp32 vectors (8 for each of 5 bf16 ones): 42; block_sum 6 + 3; the last workgroup adds
    # ceil(1035 / 256) = 5 partials per thread and 6 + 3 again: 65.  WRAP: two regions of 37 elements per workgroup
    # at the most, per region one head, one tail and one vector of a thread: 2 x (1 + 1 + 8) = 20; 9; 2048 / 256 =
    # 8 partials; 9: 46.  Non-negative terms, chains < 100: relative error <= 100 * 2**-24 < 1e-5, the bound of
    # test_sqnorm_matches_float64_and_is_deterministic.
    print(f"SQNORM S={S} C={C} src={src} got={float(got[0]):.9e} want={want:.9e} rel={abs(float(got[0]) - want) / want:.3e}")
    assert abs(float(got[0]) - want) <= 1e-5 * want, (float(got[0]), want)
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])  # the ticket re-arms
    assert float(ws[1]) == 0.0


# ---- count_optim: one geometry against another ---------------------------------------------------------------------------
KINDS = {**HYPER, "lamb": dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)}
GROUP_SCALE, GROUP_WD = (1.0, 0.1, 2.5), (0.01, 0.0, 0.1)  # round-robin over the segments: neighbours differ
SEED = 5


def _native():
    from akka_allreduce_amd._native_loader import load

    return load()


def _groups(kind, cuts):
    g = OptimGroups(cuts, [i % 3 for i in range(len(cuts))], 3, _dev())
    g.write_rows(OptimGroups.row_values(KINDS[kind]["lr"], list(zip(GROUP_SCALE, GROUP_WD))))
    return g


def _group_args(g):
    return (g.seg_end.data_ptr(), g.seg_group.data_ptr(), g.rows.data_ptr(), g.host_seg_end, g.host_seg_group,
            g.ngroups)


def _start(inp, state):
    """[p, m, v, t, shadow]: fp32 everything; bf16 moments; bf16 moments and parameters (no shadow then)."""
    st = _kernel_state(inp, shadow=state != "bf16 p", dtype=None if state == "fp32" else BF)
    if state == "bf16 p":
        st[0] = st[0].to(BF)
    return st


def _hyper_args(kind, st, groups, sq, max_norm):
    h = KINDS[kind]
    b1, b2 = h.get("betas", (0.9, 0.999))
    kw = dict(beta1=b1, beta2=b2, eps=h.get("eps", 1e-8), max_norm=max_norm if sq is not None else 0.0,
              state_dtype=DTYPE_NAME[st[1].dtype])
    if st[0].dtype == BF:
        kw["param_dtype"] = DTYPE_NAME[BF]
    return kw


def _trust(kind, st, src, geo, pc, groups, sq, max_norm, lamb):
    """LAMB's two norm kernels from the state in front of the step: the ratios land in ``lamb["trust"]``."""
    p, m, v, t, _ = st
    keep, table = counts_table(pc, geo)
    stream = torch.cuda.current_stream().cuda_stream
    ws = lamb["ws"]
    _native().lamb_norms(ws.data_ptr(), ws.numel() // 2, p.data_ptr(), m.data_ptr(), v.data_ptr(), src.data_ptr(),
                         DTYPE_NAME[src.dtype], table, t.data_ptr(), sq.data_ptr() if sq is not None else 0,
                         _group_args(groups), stream, **_hyper_args(kind, st, groups, sq, max_norm))
    _native().lamb_trust(lamb["trust"].data_ptr(), ws.data_ptr(), ws.numel() // 2, _group_args(groups), p.numel(),
                         lamb["adapt"].data_ptr(), stream)


def _update(kind, st, src, geo, pc, groups, sq, max_norm, trust):
    """The update pass alone (``count_optim``) through the geometry ``geo`` with the counts ``pc``; ``sq`` and
    ``trust``: the squared norm and the ratios it reads, whoever computed them."""
    p, m, v, t, sh = st
    h = KINDS[kind]
    adam = kind in ("adamw", "lamb")
    keep, table = counts_table(pc, geo)
    kw = _hyper_args(kind, st, groups, sq, max_norm)
    if groups is None:
        kw.update(lr=h["lr"], weight_decay=h["weight_decay"])
    _native().count_optim(kind if adam else "sgd", p.data_ptr(), m.data_ptr(), v.data_ptr() if adam else 0,
                          sh.data_ptr() if sh is not None else 0, src.data_ptr(), DTYPE_NAME[src.dtype], table,
                          t.data_ptr(), sq.data_ptr() if sq is not None else 0,
                          torch.cuda.current_stream().cuda_stream, False, momentum=h.get("momentum", 0.0),
                          nesterov=h.get("nesterov", False), seed=SEED,
                          groups=None if groups is None else _group_args(groups),
                          trust=trust.data_ptr() if trust is not None else 0, **kw)


# the topmost parameter varies fastest: every case of a source dtype shares its inputs
@pytest.mark.parametrize("mode", ["plain", "clip", "clip+groups"])
@pytest.mark.parametrize("state", ["fp32", "bf16", "bf16 p"])
@pytest.mark.parametrize("kind", ["sgd", "nesterov", "adamw", "lamb"])
@pytest.mark.parametrize("src", ["fp32", "bf16"])
def test_update_through_deep_and_shallow_is_bitwise_the_same(src, kind, state, mode):
    L.require_deep()
    L.require_shallow()
    S, N, C = L.DEEP
    inp = _inputs(S, N, C, src)
    deep = (inp["geo"], inp["pc"])
    shallow = (Geometry(*L.SHALLOW), L.shallow_counts(inp["pc"]))
    assert shallow[1].shape == (N, shallow[0].kmax)
    clip = mode != "plain"
    cuts = L.DEEP_CUTS if mode == "clip+groups" else (S,)
    if len(cuts) > 1:
        L.require_deep_cuts(cuts)
    groups = _groups(kind, cuts) if (len(cuts) > 1 or kind == "lamb") else None  # LAMB: layers, one at the least
    lamb = None
    if kind == "lamb":
        lamb = dict(trust=torch.full((len(cuts),), -7.0, device=_dev()), ws=lamb_workspace(S, len(cuts), _dev()),
                    adapt=torch.tensor([i % 3 != 1 for i in range(len(cuts))], dtype=torch.int32, device=_dev()))
    a, b = _start(inp, state), _start(inp, state)
    start = [x.clone() for x in a[:3]]
    ws = sqnorm_workspace(_dev())
    missing = inp["missing"]
    names = ("p", "m", "v", "t", "shadow")
    for i in range(3):
        sum_i = inp["sums"][i]
        sq = AllReduceOutput(sum_i, counts_per_chunk=deep[1], geometry=deep[0]).sqnorm(ws) if clip else None
        a[3].add_(1)
        b[3].add_(1)
        if lamb is not None:
            _trust(kind, a, sum_i, *deep, groups, sq, inp["max_norm"], lamb)
        trust = lamb["trust"] if lamb is not None else None
        _update(kind, a, sum_i, *deep, groups, sq, inp["max_norm"], trust)
        _update(kind, b, sum_i, *shallow, groups, sq, inp["max_norm"], trust)
        if i + 1 not in (1, 3):
            continue
        torch.cuda.synchronize()
        for name, x, y in zip(names, a, b):
            if x is not None and not (name == "v" and kind in ("sgd", "nesterov")):
                assert _bits_equal(x, y), f"{name} after {i + 1} step(s)"
        # the step moved what has a contributor and nothing else
        for name, x, x0 in zip("pmv", a[:3], start):
            if name == "v" and kind in ("sgd", "nesterov"):
                assert _bits_equal(x, x0)  # no second moment: untouched everywhere
                continue
            assert _bits_equal(x[missing], x0.to(x.dtype)[missing]), name
            assert not _bits_equal(x[~missing], x0.to(x.dtype)[~missing]), name
        if lamb is not None:
            r = lamb["trust"].tolist()
            assert all(x > 0 for x in r) and (len(r) == 1 or any(x != 1.0 for x in r)), r
            assert all(r[j] == 1.0 for j in range(len(r)) if j % 3 == 1)  # the opted-out layers
