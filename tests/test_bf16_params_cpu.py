"""bf16 parameters in the fused optimizers on the CPU: the torch path of
``optim_step_`` against the definition (README, "bf16 parameters"), the fixed
points, missing chunks and the guard, the stall a nearest rounding would show,
the optimizers' interface and a small training run.

``_bits_p`` / ``_sr`` are the tests' own copy of the definition
(``bf16_param_cases.py`` / ``optim_cases.py``); nothing of it is imported from
the package."""
import copy
import math

import pytest
import torch

from akka_allreduce_amd.data import AllReduceOutput, Geometry
from akka_allreduce_amd.parallel import FusedAdamW, FusedLAMB, FusedSGD
from akka_allreduce_amd.parallel.dp import GradientBucket
from bf16_param_cases import (M_SENTINEL, P_SENTINEL, V_SENTINEL, Opts, _bits_p, check_stall, check_steps,
                              make_inputs, stall_run, start_state)
from optim_cases import BF, _same_bits

SHAPES = [(7, 3, 2), (1003, 4, 67)]
OPTIONS = {"plain": {}, "groups": dict(grouped=True), "clip": dict(clip=True), "guard": dict(guard=True),
           "all": dict(grouped=True, clip=True, guard=True)}


# ---- 1. one step against the definition ----------------------------------------------------------------------------
@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("src", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["sgd", "nesterov", "adamw", "lamb"])
@pytest.mark.parametrize("S,N,C", SHAPES)
def test_torch_path_is_the_fp32_p_path_then_sr(S, N, C, kind, src, option):
    check_steps(Opts(kind, make_inputs(S, N, C, src, "cpu"), **OPTIONS[option]))


def test_the_second_hash_is_not_the_first():
    """r_p is a stream of its own: it agrees with r_m and with r_v in about 1 of 65536 elements, its bits are
    fair, and the package's ``sr_bits_p`` is the definition."""
    from akka_allreduce_amd.data import sr_bits_p
    from optim_cases import _bits

    n = 1 << 16
    for t, seed in ((1, 0), (2, 0), (1, 7)):
        r_p = _bits_p(n, t, seed)
        r_m, r_v = _bits(n, t, seed)
        assert int((r_p == r_m).sum()) < 16 and int((r_p == r_v).sum()) < 16
        assert abs(float(r_p.mean()) / 65536 - 0.5) < 0.01
        got = sr_bits_p(n, torch.tensor([t]), seed)
        assert got.tolist() == r_p.tolist()
    assert _bits_p(n, 1, 0).tolist() != _bits_p(n, 2, 0).tolist()


# ---- 2. fixed points -----------------------------------------------------------------------------------------------
def test_a_zero_update_keeps_p_bitwise():
    S, N, C = 1003, 4, 67
    inp = make_inputs(S, N, C, "fp32", "cpu")
    p, m, v, t = start_state(inp)
    p0 = p.clone()
    out = AllReduceOutput(torch.zeros(S), counts_per_chunk=inp["pc"], geometry=inp["geo"])
    m.zero_()
    for _ in range(3):
        t.add_(1)
        out.optim_step_("sgd", p, m, None, t, 0.05, momentum=0.0, weight_decay=0.0, seed=3)
    assert _same_bits(p, p0)


@pytest.mark.parametrize("kind", ["sgd", "adamw", "lamb"])
def test_a_group_at_lr_zero_keeps_p_bitwise_and_advances_the_state(kind):
    S, N, C = 1003, 4, 67
    inp = make_inputs(S, N, C, "fp32", "cpu")
    o = Opts(kind, inp, grouped=True, group1=(0.0, 0.1))
    (p, m, v, t), _ = check_steps(o)
    still = torch.zeros(S, dtype=torch.bool)
    still[5:130] = still[771:] = True
    live = ~inp["missing"]
    assert _same_bits(p[still], inp["p0"][still])
    assert not _same_bits(m[still & live], inp["m0"][still & live])
    if o.adam:
        assert not _same_bits(v[still & live], inp["v0"][still & live])
    assert bool((p[~still & live] != inp["p0"][~still & live]).any())


# ---- 3. missing chunks and the guard -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sgd", "adamw", "lamb"])
def test_all_chunks_missing_keeps_everything(kind):
    S, N, C = 1003, 4, 67
    inp = dict(make_inputs(S, N, C, "fp32", "cpu"))
    inp["pc"] = torch.zeros_like(inp["pc"])
    o = Opts(kind, inp)
    st = start_state(inp)
    before = [x.clone() for x in st]
    o.step(o.buffers(), st, 0)
    for name, a, b in zip("pmv", st, before):
        assert _same_bits(a, b), name
    assert int(st[3]) == 1


@pytest.mark.parametrize("kind", ["sgd", "adamw", "lamb"])
def test_a_nan_in_a_contributing_chunk_leaves_everything_bitwise(kind):
    S, N, C = 1003, 4, 67
    inp = make_inputs(S, N, C, "fp32", "cpu")
    o = Opts(kind, inp, clip=True, guard=True)
    st, bufs = check_steps(o, steps=1)
    before = [x.clone() for x in st]
    trust = bufs["lamb"]["trust"].clone() if kind == "lamb" else None
    bad = inp["sums"][1].clone()
    bad[(~inp["missing"]).nonzero().flatten()[17]] = math.nan
    o.step(bufs, st, 1, src=bad)
    assert bufs["guard"].tolist() == [0, 1, 1, 0]
    for name, a, b in zip("pmvt", st, before):
        assert _same_bits(a, b) if a.is_floating_point() else torch.equal(a, b), name
    if trust is not None:
        assert _same_bits(bufs["lamb"]["trust"], trust)
    # a NaN inside a count-0 chunk is never read
    quiet = inp["sums"][2].clone()
    quiet[inp["missing"].nonzero().flatten()[0]] = math.nan
    o.step(bufs, st, 2, src=quiet)
    assert bufs["guard"].tolist() == [1, 1, 0, 0] and int(st[3]) == 2
    assert bool(torch.isfinite(st[0].float()).all())
    missing = inp["missing"]
    assert bool((st[0][missing].float() == P_SENTINEL).all()) and bool((st[1][missing].float() == M_SENTINEL).all())
    assert bool((st[2][missing].float() == V_SENTINEL).all())


# ---- 4. the stall, and its cure ------------------------------------------------------------------------------------
def test_p_does_not_stall():
    """S = 4096, p0 = 1, a gradient of 1, plain SGD at lr = 1e-4 for 1000 steps, seed 0.  Every stored p stays
    in [0.5, 1], where a bf16 ulp is 2^-8, so a step moves an element one ulp down with probability
    1e-4 / 2^-8 = 0.0256, unbiasedly: after 1000 steps the expectation is 0.9, the standard deviation of one
    element 2^-8 * sqrt(1000 * 0.0256 * 0.9744) = 0.0195 and that of the mean of 4096 elements 3.1e-4.  The
    bound on the mean is 2e-3 (6.5 standard deviations); nearest rounding gives exactly 1.0.  No element may
    be outside 0.9 +- 0.15 (7.7 standard deviations).

    Observed (the bits are deterministic: the kernel must give the same): mean 0.9000749588012695 (exact in
    float64: every p is a multiple of 2^-8), min 0.83203125, max 0.953125."""
    p = stall_run("cpu")
    assert p.dtype == BF
    mean = check_stall(p)
    assert mean == OBSERVED_MEAN, mean
    # what nearest rounding does: the fp32 result 1 - 1e-4 rounds back to 1
    assert float((torch.ones(1) - 1e-4).to(BF)) == 1.0


OBSERVED_MEAN = 0.9000749588012695


# ---- 5. constructor and validation errors --------------------------------------------------------------------------
def _bf_bucket(sizes=(640, 60, 300, 3), grads=BF):
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(n).to(BF)) for n in sizes]
    return GradientBucket(ps, dtype=grads, flatten_params=True)


class _OneContributor:
    def __init__(self, S, C=64):
        self.geometry = Geometry(S, 1, C)
        self.counts = torch.ones((1, self.geometry.kmax), dtype=torch.int32)

    def __call__(self, t, out=None):
        return AllReduceOutput(t.clone(), counts_per_chunk=self.counts, geometry=self.geometry)


def test_constructor_errors():
    for cls in (FusedSGD, FusedAdamW, FusedLAMB):
        with pytest.raises(ValueError, match=r"state_dtype=torch\.bfloat16"):
            cls(_bf_bucket())  # the default state_dtype stays float32
        with pytest.raises(ValueError, match=r"state_dtype=torch\.bfloat16"):
            cls(_bf_bucket(), state_dtype=torch.float32)
        opt = cls(_bf_bucket(), state_dtype=BF)
        assert opt.param_dtype == BF and opt.m.dtype == BF and opt.bucket.pflat.dtype == BF
        with pytest.raises(AttributeError):
            opt.param_dtype = torch.float32
    # a bucket whose two flat buffers differ in dtype is refused, either way round
    from optim_cases import _bucket

    b = _bf_bucket()
    b.flat = b.flat.float()
    with pytest.raises(ValueError, match="not a mix"):
        FusedAdamW(b, state_dtype=BF)
    b = _bucket()
    b.flat = b.flat.to(BF)
    with pytest.raises(ValueError, match="not a mix"):
        FusedAdamW(b, state_dtype=BF)
    b = _bf_bucket()
    assert b.use_shadow(BF) is False and b.sflat is None  # the parameter is the bf16 weight: no shadow


def test_optim_step_refusals():
    S = 16
    out = AllReduceOutput(torch.ones(S), counts_per_chunk=torch.ones((1, 1), dtype=torch.int32),
                          geometry=Geometry(S, 1, S))
    p, t = torch.ones(S, dtype=BF), torch.ones(1, dtype=torch.int32)
    bf = lambda: torch.zeros(S, dtype=BF)  # noqa: E731
    with pytest.raises(ValueError, match="bfloat16 m and v"):
        out.optim_step_("sgd", p, torch.zeros(S), None, t, 1e-3)
    with pytest.raises(ValueError, match="bfloat16 m and v"):
        out.optim_step_("adamw", p, torch.zeros(S), torch.zeros(S), t, 1e-3)
    with pytest.raises(ValueError, match="shadow"):
        out.optim_step_("adamw", p, bf(), bf(), t, 1e-3, shadow=bf())
    with pytest.raises(ValueError, match="nt"):
        out.optim_step_("sgd", p, bf(), None, t, 1e-3, nt=True)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        out.optim_step_("sgd", p.to(torch.float16), bf(), None, t, 1e-3)
    assert torch.equal(p, torch.ones(S, dtype=BF))


@pytest.mark.parametrize("cls", [FusedSGD, FusedAdamW, FusedLAMB])
def test_state_dict_round_trip_and_param_dtype(cls):
    def steps(b, opt, ar, which):
        for i in which:
            b.flat.copy_(torch.randn(b.numel, generator=torch.Generator().manual_seed(100 + i)))
            opt.step_from(ar, 1e-2)

    b1 = _bf_bucket()
    o1, ar = cls(b1, state_dtype=BF, seed=9), _OneContributor(b1.numel)
    steps(b1, o1, ar, range(3))
    saved, p_saved = o1.state_dict(), b1.pflat.clone()
    assert saved["param_dtype"] == BF and saved["state_dtype"] == BF
    steps(b1, o1, ar, range(3, 5))
    assert not _same_bits(b1.pflat, p_saved)
    # the run continues bit for bit, nothing moves
    b2 = _bf_bucket()
    o2 = cls(b2, state_dtype=BF, seed=9)
    with torch.no_grad():
        b2.pflat.copy_(p_saved)
    ptrs = o2.state_pointers()
    o2.load_state_dict(saved)
    assert o2.state_pointers() == ptrs and int(o2.t) == 3
    steps(b2, o2, ar, range(3, 5))
    assert _same_bits(b1.pflat, b2.pflat) and _same_bits(o1.m, o2.m)
    # another param_dtype is refused, either way
    from optim_cases import _bucket

    with pytest.raises(ValueError, match="param_dtype"):
        cls(_bucket(), state_dtype=BF, seed=9).load_state_dict(saved)
    o32 = cls(_bucket(), state_dtype=BF, seed=9)
    d32 = o32.state_dict()
    assert d32["param_dtype"] == torch.float32 and o32.param_dtype == torch.float32
    with pytest.raises(ValueError, match="param_dtype"):
        cls(_bf_bucket(), state_dtype=BF, seed=9).load_state_dict(d32)
    # a dict from before the key existed counts as float32
    old = {k: x for k, x in d32.items() if k != "param_dtype"}
    cls(_bucket(), state_dtype=BF, seed=9).load_state_dict(old)
    with pytest.raises(ValueError, match="param_dtype"):
        cls(_bf_bucket(), state_dtype=BF, seed=9).load_state_dict(old)


# ---- 6. a small training run ---------------------------------------------------------------------------------------
def test_a_bf16_model_trains_and_equals_the_hand_rolled_loop():
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 4)).to(BF)
    twin = copy.deepcopy(model)
    x = torch.randn(64, 16).to(BF)
    y = torch.randint(0, 4, (64,), generator=torch.Generator().manual_seed(1))
    lr, wd, seed = 1e-2, 0.01, 4
    bucket = GradientBucket(list(model.parameters()), flatten_params=True)
    assert bucket.pflat.dtype == BF and bucket.flat.dtype == BF
    opt = FusedAdamW(bucket, weight_decay=wd, state_dtype=BF, seed=seed)
    losses = []
    for _ in range(30):
        bucket.zero_()
        loss = torch.nn.functional.cross_entropy(model(x).float(), y)
        loss.backward()
        losses.append(float(loss.detach()))
        assert opt.step_from(None, lr) is None
    assert int(opt.t) == 30 and losses[-1] < 0.7 * losses[0], losses
    assert bucket.params_bound() and all(p.dtype == BF for p in model.parameters())

    # the same run by hand: the gradients flattened, one optim_step_ per step on flat copies
    params = list(twin.parameters())
    n = sum(p.numel() for p in params)
    pf = torch.cat([p.detach().reshape(-1) for p in params]).clone()
    m, v, t = torch.zeros(n, dtype=BF), torch.zeros(n, dtype=BF), torch.zeros(1, dtype=torch.int32)
    ones, geo = torch.ones((1, 1), dtype=torch.int32), Geometry(n, 1, n)
    for _ in range(30):
        for p in params:
            p.grad = None
        torch.nn.functional.cross_entropy(twin(x).float(), y).backward()
        g = torch.cat([p.grad.reshape(-1) for p in params])
        t.add_(1)
        AllReduceOutput(g, counts_per_chunk=ones, geometry=geo).optim_step_(
            "adamw", pf, m, v, t, lr, weight_decay=wd, seed=seed)
        off = 0
        with torch.no_grad():
            for p in params:
                p.copy_(pf[off:off + p.numel()].view_as(p))
                off += p.numel()
    assert _same_bits(bucket.pflat, pf) and _same_bits(opt.m, m) and _same_bits(opt.v, v)
