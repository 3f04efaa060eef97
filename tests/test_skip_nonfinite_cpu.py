"""``skip_nonfinite=True`` of FusedSGD / FusedAdamW on the CPU path: a step
whose gradient is not finite (judged by the squared global norm of the round's
mean gradient) leaves parameters, moments, shadow and the step ``t`` bit for
bit as they were and is counted in the guard's record; a run with a skipped
step continues exactly as a run in which that round never happened.  Every
comparison is bitwise."""
import pytest
import torch

from akka_allreduce_amd.data import guard_state, sqnorm_workspace
from akka_allreduce_amd.parallel import FusedAdamW, FusedSGD
from akka_allreduce_amd.parallel.dp import GradientBucket
from optim_cases import BF, H_SENTINEL, StubAllreduce, _bucket, _same_bits

S, N, C = 1003, 4, 67
KINDS = ["sgd", "nesterov", "adamw"]
POISON = {"+inf": float("inf"), "-inf": float("-inf"), "nan": float("nan"), "2e19": 2e19}


def _opt(b, kind, guard, clip=None, bf_state=False, groups=False):
    kw = dict(max_grad_norm=clip, state_dtype=BF if bf_state else torch.float32, seed=3)
    if guard is not None:  # None: the keyword is not passed at all
        kw["skip_nonfinite"] = guard
    if groups:
        kw["param_groups"] = [{"params": [b.params[1], b.params[3]], "weight_decay": 0.0, "lr_scale": 0.5}]
    if kind == "adamw":
        return FusedAdamW(b, weight_decay=0.01, **kw), 1e-3
    return FusedSGD(b, momentum=0.9, nesterov=kind == "nesterov", weight_decay=1e-2, **kw), 0.05


def _setup(kind, guard, **kw):
    """Bucket, optimizer, learning rate and round; the bucket gets a shadow of sentinels (the bucket itself
    keeps one on the GPU only, the CPU path of the pass writes whichever it is handed)."""
    b = _bucket()
    assert b.numel == S
    opt, lr = _opt(b, kind, guard, **kw)
    b.sflat = torch.full((S,), H_SENTINEL, dtype=BF)
    b._shadow_on = True
    return b, opt, lr, StubAllreduce(S, N, C)


def _grads(n, seed=7):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(S, generator=gen) for _ in range(n)]


def _state(b, opt):
    return [x.clone() for x in (b.pflat, opt.m, opt.v, b.sflat, opt.t) if x is not None]


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert _same_bits(g, w), f"{what}: buffer {i} differs"


def _run(kind, guard, grads, **kw):
    b, opt, lr, ar = _setup(kind, guard, **kw)
    for g in grads:
        b.flat.copy_(g)
        opt.step_from(ar, lr)
    return b, opt


@pytest.mark.parametrize("groups", [False, True])
@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("bf_state", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_guard_on_equals_guard_off_over_finite_rounds(kind, bf_state, clip, groups):
    grads = _grads(3)
    b0, o0 = _run(kind, None, grads, clip=clip, bf_state=bf_state, groups=groups)
    b1, o1 = _run(kind, True, grads, clip=clip, bf_state=bf_state, groups=groups)
    assert o0.guard is None and (o0.norm_ws is None) == (clip is None)
    assert o1.norm_ws is not None and o1.guard.tolist() == [1, 0, 0, 0]
    assert int(o1.t) == 3 and o1.last_step_applied and o1.skipped_steps == 0 and o1.skipped_in_a_row == 0
    _assert_same(_state(b1, o1), _state(b0, o0), "guard on against guard off")
    assert bool((b1.sflat != H_SENTINEL).any())  # the shadow was written
    # the norm the pass left, without a sync of its own
    assert o1.grad_norm().shape == () and _same_bits(o1.grad_norm(), o1.norm_ws[0].sqrt())
    if clip is not None:
        assert _same_bits(o0.grad_norm(), o1.grad_norm())


@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("bf_state", [False, True])
@pytest.mark.parametrize("value", list(POISON))
@pytest.mark.parametrize("kind", KINDS)
def test_poisoned_round_is_skipped_and_the_run_goes_on_as_if_it_never_happened(kind, value, bf_state, clip):
    g0, bad, g2 = _grads(3)
    b, opt, lr, ar = _setup(kind, True, clip=clip, bf_state=bf_state)
    at = int((ar.count > 0).nonzero()[17])
    bad = bad.clone()
    bad[at] = POISON[value]
    b.flat.copy_(g0)
    opt.step_from(ar, lr)
    before = _state(b, opt)
    assert int(opt.t) == 1
    b.flat.copy_(bad)
    opt.step_from(ar, lr)
    assert not bool(torch.isfinite(opt.norm_ws[0]))
    _assert_same(_state(b, opt), before, "after the skipped step")
    assert opt.guard.tolist() == [0, 1, 1, 0]
    assert not opt.last_step_applied and opt.skipped_steps == 1 and opt.skipped_in_a_row == 1
    b.flat.copy_(g2)
    opt.step_from(ar, lr)
    assert opt.guard.tolist() == [1, 1, 0, 0] and int(opt.t) == 2
    ref_b, ref_o = _run(kind, None, [g0, g2], clip=clip, bf_state=bf_state)
    _assert_same(_state(b, opt), _state(ref_b, ref_o), "against the run without the bad round")


@pytest.mark.parametrize("value", ["+inf", "nan"])
@pytest.mark.parametrize("kind", KINDS)
def test_nonfinite_value_in_a_count_0_chunk_skips_nothing(kind, value):
    g0, g1 = _grads(2)

    def run(poison):
        b, opt, lr, ar = _setup(kind, True, clip=1.0)
        at = int((ar.count == 0).nonzero()[5])

        def round_(t, out=None):
            o = ar(t)
            if poison:
                o.data[at] = POISON[value]  # inside the sum, where no contributor reached
            return o

        for g in (g0, g1):
            b.flat.copy_(g)
            opt.step_from(round_, lr)
        return b, opt

    b, opt = run(True)
    assert opt.guard.tolist() == [1, 0, 0, 0] and int(opt.t) == 2
    ref_b, ref_o = run(False)
    _assert_same(_state(b, opt), _state(ref_b, ref_o), "a count-0 chunk is never read")


def test_a_round_with_every_count_0_is_applied_and_changes_only_t():
    b, opt, lr, ar = _setup("adamw", True)
    ar.counts.zero_()
    ar.count.zero_()
    b.flat.copy_(_grads(1)[0])
    before = _state(b, opt)
    opt.step_from(ar, lr)
    assert float(opt.norm_ws[0]) == 0.0 and opt.guard.tolist() == [1, 0, 0, 0] and int(opt.t) == 1
    _assert_same(_state(b, opt)[:-1], before[:-1], "every chunk missing")


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_state_dict_round_trip_carries_the_record(kind):
    g0, bad, g2 = _grads(3)
    bad = bad.clone()
    b, opt, lr, ar = _setup(kind, True, clip=1.0)
    bad[int((ar.count > 0).nonzero()[0])] = float("nan")
    for g in (g0, bad):
        b.flat.copy_(g)
        opt.step_from(ar, lr)
    d = opt.state_dict()
    assert d["skip_nonfinite"] is True and d["guard"] == [0, 1, 1, 0] and d["t"] == 1
    b2, opt2, _, _ = _setup(kind, True, clip=1.0)
    ptr = opt2.guard.data_ptr()
    opt2.load_state_dict(d)
    assert opt2.guard.data_ptr() == ptr and opt2.guard.tolist() == [0, 1, 1, 0] and int(opt2.t) == 1
    with torch.no_grad():
        b2.pflat.copy_(b.pflat)
    b2.sflat.copy_(b.sflat)
    for bb, oo in ((b, opt), (b2, opt2)):
        bb.flat.copy_(g2)
        oo.step_from(ar, lr)
    assert opt2.guard.tolist() == [1, 1, 0, 0]
    _assert_same(_state(b2, opt2), _state(b, opt), "after the round trip")


def test_load_state_dict_accepts_an_older_dict_and_refuses_a_mismatch():
    _, off, _, _ = _setup("adamw", None)
    _, on, _, _ = _setup("adamw", True)
    old = off.state_dict()
    assert old["skip_nonfinite"] is False and old["guard"] is None
    del old["skip_nonfinite"], old["guard"]  # as saved before the guard existed
    off.load_state_dict(old)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        on.load_state_dict(old)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        off.load_state_dict(on.state_dict())
    # a guard-on dict without a record: zero counters
    on.guard.copy_(torch.tensor([0, 5, 2, 0], dtype=torch.int32))
    d = on.state_dict()
    assert d["guard"] == [0, 5, 2, 0]
    d["guard"] = None
    on.load_state_dict(d)
    assert on.guard.tolist() == [0, 0, 0, 0]


def test_constructor_and_argument_errors():
    ps = [torch.nn.Parameter(torch.randn(8))]
    for cls in (FusedSGD, FusedAdamW):
        with pytest.raises(ValueError, match="skip_nonfinite"):
            cls(GradientBucket(ps, flatten_params=True), skip_nonfinite="yes")
        with pytest.raises(ValueError, match="skip_nonfinite"):
            cls(GradientBucket(ps, flatten_params=True), skip_nonfinite=1)
        plain = cls(GradientBucket(ps, flatten_params=True))
        assert plain.skip_nonfinite is False and plain.guard is None and plain.norm_ws is None
        for prop in ("skipped_steps", "skipped_in_a_row", "last_step_applied"):
            with pytest.raises(RuntimeError, match="skip_nonfinite"):
                getattr(plain, prop)
        with pytest.raises(RuntimeError, match="norm pass"):
            plain.grad_norm()
        on = cls(GradientBucket(ps, flatten_params=True), skip_nonfinite=True)
        assert on.guard.dtype == torch.int32 and on.guard.tolist() == [0, 0, 0, 0] and on.norm_ws is not None
        assert on.guard.data_ptr() in on.state_pointers() and any(x is on.guard for x in on.state_tensors())
    # FusedSGD(momentum=0, skip_nonfinite=True): the guarded plain SGD
    assert FusedSGD(GradientBucket(ps, flatten_params=True), momentum=0.0, skip_nonfinite=True).guard is not None
    ar = StubAllreduce(S, N, C)
    out = ar(torch.randn(S))
    p, m, t = torch.zeros(S), torch.zeros(S), torch.zeros(1, dtype=torch.int32)
    ws, guard = sqnorm_workspace("cpu"), guard_state("cpu")
    with pytest.raises(ValueError, match="workspace"):
        out.optim_step_("sgd", p, m, None, t, 0.1, guard=guard)
    with pytest.raises(ValueError, match="both or neither"):
        out.sqnorm(ws, guard=guard)
    with pytest.raises(ValueError, match="both or neither"):
        out.sqnorm(ws, t=t)
    with pytest.raises(ValueError, match="int32"):
        out.sqnorm(ws, guard=torch.zeros(4), t=t)
    with pytest.raises(ValueError, match="int32"):
        out.sqnorm(ws, guard=torch.zeros(3, dtype=torch.int32), t=t)
    with pytest.raises(ValueError, match="int32"):
        out.optim_step_("sgd", p, m, None, t, 0.1, norm_ws=ws, guard=torch.zeros(4))
    assert int(t) == 0 and guard.tolist() == [0, 0, 0, 0]


def test_the_pass_owns_the_step_and_sq_has_the_same_bits_with_a_guard():
    ar = StubAllreduce(S, N, C)
    out = ar(_grads(1)[0])
    ws0, ws1, guard, t = sqnorm_workspace("cpu"), sqnorm_workspace("cpu"), guard_state("cpu"), \
        torch.zeros(1, dtype=torch.int32)
    assert _same_bits(out.sqnorm(ws0), out.sqnorm(ws1, guard, t))
    assert int(t) == 1 and guard.tolist() == [1, 0, 0, 0]


@pytest.mark.parametrize("kind", KINDS)
def test_without_the_guard_a_nan_under_the_clip_poisons_every_reached_parameter(kind):
    """What the guard is for: today's behaviour, which ``skip_nonfinite=False`` keeps."""
    b, opt, lr, ar = _setup(kind, False, clip=1.0)
    g = _grads(1)[0]
    g[int((ar.count > 0).nonzero()[17])] = float("nan")
    p0 = b.pflat.clone()
    b.flat.copy_(g)
    opt.step_from(ar, lr)
    reached = ar.count > 0
    assert int(opt.t) == 1 and bool(torch.isnan(b.pflat[reached]).all()) and bool(torch.isnan(opt.m[reached]).all())
    assert torch.equal(b.pflat[~reached], p0[~reached])
