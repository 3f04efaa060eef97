"""FusedLAMB on the CPU: the torch expression of ``optim_step_(kind="lamb")``
against the rule in float64 (``lamb_cases.lamb_rule``), the arguments it
refuses, ``layer_adaptation`` groups, and the in-place ``state_dict`` round
trip."""
import math

import pytest
import torch

from akka_allreduce_amd.data import OptimGroups, lamb_workspace
from akka_allreduce_amd.parallel import FusedLAMB
from akka_allreduce_amd.parallel.dp import GradientBucket
from lamb_cases import clip_coefficient, lamb_rule
from optim_cases import StubAllreduce, _bucket, _close

S, N, C = 1003, 4, 67
ENDS = [640, 700, 1000, 1003]
STEPS = 5


def _groups(b):
    """The biases: no decay, half the rate, no layer adaptation."""
    return [{"params": [b.params[1], b.params[3]], "weight_decay": 0.0, "lr_scale": 0.5, "layer_adaptation": False}]


@pytest.mark.parametrize("wire", [False, True])
@pytest.mark.parametrize("clip", [None, 0.5])
def test_steps_match_the_rule_in_float64(clip, wire):
    b = _bucket(wire)
    assert b.numel == S
    ar = StubAllreduce(S, N, C)
    missing = ar.count == 0
    assert bool(missing.any()) and bool((~missing).any())
    opt = FusedLAMB(b, weight_decay=0.01, max_grad_norm=clip, param_groups=_groups(b))
    assert opt.device_lr and opt.groups.host_seg_end == ENDS and opt.groups.host_seg_group == [1, 0, 1, 0]
    assert opt.layer_adapt.tolist() == [1, 0, 1, 0]
    lr = 1e-2
    wd, lrs, adapt = [0.01, 0.0, 0.01, 0.0], [lr, lr / 2, lr, lr / 2], [True, False, True, False]
    p, m, v = b.pflat.detach().double(), torch.zeros(S, dtype=torch.float64), torch.zeros(S, dtype=torch.float64)
    gen = torch.Generator().manual_seed(7)
    for step in range(STEPS):
        b.flat.copy_(torch.randn(S, generator=gen))
        opt.step_from(ar, lr)
        g = ar.mean().double()
        if clip is not None:
            g = g * clip_coefficient(float((g * g).sum()), clip)
        p, m, v, r = lamb_rule(p, m, v, g, missing, ENDS, wd, lrs, adapt, step + 1, opt.betas, opt.eps)
        got = torch.cat(opt.trust_ratios())
        # the fp32 path holds b2 = 0.999 as fp32, off by up to 2**-25 * 0.999 = 3e-8; bc2 = 1 - b2**t = 1e-3 at
        # t = 1 takes that as a relative 3e-5, u ~ sqrt(bc2) and r ~ 1 / ||u|| half of it; the sums' own
        # rounding (1003 terms) is below 1e-5: 3e-5 in all
        torch.testing.assert_close(got.double(), r, rtol=3e-5, atol=0)
        assert got[1] == 1.0 and got[3] == 1.0  # opted out: exactly 1
    assert int(opt.t) == STEPS
    _close(b.pflat, p.float(), "p")
    _close(opt.m, m.float(), "m")
    _close(opt.v, v.float(), "v")
    assert b.params_bound() and torch.equal(torch.cat([q.detach().view(-1) for q in b.params]), b.pflat)


def test_missing_and_zero_layers_keep_a_ratio_of_one():
    """The first 67 elements are the stub's count-0 chunk: a layer inside it has no contributor; an all-zero
    layer has no norm."""
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (60, 7, 636, 300)]
    with torch.no_grad():
        ps[3].zero_()
    b = GradientBucket(ps, flatten_params=True)
    ar = StubAllreduce(S, N, C)
    assert bool((ar.count[:67] == 0).all())
    opt = FusedLAMB(b, weight_decay=0.0)
    opt.m.fill_(0.25)
    opt.v.fill_(0.5)
    p0 = b.pflat.clone()
    b.flat.copy_(torch.randn(S))
    opt.step_from(ar, 1e-2)
    r = [float(x) for x in opt.trust_ratios()]
    assert r[0] == 1.0 and r[1] == 1.0 and r[3] == 1.0 and r[2] != 1.0
    missing = ar.count == 0
    assert torch.equal(b.pflat[missing], p0[missing])
    assert bool((opt.m[missing] == 0.25).all()) and bool((opt.v[missing] == 0.5).all())
    assert bool((opt.m[~missing] != 0.25).all()) and bool((b.pflat[67:703][~missing[67:703]] != p0[67:703][~missing[67:703]]).all())


def test_lr_zero_group_advances_the_state_and_keeps_p():
    b = _bucket()
    ar = StubAllreduce(S, N, C)
    opt = FusedLAMB(b, param_groups=[{"params": [b.params[0]], "lr_scale": 0.0}])
    p0 = b.pflat.clone()
    b.flat.copy_(torch.randn(S))
    opt.step_from(ar, 1e-2)
    live = ar.count > 0
    assert torch.equal(b.pflat[:640], p0[:640])
    assert bool((opt.m[:640][live[:640]] != 0).all()) and bool((opt.v[:640][live[:640]] != 0).all())
    assert bool((b.pflat[640:][live[640:]] != p0[640:][live[640:]]).all())


def test_constructor_and_groups():
    ps = [torch.nn.Parameter(torch.randn(8)), torch.nn.Parameter(torch.randn(0)), torch.nn.Parameter(torch.randn(3))]
    with pytest.raises(ValueError, match="flatten_params"):
        FusedLAMB(GradientBucket(ps))
    b = GradientBucket(ps, flatten_params=True)
    for bad in (dict(betas=(0.9, 1.0)), dict(eps=-1.0), dict(weight_decay=-0.1), dict(max_grad_norm=0.0),
                dict(state_dtype=torch.float16), dict(seed=-1), dict(skip_nonfinite=1)):
        with pytest.raises(ValueError):
            FusedLAMB(b, **bad)
    with pytest.raises(TypeError):
        FusedLAMB(b, device_lr=False)  # always on: not an argument
    with pytest.raises(ValueError, match="layer_adaptation"):
        FusedLAMB(b, param_groups=[{"params": [ps[2]], "layer_adaptation": 0}])
    with pytest.raises(ValueError, match="unknown key"):
        FusedLAMB(b, param_groups=[{"params": [ps[2]], "trust_clip": 10.0}])
    from akka_allreduce_amd.parallel import FusedAdamW
    with pytest.raises(ValueError, match="unknown key"):
        FusedAdamW(b, param_groups=[{"params": [ps[2]], "layer_adaptation": False}])  # LAMB's key only
    # one segment per non-empty parameter, neighbours of one group not merged
    opt = FusedLAMB(b)
    assert opt.groups.host_seg_end == [8, 11] and opt.groups.host_seg_group == [0, 0]
    assert opt.param_groups == [{"lr_scale": 1.0, "weight_decay": 0.01, "layer_adaptation": True,
                                 "spans": [(0, 8), (8, 3)]}]
    tr = opt.trust_ratios()
    assert [x.numel() for x in tr] == [1, 0, 1] and all(x.data_ptr() - opt.trust.data_ptr() == 4 * i
                                                         for x, i in ((tr[0], 0), (tr[2], 1)))
    assert float(tr[0]) == 1.0
    opt = FusedLAMB(b, param_groups=[{"params": ps[2], "layer_adaptation": False, "weight_decay": 0.0}])
    assert opt.layer_adapt.tolist() == [1, 0] and opt.groups.host_seg_group == [1, 0]
    assert [g["layer_adaptation"] for g in opt.param_groups] == [False, True]
    ptrs = opt.state_pointers()
    for x in (opt.lamb_ws, opt.trust, opt.layer_adapt, opt.m, opt.v, opt.t):
        assert x.data_ptr() in ptrs
    opt.set_lr(0.1)
    assert opt.lr == 0.1 and torch.equal(opt.groups.rows[:, 2], torch.tensor([0.1, 0.1]))


def test_optim_step_validates_lamb():
    ar = StubAllreduce(S, N, C)
    out = ar(torch.randn(S))
    p, m, v, t = torch.zeros(S), torch.zeros(S), torch.zeros(S), torch.ones(1, dtype=torch.int32)
    gr = OptimGroups(ENDS, [0, 0, 0, 0], 1, "cpu")
    gr.write_rows(OptimGroups.row_values(0.1, [(1.0, 0.01)]))
    ok = dict(groups=gr, trust=torch.ones(4), layer_adapt=torch.ones(4, dtype=torch.int32),
              lamb_ws=lamb_workspace(S, 4, "cpu"))
    out.optim_step_("lamb", p, m, v, t, 0.0, **ok)  # what is refused below is complete here
    with pytest.raises(ValueError, match="kind"):
        out.optim_step_("lars", p, m, v, t, 0.1, **ok)
    with pytest.raises(ValueError, match="v must"):
        out.optim_step_("lamb", p, m, None, t, 0.1, **ok)
    with pytest.raises(ValueError, match="nt=True"):
        out.optim_step_("lamb", p, m, v, t, 0.1, nt=True, **ok)
    with pytest.raises(ValueError, match="needs groups"):
        out.optim_step_("lamb", p, m, v, t, 0.1, **{**ok, "groups": None})
    with pytest.raises(ValueError, match="trust"):
        out.optim_step_("lamb", p, m, v, t, 0.1, **{**ok, "trust": torch.ones(3)})
    with pytest.raises(ValueError, match="trust"):
        out.optim_step_("lamb", p, m, v, t, 0.1, **{**ok, "trust": None})
    with pytest.raises(ValueError, match="layer_adapt"):
        out.optim_step_("lamb", p, m, v, t, 0.1, **{**ok, "layer_adapt": torch.ones(4)})
    with pytest.raises(ValueError, match="lamb_ws"):
        out.optim_step_("lamb", p, m, v, t, 0.1, **{**ok, "lamb_ws": None})
    with pytest.raises(ValueError, match="lamb_ws"):
        out.optim_step_("lamb", p, m, v, t, 0.1, **{**ok, "lamb_ws": torch.zeros(8, dtype=torch.float64)})
    with pytest.raises(ValueError, match="workspace"):
        out.optim_step_("lamb", p, m, v, t, 0.1, max_norm=1.0, **ok)


@pytest.mark.parametrize("state_dtype", [torch.float32, torch.bfloat16])
def test_state_dict_round_trip_in_place(state_dtype):
    def make():
        b = _bucket()
        return b, FusedLAMB(b, weight_decay=0.01, max_grad_norm=1.0, param_groups=_groups(b), state_dtype=state_dtype,
                            seed=3, skip_nonfinite=True)

    ar = StubAllreduce(S, N, C)
    gen = torch.Generator().manual_seed(3)
    grads = [torch.randn(S, generator=gen) for _ in range(4)]
    b1, o1 = make()
    for g in grads[:2]:
        b1.flat.copy_(g)
        o1.step_from(ar, 1e-2)
    d = o1.state_dict()
    assert d["kind"] == "lamb" and d["t"] == 2 and d["seed"] == 3 and d["state_dtype"] == state_dtype
    assert d["param_groups"][0]["layer_adaptation"] is False and d["param_groups"][1]["layer_adaptation"] is True
    b2, o2 = make()
    ptrs = o2.state_pointers()
    with torch.no_grad():
        b2.pflat.copy_(b1.pflat)
    o2.load_state_dict(d)
    assert o2.state_pointers() == ptrs and int(o2.t) == 2 and o2.lr == 1e-2
    for g in grads[2:]:
        for b, o in ((b1, o1), (b2, o2)):
            b.flat.copy_(g)
            o.step_from(ar, 1e-2)
    assert torch.equal(b1.pflat, b2.pflat) and torch.equal(o1.m, o2.m) and torch.equal(o1.v, o2.v)
    assert int(o2.t) == 4 and torch.equal(o1.trust, o2.trust) and torch.equal(o1.guard, o2.guard)
    # the refusals
    _, other = make()
    with pytest.raises(ValueError, match="layer_adaptation"):
        flipped = {**d, "param_groups": [{**g, "layer_adaptation": True} for g in d["param_groups"]]}
        other.load_state_dict(flipped)
    with pytest.raises(ValueError, match="kind"):
        other.load_state_dict({**d, "kind": "adamw"})
    with pytest.raises(ValueError, match="seed"):
        other.load_state_dict({**d, "seed": 4})
    with pytest.raises(ValueError, match="skip_nonfinite"):
        other.load_state_dict({**d, "skip_nonfinite": False})
    with pytest.raises(ValueError, match="eps"):
        other.load_state_dict({**d, "hyper": {**d["hyper"], "eps": 1e-3}})
    with pytest.raises(ValueError, match="spans"):
        other.load_state_dict({**d, "param_groups": list(reversed(d["param_groups"]))})
    with pytest.raises(ValueError, match="numel"):
        other.load_state_dict({**d, "numel": S + 1})


def test_mlp_trains_on_cpu_with_fused_lamb():
    from akka_allreduce_amd.models.mlp import MLP, dp_sgd_step, synthetic_batch
    from akka_allreduce_amd.parallel import ThresholdAllreduce

    gen = torch.Generator().manual_seed(11)
    x, y = synthetic_batch(64, 32, 10, device="cpu", generator=gen)
    torch.manual_seed(0)
    model = MLP(32, 64, 10)
    bucket = GradientBucket(list(model.parameters()), flatten_params=True)
    opt = FusedLAMB(bucket, weight_decay=0.01, max_grad_norm=1.0,
                    param_groups=[{"params": [model.fc1.bias, model.fc2.bias], "weight_decay": 0.0,
                                   "layer_adaptation": False}])
    ar = ThresholdAllreduce(bucket.numel, max_chunk_size=512, device="cpu", rank=0, world_size=1)
    losses = [dp_sgd_step(model, x, y, 1e-2, ar, optimizer=opt) for _ in range(30)]
    # a LAMB step moves a layer by lr * ||p||: 30 steps at 1e-2 lower the loss steadily, not to the bottom
    assert all(math.isfinite(v) for v in losses) and max(losses[-5:]) < min(losses[:5]), losses
    r = [float(v) for v in opt.trust_ratios()]
    assert r[1] == 1.0 and r[3] == 1.0 and r[0] != 1.0 and r[2] != 1.0
