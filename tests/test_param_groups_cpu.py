"""Parameter groups and the device-resident learning rate of FusedSGD /
FusedAdamW on the CPU: validation, segment merging, the torch expression of
the grouped pass (``optim_step_(groups=...)``) against torch's optimizers with
the same ``param_groups``, the zero-lr rule and the ``state_dict`` round trip.
Bound and method of the torch comparison are ``test_fused_optim_cpu.py``'s."""
import itertools

import pytest
import torch

from akka_allreduce_amd.data import AllReduceOutput, Geometry, OptimGroups, sqnorm_workspace
from akka_allreduce_amd.parallel import FusedAdamW, FusedSGD
from optim_cases import BF, HYPER, StubAllreduce, _bucket, _close, _same_bits

S, N, C = 1003, 4, 67
STEPS = 20


@pytest.mark.parametrize("cls", [FusedSGD, FusedAdamW])
def test_param_groups_are_validated(cls):
    b = _bucket()
    w1, b1, w2, b2 = b.params
    with pytest.raises(ValueError, match="already in group"):
        cls(b, param_groups=[{"params": [b1]}, {"params": [b2, b1]}])
    with pytest.raises(ValueError, match="not in the bucket"):
        cls(b, param_groups=[{"params": [torch.nn.Parameter(torch.zeros(3))]}])
    with pytest.raises(ValueError, match="unknown key 'lr'"):
        cls(b, param_groups=[{"params": [b1], "lr": 0.1}])
    with pytest.raises(ValueError, match=">= 0"):
        cls(b, param_groups=[{"params": [b1], "weight_decay": -1.0}])
    with pytest.raises(ValueError, match=">= 0"):
        cls(b, param_groups=[{"params": [b1], "lr_scale": -0.5}])
    with pytest.raises(ValueError, match="params"):
        cls(b, param_groups=[{"weight_decay": 0.0}])
    plain = cls(b)
    assert not plain.device_lr and plain.groups is None
    with pytest.raises(RuntimeError, match="launch arguments"):
        plain.set_lr(0.1)
    with pytest.raises(RuntimeError, match="launch arguments"):
        plain.set_group(0, weight_decay=0.0)


def test_segments_merge_and_the_rest_is_a_default_group():
    b = _bucket(sizes=(5, 7, 11, 13, 17))
    p = b.params
    assert b.spans() == [(0, 5), (5, 7), (12, 11), (23, 13), (36, 17)]
    # group 0: parameters 1 and 2 (adjacent: one segment) and 4; the rest (0 and 3) form the last group
    opt = FusedAdamW(b, weight_decay=0.05, param_groups=[{"params": [p[2], p[4], p[1]], "weight_decay": 0.0,
                                                           "lr_scale": 0.5}])
    assert opt.device_lr
    assert opt.groups.host_seg_end == [5, 23, 36, 53] and opt.groups.host_seg_group == [1, 0, 1, 0]
    assert opt.param_groups == [{"lr_scale": 0.5, "weight_decay": 0.0, "spans": [(5, 18), (36, 17)]},
                                {"lr_scale": 1.0, "weight_decay": 0.05, "spans": [(0, 5), (23, 13)]}]
    opt.param_groups[0]["weight_decay"] = 9.0  # copies
    assert opt.param_groups[0]["weight_decay"] == 0.0
    # every parameter listed: no default group; device_lr alone: one group, one segment
    full = FusedSGD(b, param_groups=[{"params": p[:2]}, {"params": p[2:], "lr_scale": 2.0}])
    assert full.groups.host_seg_end == [12, 53] and full.groups.ngroups == 2
    one = FusedSGD(b, weight_decay=0.1, device_lr=True)
    assert one.groups.host_seg_end == [53] and one.param_groups == [
        {"lr_scale": 1.0, "weight_decay": 0.1, "spans": [(0, 53)]}]
    # the rows: host-rounded in double, uploaded by set_lr / set_group, part of the captured addresses
    assert opt.lr is None
    opt.set_lr(0.3)
    want = torch.tensor([[-0.15, 0.0, 0.15, 1.0], [-0.3, 0.05, 0.3, 1.0 - 0.3 * 0.05]], dtype=torch.float64).float()
    assert torch.equal(opt.groups.rows, want) and opt.lr == 0.3
    rows_ptr = opt.groups.rows.data_ptr()
    opt.set_group(1, weight_decay=0.5, lr_scale=3.0)
    assert torch.equal(opt.groups.rows[1], torch.tensor([-0.3 * 3.0, 0.5, 0.3 * 3.0, 1.0 - 0.3 * 3.0 * 0.5],
                                                        dtype=torch.float64).float())
    assert opt.groups.rows.data_ptr() == rows_ptr and rows_ptr in opt.state_pointers()
    with pytest.raises(ValueError):
        OptimGroups([5, 5], [0, 0], 1, "cpu")
    with pytest.raises(ValueError):
        OptimGroups([5], [1], 1, "cpu")


GROUPS = (dict(lr_scale=1.0, weight_decay=0.01), dict(lr_scale=0.1, weight_decay=0.0),
          dict(lr_scale=2.5, weight_decay=0.1))


@pytest.mark.parametrize("wire", [False, True])
@pytest.mark.parametrize("clip", [None, 0.5])
@pytest.mark.parametrize("kind", ["sgd", "nesterov", "adamw"])
def test_grouped_steps_match_torch_with_the_same_param_groups(kind, clip, wire):
    b = _bucket(wire)
    ar = StubAllreduce(S, N, C)
    missing = ar.count == 0
    assert bool(missing.any())
    # weights / first bias / last bias: neighbours always differ
    members = ([b.params[0], b.params[2]], [b.params[1]], [b.params[3]])
    pg = [{"params": ps, **h} for ps, h in zip(members, GROUPS)]
    spans = b.spans()
    refs = [torch.nn.Parameter(b.pflat[o:o + n].detach().clone()) for o, n in spans]  # one Parameter per segment
    ref_of = {id(p): r for p, r in zip(b.params, refs)}
    if kind == "adamw":
        opt, lr = FusedAdamW(b, weight_decay=0.3, max_grad_norm=clip, param_groups=pg), 1e-3
        ref = torch.optim.AdamW([{"params": [ref_of[id(p)] for p in ps], "lr": lr * h["lr_scale"],
                                  "weight_decay": h["weight_decay"]} for ps, h in zip(members, GROUPS)],
                                lr=lr, foreach=False)
        names = ("exp_avg", "exp_avg_sq")
    else:
        opt, lr = FusedSGD(b, momentum=0.9, nesterov=kind == "nesterov", weight_decay=0.3, max_grad_norm=clip,
                           param_groups=pg), 0.05
        ref = torch.optim.SGD([{"params": [ref_of[id(p)] for p in ps], "lr": lr * h["lr_scale"],
                                "weight_decay": h["weight_decay"]} for ps, h in zip(members, GROUPS)],
                              lr=lr, momentum=0.9, nesterov=kind == "nesterov", foreach=False)
        names = ("momentum_buffer",)
    assert len(opt.groups.host_seg_end) == 4 and opt.groups.ngroups == 3
    gen = torch.Generator().manual_seed(7)
    for step in range(STEPS):
        b.flat.copy_(torch.randn(S, generator=gen))
        opt.step_from(ar, lr)
        mean = ar.mean()
        for (o, n), r in zip(spans, refs):
            r.grad = mean[o:o + n].clone()
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(refs, clip, foreach=False)
        before = [(r.detach().clone(), {k: ref.state[r][k].clone() if k in ref.state.get(r, {})
                                        else torch.zeros(n) for k in names}) for (o, n), r in zip(spans, refs)]
        ref.step()
        with torch.no_grad():  # count-0 chunks put back
            for (o, n), r, (p0, st0) in zip(spans, refs, before):
                miss = missing[o:o + n]
                r[miss] = p0[miss]
                for k in names:
                    ref.state[r][k][miss] = st0[k][miss]
    assert int(opt.t) == STEPS and opt.lr == lr
    _close(b.pflat, torch.cat([r.detach() for r in refs]), "p")
    _close(opt.m, torch.cat([ref.state[r][names[0]] for r in refs]), "m")
    if kind == "adamw":
        _close(opt.v, torch.cat([ref.state[r]["exp_avg_sq"] for r in refs]), "v")
    assert b.params_bound() and torch.equal(torch.cat([p.detach().view(-1) for p in b.params]), b.pflat)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_a_group_with_lr_zero_advances_the_state_and_leaves_p(kind):
    def run(scale):
        b = _bucket()
        ar = StubAllreduce(S, N, C)
        pg = [{"params": [b.params[1], b.params[3]], "lr_scale": scale, "weight_decay": 0.2}]
        opt = FusedAdamW(b, param_groups=pg) if kind == "adamw" else FusedSGD(b, param_groups=pg)
        p0 = b.pflat.clone()
        b.flat.copy_(torch.randn(S, generator=torch.Generator().manual_seed(3)))
        opt.step_from(ar, 1e-2)  # AdamW: from v == 0, where the step's formula is 0 / -0
        return b, opt, p0, ar.count == 0

    b, opt, p0, missing = run(0.0)
    _, pos, _, _ = run(1.0)
    for x in (b.pflat, opt.m) + ((opt.v,) if kind == "adamw" else ()):
        assert bool(torch.isfinite(x).all())
    in_group = torch.zeros(S, dtype=torch.bool)
    for o, n in opt.param_groups[0]["spans"]:
        in_group[o:o + n] = True
    assert torch.equal(b.pflat[in_group], p0[in_group])
    live = ~in_group & ~missing
    assert bool((b.pflat[live] != p0[live]).all())  # the other group moved
    assert torch.equal(opt.m, pos.m)
    if kind == "adamw":
        assert torch.equal(opt.v, pos.v)
    assert float(opt.m[in_group & ~missing].abs().min()) > 0


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("cls", [FusedSGD, FusedAdamW])
def test_state_dict_round_trip(cls, grouped):
    lrs = (1e-2, 8e-3, 6e-3, 4e-3, 2e-3)

    def make():
        b = _bucket()
        kw = dict(param_groups=[{"params": [b.params[1], b.params[3]], "weight_decay": 0.0, "lr_scale": 0.5}]) \
            if grouped else {}
        return b, cls(b, weight_decay=0.05, max_grad_norm=1.0, **kw), StubAllreduce(S, N, C)

    def steps(b, opt, ar, which):
        for i in which:
            b.flat.copy_(torch.randn(S, generator=torch.Generator().manual_seed(100 + i)))
            opt.step_from(ar, lrs[i])

    b1, o1, ar1 = make()
    steps(b1, o1, ar1, range(3))
    saved, p_saved = o1.state_dict(), b1.pflat.clone()
    assert saved["kind"] == o1.kind and saved["numel"] == S and saved["t"] == 3
    assert saved["lr"] == (lrs[2] if grouped else None) and saved["param_groups"] == o1.param_groups
    assert saved["hyper"]["max_grad_norm"] == 1.0 and saved["hyper"]["weight_decay"] == 0.05
    assert saved["m"].data_ptr() != o1.m.data_ptr()
    steps(b1, o1, ar1, range(3, 5))
    assert not torch.equal(saved["m"], o1.m)  # a clone

    b2, o2, ar2 = make()
    with torch.no_grad():
        b2.pflat.copy_(p_saved)
    ptrs = o2.state_pointers()
    o2.load_state_dict(saved)
    assert o2.state_pointers() == ptrs and int(o2.t) == 3 and o2.lr == saved["lr"]
    steps(b2, o2, ar2, range(3, 5))
    assert torch.equal(b1.pflat, b2.pflat) and torch.equal(o1.m, o2.m) and int(o2.t) == 5
    if o1.v is not None:
        assert torch.equal(o1.v, o2.v)

    # mismatches are named
    other = FusedSGD(b2) if cls is FusedAdamW else FusedAdamW(b2)
    with pytest.raises(ValueError, match="kind"):
        other.load_state_dict(saved)
    with pytest.raises(ValueError, match="numel"):
        cls(_bucket(sizes=(8, 4))).load_state_dict(saved)
    with pytest.raises(ValueError, match="param_groups"):
        bb = _bucket()
        # another layout: fewer groups than an ungrouped state has spans for, other spans than the grouped one's
        cls(bb, weight_decay=0.05, max_grad_norm=1.0, param_groups=[{"params": [bb.params[0]]}]).load_state_dict(saved)
    with pytest.raises(ValueError, match="max_grad_norm"):
        bb = _bucket()
        kw = dict(param_groups=[{"params": [bb.params[1], bb.params[3]]}]) if grouped else {}
        cls(bb, weight_decay=0.05, max_grad_norm=2.0, **kw).load_state_dict(saved)


def test_load_state_dict_takes_the_groups_hyper_parameters_and_rewrites_the_rows():
    b = _bucket()
    o = FusedAdamW(b, param_groups=[{"params": [b.params[1]], "weight_decay": 0.0}])
    o.set_lr(0.5)
    o.set_group(0, weight_decay=0.25, lr_scale=4.0)
    d = o.state_dict()
    b2 = _bucket()
    o2 = FusedAdamW(b2, param_groups=[{"params": [b2.params[1]], "weight_decay": 0.0}])
    o2.load_state_dict(d)
    assert o2.param_groups == o.param_groups and torch.equal(o2.groups.rows, o.groups.rows)
    assert float(o2.groups.rows[0, 2]) == 2.0 and float(o2.groups.rows[0, 1]) == 0.25


def test_plain_torch_path_is_the_one_group_path_bitwise():
    """The torch path of ``optim_step_`` has one set of formulas and two ways in: ``lr`` / ``weight_decay`` as
    0-dim values, or the rows of ``groups`` expanded per element.  With one group over the whole buffer, whose row
    is made from the same ``lr`` and ``weight_decay``, both give the same bits: fp32 and bf16 sums and state, every
    kind, with and without the clip, random counts in [0, N] (some chunks missing), at step 7."""
    t = torch.full((1,), 7, dtype=torch.int32)
    cases = 0
    for (S, N, C), src, sdt, kind, clip in itertools.product(
            [(1000, 3, 64), (4099, 4, 257), (37, 5, 3)], (torch.float32, BF), (torch.float32, BF),
            ("sgd", "nesterov", "adamw"), (False, True)):
        geo = Geometry(S, N, C)
        g = torch.Generator().manual_seed(S * 31 + N)
        pc = torch.randint(0, N + 1, (N, geo.kmax), dtype=torch.int32, generator=g)
        count = geo.expand_counts(pc)
        assert bool((count == 0).any()) and bool((count > 0).any())
        data = (torch.randn(S, generator=g) * count).to(src)
        start = [torch.randn(S, generator=g), (0.1 * torch.randn(S, generator=g)).to(sdt),
                 (0.01 * torch.rand(S, generator=g)).to(sdt), torch.full((S,), -3.5, dtype=BF)]
        adam = kind == "adamw"
        h = dict(HYPER[kind])
        lr, wd = h.pop("lr"), h.pop("weight_decay")
        groups = OptimGroups([S], [0], 1, "cpu")
        groups.write_rows(OptimGroups.row_values(lr, [(1.0, wd)]))
        runs = []
        for gr in (None, groups):
            p, m, v, sh = (x.clone() for x in start)
            out = AllReduceOutput(data, counts_per_chunk=pc, geometry=geo)
            # with groups lr and weight_decay are not used: 0 is passed
            out.optim_step_("adamw" if adam else "sgd", p, m, v if adam else None, t, lr if gr is None else 0.0,
                            weight_decay=wd if gr is None else 0.0, shadow=sh, seed=5,
                            max_norm=0.1 * S ** 0.5 if clip else None,
                            norm_ws=sqnorm_workspace("cpu") if clip else None, groups=gr, **h)
            runs.append((p, m, v, sh))
        for name, a, b in zip(("p", "m", "v", "shadow"), *runs):
            assert _same_bits(a, b), (S, src, sdt, kind, clip, name)
        assert not _same_bits(runs[0][0], start[0]) and not _same_bits(runs[0][1], start[1])
        cases += 1
    assert cases == 72
