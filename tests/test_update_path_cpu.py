"""The one update path: ``GradientBucket.update_from`` with the plain SGD rule
and the fused optimizers behind ``sgd_from`` / ``step_from`` / ``dp_sgd_step``,
the bucket's ``snapshot`` / ``restore``, and what the native count passes
refuse before they launch (checked on the host, so no GPU is needed)."""
import pytest
import torch

from akka_allreduce_amd._native_loader import load
from akka_allreduce_amd.data import AllReduceOutput, Geometry
from akka_allreduce_amd.models.mlp import MLP, _forward_backward, dp_sgd_step, synthetic_batch
from akka_allreduce_amd.parallel import FusedAdamW, FusedSGD
from akka_allreduce_amd.parallel.dp import GradientBucket

LR = 0.05
RULES = {
    "plain": lambda b: b.sgd,
    "sgd": lambda b: FusedSGD(b, momentum=0.9, weight_decay=1e-2),
    "adamw": lambda b: FusedAdamW(b, weight_decay=0.01, max_grad_norm=1.0),
}


class ExactAllreduce:
    """A complete round of one rank: the sum is the input, every count is 1."""

    def __init__(self, S):
        self.geometry = Geometry(S, 1, S)
        self.counts = torch.ones((1, 1), dtype=torch.int32)

    def __call__(self, t, out=None):
        data = t.clone() if out is None else out.copy_(t)
        return AllReduceOutput(data, counts_per_chunk=self.counts, geometry=self.geometry)


def _setup(wire, rule="adamw"):
    torch.manual_seed(0)
    model = MLP(6, 5, 3)
    bucket = GradientBucket(list(model.parameters()), flatten_params=True,
                            wire_dtype=torch.bfloat16 if wire else None)
    gen = torch.Generator().manual_seed(3)
    batches = [synthetic_batch(8, 6, 3, device="cpu", generator=gen) for _ in range(3)]
    return model, bucket, RULES[rule](bucket), ExactAllreduce(bucket.numel), batches


# ---- the native launchers check before they launch --------------------------------------------

# fake addresses, 16-B aligned: nothing is launched, so nothing reads them
DST, SRC, COUNTS = 1 << 20, 2 << 20, 3 << 20


@pytest.mark.parametrize("C,kmax", [(8, 0), (0, 1)])
def test_count_passes_refuse_bad_geometry(C, kmax):
    nat = load()
    table = (COUNTS, 8, 8, 1, C, kmax)  # S = 8 > 0
    with pytest.raises(RuntimeError, match="count_mean: bad geometry"):
        nat.count_mean(DST, SRC, table, "float32", 0)
    with pytest.raises(RuntimeError, match="count_expand: bad geometry"):
        nat.count_expand(DST, table, 0)


def test_unknown_dtype_names_are_refused():
    nat = load()
    with pytest.raises(RuntimeError, match="unsupported dtype float16"):
        nat.count_mean(DST, SRC, (COUNTS, 8, 8, 1, 8, 1), "float16", 0)
    with pytest.raises(RuntimeError, match="unsupported dtype float16"):
        nat.count_mean(DST, SRC, (COUNTS, 8, 8, 1, 8, 1), "float32", 0, src_dtype="float16")
    with pytest.raises(RuntimeError, match="unsupported dtype float16"):
        nat.reduce(DST, [SRC], 8, "float16", 0, "auto")


# ---- snapshot / restore ----------------------------------------------------------------------


@pytest.mark.parametrize("wire", [False, True])
def test_snapshot_restore_round_trip(wire):
    model, bucket, opt, ar, batches = _setup(wire)
    dp_sgd_step(model, *batches[0], LR, ar, optimizer=opt)  # state, step counter and residual are not zero
    assert (bucket.residual is not None) == wire
    want = [x.clone() for x in (bucket.pflat, *opt.state_tensors())] + ([bucket.residual.clone()] if wire else [])
    assert int(opt.t) == 1 and all(bool(x.any()) for x in want)
    snap, state = bucket.snapshot(), [s.clone() for s in opt.state_tensors()]
    for x, y in batches[1:]:
        dp_sgd_step(model, x, y, LR, ar, optimizer=opt)
    assert int(opt.t) == 3 and not torch.equal(bucket.pflat, want[0])
    bucket.restore(snap)
    for s, keep in zip(opt.state_tensors(), state):
        s.copy_(keep)
    got = [bucket.pflat, opt.m, opt.v, opt.t] + ([bucket.residual] if wire else [])
    assert len(got) == len(want)
    for name, a, b in zip(("pflat", "m", "v", "t", "residual"), got, want):
        assert torch.equal(a, b), name
    # the parameters are still the views of pflat, and the snapshot is a copy of its own
    assert bucket.params_bound() and snap[0].data_ptr() != bucket.pflat.data_ptr()


# ---- one path behind every entry point -------------------------------------------------------


def _run(entry, rule, wire):
    model, bucket, r, ar, batches = _setup(wire, rule)
    for x, y in batches:
        if entry == "step":
            dp_sgd_step(model, x, y, LR, ar, bucket, optimizer=None if rule == "plain" else r)
            continue
        _forward_backward(model, x, y, bucket, None, True, True, True)  # what dp_sgd_step runs before the update
        if entry == "update_from":
            out = bucket.update_from(ar, LR, r)
        else:
            out = bucket.sgd_from(ar, LR) if rule == "plain" else r.step_from(ar, LR)
        assert out.data.dtype == (torch.bfloat16 if wire else torch.float32)
    return bucket.pflat.clone(), [s.clone() for s in r.state_tensors()]


@pytest.mark.parametrize("wire", [False, True])
@pytest.mark.parametrize("rule", list(RULES))
def test_every_entry_point_leaves_the_same_parameters(rule, wire):
    p0 = _setup(wire, rule)[1].pflat.clone()
    want_p, want_state = _run("from", rule, wire)
    assert not torch.equal(want_p, p0)
    assert len(want_state) == {"plain": 0, "sgd": 2, "adamw": 3}[rule]
    for entry in ("update_from", "step"):
        p, state = _run(entry, rule, wire)
        assert torch.equal(p, want_p), entry
        for a, b in zip(state, want_state):
            assert torch.equal(a, b), entry


@pytest.mark.parametrize("rule", ["sgd", "adamw"])
def test_without_an_allreduce_the_update_is_a_one_rank_round(rule):
    runs = []
    for solo in (True, False):
        model, bucket, opt, ar, batches = _setup(False, rule)
        for x, y in batches:
            _forward_backward(model, x, y, bucket, None, True, True, True)
            out = opt.step_from(None if solo else ar, LR)
            assert (out is None) == solo
        runs.append([bucket.pflat, *opt.state_tensors()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_plain_sgd_without_an_allreduce_is_the_per_parameter_update():
    model, bucket, rule, ar, batches = _setup(False, "plain")
    _forward_backward(model, *batches[0], bucket, None, True, True, True)
    want = [torch.add(p.detach(), p.grad, alpha=-LR) for p in bucket.params]
    assert bucket.update_from(None, LR, rule) is None
    for p, w in zip(bucket.params, want):
        assert torch.equal(p.detach(), w)
