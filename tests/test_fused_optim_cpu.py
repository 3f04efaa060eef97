"""FusedSGD / FusedAdamW on the CPU: the torch expression of the fused
optimizer pass (``AllReduceOutput.optim_step_``) against torch's own
optimizers run on the count-weighted mean, with the elements of count-0 chunks
put back afterwards (a missing chunk leaves parameters and state untouched)."""
import pytest
import torch

import optim_cases
from akka_allreduce_amd.parallel import FusedAdamW, FusedSGD
from akka_allreduce_amd.parallel.dp import GradientBucket
from optim_cases import StubAllreduce, _close

S, N, C = 1003, 4, 67
STEPS = 5


def _bucket(wire):
    b = optim_cases._bucket(wire, sizes=(700, 300, 3))
    assert b.numel == S
    return b


@pytest.mark.parametrize("wire", [False, True])
@pytest.mark.parametrize("clip", [None, 0.5])
@pytest.mark.parametrize("kind", ["sgd", "nesterov", "adamw"])
def test_steps_match_torch_with_missing_chunks_restored(kind, clip, wire):
    b = _bucket(wire)
    ar = StubAllreduce(S, N, C)
    missing = ar.count == 0
    assert bool(missing.any()) and bool((ar.count == N).any()) and bool(((ar.count > 0) & (ar.count < N)).any())
    if kind == "adamw":
        opt, lr = FusedAdamW(b, weight_decay=0.01, max_grad_norm=clip), 1e-3
        ref_p = torch.nn.Parameter(b.pflat.detach().clone())
        ref = torch.optim.AdamW([ref_p], lr=lr, weight_decay=0.01, foreach=False)
        names = ("exp_avg", "exp_avg_sq")
    else:
        opt, lr = FusedSGD(b, momentum=0.9, nesterov=kind == "nesterov", weight_decay=1e-2, max_grad_norm=clip), 0.05
        ref_p = torch.nn.Parameter(b.pflat.detach().clone())
        ref = torch.optim.SGD([ref_p], lr=lr, momentum=0.9, nesterov=kind == "nesterov", weight_decay=1e-2,
                              foreach=False)
        names = ("momentum_buffer",)
    gen = torch.Generator().manual_seed(7)
    for step in range(STEPS):
        b.flat.copy_(torch.randn(S, generator=gen))
        out = opt.step_from(ar, lr)
        assert out.data is ar.last and out.data.dtype == (torch.bfloat16 if wire else torch.float32)
        ref_p.grad = ar.mean()
        if clip is not None:
            torch.nn.utils.clip_grad_norm_([ref_p], clip, foreach=False)
        p0 = ref_p.detach().clone()
        st0 = {k: ref.state[ref_p][k].clone() if k in ref.state.get(ref_p, {}) else torch.zeros(S) for k in names}
        ref.step()
        with torch.no_grad():
            ref_p[missing] = p0[missing]
            for k in names:
                ref.state[ref_p][k][missing] = st0[k][missing]
    assert int(opt.t) == STEPS
    _close(b.pflat, ref_p.detach(), "p")
    _close(opt.m, ref.state[ref_p][names[0]], "m")
    if kind == "adamw":
        _close(opt.v, ref.state[ref_p]["exp_avg_sq"], "v")
    # the parameters are still the bucket's views
    assert b.params_bound() and torch.equal(torch.cat([p.detach().view(-1) for p in b.params]), b.pflat)


def test_missing_chunk_keeps_parameters_and_state_bitwise():
    b = _bucket(False)
    ar = StubAllreduce(S, N, C)
    missing = ar.count == 0
    opt = FusedAdamW(b)
    opt.m.fill_(0.25)
    opt.v.fill_(0.5)
    p0 = b.pflat.clone()
    b.flat.copy_(torch.randn(S))
    opt.step_from(ar, 1e-2)
    assert torch.equal(b.pflat[missing], p0[missing])
    assert bool((opt.m[missing] == 0.25).all()) and bool((opt.v[missing] == 0.5).all())
    assert bool((b.pflat[~missing] != p0[~missing]).all())
    assert bool((opt.m[~missing] != 0.25).all()) and bool((opt.v[~missing] != 0.5).all())


def test_without_an_allreduce_the_bucket_is_a_round_of_one():
    b = _bucket(False)
    opt = FusedSGD(b, momentum=0.9, weight_decay=0.0)
    ref_p = torch.nn.Parameter(b.pflat.detach().clone())
    ref = torch.optim.SGD([ref_p], lr=0.1, momentum=0.9, foreach=False)
    for _ in range(3):
        g = torch.randn(S)
        b.flat.copy_(g)
        assert opt.step_from(None, 0.1) is None
        ref_p.grad = g.clone()
        ref.step()
    _close(b.pflat, ref_p.detach(), "p")


def test_constructor_refuses_what_the_fused_pass_cannot_update():
    ps = [torch.nn.Parameter(torch.randn(8))]
    for cls in (FusedSGD, FusedAdamW):
        with pytest.raises(ValueError, match="flatten_params"):
            cls(GradientBucket(ps))  # not flattened
        with pytest.raises(ValueError, match="flatten_params"):
            cls(GradientBucket([torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16))], flatten_params=True))
        with pytest.raises(ValueError):
            cls(GradientBucket(ps, flatten_params=True), max_grad_norm=0.0)
    with pytest.raises(ValueError):
        FusedSGD(GradientBucket(ps, flatten_params=True), momentum=0.0, nesterov=True)
    with pytest.raises(ValueError):
        FusedAdamW(GradientBucket(ps, flatten_params=True), betas=(0.9, 1.0))


def test_optim_step_validates():
    ar = StubAllreduce(S, N, C)
    out = ar(torch.randn(S))
    p, m, t = torch.zeros(S), torch.zeros(S), torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="kind"):
        out.optim_step_("adam", p, m, None, t, 0.1)
    with pytest.raises(ValueError, match="v must"):
        out.optim_step_("adamw", p, m, None, t, 0.1)
    with pytest.raises(ValueError, match="m must"):
        out.optim_step_("sgd", p, torch.zeros(S + 1), None, t, 0.1)
    with pytest.raises(ValueError, match="int32"):
        out.optim_step_("sgd", p, m, None, torch.ones(1), 0.1)
    with pytest.raises(ValueError, match="workspace"):
        out.optim_step_("sgd", p, m, None, t, 0.1, max_norm=1.0)
    with pytest.raises(ValueError, match="shadow"):
        out.optim_step_("sgd", p, m, None, t, 0.1, shadow=torch.zeros(S))


def test_mlp_trains_on_cpu_with_a_fused_optimizer():
    from akka_allreduce_amd.models.mlp import MLP, dp_sgd_step, synthetic_batch
    from akka_allreduce_amd.parallel import ThresholdAllreduce

    gen = torch.Generator().manual_seed(11)
    batches = [synthetic_batch(64, 32, 10, device="cpu", generator=gen)] * 30  # one batch, 30 steps
    torch.manual_seed(0)
    model = MLP(32, 64, 10)
    twin = MLP(32, 64, 10)
    twin.load_state_dict(model.state_dict())
    bucket = GradientBucket(list(model.parameters()), flatten_params=True)
    opt = FusedAdamW(bucket, weight_decay=0.01, max_grad_norm=1.0)
    ar = ThresholdAllreduce(bucket.numel, max_chunk_size=512, device="cpu", rank=0, world_size=1)
    ref = torch.optim.AdamW(twin.parameters(), lr=1e-2, weight_decay=0.01, foreach=False)
    losses, ref_losses = [], []
    for x, y in batches:
        losses.append(dp_sgd_step(model, x, y, 1e-2, ar, optimizer=opt))
        ref.zero_grad()
        loss = torch.nn.functional.cross_entropy(twin(x), y)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), 1.0, foreach=False)
        ref.step()
        ref_losses.append(float(loss.detach()))
    assert losses[-1] < 0.6 * losses[0], losses
    # the same training as torch's AdamW + clip_grad_norm_ (N = 1: every count is 1)
    torch.testing.assert_close(torch.tensor(losses), torch.tensor(ref_losses), rtol=1e-3, atol=1e-4)
    with pytest.raises(ValueError, match="another bucket"):
        dp_sgd_step(model, *batches[0], 1e-2, ar, GradientBucket(list(twin.parameters()), flatten_params=True),
                    optimizer=opt)
