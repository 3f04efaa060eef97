"""bf16 moments with stochastic rounding on the CPU: the torch path of
``optim_step_`` against the definition at the top of the bf16 code in
``csrc/kernels/optim.hip``, the drift a nearest rounding would show, the
rounding bits across steps and seeds, non-finite values, and the optimizers'
interface.

``_bits`` / ``_sr`` are the tests' own copy of that definition
(``optim_cases.py``: numpy, uint32 arithmetic that wraps), written from the
documentation; nothing of it is imported from the package."""
import numpy as np
import pytest
import torch

from akka_allreduce_amd.data import AllReduceOutput, Geometry, OptimGroups
from akka_allreduce_amd.parallel import FusedAdamW, FusedSGD
from optim_cases import BF, H_SENTINEL, HYPER, _bits, _bucket, _same_bits, _sr

M_SENTINEL, V_SENTINEL = 123.0, 77.5  # bf16-representable
SHAPES = [(1, 1, 1), (7, 3, 2), (1003, 4, 67)]

def _inputs(S, N, C, src):
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
        sums.append(torch.where(missing, base, base * count).to(BF if src == "bf16" else torch.float32))
    p0 = torch.randn(S, generator=g)
    m0 = torch.where(missing, torch.full((S,), M_SENTINEL), 0.1 * torch.randn(S, generator=g)).to(BF)
    v0 = torch.where(missing, torch.full((S,), V_SENTINEL), 0.01 * torch.rand(S, generator=g)).to(BF)
    return geo, pc, missing, sums, p0, m0, v0


def _groups(S):
    # two groups over four segments at S = 1003; group 1 has lr 0: its state advances and its p stays
    ends, owner = ([5, 130, 771, 1003], [0, 1, 0, 1]) if S == 1003 else ([S], [0])
    g = OptimGroups(ends, owner, 2, "cpu")
    return g


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("src", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["sgd", "nesterov", "adamw"])
@pytest.mark.parametrize("S,N,C", SHAPES)
def test_torch_path_is_the_fp32_path_then_sr(S, N, C, kind, src, grouped):
    geo, pc, missing, sums, p0, m0, v0 = _inputs(S, N, C, src)
    adam = kind == "adamw"
    h = dict(HYPER[kind])
    lr = h.pop("lr")
    groups = None
    if grouped:
        groups = _groups(S)
        groups.write_rows(OptimGroups.row_values(lr, [(1.0, h["weight_decay"]), (0.0, 0.1)]))
    seed = 5
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    sh = torch.full((S,), H_SENTINEL, dtype=BF)
    t = torch.zeros(1, dtype=torch.int32)
    for step in range(3):
        out = AllReduceOutput(sums[step], counts_per_chunk=pc, geometry=geo)
        t.add_(1)
        # the fp32 path from the widened state
        pr, mr, vr, shr = p.clone(), m.float(), v.float(), sh.clone()
        out.optim_step_("adamw" if adam else "sgd", pr, mr, vr if adam else None, t, lr, shadow=shr, groups=groups,
                        **h)
        out = AllReduceOutput(sums[step], counts_per_chunk=pc, geometry=geo)
        out.optim_step_("adamw" if adam else "sgd", p, m, v if adam else None, t, lr, shadow=sh, groups=groups,
                        seed=seed, **h)
        assert m.dtype == BF and v.dtype == BF
        r_m, r_v = _bits(S, step + 1, seed)
        assert _same_bits(p, pr), f"p at step {step + 1}"
        assert _same_bits(sh, shr), f"shadow at step {step + 1}"
        assert _same_bits(m, _sr(mr, r_m)), f"m at step {step + 1}"
        if adam:
            assert _same_bits(v, _sr(vr, r_v)), f"v at step {step + 1}"
        else:
            assert _same_bits(v, v0)
        # count-0 elements keep everything
        assert torch.equal(p[missing], p0[missing])
        assert bool((m[missing].float() == M_SENTINEL).all()) and bool((v[missing].float() == V_SENTINEL).all())
        assert bool((sh[missing].float() == H_SENTINEL).all())
    if S > 1:
        live = ~missing
        assert not torch.equal(m[live], m0[live])
        if grouped and S == 1003:
            still = torch.zeros(S, dtype=torch.bool)
            still[5:130] = still[771:] = True
            assert torch.equal(p[still], p0[still]) and not torch.equal(m[still & live], m0[still & live])


def _drift_run(state_dtype, S=4096, steps=1000):
    geo = Geometry(S, 1, S)
    pc = torch.ones((1, 1), dtype=torch.int32)
    out = AllReduceOutput(torch.ones(S), counts_per_chunk=pc, geometry=geo)
    p, m, v = torch.zeros(S), torch.zeros(S, dtype=state_dtype), torch.zeros(S, dtype=state_dtype)
    t = torch.zeros(1, dtype=torch.int32)
    for _ in range(steps):
        t.add_(1)
        out.optim_step_("adamw", p, m, v, t, 1e-3, betas=(0.9, 0.999), weight_decay=0.0)
    return v.float()


def test_v_does_not_stall():
    """g = 1, beta2 = 0.999, 1000 steps: fp32 v reaches 0.632; a bf16 v rounded to nearest stalls at 0.25.  The
    mean over 4096 elements is within 1 % of the fp32 run (emulated: +0.06 %; one element is within 11 %, so 1 %
    is about 20 standard deviations of the mean), and above 0.5, which a missing or constant r does not reach."""
    v32 = _drift_run(torch.float32)
    assert bool((v32 == v32[0]).all()) and abs(float(v32[0]) - 0.6323) < 1e-3
    vbf = _drift_run(BF)
    mean = float(vbf.double().mean())
    print(f"DRIFT cpu fp32={float(v32[0]):.6f} bf16_mean={mean:.6f} rel={mean / float(v32[0]) - 1:+.3e} "
          f"worst_elem={float((vbf / v32[0] - 1).abs().max()):.3e}")
    assert mean > 0.5
    assert abs(mean - float(v32[0])) <= 0.01 * float(v32[0])


def _decisions(t_value, seed, S=4096):
    """Which elements round up when every fp32 m' sits exactly half way between two bf16 values: the top bit
    of r_m.  SGD with momentum 0 and no decay makes m' the mean gradient itself."""
    geo = Geometry(S, 1, S)
    pc = torch.ones((1, 1), dtype=torch.int32)
    half = torch.from_numpy(np.full(S, 0x3F808000, np.uint32).view(np.float32).copy())  # 1 + 2**-8
    out = AllReduceOutput(half, counts_per_chunk=pc, geometry=geo)
    p, m = torch.zeros(S), torch.zeros(S, dtype=BF)
    t = torch.full((1,), t_value, dtype=torch.int32)
    out.optim_step_("sgd", p, m, None, t, 0.1, momentum=0.0, weight_decay=0.0, seed=seed)
    up = m.float() > 1.0
    assert bool(((m.float() == 1.0) | (m.float() == 1.0078125)).all())
    return up


def test_bits_differ_between_steps_and_seeds_and_not_between_optimizers():
    d = {(t, s): _decisions(t, s) for t in (1, 2, 3) for s in (0, 1)}
    for (t, s), up in d.items():
        r_m, _ = _bits(4096, t, s)
        assert torch.equal(up, torch.from_numpy(r_m >= 0x8000)), (t, s)
        assert 0.4 < float(up.float().mean()) < 0.6  # 4096 fair bits: 0.5 +- 0.008
    for a, b in (((1, 0), (2, 0)), ((2, 0), (3, 0)), ((1, 0), (3, 0)), ((1, 0), (1, 1)), ((2, 0), (2, 1))):
        assert not torch.equal(d[a], d[b]), (a, b)
    assert torch.equal(_decisions(2, 1), d[(2, 1)])

    # two optimizers with one seed give the same bits; another seed gives others
    def run(seed):
        b = _bucket()
        opt = FusedAdamW(b, state_dtype=BF, seed=seed)
        ar = _OneContributor(b.numel)
        for i in range(3):
            b.flat.copy_(torch.randn(b.numel, generator=torch.Generator().manual_seed(10 + i)))
            opt.step_from(ar, 1e-2)
        return b.pflat.clone(), opt.m.clone(), opt.v.clone()

    a, b, c = run(0), run(0), run(1)
    assert all(_same_bits(x, y) for x, y in zip(a, b))
    assert not _same_bits(a[1], c[1]) and not _same_bits(a[2], c[2])


def test_non_finite_and_extreme_values():
    from akka_allreduce_amd.data import sr_bf16

    big = float(np.finfo(np.float32).max)
    x = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 1e-40, -1e-40, big, -big])
    for r in (0, 0x8000, 0xFFFF):
        for got in (sr_bf16(x, torch.full((9,), r, dtype=torch.int64)), _sr(x, np.full(9, r, np.uint32))):
            assert got.dtype == BF
            f = got.float()
            assert bool(torch.isnan(f[0])) and not bool(torch.isnan(f[1:]).any())
            assert float(f[1]) == float("inf") and float(f[2]) == float("-inf")
            assert torch.equal(torch.signbit(f[1:]), torch.signbit(x[1:]))  # no sign flips
            assert float(f[3]) == 0.0 and float(f[4]) == 0.0
        assert _same_bits(sr_bf16(x, torch.full((9,), r, dtype=torch.int64))[1:], _sr(x, np.full(9, r, np.uint32))[1:])
    top = sr_bf16(x, torch.full((9,), 0xFFFF, dtype=torch.int64)).float()
    assert float(top[7]) == float("inf") and float(top[8]) == float("-inf")  # past the largest bf16, as under RNE
    assert abs(float(top[5])) <= 2e-40 and abs(float(top[6])) <= 2e-40
    # through the pass: a NaN or inf gradient reaches m as NaN or inf, whatever the bits
    geo = Geometry(9, 1, 9)
    out = AllReduceOutput(x.clone(), counts_per_chunk=torch.ones((1, 1), dtype=torch.int32), geometry=geo)
    p, m = torch.zeros(9), torch.zeros(9, dtype=BF)
    out.optim_step_("sgd", p, m, None, torch.ones(1, dtype=torch.int32), 0.1, momentum=0.0, seed=3)
    f = m.float()
    assert bool(torch.isnan(f[0])) and float(f[1]) == float("inf") and float(f[2]) == float("-inf")
    assert not bool(torch.isnan(f[3:]).any())


class _OneContributor:
    """A round of one contributor: the sum is the input, every count is 1."""

    def __init__(self, S, C=64):
        self.geometry = Geometry(S, 1, C)
        self.counts = torch.ones((1, self.geometry.kmax), dtype=torch.int32)

    def __call__(self, t, out=None):
        return AllReduceOutput(t.clone(), counts_per_chunk=self.counts, geometry=self.geometry)


def _steps(b, opt, ar, which):
    for i in which:
        b.flat.copy_(torch.randn(b.numel, generator=torch.Generator().manual_seed(100 + i)))
        opt.step_from(ar, 1e-2)


@pytest.mark.parametrize("cls", [FusedSGD, FusedAdamW])
def test_state_dict_round_trips_within_and_across_state_dtypes(cls):
    b1 = _bucket()
    o1, ar = cls(b1, state_dtype=BF, seed=9), _OneContributor(b1.numel)
    assert o1.m.dtype == BF and (o1.v is None or o1.v.dtype == BF)
    assert len(o1.state_tensors()) == (3 if o1.v is not None else 2) and len(o1.state_pointers()) == 4
    _steps(b1, o1, ar, range(3))
    saved, p_saved = o1.state_dict(), b1.pflat.clone()
    assert saved["state_dtype"] == BF and saved["seed"] == 9 and saved["m"].dtype == BF
    _steps(b1, o1, ar, range(3, 5))

    # same dtype: the run continues bit for bit, nothing moves
    b2 = _bucket()
    o2 = cls(b2, state_dtype=BF, seed=9)
    with torch.no_grad():
        b2.pflat.copy_(p_saved)
    ptrs = o2.state_pointers()
    o2.load_state_dict(saved)
    assert o2.state_pointers() == ptrs and int(o2.t) == 3
    _steps(b2, o2, ar, range(3, 5))
    assert _same_bits(b1.pflat, b2.pflat) and _same_bits(o1.m, o2.m)
    if o1.v is not None:
        assert _same_bits(o1.v, o2.v)

    # bf16 into fp32 state: exact
    o3 = cls(_bucket(), seed=9)
    ptrs = o3.state_pointers()
    o3.load_state_dict(saved)
    assert o3.state_pointers() == ptrs and o3.m.dtype == torch.float32 and torch.equal(o3.m, saved["m"].float())
    if o3.v is not None:
        assert torch.equal(o3.v, saved["v"].float())

    # fp32 into bf16 state: rounded to nearest, once
    b4 = _bucket()
    o4 = cls(b4, seed=9)
    _steps(b4, o4, ar, range(2))
    d32 = o4.state_dict()
    assert d32["state_dtype"] == torch.float32 and d32["m"].dtype == torch.float32
    o5 = cls(_bucket(), state_dtype=BF, seed=9)
    o5.load_state_dict(d32)
    assert _same_bits(o5.m, d32["m"].to(BF)) and int(o5.t) == 2
    if o5.v is not None:
        assert _same_bits(o5.v, d32["v"].to(BF))

    # the seed is a launch argument; a dict from before the seed existed was saved with 0
    with pytest.raises(ValueError, match="seed"):
        cls(_bucket(), state_dtype=BF, seed=8).load_state_dict(saved)
    old = {k: x for k, x in d32.items() if k not in ("seed", "state_dtype")}
    with pytest.raises(ValueError, match="seed"):
        cls(_bucket(), seed=9).load_state_dict(old)
    cls(_bucket(), seed=0).load_state_dict(old)
    # any other dtype of m or v raises
    bad = dict(saved, m=saved["m"].to(torch.float16))
    with pytest.raises(ValueError, match="float16"):
        cls(_bucket(), state_dtype=BF, seed=9).load_state_dict(bad)


def test_wrong_arguments_raise():
    for cls in (FusedSGD, FusedAdamW):
        for bad in (torch.float16, torch.float64, torch.int32, "bfloat16"):
            with pytest.raises(ValueError, match="state_dtype"):
                cls(_bucket(), state_dtype=bad)
        for bad in (-1, 1 << 32, 1.5):
            with pytest.raises(ValueError, match="seed"):
                cls(_bucket(), state_dtype=BF, seed=bad)
    S = 16
    geo = Geometry(S, 1, S)
    out = AllReduceOutput(torch.ones(S), counts_per_chunk=torch.ones((1, 1), dtype=torch.int32), geometry=geo)
    p, t = torch.zeros(S), torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="agree"):
        out.optim_step_("adamw", p, torch.zeros(S, dtype=BF), torch.zeros(S), t, 1e-3)
    with pytest.raises(ValueError, match="agree"):
        out.optim_step_("adamw", p, torch.zeros(S), torch.zeros(S, dtype=BF), t, 1e-3)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        out.optim_step_("sgd", p, torch.zeros(S, dtype=torch.float16), None, t, 1e-3)
    with pytest.raises(ValueError, match="nt"):
        out.optim_step_("adamw", p, torch.zeros(S, dtype=BF), torch.zeros(S, dtype=BF), t, 1e-3, nt=True)
    with pytest.raises(ValueError, match="seed"):
        out.optim_step_("sgd", p, torch.zeros(S, dtype=BF), None, t, 1e-3, seed=1 << 32)
    assert torch.equal(p, torch.zeros(S))
