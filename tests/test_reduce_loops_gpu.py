"""The chunk sum (``reduce.hip``) where its loops go round: a wave's third and
fourth LDS tile, a second and a ragged third sweep of the Vec grid, every
UNROLL and every named cache policy -- at sizes the launch arithmetic mirrored
in ``loop_cases.py`` says reach them.

The data depends on the position and is exact: source ``s`` holds
``((i * (2 s + 3) + 7 s) mod 251) - 125`` at element ``i``.  Every value is
exact in bf16 and every partial sum (at most 16 x 125) in fp32, so the result
is the int64 sum rounded once to the dtype, whatever the order -- and a
misplaced, stale or dropped vector changes it."""
import functools
import math

import pytest
import torch

import loop_cases as L
from akka_allreduce_amd.ops import chunk_reduce

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DTYPES = [torch.float32, BF]
PER_VEC = {torch.float32: 4, BF: 8}
ES = {torch.float32: 4, BF: 2}


def _dev():
    return torch.device("cuda", 0)


def _pattern(n, nsrc, first=0):
    """int64 [nsrc, n]: the sources ``first`` .. ``first + nsrc - 1``."""
    i = torch.arange(n, dtype=torch.int64, device=_dev())
    return torch.stack([(i * (2 * s + 3) + 7 * s) % 251 - 125 for s in range(first, first + nsrc)])


@functools.lru_cache(maxsize=2)
def _exact(n, nsrc, dtype):
    """``nsrc`` sources of ``n`` elements and the expected sum of the first k of them, k = 1 .. nsrc."""
    ints = _pattern(n, nsrc)
    srcs = [row.to(dtype) for row in ints]
    assert all(torch.equal(s.to(torch.int64), row) for s, row in zip(srcs, ints))  # exact in the dtype
    want = [w.to(torch.float32).to(dtype) for w in ints.cumsum(0)]  # |sum| <= 2000: exact in fp32, rounded once
    torch.cuda.synchronize()
    return srcs, want


def _check(n, nsrc, dtype, impl, most=None):
    srcs, want = _exact(n, most or nsrc, dtype)
    out = torch.full((n,), 7.0, dtype=dtype, device=_dev())
    assert chunk_reduce(srcs[:nsrc], out=out, impl=impl) is out
    assert torch.equal(out, want[nsrc - 1]), (impl, nsrc, n)


# ---- Lds ------------------------------------------------------------------------------------------------------------------
# the topmost parameter varies fastest: the cases of one (dtype, rest) share their eight sources
@pytest.mark.parametrize("impl", ["lds", "auto"])
@pytest.mark.parametrize("nsrc", [1, 2, 3, 8])
@pytest.mark.parametrize("rest", [0, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lds_third_tile_and_tail(dtype, rest, nsrc, impl):
    """Three tiles for every wave on the capped grid (the third re-targets the buffer the first was read from),
    four for five waves, a 17-vector tail; ``rest``: elements behind the last vector, for the scalar kernel.

    ``auto`` is Lds while sources and output together are at most 96 MiB: at this depth (25 MB a source) that
    holds for one and two sources; three (21 568 B over) and eight go to Vec's default grid, and run here as such."""
    L.require_lds_depth()
    n = L.LDS_NVEC * PER_VEC[dtype] + rest
    if impl == "auto":
        assert L.auto_impl(nsrc, n, ES[dtype]) == ("lds" if nsrc <= 2 else "vec")
    _check(n, nsrc, dtype, impl, most=8)


@pytest.mark.parametrize("dtype", DTYPES)
def test_lds_depth_behind_a_common_misalignment(dtype):
    """Every pointer one element past a 16-B boundary: block 0 sums the peeled head, the body is the Lds depth."""
    per, nsrc = PER_VEC[dtype], 3
    head = per - 1
    n = head + L.LDS_NVEC * per + 2
    L.require_lds_depth((n - head) // per)
    ints = _pattern(n + 16, nsrc)
    base = [row.to(dtype) for row in ints]
    srcs = [b[1:1 + n] for b in base]
    assert all(s.data_ptr() % 16 == ES[dtype] for s in srcs)
    out_base = torch.full((n + 16,), 7.0, dtype=dtype, device=_dev())
    out = out_base[1:1 + n]
    chunk_reduce(srcs, out=out, impl="lds")
    assert torch.equal(out, ints.sum(0)[1:1 + n].to(torch.float32).to(dtype))
    assert float(out_base[0]) == 7.0 and bool((out_base[1 + n:] == 7.0).all())  # nothing outside the view


# ---- Vec ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["vec", "vec_nts", "vec_ntl", "vec_both"])
@pytest.mark.parametrize("nsrc", [1, 3, 8, 9, 16])
@pytest.mark.parametrize("dtype", DTYPES)
def test_vec_sweeps_on_a_capped_grid(monkeypatch, dtype, nsrc, impl):
    """One workgroup per CU (the launcher reads AKKA_VEC_BPC on every call): two full sweeps of the grid and a
    ragged third, in which a thread's first ``u`` is in range and a later one is not.  The source counts cover
    every UNROLL: 4, 2 and 1, and kBoth's 4 (one source) and 2."""
    monkeypatch.setenv("AKKA_VEC_BPC", "1")
    unroll = L.vec_launch(nsrc, 1 << 20, ES[dtype], impl, 1)["unroll"]
    n = L.vec_ragged_nvec(unroll) * PER_VEC[dtype]
    L.require_vec_sweeps(nsrc, n, ES[dtype], impl, 1, unroll, L.K_CUS)
    _check(n, nsrc, dtype, impl)


@pytest.mark.parametrize("dtype", DTYPES)
def test_vec_both_on_its_default_grid(dtype):
    """kBoth by name with no knob set: 512 workgroups, UNROLL 2, two full sweeps and a ragged third."""
    n = (2 * 512 * 256 * 2 + 512 * 256 + 77) * PER_VEC[dtype]
    v = L.require_vec_sweeps(2, n, ES[dtype], "vec_both", None, 2, 512)
    assert v["pol"] == "both"
    _check(n, 2, dtype, "vec_both")


# ---- bf16: source counts and launchers the suite had not run ---------------------------------------------------------------
def _bf16_want(srcs):
    """fp32 accumulation in source order, rounded once per pass; more than 16 sources are summed in passes of 16
    (``split_reduce``: the output of a pass is the first source of the next)."""
    acc = torch.zeros_like(srcs[0], dtype=torch.float32)
    left = list(srcs)
    for s in left[:16]:
        acc += s.float()
    left = left[16:]
    while left:
        acc = acc.to(BF).float()
        for s in left[:15]:
            acc += s.float()
        left = left[15:]
    return acc.to(BF)


OLD_BF16 = {(impl, nsrc) for impl in ("vec", "lds") for nsrc in (1, 2, 4, 8, 16)}
NEW_BF16 = [(impl, nsrc) for nsrc in (1, 2, 3, 4, 7, 8, 9, 16, 17, 23) for impl in ("vec", "lds", "scalar", "auto")
            if (impl, nsrc) not in OLD_BF16]


@pytest.mark.parametrize("impl,nsrc", NEW_BF16)
@pytest.mark.parametrize("n", [7, 1024, 100_003])
def test_chunk_reduce_bf16_more_counts_and_launchers(n, impl, nsrc):
    g = torch.Generator(device=_dev()).manual_seed(nsrc + n)
    srcs = [torch.randn(n, device=_dev(), generator=g).bfloat16() for _ in range(nsrc)]
    got = chunk_reduce(srcs, impl=impl)
    assert torch.equal(got, _bf16_want(srcs))


# ---- one source: what comes through bit for bit ----------------------------------------------------------------------------
def _bits(x):
    return x.view(torch.int16 if x.dtype == BF else torch.int32)


def _specials(dtype, n):
    """A position-dependent buffer with -0.0 and a NaN with a payload in the first vector, the middle and the end."""
    x = _pattern(n, 1)[0].to(dtype)
    nan = torch.tensor([0x7FC1 if dtype == BF else 0x7FC12345], dtype=torch.int32).to(_bits(x).dtype).to(_dev())
    for at in (1, n // 2, n - 2):
        x[at] = -0.0
        _bits(x)[at + 1] = nan[0]
    return x


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_source_through_vec_is_a_copy_bit_for_bit(dtype):
    """The Vec body hands a lone source's vectors through untouched: -0.0 and a NaN's payload survive."""
    n = 4096 * PER_VEC[dtype]
    x = _specials(dtype, n)
    for impl in ("vec", "vec_nts", "vec_ntl", "vec_both"):
        got = chunk_reduce([x], impl=impl)
        assert torch.equal(_bits(got), _bits(x)), impl


@pytest.mark.parametrize("impl", ["lds", "scalar", "auto"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_source_through_the_adding_paths(dtype, impl):
    """Lds, the scalar kernel, the peeled head and the scalar rest have no one-source case: they add the source
    to +0.0, as for any other count.  Every value comes out equal, a NaN as a NaN; the sign of -0.0 is not kept
    (+0.0 + -0.0 is +0.0) -- the comment in reduce.hip promises bits for the Vec body alone."""
    n = (64 * 9 + 17) * PER_VEC[dtype] + 3
    x = _specials(dtype, n)
    got = chunk_reduce([x], impl=impl)
    nan = torch.isnan(x)
    assert int(nan.sum()) == 3 and torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan], x[~nan])
    ordinary = ~nan & (x != 0)
    assert torch.equal(_bits(got)[ordinary], _bits(x)[ordinary])


# ---- non-finite values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["vec", "lds", "auto", "scalar"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_infinities_and_nans_come_out_as_torchs_sum_gives_them(dtype, impl):
    """+inf, -inf, a NaN and inf + -inf in the peeled head, the body, the last tile, the tail behind the tiles
    and the scalar rest, of three sources one element past a 16-B boundary."""
    per, nsrc = PER_VEC[dtype], 3
    head, tiles, tail, rest = per - 1, 5, 17, 3
    n = head + (64 * tiles + tail) * per + rest
    base = [row.to(dtype) for row in _pattern(n + 16, nsrc) % 9]
    srcs = [b[1:1 + n] for b in base]
    zones = {"head": 0, "body": head + 64 * per + 5, "last tile": head + 64 * (tiles - 1) * per + 9,
             "tail": head + 64 * tiles * per + 2, "rest": n - rest}
    for z in zones.values():
        srcs[0][z] = math.inf
        srcs[1][z + 1] = -math.inf
        srcs[2][z + 2] = math.nan
        if z + 3 < n and z != 0:
            srcs[0][z + 3], srcs[1][z + 3] = math.inf, -math.inf
    out_base = torch.empty(n + 16, dtype=dtype, device=_dev())
    out = out_base[1:1 + n]
    chunk_reduce(srcs, out=out, impl=impl)
    want = torch.stack([s.float() for s in srcs]).sum(0).to(dtype)
    assert int(torch.isnan(want).sum()) >= 8 and int(torch.isinf(want).sum()) >= 10
    assert torch.equal(torch.isnan(out), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(out.float(), nan=0.0), torch.nan_to_num(want.float(), nan=0.0))
