"""The shape table of ``loop_cases.py`` on the CPU: the constants it restates
are the sources', every new shape has the loop property it is declared with,
and no shape the GPU suite had before reached a pipelined loop or wrapped the
grid -- the gap the new shapes close."""
import os
import re

import pytest

import loop_cases as L

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "kernels")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constant(text, name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([^;]+);", text)
    assert m, name
    return m.group(1).strip()


def test_the_constants_are_the_sources():
    util, counts, optim, reduce = (_source(n) for n in ("launch_util.h", "counts.hip", "optim.hip", "reduce.hip"))
    assert int(_constant(util, "kBlock")) == L.K_BLOCK
    assert int(_constant(util, "kCUs")) == L.K_CUS
    assert _constant(util, "kMaxGrid") == "kCUs * 8" and L.K_MAX_GRID == L.K_CUS * 8
    assert int(_constant(counts, "kCmUnroll")) == L.CM_UNROLL
    assert int(_constant(optim, "kSqUnroll")) == L.SQ_UNROLL
    # update_range: 8 elements per unit, two units per trip of the pipelined loop
    assert re.search(r"constexpr int E = 8;\s*// elements per unit", optim)
    assert "for (; i + stride < nv; i += 2 * stride)" in optim and L.OPTIM_UNROLL == 2 and L.UNIT == 8
    # the lines the reduce mirrors restate
    assert "constexpr int U0 = NSRC <= 4 ? 4 : (NSRC <= 8 ? 2 : 1);" in reduce
    assert "constexpr int UNROLL = POL == kBoth ? (NSRC == 1 ? 4 : (U0 < 2 ? U0 : 2)) : U0;" in reduce
    assert "int64_t want = (tiles + kWaves * 2 - 1) / (kWaves * 2);" in reduce
    assert "(rbytes + wbytes <= (int64_t(96) << 20) && sp.nsrc <= 8) ? ReduceImpl::Lds : ReduceImpl::Vec" in reduce
    assert 'std::getenv("AKKA_VEC_BPC")' in reduce


def test_region_grid_of_the_old_shapes():
    """The table of the shapes the suite had: regions, split and stride."""
    want = {(1, 1, 1): (1, 1, 256), (7, 3, 2): (6, 1, 256), (1003, 4, 67): (16, 1, 256),
            (100_003, 3, 777): (129, 1, 256), (1_048_576, 8, 4096): (256, 5, 1280),
            (1_048_576, 8, 16_384): (64, 17, 4352), (1_000_003, 4, 4099): (244, 5, 1280),
            (300_001, 2, 150_000): (4, 74, 18_944)}
    for shape in L.OLD_SHAPES:
        w = L.walk(*shape)
        assert (w["regions"], w["split"], w["stride"]) == want[shape], shape


@pytest.mark.parametrize("S,N,C", L.OLD_SHAPES)
def test_no_old_shape_reaches_a_main_loop_or_wraps(S, N, C):
    assert not L.walk(S, N, C)["wraps"]
    assert not L.main_loop_runs(S, N, C, 4, L.CM_UNROLL)  # count_mean, count_sqnorm: fp32 vectors
    assert not L.main_loop_runs(S, N, C, 8, L.CM_UNROLL)  # the same two over a bf16 sum
    assert not L.main_loop_runs(S, N, C, L.UNIT, L.OPTIM_UNROLL)  # update_range


def test_the_old_shape_lists_are_what_the_table_says():
    """The lists of the GPU files themselves (importing them needs no GPU)."""
    import test_bf16_state_gpu
    import test_fused_optim_gpu
    import test_param_groups_gpu

    shapes = set(test_fused_optim_gpu.SHAPES) | set(test_bf16_state_gpu.SHAPES)
    shapes |= {shape for shape, _ in test_param_groups_gpu.CASES.values()}
    assert shapes <= set(L.OLD_SHAPES), shapes - set(L.OLD_SHAPES)


def test_the_new_shapes_have_their_properties():
    assert L.require_deep()["regions"] == 1035
    assert L.require_shallow()["regions"] == 5163
    assert L.require_wrap()["grid"] == 2048
    assert L.require_deep_cuts() >= 3
    # per region of DEEP: 2348 fp32 vectors, 1173 or 1174 units; of SHALLOW: at most 234 units
    full = [(s, e) for _, s, e in L.regions(*L.DEEP) if e - s == L.DEEP[2]]
    assert {L.body_vectors(s, e, 4) for s, e in full} == {2348}
    assert {L.body_vectors(s, e, 8) for s, e in full} <= {1173, 1174}
    assert max(L.body_vectors(s, e, 8) for _, s, e in L.regions(*L.SHALLOW)) == 234


def test_shallow_counts_expand_to_deeps():
    torch = pytest.importorskip("torch")
    from akka_allreduce_amd.data import Geometry

    S, N, C = L.DEEP
    deep, shallow = Geometry(S, N, C), Geometry(*L.SHALLOW)
    assert (deep.step, deep.kmax) == L.geometry(S, N, C) and (shallow.step, shallow.kmax) == L.geometry(*L.SHALLOW)
    pc = torch.randint(0, N + 1, (N, deep.kmax), dtype=torch.int32, generator=torch.Generator().manual_seed(3))
    assert torch.equal(deep.expand_counts(pc), shallow.expand_counts(L.shallow_counts(pc)))


def test_the_lds_depth():
    l = L.require_lds_depth()
    assert l["tiles"] == 24_581 and l["waves"] == 8192
    # what the suite had: at most two tiles per wave below the capped grid; the 64 MiB case alone went deeper
    for n in (1, 5, 63, 256, 4096 + 3, 1 << 18, 100_003):
        assert L.lds_launch(n // 4)["max_tiles"] <= 2
    assert L.lds_launch((64 << 20) // 16)["min_tiles"] >= 3


def test_auto_at_the_lds_depth():
    """96 MiB is the bound on sources plus output: at 25 MB a source, one and two sources stay on Lds, three and
    eight go to Vec (4 x 25 171 216 B is 21 568 B over)."""
    for es in (4, 2):
        n = L.LDS_NVEC * (16 // es)
        assert [L.auto_impl(k, n, es) for k in (1, 2, 3, 8)] == ["lds", "lds", "vec", "vec"]
    assert L.auto_impl(8, 100_003, 4) == "lds" and L.auto_impl(9, 100_003, 4) == "vec"


@pytest.mark.parametrize("nsrc,impl,unroll", [(1, "vec", 4), (3, "vec_nts", 4), (8, "vec_ntl", 2), (9, "vec", 1),
                                              (16, "vec_ntl", 1), (1, "vec_both", 4), (3, "vec_both", 2),
                                              (8, "vec_both", 2), (16, "vec_both", 1)])
def test_the_vec_sweeps(nsrc, impl, unroll):
    for es in (4, 2):
        n = L.vec_ragged_nvec(unroll) * (16 // es)
        v = L.require_vec_sweeps(nsrc, n, es, impl, 1, unroll, 256)
        assert v["bpc"] == 1
    # without the cap the same size is one sweep or two: the outer loop never got a third
    assert L.vec_launch(nsrc, L.vec_ragged_nvec(unroll) * 4, 4, impl)["sweeps"] <= 2


def test_every_unroll_is_covered():
    got = {(v["pol"] == "both", v["unroll"]) for v in (L.vec_launch(k, 1 << 20, 4, impl, 1) for k in (1, 3, 8, 9, 16)
                                                      for impl in ("vec", "vec_nts", "vec_ntl", "vec_both"))}
    assert got == {(False, 4), (False, 2), (False, 1), (True, 4), (True, 2), (True, 1)}


def test_the_default_grid_vec_both_case():
    n = (2 * 512 * 256 * 2 + 512 * 256 + 77) * 4
    v = L.require_vec_sweeps(2, n, 4, "vec_both", None, 2, 512)
    assert v["pol"] == "both" and v["bpc"] == 2
    # "vec" picks kBoth for outputs of 512 MiB or more alone
    assert L.vec_launch(2, n, 4, "vec")["pol"] == "nts"
    assert L.vec_launch(2, (512 << 20) // 4, 4, "vec")["pol"] == "both"


def test_no_old_reduce_shape_swept_twice():
    for n in (1, 5, 63, 256, 4096 + 3, 1 << 18, 100_003):
        for nsrc in (1, 2, 3, 7, 8, 9, 16):
            assert L.vec_launch(nsrc, n, 4, "vec")["sweeps"] <= 1
