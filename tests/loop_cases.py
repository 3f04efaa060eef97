"""Shapes that reach the streaming kernels' pipelined main loops and the wrap
of a capped grid, with the launch arithmetic that says so.

Every hot kernel has a software-pipelined main loop (several vectors in flight
per thread), a remainder loop and an outer loop that wraps once the grid is
capped.  Which of them a shape reaches is decided by host code; this file
restates that host code in plain Python (each function names the C++ it
mirrors) and declares, per shape, the property the shape is there for.  The GPU
tests call the ``require_*`` helpers before they run, so a later change of
``kMaxGrid`` or of an unroll factor fails loudly instead of silently
un-covering a loop.

Nothing of this is imported from the package; ``test_loop_cases_cpu.py``
compares the constants and the mirrored lines with the sources."""
import math

# csrc/kernels/launch_util.h: kBlock, kCUs, kMaxGrid
K_BLOCK = 256
K_CUS = 256
K_MAX_GRID = K_CUS * 8
# csrc/kernels/counts.hip: kCmUnroll; csrc/kernels/optim.hip: kSqUnroll, the two-unit loop of update_range
CM_UNROLL = 4
SQ_UNROLL = 4
OPTIM_UNROLL = 2
UNIT = 8  # elements per unit of update_range (optim.hip)

# (S, N, C) of every GPU test of the count kernels before this file existed
OLD_SHAPES = [(1, 1, 1), (7, 3, 2), (1003, 4, 67), (100_003, 3, 777), (1_048_576, 8, 4096), (1_048_576, 8, 16_384),
              (1_000_003, 4, 4099), (300_001, 2, 150_000)]

DEEP = (9_700_003, 3, 9395)
SHALLOW = (9_700_003, 3, 1879)
WRAP = (100_003, 8, 37)
SHALLOW_PER_DEEP = 5  # 9395 = 5 * 1879: every DEEP chunk is exactly five SHALLOW chunks


# ---- the geometry (akka_allreduce_amd/data.py: Geometry; the kernels' own region arithmetic) ---------------------------
def geometry(S, N, C):
    """(step, kmax) as Geometry.step / Geometry.kmax give them."""
    step = (S + N - 1) // N
    kmax = 1
    for j in range(N):
        bs = min(j * step, S)
        be = S if j >= N - 1 else min((j + 1) * step, S)
        kmax = max(kmax, -(-(be - bs) // C))
    return step, kmax


def regions(S, N, C):
    """The non-empty regions [s, e) in the order of ``reg``: the head of the region loop that count_expand,
    count_mean (counts.hip), count_optim and count_sqnorm (optim.hip) all spell out."""
    step, kmax = geometry(S, N, C)
    out = []
    for reg in range(N * kmax):
        j, k = divmod(reg, kmax)
        bs = min(j * step, S)
        be = S if j >= N - 1 else min((j + 1) * step, S)
        s = bs + k * C
        if s >= be:
            continue
        out.append((reg, s, min(s + C, be)))
    return out


def body_vectors(s, e, E):
    """nv of the range [s, e) for vectors of E elements: ``a = (s + E - 1) & ~(E - 1); nv = (e - a) / E``."""
    a = min((s + E - 1) & ~(E - 1), e)
    return (e - a) // E


# ---- launch_util.h: region_grid ------------------------------------------------------------------------------------------
def region_grid(nregions, S, max_grid=K_MAX_GRID):
    """(grid, split) of ``region_grid(regions, S, max_grid)``; regions = N * kmax (CountsTable::regions)."""
    grid = min(nregions, max_grid)
    split = max_grid // grid
    per_region_vecs = (S // nregions) // 4 + 1
    useful = (per_region_vecs + K_BLOCK - 1) // K_BLOCK
    split = max(1, min(split, useful))
    return grid, split


def loop_trips(nv, stride, unroll, i0):
    """(main, rest): the trips of ``for (; i + (U - 1) * stride < nv; i += U * stride)`` from ``i = i0`` and of
    the ``for (; i < nv; i += stride)`` behind it -- the loop pair of count_mean_kernel, count_sqnorm_kernel
    (U = 4) and update_range (U = 2)."""
    main, i = 0, i0
    while i + (unroll - 1) * stride < nv:
        main += 1
        i += unroll * stride
    rest = 0
    while i < nv:
        rest += 1
        i += stride
    return main, rest


def walk(S, N, C):
    """The launch of a region walk at (S, N, C): grid, split, the in-region stride and whether the region loop
    takes a second step (``reg += gridDim.x``)."""
    step, kmax = geometry(S, N, C)
    nreg = N * kmax
    grid, split = region_grid(nreg, S)
    return dict(regions=nreg, grid=grid, split=split, stride=K_BLOCK * split, wraps=nreg > grid, kmax=kmax, step=step)


def main_loop_runs(S, N, C, E, unroll):
    """True if any thread of any workgroup runs the pipelined loop at all: thread 0 of blockIdx.y == 0 is the
    first to, in the region with the most vectors."""
    w = walk(S, N, C)
    nv = max(body_vectors(s, e, E) for _, s, e in regions(S, N, C))
    return loop_trips(nv, w["stride"], unroll, 0)[0] > 0


def min_trips_in_full_regions(S, N, C, E, unroll):
    """Over the regions of full length C and every thread of the workgroups that share one: the fewest trips of
    the pipelined loop and the fewest of the remainder loop."""
    w = walk(S, N, C)
    nvs = {body_vectors(s, e, E) for _, s, e in regions(S, N, C) if e - s == C}
    assert nvs, "no region of full length"
    trips = [loop_trips(nv, w["stride"], unroll, i0) for nv in nvs for i0 in range(w["stride"])]
    return min(t[0] for t in trips), min(t[1] for t in trips)


# ---- the guards -----------------------------------------------------------------------------------------------------------
def require_deep():
    """DEEP: one workgroup per region and no wrap, and in every full region EVERY thread runs count_mean's and
    count_sqnorm's four-vector loop at least twice and then the remainder (fp32 vectors), update_range's
    two-unit loop at least twice, and the four-vector loop over 8-element vectors (bf16) at least once; the
    regions start unaligned (C is odd)."""
    S, N, C = DEEP
    w = walk(S, N, C)
    assert (w["regions"], w["split"], w["stride"], w["wraps"]) == (1035, 1, 256, False), w
    for unroll in (CM_UNROLL, SQ_UNROLL):
        main, rest = min_trips_in_full_regions(S, N, C, 4, unroll)
        assert main >= 2 and rest >= 1, (unroll, main, rest)
    assert min_trips_in_full_regions(S, N, C, UNIT, OPTIM_UNROLL)[0] >= 2
    assert min_trips_in_full_regions(S, N, C, 8, CM_UNROLL)[0] >= 1
    assert C % 2 == 1 and any(s % 8 for _, s, _ in regions(S, N, C))
    return w


def require_shallow():
    """SHALLOW: DEEP's blocks, every DEEP chunk exactly five SHALLOW chunks, no pipelined loop of update_range
    anywhere (remainder loops only), and the grid wraps."""
    S, N, C = SHALLOW
    assert (S, N) == DEEP[:2] and DEEP[2] == SHALLOW_PER_DEEP * C
    w = walk(S, N, C)
    assert w["wraps"] and w["split"] == 1, w
    assert not main_loop_runs(S, N, C, UNIT, OPTIM_UNROLL)
    deep = {(s, e) for _, s, e in regions(*DEEP)}
    shallow = regions(S, N, C)
    ends = {e for _, _, e in shallow}
    starts = {s for _, s, _ in shallow}
    assert all(s in starts and e in ends for s, e in deep)  # no SHALLOW chunk straddles a DEEP boundary
    return w


def require_wrap():
    """WRAP: more regions than kMaxGrid, so the region loop of every count kernel takes a second step; the
    regions are heads and tails around a few vectors."""
    S, N, C = WRAP
    w = walk(S, N, C)
    assert w["regions"] == 2704 and w["grid"] == K_MAX_GRID and w["wraps"] and w["split"] == 1, w
    assert K_MAX_GRID < len(regions(S, N, C)) <= 2 * K_MAX_GRID  # some workgroups take two regions, none three
    return w


def shallow_counts(pc_deep):
    """DEEP's per-chunk counts as SHALLOW's: every count five times, so the per-element counts are identical."""
    kmax = geometry(*SHALLOW)[1]
    return pc_deep.repeat_interleave(SHALLOW_PER_DEEP, dim=1)[:, :kmax].contiguous()


# Segment ends for the grouped pass at DEEP.  Region 10 of block 0 is [93_950, 103_345): the cuts at 96_951 and
# 101_052 fall inside its body, none a multiple of 8, and leave sub-ranges of 3001, 4101 and 2293 elements -- 375,
# 511 and 285 units, each more than the stride of 256, so each sub-range runs the two-unit loop and its
# remainder on its own.  The others: a one-element first segment, a cut on a region's end (103_345), one on a
# block's end (3_233_335), short segments inside one region, long ones over many.
DEEP_CUTS = (1, 96_951, 101_052, 103_345, 103_350, 103_361, 2_000_003, 3_233_335, 5_555_555, 6_466_671, 9_700_003)


def require_deep_cuts(cuts=DEEP_CUTS):
    """At least three (region x segment) sub-ranges that are a strict part of one region and run the two-unit
    loop; returns how many there are."""
    S, N, C = DEEP
    assert cuts[-1] == S and list(cuts) == sorted(set(cuts))
    stride = walk(S, N, C)["stride"]
    n, lo = 0, 0
    regs = regions(S, N, C)
    for hi in cuts:
        for _, s, e in regs:
            a, b = max(s, lo), min(e, hi)
            if a < b and (a, b) != (s, e) and loop_trips(body_vectors(a, b, UNIT), stride, OPTIM_UNROLL, 0)[0] > 0:
                n += 1
        lo = hi
    assert n >= 3, n
    return n


# ---- reduce.hip: launch_reduce, launch_lds_n, launch_vec_pol / launch_vec_u ------------------------------------------------
AUTO_LDS_BYTES = 96 << 20


def auto_impl(nsrc, n, es):
    """What ``impl == ReduceImpl::Auto`` becomes in launch_reduce: Lds while sources and output together are at
    most 96 MiB and there are at most 8 sources, else Vec."""
    return "lds" if (nsrc + 1) * n * es <= AUTO_LDS_BYTES and nsrc <= 8 else "vec"


def lds_launch(nvec):
    """launch_lds_n and the tile loop of reduce_lds_kernel: ``grid = min(ceil(tiles / 8), kMaxGrid)`` workgroups
    of four waves, wave w taking the tiles w, w + waves, ...; returns the fewest and the most tiles a wave sums,
    how many waves sum the most, and the vectors of the tail."""
    waves_per_block = K_BLOCK // 64
    tiles = nvec // 64
    want = (tiles + waves_per_block * 2 - 1) // (waves_per_block * 2)
    grid = min(max(want, 1), K_MAX_GRID)
    waves = grid * waves_per_block
    per = [len(range(w, tiles, waves)) for w in range(waves)]
    return dict(tiles=tiles, grid=grid, waves=waves, min_tiles=min(per), max_tiles=max(per),
                at_max=per.count(max(per)), tail=nvec - tiles * 64)


def vec_launch(nsrc, n, es, impl, bpc_env=None):
    """The Vec launch of ``n`` aligned elements of ``es`` bytes: the policy and blocks per CU that launch_reduce
    picks for ``impl`` (``AKKA_VEC_BPC`` = ``bpc_env`` overrides the latter), the UNROLL of launch_vec_pol and the
    grid of launch_vec_u.  ``sweep``: the vectors one pass of the whole grid covers; ``sweeps``: how many passes
    the outer loop of reduce_vec_kernel makes."""
    nvec = n // (16 // es)
    rbytes, wbytes = nsrc * n * es, n * es
    if impl == "vec":
        if rbytes <= 256 << 20:
            pol, bpc = "nts", (64 if nsrc == 1 else 16)
        elif wbytes >= 512 << 20:
            pol, bpc = "both", 2
        else:
            pol, bpc = "ntl", 4
    else:
        pol, bpc = {"vec_nts": ("nts", 16), "vec_both": ("both", 2), "vec_ntl": ("ntl", 8)}[impl]
    if bpc_env is not None:
        bpc = max(1, bpc_env)
    u0 = 4 if nsrc <= 4 else (2 if nsrc <= 8 else 1)
    unroll = (4 if nsrc == 1 else min(u0, 2)) if pol == "both" else u0
    cap = K_CUS * bpc
    want = (nvec + K_BLOCK * unroll - 1) // (K_BLOCK * unroll)
    grid = min(max(want, 1), cap)
    sweep = grid * K_BLOCK * unroll
    return dict(pol=pol, bpc=bpc, unroll=unroll, grid=grid, nvec=nvec, sweep=sweep, sweeps=math.ceil(nvec / sweep))


def ragged_last_sweep(launch):
    """True if in the last sweep some thread has a ``u`` in range and a later ``u`` out of range (UNROLL > 1), or,
    with UNROLL == 1, if the last sweep covers only part of the grid."""
    left = launch["nvec"] - (launch["sweeps"] - 1) * launch["sweep"]  # vectors of the last sweep
    return 0 < left < launch["sweep"]


# The Lds depth: 24 581 tiles on the capped grid of 8192 waves -- three tiles for every wave, so the third
# re-targets the LDS buffer the first was read from; four for five waves; and a tail of 17 vectors.
LDS_NVEC = 64 * (3 * 8192 + 5) + 17


def require_lds_depth(nvec=LDS_NVEC):
    l = lds_launch(nvec)
    assert l["grid"] == K_MAX_GRID and l["min_tiles"] == 3 and l["max_tiles"] == 4 and l["at_max"] == 5, l
    assert l["tail"] == 17, l
    return l


def vec_ragged_nvec(unroll, cus=K_CUS):
    """Two full sweeps of a grid of ``cus`` workgroups (AKKA_VEC_BPC=1) and a ragged third."""
    sweep = cus * K_BLOCK * unroll
    return 2 * sweep + cus * K_BLOCK + 77


def require_vec_sweeps(nsrc, n, es, impl, bpc_env, unroll, grid):
    """The launch has the declared UNROLL and grid, sweeps at least three times and ends ragged."""
    v = vec_launch(nsrc, n, es, impl, bpc_env)
    assert v["unroll"] == unroll and v["grid"] == grid, v
    assert v["sweeps"] >= 3 and ragged_last_sweep(v), v
    return v
