"""Rank program for tests/test_codec_gpu.py (torch.distributed.run, 2 ranks on
the box's one GPU): one bf16 round on an exact ipc lane and one on the
one-sided lane per buffer size, each compared bit for bit with the standalone
reduce kernels (ops.chunk_reduce: vec, lds, scalar) over the same two inputs.
Every rank generates both ranks' inputs from the seed.  Writes rank<i>.json."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

# bf16 bit patterns (x0, x1) whose fp32 sum is a rounding edge
PAIRS = [
    (0x3F80, 0x3B80),  # 1 + 2^-8: an exact tie, to even = down
    (0x3F81, 0x3B80),  # (1 + 2^-7) + 2^-8: an exact tie, to even = up
    (0xBF80, 0xBB80),  # the same two, negative
    (0xBF81, 0xBB80),
    (0x7F7F, 0x7F7F),  # max + max: the fp32 sum overflows
    (0x7F7F, 0x7B00),  # max + 2^119: a finite fp32 sum that rounds to inf
    (0xFF7F, 0xFB00),
    (0x0001, 0x0001),  # smallest subnormals
    (0x007F, 0x0001),  # largest subnormal + smallest: the smallest normal
    (0x8000, 0x8000),  # -0 + -0
    (0x7F80, 0xFF80),  # inf + -inf
    (0x7FC0, 0x3F80),  # a NaN input, either side, quiet and signalling
    (0x3F80, 0x7FA1),
]
PERIOD = 32  # the table sits at the head of every 32 elements, randn between
SCALES = [-120, -60, -8, 0, 8, 60, 120]  # randn times 2^k


def inputs(size: int, seed: int):
    """x0, x1: bf16 CPU tensors of `size` elements, the same on every rank."""
    g = torch.Generator().manual_seed(seed)
    k = torch.tensor(SCALES, dtype=torch.float32)[torch.randint(len(SCALES), (2, size), generator=g)]
    x = (torch.randn(2, size, generator=g) * torch.exp2(k)).to(torch.bfloat16)
    bits = x.view(torch.int16)  # the patterns go in as bits: no conversion touches a NaN's payload
    table = np.array(PAIRS, dtype=np.uint16).view(np.int16)
    for p in range(len(PAIRS)):
        bits[0, p::PERIOD] = int(table[p, 0])
        bits[1, p::PERIOD] = int(table[p, 1])
    return x[0].contiguous(), x[1].contiguous()


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Same bits (-0 is not +0), any NaN equal to any NaN."""
    a, b = a.cpu(), b.cpu()
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and torch.equal(a.view(torch.int16)[~nan], b.view(torch.int16)[~nan])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--sizes", default="8192,8198")
    ap.add_argument("--lanes", default="ipc_fused_lite,onesided")
    a = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    assert world == 2
    dist.init_process_group("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from akka_allreduce_amd.ops import chunk_reduce
    from akka_allreduce_amd.parallel import ThresholdAllreduce

    res = {"rank": rank, "rounds": []}
    engines = []
    for size in [int(s) for s in a.sizes.split(",")]:
        xs = [x.to(dev) for x in inputs(size, 1234 + size)]
        refs = {impl: chunk_reduce(xs, impl=impl) for impl in ("vec", "lds", "scalar")}
        ar = ThresholdAllreduce(size, max_chunk_size=2048, dtype=torch.bfloat16, device=dev, data_plane="ipc")
        engines.append(ar)
        for lane in a.lanes.split(","):
            ar.use_lane(lane)
            o = ar(xs[rank])
            torch.cuda.synchronize()
            res["rounds"].append({
                "size": size, "lane": lane, "state_lane": ar.state()["link"].get("lane"),
                "counts_ok": bool((o.count.cpu() == world).all()),
                "nan": int(torch.isnan(o.data).sum()), "inf": int(torch.isinf(o.data).sum()),
                "equal": {impl: bits_equal(o.data, ref) for impl, ref in refs.items()},
            })
        res["ipc_error"] = res.get("ipc_error", 0) or ar.ipc_error()
    with open(os.path.join(a.out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(res, f)
    # every rank's kernels have drained before any window is released
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
