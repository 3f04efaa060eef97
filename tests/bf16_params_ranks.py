"""Rank program for tests/test_bf16_params_ranks_gpu.py: a bucket of bf16
parameters and bf16 gradients, exact rounds of a bf16 engine over the ipc data
plane (every rank on the box's one GPU), and FusedAdamW with bf16 moments.  The
ranks' gradients differ; the round hands both the same sum, and with one seed
both round ``p``, ``m`` and ``v`` alike.  Writes rank<i>.pt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    rank = int(os.environ["RANK"])
    dist.init_process_group("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from akka_allreduce_amd.parallel import FusedAdamW, ThresholdAllreduce
    from akka_allreduce_amd.parallel.dp import GradientBucket

    bf = torch.bfloat16
    g0 = torch.Generator().manual_seed(0)  # identical parameters on every rank
    ps = [torch.nn.Parameter(torch.randn(n, generator=g0).to(dev).to(bf)) for n in (20_000, 60, 12_345, 3)]
    bucket = GradientBucket(ps, flatten_params=True)
    assert bucket.pflat.dtype == bf and bucket.flat.dtype == bf
    opt = FusedAdamW(bucket, weight_decay=0.01, max_grad_norm=1.0, state_dtype=bf, seed=11)
    ar = ThresholdAllreduce(bucket.numel, max_chunk_size=1 << 12, dtype=bf, device=dev, data_plane="ipc")
    p0 = bucket.pflat.detach().clone()
    sums = []
    for s in range(a.steps):
        g = torch.Generator().manual_seed(1000 * s + rank + 1)
        bucket.flat.copy_(torch.randn(bucket.numel, generator=g).to(dev))
        mine = bucket.flat.clone()
        out = opt.step_from(ar, 1e-2)
        sums.append((mine.cpu(), out.data.detach().cpu()))
    torch.cuda.synchronize()
    torch.save({"p0": p0.cpu(), "p": bucket.pflat.detach().cpu(), "m": opt.m.cpu(), "v": opt.v.cpu(), "t": int(opt.t),
                "mine": [x for x, _ in sums], "sums": [y for _, y in sums], "ipc_error": ar.ipc_error()},
               os.path.join(a.out_dir, f"rank{rank}.pt"))
    ar.retire()
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
