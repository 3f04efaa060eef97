"""Rank program for tests/test_skip_nonfinite_ranks_gpu.py: the MLP's DP step
with a guarded fused AdamW update (``skip_nonfinite=True``, global-norm clip
on) over the one-sided allreduce, every rank on the box's one GPU.  Rank 1's
batch holds an inf at step 2 and a NaN at step 4: both ranks must skip those
two rounds.  Run eager and as the WHOLE step in one graph replay, against the
unguarded eager run over the four clean batches.  Writes rank<i>.pt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

BAD = {2: float("inf"), 4: float("nan")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--steps", type=int, default=6)
    a = ap.parse_args()
    rank = int(os.environ["RANK"])
    dist.init_process_group("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from akka_allreduce_amd.models.mlp import MLP, GraphedDPStep, dp_sgd_step, synthetic_batch
    from akka_allreduce_amd.parallel import FusedAdamW
    from akka_allreduce_amd.parallel.dp import GradientBucket
    from akka_allreduce_amd.parallel.onesided import OneSidedAllreduce

    cdt, lr = torch.bfloat16, 1e-2

    def batches(clean_only=False):
        for s in range(a.steps):
            if clean_only and s in BAD:
                continue
            g = torch.Generator(device=dev).manual_seed(1000 * s + rank)
            x, y = synthetic_batch(32, 64, 10, device=dev, generator=g)
            if s in BAD and rank == 1:
                x[5, 7] = BAD[s]
            yield x, y

    def fresh(guard):
        torch.manual_seed(0)
        m = MLP(64, 128, 10).to(dev)
        b = GradientBucket(list(m.parameters()), flatten_params=True)
        return m, b, FusedAdamW(b, weight_decay=0.01, max_grad_norm=1.0, **({"skip_nonfinite": True} if guard else {}))

    def result(prefix, b, o):
        d = {prefix: b.pflat.cpu(), prefix + "_m": o.m.cpu(), prefix + "_v": o.v.cpu(),
             prefix + "_shadow": b.sflat.cpu(), prefix + "_t": int(o.t)}
        if o.guard is not None:
            d[prefix + "_record"] = o.guard.tolist()
        return d

    # the four clean batches, unguarded
    m0, b0, o0 = fresh(False)
    ar = OneSidedAllreduce(b0.numel, max_chunk_size=1 << 12, device=dev)
    for x, y in batches(clean_only=True):
        dp_sgd_step(m0, x, y, lr, ar, b0, sync_loss=False, compute_dtype=cdt, optimizer=o0)

    # all six, guarded, eager
    m1, b1, o1 = fresh(True)
    for x, y in batches():
        dp_sgd_step(m1, x, y, lr, ar, b1, sync_loss=False, compute_dtype=cdt, optimizer=o1)

    # all six, guarded, the whole step one graph replay
    m2, b2, o2 = fresh(True)
    x0, y0 = next(batches())
    gs = GraphedDPStep(m2, b2, x0, y0, compute_dtype=cdt, allreduce=ar, lr=lr, optimizer=o2)
    after_capture = (int(o2.t), o2.guard.tolist())  # the warmup's steps and their record were put back
    sx, sy = gs.static_inputs()
    for x, y in batches():
        sx.copy_(x)
        sy.copy_(y)
        gs(sx, sy, lr, None)
    torch.cuda.synchronize()
    torch.save({**result("clean", b0, o0), **result("eager", b1, o1), **result("graphed", b2, o2),
                "after_capture_t": after_capture[0], "after_capture_record": after_capture[1],
                "replays": gs.replays, "error": ar.error()}, os.path.join(a.out_dir, f"rank{rank}.pt"))
    ar.retire()
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
