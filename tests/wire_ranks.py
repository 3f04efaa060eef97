"""Rank program for tests/test_wire_bf16_gpu.py (torch.distributed.run): DP-SGD
of the 2-layer MLP with a compressed gradient bucket (bf16 wire, error
feedback) on a bf16 engine, ipc data plane, every rank on the box's one GPU.
First eager steps, every round's fp32 gradients, wire input and output
recorded; then the same bucket through the whole-step capture (pack, round
and mixed update in one HIP graph).  Writes rank<i>.pt."""
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
    from akka_allreduce_amd.models.mlp import MLP, GraphedDPStep, dp_sgd_step, synthetic_batch
    from akka_allreduce_amd.parallel import ThresholdAllreduce
    from akka_allreduce_amd.parallel.dp import GradientBucket

    lr = 0.1
    torch.manual_seed(0)  # identical init on every rank
    model = MLP(256, 512, 10).to(dev)
    bucket = GradientBucket(list(model.parameters()), flatten_params=True, wire_dtype=torch.bfloat16)
    ar = ThresholdAllreduce(bucket.numel, max_chunk_size=1 << 14, dtype=torch.bfloat16, device=dev, data_plane="ipc")
    ar.use_lane("ipc_fused_lite")
    rec = []

    def recording_ar(t):
        grads, xin = bucket.flat.detach().clone(), t.detach().clone()  # the pack leaves flat as it was
        o = ar(t)
        rec.append((grads, xin, o.data.detach().clone()))
        return o

    def batch(s):
        g = torch.Generator(device=dev).manual_seed(100 * s + rank)
        return synthetic_batch(64, 256, 10, device=dev, generator=g)

    for s in range(a.steps):
        dp_sgd_step(model, *batch(s), lr, recording_ar, bucket, sync_loss=False)
    torch.cuda.synchronize()
    eager = bucket.pflat.detach().clone()
    residual = bucket.residual.detach().clone()

    cap = ar.capturable()
    gs = GraphedDPStep(model, bucket, *batch(a.steps), allreduce=cap, lr=lr)
    after_capture = (torch.equal(bucket.pflat, eager), torch.equal(bucket.residual, residual))
    sx, sy = gs.static_inputs()
    for s in range(a.steps, 2 * a.steps):
        x, y = batch(s)
        sx.copy_(x)
        sy.copy_(y)
        gs(sx, sy, lr, None)
    torch.cuda.synchronize()
    cap.close()
    torch.save({"eager": eager.cpu(), "graphed": bucket.pflat.detach().cpu(), "replays": gs.replays,
                "after_capture": after_capture, "ipc_error": ar.ipc_error(),
                "grads": [r[0].cpu() for r in rec], "wire_in": [r[1].cpu() for r in rec],
                "wire_out": [r[2].cpu() for r in rec]}, os.path.join(a.out_dir, f"rank{rank}.pt"))
    ar.retire()
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
