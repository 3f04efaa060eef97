"""Rank program for tests/test_param_groups_graph_gpu.py: the MLP's DP step with
a fused AdamW update whose biases are in a no-decay group (global-norm clip
on), the WHOLE step -- forward, backward, the one-sided allreduce, the norm
pass and the grouped optimizer pass -- captured in one HIP graph and called
with a different learning rate every step (a linear warm-up from 0: the rows
in device memory are rewritten before each replay), against the eager steps
with the same learning rates on the same batches (every rank on the box's one
GPU).  An ungrouped optimizer captured the same way still refuses another
learning rate.  Writes rank<i>.pt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


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

    cdt, peak = torch.bfloat16, 1e-2
    lrs = [peak * s / (a.steps - 1) for s in range(a.steps)]  # 0, ..., peak

    def batches():
        for s in range(a.steps):
            g = torch.Generator(device=dev).manual_seed(1000 * s + rank)
            yield synthetic_batch(32, 64, 10, device=dev, generator=g)

    def fresh(grouped=True):
        torch.manual_seed(0)
        m = MLP(64, 128, 10).to(dev)
        b = GradientBucket(list(m.parameters()), flatten_params=True)
        pg = [{"params": [m.fc1.bias, m.fc2.bias], "weight_decay": 0.0}] if grouped else None
        return m, b, FusedAdamW(b, weight_decay=0.01, max_grad_norm=1.0, param_groups=pg)

    m1, b1, o1 = fresh()
    ar = OneSidedAllreduce(b1.numel, max_chunk_size=1 << 12, device=dev)
    eager_losses = [dp_sgd_step(m1, x, y, lr, ar, b1, sync_loss=False, compute_dtype=cdt, optimizer=o1)
                    for (x, y), lr in zip(batches(), lrs)]

    m2, b2, o2 = fresh()
    x0, y0 = next(batches())
    gs = GraphedDPStep(m2, b2, x0, y0, compute_dtype=cdt, allreduce=ar, lr=peak, optimizer=o2)
    t_after_capture = int(o2.t)  # the warmup's steps were put back
    state_clean = bool((o2.m == 0).all() and (o2.v == 0).all())
    lr_after_capture = o2.lr
    sx, sy = gs.static_inputs()
    graph_losses = []
    for (x, y), lr in zip(batches(), lrs):
        sx.copy_(x)
        sy.copy_(y)
        graph_losses.append(gs(sx, sy, lr, None).clone())
    torch.cuda.synchronize()

    # an ungrouped optimizer has its learning rate baked into the capture
    m3, b3, o3 = fresh(grouped=False)
    gs3 = GraphedDPStep(m3, b3, x0, y0, compute_dtype=cdt, allreduce=ar, lr=peak, optimizer=o3)
    try:
        gs3(sx, sy, 0.5 * peak, None)
        refused = False
    except RuntimeError as e:
        refused = "captured with lr" in str(e)
    torch.cuda.synchronize()

    torch.save({"eager": b1.pflat.cpu(), "graphed": b2.pflat.cpu(), "eager_m": o1.m.cpu(), "graphed_m": o2.m.cpu(),
                "eager_v": o1.v.cpu(), "graphed_v": o2.v.cpu(), "eager_shadow": b1.sflat.cpu(),
                "graphed_shadow": b2.sflat.cpu(), "eager_losses": torch.stack(eager_losses).cpu(),
                "graph_losses": torch.stack(graph_losses).cpu(), "replays": gs.replays, "t_eager": int(o1.t),
                "t_graphed": int(o2.t), "t_after_capture": t_after_capture, "state_clean": state_clean,
                "lr_after_capture": lr_after_capture, "lr_last": o2.lr, "step_lr": gs.lr,
                "segments": len(o2.groups.host_seg_end), "ungrouped_refused": refused,
                "ungrouped_replays": gs3.replays, "error": ar.error()}, os.path.join(a.out_dir, f"rank{rank}.pt"))
    ar.retire()
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
