"""Rank program for tests/test_fused_optim_graph_gpu.py: the MLP's DP step with
a fused AdamW update (global-norm clip on), the WHOLE step -- forward,
backward, the one-sided allreduce, the norm pass and the optimizer pass --
captured in one HIP graph, against the eager step on the same batches (every
rank on the box's one GPU).  Writes rank<i>.pt."""
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

    cdt, lr = torch.bfloat16, 1e-2

    def batches():
        for s in range(a.steps):
            g = torch.Generator(device=dev).manual_seed(1000 * s + rank)
            yield synthetic_batch(32, 64, 10, device=dev, generator=g)

    def fresh():
        torch.manual_seed(0)
        m = MLP(64, 128, 10).to(dev)
        b = GradientBucket(list(m.parameters()), flatten_params=True)
        return m, b, FusedAdamW(b, weight_decay=0.01, max_grad_norm=1.0)

    m1, b1, o1 = fresh()
    ar = OneSidedAllreduce(b1.numel, max_chunk_size=1 << 12, device=dev)
    eager_losses = [dp_sgd_step(m1, x, y, lr, ar, b1, sync_loss=False, compute_dtype=cdt, optimizer=o1)
                    for x, y in batches()]

    m2, b2, o2 = fresh()
    x0, y0 = next(batches())
    gs = GraphedDPStep(m2, b2, x0, y0, compute_dtype=cdt, allreduce=ar, lr=lr, optimizer=o2)
    t_after_capture = int(o2.t)  # the warmup's steps were put back
    state_clean = bool((o2.m == 0).all() and (o2.v == 0).all())
    sx, sy = gs.static_inputs()
    graph_losses = []
    for x, y in batches():
        sx.copy_(x)
        sy.copy_(y)
        graph_losses.append(gs(sx, sy, lr, None).clone())
    torch.cuda.synchronize()
    torch.save({"eager": b1.pflat.cpu(), "graphed": b2.pflat.cpu(), "eager_m": o1.m.cpu(), "graphed_m": o2.m.cpu(),
                "eager_v": o1.v.cpu(), "graphed_v": o2.v.cpu(), "eager_shadow": b1.sflat.cpu(),
                "graphed_shadow": b2.sflat.cpu(), "eager_losses": torch.stack(eager_losses).cpu(),
                "graph_losses": torch.stack(graph_losses).cpu(), "replays": gs.replays, "t_eager": int(o1.t),
                "t_graphed": int(o2.t), "t_after_capture": t_after_capture, "state_clean": state_clean,
                "error": ar.error()}, os.path.join(a.out_dir, f"rank{rank}.pt"))
    ar.retire()
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
