"""The whole DP step with a grouped fused AdamW update in one HIP graph, on 2
processes sharing the card, called with a different learning rate every step:
the update reads its learning rate (and each group's weight decay) from device
memory when the replay runs, so a captured step follows a schedule.
Parameters, optimizer state, shadow and losses bitwise equal the eager steps'
with the same learning rates on the same batches."""
import os
import socket
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_fully_graphed_grouped_adamw_step_follows_a_schedule():
    n, steps = 2, 6
    with tempfile.TemporaryDirectory() as out:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
               "--master-addr", "127.0.0.1", "--master-port", str(_port()),
               os.path.join(ROOT, "tests", "param_groups_ranks.py"), "--out-dir", out, "--steps", str(steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        rows = [torch.load(os.path.join(out, f"rank{i}.pt"), weights_only=True) for i in range(n)]
    for d in rows:
        assert d["replays"] == steps and d["error"] == 0
        assert d["t_after_capture"] == 0 and d["state_clean"] and d["lr_after_capture"] == 1e-2
        assert d["t_eager"] == steps and d["t_graphed"] == steps
        last = 1e-2 * (steps - 1) / (steps - 1)  # the warm-up's last learning rate, as the rank program spells it
        assert d["segments"] == 4 and d["lr_last"] == last and d["step_lr"] == last
        for k in ("", "_m", "_v", "_shadow"):
            assert torch.equal(d["eager" + k], d["graphed" + k]), k
        assert torch.equal(d["eager_losses"], d["graph_losses"])
        assert float(d["eager_m"].abs().max()) > 0 and float(d["eager_v"].abs().max()) > 0
        assert bool(torch.isfinite(d["graphed"]).all())  # the first step's lr is 0
        assert d["ungrouped_refused"] and d["ungrouped_replays"] == 0
    assert torch.equal(rows[0]["graphed"], rows[1]["graphed"])  # every rank holds the same model
