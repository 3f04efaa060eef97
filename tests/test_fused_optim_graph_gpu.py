"""The whole DP step with a fused AdamW update in one HIP graph: forward,
backward, the one-sided allreduce, the norm pass and the optimizer pass
replayed as one graph on 2 processes sharing the card.  The step counter is on
the device, so each replay is one more step: parameters, optimizer state,
shadow and losses bitwise equal the eager steps' on the same batches."""
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


def test_fully_graphed_adamw_step_matches_eager():
    n, steps = 2, 6
    with tempfile.TemporaryDirectory() as out:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
               "--master-addr", "127.0.0.1", "--master-port", str(_port()),
               os.path.join(ROOT, "tests", "fused_optim_ranks.py"), "--out-dir", out, "--steps", str(steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        rows = [torch.load(os.path.join(out, f"rank{i}.pt"), weights_only=True) for i in range(n)]
    for d in rows:
        assert d["replays"] == steps and d["error"] == 0
        assert d["t_after_capture"] == 0 and d["state_clean"]
        assert d["t_eager"] == steps and d["t_graphed"] == steps
        for k in ("", "_m", "_v", "_shadow"):
            assert torch.equal(d["eager" + k], d["graphed" + k]), k
        assert torch.equal(d["eager_losses"], d["graph_losses"])
        assert float(d["eager_m"].abs().max()) > 0 and float(d["eager_v"].abs().max()) > 0
    assert torch.equal(rows[0]["graphed"], rows[1]["graphed"])  # every rank holds the same model
