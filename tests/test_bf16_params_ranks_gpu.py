"""Two ranks with bf16 parameters: exact rounds of a bf16 engine over the ipc
data plane, three FusedAdamW steps from different per-rank gradients.  Both
ranks hold the same ``pflat``, ``m`` and ``v`` bit for bit -- the rounding bits
of ``p`` too are a function of the index, the step and the shared seed."""
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


def test_both_ranks_hold_the_same_bf16_model():
    n, steps = 2, 3
    with tempfile.TemporaryDirectory() as out:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
               "--master-addr", "127.0.0.1", "--master-port", str(_port()),
               os.path.join(ROOT, "tests", "bf16_params_ranks.py"), "--out-dir", out, "--steps", str(steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=180, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        rows = [torch.load(os.path.join(out, f"rank{i}.pt"), weights_only=True) for i in range(n)]
    for d in rows:
        assert d["t"] == steps and d["ipc_error"] == 0
        for k in ("p", "m", "v"):
            assert d[k].dtype == torch.bfloat16 and bool(torch.isfinite(d[k].float()).all()), k
        assert not torch.equal(d["p"], d["p0"]) and float(d["v"].float().max()) > 0
    for s in range(steps):
        assert not torch.equal(rows[0]["mine"][s], rows[1]["mine"][s])  # the ranks' gradients differ
        assert torch.equal(rows[0]["sums"][s].view(torch.int16), rows[1]["sums"][s].view(torch.int16))
    for k in ("p0", "p", "m", "v"):
        assert torch.equal(rows[0][k].view(torch.int16), rows[1][k].view(torch.int16)), k
